"""mev_step_repeat without a device: the header declares it, the library exports it and refuses
null arguments, and the reference loop the GPU tests compare against (tests/window_ref.py) is,
at repeat = 1, the reference's step as its goldens recorded it."""
import ctypes
import os
import re

import numpy as np
import pytest

import golden_replay as G
import oracle_replay as R
import window_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_step_repeat():
    src = open(os.path.join(ROOT, "include", "marlenv.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+mev_step_repeat\s*\(\s*mev_handle\s*\*\s*\w+\s*,\s*const\s+mev_repeat_args\s*\*", code)
    assert re.search(r"#define\s+MEV_MAX_REPEAT\s+64\b", code)
    assert re.search(r"mev_step_args\s+step\s*;.*int32_t\s+repeat\s*;.*int32_t\s*\*\s*substeps\s*;", code, flags=re.S)
    assert re.search(r"#define\s+MEV_ABI_VERSION\s+3\b", code)  # additive: the ABI version stays


def test_library_exports_step_repeat(mev):
    lib = mev.load_library()
    assert hasattr(lib, "mev_step_repeat")
    assert "mev_step_repeat" in mev._capi.EXPORTED and mev._capi.MEV_MAX_REPEAT == 64
    # the ctypes struct is the header's: mev_step_args, then repeat, then the substeps pointer
    a = mev._capi.MevRepeatArgs
    assert [f[0] for f in a._fields_] == ["step", "repeat", "substeps"]
    assert a.repeat.offset == ctypes.sizeof(mev._capi.MevStepArgs)


def test_null_arguments_are_refused_without_a_device(mev):
    lib = mev.load_library()
    args = mev._capi.MevRepeatArgs()
    args.repeat = 2
    assert lib.mev_step_repeat(None, ctypes.byref(args)) == -1
    assert b"null" in lib.mev_last_error()
    assert lib.mev_step_repeat(None, None) == -1
    assert b"null" in lib.mev_last_error()


@pytest.mark.parametrize("name", G.scenario_names("cfg3_team_"))
def test_reference_loop_at_repeat_one_is_the_recorded_step(name):
    d = G.load(name)
    meta = d["meta"]
    L = int(meta["num_lanes"])
    o = R.make_oracle(meta)
    cids = G.custom_route_ids(o, d)
    egos = R.state_from_records(d["init_ego_f"], d["init_ego_i"], G.ego_route_ids(o, d, L, cids))
    o.set_state(egos, [], int(meta.get("init_step", 0)))
    for t in range(int(meta["steps"])):
        w = RR.window_step(o, *RR.held(d["actions"][t], float(meta["dt"]), 1))
        assert w["substeps"] == 1
        assert G.bits_equal(w["rew"], d["rew"][t]), f"step {t + 1}: reward"
        assert G.bits_equal(w["obs"][:, :127], d["obs"][t]), f"step {t + 1}: obs"
        assert G.bits_equal(w["status"], d["status"][t]) and G.bits_equal(w["done"], d["done"][t]), f"step {t + 1}"
        assert [w["terminated"], w["truncated"], w["agents_alive"], w["step"]] == [int(x) for x in d["flags"][t]]
    o.close()
