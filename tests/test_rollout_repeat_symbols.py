"""mev_rollout_policy_repeat at the boundary, without a GPU: the header declares the call, its argument struct and
the sub-step cap; the ABI version is unchanged; the library exports the symbol; the ctypes struct lays value_seq
where mev_rollout_values_args has it, followed by repeat and substeps_seq; ROLLOUT_OUTPUTS keeps its 8 names."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "marlenv.h")).read()


def test_header_declares_the_call():
    src = header()
    assert re.search(r"#define\s+MEV_MAX_ROLLOUT_SUBSTEPS\s+4096\b", src)
    assert re.search(r"#define\s+MEV_ABI_VERSION\s+3\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+mev_rollout_policy_repeat\s*\(\s*mev_handle\s*\*\s*h\s*,\s*const\s+mev_rollout_repeat_args\s*\*\s*args\s*\)\s*;",
                     code)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*mev_rollout_repeat_args\s*;", code)
    assert m, "mev_rollout_repeat_args"
    fields = [re.sub(r"\s+", " ", f).strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == ["mev_rollout_args rollout", "float* value_seq", "int32_t repeat", "int32_t* substeps_seq"], fields


def test_library_exports_the_symbol(mev):
    lib = mev.load_library()
    assert hasattr(lib, "mev_rollout_policy_repeat")
    assert "mev_rollout_policy_repeat" in mev._capi.EXPORTED
    assert lib.mev_abi_version() == 3
    assert lib.mev_rollout_policy_repeat(None, None) != 0  # (null arguments: refused before any device call)


def test_ctypes_struct_layout(mev):
    cap = mev._capi
    R = cap.MevRolloutRepeatArgs
    assert [f[0] for f in R._fields_] == ["rollout", "value_seq", "repeat", "substeps_seq"]
    assert R.rollout.offset == 0 and R.rollout.size == ctypes.sizeof(cap.MevRolloutArgs)
    assert R.value_seq.offset == ctypes.sizeof(cap.MevRolloutArgs) == cap.MevRolloutValuesArgs.value_seq.offset
    assert R.repeat.offset == R.value_seq.offset + ctypes.sizeof(ctypes.c_void_p) and R.repeat.size == 4
    assert R.substeps_seq.offset == R.repeat.offset + 8  # (the pointer's alignment)
    assert ctypes.sizeof(R) == R.substeps_seq.offset + ctypes.sizeof(ctypes.c_void_p)
    assert cap.MEV_MAX_ROLLOUT_SUBSTEPS == 4096


def test_rollout_outputs_keep_their_names(mev):
    cap = mev._capi
    assert len(cap.ROLLOUT_OUTPUTS) == 8 and "substeps_seq" not in cap.ROLLOUT_OUTPUTS
    assert cap.ROLLOUT_OUTPUTS == ("obs_seq", "actions_seq", "mean_seq", "reward_seq", "done_seq", "status_seq",
                                   "terminated_seq", "truncated_seq")
