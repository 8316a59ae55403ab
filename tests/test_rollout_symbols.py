"""The closed-loop rollout's C boundary: the cross-compiled library exports mev_policy_create,
mev_policy_update, mev_policy_destroy, mev_rollout_policy and mev_get_rollout_row, and include/marlenv.h
declares them (no compute calls: this runs without a device)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mev_policy_create", "mev_policy_update", "mev_policy_destroy", "mev_rollout_policy", "mev_get_rollout_row")


def test_header_declares_the_rollout_calls():
    src = open(os.path.join(ROOT, "include", "marlenv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), n
    for macro in ("MEV_POLICY_MAX_WIDTH 128", "MEV_MAX_ROLLOUT 1024"):
        assert re.search(r"#define\s+" + macro.replace(" ", r"\s+") + r"\b", src), macro
    assert "mev_policy_spec" in src and "mev_rollout_args" in src


def test_library_exports_the_rollout_calls(mev):
    lib = mev.load_library()
    missing = [n for n in NAMES if not hasattr(lib, n)]
    assert not missing, missing
    assert set(NAMES) <= set(mev._capi.EXPORTED)
    cap = mev._capi
    assert cap.MEV_POLICY_MAX_WIDTH == 128 and cap.MEV_MAX_ROLLOUT == 1024
    assert callable(cap.Handle.policy) and callable(cap.Handle.rollout_policy)
