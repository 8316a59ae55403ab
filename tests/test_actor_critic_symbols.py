"""The actor-critic calls' C boundary: the cross-compiled library exports mev_policy_set_value_head,
mev_policy_has_value_head, mev_rollout_policy_values and mev_gae, include/marlenv.h declares them with
MEV_GAE_MASK_RESET_STEPS, and the ABI version stays 3 (no compute calls: this runs without a device)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mev_policy_set_value_head", "mev_policy_has_value_head", "mev_rollout_policy_values", "mev_gae")


def test_header_declares_the_actor_critic_calls():
    src = open(os.path.join(ROOT, "include", "marlenv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), n
    assert re.search(r"#define\s+MEV_GAE_MASK_RESET_STEPS\s+0x100u\b", src)
    assert re.search(r"#define\s+MEV_ABI_VERSION\s+3\b", src)
    assert "mev_rollout_values_args" in src and "mev_gae_args" in src
    assert os.path.exists(os.path.join(ROOT, "marl-traffic-intersection_amd", "csrc", "mev_gae.h"))


def test_library_exports_the_actor_critic_calls(mev):
    lib = mev.load_library()
    missing = [n for n in NAMES if not hasattr(lib, n)]
    assert not missing, missing
    cap = mev._capi
    assert set(NAMES) <= set(cap.EXPORTED)
    assert cap.MEV_GAE_MASK_RESET_STEPS == 0x100
    assert "value_seq" not in cap.ROLLOUT_OUTPUTS and len(cap.ROLLOUT_OUTPUTS) == 8
    assert callable(cap.Handle.gae) and callable(cap.Policy.set_value_head)
    # the wrapper structs are the header's: mev_rollout_args unchanged, value_seq behind it; mev_gae_args' fields
    assert cap.MevRolloutValuesArgs.value_seq.offset == ctypes.sizeof(cap.MevRolloutArgs)
    assert [f[0] for f in cap.MevGaeArgs._fields_] == [
        "reward_seq", "value_seq", "done_seq", "terminated_seq", "truncated_seq", "ended_before", "length", "gamma",
        "lam", "advantages", "returns", "valid", "flags"]
