"""mev_rollout_policies at the boundary, without a GPU: the header declares the call, its argument struct and the
policy cap; the ABI version is unchanged; the library exports the symbol and refuses null arguments; the ctypes
struct lays mev_rollout_repeat_args first, then the table, its count, assign and sigma at their natural alignments;
ROLLOUT_OUTPUTS keeps its 8 names."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "marlenv.h")).read()


def test_header_declares_the_call():
    src = header()
    assert re.search(r"#define\s+MEV_MAX_ROLLOUT_POLICIES\s+8\b", src)
    assert re.search(r"#define\s+MEV_ABI_VERSION\s+3\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+mev_rollout_policies\s*\(\s*mev_handle\s*\*\s*h\s*,\s*const\s+mev_rollout_multi_args\s*\*\s*args\s*\)\s*;",
                     code)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*mev_rollout_multi_args\s*;", code)
    assert m, "mev_rollout_multi_args"
    fields = [re.sub(r"\s+", " ", f).strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == ["mev_rollout_repeat_args base", "const mev_policy* const* policies", "int32_t count",
                      "const uint8_t* assign", "const float* sigma"], fields


def test_library_exports_the_symbol(mev):
    lib = mev.load_library()
    assert hasattr(lib, "mev_rollout_policies")
    assert "mev_rollout_policies" in mev._capi.EXPORTED
    assert lib.mev_abi_version() == 3
    assert lib.mev_rollout_policies(None, None) != 0  # (null arguments: refused before any device call)


def test_ctypes_struct_layout(mev):
    cap = mev._capi
    M, ptr = cap.MevRolloutMultiArgs, ctypes.sizeof(ctypes.c_void_p)
    assert [f[0] for f in M._fields_] == ["base", "policies", "count", "assign", "sigma"]
    assert M.base.offset == 0 and M.base.size == ctypes.sizeof(cap.MevRolloutRepeatArgs)
    assert M.policies.offset == ctypes.sizeof(cap.MevRolloutRepeatArgs) and M.policies.size == ptr
    assert M.count.offset == M.policies.offset + ptr and M.count.size == 4
    assert M.assign.offset == M.count.offset + 8 and M.assign.size == ptr  # (the pointer's alignment)
    assert M.sigma.offset == M.assign.offset + ptr and M.sigma.size == ptr
    assert ctypes.sizeof(M) == M.sigma.offset + ptr
    assert cap.MEV_MAX_ROLLOUT_POLICIES == 8


def test_rollout_outputs_keep_their_names(mev):
    cap = mev._capi
    assert cap.ROLLOUT_OUTPUTS == ("obs_seq", "actions_seq", "mean_seq", "reward_seq", "done_seq", "status_seq",
                                   "terminated_seq", "truncated_seq")
