"""mev_evaluate_leaves without a device: the header declares mev_leaf_args (eval, leaf_obs) and the
function's signature, the addition is additive (ABI version 3, mev_evaluate_args as it was), the
ctypes struct is the header's, the library exports the symbol, and null arguments -- a null
leaf_obs among them -- are refused before any device is touched."""
import ctypes
import os
import re

import test_evaluate_plans_cpu as EP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_code():
    src = open(os.path.join(ROOT, "include", "marlenv.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_struct():
    code = _header_code()
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*mev_leaf_args\s*;", code, flags=re.S)
    assert m, "mev_leaf_args is not declared"
    decls = [d.strip() for d in m.group(1).split(";") if d.strip()]
    assert len(decls) == 2
    assert re.fullmatch(r"mev_evaluate_args\s+eval", decls[0]), decls[0]
    assert re.fullmatch(r"float\s*\*\s*leaf_obs", decls[1]), decls[1]


def test_header_declares_the_entry_point():
    code = _header_code()
    assert re.search(r"\bint\s+mev_evaluate_leaves\s*\(\s*mev_handle\s*\*\s*\w+\s*,\s*const\s+mev_leaf_args\s*\*\s*\w+\s*\)",
                     code)
    # declared after the struct it embeds
    assert code.index("mev_evaluate_args;") < code.index("mev_leaf_args;")
    # additive: the ABI version stays, and the struct it embeds is as it was
    assert re.search(r"#define\s+MEV_ABI_VERSION\s+3\b", code)
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*mev_evaluate_args\s*;", code, flags=re.S)
    assert m and re.findall(r"(\w+)\s*;", m.group(1)) == EP.FIELDS
    decls = [d.strip() for d in m.group(1).split(";") if d.strip()]
    for d, name, ty in zip(decls, EP.FIELDS, EP.TYPES):
        assert re.fullmatch(ty + r"\s*" + name, d), d


def test_ctypes_struct_is_the_headers(mev):
    a = mev._capi.MevLeafArgs
    assert [f[0] for f in a._fields_] == ["eval", "leaf_obs"]
    assert a._fields_[0][1] is mev._capi.MevEvaluateArgs
    assert a.eval.offset == 0 and a.leaf_obs.offset == 120
    assert ctypes.sizeof(a) == 128
    assert ctypes.sizeof(mev._capi.MevEvaluateArgs) == 120  # (pinned by the scoring call's own test too)


def test_library_exports_the_symbol(mev):
    lib = mev.load_library()
    assert hasattr(lib, "mev_evaluate_leaves")
    assert "mev_evaluate_leaves" in mev._capi.EXPORTED
    assert lib.mev_abi_version() == 3


def test_null_arguments_are_refused_without_a_device(mev):
    lib = mev.load_library()
    lib.mev_last_error.restype = ctypes.c_char_p
    args = mev._capi.MevLeafArgs()
    args.eval.candidates, args.eval.length = 2, 2
    assert lib.mev_evaluate_leaves(None, ctypes.byref(args)) == -1
    assert b"null" in lib.mev_last_error()
    # (handle, NULL) and a null leaf_obs: checked before the handle is looked at, so any address serves
    dummy = (ctypes.c_uint8 * 64)()
    assert lib.mev_evaluate_leaves(ctypes.addressof(dummy), None) == -1
    assert b"null" in lib.mev_last_error()
    buf = (ctypes.c_float * 16)()
    args.eval.actions = args.eval.roots = ctypes.addressof(buf)
    assert args.leaf_obs is None
    assert lib.mev_evaluate_leaves(ctypes.addressof(dummy), ctypes.byref(args)) == -1
    assert b"leaf_obs" in lib.mev_last_error()
