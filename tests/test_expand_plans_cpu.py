"""State pools and mev_expand_plans without a device: the header declares mev_pool, the pool entry
points and mev_expand_args in the stated field order, the addition is additive (ABI version 3,
mev_evaluate_args and mev_leaf_args as they were), the ctypes struct is the header's, the library
exports the symbols, and null arguments are refused before any device is touched."""
import ctypes
import os
import re

import test_evaluate_plans_cpu as EP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ["eval", "leaf_obs", "src", "dst", "dst_slots", "counter_offset"]
TYPES = [r"mev_evaluate_args\s", r"float\s*\*", r"const\s+mev_pool\s*\*", r"mev_pool\s*\*", r"const\s+int32_t\s*\*",
         r"uint64_t\s"]
POOL_CALLS = {
    "mev_pool_create": r"mev_handle\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*mev_pool\s*\*\*\s*\w+",
    "mev_pool_destroy": r"mev_pool\s*\*\s*\w+",
    "mev_pool_slots": r"const\s+mev_pool\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+",
    "mev_pool_capture": r"mev_handle\s*\*\s*\w+\s*,\s*mev_pool\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,\s*"
                        r"const\s+int32_t\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*uint32_t\s+\w+",
    "mev_pool_get_state": r"mev_pool\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*"
                          r"const\s+mev_state\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*,\s*"
                          r"uint8_t\s*\*\s*\w+",
    "mev_expand_plans": r"mev_handle\s*\*\s*\w+\s*,\s*const\s+mev_expand_args\s*\*\s*\w+",
}


def _header_code():
    src = open(os.path.join(ROOT, "include", "marlenv.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_pool_and_the_entry_points():
    code = _header_code()
    assert re.search(r"typedef\s+struct\s+mev_pool\s+mev_pool\s*;", code)
    assert re.search(r"#define\s+MEV_MAX_POOL_SLOTS\s+\(\s*1\s*<<\s*20\s*\)", code)
    for name, params in POOL_CALLS.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + params + r"\s*\)\s*;", code), name
    # each after what it uses
    assert code.index("mev_pool;") < code.index("mev_pool_create") < code.index("mev_expand_args;")
    assert code.index("mev_leaf_args;") < code.index("mev_expand_args;") < code.index("mev_expand_plans")
    assert code.index("} mev_state;") < code.index("mev_pool_get_state")


def test_header_struct_field_order():
    code = _header_code()
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*mev_expand_args\s*;", code, flags=re.S)
    assert m, "mev_expand_args is not declared"
    decls = [d.strip() for d in m.group(1).split(";") if d.strip()]
    assert re.findall(r"(\w+)\s*;", m.group(1)) == FIELDS and len(decls) == len(FIELDS)
    for d, name, ty in zip(decls, FIELDS, TYPES):
        assert re.fullmatch(ty + r"\s*" + name, d), d


def test_the_addition_is_additive():
    code = _header_code()
    assert re.search(r"#define\s+MEV_ABI_VERSION\s+3\b", code)
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*mev_evaluate_args\s*;", code, flags=re.S)
    assert m and re.findall(r"(\w+)\s*;", m.group(1)) == EP.FIELDS
    decls = [d.strip() for d in m.group(1).split(";") if d.strip()]
    for d, name, ty in zip(decls, EP.FIELDS, EP.TYPES):
        assert re.fullmatch(ty + r"\s*" + name, d), d
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*mev_leaf_args\s*;", code, flags=re.S)
    decls = [d.strip() for d in m.group(1).split(";") if d.strip()]
    assert len(decls) == 2 and re.fullmatch(r"mev_evaluate_args\s+eval", decls[0])
    assert re.fullmatch(r"float\s*\*\s*leaf_obs", decls[1])


def test_ctypes_struct_is_the_headers(mev):
    a = mev._capi.MevExpandArgs
    assert [f[0] for f in a._fields_] == FIELDS
    assert a._fields_[0][1] is mev._capi.MevEvaluateArgs
    assert ctypes.sizeof(ctypes.c_void_p) == 8
    # LP64: the 120-byte evaluation struct, four pointers, a uint64
    want = dict(eval=0, leaf_obs=120, src=128, dst=136, dst_slots=144, counter_offset=152)
    assert {k: getattr(a, k).offset for k in FIELDS} == want
    assert ctypes.sizeof(a) == 160
    assert a._fields_[5][1] is ctypes.c_uint64
    assert ctypes.sizeof(mev._capi.MevEvaluateArgs) == 120 and ctypes.sizeof(mev._capi.MevLeafArgs) == 128
    assert mev._capi.MevLeafArgs.leaf_obs.offset == 120


def test_library_exports_the_symbols(mev):
    lib = mev.load_library()
    for name in POOL_CALLS:
        assert hasattr(lib, name), name
        assert name in mev._capi.EXPORTED, name
    assert lib.mev_abi_version() == 3
    assert mev._capi.MEV_MAX_POOL_SLOTS == 1 << 20


def test_null_arguments_are_refused_without_a_device(mev):
    lib = mev.load_library()
    lib.mev_last_error.restype = ctypes.c_char_p
    # (arguments are checked before the handle is looked at, so any address serves as one)
    dummy = (ctypes.c_uint8 * 64)()
    hd = ctypes.addressof(dummy)
    args = mev._capi.MevExpandArgs()
    args.eval.candidates, args.eval.length = 2, 2
    assert lib.mev_expand_plans(None, ctypes.byref(args)) == -1
    assert b"null" in lib.mev_last_error()
    assert lib.mev_expand_plans(hd, None) == -1
    assert b"null" in lib.mev_last_error()
    buf = (ctypes.c_int32 * 16)()
    args.eval.actions = args.eval.roots = ctypes.addressof(buf)
    assert args.dst is None and args.dst_slots is None
    assert lib.mev_expand_plans(hd, ctypes.byref(args)) == -1  # a null dst
    assert b"dst" in lib.mev_last_error()
    args.dst = hd
    assert lib.mev_expand_plans(hd, ctypes.byref(args)) == -1  # a null dst_slots
    assert b"dst_slots" in lib.mev_last_error()
    out = ctypes.c_void_p(1)
    assert lib.mev_pool_create(None, 4, ctypes.byref(out)) == -1
    assert b"null" in lib.mev_last_error()
    assert lib.mev_pool_create(hd, 4, None) == -1
    assert lib.mev_pool_create(hd, 0, ctypes.byref(out)) == -1  # (the slot count before the handle, too)
    assert b"slots" in lib.mev_last_error() and out.value is None
    assert lib.mev_pool_create(hd, (1 << 20) + 1, ctypes.byref(out)) == -1
    n = ctypes.c_int32(7)
    assert lib.mev_pool_slots(None, ctypes.byref(n)) == -1 and n.value == 7
    assert lib.mev_pool_capture(None, None, None, None, 1, 0) == -1
    assert lib.mev_pool_capture(hd, None, ctypes.addressof(buf), ctypes.addressof(buf), 1, 0) == -1
    assert lib.mev_pool_get_state(None, ctypes.addressof(buf), 1, None, None, None, None) == -1
    assert lib.mev_pool_destroy(None) == 0  # (as mev_destroy(NULL))
