"""mev_evaluate_plans without a device: the header declares the struct in its stated field order and
the function's signature, the ABI version stays 3, the library exports the symbol, the ctypes
struct is the header's, and null arguments are refused."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = ["actions", "roots", "spawn_route", "candidates", "length", "dt", "dt_seq", "gamma", "returns", "reward_seq",
          "done_seq", "status_seq", "substeps", "terminated", "truncated", "flags"]
# the header's declaration of each field, as a pattern
TYPES = [r"const\s+float\s*\*", r"const\s+int32_t\s*\*", r"const\s+int32_t\s*\*", r"int32_t\s", r"int32_t\s", r"float\s",
         r"const\s+float\s*\*", r"float\s", r"float\s*\*", r"float\s*\*", r"uint8_t\s*\*", r"uint8_t\s*\*", r"int32_t\s*\*",
         r"uint8_t\s*\*", r"uint8_t\s*\*", r"uint32_t\s"]


def _header_code():
    src = open(os.path.join(ROOT, "include", "marlenv.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_entry_point():
    code = _header_code()
    assert re.search(r"\bint\s+mev_evaluate_plans\s*\(\s*mev_handle\s*\*\s*\w+\s*,\s*const\s+mev_evaluate_args\s*\*\s*\w+\s*\)",
                     code)
    assert re.search(r"#define\s+MEV_ABI_VERSION\s+3\b", code)  # additive: the ABI version stays
    assert re.search(r"#define\s+MEV_MAX_CANDIDATES\s+\(\s*1\s*<<\s*20\s*\)", code)
    assert re.search(r"#define\s+MEV_MAX_REPEAT\s+64\b", code)


def test_header_struct_field_order():
    code = _header_code()
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*mev_evaluate_args\s*;", code, flags=re.S)
    assert m, "mev_evaluate_args is not declared"
    body = m.group(1)
    assert re.findall(r"(\w+)\s*;", body) == FIELDS
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert len(decls) == len(FIELDS)
    for d, name, ty in zip(decls, FIELDS, TYPES):
        assert re.fullmatch(ty + r"\s*" + name, d), d
    # the neighbouring structs are untouched
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*mev_sequence_args\s*;", code, flags=re.S)
    assert re.findall(r"(\w+)\s*;", m.group(1)) == ["step", "length", "dt_seq", "reward_seq", "done_seq", "status_seq",
                                                     "substeps"]


def test_library_exports_the_symbol(mev):
    lib = mev.load_library()
    assert hasattr(lib, "mev_evaluate_plans")
    assert "mev_evaluate_plans" in mev._capi.EXPORTED
    assert lib.mev_abi_version() == 3
    assert mev._capi.MEV_MAX_CANDIDATES == 1 << 20


def test_ctypes_struct_is_the_headers(mev):
    a = mev._capi.MevEvaluateArgs
    assert [f[0] for f in a._fields_] == FIELDS
    p = ctypes.sizeof(ctypes.c_void_p)
    assert p == 8
    # the C layout of the header's struct on an LP64 target: three pointers, two int32, a float, padding to the
    # next pointer, a float, padding, seven pointers, a uint32 and the tail padding
    want = dict(actions=0, roots=8, spawn_route=16, candidates=24, length=28, dt=32, dt_seq=40, gamma=48, returns=56,
                reward_seq=64, done_seq=72, status_seq=80, substeps=88, terminated=96, truncated=104, flags=112)
    assert {k: getattr(a, k).offset for k in FIELDS} == want
    assert ctypes.sizeof(a) == 120


def test_null_arguments_are_refused_without_a_device(mev):
    lib = mev.load_library()
    args = mev._capi.MevEvaluateArgs()
    args.candidates, args.length = 2, 2
    assert lib.mev_evaluate_plans(None, ctypes.byref(args)) == -1
    assert b"null" in lib.mev_last_error()
    assert lib.mev_evaluate_plans(None, None) == -1
    assert b"null" in lib.mev_last_error()
    # (handle, NULL): the arguments are checked before the handle is looked at, so any address serves
    lib.mev_last_error.restype = ctypes.c_char_p
    dummy = (ctypes.c_uint8 * 64)()
    assert lib.mev_evaluate_plans(ctypes.addressof(dummy), None) == -1
    assert b"null" in lib.mev_last_error()
