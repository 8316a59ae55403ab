"""mev_sample_expand_plans without a device: the header declares the struct in its stated field order
and the signature, the ABI version stays 3, the library exports the symbol, the ctypes struct is the
header's, and null arguments are refused."""
import ctypes
import re

import test_sample_plans_cpu as SC

FIELDS = ["sample", "src", "dst", "dst_slots", "counter_offset"]


def test_header_declares_the_entry_point():
    code = SC._header_code()
    assert re.search(r"\bint\s+mev_sample_expand_plans\s*\(\s*mev_handle\s*\*\s*\w+\s*,\s*const\s+"
                     r"mev_sample_expand_args\s*\*\s*\w+\s*\)", code)
    assert re.search(r"#define\s+MEV_ABI_VERSION\s+3\b", code)  # additive: the ABI version stays


def test_header_struct_field_order():
    code = SC._header_code()
    assert SC._struct_names(code, "mev_sample_expand_args") == FIELDS
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*mev_sample_expand_args\s*;", code, flags=re.S)
    types = [re.sub(r"\s+", " ", d.strip()) for d in m.group(1).split(";") if d.strip()]
    assert types == ["mev_sample_args sample", "const mev_pool* src", "mev_pool* dst", "const int32_t* dst_slots",
                     "uint64_t counter_offset"]
    # the structs it is made of are untouched
    assert SC._struct_names(code, "mev_sample_args") == SC.SAMPLE_FIELDS
    assert SC._struct_names(code, "mev_expand_args") == ["eval", "leaf_obs", "src", "dst", "dst_slots", "counter_offset"]


def test_library_exports_the_symbol(mev):
    lib = mev.load_library()
    assert hasattr(lib, "mev_sample_expand_plans")
    assert "mev_sample_expand_plans" in mev._capi.EXPORTED
    assert lib.mev_abi_version() == 3


def test_ctypes_struct_is_the_headers(mev):
    x = mev._capi.MevSampleExpandArgs
    assert [f[0] for f in x._fields_] == FIELDS
    assert dict(x._fields_)["sample"] is mev._capi.MevSampleArgs
    # the C layout on an LP64 target: mev_sample_args (200 bytes), three pointers, a uint64
    assert {k: getattr(x, k).offset for k in FIELDS} == dict(sample=0, src=200, dst=208, dst_slots=216, counter_offset=224)
    assert ctypes.sizeof(x) == 232
    assert dict(x._fields_)["counter_offset"] is ctypes.c_uint64


def test_null_arguments_are_refused_without_a_device(mev):
    lib = mev.load_library()
    lib.mev_last_error.restype = ctypes.c_char_p
    dummy = (ctypes.c_uint8 * 64)()
    fn, args = lib.mev_sample_expand_plans, mev._capi.MevSampleExpandArgs()
    assert fn(None, ctypes.byref(args)) == -1
    assert b"null" in lib.mev_last_error()
    assert fn(None, None) == -1
    assert b"null" in lib.mev_last_error()
    # (handle, NULL): the arguments are checked before the handle is looked at, so any address serves
    assert fn(ctypes.addressof(dummy), None) == -1
    assert b"null" in lib.mev_last_error()
