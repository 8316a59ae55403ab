"""mev_step_sequence and mev_restore_map without a device: the header declares them with the
struct in its stated field order, the library exports both, the ctypes struct is the header's,
and null arguments are refused."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_code():
    src = open(os.path.join(ROOT, "include", "marlenv.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_both_entry_points():
    code = _header_code()
    assert re.search(r"\bint\s+mev_step_sequence\s*\(\s*mev_handle\s*\*\s*\w+\s*,\s*const\s+mev_sequence_args\s*\*", code)
    assert re.search(r"\bint\s+mev_restore_map\s*\(\s*mev_handle\s*\*\s*\w+\s*,\s*const\s+void\s*\*\s*\w+\s*,"
                     r"\s*const\s+int32_t\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*\)", code)
    assert re.search(r"#define\s+MEV_ABI_VERSION\s+3\b", code)  # additive: the ABI version stays
    assert re.search(r"#define\s+MEV_MAX_REPEAT\s+64\b", code)


def test_header_struct_field_order():
    code = _header_code()
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*mev_sequence_args\s*;", code, flags=re.S)
    assert m, "mev_sequence_args is not declared"
    names = re.findall(r"(\w+)\s*;", m.group(1))
    assert names == ["step", "length", "dt_seq", "reward_seq", "done_seq", "status_seq", "substeps"]
    body = m.group(1)
    assert re.search(r"mev_step_args\s+step\s*;", body) and re.search(r"int32_t\s+length\s*;", body)
    assert re.search(r"const\s+float\s*\*\s*dt_seq\s*;", body) and re.search(r"float\s*\*\s*reward_seq\s*;", body)
    assert re.search(r"uint8_t\s*\*\s*done_seq\s*;", body) and re.search(r"uint8_t\s*\*\s*status_seq\s*;", body)
    assert re.search(r"int32_t\s*\*\s*substeps\s*;", body)
    # the frame-skip struct is untouched
    assert re.search(r"mev_step_args\s+step\s*;[^{}]*int32_t\s+repeat\s*;[^{}]*int32_t\s*\*\s*substeps\s*;[^{}]*\}"
                     r"\s*mev_repeat_args\s*;", code, flags=re.S)


def test_library_exports_both(mev):
    lib = mev.load_library()
    assert hasattr(lib, "mev_step_sequence") and hasattr(lib, "mev_restore_map")
    assert "mev_step_sequence" in mev._capi.EXPORTED and "mev_restore_map" in mev._capi.EXPORTED
    assert lib.mev_abi_version() == 3
    # the ctypes struct is the header's
    a = mev._capi.MevSequenceArgs
    assert [f[0] for f in a._fields_] == ["step", "length", "dt_seq", "reward_seq", "done_seq", "status_seq", "substeps"]
    assert a.length.offset == ctypes.sizeof(mev._capi.MevStepArgs)
    p = ctypes.sizeof(ctypes.c_void_p)
    assert a.dt_seq.offset == a.length.offset + p  # (int32 + padding to the pointer's alignment)
    assert [getattr(a, k).offset - a.dt_seq.offset for k in ("reward_seq", "done_seq", "status_seq", "substeps")] == \
        [p, 2 * p, 3 * p, 4 * p]
    assert ctypes.sizeof(a) == a.substeps.offset + p
    assert [f[0] for f in mev._capi.MevRepeatArgs._fields_] == ["step", "repeat", "substeps"]


def test_null_arguments_are_refused_without_a_device(mev):
    lib = mev.load_library()
    args = mev._capi.MevSequenceArgs()
    args.length = 2
    assert lib.mev_step_sequence(None, ctypes.byref(args)) == -1
    assert b"null" in lib.mev_last_error()
    assert lib.mev_step_sequence(None, None) == -1
    assert b"null" in lib.mev_last_error()
    buf = (ctypes.c_uint8 * 64)()
    emap = (ctypes.c_int32 * 4)()
    assert lib.mev_restore_map(None, buf, emap, 0) == -1
    assert b"null" in lib.mev_last_error()
    assert lib.mev_restore_map(None, None, None, 0) == -1
    assert b"null" in lib.mev_last_error()
