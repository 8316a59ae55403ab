"""mev_sample_plans and mev_update_plans without a device: the header declares both structs in their
stated field order and both signatures, the ABI version stays 3, the library exports the symbols,
the ctypes structs are the header's, null arguments are refused, and the restated noise
(plan_noise_ref) has the stated constant and the stated moments."""
import ctypes
import os
import re

import numpy as np

import plan_noise_ref as PN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SAMPLE_FIELDS = ["eval", "leaf_obs", "mean", "sigma", "lo", "hi", "groups", "samples", "noise_seed", "noise_counter",
                 "actions_out", "sample_flags"]
UPDATE_FIELDS = ["actions", "scores", "returns", "groups", "samples", "length", "mode", "elites", "inv_temperature",
                 "sigma_min", "new_mean", "new_sigma", "best", "best_score", "order", "weights", "flags"]


def _header_code():
    src = open(os.path.join(ROOT, "include", "marlenv.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def _struct_names(code, name):
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*" + name + r"\s*;", code, flags=re.S)
    assert m, name + " is not declared"
    names = []
    for decl in m.group(1).split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, *rest = decl.split(",")
        names.append(re.search(r"(\w+)\s*(\[\d+\])?$", first.strip()).group(1))
        names += [re.search(r"(\w+)", r).group(1) for r in rest]
    return names


def test_header_declares_the_entry_points():
    code = _header_code()
    for fn, st in (("mev_sample_plans", "mev_sample_args"), ("mev_update_plans", "mev_update_args")):
        assert re.search(r"\bint\s+" + fn + r"\s*\(\s*mev_handle\s*\*\s*\w+\s*,\s*const\s+" + st + r"\s*\*\s*\w+\s*\)", code)
    assert re.search(r"#define\s+MEV_ABI_VERSION\s+3\b", code)  # additive: the ABI version stays
    assert re.search(r"#define\s+MEV_SAMPLE_MEAN_FIRST\s+0x1u\b", code)
    assert re.search(r"#define\s+MEV_MAX_SAMPLES\s+4096\b", code)
    assert re.search(r"MEV_UPDATE_ELITES\s*=\s*0\s*,\s*MEV_UPDATE_SOFTMAX\s*=\s*1", code)


def test_header_struct_field_order():
    code = _header_code()
    assert _struct_names(code, "mev_sample_args") == SAMPLE_FIELDS
    assert _struct_names(code, "mev_update_args") == UPDATE_FIELDS
    # the neighbouring struct is untouched
    assert _struct_names(code, "mev_expand_args") == ["eval", "leaf_obs", "src", "dst", "dst_slots", "counter_offset"]


def test_library_exports_the_symbols(mev):
    lib = mev.load_library()
    for fn in ("mev_sample_plans", "mev_update_plans"):
        assert hasattr(lib, fn)
        assert fn in mev._capi.EXPORTED
    assert lib.mev_abi_version() == 3
    assert mev._capi.MEV_MAX_SAMPLES == 4096 and mev._capi.MEV_SAMPLE_MEAN_FIRST == 1
    assert (mev._capi.MEV_UPDATE_ELITES, mev._capi.MEV_UPDATE_SOFTMAX) == (0, 1)


def test_ctypes_structs_are_the_headers(mev):
    s, u = mev._capi.MevSampleArgs, mev._capi.MevUpdateArgs
    assert [f[0] for f in s._fields_] == SAMPLE_FIELDS
    assert [f[0] for f in u._fields_] == UPDATE_FIELDS
    assert ctypes.sizeof(ctypes.c_void_p) == 8
    # the C layout of the header's structs on an LP64 target.  mev_sample_args: mev_evaluate_args (120 bytes), three
    # pointers, four floats, two int32, two uint64, a pointer, a uint32 and the tail padding
    want = dict(eval=0, leaf_obs=120, mean=128, sigma=136, lo=144, hi=152, groups=160, samples=164, noise_seed=168,
                noise_counter=176, actions_out=184, sample_flags=192)
    assert {k: getattr(s, k).offset for k in SAMPLE_FIELDS} == want
    assert ctypes.sizeof(s) == 200
    # mev_update_args: three pointers, five int32, two floats, padding to the next pointer, six pointers, a uint32
    want = dict(actions=0, scores=8, returns=16, groups=24, samples=28, length=32, mode=36, elites=40, inv_temperature=44,
                sigma_min=48, new_mean=56, new_sigma=64, best=72, best_score=80, order=88, weights=96, flags=104)
    assert {k: getattr(u, k).offset for k in UPDATE_FIELDS} == want
    assert ctypes.sizeof(u) == 112


def test_null_arguments_are_refused_without_a_device(mev):
    lib = mev.load_library()
    lib.mev_last_error.restype = ctypes.c_char_p
    dummy = (ctypes.c_uint8 * 64)()
    for fn, args in ((lib.mev_sample_plans, mev._capi.MevSampleArgs()), (lib.mev_update_plans, mev._capi.MevUpdateArgs())):
        assert fn(None, ctypes.byref(args)) == -1
        assert b"null" in lib.mev_last_error()
        assert fn(None, None) == -1
        assert b"null" in lib.mev_last_error()
        # (handle, NULL): the arguments are checked before the handle is looked at, so any address serves
        assert fn(ctypes.addressof(dummy), None) == -1
        assert b"null" in lib.mev_last_error()


def test_noise_constant_bits():
    assert PN.EPS_SCALE.dtype == np.float32
    assert int(PN.EPS_SCALE.view(np.uint32)) == 0x3B9CC4BF
    assert float(PN.EPS_SCALE) == float.fromhex("0x1.39897ep-8")


def test_philox4_known_answer():
    """Random123's known-answer vectors for philox4x32-10: the round function and key schedule are the standard's."""
    assert [int(w) for w in PN.philox4(0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    m = 0xFFFFFFFF
    assert [int(w) for w in PN.philox4(m, m, m, m, (m << 32) | m)] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_noise_moments():
    n = 65536
    c, i, s = np.meshgrid(np.arange(512), np.arange(16), np.arange(4), indexing="ij")  # 32768 draws of two floats
    eps = PN.noise(0x123456789ABCDEF, 7, c, i, s).reshape(-1).astype(np.float64)
    assert eps.size == n
    mean, var = eps.mean(), eps.var()
    print("mean", mean, "variance", var, "max |eps|", np.abs(eps).max())
    assert abs(mean) < 5 / np.sqrt(n)                 # 0.0195
    assert abs(var - 1.0) < 5 * np.sqrt(1.85 / n)     # 0.0266: var(eps^2) = kurtosis - 1 = 1.85
    assert np.abs(eps).max() <= 4.88
    # the levels: an integer in [-1020, 1020] times the constant
    k = np.rint(eps / float(PN.EPS_SCALE))
    assert np.array_equal((k.astype(np.float32) * PN.EPS_SCALE).astype(np.float64), eps)
