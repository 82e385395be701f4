"""CPU: the C ABI of a round of the inner-product argument as one call (include/halo2hip_ipa_round.h, part of halo2hip_ipa.h).
  * halo2-pse_amd/_abi_ipa_round.py and halo2hip-sys/src/ffi_ipa_round.rs are the translations of the header; the library exports both
    entry points, the boundary query and the knob's pair, and lib() binds each to its row of the regenerated table;
  * every contract violation is answered with H2HIP_EINVAL and its text before the engine is entered, so without a GPU;
  * the knob is a setting, on by default, and the boundary of the single run follows the tuning values;
  * the index and plan arithmetic of the pair MSM (csrc/msm_pair.h) as a stand-alone program, plain and under ASan + UBSan."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_ctypes_abi  # noqa: E402
import gen_rust_extern  # noqa: E402

HEADER = "halo2hip_ipa_round.h"
H2HIP_EINVAL = 1
NAMES = ["h2hip_ipa_round_msms_bn254_device", "h2hip_ipa_round_msms_fused_max_half", "h2hip_ipa_round_bn254_device",
         "h2hip_ipa_set_round_call", "h2hip_ipa_get_round_call"]


def test_tables_are_the_translation_of_the_header(h2):
    assert open(os.path.join(ROOT, "halo2-pse_amd", "_abi_ipa_round.py")).read() == gen_ctypes_abi.render((HEADER,), "test_ipa_round_abi.py")
    assert open(os.path.join(ROOT, "halo2hip-sys", "src", "ffi_ipa_round.rs")).read() == gen_rust_extern.render(HEADER, "test_ipa_round_abi.py")
    table = sys.modules["halo2_pse_amd._abi_ipa_round"].PROTOTYPES
    declared = {name: args for _, name, args in gen_rust_extern.prototypes(HEADER)}
    assert list(table) == NAMES == list(declared)
    others = [sys.modules["halo2_pse_amd." + m].PROTOTYPES for m in ("_abi", "_abi_ipa", "_abi_g1", "_abi_pairing")]
    assert not any(set(table) & set(o) for o in others)
    v, z = ctypes.c_void_p, ctypes.c_size_t
    assert table["h2hip_ipa_round_msms_bn254_device"] == (ctypes.c_int, [v, v, z, v, v, v])
    assert table["h2hip_ipa_round_bn254_device"] == (ctypes.c_int, [v, v, v, z, v, v, v, v, v, v])
    assert table["h2hip_ipa_set_round_call"] == (ctypes.c_int, [ctypes.c_int]) and table["h2hip_ipa_get_round_call"] == (ctypes.c_int, [])
    # halo2hip_ipa.h carries the declarations to whoever includes it
    assert '#include "halo2hip_ipa_round.h"' in open(os.path.join(ROOT, "include", "halo2hip_ipa.h")).read()
    lib_rs = open(os.path.join(ROOT, "halo2hip-sys", "src", "lib.rs")).read()
    assert "mod ffi_ipa_round;" in lib_rs and "pub mod ipa_round;" in lib_rs
    wrappers = open(os.path.join(ROOT, "halo2hip-sys", "src", "ipa_round.rs")).read()
    for fn in ("try_ipa_round", "try_ipa_round_msms"):
        assert re.search(r"pub (unsafe )?fn %s<" % fn, wrappers), fn
    assert set(re.findall(r"ffi::(h2hip_[a-z0-9_]+)\(", wrappers)) <= set(NAMES)


def test_library_exports_and_lib_binds_every_name(h2):
    raw = ctypes.CDLL(h2.LIB_PATH)
    L, table = h2.lib(), sys.modules["halo2_pse_amd._abi_ipa_round"].PROTOTYPES
    for name, (restype, argtypes) in table.items():
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    with pytest.raises(TypeError):
        L.h2hip_ipa_round_msms_bn254_device(None, None, 1, None, None)  # the count is exact
    with pytest.raises(TypeError):
        L.h2hip_ipa_set_round_call()


DEV, ODD = 0x10000, 0x10008  # a 16-byte aligned and a misaligned "device" address: a rejected call dereferences neither


def _cases(h2):
    one = h2.fr_from_int(1)
    big = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)  # not reduced
    out = np.zeros((2, 12), dtype=np.uint64)
    val = np.zeros((2, 4), dtype=np.uint64)
    p, q = h2._p, None
    o0, o1, v, u = p(out[0]), p(out[1]), p(val), p(one)
    top = (1 << 26) + 1
    m, r = "h2hip_ipa_round_msms_bn254_device", "h2hip_ipa_round_bn254_device"
    return [
        (m, (q, DEV, 1, o0, o1, None), "ipa_round_msms: null d_p"),
        (m, (DEV, q, 1, o0, o1, None), "ipa_round_msms: null d_g_xy"),
        (m, (DEV, DEV, 1, q, o1, None), "ipa_round_msms: null out_l"),
        (m, (DEV, DEV, 1, o0, q, None), "ipa_round_msms: null out_r"),
        (m, (DEV, DEV, 0, o0, o1, None), "ipa_round_msms: half = 0 is outside 1 .. 2^26"),
        (m, (DEV, DEV, top, o0, o1, None), "ipa_round_msms: half = %d is outside 1 .. 2^26" % top),
        (m, (ODD, DEV, 1, o0, o1, None), "ipa_round_msms: d_p is not 16-byte aligned"),
        (m, (DEV, ODD, 1, o0, o1, None), "ipa_round_msms: d_g_xy is not 16-byte aligned"),
        (r, (q, DEV, DEV, 1, q, q, o0, o1, v, None), "ipa_round: null d_p"),
        (r, (DEV, q, DEV, 1, q, q, o0, o1, v, None), "ipa_round: null d_b"),
        (r, (DEV, DEV, q, 1, q, q, o0, o1, v, None), "ipa_round: null d_g_xy"),
        (r, (DEV, DEV, DEV, 1, q, q, q, o1, v, None), "ipa_round: null out_l"),
        (r, (DEV, DEV, DEV, 1, q, q, o0, q, v, None), "ipa_round: null out_r"),
        (r, (DEV, DEV, DEV, 1, q, q, o0, o1, q, None), "ipa_round: null values"),
        (r, (DEV, DEV, DEV, 0, q, q, o0, o1, v, None), "ipa_round: half = 0 is outside 1 .. 2^26"),
        (r, (DEV, DEV, DEV, top, u, u, o0, o1, v, None), "ipa_round: half = %d is outside 1 .. 2^26" % top),
        (r, (ODD, DEV, DEV, 1, q, q, o0, o1, v, None), "ipa_round: d_p is not 16-byte aligned"),
        (r, (DEV, ODD, DEV, 1, q, q, o0, o1, v, None), "ipa_round: d_b is not 16-byte aligned"),
        (r, (DEV, DEV, ODD, 1, q, q, o0, o1, v, None), "ipa_round: d_g_xy is not 16-byte aligned"),
        (r, (DEV, DEV, DEV, 1, u, q, o0, o1, v, None), "ipa_round: u given without u_inv"),
        (r, (DEV, DEV, DEV, 1, q, u, o0, o1, v, None), "ipa_round: u_inv given without u"),
        (r, (DEV, DEV, DEV, 1, p(big), u, o0, o1, v, None), None),
        (r, (DEV, DEV, DEV, 1, u, p(big), o0, o1, v, None), None),
    ]


def test_contract_violations_are_rejected_before_the_engine(h2):
    L = h2.lib()
    for name, args, text in _cases(h2):
        rc = getattr(L, name)(*args)
        err = L.h2hip_last_error().decode()
        assert rc == H2HIP_EINVAL, (name, args, rc, err)
        if text is None:  # a scalar that is not reduced: check_fr's text names the argument
            assert "not a reduced Fr element" in err, (name, err)
        else:
            assert err == text, (name, err)


def test_the_knob_and_the_boundary_are_settings(h2):
    ipa = __import__("halo2_pse_amd.ipa", fromlist=["ipa"])
    L = h2.lib()
    assert L.h2hip_ipa_get_round_call() == 1  # the default
    try:
        assert ipa.set_round_call(False) is False and L.h2hip_ipa_get_round_call() == 0
        assert ipa.set_round_call(True) is True
    finally:
        ipa.set_round_call(True)
    # the single run's boundary is read from Tuning::msm_fuse_max_n and Tuning::msm_fuse_entries
    assert ipa.round_msms_fused_max_half() == 1 << 19
    try:
        L.h2hip_debug_set_msm_fuse_limits(0, 1 << 11)
        assert ipa.round_msms_fused_max_half() == 1 << 11
        L.h2hip_debug_set_msm_fuse_limits(1 << 20, 0)  # 2 half W <= 2^20 with the fused plan's W = 22 windows at 2^14 <= half < 2^15
        assert ipa.round_msms_fused_max_half() == (1 << 20) // (2 * 22)
    finally:
        L.h2hip_debug_set_msm_fuse_limits(0, 0)
    assert ipa.round_msms_fused_max_half() == 1 << 19


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan_ubsan"])
def test_pair_index_and_plan_arithmetic_on_the_host(tmp_path, flags):
    """the rotated index, the set assignment and the fall-back boundary (csrc/msm_pair.h) as a program of their own"""
    exe = str(tmp_path / "test_msm_pair_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "test_msm_pair_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "msm pair host tests ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
