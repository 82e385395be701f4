"""CPU: the host pairing of include/halo2hip_pairing.h (csrc/pairing_host.h) and kzg.py's DualMSM against the integer model of
tests/pairing_util.py (single-variable Fq12, affine lines, one plain pow: it shares no structure with the C++).
  * tests/golden/pairing.json was minted once from the model (tests/golden/make_pairing_golden.py); the library's Gt equals it limb for
    limb, one test re-runs the model for one vector, and e(G1, G2) has the digest the definition was first checked with;
  * e(a P, b Q) = e(P, Q)^(ab), the power taken by the model on the library's value;
  * pairing_check closes {(L, s G2), (-s L, G2)} and refuses s + 1; g2_mul against the model;
  * every contract violation is H2HIP_EINVAL with its text, a rejected call writes nothing, and no call needs h2.init;
  * halo2-pse_amd/_abi_pairing.py and halo2hip-sys/src/ffi_pairing.rs are the translations of the header, and lib() binds every name;
  * DualMSM.check on hand-made term lists, both evaluation paths (the engine's MSM path is forced by a low threshold and needs a GPU);
  * tests/cpp/test_pairing_host.cpp runs the same header plain and under ASan + UBSan, as a program of its own."""
import ctypes
import importlib
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import pairing_util as pu
from conftest import ROOT, load_pkg

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_ctypes_abi  # noqa: E402
import gen_rust_extern  # noqa: E402

load_pkg()
kzg = importlib.import_module("halo2_pse_amd.kzg")
verifier = importlib.import_module("halo2_pse_amd.verifier")

HEADER = "halo2hip_pairing.h"
NAMES = ["h2hip_pairing_check_bn254", "h2hip_pairing_bn254", "h2hip_g2_mul_bn254", "h2hip_g2_check_bn254"]
H2HIP_EINVAL = 1
R, Q = pu.R, pu.Q
G2_RAW = pu.g2_raw(pu.G2)

with open(os.path.join(ROOT, "tests", "golden", "pairing.json")) as _f:
    GOLDEN = json.load(_f)
CASES = {c["name"]: ([(int(a, 16), int(b, 16)) for a, b in c["pairs"]], tuple(int(x, 16) for x in c["gt"])) for c in GOLDEN["cases"]}


def points_of(pairs):
    return [pu.g1_mul(pu.G1, a) for a, _ in pairs], [pu.g2_raw(pu.g2_mul(pu.G2, b)) for _, b in pairs]


def test_the_golden_file_has_the_issue_s_vectors():
    assert set(CASES) == {"generators", "2_3", "r-1_1", "1_r-1", "254_bits", "three_pairs", "identity_g1", "identity_g2",
                          "identity_among_pairs", "empty"}
    assert CASES["r-1_1"][0] == [(R - 1, 1)] and CASES["1_r-1"][0] == [(1, R - 1)] and len(CASES["three_pairs"][0]) == 3
    assert all(v.bit_length() == 254 for v in CASES["254_bits"][0][0])
    assert GOLDEN["sha256_generators"] == pu.E_G1_G2_SHA256 == pu.gt_digest(CASES["generators"][1])
    for name in ("identity_g1", "identity_g2", "empty"):
        assert CASES[name][1] == pu.ONE


@pytest.mark.parametrize("name", sorted(CASES))
def test_gt_equals_the_golden_limb_for_limb(h2, name):
    pairs, want = CASES[name]
    g1, g2 = points_of(pairs)
    got = kzg.pairing(g1, g2)
    assert got.shape == (48,) and np.array_equal(got, pu.gt_to_limbs(want))
    assert pu.gt_from_limbs(got) == want
    assert kzg.pairing_check(g1, g2) == (want == pu.ONE)


def test_the_model_again_for_one_vector():
    pairs, want = CASES["2_3"]
    assert pu.pairing(pu.g1_mul(pu.G1, 2), pu.g2_mul(pu.G2, 3)) == want
    assert want != pu.ONE and pu.f12_pow(want, R) == pu.ONE


@pytest.mark.parametrize("name", ["2_3", "r-1_1", "1_r-1", "254_bits"])
def test_bilinear_in_both_arguments(h2, name):
    (a, b), = CASES[name][0]
    base = pu.gt_from_limbs(kzg.pairing([pu.G1], [G2_RAW]))
    g1, g2 = points_of([(a, b)])
    assert pu.gt_from_limbs(kzg.pairing(g1, g2)) == pu.f12_pow(base, a * b % R)


def test_pairing_check_closes_with_the_same_s_only(h2):
    rng = random.Random(11)
    s = rng.randrange(2, R - 1)
    L = pu.g1_mul(pu.G1, rng.randrange(1, R))
    minus_sL = pu.g1_neg(pu.g1_mul(L, s))
    assert kzg.pairing_check([L, minus_sL], [kzg.g2_mul(G2_RAW, s), G2_RAW])
    assert not kzg.pairing_check([L, minus_sL], [kzg.g2_mul(G2_RAW, s + 1), G2_RAW])
    assert kzg.pairing_check([], []) and kzg.pairing_check([None, L], [G2_RAW, bytes(128)])
    assert kzg.g2_neg(kzg.g2_neg(G2_RAW)) == G2_RAW and kzg.g2_neg(bytes(128)) == bytes(128)
    assert kzg.pairing_check([L, L], [G2_RAW, kzg.g2_neg(G2_RAW)])


def test_g2_mul_against_the_model(h2):
    rng = random.Random(12)
    for k in (0, 1, 2, R - 1, rng.randrange(R)):
        assert kzg.g2_mul(G2_RAW, k) == pu.g2_raw(pu.g2_mul(pu.G2, k)), k
    assert kzg.g2_mul(G2_RAW, h2.fr_from_int(5)) == pu.g2_raw(pu.g2_mul(pu.G2, 5))       # Montgomery limbs as they are
    assert kzg.g2_mul(bytes(128), 7) == bytes(128)
    assert kzg.G2_GENERATOR == G2_RAW == h2.G2_GENERATOR
    # a twist point outside the subgroup is multiplied (it is on the twist) and told apart
    out = pu.twist_point_outside_subgroup()
    assert kzg.g2_mul(pu.g2_raw(out), 3) == pu.g2_raw(pu.g2_mul(out, 3))
    assert kzg.g2_check(pu.g2_raw(out)) == (True, False) and kzg.g2_check(G2_RAW) == (True, True) and kzg.g2_check(bytes(128)) == (True, True)
    off = pu.g2_raw((pu.G2[0], (pu.G2[1][0] + 1, pu.G2[1][1])))
    assert kzg.g2_check(off) == (False, False)


def test_contract_violations(h2):
    L, p = h2.lib(), h2._p
    P = pu.g1_limbs([pu.G1])
    Qr = pu.g2_limbs([pu.G2])
    big = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    off1 = pu.g1_limbs([(1, 3)])
    unreduced1 = P.copy()
    unreduced1[0, :4] = big
    off2 = pu.g2_limbs([(pu.G2[0], (pu.G2[1][0] + 1, pu.G2[1][1]))])
    unreduced2 = Qr.copy()
    unreduced2[0, 12:] = big
    outside = pu.g2_limbs([pu.twist_point_outside_subgroup()])
    two_p, two_q = np.concatenate([P, P]), np.concatenate([Qr, outside])
    cases = [
        ((None, p(Qr), 1), "null g1_xy"),
        ((p(P), None, 1), "null g2_raw"),
        ((p(P), p(Qr), 65537), "n = 65537 pairs are more than 65536: fold the batch first"),
        ((p(P), p(Qr), 1 << 63), "n = %d pairs are more than 65536: fold the batch first" % (1 << 63)),
        ((p(unreduced1), p(Qr), 1), "g1_xy[0] has a coordinate that is not below q"),
        ((p(off1), p(Qr), 1), "g1_xy[0] is neither on the curve nor (0, 0)"),
        ((p(P), p(unreduced2), 1), "g2_raw[0] has a coordinate that is not below q"),
        ((p(P), p(off2), 1), "g2_raw[0] is neither on the twist nor the identity"),
        ((p(P), p(outside), 1), "g2_raw[0] is not in the subgroup of order r"),
        ((p(two_p), p(two_q), 2), "g2_raw[1] is not in the subgroup of order r"),
    ]
    gt, ok = np.zeros(48, dtype=np.uint64), ctypes.c_int(0)
    for args, text in cases:
        gt[:], ok.value = 0xAB, 0xAB
        rc = L.h2hip_pairing_bn254(*args, p(gt))
        assert rc == H2HIP_EINVAL and L.h2hip_last_error().decode() == "pairing: " + text, (rc, L.h2hip_last_error().decode(), text)
        rc = L.h2hip_pairing_check_bn254(*args, ctypes.byref(ok))
        assert rc == H2HIP_EINVAL and L.h2hip_last_error().decode() == "pairing_check: " + text, (rc, L.h2hip_last_error().decode(), text)
        assert (gt == 0xAB).all() and ok.value == 0xAB                # a rejected call writes nothing
    assert L.h2hip_pairing_bn254(p(P), p(Qr), 1, None) == H2HIP_EINVAL and L.h2hip_last_error().decode() == "pairing: null out_gt"
    assert L.h2hip_pairing_check_bn254(p(P), p(Qr), 1, None) == H2HIP_EINVAL and L.h2hip_last_error().decode() == "pairing_check: null ok"
    assert L.h2hip_pairing_check_bn254(None, None, 0, ctypes.byref(ok)) == 0 and ok.value == 1   # n = 0 reads neither array
    one, out = h2.fr_from_int(1), np.zeros(16, dtype=np.uint64)
    g2_cases = [
        ((None, p(one), p(out)), "null g2_raw"), ((p(Qr), None, p(out)), "null scalar"), ((p(Qr), p(one), None), "null out_raw"),
        ((p(Qr), p(big), p(out)), "the scalar is not a reduced Fr element"),
        ((p(unreduced2), p(one), p(out)), "g2_raw has a coordinate that is not below q"),
        ((p(off2), p(one), p(out)), "g2_raw is neither on the twist nor the identity"),
    ]
    for args, text in g2_cases:
        out[:] = 0xAB
        rc = L.h2hip_g2_mul_bn254(*args)
        assert rc == H2HIP_EINVAL and L.h2hip_last_error().decode() == "g2_mul: " + text, (rc, L.h2hip_last_error().decode(), text)
        assert (out == 0xAB).all()
    a, b = ctypes.c_int(7), ctypes.c_int(7)
    for args, text in [((None, ctypes.byref(a), ctypes.byref(b)), "null g2_raw"), ((p(Qr), None, ctypes.byref(b)), "null on_curve"),
                       ((p(Qr), ctypes.byref(a), None), "null in_subgroup"),
                       ((p(unreduced2), ctypes.byref(a), ctypes.byref(b)), "g2_raw has a coordinate that is not below q")]:
        rc = L.h2hip_g2_check_bn254(*args)
        assert rc == H2HIP_EINVAL and L.h2hip_last_error().decode() == "g2_check: " + text and (a.value, b.value) == (7, 7)
    with pytest.raises(h2.H2HipError, match="not in the subgroup"):
        kzg.pairing([pu.G1], [pu.g2_raw(pu.twist_point_outside_subgroup())])
    with pytest.raises(ValueError):
        kzg.pairing([pu.G1], [])
    with pytest.raises(ValueError):
        kzg.pairing([pu.G1], [bytes(64)])


def test_tables_are_the_translation_of_the_header(h2):
    assert open(os.path.join(ROOT, "halo2-pse_amd", "_abi_pairing.py")).read() == gen_ctypes_abi.render((HEADER,), "test_pairing.py")
    assert open(os.path.join(ROOT, "halo2hip-sys", "src", "ffi_pairing.rs")).read() == gen_rust_extern.render(HEADER, "test_pairing.py")
    table = sys.modules["halo2_pse_amd._abi_pairing"].PROTOTYPES
    declared = {name: args for _, name, args in gen_rust_extern.prototypes(HEADER)}
    assert list(table) == NAMES == list(declared)
    others = [sys.modules["halo2_pse_amd." + m].PROTOTYPES for m in ("_abi", "_abi_ipa", "_abi_g1")]
    assert not any(set(table) & set(o) for o in others)
    v, i, z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    assert table == {NAMES[0]: (i, [v, v, z, v]), NAMES[1]: (i, [v, v, z, v]), NAMES[2]: (i, [v, v, v]), NAMES[3]: (i, [v, v, v])}
    rust = open(os.path.join(ROOT, "halo2hip-sys", "src", "ffi_pairing.rs")).read()
    assert re.findall(r"pub fn (h2hip_[a-z0-9_]+)\(", rust) == NAMES
    lib_rs = open(os.path.join(ROOT, "halo2hip-sys", "src", "lib.rs")).read()
    assert "mod ffi_pairing;" in lib_rs and "pub mod pairing;" in lib_rs
    wrappers = open(os.path.join(ROOT, "halo2hip-sys", "src", "pairing.rs")).read()
    for name in ("try_pairing_check", "try_pairing", "try_g2_mul"):
        assert re.search(r"pub fn %s\(" % name, wrappers)
    assert set(re.findall(r"ffi::(h2hip_[a-z0-9_]+)\(", wrappers)) == set(NAMES[:3])


def test_library_exports_and_lib_binds_every_name(h2):
    raw = ctypes.CDLL(h2.LIB_PATH)
    L, table = h2.lib(), sys.modules["halo2_pse_amd._abi_pairing"].PROTOTYPES
    for name, (restype, argtypes) in table.items():
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    with pytest.raises(TypeError):
        L.h2hip_pairing_check_bn254(None, None, 0)  # the count is exact


def test_the_calls_need_no_init():
    """a fresh process that never calls h2.init: the pairing, g2_mul and a DualMSM check run on the calling thread"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from conftest import load_pkg\n"
            "import importlib, pairing_util as pu\n"
            "h2 = load_pkg(); kzg = importlib.import_module('halo2_pse_amd.kzg')\n"
            "g2 = pu.g2_raw(pu.G2)\n"
            "assert pu.gt_digest(pu.gt_from_limbs(kzg.pairing([pu.G1], [g2]))) == pu.E_G1_G2_SHA256\n"
            "assert kzg.pairing_check([pu.G1, pu.g1_neg(pu.g1_mul(pu.G1, 5))], [kzg.g2_mul(g2, 5), g2])\n"
            "assert kzg.g2_check(g2) == (True, True)\n"
            "print('no init ok')\n") % (os.path.join(ROOT, "tests"), ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "no init ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- DualMSM on hand-made term lists -------------------------------------------------------------------------------------------------
class _Params:
    """what DualMSM reads of a ParamsKZG"""

    def __init__(self, s):
        self.g2, self.s_g2 = G2_RAW, pu.g2_raw(pu.g2_mul(pu.G2, s))


def _dual(s, shift=0, seed=21):
    """left = sum a_i P_i and right = s left (+ shift G1) as other terms: duplicates, an identity and a zero scalar among them"""
    rng = random.Random(seed)
    params = _Params(s)
    msm = kzg.DualMSM(params)
    pts = [pu.g1_mul(pu.G1, rng.randrange(1, R)) for _ in range(3)]
    coeffs = [rng.randrange(R) for _ in pts]
    for a, p in zip(coeffs, pts):
        msm.left.append_term(a, p)
    msm.left.append_term(5, None)
    msm.left.append_term(0, pts[0])
    for a, p in zip(coeffs, pts):                                     # s a_i = (s a_i - 1) + 1
        msm.right.append_term(s * a - 1, p)
        msm.right.append_term(1, p)
    if shift:
        msm.right.append_term(shift, pu.G1)
    return msm


def test_dual_msm_on_the_host_path(h2):
    s = 0x1234567890ABCDEF1234567
    assert _dual(s).check() and not _dual(s, shift=1).check()
    scaled = _dual(s)
    scaled.scale(12345)
    other = _dual(s, seed=22)
    scaled.add_msm(other)
    assert scaled.check() and len(scaled.left.terms) == 10
    bad = _dual(s)
    bad.add_msm(_dual(s, shift=3, seed=23))
    assert not bad.check()
    assert kzg.DualMSM(_Params(s)).check()                            # nothing accumulated: 1 = 1
    assert kzg.eval_msm(_dual(s).left) == verifier.MSM(_dual(s).left.terms).eval()
    empty = _Params(s)
    empty.g2 = bytes(128)
    with pytest.raises(verifier.VerifyError, match="no G2 points"):
        kzg.DualMSM(empty).check()
    # the strategies over a hand-made opening
    guard = lambda dual: (lambda acc: (acc.add_msm(dual), kzg.GuardKZG(acc))[1])  # noqa: E731
    assert kzg.SingleStrategy(_Params(s)).process(guard(_dual(s))) is None
    with pytest.raises(verifier.VerifyError, match="ConstraintSystemFailure"):
        kzg.SingleStrategy(_Params(s)).process(guard(_dual(s, shift=1)))


@pytest.mark.gpu
def test_dual_msm_on_the_engine_path(h2):
    """lincomb_terms = 2 sends both sides (5 and 6 terms after the identity is dropped) through h2hip_msm_bn254"""
    h2.init(0)
    s = 0x1234567890ABCDEF1234567
    good, bad = _dual(s), _dual(s, shift=1)
    assert kzg.eval_msm(good.left, 2) == kzg.eval_msm(good.left) == verifier.MSM(good.left.terms).eval()
    assert kzg.eval_msm(good.right, 2) == kzg.eval_msm(good.right)
    assert good.check(lincomb_terms=2) and not bad.check(lincomb_terms=2)
    acc = kzg.AccumulatorStrategy(_Params(s), h2.FrRng(b"\x05" * 32))
    for seed in (31, 32, 33):
        acc = acc.process(lambda a, seed=seed: (a.add_msm(_dual(s, seed=seed)), kzg.GuardKZG(a))[1])
    assert acc.finalize(lincomb_terms=2) and acc.finalize()


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan_ubsan"])
def test_the_same_header_in_a_program_of_its_own(tmp_path, flags):
    """csrc/pairing_host.h compiled into tests/cpp/test_pairing_host.cpp: the tower against schoolbook products, Frobenius and the hard
    part against plain powers, the G2 group law; its e(G1, G2) line equals the golden"""
    exe = str(tmp_path / "test_pairing_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "test_pairing_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "pairing host tests ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    line, = [ln for ln in r.stdout.splitlines() if ln.startswith("gt ")]
    limbs = np.array([int(x, 16) for x in line.split()[1:]], dtype=np.uint64)
    assert pu.gt_from_limbs(limbs) == CASES["generators"][1]
