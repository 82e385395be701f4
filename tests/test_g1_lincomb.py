"""CPU: few-term group sums on the host (include/halo2hip_g1.h, csrc/g1_host.h) against the integer arithmetic of proof_util.g1_add /
g1_mul.
  * random sums at several (m, t), the scalars 0, 1 and r - 1, identities among the points and the addends, and every exceptional case
    of the closing addition and of the additions inside the ladder (a doubling, a cancellation);
  * every contract violation is H2HIP_EINVAL with its text, and needs no GPU;
  * halo2-pse_amd/_abi_g1.py and halo2hip-sys/src/ffi_g1.rs are the translations of the header, and lib() binds every name;
  * tests/cpp/test_g1_lincomb.cpp calls the same function on the same edge cases, plain and under ASan + UBSan (a program of its own:
    nothing sanitised is loaded into Python)."""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from proof_util import G1, Q, g1_add, g1_mul
from lookup_util import R_MOD as R

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_ctypes_abi  # noqa: E402
import gen_rust_extern  # noqa: E402

HEADER = "halo2hip_g1.h"
NAMES = ["h2hip_g1_linear_combinations_bn254"]
H2HIP_EINVAL = 1
_FQ_R = (1 << 256) % Q


def neg(p):
    return None if p is None else (p[0], -p[1] % Q)


def jacobian(p, z):
    """the Jacobian limbs of the affine integer pair p with the given z, as an MSM returns a sum (z = 0: the identity)"""
    if p is None:
        coords = (0, 1, 0)
    else:
        coords = (p[0] * z * z % Q, p[1] * z * z * z % Q, z % Q)
    return np.array([(c * _FQ_R % Q >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for c in coords for i in range(4)], dtype=np.uint64)


def want(addends, scalars, points):
    out = []
    for j, row in enumerate(scalars):
        acc = None if addends is None else addends[j]
        for s, p in zip(row, points):
            acc = g1_add(acc, None if p is None else g1_mul(p, s))
        out.append(acc)
    return out


def run(h2, addends, scalars, points, rng):
    """the wrapper over integer inputs; an addend is handed over with a random z"""
    jac = None if addends is None else [jacobian(a, rng.randrange(1, Q)) for a in addends]
    return h2.g1_linear_combinations(jac, scalars, points)


def pt(rng):
    return g1_mul(G1, rng.randrange(1, R))


@pytest.mark.parametrize("m,t", [(1, 1), (2, 2), (5, 1), (1, 40), (3, 0)])
def test_random_sums(h2, m, t):
    rng = random.Random(1000 * m + t)
    points = [pt(rng) for _ in range(t)]
    scalars = [[rng.randrange(R) for _ in range(t)] for _ in range(m)]
    addends = [pt(rng) for _ in range(m)]
    assert run(h2, addends, scalars, points, rng) == want(addends, scalars, points)
    if t:
        assert run(h2, None, scalars, points, rng) == want(None, scalars, points)


def test_edge_operands(h2):
    rng = random.Random(7)
    P, S, A = pt(rng), pt(rng), pt(rng)
    s = rng.randrange(2, R)
    # the scalars 0, 1 and r - 1
    scalars = [[0, 1], [1, R - 1], [R - 1, 0], [0, 0]]
    assert run(h2, [A] * 4, scalars, [P, S], rng) == want([A] * 4, scalars, [P, S])
    assert run(h2, None, scalars, [P, S], rng) == [S, g1_add(P, neg(S)), neg(P), None]
    # a (0, 0) point, whatever its scalar
    assert run(h2, [A], [[s, 5]], [None, S], rng) == [g1_add(A, g1_mul(S, 5))]
    assert run(h2, None, [[s]], [None], rng) == [None]
    # an identity addend
    assert run(h2, [None, None], [[s, 3], [0, 0]], [P, S], rng) == [g1_add(g1_mul(P, s), g1_mul(S, 3)), None]
    # the addend equals the rest of the sum: the closing addition is a doubling
    rest = g1_add(g1_mul(P, s), g1_mul(S, 3))
    assert run(h2, [rest], [[s, 3]], [P, S], rng) == [g1_add(rest, rest)]
    # the addend is the negative of the rest: the identity comes out, beside a sum that does not cancel
    assert run(h2, [neg(rest), A], [[s, 3], [s, 3]], [P, S], rng) == [None, g1_add(A, rest)]
    # equal and opposite points under equal scalars: a doubling and a cancellation inside the ladder
    assert run(h2, [A], [[s, s]], [P, P], rng) == [g1_add(A, g1_mul(P, 2 * s))]
    assert run(h2, [A], [[s, s]], [P, neg(P)], rng) == [A]
    assert run(h2, None, [[s, s]], [P, neg(P)], rng) == [None]
    assert run(h2, None, [[1, 1]], [P, P], rng) == [g1_add(P, P)]
    # t = 0: a batch normalisation, identities among the addends
    assert run(h2, [A, None, P], [[], [], []], [], rng) == [A, None, P]
    # m = 0 succeeds and writes nothing, with or without pointers
    assert h2.g1_linear_combinations(None, [], [P]) == []
    assert h2.g1_linear_combinations([], [], []) == []
    assert h2.lib().h2hip_g1_linear_combinations_bn254(None, None, None, 0, 3, None) == 0


def test_contract_violations(h2):
    L, p = h2.lib(), h2._p
    one = h2.fr_from_int(1)
    big = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    P = h2.g1_from_int(G1)
    off = h2.g1_from_int((1, 3))                                    # not on the curve
    unreduced = P.copy()
    unreduced[:4] = big                                             # a coordinate that is not below q
    out = np.zeros((2, 8), dtype=np.uint64)
    addend = jacobian(G1, 1)
    pts2, sc2 = np.stack([P, off]), np.stack([one, one])
    cases = [
        ((None, p(np.stack([one, big])), p(np.stack([P, P])), 1, 2, p(out)), "g1_linear_combinations: scalars[1] is not a reduced Fr element"),
        ((None, p(sc2), p(pts2), 1, 2, p(out)), "g1_linear_combinations: points_xy[1] is neither on the curve nor (0, 0)"),
        ((None, p(one), p(unreduced), 1, 1, p(out)), "g1_linear_combinations: points_xy[0] is neither on the curve nor (0, 0)"),
        ((None, p(one), p(P), 1, 1, None), "g1_linear_combinations: null out_xy"),
        ((p(addend), None, None, 1, 0, None), "g1_linear_combinations: null out_xy"),
        ((None, None, p(P), 1, 1, p(out)), "g1_linear_combinations: null scalars"),
        ((None, p(one), None, 1, 1, p(out)), "g1_linear_combinations: null points_xy"),
        ((None, p(one), p(P), 4097, 1, p(out)), "g1_linear_combinations: m = 4097 sums of t = 1 terms are more than 4096 terms: that is an MSM"),
        ((None, p(one), p(P), 2, 2049, p(out)), "g1_linear_combinations: m = 2 sums of t = 2049 terms are more than 4096 terms: that is an MSM"),
        ((None, p(one), p(P), 1 << 63, 4, p(out)), "g1_linear_combinations: m = %d sums of t = 4 terms are more than 4096 terms: that is an MSM" % (1 << 63)),
    ]
    for args, text in cases:
        out[:] = 0xAB
        rc = L.h2hip_g1_linear_combinations_bn254(*args)
        assert rc == H2HIP_EINVAL and L.h2hip_last_error().decode() == text, (rc, L.h2hip_last_error().decode(), text)
        assert (out == 0xAB).all()                                  # a rejected call writes nothing
    with pytest.raises(h2.H2HipError, match="is not a reduced Fr element"):
        h2.g1_linear_combinations_limbs(None, big, P)
    with pytest.raises(h2.H2HipError, match="neither on the curve"):
        h2.g1_linear_combinations(None, [[1]], [(1, 3)])
    with pytest.raises(ValueError):
        h2.g1_linear_combinations(None, [[1, 2]], [G1])
    # 4096 terms are taken (t = 0 has no bound on m)
    assert L.h2hip_g1_linear_combinations_bn254(None, p(np.zeros((4096, 4), dtype=np.uint64)), p(P), 4096, 1, p(np.zeros((4096, 8), dtype=np.uint64))) == 0


def test_tables_are_the_translation_of_the_header(h2):
    assert open(os.path.join(ROOT, "halo2-pse_amd", "_abi_g1.py")).read() == gen_ctypes_abi.render((HEADER,), "test_g1_lincomb.py")
    assert open(os.path.join(ROOT, "halo2hip-sys", "src", "ffi_g1.rs")).read() == gen_rust_extern.render(HEADER, "test_g1_lincomb.py")
    table = sys.modules["halo2_pse_amd._abi_g1"].PROTOTYPES
    declared = {name: args for _, name, args in gen_rust_extern.prototypes(HEADER)}
    assert list(table) == NAMES == list(declared)
    assert not set(table) & (set(sys.modules["halo2_pse_amd._abi"].PROTOTYPES) | set(sys.modules["halo2_pse_amd._abi_ipa"].PROTOTYPES))
    v = ctypes.c_void_p
    assert table[NAMES[0]] == (ctypes.c_int, [v, v, v, ctypes.c_size_t, ctypes.c_size_t, v])
    rust = open(os.path.join(ROOT, "halo2hip-sys", "src", "ffi_g1.rs")).read()
    assert re.findall(r"pub fn (h2hip_[a-z0-9_]+)\(", rust) == NAMES
    lib_rs = open(os.path.join(ROOT, "halo2hip-sys", "src", "lib.rs")).read()
    assert "mod ffi_g1;" in lib_rs and "pub mod g1;" in lib_rs
    wrappers = open(os.path.join(ROOT, "halo2hip-sys", "src", "g1.rs")).read()
    assert re.search(r"pub fn try_g1_linear_combinations<", wrappers)
    assert set(re.findall(r"ffi::(h2hip_[a-z0-9_]+)\(", wrappers)) == set(NAMES)


def test_library_exports_and_lib_binds_every_name(h2):
    raw = ctypes.CDLL(h2.LIB_PATH)
    L, table = h2.lib(), sys.modules["halo2_pse_amd._abi_g1"].PROTOTYPES
    for name, (restype, argtypes) in table.items():
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    with pytest.raises(TypeError):
        L.h2hip_g1_linear_combinations_bn254(None, None, None, 0, 0)  # the count is exact


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan_ubsan"])
def test_the_same_function_in_a_program_of_its_own(tmp_path, flags):
    """csrc/g1_host.h compiled into tests/cpp/test_g1_lincomb.cpp: the edge cases above against a double-and-add of its own"""
    exe = str(tmp_path / "test_g1_lincomb")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "test_g1_lincomb.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "g1 lincomb host tests ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
