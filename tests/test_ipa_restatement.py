"""CPU: the definitions the inner-product argument's GPU tests rest on.
  * the generator derivation: the product's integer form (ipa.hash_to_curve_int) and the tests' restatement (ipa_util.derive) give the
    golden points of tests/golden/ipa_generators.json, which are on the curve and come from the least valid counter;
  * the restatement itself (tests/ipa_util.py) at k = 1 .. 5: an opening verifies, a tampered one does not, <compute_s(u, 1), (x^i)> =
    compute_b(x, u), and construct_intermediate_sets gives the sets the reference's code gives on the query list of
    poly/multiopen_test.rs and on the same list with one polynomial opened at both points;
  * csrc/ipa_elem.h on the host (tests/cpp/test_ipa_host.cpp), plain and under ASan + UBSan."""
import hashlib
import json
import os
import subprocess

import pytest

import ipa_util as iu
from conftest import ROOT

R, Q = iu.R, iu.Q
SEED = bytes(range(32))


def _ipa():
    return __import__("halo2_pse_amd.ipa", fromlist=["ipa"])


def _transcript():
    return __import__("halo2_pse_amd.transcript", fromlist=["transcript"])


def test_generators_match_the_golden_points(h2):
    ipa = _ipa()
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "ipa_generators.json")))
    assert [r["name"] for r in rows] == ["g[%d]" % i for i in range(8)] + ["w", "u"]
    for i, row in enumerate(rows):
        message = bytes.fromhex(row["message"])
        assert message == (iu.g_message(i) if i < 8 else bytes([i - 7]))
        assert message == (ipa.generator_message(i) if i < 8 else (ipa.W_MESSAGE, ipa.U_MESSAGE)[i - 8])
        want = (int(row["x"], 16), int(row["y"], 16))
        assert iu.derive(message) == (want, row["counter"])
        assert ipa.hash_to_curve_int(message) == (want, row["counter"])
        assert iu.on_curve(want) and 0 < want[0] < Q and 0 < want[1] < Q
        assert ipa.generator_candidate(message, row["counter"]).hex() == row["compressed"]
        # the counter is the least valid one: every smaller counter's x has x^3 + 3 a non-residue
        for ctr in range(row["counter"]):
            h = hashlib.blake2b(message + ctr.to_bytes(4, "little"), digest_size=64, person=b"Halo2-Parameters").digest()
            x = int.from_bytes(h[:48], "little") % Q
            assert x == 0 or pow((x ** 3 + 3) % Q, (Q - 1) // 2, Q) == Q - 1, (row["name"], ctr)
    assert len({r["compressed"] for r in rows}) == len(rows)
    assert any(r["counter"] > 0 for r in rows)  # about half of the candidates are rejected: the redo path is exercised


@pytest.fixture(scope="module")
def params5():
    return iu.Params(5)


def _params(params5, k):
    return iu.Params(k, params5.g[:1 << k], params5.w, params5.u)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_restated_opening_verifies(h2, params5, k):
    T, grp = _transcript(), iu.Ints()
    params = _params(params5, k)
    rng = iu.Rng(SEED)
    poly = rng.draw(params.n)
    blind, x = rng.draw(2)
    commitment = params.commit(grp, poly, blind)
    v = iu.eval_poly(poly, x)
    w = T.Blake2bWrite()
    w.write_point(commitment)
    iu.create_proof(grp, params, rng, w, poly, blind, x)
    proof = w.finalize()
    assert len(proof) == 32 * (1 + 1 + 2 * k + 2)

    def check(proof, v):
        r = T.Blake2bRead(proof)
        msm = iu.MSM(params)
        msm.append_term(1, r.read_point())
        return iu.verify_proof(params, msm, r, x, v).eval(grp) is None

    assert check(proof, v)
    assert not check(proof, (v + 1) % R)
    bad = bytearray(proof)
    bad[-1 - 32] ^= 1  # a bit of c
    assert not check(bytes(bad), v)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_compute_s_and_compute_b_agree(k):
    rng = iu.Rng(SEED, stream_id=k)
    u = rng.draw(k)
    for x in [0, 1, R - 1, pow(iu.OMEGA_28, 1 << (28 - k), R)] + rng.draw(2):
        s = iu.compute_s(u, 1)
        assert sum(c * pow(x, i, R) for i, c in enumerate(s)) % R == iu.compute_b(x, u)
        # the product formula the engine's byte tables implement
        for i in range(1 << k):
            want = 7
            for t in range(k):
                if (i >> t) & 1:
                    want = want * u[k - 1 - t] % R
            assert iu.compute_s(u, 7)[i] == want


def test_construct_intermediate_sets(h2):
    ipa = _ipa()
    x, y = 0x1234, 0x99  # x > y as integers: an ordering by value would put y first, the reference orders by first appearance
    avx, bvx, cvy, avy = 11, 22, 33, 44
    # poly/multiopen_test.rs:198-201: a and b at x, c at y
    queries = [("a", x, avx), ("b", x, bvx), ("c", y, cvy)]
    want = ([("a", 0, [0], [avx]), ("b", 0, [0], [bvx]), ("c", 1, [1], [cvy])], [[x], [y]])
    assert iu.construct_intermediate_sets(queries) == want
    assert ipa.construct_intermediate_sets(queries) == want
    # one polynomial at both points: three sets, in the order their first commitment appears; a's evals follow the point indices
    queries = [("a", y, avy), ("b", x, bvx), ("c", y, cvy), ("a", x, avx)]
    want = ([("a", 0, [0, 1], [avy, avx]), ("b", 1, [1], [bvx]), ("c", 2, [0], [cvy])], [[y, x], [x], [y]])
    assert iu.construct_intermediate_sets(queries) == want
    assert ipa.construct_intermediate_sets(queries) == want
    # the same point queried twice for one commitment: point_indices repeats, the set does not
    queries = [("a", x, avx), ("a", x, avx), ("b", y, 5), ("b", x, 6)]
    got = iu.construct_intermediate_sets(queries)
    assert got == ipa.construct_intermediate_sets(queries)
    assert got[0][0] == ("a", 0, [0, 0], [avx, 0]) and got[0][1] == ("b", 1, [1, 0], [6, 5]) and got[1] == [[x], [x, y]]


SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.parametrize("flags,divide", [(["-O2"], 1), (SAN, 10)], ids=["plain", "asan_ubsan"])
def test_per_element_code_on_the_host(tmp_path, flags, divide):
    """the ladder, the collapse of one pair, the fold and the byte tables against 256-bit arithmetic, limb bounds asserted; the
    sanitised build runs a tenth of the random scalars and every crafted one"""
    exe = str(tmp_path / "test_ipa_host")
    subprocess.check_call(["g++", "-std=c++17", "-DH2_FU_CHECK", "-Wall", "-Wno-unknown-pragmas"] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "test_ipa_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(divide)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ipa host tests ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
