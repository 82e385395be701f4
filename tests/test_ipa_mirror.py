"""The C++ mirror of the inner-product-argument commitment scheme (halo2-pse_amd/host/ipa.hpp: transcript::Blake2b{Write,Read},
poly::ipa::{ParamsIPA, MSMIPA, create_proof, verify_proof, ProverIPA, VerifierIPA, SingleStrategy}) through the stand-alone program
tests/cpp/test_ipa_mirror: at K = 4 and 10 it proves the round trip of poly/multiopen_test.rs::test_roundtrip_ipa on
ParamsIPA::new_(K)'s generators, verifies it, and rejects a wrong claimed evaluation and a flipped byte in every field.  The proof it
prints equals, byte for byte, the one halo2-pse_amd/ipa.py makes for the same seed: transcript, generator derivation, draw order and
every round agree between the two compositions."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "tests", "cpp", "test_ipa_mirror")
SEED = bytes(range(7, 39))  # the program's own


def test_cpp_ipa_mirror_builds():
    """the Makefile target of the program, which `all` and `tests` list"""
    target = os.path.join("..", "tests", "cpp", "test_ipa_mirror")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "halo2-pse_amd"), target], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert os.path.exists(EXE)
    makefile = open(os.path.join(ROOT, "halo2-pse_amd", "Makefile")).read()
    for goal in ("all:", "tests:"):
        line = [ln for ln in makefile.splitlines() if ln.startswith(goal)][0]
        assert "../tests/cpp/test_ipa_mirror" in line.split(), goal


def _python_proof(h2, k):
    import torch
    ipa = __import__("halo2_pse_amd.ipa", fromlist=["ipa"])
    T = __import__("halo2_pse_amd.transcript", fromlist=["transcript"])
    n = 1 << k
    with ipa.ParamsIPA.new(k) as params:
        rng = h2.FrRng(SEED)
        blind = h2.fr_to_int(rng.draw(1)[0])
        polys = [[10 + i for i in range(n)], [100 + i for i in range(n)], [100 + i for i in range(n)]]
        d_polys = [torch.from_numpy(np.stack([h2.fr_from_int(v) for v in p]).view(np.int64)).cuda() for p in polys]
        w = T.Blake2bWrite()
        for c in params.commit_many(d_polys, [blind] * 3):
            w.write_point(c)
        x, y = w.squeeze_challenge(), w.squeeze_challenge()
        for p, at in zip(polys, (x, x, y)):
            acc = 0
            for coeff in reversed(p):
                acc = (acc * at + coeff) % ipa.R
            w.write_scalar(acc)
        ipa.ProverIPA(params).create_proof(rng, w, [(x, d_polys[0], blind), (x, d_polys[1], blind), (y, d_polys[2], blind)])
        return w.finalize()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [4, 10])
def test_gpu_cpp_ipa_mirror(h2, k):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    h2.init()
    r = subprocess.run([EXE, str(k)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ipa mirror ok" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("proof ")]
    assert len(lines) == 1
    proof = bytes.fromhex(lines[0].split()[1])
    assert len(proof) == 32 * (6 + 1 + 2 + 1 + 2 * k + 2)
    assert proof == _python_proof(h2, k)
