"""The C++ mirror of the KZG closing (halo2-pse_amd/host/kzg.hpp: poly::kzg::{MSMKZG, DualMSM, GuardKZG, SingleStrategy,
AccumulatorStrategy}, pairing) through the stand-alone program tests/cpp/test_pairing_mirror, on the hand-made term lists of
tests/test_pairing.py: DualMSM::check is true on the lists that close and false on the shifted ones, SingleStrategy and
AccumulatorStrategy follow, params without G2 points give an error instead of a verdict, and the Gt bytes equal kzg.py's.  The host
path needs no GPU; with the threshold forced below the lists' lengths both sides go through the engine's MSM."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import pairing_util as pu
from conftest import ROOT, load_pkg
from test_pairing import _dual

h2 = load_pkg()
kzg = importlib.import_module("halo2_pse_amd.kzg")
EXE = os.path.join(ROOT, "tests", "cpp", "test_pairing_mirror")
S = 0x1234567890ABCDEF1234567


def test_cpp_pairing_mirror_builds():
    """the Makefile targets of the two programs, which `all` and `tests` list"""
    makefile = open(os.path.join(ROOT, "halo2-pse_amd", "Makefile")).read()
    for name in ("test_pairing_mirror", "test_pairing_host"):
        target = os.path.join("..", "tests", "cpp", name)
        r = subprocess.run(["make", "-C", os.path.join(ROOT, "halo2-pse_amd"), target], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert os.path.exists(os.path.join(ROOT, "tests", "cpp", name))
        for goal in ("all:", "tests:"):
            line = [ln for ln in makefile.splitlines() if ln.startswith(goal)][0]
            assert "../tests/cpp/" + name in line.split(), (goal, name)
    assert "../include/halo2hip_pairing.h" in [ln for ln in makefile.splitlines() if ln.startswith("HDRS :=")][0].split()


def _write(path, dual):
    with open(path, "wb") as f:
        f.write(np.array([len(dual.left.terms), len(dual.right.terms)], dtype=np.uint64).tobytes())
        for side in (dual.left, dual.right):
            for s, p in side.terms:
                f.write(h2.fr_from_int(s).tobytes() + h2.g1_from_int(p).tobytes())
        f.write(dual.params.g2 + dual.params.s_g2)


def _run(tmp_path, dual, *args):
    path = str(tmp_path / "terms.bin")
    _write(path, dual)
    r = subprocess.run([EXE, path] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pairing mirror ok" in r.stdout and "FAIL" not in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout.splitlines()


def _compare(lines, dual, closes):
    left, right = kzg.eval_msm(dual.left), kzg.eval_msm(dual.right)
    want = kzg.pairing([left, right], [dual.params.s_g2, kzg.g2_neg(dual.params.g2)])
    assert lines[0] == "check %d" % closes and dual.check() == bool(closes)
    got = np.array([int(x, 16) for x in lines[1].split()[1:]], dtype=np.uint64)
    assert lines[1].startswith("gt ") and np.array_equal(got, want)
    assert (pu.gt_from_limbs(got) == pu.ONE) == bool(closes)
    assert lines[2].startswith("single accepted" if closes else "single refused: ConstraintSystemFailure")
    assert lines[3] == "accumulated %d %d" % (2 * len(dual.left.terms), closes)
    assert lines[4] == "no g2: error"


@pytest.mark.parametrize("shift,closes", [(0, 1), (1, 0)], ids=["closes", "shifted"])
def test_cpp_dual_msm_on_the_host_path(tmp_path, shift, closes):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    dual = _dual(S, shift=shift)
    _compare(_run(tmp_path, dual), dual, closes)


@pytest.mark.gpu
@pytest.mark.parametrize("shift,closes", [(0, 1), (1, 0)], ids=["closes", "shifted"])
def test_gpu_cpp_dual_msm_on_the_engine_path(tmp_path, shift, closes):
    assert os.path.exists(EXE), "run __graft_entry__.build() first"
    dual = _dual(S, shift=shift)
    _compare(_run(tmp_path, dual, 2), dual, closes)
