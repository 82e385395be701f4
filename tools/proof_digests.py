#!/usr/bin/python3
"""The sha256 of the proof bytes of the seven constraint systems of tests/systems_util.py: one SHPLONK and one GWC proof each, resident
columns, parts form, the default witnesses and the tests' fixed seeds.  A proof is a deterministic function of the key, the witness,
the seed and the code, so the digests of one tree pin what its prover writes: tests/golden/proof_digests.json holds the output of this
tool run on the tree before the shuffle and mv-lookup arguments entered create_proof, and tests/test_proof_arguments.py asserts that
the present tree reproduces it.
  python tools/proof_digests.py     (run on the GPU box; prints one JSON object)"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED = b"\x07" * 32


def digests():
    import systems_util as fam
    out = {}
    for name in fam.NAMES:
        su = fam.setup(name)
        out[name] = {multiopen: hashlib.sha256(su.prove(multiopen=multiopen, form="parts", resident=True, seed=SEED).bytes).hexdigest()
                     for multiopen in ("shplonk", "gwc")}
    return out


if __name__ == "__main__":
    print(json.dumps(digests(), indent=1, sort_keys=True))
