#!/usr/bin/python3
"""Mint tests/golden/pairing.json from the integer model of tests/pairing_util.py: products of pairings e([a] G1, [b] G2) as twelve
integers c_0..c_11 (the coefficients of w^i in Fq[w] / (w^12 - 18 w^6 + 82)).  A scalar 0 stands for the identity.  The library is not
called.  Run: python tests/golden/make_pairing_golden.py   (about 5 s)"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pairing_util as pu  # noqa: E402

A254 = 0x2b3c5d7e9f10213243546576879809a1b2c3d4e5f60718293a4b5c6d7e8f9012
B254 = 0x2f0e1d2c3b4a59687786958473625140f1e2d3c4b5a69788796a5b4c3d2e1f07
assert A254.bit_length() == B254.bit_length() == 254 and A254 < pu.R and B254 < pu.R

CASES = [
    ("generators", [(1, 1)]),
    ("2_3", [(2, 3)]),
    ("r-1_1", [(pu.R - 1, 1)]),
    ("1_r-1", [(1, pu.R - 1)]),
    ("254_bits", [(A254, B254)]),
    ("three_pairs", [(5, 7), (11, 13), (pu.R - 17, 19)]),
    ("identity_g1", [(0, 5)]),
    ("identity_g2", [(5, 0)]),
    ("identity_among_pairs", [(0, 5), (3, 4), (6, 0)]),
    ("empty", []),
]


def main():
    out = {"sha256_generators": None, "cases": []}
    for name, pairs in CASES:
        points = [(pu.g1_mul(pu.G1, a), pu.g2_mul(pu.G2, b)) for a, b in pairs]
        gt = pu.pairing_product(points)
        if name == "generators":
            out["sha256_generators"] = pu.gt_digest(gt)
            assert out["sha256_generators"] == pu.E_G1_G2_SHA256
        out["cases"].append({"name": name, "pairs": [["%x" % a, "%x" % b] for a, b in pairs], "gt": ["%x" % c for c in gt]})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pairing.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
