#!/usr/bin/python3
"""tests/golden/ipa_generators.json: the first eight g[i], w and u of ParamsIPA::new as this project derives them (DESIGN.md section 2,
"IPA generators"), minted with hashlib and Python integers only -- for message M and counter ctr = 0, 1, ...:
h = BLAKE2b-512(person = b"Halo2-Parameters", data = M || ctr as 4 bytes LE), x = (h[0:48] little-endian) mod q, sign = h[63] & 1, the
first counter with x != 0 and x^3 + 3 a square gives (x, the root whose low bit is sign).  Each row keeps the
message, the counter, both coordinates and the 32-byte compressed encoding, all as hex.

Run: python tests/golden/make_ipa_golden.py
"""
import hashlib
import json
import os

Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
HERE = os.path.dirname(os.path.abspath(__file__))


def derive(message):
    ctr = 0
    while True:
        h = hashlib.blake2b(message + ctr.to_bytes(4, "little"), digest_size=64, person=b"Halo2-Parameters").digest()
        x, sign = int.from_bytes(h[:48], "little") % Q, h[63] & 1
        t = (pow(x, 3, Q) + 3) % Q
        # Euler's criterion (x^3 + 3 = 0 has no solution: the group has odd order, so no point has y = 0)
        if x != 0 and pow(t, (Q - 1) // 2, Q) == 1:
            y = pow(t, (Q + 1) // 4, Q)
            return ctr, x, y if y & 1 == sign else Q - y
        ctr += 1


def main():
    rows = []
    for name, message in [("g[%d]" % i, bytes([0]) + i.to_bytes(4, "little")) for i in range(8)] + [("w", bytes([1])), ("u", bytes([2]))]:
        ctr, x, y = derive(message)
        assert (y * y - x ** 3 - 3) % Q == 0
        rows.append({"name": name, "message": message.hex(), "counter": ctr, "x": "%064x" % x, "y": "%064x" % y,
                     "compressed": (x | (y & 1) << 255).to_bytes(32, "little").hex()})
    path = os.path.join(HERE, "ipa_generators.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("wrote", path, [r["counter"] for r in rows])


if __name__ == "__main__":
    main()
