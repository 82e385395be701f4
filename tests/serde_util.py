"""Python-integer reference for the serialisation tests (tests/test_serde.py, tests/golden/make_serde_golden.py): the five per-element
conversions of SerdeFormat (helpers.rs:8-20) and the G2 encoding, written from the definitions alone -- nothing here calls the library.
What pins the encodings is this file and the known points (1, 2) and EIP-197's G2 generator.
Arrays are numpy: compressed points and Fr reprs (n, 32) uint8, raw points (n, 8) uint64, Fr (n, 4) uint64, Montgomery R = 2^256."""
import numpy as np

Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
MONT = 1 << 256
QR, QRINV = MONT % Q, pow(MONT, -1, Q)
RR, RRINV = MONT % R, pow(MONT, -1, R)
H2HIP_EENCODING = 5


def sqrt_q(t):
    """a square root of t in Fq, or None (q = 3 mod 4)"""
    y = pow(t, (Q + 1) // 4, Q)
    return y if y * y % Q == t % Q else None


def ints(a):
    """(n, 4k) uint64 -> n tuples of k integers"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return [tuple(int.from_bytes(row[32 * j:32 * j + 32], "little") for j in range(len(row) // 32)) for row in (r.tobytes() for r in a)]


def limbs(values):
    """integers below 2^256 -> (n, 4) uint64"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint64).reshape(-1, 4).copy()


def points(xy):
    """[(x, y)] plain integers -> (n, 8) uint64 Montgomery; None or (0, 0): the identity"""
    return limbs([c * QR % Q for p in xy for c in (p or (0, 0))]).reshape(-1, 8)


def g1_compress_one(x, y):
    """plain affine coordinates -> 32 bytes; (0, 0) is the identity"""
    if (x, y) == (0, 0):
        return bytes(32)
    b = bytearray(x.to_bytes(32, "little"))
    b[31] |= (y & 1) << 7
    return bytes(b)


def g1_decompress_one(b):
    """32 bytes -> plain (x, y), (0, 0) for the identity, None for an invalid encoding"""
    sign = b[31] >> 7
    x = int.from_bytes(bytes(b[:31]) + bytes([b[31] & 0x7f]), "little")
    if x == 0 and not sign:
        return (0, 0)
    if x >= Q:
        return None
    y = sqrt_q((x * x * x + 3) % Q)
    if y is None:
        return None
    if (y & 1) != sign:
        y = (Q - y) % Q
    return (x, y)


def g1_from_bytes(data):
    """(n, 32) uint8 -> ((n, 8) uint64 with invalid encodings as zeros, [invalid indices])"""
    pts = [g1_decompress_one(bytes(row)) for row in np.asarray(data, dtype=np.uint8).reshape(-1, 32)]
    return points(pts), [i for i, p in enumerate(pts) if p is None]


def g1_to_bytes(pts):
    return np.frombuffer(b"".join(g1_compress_one(x * QRINV % Q, y * QRINV % Q) for x, y in ints(pts)), dtype=np.uint8).reshape(-1, 32).copy()


def g1_invalid(pts):
    """indices that fail read_raw's checks: a coordinate not below q, or neither (0, 0) nor on y^2 = x^3 + 3"""
    bad = []
    for i, (xm, ym) in enumerate(ints(pts)):
        x, y = xm * QRINV % Q, ym * QRINV % Q
        if xm >= Q or ym >= Q or ((xm, ym) != (0, 0) and (y * y - x * x * x - 3) % Q):
            bad.append(i)
    return bad


def fr_from_repr(data):
    """(n, 32) uint8 -> ((n, 4) uint64 with values >= r as zeros, [invalid indices])"""
    vals = [int.from_bytes(bytes(row), "little") for row in np.asarray(data, dtype=np.uint8).reshape(-1, 32)]
    return limbs([v * RR % R if v < R else 0 for v in vals]), [i for i, v in enumerate(vals) if v >= R]


def fr_to_repr(a):
    return np.frombuffer(b"".join((v * RRINV % R).to_bytes(32, "little") for (v,) in ints(a)), dtype=np.uint8).reshape(-1, 32).copy()


def g1_mul(k, p=(1, 2)):
    """[k] p on y^2 = x^3 + 3, plain affine integers; (0, 0) is the identity"""
    def add(a, b):
        if a == (0, 0):
            return b
        if b == (0, 0):
            return a
        if a[0] == b[0]:
            if (a[1] + b[1]) % Q == 0:
                return (0, 0)
            lam = 3 * a[0] * a[0] * pow(2 * a[1], -1, Q) % Q
        else:
            lam = (b[1] - a[1]) * pow(b[0] - a[0], -1, Q) % Q
        x = (lam * lam - a[0] - b[0]) % Q
        return (x, (lam * (a[0] - x) - a[1]) % Q)
    acc = (0, 0)
    while k:
        if k & 1:
            acc = add(acc, p)
        p = add(p, p)
        k >>= 1
    return acc


# ---- G2: Fq2 = Fq[u] / (u^2 + 1), y^2 = x^3 + 3 / (9 + u) ---------------------------------------------------------------------------
# EIP-197's generator, as (c0, c1) = (real, imaginary) parts
G2_GEN = ((0x1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed, 0x198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2),
          (0x12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa, 0x090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b))


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2_inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
    return (a[0] * d % Q, -a[1] * d % Q)


G2_B = f2_mul((3, 0), f2_inv((9, 1)))


def g2_on_twist(x, y):
    x3 = f2_mul(f2_mul(x, x), x)
    return f2_mul(y, y) == ((x3[0] + G2_B[0]) % Q, (x3[1] + G2_B[1]) % Q)


def f2_sqrt(a):
    """a square root in Fq2 by a^((q^2 + 7) / 16)-free means: try both signs of the norm's root (a = (x0 + x1 u)^2 gives x0^2 - x1^2 = a0,
    2 x0 x1 = a1, so x0^2 = (a0 +- |a|) / 2); None when a is not a square"""
    if a == (0, 0):
        return a
    n = sqrt_q((a[0] * a[0] + a[1] * a[1]) % Q)
    if n is None:
        return None
    for s in (n, Q - n):
        x0 = sqrt_q((a[0] + s) * pow(2, -1, Q) % Q)
        if x0:
            r = (x0, a[1] * pow(2 * x0, -1, Q) % Q)
            if f2_mul(r, r) == a:
                return r
    x1 = sqrt_q(-a[0] % Q)  # a1 == 0 and a0 a non-residue
    return (0, x1) if a[1] == 0 and x1 is not None else None


def g2_raw(x, y):
    """plain Fq2 coordinates -> 128 raw bytes; None: the identity"""
    if x is None:
        return bytes(128)
    return b"".join((c * QR % Q).to_bytes(32, "little") for c in x + y)


def g2_raw_to_plain(raw):
    c = [int.from_bytes(raw[32 * i:32 * i + 32], "little") * QRINV % Q for i in range(4)]
    return (c[0], c[1]), (c[2], c[3])


def g2_compress(raw):
    if raw == bytes(128):
        return bytes(64)
    x, y = g2_raw_to_plain(raw)
    b = bytearray(x[0].to_bytes(32, "little") + x[1].to_bytes(32, "little"))
    b[63] |= (y[0] & 1) << 7
    return bytes(b)


def g2_decompress(b):
    """64 bytes -> 128 raw bytes, or None for an invalid encoding"""
    if b == bytes(64):
        return bytes(128)
    sign = b[63] >> 7
    x = (int.from_bytes(b[:32], "little"), int.from_bytes(bytes(b[32:63]) + bytes([b[63] & 0x7f]), "little"))
    if max(x) >= Q:
        return None
    x3 = f2_mul(f2_mul(x, x), x)
    y = f2_sqrt(((x3[0] + G2_B[0]) % Q, (x3[1] + G2_B[1]) % Q))
    if y is None:
        return None
    if (y[0] & 1) != sign:
        y = (-y[0] % Q, -y[1] % Q)
    return g2_raw(x, y)


# ---- whole params files (poly/kzg/commitment.rs:142-244): k u32 LE | g | g_lagrange | g2 | s_g2 ----------------------------------------
def params_raw_to_processed(raw):
    k = int.from_bytes(raw[:4], "little")
    n = 1 << k
    assert len(raw) == 4 + 2 * n * 64 + 256
    pts = np.frombuffer(raw[4:4 + 2 * n * 64], dtype=np.uint64).reshape(-1, 8)
    assert not g1_invalid(pts)
    g2 = raw[4 + 2 * n * 64:]
    return raw[:4] + g1_to_bytes(pts).tobytes() + g2_compress(g2[:128]) + g2_compress(g2[128:])


def params_processed_to_raw(proc):
    k = int.from_bytes(proc[:4], "little")
    n = 1 << k
    assert len(proc) == 4 + 2 * n * 32 + 128
    pts, bad = g1_from_bytes(np.frombuffer(proc[4:4 + 2 * n * 32], dtype=np.uint8))
    assert not bad
    g2 = proc[4 + 2 * n * 32:]
    return proc[:4] + pts.tobytes() + g2_decompress(g2[:64]) + g2_decompress(g2[64:])
