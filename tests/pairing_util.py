"""Python-integer model of the BN254 optimal ate pairing for tests/test_pairing.py and tests/golden/make_pairing_golden.py, written from
the definition alone: nothing here calls the library and nothing is shaped like csrc/pairing_host.h.

  * Fq12 is the single-variable ring Fq[w] / (w^12 - 18 w^6 + 82): twelve integers, schoolbook products.  u = w^6 - 9 (so u^2 = -1 and
    xi = 9 + u = w^6); an Fq2 element a + b u is (a - 9 b) + b w^6.
  * G2 is affine over Fq2 on the twist y^2 = x^3 + 3 / xi; (x', y') untwists to (x' w^2, y' w^3).
  * lines are affine, l(P) = (y_P - y_T) - lambda (x_P - x_T) with lambda = lambda' w, verticals left out (the exponent kills them);
  * the final exponentiation is one plain pow by (q^12 - 1) / r.

  e(P, Q) = ( f_{6t+2,Q}(P) * l_{T,pi(Q)}(P) * l_{T+pi(Q),-pi^2(Q)}(P) )^((q^12 - 1) / r),   t = 4965661367192848881

About 5 s per pairing.  Gt values travel as twelve integers c_0..c_11 (the coefficients of w^i); the library's 48 limbs are twelve
Montgomery Fq a_0, b_0, ..., a_5, b_5 with c_i = a_i - 9 b_i and c_{i+6} = b_i (include/halo2hip_pairing.h)."""
import hashlib

import numpy as np

Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
T = 4965661367192848881
ATE = 6 * T + 2
EXPONENT = (Q ** 12 - 1) // R
MONT = (1 << 256) % Q
MONT_INV = pow(MONT, -1, Q)
G1 = (1, 2)
G2 = ((0x1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed, 0x198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2),
      (0x12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa, 0x090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b))
E_G1_G2_SHA256 = "b504b117b4fe4dd61d484a8cc670ae6222cd8c37f10384186a3650f3439b07a9"

assert (Q ** 12 - 1) % R == 0 and ATE.bit_length() == 65 and bin(ATE).count("1") == 37

ONE = (1,) + (0,) * 11


# ---- Fq12 = Fq[w] / (w^12 - 18 w^6 + 82) ----------------------------------------------------------------------------------------------
def f12_mul(a, b):
    t = [0] * 23
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                t[i + j] += x * y
    for i in range(22, 11, -1):  # w^i = 18 w^(i-6) - 82 w^(i-12)
        t[i - 6] += 18 * t[i]
        t[i - 12] -= 82 * t[i]
    return tuple(x % Q for x in t[:12])


def f12_pow(a, e):
    out = ONE
    while e:
        if e & 1:
            out = f12_mul(out, a)
        a = f12_mul(a, a)
        e >>= 1
    return out


def f12_from_fq2(z, shift):
    """(a + b u) w^shift, shift < 6"""
    out = [0] * 12
    out[shift] = (z[0] - 9 * z[1]) % Q
    out[shift + 6] = z[1] % Q
    return tuple(out)


# ---- Fq2 and the twist ------------------------------------------------------------------------------------------------------------
def f2_add(a, b):
    return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)


def f2_sub(a, b):
    return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2_inv(a):
    d = pow((a[0] * a[0] + a[1] * a[1]) % Q, Q - 2, Q)
    return (a[0] * d % Q, -a[1] * d % Q)


def f2_pow(a, e):
    out = (1, 0)
    while e:
        if e & 1:
            out = f2_mul(out, a)
        a = f2_mul(a, a)
        e >>= 1
    return out


XI = (9, 1)
B2 = f2_mul((3, 0), f2_inv(XI))


def g2_on_twist(p):
    if p is None:
        return True
    x, y = p
    return f2_mul(y, y) == f2_add(f2_mul(f2_mul(x, x), x), B2)


def g2_neg(p):
    return None if p is None else (p[0], ((-p[1][0]) % Q, (-p[1][1]) % Q))


def _slope(a, b):
    """the slope of the line through a and b (the tangent when they are equal), or None when it is vertical"""
    if a[0] == b[0]:
        if a[1] != b[1] or a[1] == (0, 0):
            return None
        xx = f2_mul(a[0], a[0])
        return f2_mul(f2_add(f2_add(xx, xx), xx), f2_inv(f2_add(a[1], a[1])))
    return f2_mul(f2_sub(b[1], a[1]), f2_inv(f2_sub(b[0], a[0])))


def g2_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    lam = _slope(a, b)
    if lam is None:
        return None
    x = f2_sub(f2_sub(f2_mul(lam, lam), a[0]), b[0])
    return (x, f2_sub(f2_mul(lam, f2_sub(a[0], x)), a[1]))


def g2_mul(p, k):
    acc = None
    while k:
        if k & 1:
            acc = g2_add(acc, p)
        p = g2_add(p, p)
        k >>= 1
    return acc


def g1_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    if a[0] == b[0]:
        if (a[1] + b[1]) % Q == 0:
            return None
        lam = 3 * a[0] * a[0] * pow(2 * a[1], Q - 2, Q) % Q
    else:
        lam = (b[1] - a[1]) * pow(b[0] - a[0], Q - 2, Q) % Q
    x = (lam * lam - a[0] - b[0]) % Q
    return (x, (lam * (a[0] - x) - a[1]) % Q)


def g1_mul(p, k):
    acc = None
    while k:
        if k & 1:
            acc = g1_add(acc, p)
        p = g1_add(p, p)
        k >>= 1
    return acc


def g1_neg(p):
    return None if p is None else (p[0], -p[1] % Q)


def frobenius(p):
    """pi on the untwisted point, back in twist coordinates: (x' w^2)^q = conj(x') xi^((q-1)/3) w^2, (y' w^3)^q = conj(y') xi^((q-1)/2) w^3"""
    (x0, x1), (y0, y1) = p
    return (f2_mul((x0, -x1 % Q), f2_pow(XI, (Q - 1) // 3)), f2_mul((y0, -y1 % Q), f2_pow(XI, (Q - 1) // 2)))


# ---- the pairing ------------------------------------------------------------------------------------------------------------------
def _line(t, s, p):
    """l_{t,s}(p) and t + s; 1 for a vertical line"""
    lam = _slope(t, s)
    if lam is None:
        return ONE, None
    # y_P - (y' w^3) - lam' w (x_P - x' w^2) = y_P - lam' x_P w + (lam' x' - y') w^3
    val = [0] * 12
    val[0] = p[1] % Q
    for z, shift in (((-lam[0] * p[0]) % Q, (-lam[1] * p[0]) % Q), 1), (f2_sub(f2_mul(lam, t[0]), t[1]), 3):
        for i, c in enumerate(f12_from_fq2(z, shift)):
            val[i] = (val[i] + c) % Q
    return tuple(val), g2_add(t, s)


def miller(p, q):
    """f_{6t+2,Q}(P) l_{T,pi(Q)}(P) l_{T+pi(Q),-pi^2(Q)}(P), P and Q not the identity"""
    f, t = ONE, q
    for bit in bin(ATE)[3:]:
        l, t2 = _line(t, t, p)
        f = f12_mul(f12_mul(f, f), l)
        t = t2
        if bit == "1":
            l, t = _line(t, q, p)
            f = f12_mul(f, l)
    q1 = frobenius(q)
    q2 = g2_neg(frobenius(q1))
    l, t = _line(t, q1, p)
    f = f12_mul(f, l)
    l, t = _line(t, q2, p)
    return f12_mul(f, l)


def final_exponentiation(f):
    return f12_pow(f, EXPONENT)


def pairing(p, q):
    """e(P, Q) as twelve integers; 1 when either side is the identity (None)"""
    if p is None or q is None:
        return ONE
    return final_exponentiation(miller(p, q))


def pairing_product(pairs):
    f = ONE
    for p, q in pairs:
        if p is not None and q is not None:
            f = f12_mul(f, miller(p, q))
    return final_exponentiation(f)


def gt_digest(c):
    return hashlib.sha256(b"".join(int(x).to_bytes(32, "little") for x in c)).hexdigest()


# ---- the library's layouts --------------------------------------------------------------------------------------------------------
def gt_from_limbs(limbs):
    """(48,) uint64 -> the twelve integers c_i"""
    v = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(12, 4)
    m = [int.from_bytes(row.tobytes(), "little") * MONT_INV % Q for row in v]
    c = [0] * 12
    for i in range(6):
        a, b = m[2 * i], m[2 * i + 1]
        c[i], c[i + 6] = (a - 9 * b) % Q, b
    return tuple(c)


def gt_to_limbs(c):
    m = []
    for i in range(6):
        b = c[i + 6]
        m += [(c[i] + 9 * b) % Q, b]
    return np.frombuffer(b"".join((x * MONT % Q).to_bytes(32, "little") for x in m), dtype=np.uint64).copy()


def g2_raw(p):
    """an affine twist point over plain integers -> the 128 raw bytes of ParamsKZG.g2 (None: the identity)"""
    if p is None:
        return bytes(128)
    return b"".join((c * MONT % Q).to_bytes(32, "little") for c in p[0] + p[1])


def g2_plain(raw):
    raw = bytes(raw)
    if raw == bytes(128):
        return None
    c = [int.from_bytes(raw[32 * i:32 * i + 32], "little") * MONT_INV % Q for i in range(4)]
    return (c[0], c[1]), (c[2], c[3])


def g1_limbs(points):
    """[(x, y) | None] -> (n, 8) uint64 Montgomery"""
    data = b"".join((c * MONT % Q).to_bytes(32, "little") for p in points for c in (p or (0, 0)))
    return np.frombuffer(data, dtype=np.uint64).reshape(-1, 8).copy()


def g2_limbs(points):
    """[twist point | None] -> (n, 16) uint64"""
    return np.frombuffer(b"".join(g2_raw(p) for p in points), dtype=np.uint64).reshape(-1, 16).copy()


def twist_point_outside_subgroup():
    """a point of the twist whose order does not divide r: the twist's group has order r (2q - r), so a point found by solving y for a
    small x lies outside the r-torsion with overwhelming probability; checked against [r]Q"""
    from serde_util import f2_sqrt
    for c in range(1, 100):
        x = (c, 1)
        y = f2_sqrt(f2_add(f2_mul(f2_mul(x, x), x), B2))
        if y is not None and g2_mul((x, y), R) is not None:
            return (x, y)
    raise AssertionError("no twist point found")
