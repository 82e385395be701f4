"""Inputs of the scalar NTT that random data never is (test infrastructure only).

Every input is built as raw stored words -- uint64[n, 4], the E-form integers below r that csrc/ntt.hip slices into 9 x 29-bit limbs --
because it is those integers whose size and limb pattern decide how far the lazily reduced arithmetic of csrc/fieldu.h is pushed.  The
transform is linear over them (a stored word is the field element times 2^256), so the closed forms below hold on the words directly:
with w the field value of the transform's root and n = 2^k,

    zero            all 0                          -> all 0
    const(c)        all c                          -> out[0] = n c, the others 0
    nyquist(c)      c, r - c, c, ...               -> out[n / 2] = n c, the others 0
    even_only(c)    c on even rows, 0 on odd       -> out[0] = out[n / 2] = (n / 2) c, the others 0
    delta(c, m)     c at row m, 0 elsewhere        -> out[i] = c w^(i m)
    tone(c, t)      a[j] = c w^(-t j)              -> out[t] = n c, the others 0
    extremes(seed)  every word drawn from VALUES   -> oracle only
    signs(c, seed)  every word c or r - c          -> oracle only

const(r - 1) walks the all-plus path of every butterfly (the largest unreduced values the tiles ever hold); the cancelling ones leave
exact multiples of r in front of the closing reductions, which must store them as 0 and not as r; limbmax saturates every 29-bit limb.
"""
import functools

import numpy as np

from product_util import R_MOD, from_mont, to_mont

ONE_E = (1 << 256) % R_MOD
LIMBMAX = (0x30644D << 232) | ((1 << 232) - 1)  # every 29-bit limb at its maximum, still below r
VALUES = {
    "0": 0,
    "1": 1,
    "r-1": R_MOD - 1,
    "r-2": R_MOD - 2,
    "limbmax": LIMBMAX,
    "2^253": 1 << 253,
    "(r-1)/2": (R_MOD - 1) // 2,
    "ONE_E": ONE_E,
    "r-ONE_E": R_MOD - ONE_E,
}
assert all(0 <= v < R_MOD for v in VALUES.values())
_VALUE_LIST = list(VALUES.values())
_M64 = (1 << 64) - 1
_R_WORDS = [(R_MOD >> (64 * j)) & _M64 for j in range(4)]
SPARSE = ("zero", "const", "nyquist", "even_only", "tone")  # patterns whose whole output is one or two rows and zeros


def words(ints):
    """integers below 2^256 -> uint64[len, 4] little-endian words, as they are (no Montgomery conversion)"""
    out = np.zeros((len(ints), 4), dtype=np.uint64)
    for i, v in enumerate(ints):
        for j in range(4):
            out[i, j] = (v >> (64 * j)) & _M64
    return out


def ints(arr):
    """uint64[n, 4] -> the integers they hold"""
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in np.asarray(arr, dtype=np.uint64).reshape(-1, 4)]


def _pick(table_ints, idx):
    return words(table_ints)[np.asarray(idx, dtype=np.int64)]


def below_r(arr):
    """per row: the stored word is canonical (< r)"""
    a = np.asarray(arr, dtype=np.uint64).reshape(-1, 4)
    lt = np.zeros(a.shape[0], dtype=bool)
    eq = np.ones(a.shape[0], dtype=bool)
    for j in (3, 2, 1, 0):
        lt |= eq & (a[:, j] < np.uint64(_R_WORDS[j]))
        eq &= a[:, j] == np.uint64(_R_WORDS[j])
    return lt


def root_int(fe):
    """the field value of a root (or any constant) handed over in the reference's Montgomery words"""
    return from_mont(fe)[0]


# ---------------------------------------------------------------------------------------------------------- the patterns
def zero(n):
    return np.zeros((n, 4), dtype=np.uint64)


def const(n, c):
    return _pick([c], np.zeros(n, dtype=np.int64))


def nyquist(n, c):
    return _pick([c, (R_MOD - c) % R_MOD], np.arange(n) & 1)


def even_only(n, c):
    return _pick([c, 0], np.arange(n) & 1)


def delta(n, c, m):
    a = zero(n)
    a[m] = words([c])[0]
    return a


def tone_ints(n, c, t, w):
    step, p, out = pow(w, -t, R_MOD), 1, []
    for _ in range(n):
        out.append(c * p % R_MOD)
        p = p * step % R_MOD
    return out


def tone(n, c, t, w, oracle=None):
    """a[j] = c w^(-t j).  Up to 2^12 points from Python integers; beyond, with an oracle given, as the transform of delta(c, t) with the
    root 1 / w (out[j] = c (1/w)^(j t): the same words, test_tone_from_the_oracle_equals_the_integers), n big-integer products otherwise"""
    if n > 1 << 12 and oracle is not None:
        return oracle.best_fft(delta(n, c, t), to_mont([pow(w, -1, R_MOD)])[0], n.bit_length() - 1, 16)
    return words(tone_ints(n, c, t, w))


def extremes(n, seed):
    return _pick(_VALUE_LIST, np.random.RandomState(seed).randint(len(_VALUE_LIST), size=n))


def signs(n, c, seed):
    return _pick([c, (R_MOD - c) % R_MOD], np.random.RandomState(seed).randint(2, size=n))


def build(spec, n, w, oracle=None):
    """spec = (pattern, value name or None, argument): the input of n points for the transform with root w (an integer).  The argument is
    a row or tone as a string -- "0", "1", "half", "last" -- or a seed"""
    name, vname, arg = spec
    c = None if vname is None else VALUES[vname]
    if name == "zero":
        return zero(n)
    if name == "const":
        return const(n, c)
    if name == "nyquist":
        return nyquist(n, c)
    if name == "even_only":
        return even_only(n, c)
    if name == "delta":
        return delta(n, c, position(arg, n))
    if name == "tone":
        return tone(n, c, position(arg, n), w, oracle)
    if name == "extremes":
        return extremes(n, arg)
    if name == "signs":
        return signs(n, c, arg)
    raise KeyError(name)


def position(arg, n):
    return {"0": 0, "1": 1 % n, "half": n // 2, "last": n - 1}[arg]


@functools.lru_cache(maxsize=4096)
def _small(spec, n, w):
    a = build(spec, n, w)
    a.setflags(write=False)
    return a


def case_input(spec, n, w, oracle=None):
    """build(), computed once and shared read-only up to 2^13 points"""
    return _small(spec, n, w) if n <= 1 << 13 else build(spec, n, w, oracle)


def spec_id(spec):
    name, vname, arg = spec
    parts = [p for p in (vname, None if arg is None else str(arg)) if p is not None]
    return name + ("(" + ",".join(parts) + ")" if parts else "")


def full_specs(n):
    """every pattern with every value; rows and tones that coincide at small n appear once"""
    out = [("zero", None, None)]
    for v in VALUES:
        out += [("const", v, None), ("nyquist", v, None), ("even_only", v, None)]
        seen = set()
        for m in ("0", "1", "half", "last"):
            if position(m, n) not in seen:
                seen.add(position(m, n))
                out.append(("delta", v, m))
        out.append(("tone", v, "1"))
        if n > 2:
            out.append(("tone", v, "last"))
        out.append(("signs", v, 7))
    return out + [("extremes", None, 1), ("extremes", None, 2)]


# the columns every kernel family, closing reduction, twiddle source and the quarter branch see at the sizes where the oracle costs time
CORE_SPECS = [
    ("zero", None, None), ("const", "r-1", None), ("nyquist", "limbmax", None), ("even_only", "(r-1)/2", None), ("delta", "2^253", "1"),
    ("tone", "ONE_E", "1"), ("tone", "limbmax", "last"), ("signs", "r-1", 7), ("extremes", None, 1),
]
BIG_SPECS = [("const", "r-1", None), ("nyquist", "limbmax", None), ("signs", "r-1", 7), ("extremes", None, 1)]  # 2^21 and 2^22


# ------------------------------------------------------------------------------------------------------- the closed forms
def closed_form(spec, n, w, scale=1):
    """scale * DFT of the named input: {row: integer} for the SPARSE patterns (every other row is 0), a list for delta.  None for the
    patterns that have none"""
    name, vname, arg = spec
    c = None if vname is None else VALUES[vname]
    if name == "zero":
        return {}
    if name == "const":
        return {0: n * c * scale % R_MOD}
    if name == "nyquist":
        return {n // 2: n * c * scale % R_MOD}
    if name == "even_only":
        return {0: (n // 2) * c * scale % R_MOD, n // 2: (n // 2) * c * scale % R_MOD}
    if name == "tone":
        return {position(arg, n): n * c * scale % R_MOD}
    if name == "delta":
        step, p, out = pow(w, position(arg, n), R_MOD), 1, []
        for _ in range(n):
            out.append(c * p * scale % R_MOD)
            p = p * step % R_MOD
        return out
    return None


def dense(rows, n):
    """a SPARSE closed form as uint64[n, 4]"""
    out = zero(n)
    for i, v in rows.items():
        out[i] = words([v])[0]
    return out


def assert_below_r(got, tag=None):
    """a clear message when a reduction leaves a non-canonical word, a zero stored as r above all"""
    bad = np.flatnonzero(~below_r(got))
    assert bad.size == 0, ("output words not below r (a zero stored as r?)", tag, bad[:8], [hex(v) for v in ints(got[bad[:2]])])


def check_result(got, spec, n, w, scale=1, tag=None):
    """every output word canonical; for the SPARSE patterns the closed form, without the oracle: the one or two non-zero rows and
    nothing but zeros elsewhere"""
    assert_below_r(got, (tag, spec))
    if spec[0] not in SPARSE:
        return
    rows = closed_form(spec, n, w, scale)
    for i, v in rows.items():
        assert ints(got[i])[0] == v, ("closed form", tag, spec, i)
    rest = np.ones(n, dtype=bool)
    rest[list(rows)] = False
    assert np.count_nonzero(got[rest]) == 0, ("rows that must cancel to 0", tag, spec, np.flatnonzero(got[rest].any(axis=1))[:8])
