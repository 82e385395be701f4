"""Bucket sums chosen by the test, and an integer model of the MSM's bucket reduction (test infrastructure only).

Stage C of csrc/msm.hip turns the bucket sums B_b of a set into  set = sum_b (b + 1) B_b  with row/column passes, bit planes or a
final scaling, every one of them built from general XYZZ additions whose exceptional branches (equal operands, opposite operands, an
identity operand) random inputs never take.  Here every pair is (scalar, a) with the base [a]G, G the generator (1, 2):

  * a scalar whose signed digit in window w is d = b + 1 (1 <= d <= 2^(width - 1)) and zero elsewhere puts [a]G into slot b of set w in
    the plain form, and [2^pos_w a]G into slot b of the one shared set in the fixed-base form;
  * the expected result needs no MSM: [sum_i s_i a_i mod r]G.

`contents` names the bucket contents m[b] (B_b = [m[b]]G) after what they provoke.  `Model` restates stage C on integers mod r -- a point
is its multiple of G, G has prime order r, so two points are equal, opposite or the identity exactly when the integers are -- with the
geometry h2hip_debug_msm_reduce_plan reports, and classifies every addition per stage (STAGES x CLASSES).  It mirrors only the PAIRING
of operands (which two values meet in which addition), not the arithmetic.

Order inside a bucket: the model adds a bucket's entries in index order (pair index, then window).  The engine's sort places entries
with LDS cursors taken by atomics, so on the GPU entries of one bucket may arrive in another order; the bucket's SUM is the same, and
every content with at most one entry per bucket, or with equal entries, is exact.  heavy_alternate, heavy_chunks_cancel and
parts_cancel name the pairing of the index order; the GPU result is compared all the same.
"""
import ctypes
import functools

import numpy as np

from product_util import R_MOD

R = R_MOD
_MONT = (1 << 256) % R
STAGES = ("combine", "pass-1 chain", "pass-1 tree", "pass-2 chain", "pass-2 tree", "plane leaf", "plane tree", "plane partials",
          "final scale", "final tree", "heavy chain", "heavy tree", "heavy chunk sums")
CLASSES = ("generic", "doubling", "cancel", "identity-left", "identity-right", "both-identity")
GEN, DBL, CANCEL, ID_L, ID_R, BOTH = range(6)
TAILS = ("lane", "quad", "planes")


# ---------------------------------------------------------------------------------------------------------------- the hook
def reduce_plan(h2, n, fuse=1, table_c=0):
    """h2hip_debug_msm_reduce_plan as a dict (needs no GPU); g_log: one entry per row/column job in launch order"""
    out = (ctypes.c_uint32 * 32)()
    got = h2.lib().h2hip_debug_msm_reduce_plan(ctypes.c_size_t(n), ctypes.c_uint32(fuse), ctypes.c_uint32(table_c), out, ctypes.c_size_t(32))
    assert 14 <= got <= 32, got
    keys = ("n_sets", "cb", "levels", "s", "rb", "s2", "s3", "split_log", "heavy_t", "tail", "c", "W", "chunk")
    geo = {k: int(out[i]) for i, k in enumerate(keys)}
    geo["tail"] = TAILS[geo["tail"]]
    geo["g_log"] = [int(out[14 + i]) for i in range(int(out[13]))]
    assert got == 14 + len(geo["g_log"])
    geo["fixed"] = table_c != 0
    geo["fuse"] = fuse
    geo["q"] = 255 - geo["W"] * (geo["c"] - 1)
    widths = [geo["c"] if w < geo["q"] else geo["c"] - 1 for w in range(geo["W"])]
    geo["pos"] = [sum(widths[:w]) for w in range(geo["W"])]
    return geo


KNOBS = {  # name -> (setter, ctype, the value that restores the default)
    "quad_tail": ("h2hip_debug_set_msm_quad_tail", ctypes.c_int, 1),
    "plane_tail": ("h2hip_debug_set_msm_plane_tail", ctypes.c_int, 1),
    "rowcol": ("h2hip_debug_set_msm_rowcol", ctypes.c_uint64, 0),
    "heavy_div": ("h2hip_debug_set_msm_heavy_div", ctypes.c_size_t, 0),
    "split": ("h2hip_debug_set_msm_split_buckets", ctypes.c_int, 1),
    "window": ("h2hip_set_msm_window", ctypes.c_uint32, 0),
}


def set_knobs(h2, **knobs):
    for name, value in knobs.items():
        fn, ct, _ = KNOBS[name]
        assert getattr(h2.lib(), fn)(ct(value)) == 0, name


def reset_knobs(h2):
    set_knobs(h2, **{name: default for name, (_, _, default) in KNOBS.items()})


# ------------------------------------------------------------------------------------------------- points and scalars
def _norm(a):
    """a multiple of G as a signed integer of least magnitude (the key of the point table)"""
    a %= R
    return a - R if a > R // 2 else a


class Points:
    """[a]G for the multiples a case uses: one oracle.g1_mul per magnitude, the negative by negating y; at most 256 distinct points a case"""

    def __init__(self, oracle):
        self.oracle = oracle
        self.g = np.concatenate([oracle.fe_from_int(oracle.FQ, 1), oracle.fe_from_int(oracle.FQ, 2)])
        self.table = {0: np.zeros(8, dtype=np.uint64)}

    def point(self, a):
        a = _norm(a)
        if a not in self.table:
            o = self.oracle
            p = o.g1_to_affine(o.g1_mul(self.g, o.fe_from_int(o.FR, abs(a))))
            neg = p.copy()
            neg[4:] = o.fe_binop("sub", o.FQ, np.zeros((1, 4), dtype=np.uint64), p[4:].reshape(1, 4))[0]
            self.table[abs(a)], self.table[-abs(a)] = p, neg
        return self.table[a]

    def bases(self, multiples):
        """uint64[n, 8] for a list of multiples: the distinct points once, tiled with numpy"""
        keys = [_norm(a) for a in multiples]
        distinct = sorted(set(keys))
        assert len(distinct) <= 256, len(distinct)
        small = np.stack([self.point(a) for a in distinct])
        index = {a: i for i, a in enumerate(distinct)}
        return np.ascontiguousarray(small[np.fromiter((index[a] for a in keys), dtype=np.int64, count=len(keys))])

    def expected(self, total):
        """affine [total mod r]G"""
        o = self.oracle
        return o.g1_to_affine(o.g1_mul(self.g, o.fe_from_int(o.FR, total % R)))


def scalars(ints):
    """uint64[n, 4] Montgomery form of integers (plain Python: 2^19 of them take about a second)"""
    buf = b"".join(((int(v) % R) * _MONT % R).to_bytes(32, "little") for v in ints)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


@functools.lru_cache(maxsize=2)
def counting_scalars(n):
    return scalars(range(1, n + 1))


def integer_sum(pairs):
    return sum(s * a for s, a in pairs) % R


def pad(pairs, n):
    """n pairs: the given ones, then zero scalars on G (no digit, no entry)"""
    assert len(pairs) <= n, (len(pairs), n)
    return list(pairs) + [(0, 1)] * (n - len(pairs))


# ------------------------------------------------------------------------------------------------- bucket contents
def pairs_of(m, geo, window=0):
    """pairs that make B_b = [m[b]]G in window `window` (the fixed-base form scales by 2^pos there: use window 0); m: {bucket: multiple}"""
    width = geo["c"] if window < geo["q"] else geo["c"] - 1
    out = []
    for b, a in sorted(m.items()):
        assert 0 <= b < (1 << (width - 1)), (b, width)
        if a % R:
            out.append(((b + 1) << geo["pos"][window], a))
    return out


def _all(geo, f):
    s = geo["s"]
    return {b: f(b, b >> s, b & ((1 << s) - 1)) for b in range(1 << geo["cb"])}


def uniform(geo):
    return _all(geo, lambda b, hi, lo: 1)


def alternate(geo):
    return _all(geo, lambda b, hi, lo: -1 if b & 1 else 1)


def row_alternate(geo):
    return _all(geo, lambda b, hi, lo: -1 if hi & 1 else 1)


def halves(geo):
    half = 1 << (geo["cb"] - 1)
    return _all(geo, lambda b, hi, lo: 1 if b < half else -1)


def single(geo, slot, a=5):
    return {slot: a}


def row_constant(geo):
    """m = f(lo): every row sum is the same point"""
    return _all(geo, lambda b, hi, lo: lo % 251 + 1)


def column_constant(geo):
    """m = g(hi): every column sum is the same point"""
    return _all(geo, lambda b, hi, lo: hi % 251 + 1)


def inverse_weights(geo, M=7, signed=False):
    """every weighted term of one final array equals [M]G (signed: [-M]G in the array's upper half, which the final trees of both tails
    fold onto the lower half).  Levels 0: the buckets themselves, weights b + 1.  Levels 1: the row sums, weights hi << s, through
    column 0.  Levels 2: the array RC (weights l2 << s) through rows l2 < 2^s2.  (Element 0 of a row-sum array weighs nothing.)"""
    if geo["levels"] == 0:
        half = 1 << (geo["cb"] - 1)
        return {b: (-1 if signed and b & half else 1) * M * pow(b + 1, -1, R) % R for b in range(2 * half)}
    s = geo["s"]
    rows = 1 << (geo["rb"] if geo["levels"] == 1 else geo["s2"])
    return {hi << s: (-1 if signed and hi & (rows >> 1) else 1) * M * pow(hi << s, -1, R) % R for hi in range(1, rows)}


def chain_powers(geo, kind=0):
    """along the terms one lane of the first pass chains (stride 2^g_log: the row job's for kind 0, the column job's for kind 1) the
    multiples 1, 1, 2, 4, 8, ...: every step after the first is a doubling"""
    g = geo["g_log"][kind]
    if kind == 0:
        return _all(geo, lambda b, hi, lo: pow(2, max((lo >> g) - 1, 0), R))
    return _all(geo, lambda b, hi, lo: pow(2, max((hi >> g) - 1, 0), R))


def plane_partials(geo):
    """column sums placed so that the partials of the C planes with several workgroups (s >= 9) meet as identity-left, cancel and generic"""
    s = geo["s"]
    assert s >= 10
    top = 1 << (s - 1)
    m = {top - 1 + 128 * p: a for p, a in enumerate((0, 3, 5, -3)) if a}
    m[(top >> 1) - 1] = 7
    m[(top >> 1) + 127] = 11
    return m


def bucket_entries(geo, slot, multiples):
    """pairs that put the given multiples, in this order of pair indices, into bucket `slot` of window 0"""
    return [(slot + 1, a) for a in multiples]


# ------------------------------------------------------------------------------------------------- the model
class Events:
    def __init__(self):
        self.n = {st: [0] * 6 for st in STAGES}

    def add(self, stage, a, b):
        if a == 0:
            k = BOTH if b == 0 else ID_L
        elif b == 0:
            k = ID_R
        elif a == b:
            k = DBL
        elif a + b == R:
            k = CANCEL
        else:
            k = GEN
        self.n[stage][k] += 1
        t = a + b
        return t - R if t >= R else t

    def bulk(self, stage, cls, count):
        self.n[stage][cls] += count

    def merge(self, other, times=1):
        for st in STAGES:
            for k in range(6):
                self.n[st][k] += other.n[st][k] * times

    def count(self, stage, cls):
        return self.n[stage][CLASSES.index(cls)]

    def cells(self):
        return {(st, CLASSES[k]) for st in STAGES for k in range(6) if self.n[st][k]}

    def table(self):
        lines = ["%-18s" % "" + "".join("%16s" % c for c in CLASSES)]
        for st in STAGES:
            lines.append("%-18s" % st + "".join("%16d" % v for v in self.n[st]))
        return "\n".join(lines)


def digits(sc, geo):
    """for_each_digit (msm.hip): (window, |digit| - 1, negative) of every non-zero signed digit of a canonical scalar"""
    c, q, W = geo["c"], geo["q"], geo["W"]
    if sc <= (1 << (c - 1)):  # one digit in window 0 (q >= 1: window 0 is c bits wide)
        return [(0, sc - 1, 0)] if sc else []
    out, carry = [], 0
    for w in range(W):
        width = c if w < q else c - 1
        d = (sc & ((1 << width) - 1)) + carry
        sc >>= width
        carry = neg = 0
        if d > (1 << (width - 1)):
            d, neg, carry = (1 << width) - d, 1, 1
        if d:
            out.append((w, d - 1, neg))
    assert sc == 0 and carry == 0
    return out


def _tree(ev, stage, vals):
    """sh[a] += sh[a + stride] for a < stride, stride = len / 2 .. 1 (block_tree_sum, block_tree_sum_q and the quad kernels' trees)"""
    stride = len(vals) >> 1
    while stride >= 1:
        if not any(vals[:2 * stride]):
            ev.bulk(stage, BOTH, stride)
        else:
            for a in range(stride):
                vals[a] = ev.add(stage, vals[a], vals[a + stride])
        stride >>= 1
    return vals[0]


class Model:
    """one run of stage C (and of the part of stage B that adds bucket sums: the heavy role and msm_combine_kernel) on integers"""

    def __init__(self, geo):
        self.geo = geo
        self.ev = Events()
        self.parts = None  # streamed runs: what the earlier chunks left, {(set, bucket): [parts]}
        self._empty = None
        self._memo = {}

    # -- stage B as far as it adds sums ------------------------------------------------------------------------------
    def entries(self, msms):
        """{(set, bucket): [multiples in index order]} of a run: msms = one list of (scalar, a) pairs per fused MSM"""
        geo, out = self.geo, {}
        assert len(msms) == geo["fuse"]
        for y, pairs in enumerate(msms):
            for sc, a in pairs:
                for w, slot, neg in digits(sc % R, geo):
                    v = (-a if neg else a) % R
                    if geo["fixed"]:
                        key, v = (y, slot), (v << geo["pos"][w]) % R
                    else:
                        key = (y * geo["W"] + w, slot)
                    out.setdefault(key, []).append(v)
        return out

    def _heavy(self, lst):
        ev, chunk = self.ev, self.geo["chunk"]
        sums = []
        for o in range(0, len(lst), chunk):
            part = lst[o:o + chunk]
            lanes = [0] * 256
            for t in range(min(256, len(part))):
                acc = 0
                for v in part[t::256]:
                    acc = ev.add("heavy chain", acc, v)
                lanes[t] = acc
            sums.append(_tree(ev, "heavy tree", lanes))
        lanes = [0] * 256
        for q in range(min(256, len(sums))):
            acc = 0
            for v in sums[q::256]:
                acc = ev.add("heavy chunk sums", acc, v)
            lanes[q] = acc
        return _tree(ev, "heavy chunk sums", lanes)

    def fill(self, entries, heavy_t=None, last=True):
        """bucket sums of every set, [n_sets][NB]; the heavy role and the combine are classified.  A streamed run calls this once per
        chunk (last = False keeps the parts for the next chunk: cont = 1) with that chunk's heavy_t."""
        geo, ev = self.geo, self.ev
        S, nb = 1 << geo["split_log"], 1 << geo["cb"]
        heavy_t = geo["heavy_t"] if heavy_t is None else heavy_t
        cont = self.parts is not None
        parts = self.parts if cont else {}
        for key, lst in entries.items():
            if S == 1 and not cont and len(lst) == 1:
                parts[key] = lst
                continue
            cur = parts.get(key, [0] * S)
            if len(lst) > heavy_t:
                tot = self._heavy(lst)
                cur[0] = ev.add("heavy chunk sums", cur[0], tot) if cont else tot  # the heavy total onto the part an earlier chunk left
            else:
                for sub in range(S):
                    cur[sub] = (cur[sub] + sum(lst[sub::S])) % R
            parts[key] = cur
        self.parts = parts
        if not last:
            return None
        sets = [[0] * nb for _ in range(geo["n_sets"])]
        n_combine = 0
        memo = {}
        for (st, b), cur in parts.items():
            if S == 1:
                sets[st][b] = cur[0]
                continue
            n_combine += 1  # msm_combine_kernel: lane j adds parts 2j and 2j + 1, the pair sums then meet in a tree
            hit = memo.get(tuple(cur))
            if hit is None:
                was = list(ev.n["combine"])
                tot = _tree(ev, "combine", [ev.add("combine", cur[2 * j], cur[2 * j + 1]) for j in range(S >> 1)])
                hit = memo[tuple(cur)] = (tot, [a - b for a, b in zip(ev.n["combine"], was)])
            else:
                for k, d in enumerate(hit[1]):
                    ev.n["combine"][k] += d
            sets[st][b] = hit[0]
        if S > 1:
            ev.bulk("combine", BOTH, (geo["n_sets"] * nb - n_combine) * (S - 1))
        return sets

    # -- stage C ------------------------------------------------------------------------------------------------------------
    def _sums(self, stages, X, n_sums, n_terms, first, step, g_log):
        """one row/column job: sum j of n_terms terms X[first(j) + i * step]; 2^g_log lanes chain every 2^g_log-th term, then a tree"""
        ev, G = self.ev, 1 << g_log
        out = [0] * n_sums
        for j in range(n_sums):
            f = first(j)
            terms = X[f:f + n_terms * step:step]
            if not any(terms):
                ev.bulk(stages[0], BOTH, n_terms)
                ev.bulk(stages[1], BOTH, G - 1)
                continue
            key = (stages[0], g_log, tuple(terms))  # patterned contents repeat their rows: every distinct one is walked once
            hit = self._memo.get(key)
            if hit is None:
                before = [list(ev.n[st]) for st in stages]
                lanes = [0] * G
                for g in range(G):
                    acc = 0
                    for v in terms[g::G]:
                        acc = ev.add(stages[0], acc, v)
                    lanes[g] = acc
                out[j] = _tree(ev, stages[1], lanes)
                self._memo[key] = (out[j], [[a - b for a, b in zip(ev.n[st], was)] for st, was in zip(stages, before)])
                continue
            out[j] = hit[0]
            for st, delta in zip(stages, hit[1]):
                for k, d in enumerate(delta):
                    ev.n[st][k] += d
        return out

    def rowcol(self, stages, X, log_rows, log_cols, g_rows, g_cols):
        rows, cols = 1 << log_rows, 1 << log_cols
        Rs = self._sums(stages, X, rows, cols, lambda h: h * cols, 1, g_rows)
        Cs = self._sums(stages, X, cols, rows, lambda l: l, cols, g_cols)
        return Rs, Cs

    def planes(self, X, log_len, o):
        """msm_planes_kernel on one array: the plain sum of the elements whose weight i + o has bit j set, for every j"""
        ev = self.ev
        n_planes = log_len + o
        wgs = 1 << (log_len - 8) if log_len > 7 else 1
        out = []
        for plane in range(n_planes):
            top = plane == log_len
            count = 1 if top else 1 << (log_len - 1)

            def elem(t):
                if t >= count:
                    return 0
                v = (1 << log_len) if top else ((t >> plane) << (plane + 1)) | (1 << plane) | (t & ((1 << plane) - 1))
                return X[v - o]

            partials = []
            for part in range(wgs):
                sh = [ev.add("plane leaf", elem(part * 128 + 2 * q), elem(part * 128 + 2 * q + 1)) for q in range(64)]
                partials.append(_tree(ev, "plane tree", sh))
            out.append(partials[0] if wgs == 1 else _tree(ev, "plane partials", partials + [0] * (16 - wgs)))
        return out

    def final(self, arrs):
        """msm_final_quad_kernel / msm_final_kernel: arrs = [(values, o, k)], element v weighs (v + o) << k"""
        ev, scaled = self.ev, []
        for vals, o, k in arrs:
            nbits = (((len(vals) - 1 + o) << k)).bit_length()
            col = []
            for v, p in enumerate(vals):
                wgt, acc = (v + o) << k, 0
                for i in range(nbits - 1, -1, -1):
                    acc = 2 * acc % R
                    if (wgt >> i) & 1:
                        acc = ev.add("final scale", acc, p)
                col.append(acc)
            scaled.append(col)
        if self.geo["tail"] == "quad":
            flat = [x for col in scaled for x in col]
            n_groups = (len(flat) + 15) // 16
            assert n_groups <= 16
            flat += [0] * (n_groups * 16 - len(flat))
            partials = [_tree(ev, "final tree", flat[16 * g:16 * g + 16]) for g in range(n_groups)]
            return partials[0] if n_groups == 1 else _tree(ev, "final tree", partials + [0] * (16 - n_groups))
        sh = [0] * 256
        for ai, col in enumerate(scaled):
            assert len(col) <= 64
            sh[64 * ai:64 * ai + len(col)] = col
        return _tree(ev, "final tree", sh)

    def reduce_set(self, B):
        geo = self.geo
        cb, s, rb, s2, s3, g = geo["cb"], geo["s"], geo["rb"], geo["s2"], geo["s3"], geo["g_log"]
        if geo["levels"] == 0:
            return self.final([(B, 1, 0)])
        RA, CA = self.rowcol(("pass-1 chain", "pass-1 tree"), B, rb, s, g[0], g[1])
        if geo["tail"] == "planes":
            cp, rp = self.planes(CA, s, 1), self.planes(RA, rb, 0)
            return (sum(v << j for j, v in enumerate(cp)) + sum(v << (s + j) for j, v in enumerate(rp))) % R  # the host's Horner
        if geo["levels"] == 1:
            return self.final([(RA, 0, s), (CA, 1, 0)])
        RR, RC = self.rowcol(("pass-2 chain", "pass-2 tree"), RA, rb - s2, s2, g[2], g[3])
        CR, CC = self.rowcol(("pass-2 chain", "pass-2 tree"), CA, s - s3, s3, g[4], g[5])
        return self.final([(RR, 0, s + s2), (RC, 0, s), (CR, 0, s3), (CC, 1, 0)])

    def reduce(self, sets):
        """the run's MSM results (integers): every set reduced, the plain form's windows combined as the host does"""
        geo, sums = self.geo, []
        for B in sets:
            if any(B):
                sums.append(self.reduce_set(B))
                continue
            if self._empty is None:  # an empty set takes the same additions every time: count them once
                keep, self.ev = self.ev, Events()
                assert self.reduce_set(B) == 0
                self._empty, self.ev = self.ev, keep
            self.ev.merge(self._empty)
            sums.append(0)
        if geo["fixed"]:
            return sums
        W = geo["W"]
        return [sum(sums[y * W + w] << geo["pos"][w] for w in range(W)) % R for y in range(geo["fuse"])]

    def run(self, msms):
        return self.reduce(self.fill(self.entries(msms)))


# ------------------------------------------------------------------------------------------------- the corpus
class Case:
    """one run: `make(geo)` gives the pairs of each of its `fuse` MSMs (padded to n by the runner); `group` is the id of the GPU test's
    parameter it runs under and names the form, the window width, the level count and the tail the hook must report"""

    def __init__(self, group, name, form, c, n, make, tail, levels, knobs=None, fuse=1, named=None, stream=None, records=(0,), oracle_too=True,
                 chunks=None, counting=False):
        self.group, self.name, self.id = group, name, group + "-" + name
        self.form, self.c, self.n, self.make, self.tail, self.levels = form, c, n, make, tail, levels
        self.knobs, self.fuse, self.named, self.stream, self.records = dict(knobs or {}), fuse, named, stream, records
        self.oracle_too = oracle_too and n <= (1 << 17)
        self.chunks = chunks  # streamed: the pair counts of the chunks
        self.counting = counting  # the scalars are 1, 2, ..., n (every bucket of window 0 once): counting_scalars

    def plan(self, h2):
        """set the case's knobs and ask the hook (the caller resets the knobs)"""
        set_knobs(h2, window=self.c, **self.knobs)
        geo = reduce_plan(h2, self.n, self.fuse, self.c if self.form == "fixed" else 0)
        assert geo["c"] == self.c, (self.id, geo["c"])
        return geo

    def msms(self, geo):
        """the pairs of every MSM of the run, n each.  The MSMs of a fused batch share their bases: MSM y's pairs keep their places in the
        concatenation of all of them and carry zero scalars on the others' bases."""
        made = self.make(geo)
        assert len(made) == self.fuse
        if self.fuse == 1:
            return [pad(made[0], self.n)]
        return [pad([(s if z == y else 0, a) for z, p in enumerate(made) for s, a in p], self.n) for y in range(self.fuse)]


def _any(*cells):
    return [tuple(cells)]


def named_cells(name, geo):
    """what a content is named for, under this geometry: a list of groups of (stage, class) cells, one cell of every group must be hit"""
    L, tail = geo["levels"], geo["tail"]
    p1 = lambda k: (("pass-1 chain", k), ("pass-1 tree", k))
    after = lambda k: ((("plane leaf", k), ("plane tree", k)) if tail == "planes" else
                       (("pass-2 chain", k), ("pass-2 tree", k)) if L == 2 else (("final scale", k), ("final tree", k)))
    if name == "uniform" and L:
        return ([(("pass-1 chain", "doubling"),)] + ([after("doubling")] if L == 2 or tail == "planes" else []) +
                ([(("pass-1 tree", "doubling"),)] if max(geo["g_log"][:2]) else []))
    if name == "alternate" and L:
        return [p1("cancel"), after("both-identity")]
    if name == "row_alternate":
        return [p1("cancel"), p1("doubling"), after("both-identity")]
    if name == "halves" and L:
        return [p1("cancel")]
    if name.startswith("single"):
        return [(("plane leaf", "identity-left"), ("plane leaf", "identity-right"), ("final tree", "identity-left"), ("final tree", "identity-right"))]
    if name in ("row_constant", "column_constant") and (L == 2 or tail == "planes"):
        return [after("doubling")]
    if name == "inverse_weights" and tail != "planes":
        return [(("final tree", "doubling"),)]
    if name == "inverse_weights_signed" and tail != "planes":
        return [(("final tree", "cancel"),)]
    if name.startswith("chain_powers"):
        return [(("pass-1 chain", "doubling"),)]
    return []


def _simple(content):
    return lambda geo: [pairs_of(content(geo), geo)]


def _contents(levels):
    out = [("uniform", uniform), ("alternate", alternate), ("halves", halves), ("inverse_weights", inverse_weights),
           ("inverse_weights_signed", lambda g: inverse_weights(g, signed=True)),
           ("single_first", lambda g: single(g, 0)), ("single_row_end", lambda g: single(g, (1 << g["s"]) - 1)),
           ("single_row_start", lambda g: single(g, (1 << g["s"]) % (1 << g["cb"]))), ("single_last", lambda g: single(g, (1 << g["cb"]) - 1))]
    if levels:
        out += [("row_alternate", row_alternate), ("row_constant", row_constant), ("column_constant", column_constant),
                ("chain_powers_rows", lambda g: chain_powers(g, 0)), ("chain_powers_columns", lambda g: chain_powers(g, 1))]
    return out


def _windows(geo, ms):
    """one MSM of the plain form whose windows 0, 1, ... hold different contents"""
    return [p for w, m in enumerate(ms) for p in pairs_of(m, geo, w)]


LEVELS = {3: 0, 5: 0, 7: 0, 9: 1, 13: 1, 14: 2, 17: 2, 20: 2}  # msm_layout: cb <= 6: 0, <= 12: 1, else 2 (at c = 20 the planes replace the second pass)
NO_STREAM = (1, 0, 0)
BIG_DIV = 1 << 30  # heavy_div: the threshold falls to its floor (32 entries, or 8 x the mean bucket)


def corpus():
    cases = []

    def group_id(form, c, tail, extra=""):
        return "%s-c%d-L%d-%s%s" % (form, c, LEVELS[c], tail, extra)

    def add_contents(form, c, tail, knobs, n=None, contents=None, extra="", **kw):
        g = group_id(form, c, tail, extra)
        for name, fn in contents or _contents(LEVELS[c]):
            cases.append(Case(g, name, form, c, n or 1 << (c - 1), _simple(fn), tail, LEVELS[c], knobs, named=name, **kw))

    # -- a lone MSM, every level count and every tail; the whole list of contents at the smaller width of every level count
    short = lambda c: [(k, f) for k, f in _contents(LEVELS[c]) if k in ("uniform", "alternate", "row_alternate", "halves", "single_last", "row_constant",
                                                                         "inverse_weights", "inverse_weights_signed")]
    for c in (5, 7, 9, 13, 14, 17):
        add_contents("plain", c, "quad", {}, contents=short(c) if c in (7, 13, 17) else None)
    for c in (5, 9, 14):
        add_contents("plain", c, "lane", {"quad_tail": 0})
    for c in (9, 13, 14, 17):
        add_contents("fixed", c, "planes", {}, contents=short(c) if c in (13, 17) else None)
    for c in (9, 14):
        add_contents("fixed", c, "quad", {"plane_tail": 0})
        add_contents("fixed", c, "lane", {"quad_tail": 0})
    # -- lane budgets of the first pass: one lane chains a whole row (g_log = 0); the deepest tree is the default's at c = 13
    budget = [("uniform", uniform), ("alternate", alternate), ("row_alternate", row_alternate), ("chain_powers_rows", lambda g: chain_powers(g, 0)),
              ("chain_powers_columns", lambda g: chain_powers(g, 1)), ("column_constant", column_constant)]
    add_contents("fixed", 13, "planes", {"rowcol": 1}, contents=budget, extra="-rowcol1")
    add_contents("plain", 14, "quad", {"rowcol": 1}, contents=budget, extra="-rowcol1")
    # -- c = 20: 2^19 buckets, the planes of 2^10 column sums and 2^9 row sums take 4 and 2 workgroups each (arrival counter, partials tree)
    sparse = [("single_first", lambda g: single(g, 0)), ("single_row_end", lambda g: single(g, (1 << g["s"]) - 1)),
              ("single_row_start", lambda g: single(g, 1 << g["s"])), ("single_last", lambda g: single(g, (1 << g["cb"]) - 1)),
              ("plane_partials", plane_partials), ("inverse_weights", inverse_weights)]
    add_contents("fixed", 20, "planes", {}, n=256, contents=sparse, extra="-sparse")
    dense = [("uniform", uniform), ("alternate", alternate), ("row_alternate", row_alternate)]
    for k in range(3):  # (a group each: 2^19 pairs take Python seconds to lay out)
        add_contents("fixed", 20, "planes", {}, contents=dense[k:k + 1], extra="-dense%d" % k, stream=NO_STREAM, counting=True)
    add_contents("fixed", 20, "planes", {"rowcol": 1}, contents=dense[:1], extra="-dense-rowcol1", stream=NO_STREAM, counting=True)
    add_contents("fixed", 20, "planes", {"rowcol": 1 << 30}, contents=dense[:1], extra="-dense-rowcolmax", stream=NO_STREAM, counting=True)
    # -- several sets with different contents: a wrong set index shows
    for c in (9, 14):
        cases.append(Case(group_id("plain", c, "quad", "-windows"), "differ", "plain", c, 3 << (c - 1),
                          lambda g: [_windows(g, [uniform(g), row_alternate(g), column_constant(g)])], "quad", LEVELS[c]))
    cases.append(Case(group_id("plain", 3, "lane", "-windows"), "differ", "plain", 3, 16,
                      lambda g: [_windows(g, [uniform(g), alternate(g), inverse_weights(g), inverse_weights(g, signed=True)])], "lane", 0))
    five = [uniform, alternate, row_alternate, halves, column_constant]
    cases.append(Case(group_id("fixed", 13, "planes", "-fused2"), "differ", "fixed", 13, 2 << 12,
                      lambda g: [pairs_of(uniform(g), g), pairs_of(alternate(g), g)], "planes", 1, fuse=2))
    cases.append(Case(group_id("fixed", 13, "quad", "-fused5"), "differ", "fixed", 13, 5 << 12,
                      lambda g: [pairs_of(f(g), g) for f in five], "quad", 1, fuse=5))
    for c in (13, 14):  # 5 x W > 64 sets: the lane tail by default
        cases.append(Case(group_id("plain", c, "lane", "-fused5"), "differ", "plain", c, 10 << (c - 1),
                          lambda g: [_windows(g, [five[y](g), five[(y + 1) % 5](g)]) for y in range(5)], "lane", LEVELS[c], fuse=5))
    # -- one over-full bucket (the heavy role) and split buckets (msm_combine_kernel); plain, E-form table and native table
    slot = 37
    heavy = [("heavy_uniform", [3] * 3072), ("heavy_uniform_ragged", [3] * 2500), ("heavy_alternate", [3, -3] * 1024),
             ("heavy_chunks_cancel", [3] * 1024 + [-3] * 1024),
             ("heavy_identities", [0 if (i >> 8) & 1 == 0 else 3 for i in range(2048)] + [3] * 100),  # identity points among the bases
             ("heavy_lanes_cancel", ([3] * 256 + [-3] * 128 + [3] * 128) * 4)]  # lanes below 128 chain P - P + P - P, the others P + P + P + P
    parts = [("parts_equal", lambda S: {slot: [3] * (2 * S)}), ("parts_cancel", lambda S: {slot: [3, -3] * S}),
             ("parts_mixed", lambda S: {slot: [3], slot + 1: [3, 5] + [0] * (S - 2) + [-3], slot + 2: [3, 6]})]
    for form, c, n, tail, records in (("plain", 13, 1 << 12, "quad", (0,)), ("fixed", 13, 1 << 12, "planes", (64, 128))):
        g = group_id(form, c, tail, "-heavy")
        for name, lst in heavy:
            cases.append(Case(g, name, form, c, n, lambda geo, lst=lst: [bucket_entries(geo, slot, lst)], tail, 1, {"heavy_div": BIG_DIV},
                              records=records, named=name))
    for form, c, n, tail, records in (("plain", 9, 1 << 10, "quad", (0,)), ("plain", 9, 1 << 12, "quad", (0,)), ("fixed", 13, 1 << 12, "planes", (64, 128))):
        g = group_id(form, c, tail, "-parts-n%d" % n)
        for name, fn in parts:
            cases.append(Case(g, name, form, c, n, lambda geo, fn=fn: [[p for b, lst in fn(1 << geo["split_log"]).items() for p in bucket_entries(geo, b, lst)]],
                              tail, 1, records=records, named=name))
    # -- streamed, cont = 1: the first chunk leaves [T a]G in the bucket's first part, the second brings T entries [a]G: the heavy total is
    # added onto an equal part
    T = 2048
    cases.append(Case(group_id("fixed", 13, "planes", "-streamed"), "heavy_onto_equal_part", "fixed", 13, 1 << 14,
                      lambda geo: [pad([(slot + 1, 3 * T)], 1 << 13) + [(slot + 1, 3)] * T], "planes", 1, stream=(2, 1000, 1024), records=(64, 128),
                      named="heavy_onto_equal_part", chunks=[1 << 13, 1 << 13]))
    assert len({c.id for c in cases}) == len(cases)
    return cases


SPECIAL_NAMED = {
    "heavy_uniform": [(("heavy chain", "doubling"),), (("heavy tree", "doubling"),), (("heavy chunk sums", "doubling"),)],
    "heavy_uniform_ragged": [(("heavy chain", "doubling"),), (("heavy chunk sums", "generic"),)],
    "heavy_lanes_cancel": [(("heavy chain", "cancel"),), (("heavy tree", "identity-left"),)],
    "heavy_alternate": [(("heavy tree", "cancel"),), (("heavy chunk sums", "both-identity"),)],
    "heavy_chunks_cancel": [(("heavy chunk sums", "cancel"),)],
    "heavy_identities": [(("heavy chain", "both-identity"),), (("heavy chain", "identity-right"),)],
    "parts_equal": [(("combine", "doubling"),)],
    "parts_cancel": [(("combine", "cancel"),)],
    "parts_mixed": [(("combine", "identity-left"),), (("combine", "identity-right"),), (("combine", "generic"),)],
    "heavy_onto_equal_part": [(("heavy chunk sums", "doubling"),)],
}


def model_run(h2, case):
    """the case through the model under its own knobs: (geo, model, results, the integer sums); the caller resets the knobs"""
    geo = case.plan(h2)
    msms = case.msms(geo)
    model = Model(geo)
    if case.chunks:  # every chunk's heavy threshold is its own (msm_stream_host: the chunks share the whole run's window and split)
        o = 0
        for k, m in enumerate(case.chunks):
            sub = reduce_plan(h2, m, 1, case.c)
            assert sub["split_log"] == geo["split_log"]
            sets = model.fill(model.entries([msms[0][o:o + m]]), heavy_t=sub["heavy_t"], last=k + 1 == len(case.chunks))
            o += m
        got = model.reduce(sets)
    else:
        got = model.run(msms)
    return geo, model, got, [integer_sum(p) for p in msms]
