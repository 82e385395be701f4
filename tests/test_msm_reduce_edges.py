"""The MSM's bucket reduction (stage C of csrc/msm.hip, with the heavy role and msm_combine_kernel of stage B) on bucket sums chosen by the
test: equal, opposite and identity operands in every kernel of every tail, where random inputs meet them with probability 2^-254.

msm_reduce_util.py crafts the inputs (every base a known multiple of the generator, every scalar one signed digit) and restates the
reduction on integers.  The tests without the gpu mark prove on that model that every case does what its name says, that the corpus
reaches every reachable (stage, class) cell of the event table, and -- through h2hip_debug_msm_reduce_plan -- that every GPU case takes
the tail and the level count its id names under the defaults in force.  The gpu tests run the same cases bit-exact against
[sum s_i a_i mod r]G (Python integers and one oracle.g1_mul) and, up to 2^17 pairs, against oracle.best_multiexp as well.

Ids: <form>-c<width>-L<levels>-<tail>[-variant].  `levels` is msm_layout's count; at c = 20 it is 2 although only the first pass runs,
because the bit planes replace the second one.

The event table and the module's wall time on an MI355X are in DESIGN.md, section 5 ("Crafted bucket sums").  Run the gpu part with
`pytest -m gpu`."""
import ctypes
import os
import re

import numpy as np
import pytest

import msm_reduce_util as U

NT = min(16, os.cpu_count() or 1)
CORPUS = U.corpus()
GROUPS = sorted({c.group for c in CORPUS})

# Cells no input can reach, with the reason.  xyzzu_mul_small[_q] adds p onto acc = 2 j p (j >= 1) or onto the identity: for p != 0 the sum
# meets neither p itself ((2 j - 1) p = 0) nor -p ((2 j + 1) p = 0), r being prime and 2 j + 1 < r, and acc != 0; for p = 0 both are 0.
UNREACHABLE = {
    ("final scale", "doubling"): "acc = 2 j p equals p only if (2 j - 1) p = 0",
    ("final scale", "cancel"): "acc = 2 j p equals -p only if (2 j + 1) p = 0",
    ("final scale", "identity-right"): "p is the identity only where acc, a multiple of p, is as well",
}


def set_stream(h2, chunks=0, permille=0, min_n=0):
    assert h2.lib().h2hip_debug_set_msm_stream(ctypes.c_uint32(chunks), ctypes.c_uint32(permille), ctypes.c_size_t(min_n)) == 0


def set_records(h2, nbytes):
    assert h2.lib().h2hip_debug_set_table_records(ctypes.c_uint32(nbytes)) == 0


def reset(h2):
    U.reset_knobs(h2)
    set_stream(h2)
    set_records(h2, 0)


@pytest.fixture(autouse=True)
def _knobs(h2):
    yield
    reset(h2)


def named(case, geo):
    return U.SPECIAL_NAMED.get(case.named) or (U.named_cells(case.named, geo) if case.named else [])


@pytest.fixture(scope="module")
def modelled(h2):
    """every case of the corpus through the integer model, once: id -> (case, geo, events, results, integer sums)"""
    out = {}
    for case in CORPUS:
        try:
            if case.stream:
                set_stream(h2, *case.stream)
                if case.chunks:
                    sizes = (ctypes.c_size_t * 8)()
                    k = h2.lib().h2hip_debug_msm_stream_ladder(ctypes.c_size_t(case.n), ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_int(0), sizes,
                                                               ctypes.c_size_t(8))
                    assert [int(sizes[i]) for i in range(k)] == case.chunks, case.id
            geo, model, got, want = U.model_run(h2, case)
        finally:
            reset(h2)
        out[case.id] = (case, geo, model.ev, got, want)
    return out


# ------------------------------------------------------------------------------------------------------------------ no GPU
def test_reduce_plan_hook(h2):
    """the hook itself: the geometry of msm_layout, the lengths it reports, what it refuses"""
    L = h2.lib()
    out = (ctypes.c_uint32 * 32)()
    call = lambda n, fuse, c, cap: L.h2hip_debug_msm_reduce_plan(ctypes.c_size_t(n), ctypes.c_uint32(fuse), ctypes.c_uint32(c), out, ctypes.c_size_t(cap))
    assert call(0, 1, 0, 32) == -1 and call(16, 0, 0, 32) == -1
    assert L.h2hip_debug_msm_reduce_plan(ctypes.c_size_t(16), ctypes.c_uint32(1), ctypes.c_uint32(0), None, ctypes.c_size_t(4)) == -1
    assert call(1 << 12, 1 << 20, 13, 32) == -1  # more buckets than one run sorts
    out[3] = 77
    assert call(1 << 12, 1, 13, 3) == 16 and out[3] == 77  # nothing is written beyond cap
    for c, (levels, s, rb, s2, s3) in {5: (0, 0, 4, 0, 0), 7: (0, 0, 6, 0, 0), 9: (1, 4, 4, 0, 0), 13: (1, 6, 6, 0, 0), 14: (2, 7, 6, 3, 4),
                                       17: (2, 8, 8, 4, 4), 20: (2, 10, 9, 5, 5)}.items():
        g = U.reduce_plan(h2, 1 << 10, 1, c)
        assert (g["n_sets"], g["cb"], g["levels"], g["s"], g["rb"], g["s2"], g["s3"]) == (1, c - 1, levels, s, rb, s2, s3), c
        assert g["tail"] == ("planes" if levels else "quad") and len(g["g_log"]) == (2 if levels else 0)
        if c <= 17:
            U.set_knobs(h2, window=c)
            p = U.reduce_plan(h2, 1 << 10, 1, 0)
            assert (p["n_sets"], p["c"], p["levels"], p["tail"]) == (p["W"], c, levels, "quad") and len(p["g_log"]) == 2 * levels + 2 * (levels == 2)
            if c <= 14:  # (5 x 15 sets of 2^16 buckets are more than one run sorts)
                assert U.reduce_plan(h2, 1 << 10, 5, 0)["tail"] == ("lane" if 5 * p["W"] > 64 else "quad")
    # the windows msm.hip's MsmPlan cuts 255 bits into
    g = U.reduce_plan(h2, 1 << 10, 1, 13)
    assert (g["W"], g["q"], g["pos"][:3], g["chunk"]) == (20, 15, [0, 13, 26], 1024)
    # the settings in force count: the tails, the lane budget and the heavy threshold
    U.set_knobs(h2, window=0, plane_tail=0)
    assert U.reduce_plan(h2, 1 << 10, 1, 14)["tail"] == "quad" and len(U.reduce_plan(h2, 1 << 10, 1, 14)["g_log"]) == 6
    U.set_knobs(h2, quad_tail=0)
    assert U.reduce_plan(h2, 1 << 10, 1, 14)["tail"] == "lane"
    U.set_knobs(h2, quad_tail=1, plane_tail=1, rowcol=1)
    assert U.reduce_plan(h2, 1 << 10, 1, 20)["g_log"] == [0, 0]
    U.set_knobs(h2, rowcol=1 << 30)
    assert U.reduce_plan(h2, 1 << 10, 1, 20)["g_log"] == [8, 8]
    U.set_knobs(h2, rowcol=0)
    assert U.reduce_plan(h2, 1 << 12, 1, 13)["heavy_t"] == 160 and U.reduce_plan(h2, 1 << 12, 1, 13)["split_log"] == 3
    U.set_knobs(h2, split=0)
    assert U.reduce_plan(h2, 1 << 12, 1, 13)["split_log"] == 0


def test_digits_restate_the_signed_recoding():
    """digits(): sum_w (+-)(slot + 1) 2^pos_w is the scalar again, every digit within its window's half range, on edge and random scalars"""
    rng = np.random.default_rng(0xD161)
    for c in (3, 5, 13, 14, 20):
        W = (255 + c - 1) // c
        geo = {"c": c, "W": W, "q": 255 - W * (c - 1)}
        widths = [c if w < geo["q"] else c - 1 for w in range(W)]
        pos = [sum(widths[:w]) for w in range(W)]
        vals = [0, 1, 1 << (c - 1), (1 << (c - 1)) + 1, (1 << c) - 1, U.R - 1, 1 << 253] + [int.from_bytes(rng.bytes(32), "little") % U.R for _ in range(50)]
        for v in vals:
            ds = U.digits(v, geo)
            assert sum((-1 if neg else 1) * (slot + 1) << pos[w] for w, slot, neg in ds) == v
            assert all(slot + 1 <= 1 << (widths[w] - 1) for w, slot, neg in ds)


def test_model_equals_the_integer_sum(modelled):
    """the model's result of every case is sum_i s_i a_i mod r: the pairing it mirrors loses and repeats no bucket"""
    for case, geo, ev, got, want in modelled.values():
        assert got == want, case.id
        assert len(got) == case.fuse


def test_every_case_takes_the_tail_and_the_levels_its_id_names(modelled):
    """asked through the hook under the case's own settings: a changed default fails here instead of silently testing another path"""
    for case, geo, ev, got, want in modelled.values():
        form, c, levels, tail = re.match(r"(plain|fixed)-c(\d+)-L(\d)-(lane|quad|planes)", case.id).groups()
        assert (geo["fixed"], geo["c"], geo["levels"], geo["tail"]) == (form == "fixed", int(c), int(levels), tail), case.id
        assert (case.form, case.c, case.levels, case.tail) == (form, int(c), int(levels), tail)
        assert len(geo["g_log"]) == (0 if geo["levels"] == 0 else 2 if geo["levels"] == 1 or tail == "planes" else 6), case.id
        if "rowcol1" in case.id:
            assert geo["g_log"][:2] == [0, 0], case.id  # one lane chains a whole row
        if "rowcolmax" in case.id:
            assert geo["g_log"] == [8, 8], case.id  # 256 lanes per sum: the deepest tree the kernel has
        if "-parts" in case.id:
            assert geo["split_log"] == (1 if case.n == 1 << 10 else 3), case.id
        if "-heavy" in case.id or case.chunks:
            assert ev.count("heavy chain", "identity-left") > 0, case.id  # the bucket did go to the heavy role
        if case.chunks:
            assert geo["split_log"] == 3
    tails = {(c.form, c.tail, c.fuse > 1) for c, *_ in modelled.values()}
    assert {("fixed", "planes", False), ("fixed", "planes", True), ("plain", "quad", False), ("fixed", "quad", False), ("fixed", "quad", True),
            ("plain", "lane", False), ("fixed", "lane", False), ("plain", "lane", True)} <= tails
    assert {(c.levels, c.tail) for c, *_ in modelled.values() if c.tail != "planes"} == {(lv, t) for lv in (0, 1, 2) for t in ("quad", "lane")}


def test_every_named_case_hits_its_cells(modelled):
    for case, geo, ev, got, want in modelled.values():
        for group in named(case, geo):
            assert any(ev.count(st, cls) for st, cls in group), (case.id, group)
    assert sum(1 for case, geo, *_ in modelled.values() if named(case, geo)) > len(modelled) // 2


def test_event_table_reaches_every_reachable_cell(modelled):
    total = U.Events()
    for case, geo, ev, got, want in modelled.values():
        total.merge(ev)
    print("\n" + total.table())
    cells = {(st, cls) for st in U.STAGES for cls in U.CLASSES}
    assert set(UNREACHABLE) <= cells and 4 * len(UNREACHABLE) <= len(cells)
    assert not (total.cells() & set(UNREACHABLE)), "a cell listed as unreachable was reached"
    assert cells - total.cells() == set(UNREACHABLE)


# --------------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def points(oracle):
    return U.Points(oracle)


def aff(h2, xyz):
    return h2.g1_to_affine(xyz)


def run_msms(h2, sc, bs):
    return [aff(h2, h2.best_multiexp(sc[0], bs))] if len(sc) == 1 else [aff(h2, r) for r in h2.best_multiexp_batch(sc, bs)]


def run_case(h2, oracle, points, case):
    geo = case.plan(h2)
    assert (geo["tail"], geo["levels"]) == (case.tail, case.levels), case.id
    if case.stream:
        set_stream(h2, *case.stream)
    msms = case.msms(geo)
    want = [points.expected(U.integer_sum(p)) for p in msms]
    bs = points.bases([a for _, a in msms[0]])
    if case.counting:
        assert all(s == i + 1 for i, (s, _) in enumerate(msms[0]))
        sc = [U.counting_scalars(case.n)]
    else:
        sc = [U.scalars([s for s, _ in p]) for p in msms]
    if case.oracle_too:  # the two references check each other
        for y in range(case.fuse):
            assert np.array_equal(oracle.g1_to_affine(oracle.best_multiexp(sc[y], bs, NT)), want[y]), (case.id, y, "oracle")
    for records in case.records:
        if case.form == "fixed":
            set_records(h2, records)
            h2.bases_pin(bs)
            try:
                assert h2.bases_pinned_info(bs)[:2] == (case.n, case.c) and (not records or h2.bases_pinned_info(bs)[3] == geo["W"] * case.n * records)
                got = run_msms(h2, sc, bs)
            finally:
                h2.bases_unpin(bs)
                set_records(h2, 0)
        else:
            got = run_msms(h2, sc, bs)
        for y in range(case.fuse):
            assert np.array_equal(got[y], want[y]), (case.id, y, records)
    reset(h2)


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_crafted_bucket_sums(h2, oracle, points, group):
    """every case of the group: the engine's result, limb for limb after g1_to_affine, is [sum_i s_i a_i mod r]G"""
    h2.init()
    assert oracle.g1_on_curve(points.g)
    for case in CORPUS:
        if case.group == group:
            run_case(h2, oracle, points, case)
