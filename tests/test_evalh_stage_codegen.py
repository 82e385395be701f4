"""The kernels evaluate_h generates for the shuffle and mv-lookup stages, without a GPU: the source the generator emits for an argument's
programs (h2hip_debug_evalh_codegen_stage_source) and what hiprtc makes of it for gfx950, the generator's limits, what a stage graph may
read, and the new hooks' symbols.  The GPU side is tests/test_evalh_stage_codegen_gpu.py."""
import contextlib
import ctypes
import os
import re

import pytest

from conftest import ROOT
from evalh_util import GraphEvaluator, flatten_graph, mvlookup_graphs, shuffle_graphs
from test_mvlookup_evalh import _many_live_tuple

A = lambda c, r=0: ('advice', c, r)  # noqa: E731
F = lambda c, r=0: ('fixed', c, r)  # noqa: E731
I = lambda c, r=0: ('instance', c, r)  # noqa: E731
SHUFFLE, MVLOOKUP = 1, 2


def _bare_column_graph(e):
    """a graph whose value is the column itself: no Horner, no closing Add"""
    g = GraphEvaluator()
    g.add_expression(e)
    return g


def stage_source(h2, graphs, kind, compile=True):
    """-> (rc, source, bytes of code object) of one stage kernel from GraphEvaluators"""
    from halo2_pse_amd.evaluation import graph_array
    arr, keep = graph_array([flatten_graph(g) for g in graphs])
    L = h2.lib()
    n, code, secs = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_double()
    buf = ctypes.create_string_buffer(1 << 20)
    rc = L.h2hip_debug_evalh_codegen_stage_source(arr, ctypes.c_uint32(len(graphs)), ctypes.c_int(kind), buf, ctypes.c_size_t(len(buf)),
                                                  ctypes.byref(n), ctypes.c_int(1 if compile else 0), ctypes.byref(secs), ctypes.byref(code))
    del keep
    return rc, buf.value.decode() if rc in (0, 2) else "", code.value


@contextlib.contextmanager
def codegen(h2, mode, max_ops=0):
    L = h2.lib()
    assert L.h2hip_debug_set_evalh_codegen(ctypes.c_int(mode), ctypes.c_uint32(max_ops)) == 0
    try:
        yield
    finally:
        L.h2hip_debug_set_evalh_codegen(ctypes.c_int(1), ctypes.c_uint32(0))


THREE = ([A(2, 1), ('prod', F(0), A(3)), ('sum', I(0, -1), ('challenge', 1))], [A(4), F(1, 2), ('scaled', A(5, -2), 7)])
K4 = ([[A(1), ('prod', F(0), A(2))], [A(3, 1), I(0, -1)], [('sum', A(4), ('challenge', 1)), F(1, 2)], [A(5, -2), ('const', 7)]], [F(2), F(1, 1)])
CASES = {
    "shuffle_one_expression": (SHUFFLE, lambda: shuffle_graphs([A(0)], [A(1)])),
    "shuffle_three_expressions": (SHUFFLE, lambda: shuffle_graphs(*THREE)),
    "shuffle_empty_side": (SHUFFLE, lambda: (shuffle_graphs([A(0)], [A(1)])[0], GraphEvaluator())),
    "mvlookup_k1": (MVLOOKUP, lambda: mvlookup_graphs([[A(0)]], [F(0)])),
    "mvlookup_k4": (MVLOOKUP, lambda: mvlookup_graphs(*K4)),
    "mvlookup_bare_column_table": (MVLOOKUP, lambda: (mvlookup_graphs([[A(0), A(1)]], [F(0)])[0], _bare_column_graph(F(2, 1)))),
}


@pytest.mark.parametrize("name", list(CASES))
def test_stage_source_and_code_object(h2, name):
    """every shape the stages meet compiles to a non-empty code object for gfx950; the kernel has the stage's name and signature, is one
    lane per row behind the row guard, and ends with exactly one call of the stage's row function"""
    kind, make = CASES[name]
    graphs = make()
    rc, src, code = stage_source(h2, graphs, kind)
    assert rc == 0, h2.lib().h2hip_last_error()
    assert code > 0
    row, other = ("shuffle_row(", "mvlookup_row(") if kind == SHUFFLE else ("mvlookup_row(", "shuffle_row(")
    assert src.count(row) == 1 and other not in src and "lookup_row(l," not in src
    sig = "evalh_shuffle_gen(ColsDev c, ShuffleDev sh, Fe* values)" if kind == SHUFFLE else "evalh_mvlookup_gen(ColsDev c, MvLookupDev mv, Fe* values)"
    assert sig in src
    assert "const uint32_t idx = blockIdx.x * 256u + threadIdx.x;" in src and "if (idx >= (1u << c.log_size)) return;" in src
    assert "prev" not in src
    if kind == MVLOOKUP:  # Q = Q f + P; P = P f unrolled once per input tuple, the table program last
        K = len(graphs) - 1
        assert src.count("Q = addn(mul_i(Q, f), P);") == K and src.count("P = mul_i(P, f);") == K
        assert src.rindex("P = mul_i(P, f);") < src.index("mvlookup_row(")
    else:
        assert src.count("const Fu a = ") == 1 and src.index("const Fu a = ") < src.index("shuffle_row(")
    if name == "shuffle_empty_side":
        assert "shuffle_row(sh, c, idx, a, fu_zero(), values);" in src
    if name == "mvlookup_bare_column_table":
        assert "mvlookup_row(mv, c, idx, ld_i(F2[rp1]), P, Q, values);" in src


def test_columns_and_rotations_are_shared_across_the_programs(h2):
    """A(0) and F(0) are read by every tuple of the argument, rotation 1 by two of them: one pointer per distinct column and one row
    index per distinct rotation value in the whole kernel; constants are literals per program"""
    inputs = [[A(0), ('prod', F(0), A(1, 1))], [('prod', F(0), A(0)), ('scaled', A(2, 1), 9)], [A(0, -1), ('scaled', A(3), 9)]]
    rc, src, _ = stage_source(h2, mvlookup_graphs(inputs, [F(0), F(1, 1)]), MVLOOKUP, compile=False)
    assert rc == 0
    for col in ("c.advice, 0", "c.advice, 1", "c.advice, 2", "c.advice, 3", "c.fixed, 0", "c.fixed, 1"):
        assert src.count("ld_const_col(%s)" % col) == 1, col
    assert len(re.findall(r"rot_idx\(idx, ", src)) == 3  # 0, 1 and -1
    for name, rot in (("rp0", 0), ("rp1", 1), ("rm1", -1)):
        assert src.count("const uint32_t %s = rot_idx(idx, %d, c.rot_scale, c.log_size);" % (name, rot)) == 1
    assert "const Fu K1_3 = " in src and "const Fu K2_3 = " in src  # the 9 of programs 1 and 2, each its own literal
    assert len(re.findall(r"^    Fu s0", src, flags=re.M)) == 1  # one set of slot locals for all the programs
    gi, gs = shuffle_graphs([A(0), A(1, 2)], [A(0, 2), F(0)])
    rc, src, _ = stage_source(h2, (gi, gs), SHUFFLE, compile=False)
    assert rc == 0 and src.count("ld_const_col(c.advice, 0)") == 1 and src.count("= rot_idx(idx, 2,") == 1


def test_fusion_applies_per_program_and_follows_the_switch(h2):
    graphs = shuffle_graphs([('sum', ('prod', A(0), A(1)), ('prod', A(2), F(0)))], [('sum', ('prod', A(3), A(4)), ('neg', ('prod', A(5), F(1))))])
    rc, on, _ = stage_source(h2, graphs, SHUFFLE, compile=False)
    assert rc == 0 and on.count("fu_mul_sub<UF>(") == 2
    with codegen(h2, 1 + 16):
        rc, off, _ = stage_source(h2, graphs, SHUFFLE, compile=False)
    assert rc == 0 and "fu_mul_sub<UF>(" not in off and len(re.findall(r"= mul_i\((?!s\d+, fu_one_i)", off)) == 4
    for src in (on, off):  # one scheduling barrier per emitted operation (a reduction belongs to the operation that asked for it)
        ops = len(re.findall(r"^    s\d+ = (?!mul_i\(s\d+, fu_one_i)", src, flags=re.M))
        assert src.count("__builtin_amdgcn_sched_barrier(0);") == ops


def test_beyond_the_limits_and_malformed_input(h2):
    L = h2.lib()
    three = shuffle_graphs(*THREE)
    assert stage_source(h2, three, SHUFFLE, compile=False)[0] == 0
    with codegen(h2, 1, max_ops=5):  # the two programs have more than five operations between them
        assert stage_source(h2, three, SHUFFLE, compile=False)[0] == 3
        assert b"beyond the generator's limits" in L.h2hip_last_error()
    assert stage_source(h2, three, SHUFFLE, compile=False)[0] == 0  # (1, 0) restored the default
    # 60 products alive at once in one tuple: more than 48 live values
    assert stage_source(h2, mvlookup_graphs([[A(0)], _many_live_tuple(60)], [F(0)]), MVLOOKUP, compile=False)[0] == 3
    assert stage_source(h2, shuffle_graphs([A(0)], _many_live_tuple(60)), SHUFFLE, compile=False)[0] == 3
    assert stage_source(h2, mvlookup_graphs([[A(0)], _many_live_tuple(20)], [F(0)]), MVLOOKUP, compile=False)[0] == 0
    # what no kernel of the stage supplies: y and the previous value for both, beta for a shuffle, gamma for an mv-lookup
    from shuffle_util import CALC_ADD
    for kind, make, bad in ((SHUFFLE, lambda: shuffle_graphs([A(0)], [A(1)]), (6, 9, 10)), (MVLOOKUP, lambda: mvlookup_graphs([[A(0)]], [F(0)]), (7, 9, 10))):
        for vs in bad:
            graphs = make()
            (op, x, y, parts), target = graphs[1].calculations[-1]
            assert op == CALC_ADD
            graphs[1].calculations[-1] = ((op, x, (vs, 0, 0), parts), target)
            assert stage_source(h2, graphs, kind, compile=False)[0] == 1, (kind, vs)
    # kinds and counts
    assert stage_source(h2, three, 0, compile=False)[0] == 1 and stage_source(h2, three, 3, compile=False)[0] == 1
    assert stage_source(h2, three + three[:1], SHUFFLE, compile=False)[0] == 1
    assert stage_source(h2, three[:1], MVLOOKUP, compile=False)[0] == 1
    n = ctypes.c_size_t()
    assert L.h2hip_debug_evalh_codegen_stage_source(None, 2, 1, None, 0, ctypes.byref(n), 0, None, None) == 1


def test_new_hooks_are_exported_with_the_headers_arity(h2):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "halo2hip_debug.h")).read(), flags=re.S)
    for name, count in {"h2hip_debug_evalh_codegen_stage_stats": 1, "h2hip_debug_evalh_codegen_stage_source": 9, "h2hip_debug_evalh_codegen_stats": 1,
                        "h2hip_debug_set_evalh_codegen": 2}.items():
        assert hasattr(h2.lib(), name), name
        args = re.search(r"\bint %s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S).group(1)
        assert len(args.split(",")) == count, name
    out = (ctypes.c_uint64 * 9)(*([7] * 9))
    assert h2.lib().h2hip_debug_evalh_codegen_stage_stats(out) == 0 and out[8] <= 8  # the bound on queued background compilations
    assert h2.lib().h2hip_debug_evalh_codegen_stage_stats(None) != 0
    public = open(os.path.join(ROOT, "include", "halo2hip.h")).read()
    assert "stage_source" not in public and "stage_stats" not in public
