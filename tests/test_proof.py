"""create_proof and verify_proof end to end on the SYSTEM of check_util.py: every stage's output is the next stage's input, and the
verifier -- Python integers only -- decides.  The pairing equation e(left, s_g2) = e(right, g2) is closed with the setup secret:
s_g2 = s g2, so it holds iff s left = right (proof_util.pairing_holds, affine integer arithmetic).

k = 5 is the smallest size at which the copies' rows (up to 12) and the active rows lie below the usable rows (2^5 - 6 = 26); k = 10 is
the size at which a column is 32 KiB, more than a proof and everything else that crosses, so the residency bound can be derived."""
import random

import numpy as np
import pytest

import check_util as cu
import proof_util as pu
from lookup_util import R_MOD, to_mont
from proof_util import h2, prover, transcript, verifier

_SETUPS = {}


def setup(k):
    if k not in _SETUPS:
        h2.init()
        _SETUPS[k] = pu.Setup(k)
    return _SETUPS[k]


def second_columns(su, seed=0x5EC0D):
    return pu.system_columns(seed, su.k, su.b, table=su.cols["fixed"][1])


def failures(su, cols, theta=5, challenge=7):
    m = cu.mont_cols(cols)
    return h2.verify_witness(su.k, cu.SYSTEM_GATES, cu.SYSTEM_LOOKUPS, to_mont([theta])[0], su.b, cu.SYSTEM_PERM, None, m["fixed"], m["advice"],
                             m["instance"], to_mont([challenge]), copies=np.array(cu.SYSTEM_COPIES, dtype=np.uint32))


# ------------------------------------------------------------------ 1. accept
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["parts", "full"])
@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
@pytest.mark.parametrize("k,n_instances", [(5, 1), (5, 2), (10, 1)])
def test_gpu_proof_is_accepted(k, n_instances, multiopen, form):
    su = setup(k)
    columns = [su.cols, second_columns(su)][:n_instances]
    for c in columns:
        assert failures(su, c) == []
    instances = [pu.instance_of(c) for c in columns]
    proof = su.prove(columns, multiopen=multiopen, form=form)
    left, right = su.verify(proof.bytes, instances, multiopen)
    assert left is not None and right is not None
    assert pu.pairing_holds(left, right)
    assert not pu.pairing_holds(left, right, pu.SECRET + 1)  # the check is not vacuous
    # 32 bytes per point and scalar: advice 3, permuted 2, z_perm 2, z_lookup 1 per instance, random 1, h 3 points; advice 5, perm z 5
    # (2 + 2 + the first set's last), lookup 5 evaluations per instance, fixed 2, random 1, sigma 3; then the opening's points
    points, scalars = 8 * n_instances + 4, 15 * n_instances + 6
    opening = 2 if multiopen == "shplonk" else 4  # gwc: one witness per point x, omega x, omega^-1 x, omega^-6 x
    assert len(proof.bytes) == 32 * (points + scalars + opening)


# ------------------------------------------------------------------ 2. reject
def _reject_setup():
    su = setup(5)
    assert su.u == 26 and pu.ACTIVE + 2 < 25
    return su


@pytest.mark.gpu
def test_gpu_bad_gate_witness_is_rejected():
    su = _reject_setup()
    bad = {key: [list(c) for c in v] for key, v in su.cols.items()}
    bad["advice"][2][3] = (bad["advice"][2][3] + 1) % R_MOD  # c[3]: read by gate 0 at row 4 and by gate 1 at row 3
    assert failures(su, bad) == [("gate", 0, 4), ("gate", 1, 3)]
    proof = su.prove([bad])
    assert not su.accepts(proof.bytes, [pu.instance_of(bad)])


@pytest.mark.gpu
def test_gpu_bad_lookup_witness_is_rejected():
    """an input value its table lacks: commit_permuted cannot build A' and S' (the reference's ConstraintSystemFailure at
    lookup/prover.rs:391-475), so the prover raises and no proof exists"""
    su = _reject_setup()
    bad = {key: [list(c) for c in v] for key, v in su.cols.items()}
    table = set(su.cols["fixed"][1][:su.u])
    value = next(v for v in range(2, 1000) if v not in table)
    bad["advice"][0][25] = value  # a[25]: below u, past the active rows, in no copy
    assert failures(su, bad) == [("lookup", 0, 25)]
    with pytest.raises(h2.H2HipLookupError):
        su.prove([bad])


@pytest.mark.gpu
def test_gpu_bad_copy_witness_is_rejected():
    su = _reject_setup()
    bad = {key: [list(c) for c in v] for key, v in su.cols.items()}
    a = bad["advice"][0]
    a[12] = next(v for v in su.cols["fixed"][1][:su.u] if v != a[11])  # still in the table; rows 11 and 12 are past the active rows
    assert failures(su, bad) == [("permutation", 0, 11), ("permutation", 0, 12)]
    proof = su.prove([bad])
    assert not su.accepts(proof.bytes, [pu.instance_of(bad)])


@pytest.mark.gpu
def test_gpu_wrong_instance_vk_repr_and_flipped_bits_are_rejected():
    su = _reject_setup()
    instances = [pu.instance_of(su.cols)]
    proof = su.prove().bytes
    assert su.accepts(proof, instances)
    wrong = [[list(instances[0][0])]]
    wrong[0][0][2] = (wrong[0][0][2] + 1) % R_MOD
    assert not su.accepts(proof, wrong)
    assert not su.accepts(proof, [[instances[0][0][:-1]]])  # one value fewer: another transcript
    with pytest.raises(verifier.VerifyError):
        su.verify(proof, [[instances[0][0], []]])  # InvalidInstances
    vk = prover.VerifyingKey(su.cs, su.k, pu.VK_REPR + 1, su.pk.vk.fixed_commitments, su.pk.vk.permutation_commitments)
    assert not su.accepts(proof, instances, vk=vk)
    first_evaluation = 32 * 12  # after 3 + 2 + 2 + 1 + 1 + 3 points
    assert len(proof) == 32 * 35
    for offset in (0, first_evaluation, len(proof) - 32):
        for bit in (0, 3):
            flipped = bytearray(proof)
            flipped[offset] ^= 1 << bit
            assert not su.accepts(bytes(flipped), instances), (offset, bit)
    # malformed proofs raise
    with pytest.raises(transcript.TranscriptError, match="short read"):
        su.verify(proof[:-1], instances)
    non_canonical = bytearray(proof)
    non_canonical[first_evaluation:first_evaluation + 32] = (R_MOD + 1).to_bytes(32, "little")
    with pytest.raises(transcript.TranscriptError, match="invalid field element"):
        su.verify(bytes(non_canonical), instances)
    bad_point = bytearray(proof)
    bad_point[0:32] = (4).to_bytes(32, "little")  # no curve point has x = 4 (test_transcript checks 67 is not a square)
    with pytest.raises(transcript.TranscriptError, match="invalid point encoding"):
        su.verify(bytes(bad_point), instances)


# ------------------------------------------------------------------ 3. same bytes
@pytest.mark.gpu
@pytest.mark.parametrize("multiopen", ["shplonk", "gwc"])
def test_gpu_same_seed_same_bytes(multiopen):
    su = setup(5)
    base = su.prove(multiopen=multiopen).bytes
    assert su.prove(multiopen=multiopen).bytes == base, "two runs"
    assert su.prove(multiopen=multiopen, form="full").bytes == base, "parts and full form"
    assert su.prove(multiopen=multiopen, resident=False).bytes == base, "resident and host columns"
    assert su.prove(multiopen=multiopen, resident=False, form="full").bytes == base, "host columns, full form"
    assert su.prove(multiopen=multiopen, seed=b"\x08" * 32).bytes != base


# ------------------------------------------------------------------ 4. verifying key
@pytest.mark.gpu
def test_gpu_verifying_key_commitments_equal_the_oracle(oracle):
    su = setup(5)
    gl = su.params.g_lagrange
    for cols, got in ((su.fixed, su.pk.vk.fixed_commitments), (su.pk.host["permutations"], su.pk.vk.permutation_commitments)):
        assert len(cols) == len(got) and len(got) in (2, 3)
        for col, point in zip(cols, got):
            want = oracle.g1_to_affine(oracle.best_multiexp(np.ascontiguousarray(col), gl, 4))
            assert pu.mont_to_point(want) == point
    # the sigma columns are the ones the copies define: the identity permutation's would give other commitments
    ident = h2.permutation_keygen(su.pk.domain, h2.PermutationAssembly(su.n, 3).mapping, want=("permutations",))["permutations"]
    assert not np.array_equal(ident[0], su.pk.host["permutations"][0])


# ------------------------------------------------------------------ 5. residency
@pytest.mark.gpu
@pytest.mark.parametrize("multiopen,form", [("shplonk", "parts"), ("gwc", "full")])
def test_gpu_resident_proof_moves_less_than_one_column(multiopen, form):
    """With the advice columns produced in HBM (the witness callback's own upload is the test's, not the prover's), what the prover moves
    is the instance values (11 x 32 B), blinding rows, challenges, points and scalars upwards, commitments (96 B each) and evaluations
    downwards: a few KiB, whatever k is.  A column at k = 10 is 32 KiB."""
    su = setup(10)
    column_bytes = 32 << su.k
    proof = su.prove(multiopen=multiopen, form=form)
    assert proof.transfers and {d for d, _, _ in proof.transfers} == {"h2d", "d2h"}
    for direction, nbytes, what in proof.transfers:
        assert nbytes < column_bytes, (direction, nbytes, what)
    assert proof.total("h2d") < column_bytes and proof.total("d2h") < column_bytes
    assert proof.total("d2h") >= len(proof.bytes)  # everything in the proof came down
    host = su.prove(multiopen=multiopen, form=form, resident=False)
    assert host.bytes == proof.bytes
    assert host.total("h2d") > 20 * column_bytes and host.total("d2h") > 10 * column_bytes
    with pytest.raises(TypeError):  # numpy columns handed to the resident prover
        prover.create_proof(su.params, su.pk, [pu.instance_of(su.cols)], su.witness_fn([su.cols], False), transcript.Blake2bWrite(), b"\x07" * 32)


# ------------------------------------------------------------------ 6. device wrappers
def _golden_evaluator():
    from evalh_util import Evaluator
    A = lambda col, rot=0: ('advice', col, rot)  # noqa: E731
    F = lambda col, rot=0: ('fixed', col, rot)  # noqa: E731
    e_, a_, b_, c_, d_ = 0, 1, 2, 3, 4
    sf, sm, sa, sb, sc, sl = 0, 1, 2, 3, 4, 5
    gate = ('sum',
            ('sum', ('sum', ('sum', ('prod', A(a_), F(sa)), ('prod', A(b_), F(sb))), ('prod', ('prod', A(a_), A(b_)), F(sm))),
             ('neg', ('prod', A(c_), F(sc)))),
            ('prod', F(sf), ('prod', A(d_, 1), A(e_, -1))))
    gate2 = ('sum', ('scaled', ('prod', A(c_), A(c_)), 7), ('sum', ('prod', ('const', 2), A(d_)), ('neg', ('const', 5))))
    return Evaluator.new([gate, gate2], [([A(a_)], [F(sl)])])


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _to_device_case(case, column_keys, single_keys):
    out = dict(case)
    for key in column_keys:
        out[key] = [_dev(a) for a in case[key]]
    for key in single_keys:
        out[key] = _dev(case[key])
    out["lookups"] = [tuple(_dev(p) for p in l) for l in case["lookups"]]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["k3", "k4"])
def test_gpu_evaluate_h_device_wrappers_equal_the_host_wrappers(tag):
    import os
    import torch
    from conftest import ROOT
    from test_evalh import load_case
    h2.init()
    z = np.load(os.path.join(ROOT, "tests", "golden", "evalh.npz"), allow_pickle=False)
    golden, vin, vout = load_case(z, tag)
    ev = _golden_evaluator()
    case = {key: v for key, v in golden.items() if key != "custom"}
    case["lookups"] = [tuple(l[1:]) for l in golden["lookups"]]
    columns = ("fixed_cosets", "advice_polys", "instance_polys", "perm_product_cosets", "perm_cosets")
    want = ev.evaluate_h(case, vin.copy())
    assert np.array_equal(want, vout)
    d_values = _dev(vin)
    assert ev.evaluate_h_device(_to_device_case(case, columns, ("l0", "l_last", "l_active_row")), d_values) is d_values
    torch.cuda.synchronize()
    assert np.array_equal(h2.to_numpy_u64(d_values), want)
    # the parts form reads coefficient columns: any 2^k elements are a polynomial, here the first rows of the golden cosets
    n = 1 << case["k"]
    parts = {key: v for key, v in case.items() if key not in ("fixed_cosets", "perm_product_cosets", "perm_cosets", "l0", "l_last", "l_active_row")}
    parts.update(fixed_polys=[c[:n].copy() for c in case["fixed_cosets"]], perm_product_polys=[c[:n].copy() for c in case["perm_product_cosets"]],
                 perm_polys=[c[:n].copy() for c in case["perm_cosets"]], l0_poly=case["l0"][:n].copy(), l_last_poly=case["l_last"][:n].copy(),
                 l_active_row_poly=case["l_active_row"][:n].copy())
    dom = h2.EvaluationDomain.new(((1 << case["extended_k"]) >> case["k"]) + 1, case["k"])
    assert dom.extended_k == case["extended_k"]
    columns_p = ("fixed_polys", "advice_polys", "instance_polys", "perm_product_polys", "perm_polys")
    singles_p = ("l0_poly", "l_last_poly", "l_active_row_poly")
    for kwargs in ({}, {"t_evaluations": dom.t_evaluations}, {"parts": (1, 1)}):
        want_p = ev.evaluate_h_parts(parts, vin.copy(), **kwargs)
        d_values = _dev(vin)
        ev.evaluate_h_parts_device(_to_device_case(parts, columns_p, singles_p), d_values, stream=torch.cuda.current_stream(), **kwargs)
        torch.cuda.synchronize()
        assert np.array_equal(h2.to_numpy_u64(d_values), want_p), kwargs
    # a numpy column in a device call, or a tensor in a host call, is refused before the engine sees the address
    with pytest.raises(TypeError):
        ev.evaluate_h_device(case, _dev(vin))
    with pytest.raises(TypeError):
        ev.evaluate_h(_to_device_case(case, columns, ("l0", "l_last", "l_active_row")), vin.copy())
