"""Python big-integer restatement of the reference's grand-product columns (test infrastructure only).

permutation_commit restates permutation::Argument::commit (halo2_proofs/src/plonk/permutation/prover.rs:96-166) and lookup_commit
lookup::Permuted::commit_product (plonk/lookup/prover.rs:194-249), on canonical integers mod r; ff_batch_invert restates ff 0.12's
BatchInvert, which leaves zero elements in place.  Helpers convert to and from the engine's (n, 4) uint64 Montgomery columns."""
import numpy as np

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
_MONT = (1 << 256) % R_MOD
_MONT_INV = pow(_MONT, -1, R_MOD)
ROOT_OF_UNITY = 0x03ddb9f5166d18b798865ea93dd31f743215cf6dd39329c8d34f1ed960c37c9c  # bn256::Fr, a primitive 2^28-th root


def to_mont(vals):
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        m = (int(v) % R_MOD) * _MONT % R_MOD
        for j in range(4):
            out[i, j] = (m >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out


def from_mont(arr):
    a = np.asarray(arr, dtype=np.uint64).reshape(-1, 4)
    out = []
    for row in a:
        m = int(row[0]) | int(row[1]) << 64 | int(row[2]) << 128 | int(row[3]) << 192
        out.append(m * _MONT_INV % R_MOD)
    return out


def fe(v):
    return to_mont([v])[0]


def root_of_unity(k):
    """omega of exact order 2^k: ROOT_OF_UNITY^(2^(S - k)), as EvaluationDomain::new derives it (poly/domain.rs)"""
    return pow(ROOT_OF_UNITY, 1 << (28 - k), R_MOD)


def ff_batch_invert(vals):
    """ff 0.12 BatchInvert: one running product over the non-zero elements, one inversion, a back sweep; zeros stay zero"""
    vals = list(vals)
    acc, tmp = 1, []
    for v in vals:
        tmp.append(acc)
        if v:
            acc = acc * v % R_MOD
    acc = pow(acc, -1, R_MOD)
    for i in range(len(vals) - 1, -1, -1):
        v = vals[i]
        if v:
            new = acc * tmp[i] % R_MOD
            acc = acc * v % R_MOD
            vals[i] = new
    return vals


def permutation_commit(k, omega, delta, beta, gamma, columns, permutations, chunk_len, blinding, blinding_factors):
    """columns / permutations: lists of integer lists (p_c, s_c); blinding: list per set of blinding_factors integers.
    Returns the z column of every set (integers)."""
    n = 1 << k
    out = []
    last_z = 1
    deltaomega = 1  # prover.rs:76, kept across sets
    for t, start in enumerate(range(0, len(columns), chunk_len)):
        cols = columns[start:start + chunk_len]
        perms = permutations[start:start + chunk_len]
        mv = [1] * n  # :96
        for p, s in zip(cols, perms):  # :99-113
            for i in range(n):
                mv[i] = mv[i] * (beta * s[i] + gamma + p[i]) % R_MOD
        mv = ff_batch_invert(mv)  # :117
        for p in cols:  # :121-140
            d = deltaomega
            for i in range(n):
                mv[i] = mv[i] * (d * beta + gamma + p[i]) % R_MOD
                d = d * omega % R_MOD
            deltaomega = deltaomega * delta % R_MOD
        z = [last_z]  # :153-159
        for row in range(1, n):
            z.append(z[row - 1] * mv[row - 1] % R_MOD)
        for j in range(blinding_factors):  # :161-163
            z[n - blinding_factors + j] = blinding[t][j] % R_MOD
        last_z = z[n - (blinding_factors + 1)]  # :165
        out.append(z)
    return out


def lookup_commit(k, beta, gamma, a, s, ap, sp, blinding, blinding_factors):
    """one lookup: A, S, A', S' integer lists; returns z (integers)"""
    n = 1 << k
    lp = [(beta + ap[i]) * (gamma + sp[i]) % R_MOD for i in range(n)]  # :197-206
    lp = ff_batch_invert(lp)  # :208
    for i in range(n):  # :213-220
        lp[i] = lp[i] * (a[i] + beta) % R_MOD * (s[i] + gamma) % R_MOD
    z, state = [], 1  # :237-249
    for cur in [1] + lp:
        state = state * cur % R_MOD
        z.append(state)
    z = z[:n - blinding_factors] + [blinding[j] % R_MOD for j in range(blinding_factors)]
    return z

