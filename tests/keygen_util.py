"""Python big-integer restatement of the reference's key generation columns (test infrastructure only).

Assembly restates permutation::keygen::Assembly::{new, copy} (halo2_proofs/src/plonk/permutation/keygen.rs:27-103) literally, on lists
of tuples; sigma restates build_vk / build_pk's tables (:111-151); batch_invert_assigned restates poly.rs:180-209 with pow(d, -1, r);
unit_columns gives the Lagrange columns behind l0, l_blind and l_last (plonk/keygen.rs:320-339).  Values are canonical integers mod r;
to_mont / from_mont convert to and from the engine's (n, 4) uint64 Montgomery columns."""
import numpy as np

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
_MONT = (1 << 256) % R_MOD
_MONT_INV = pow(_MONT, -1, R_MOD)
S = 28
ROOT_OF_UNITY = 0x03ddb9f5166d18b798865ea93dd31f743215cf6dd39329c8d34f1ed960c37c9c  # bn256::Fr, a primitive 2^28-th root
DELTA = pow(7, 1 << S, R_MOD)  # Fr::DELTA = MULTIPLICATIVE_GENERATOR^(2^S)


def to_mont(vals):
    raw = b"".join(((int(v) % R_MOD) * _MONT % R_MOD).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def from_mont(arr):
    raw = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") * _MONT_INV % R_MOD for i in range(0, len(raw), 32)]


def fe(v):
    return to_mont([v])[0]


def root_of_unity(k):
    """omega of exact order 2^k, as EvaluationDomain::new derives it (poly/domain.rs:54-73)"""
    return pow(ROOT_OF_UNITY, 1 << (S - k), R_MOD)


class BoundsFailure(Exception):
    pass


class Assembly:
    """keygen.rs:16-103"""

    def __init__(self, n, n_columns):  # :28-46
        columns = [[(i, j) for j in range(n)] for i in range(n_columns)]
        self.mapping = [list(c) for c in columns]
        self.aux = [list(c) for c in columns]
        self.sizes = [[1] * n for _ in range(n_columns)]

    def copy(self, left_column, left_row, right_column, right_row):  # :48-103
        if left_column >= len(self.mapping) or right_column >= len(self.mapping):  # :55-64
            raise BoundsFailure("ColumnNotInPermutation")
        if left_row >= len(self.mapping[left_column]) or right_row >= len(self.mapping[right_column]):  # :67-71
            raise BoundsFailure("BoundsFailure")
        left_cycle = self.aux[left_column][left_row]  # :75
        right_cycle = self.aux[right_column][right_row]  # :76
        if left_cycle == right_cycle:  # :79-81
            return
        if self.sizes[left_cycle[0]][left_cycle[1]] < self.sizes[right_cycle[0]][right_cycle[1]]:  # :83-85
            left_cycle, right_cycle = right_cycle, left_cycle
        self.sizes[left_cycle[0]][left_cycle[1]] += self.sizes[right_cycle[0]][right_cycle[1]]  # :88
        i = right_cycle  # :89-96
        while True:
            self.aux[i[0]][i[1]] = left_cycle
            i = self.mapping[i[0]][i[1]]
            if i == right_cycle:
                break
        tmp = self.mapping[left_column][left_row]  # :98-100
        self.mapping[left_column][left_row] = self.mapping[right_column][right_row]
        self.mapping[right_column][right_row] = tmp

    def mapping_array(self):
        return np.array(self.mapping, dtype=np.uint32).reshape(len(self.mapping), -1, 2)


def omega_powers(omega, n):
    """:111-122"""
    out, cur = [], 1
    for _ in range(n):
        out.append(cur)
        cur = cur * omega % R_MOD
    return out


def sigma(mapping, omega, delta=DELTA, powers=None):
    """:124-151: permutations[i][j] = deltaomega[c][r] = delta^c omega^r for (c, r) = mapping[i][j].  mapping: (m, n, 2) array or nested
    lists of pairs.  Returns integer lists."""
    mp = np.asarray(mapping).reshape(len(mapping), -1, 2)
    m, n = mp.shape[0], mp.shape[1]
    powers = omega_powers(omega, n) if powers is None else powers
    dpow = [pow(delta, c, R_MOD) for c in range(m)]
    out = []
    for i in range(m):
        cs, rs = mp[i, :, 0].tolist(), mp[i, :, 1].tolist()
        out.append([dpow[c] * powers[r] % R_MOD for c, r in zip(cs, rs)])
    return out


def sigma_mont(mapping, omega, delta=DELTA, powers=None):
    """sigma as (n, 4) uint64 Montgomery columns, without the detour over canonical lists: the omega table carries the factor R"""
    mp = np.asarray(mapping).reshape(len(mapping), -1, 2)
    m, n = mp.shape[0], mp.shape[1]
    powers = omega_powers(omega, n) if powers is None else powers
    pm = [p * _MONT % R_MOD for p in powers]
    dpow = [pow(delta, c, R_MOD) for c in range(m)]
    out = []
    for i in range(m):
        cs, rs = mp[i, :, 0].tolist(), mp[i, :, 1].tolist()
        raw = b"".join((dpow[c] * pm[r] % R_MOD).to_bytes(32, "little") for c, r in zip(cs, rs))
        out.append(np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy())
    return out


def batch_invert_assigned(numerators, rat_rows, rat_denoms):
    """poly.rs:180-209: numerators[j] integers; rat_rows[j] / rat_denoms[j] the Rational cells.  Assigned::evaluate maps x / 0 to 0, which is
    what BatchInvert's untouched zero times the numerator gives."""
    out = []
    for nums, rows, dens in zip(numerators, rat_rows, rat_denoms):
        col = [v % R_MOD for v in nums]
        for r, d in zip(rows, dens):
            col[r] = col[r] * (pow(d, -1, R_MOD) if d % R_MOD else 0) % R_MOD
        out.append(col)
    return out


def unit_columns(k, b):
    """plonk/keygen.rs:322-339: the Lagrange columns of l0, l_blind and l_last"""
    n = 1 << k
    l0 = [0] * n
    l0[0] = 1
    l_blind = [0] * (n - b) + [1] * b
    l_last = [0] * n
    l_last[n - b - 1] = 1
    return l0, l_blind, l_last


def orbit(mapping, cell):
    """the cells reached from `cell` by following mapping until it returns"""
    out, i = [], cell
    while True:
        out.append(i)
        i = tuple(mapping[i[0]][i[1]])
        if i == cell:
            return out
        assert len(out) <= sum(len(c) for c in mapping), "not a cycle"
