"""The ordered permutation mapping of include/halo2hip.h ("permutation mapping from copy constraints") restated with a dict union-find
and `sorted`: cells are numbered id(c, r) = c 2^k + r, the copies are the edges of a graph on the cells, and every cell maps to the
cell of its connected component with the least id above its own, the component's last cell back to its least one.  The definition is
later than the reference; this file pins it."""
import numpy as np


def ordered_mapping(k, m, copies):
    """copies: an iterable of (left_column, left_row, right_column, right_row), all in range -> the (m, 2^k, 2) uint32 mapping"""
    n = 1 << k
    parent = {}

    def find(x):
        root = x
        while parent.get(root, root) != root:
            root = parent[root]
        while parent.get(x, x) != root:
            parent[x], x = root, parent[x]
        return root

    for lc, lr, rc, rr in copies:
        lc, lr, rc, rr = int(lc), int(lr), int(rc), int(rr)
        assert 0 <= lc < m and 0 <= rc < m and 0 <= lr < n and 0 <= rr < n
        a, b = find(lc * n + lr), find(rc * n + rr)
        parent.setdefault(a, a)
        parent.setdefault(b, b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    components = {}
    for x in parent:
        components.setdefault(find(x), []).append(x)
    out = np.zeros((m, n, 2), dtype=np.uint32)
    out[:, :, 0] = np.arange(m, dtype=np.uint32)[:, None]
    out[:, :, 1] = np.arange(n, dtype=np.uint32)[None, :]
    for cells in components.values():
        cells = sorted(cells)
        for x, y in zip(cells, cells[1:] + cells[:1]):
            out[x // n, x % n] = (y // n, y % n)
    return out


def valid_copies(k, m, copies):
    """the copies whose columns and rows are in range, as the device form keeps them"""
    n = 1 << k
    return [c for c in copies if c[0] < m and c[2] < m and c[1] < n and c[3] < n]


def cycles(mapping):
    """the cycles of a mapping as a set of frozensets of cell ids"""
    mp = np.asarray(mapping)
    m, n = mp.shape[0], mp.shape[1]
    nxt = (mp[:, :, 0].astype(np.int64) * n + mp[:, :, 1]).reshape(-1)
    seen = np.zeros(m * n, dtype=bool)
    out = set()
    for x in range(m * n):
        if seen[x]:
            continue
        cyc, y = [], x
        while not seen[y]:
            seen[y] = True
            cyc.append(y)
            y = int(nxt[y])
        assert y == x, "not a permutation"
        out.add(frozenset(cyc))
    return out


def random_copies(seed, k, m, count, rows=None):
    """`count` copies between uniformly drawn cells (rows below `rows`), an (count, 4) uint32 array"""
    n = 1 << k
    rng = np.random.default_rng(seed)
    out = np.zeros((count, 4), dtype=np.uint32)
    out[:, 0::2] = rng.integers(0, m, size=(count, 2), dtype=np.uint32)
    out[:, 1::2] = rng.integers(0, n if rows is None else rows, size=(count, 2), dtype=np.uint32)
    return out


def shuffled(copies, seed):
    c = np.array(copies, dtype=np.uint32).reshape(-1, 4)
    return c[np.random.default_rng(seed).permutation(len(c))]


def swapped(copies, seed):
    """a random half of the copies with their sides exchanged"""
    c = np.array(copies, dtype=np.uint32).reshape(-1, 4).copy()
    flip = np.random.default_rng(seed).integers(0, 2, size=len(c)).astype(bool)
    c[flip] = c[flip][:, [2, 3, 0, 1]]
    return c
