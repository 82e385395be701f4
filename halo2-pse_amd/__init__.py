"""halo2_pse_amd -- thin ctypes plumbing over libhalo2hip.so (include/halo2hip.h).

The product is the C-ABI library (HIP kernels for gfx950 + C++ host code); the C++ mirror of
the reference's Rust interface lives in host/halo2hip.hpp.  This module only exists so that
tests/, bench.py and __graft_entry__.py can drive the C ABI from Python; names follow the
reference (halo2_proofs::arithmetic::{best_multiexp, best_fft}, poly::EvaluationDomain,
poly::kzg::ParamsKZG).  There is no CPU fallback here: if the library or the GPU is
missing, calls raise.

Every entry point's prototype is stated once, in _abi.py, _abi_ipa.py, _abi_ipa_round.py, _abi_g1.py and _abi_pairing.py (generated from the headers by
tools/gen_ctypes_abi.py) and
bound by lib(): call sites pass plain Python ints and bools for the by-value parameters, and ctypes refuses a wrong argument count.

Arrays: numpy uint64 -- Fr elements (n,4), G1Affine (n,8), G1 Jacobian (12,): 4 x u64 LE limbs,
Montgomery form (halo2curves' in-memory / RawBytes layout).
"""
import ctypes
import os
import subprocess

import numpy as np

from ._abi import PROTOTYPES
from ._abi_g1 import PROTOTYPES as PROTOTYPES_G1
from ._abi_ipa import PROTOTYPES as PROTOTYPES_IPA
from ._abi_ipa_round import PROTOTYPES as PROTOTYPES_IPA_ROUND
from ._abi_pairing import PROTOTYPES as PROTOTYPES_PAIRING

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HALO2_HIP_LIB") or os.path.join(_HERE, "libhalo2hip.so")  # HALO2_HIP_LIB: another build of the library (A/B measurements)

_lib = None


class H2HipError(RuntimeError):
    pass


def build(force=False, jobs=4):
    """compile libhalo2hip.so in-tree (hipcc --offload-arch=gfx950)"""
    args = ["make", "-C", _HERE, "-j%d" % jobs]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise H2HipError("libhalo2hip.so is not built (run __graft_entry__.build()); no CPU fallback exists")
        # PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / libhsa-runtime64; two HIP
        # runtimes in one process cannot both open the GPU.  Import torch first so that this
        # library's NEEDED libamdhip64.so.7 binds to the runtime torch already loaded (same
        # SONAME).  A pure C++/Rust consumer gets /opt/rocm's runtime through the RUNPATH.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        # every entry point's prototype, generated from the headers (tools/gen_ctypes_abi.py): ctypes then converts plain ints at the
        # declared width and refuses a wrong argument count.  Bare argtypes would let a cdecl function take surplus arguments; naming
        # each parameter an input (paramflags) makes the count exact.  Another build (HALO2_HIP_LIB) may lack a name; tests/test_abi.py
        # holds the in-tree one to all of them.
        # The inner-product argument's entry points (include/halo2hip_ipa.h) have a table of their own, _abi_ipa.py, applied after the first; the host group
        # sums (include/halo2hip_g1.h) have _abi_g1.py, applied after those two; the host pairing (include/halo2hip_pairing.h) has
        # _abi_pairing.py, applied after those; the round as one call (include/halo2hip_ipa_round.h) has _abi_ipa_round.py, applied last.
        for name, (restype, argtypes) in (list(PROTOTYPES.items()) + list(PROTOTYPES_IPA.items()) + list(PROTOTYPES_G1.items()) +
                                          list(PROTOTYPES_PAIRING.items()) + list(PROTOTYPES_IPA_ROUND.items())):
            try:
                fn = ctypes.CFUNCTYPE(restype, *argtypes)((name, L), ((1,),) * len(argtypes))
            except AttributeError:
                continue
            setattr(L, name, fn)
        # release streams, workspaces and worker threads while the HIP runtime is still alive (a profiler's own
        # finalisation otherwise meets them in the static destructors at process exit)
        import atexit
        atexit.register(L.h2hip_shutdown)
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise H2HipError("%s failed (rc=%d): %s" % (what, rc, lib().h2hip_last_error().decode()))


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _u64(a, cols=None):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if cols is not None and (a.ndim != 2 or a.shape[1] != cols):
        raise ValueError("expected shape (n,%d), got %s" % (cols, a.shape))
    return a


def _fe(a):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(4)
    return a


def init(device=None):
    """device: None (HALO2_HIP_DEVICES or the current HIP device), one ordinal, or a list of ordinals (multi-GPU MSM)"""
    if device is None:
        _check(lib().h2hip_init(None, 0), "h2hip_init")
    else:
        devs = [int(d) for d in device] if isinstance(device, (list, tuple)) else [int(device)]
        ids = (ctypes.c_int * len(devs))(*devs)
        _check(lib().h2hip_init(ids, len(devs)), "h2hip_init")


def num_devices():
    return int(lib().h2hip_num_devices())


def shutdown():
    lib().h2hip_shutdown()


def device_count():
    return int(lib().h2hip_device_count())


def version():
    return lib().h2hip_version().decode()


# ------------------------------------------------------------------ arithmetic.rs
def best_multiexp(coeffs, bases):
    """halo2_proofs::arithmetic::best_multiexp (arithmetic.rs:132-159) for C = bn256::G1Affine.
    Returns the Jacobian result (12,) uint64."""
    coeffs, bases = _u64(coeffs, 4), _u64(bases, 8)
    assert coeffs.shape[0] == bases.shape[0]  # assert_eq!(coeffs.len(), bases.len()), arithmetic.rs:133
    out = np.zeros(12, dtype=np.uint64)
    _check(lib().h2hip_msm_bn254(_p(coeffs), _p(bases), coeffs.shape[0], _p(out)), "h2hip_msm_bn254")
    return out


def best_multiexp_batch(coeffs_list, bases):
    """`len(coeffs_list)` MSMs over the same bases (the back-to-back commits of plonk/prover.rs:361-365);
    returns (count, 12) uint64 Jacobian results."""
    bases = _u64(bases, 8)
    cols = [_u64(c, 4) for c in coeffs_list]
    n = bases.shape[0]
    for c in cols:
        assert c.shape[0] == n  # arithmetic.rs:133
    count = len(cols)
    ptrs = (ctypes.c_void_p * count)(*[c.ctypes.data for c in cols])
    out = np.zeros((count, 12), dtype=np.uint64)
    _check(lib().h2hip_msm_bn254_batch(ptrs, _p(bases), n, count, _p(out)), "h2hip_msm_bn254_batch")
    return out


def best_fft(a, omega, log_n):
    """halo2_proofs::arithmetic::best_fft (arithmetic.rs:171-234) for G = bn256::Fr; in place on `a`."""
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    assert a.shape == (1 << log_n, 4)  # assert_eq!(n, 1 << log_n), arithmetic.rs:184
    _check(lib().h2hip_ntt_bn254_fr(_p(a), _p(_fe(omega)), log_n), "h2hip_ntt_bn254_fr")


def _host_ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def best_fft_batch(columns, omega, log_n):
    """`len(columns)` in-place best_fft calls on host columns as one pipelined call (upload i + 1 | transform i | download i - 1)"""
    for a in columns:
        assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"] and a.shape == (1 << log_n, 4)
    if columns:
        _check(lib().h2hip_ntt_bn254_fr_batch(_host_ptrs(columns), len(columns), _p(_fe(omega)), log_n),
               "h2hip_ntt_bn254_fr_batch")


def g_to_lagrange(g, k):
    """arithmetic::g_to_lagrange (arithmetic.rs:277-301): (2^k, 8) affine points -> (2^k, 8) affine points"""
    g = _u64(g, 8)
    assert g.shape[0] == 1 << k
    out = np.zeros((1 << k, 8), dtype=np.uint64)
    _check(lib().h2hip_g_to_lagrange_bn254(_p(g), k, _p(out)), "h2hip_g_to_lagrange_bn254")
    return out


def best_fft_g1(a_xyz, omega, log_n):
    """halo2_proofs::arithmetic::best_fft for G = bn256::G1 (arithmetic.rs:171-234): in place on (2^log_n, 12) Jacobian points"""
    assert a_xyz.dtype == np.uint64 and a_xyz.flags["C_CONTIGUOUS"] and a_xyz.shape == (1 << log_n, 12)
    _check(lib().h2hip_fft_bn254_g1(_p(a_xyz), _p(_fe(omega)), log_n), "h2hip_fft_bn254_g1")


def g1_to_affine(xyz):
    xyz = np.ascontiguousarray(xyz, dtype=np.uint64).reshape(12)
    out = np.zeros(8, dtype=np.uint64)
    _check(lib().h2hip_g1_to_affine(_p(xyz), _p(out)), "h2hip_g1_to_affine")
    return out


def g1_fold(partials):
    partials = np.ascontiguousarray(partials, dtype=np.uint64).reshape(-1, 12)
    out = np.zeros(12, dtype=np.uint64)
    _check(lib().h2hip_g1_fold(_p(partials), partials.shape[0], _p(out)), "h2hip_g1_fold")
    return out


def bases_pin(bases):
    assert bases.dtype == np.uint64 and bases.flags["C_CONTIGUOUS"]
    _check(lib().h2hip_bases_pin(_p(bases), bases.shape[0]), "h2hip_bases_pin")


def bases_unpin(bases):
    _check(lib().h2hip_bases_unpin(_p(bases)), "h2hip_bases_unpin")


_device_pins = {}  # device address -> weakref.finalize on the STORAGE of the tensor that was pinned


def _unpin_address(addr):
    _device_pins.pop(addr, None)
    try:
        lib().h2hip_bases_unpin(ctypes.c_void_p(addr))
    except Exception:
        pass


def bases_pin_device(d_bases, n=None):
    """pin device-resident points (torch CUDA tensor): copies them and builds the fixed-base window table.  The buffer's
    address is the cache key, so the entry is tied to the lifetime of the tensor's STORAGE (not of the tensor object: pinning
    through a view or a temporary -- `t.view(-1)`, `t[:n]` -- must not unpin while `t` is alive): when the storage is freed
    without bases_unpin_device the entry goes with it (the library's own fingerprint check is the second line of defence)."""
    import weakref
    n = d_bases.numel() * d_bases.element_size() // 64 if n is None else int(n)
    _check(lib().h2hip_bases_pin_device(_dptr(d_bases), n, _stream()), "h2hip_bases_pin_device")
    addr = d_bases.data_ptr()
    old = _device_pins.pop(addr, None)
    if old is not None:
        old.detach()
    # torch keeps one Python wrapper per storage alive as long as the storage is (checked on this image: a finalizer attached to
    # `t.view(-1).untyped_storage()` fires when the last tensor over the storage goes, not when the temporary view does)
    _device_pins[addr] = weakref.finalize(d_bases.untyped_storage(), _unpin_address, addr)


def bases_unpin_device(d_bases):
    fin = _device_pins.pop(d_bases.data_ptr(), None)
    if fin is not None:
        fin.detach()
    _check(lib().h2hip_bases_unpin(_dptr(d_bases)), "h2hip_bases_unpin")


def columns_pin(columns):
    """keep a proving key's constant columns (pk.fixed_cosets, pk.l0 / l_last / l_active_row, pk.permutation.cosets: (2^extended_k, 4)
    uint64 each) in HBM across host-pointer evaluate_h calls, keyed by their host addresses (h2hip_columns_pin)"""
    cols = list(columns)
    if not cols:
        return
    for a in cols:
        assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"] and a.shape == cols[0].shape and a.shape[1] == 4
    _check(lib().h2hip_columns_pin(_host_ptrs(cols), len(cols), cols[0].shape[0]), "h2hip_columns_pin")


def columns_unpin(columns):
    cols = list(columns)
    if cols:
        _check(lib().h2hip_columns_unpin(_host_ptrs(cols), len(cols)), "h2hip_columns_unpin")


def columns_pinned_info():
    """(columns, bytes of HBM) the pinned-column cache holds"""
    n, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _check(lib().h2hip_columns_pinned_info(ctypes.byref(n), ctypes.byref(b)), "h2hip_columns_pinned_info")
    return n.value, b.value


_part_pins = {}  # address -> weakref.finalize on the array (or the tensor's storage) whose part cosets are pinned


def _part_unpin_address(addr):
    _part_pins.pop(addr, None)
    try:
        lib().h2hip_part_cosets_unpin((ctypes.c_void_p * 1)(addr), 1)
    except Exception:
        pass


def part_cosets_pin(polys, domain):
    """keep all P part cosets of a proving key's coefficient-form polynomials (pk.fixed_polys, pk.l0 / l_last / l_active_row as
    polynomials, pk.permutation.polys: (2^k, 4) uint64 arrays, or torch CUDA tensors of 2^k x 32 B) in HBM across evaluate_h_parts calls
    over `domain` (h2hip_part_cosets_pin[_device]), keyed by their addresses.  An entry goes when its array (a tensor's storage) does;
    a device tensor must stay unchanged until then."""
    import weakref
    polys = list(polys)
    if not polys:
        return
    host = isinstance(polys[0], np.ndarray)
    consts = (domain.k, domain.extended_k, _p(domain.extended_omega), _p(domain.g_coset), _p(domain.g_coset_inv))
    if host:
        for a in polys:
            assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"] and a.shape == (1 << domain.k, 4)
        _check(lib().h2hip_part_cosets_pin(_host_ptrs(polys), len(polys), *consts), "h2hip_part_cosets_pin")
    else:
        for t in polys:
            assert t.numel() * t.element_size() == 32 << domain.k
        _check(lib().h2hip_part_cosets_pin_device(_ptr_array(polys), len(polys), *consts, _stream()), "h2hip_part_cosets_pin_device")
    for a in polys:
        addr = a.ctypes.data if host else a.data_ptr()
        old = _part_pins.pop(addr, None)
        if old is not None:
            old.detach()
        try:
            _part_pins[addr] = weakref.finalize(a if host else a.untyped_storage(), _part_unpin_address, addr)
            _part_pins[addr].atexit = False  # at exit the engine's shutdown frees every entry
        except TypeError:  # a read-only view that cannot be weakly referenced: the caller unpins
            pass


def part_cosets_unpin(polys):
    polys = list(polys)
    if not polys:
        return
    addrs = [a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr() for a in polys]
    for addr in addrs:
        fin = _part_pins.pop(addr, None)
        if fin is not None:
            fin.detach()
    _check(lib().h2hip_part_cosets_unpin((ctypes.c_void_p * len(addrs))(*addrs), len(addrs)), "h2hip_part_cosets_unpin")


def part_cosets_pinned_info():
    """(polynomials, bytes of HBM) the pinned part cosets hold"""
    n, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _check(lib().h2hip_part_cosets_pinned_info(ctypes.byref(n), ctypes.byref(b)), "h2hip_part_cosets_pinned_info")
    return n.value, b.value


def evalh_parts_stats():
    """the calling thread's last evaluate_h_parts call (h2hip_debug_evalh_parts_stats): columns scaled and transformed and columns served
    from pins (both summed over parts), column bytes uploaded, arena bytes"""
    out = (ctypes.c_uint64 * 4)()
    _check(lib().h2hip_debug_evalh_parts_stats(out), "h2hip_debug_evalh_parts_stats")
    return tuple(int(x) for x in out)


def bases_pinned_info(bases):
    """(points, window bits, windows, bytes of HBM) of a pinned host array or device tensor"""
    ptr = _p(bases) if isinstance(bases, np.ndarray) else _dptr(bases)
    n, c, w, b = ctypes.c_size_t(0), ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_size_t(0)
    _check(lib().h2hip_bases_pinned_info(ptr, ctypes.byref(n), ctypes.byref(c), ctypes.byref(w), ctypes.byref(b)), "h2hip_bases_pinned_info")
    return n.value, c.value, w.value, b.value


# ------------------------------------------------------------------ bn256::Fr constants (halo2curves 0.3.1)
FR_MODULUS = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
FR_S = 28
FR_ROOT_OF_UNITY = 0x03ddb9f5166d18b798865ea93dd31f743215cf6dd39329c8d34f1ed960c37c9c
FR_ZETA = 0x30644e72e131a029048b6e193fd84104cc37a73fec2bc5e9b8ca0b2d36636f23
_FR_R = (1 << 256) % FR_MODULUS


class PrimeField:
    """what EvaluationDomain::new needs of `G::Scalar` (ff::PrimeField + FieldExt): modulus, 2-adicity S, ROOT_OF_UNITY
    (a primitive 2^S-th root), ZETA (a primitive cube root), and the 4 x u64 Montgomery limbs (R = 2^256) of an integer"""

    def __init__(self, name, modulus, S, root_of_unity, zeta):
        self.name, self.modulus, self.S, self.root_of_unity, self.zeta = name, modulus, S, root_of_unity, zeta
        self._R = (1 << 256) % modulus

    def from_int(self, v):
        m = (int(v) % self.modulus) * self._R % self.modulus
        return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


BN254_FR = PrimeField("bn256::Fr", FR_MODULUS, FR_S, FR_ROOT_OF_UNITY, FR_ZETA)
# pasta_curves Fp (the scalar field of vesta / EqAffine, the curve of the reference's pinned verification key in
# tests/plonk_api.rs:624-632): multiplicative generator 5, 2-adicity 32, ROOT_OF_UNITY = 5^((p - 1) / 2^32), ZETA a cube root
# of unity (5^((p - 1) / 3); which of the two the crate fixes is not visible in the reference and does not enter omega).
_PASTA_P = 0x40000000000000000000000000000000224698fc094cf91b992d30ed00000001
PASTA_FP = PrimeField("pasta::Fp", _PASTA_P, 32, pow(5, (_PASTA_P - 1) >> 32, _PASTA_P), pow(5, (_PASTA_P - 1) // 3, _PASTA_P))


def fr_from_int(v):
    """integer -> the 4 x u64 Montgomery limbs the reference stores"""
    m = (int(v) % FR_MODULUS) * _FR_R % FR_MODULUS
    return np.array([(m >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def fr_to_int(limbs):
    m = sum(int(x) << (64 * i) for i, x in enumerate(np.asarray(limbs, dtype=np.uint64).reshape(4)))
    return m * pow(_FR_R, -1, FR_MODULUS) % FR_MODULUS


# ------------------------------------------------------------------ few-term group sums on the host (include/halo2hip_g1.h)
FQ_MODULUS = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
_FQ_R = (1 << 256) % FQ_MODULUS
_FQ_R_INV = pow(_FQ_R, -1, FQ_MODULUS)


def g1_from_int(point):
    """an affine integer pair (None: the identity) -> (8,) uint64 Montgomery limbs"""
    if point is None:
        return np.zeros(8, dtype=np.uint64)
    x, y = point[0] * _FQ_R % FQ_MODULUS, point[1] * _FQ_R % FQ_MODULUS
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for v in (x, y) for i in range(4)], dtype=np.uint64)


def g1_to_int(limbs):
    """(8,) uint64 Montgomery limbs -> an affine integer pair, None for (0, 0)"""
    v = [int(w) for w in np.asarray(limbs, dtype=np.uint64).reshape(8)]
    x = sum(w << (64 * i) for i, w in enumerate(v[:4])) * _FQ_R_INV % FQ_MODULUS
    y = sum(w << (64 * i) for i, w in enumerate(v[4:])) * _FQ_R_INV % FQ_MODULUS
    return None if x == 0 and y == 0 else (x, y)


def g1_linear_combinations_limbs(addends, scalars, points, m=None):
    """h2hip_g1_linear_combinations_bn254 on limbs: addends (m, 12) Jacobian or None, scalars (m, t, 4) Montgomery, points (t, 8)
    affine -> (m, 8) affine.  Host code on the calling thread: no GPU, no engine lock."""
    points = np.zeros((0, 8), dtype=np.uint64) if points is None else _u64(points).reshape(-1, 8)
    t = points.shape[0]
    if addends is not None:
        addends = _u64(addends).reshape(-1, 12)
        m = addends.shape[0] if m is None else m
        if addends.shape[0] != m:
            raise ValueError("g1_linear_combinations: %d addends for %d sums" % (addends.shape[0], m))
    scalars = _u64(scalars).reshape(-1, 4) if t else np.zeros((0, 4), dtype=np.uint64)
    if m is None:
        m = scalars.shape[0] // t if t else 0
    if scalars.shape[0] != m * t:
        raise ValueError("g1_linear_combinations: %d scalars for %d sums of %d terms" % (scalars.shape[0], m, t))
    out = np.zeros((m, 8), dtype=np.uint64)
    _check(lib().h2hip_g1_linear_combinations_bn254(None if addends is None else _p(addends), _p(scalars) if m * t else None,
                                                    _p(points) if t else None, m, t, _p(out) if m else None),
           "h2hip_g1_linear_combinations_bn254")
    return out


def g1_linear_combinations(addends, scalars, points):
    """out[j] = addends[j] + sum_i [scalars[j][i]] points[i] on the host (include/halo2hip_g1.h).  addends: the engine's Jacobian sums
    ((m, 12) uint64, or a list of (12,) arrays) or None; scalars: m rows of t integers; points: t affine integer pairs (None: the
    identity).  Returns m affine integer pairs, None for the identity, as transcript.write_point takes them."""
    rows = [list(row) for row in scalars]
    t = len(points)
    if any(len(row) != t for row in rows):
        raise ValueError("g1_linear_combinations: every row of scalars has one scalar per point")
    if addends is not None:
        addends = np.stack([_u64(a).reshape(12) for a in addends]) if len(addends) else np.zeros((0, 12), dtype=np.uint64)
    m = len(rows) if addends is None or t else addends.shape[0]
    limbs = np.stack([fr_from_int(s) for row in rows for s in row]) if m * t else np.zeros((0, 4), dtype=np.uint64)
    pts = np.stack([g1_from_int(p) for p in points]) if t else None
    return [g1_to_int(row) for row in g1_linear_combinations_limbs(addends, limbs, pts, m)]

# ------------------------------------------------------------------ grand products (permutation / lookup arguments), BatchInvert
def _cols(arrays, n, what):
    out = []
    for a in arrays:
        a = _u64(a, 4)
        if a.shape[0] != n:
            raise ValueError("%s: expected %d rows, got %d" % (what, n, a.shape[0]))
        out.append(a)
    return out


def _blinding(blinding, n_out, b):
    if blinding is None:
        return np.zeros((max(1, n_out * b), 4), dtype=np.uint64)
    bl = np.ascontiguousarray(_u64(blinding).reshape(-1, 4))
    if bl.shape[0] != n_out * b:
        raise ValueError("blinding: expected %d values (%d outputs x %d), got %d" % (n_out * b, n_out, b, bl.shape[0]))
    return bl if bl.shape[0] else np.zeros((1, 4), dtype=np.uint64)


def permutation_products(k, omega, delta, beta, gamma, columns, permutations, chunk_len, blinding, blinding_factors):
    """permutation::Argument::commit's z columns (permutation/prover.rs:96-166): columns[c] / permutations[c] are (2^k, 4) uint64
    Lagrange columns p_c / s_c; blinding is (n_sets * blinding_factors, 4), the caller's values for rows 2^k - b .. 2^k - 1 of each set.
    Returns the list of n_sets = ceil(len(columns) / chunk_len) columns z_t, (2^k, 4) uint64 each."""
    n = 1 << int(k)
    cols = _cols(columns, n, "columns")
    perms = _cols(permutations, n, "permutations")
    if len(cols) != len(perms):
        raise ValueError("columns and permutations differ in length")
    n_sets = -(-len(cols) // int(chunk_len)) if chunk_len else 0
    bl = _blinding(blinding, n_sets, int(blinding_factors))
    z = [np.zeros((n, 4), dtype=np.uint64) for _ in range(n_sets)]
    _check(lib().h2hip_permutation_products_bn254(k, _p(_fe(omega)), _p(_fe(delta)), _p(_fe(beta)), _p(_fe(gamma)),
                                                  _host_ptrs(cols), _host_ptrs(perms), len(cols), chunk_len,
                                                  _p(bl), blinding_factors, _host_ptrs(z)),
           "h2hip_permutation_products_bn254")
    return z


def lookup_products(k, beta, gamma, compressed_inputs, compressed_tables, permuted_inputs, permuted_tables, blinding, blinding_factors):
    """lookup::Permuted::commit_product's z columns (lookup/prover.rs:194-249), one per lookup: lists of (2^k, 4) uint64 columns A, S, A', S';
    blinding is (count * blinding_factors, 4).  Returns the list of z columns."""
    n = 1 << int(k)
    a, s = _cols(compressed_inputs, n, "compressed_inputs"), _cols(compressed_tables, n, "compressed_tables")
    ap, sp = _cols(permuted_inputs, n, "permuted_inputs"), _cols(permuted_tables, n, "permuted_tables")
    count = len(a)
    if not (len(s) == len(ap) == len(sp) == count):
        raise ValueError("lookup columns differ in count")
    bl = _blinding(blinding, count, int(blinding_factors))
    z = [np.zeros((n, 4), dtype=np.uint64) for _ in range(count)]
    _check(lib().h2hip_lookup_products_bn254(k, _p(_fe(beta)), _p(_fe(gamma)), _host_ptrs(a), _host_ptrs(s), _host_ptrs(ap),
                                             _host_ptrs(sp), count, _p(bl), blinding_factors, _host_ptrs(z)),
           "h2hip_lookup_products_bn254")
    return z


def shuffle_products(k, gamma, compressed_inputs, compressed_shuffles, blinding, blinding_factors):
    """shuffle::Argument::commit_product's z columns (upstream PSE halo2; include/halo2hip.h states the definition), one per shuffle:
    lists of (2^k, 4) uint64 compressed columns A, S; blinding is (count * blinding_factors, 4).  Returns the list of z columns."""
    n = 1 << int(k)
    a, s = _cols(compressed_inputs, n, "compressed_inputs"), _cols(compressed_shuffles, n, "compressed_shuffles")
    count = len(a)
    if len(s) != count:
        raise ValueError("shuffle columns differ in count")
    bl = _blinding(blinding, count, int(blinding_factors))
    z = [np.zeros((n, 4), dtype=np.uint64) for _ in range(count)]
    _check(lib().h2hip_shuffle_products_bn254(k, _p(_fe(gamma)), _host_ptrs(a), _host_ptrs(s), count, _p(bl),
                                              blinding_factors, _host_ptrs(z)), "h2hip_shuffle_products_bn254")
    return z


def batch_invert(a):
    """ff's BatchInvert on a (n, 4) uint64 array of Montgomery Fr elements: a new array of the inverses, zeros stay zero"""
    out = _u64(a, 4).copy()
    _check(lib().h2hip_batch_invert_bn254_fr(_p(out), out.shape[0]), "h2hip_batch_invert_bn254_fr")
    return out


# ------------------------------------------------------------------ lookup compression and permutation (commit_permuted)
H2HIP_ELOOKUP = 4


class H2HipLookupError(H2HipError):
    """H2HIP_ELOOKUP: a lookup's input holds a value its table lacks (the reference's Error::ConstraintSystemFailure)"""


def _check_lookup(rc, what):
    if rc == H2HIP_ELOOKUP:
        raise H2HipLookupError("%s failed (rc=%d): %s" % (what, rc, lib().h2hip_last_error().decode()))
    _check(rc, what)


def _lookup_challenges(challenges):
    ch = np.ascontiguousarray(np.asarray(challenges, dtype=np.uint64).reshape(-1, 4)) if len(challenges) else np.zeros((0, 4), dtype=np.uint64)
    return (ch if ch.shape[0] else np.zeros((1, 4), dtype=np.uint64)), ch.shape[0]


def lookup_compress(k, graphs, theta, fixed=(), advice=(), instance=(), challenges=()):
    """commit_permuted's compressed expressions (lookup/prover.rs:90-115): graphs are flattened compression graphs
    (evaluation.lookup_compress_graphs), columns (2^k, 4) uint64 Lagrange values.  Returns one (2^k, 4) column per graph."""
    n = 1 << int(k)
    fx, ad, ins = _cols(fixed, n, "fixed"), _cols(advice, n, "advice"), _cols(instance, n, "instance")
    from .evaluation import graph_array
    arr, keep = graph_array(graphs)
    ch, n_ch = _lookup_challenges(challenges)
    out = [np.zeros((n, 4), dtype=np.uint64) for _ in graphs]
    _check(lib().h2hip_lookup_compress_bn254(k, _host_ptrs(fx), len(fx), _host_ptrs(ad), len(ad),
                                             _host_ptrs(ins), len(ins), _p(ch), n_ch, _p(_fe(theta)), arr,
                                             len(graphs), _host_ptrs(out)), "h2hip_lookup_compress_bn254")
    del keep
    return out


def _lookup_blinding(blinding, count, b):
    bl = np.ascontiguousarray(_u64(blinding).reshape(-1, 4)) if blinding is not None else np.zeros((0, 4), dtype=np.uint64)
    if bl.shape[0] != count * 2 * (b + 1):
        raise ValueError("blinding: expected %d values (%d lookups x 2(b + 1)), got %d" % (count * 2 * (b + 1), count, bl.shape[0]))
    return bl if bl.shape[0] else np.zeros((1, 4), dtype=np.uint64)


def lookup_permute(k, compressed_inputs, compressed_tables, blinding, blinding_factors):
    """permute_expression_pair (lookup/prover.rs:391-475) for every lookup: lists of (2^k, 4) uint64 compressed columns; blinding is
    (count * 2(b + 1), 4): per lookup the A' rows u .. n - 1, then the S' rows.  Returns (permuted_inputs, permuted_tables).
    Raises H2HipLookupError when an input value is missing from its table."""
    n = 1 << int(k)
    a, t = _cols(compressed_inputs, n, "compressed_inputs"), _cols(compressed_tables, n, "compressed_tables")
    if len(a) != len(t):
        raise ValueError("compressed inputs and tables differ in count")
    bl = _lookup_blinding(blinding, len(a), int(blinding_factors))
    pa = [np.zeros((n, 4), dtype=np.uint64) for _ in a]
    pt = [np.zeros((n, 4), dtype=np.uint64) for _ in a]
    _check_lookup(lib().h2hip_lookup_permute_bn254(k, _host_ptrs(a), _host_ptrs(t), len(a), _p(bl),
                                                   blinding_factors, _host_ptrs(pa), _host_ptrs(pt)), "h2hip_lookup_permute_bn254")
    return pa, pt


def commit_permuted(params, domain, lookups, theta, blinding, blinding_factors, blinds, fixed=(), advice=(), instance=(), challenges=()):
    """lookup::Argument::commit_permuted (lookup/prover.rs:64-170) for every lookup of one instance, in the reference's order:
    compress the input and table expressions (:90-115), permute them (:118-126), commit A' then S' in Lagrange form with the caller's
    blinds (:129-135; two per lookup, blinds[2j], blinds[2j + 1]), and take both to coefficient form (:137-143), batched.  lookups:
    [(input_exprs, table_exprs)] expression tuples (evaluation.py); blinding as for lookup_permute.  Returns one dict per lookup:
    permuted_input / permuted_table (Lagrange), permuted_input_poly / permuted_table_poly (coefficients), and the two commitments
    (Jacobian (12,) uint64; ParamsKZG's commit ignores the blind, as the reference's KZG commit_lagrange does)."""
    from .evaluation import flatten_graph, lookup_compress_graphs
    k = int(domain.k)
    graphs = []
    for inp, tab in lookups:
        gi, gt = lookup_compress_graphs(inp, tab)
        graphs += [flatten_graph(gi), flatten_graph(gt)]
    comp = lookup_compress(k, graphs, theta, fixed, advice, instance, challenges)
    pa, pt = lookup_permute(k, comp[0::2], comp[1::2], blinding, blinding_factors)
    if len(blinds) != 2 * len(lookups):
        raise ValueError("blinds: expected two per lookup")
    out = []
    for j in range(len(lookups)):
        out.append({"compressed_input": comp[2 * j], "compressed_table": comp[2 * j + 1], "permuted_input": pa[j], "permuted_table": pt[j],
                    "permuted_input_commitment": params.commit_lagrange(pa[j], blinds[2 * j]),
                    "permuted_table_commitment": params.commit_lagrange(pt[j], blinds[2 * j + 1])})
    polys = domain.lagrange_to_coeff_batch([c for j in range(len(lookups)) for c in (pa[j], pt[j])])
    for j, d in enumerate(out):
        d["permuted_input_poly"], d["permuted_table_poly"] = polys[2 * j], polys[2 * j + 1]
    return out


def commit_shuffle_products(params, domain, shuffles, theta, gamma, blinding, blinding_factors, blinds, fixed=(), advice=(), instance=(),
                            challenges=()):
    """shuffle::Argument::commit_product (upstream PSE halo2) for every shuffle of one instance, composed as commit_permuted is:
    compress the input and shuffle expressions with theta, build the grand product z with gamma, commit z in Lagrange form with the
    caller's blind (blinds[j]) and take it to coefficient form, batched.  shuffles: [(input_exprs, shuffle_exprs)] expression tuples;
    blinding as for shuffle_products.  Returns one dict per shuffle: compressed_input / compressed_shuffle, product (Lagrange),
    product_poly (coefficients) and product_commitment (Jacobian (12,) uint64)."""
    from .evaluation import flatten_graph, lookup_compress_graphs
    k = int(domain.k)
    graphs = []
    for inp, shf in shuffles:
        gi, gs = lookup_compress_graphs(inp, shf)
        graphs += [flatten_graph(gi), flatten_graph(gs)]
    comp = lookup_compress(k, graphs, theta, fixed, advice, instance, challenges)
    z = shuffle_products(k, gamma, comp[0::2], comp[1::2], blinding, blinding_factors)
    if len(blinds) != len(shuffles):
        raise ValueError("blinds: expected one per shuffle")
    polys = domain.lagrange_to_coeff_batch(z)
    return [{"compressed_input": comp[2 * j], "compressed_shuffle": comp[2 * j + 1], "product": z[j], "product_poly": polys[j],
             "product_commitment": params.commit_lagrange(z[j], blinds[j])} for j in range(len(shuffles))]


def _mv_inputs(compressed_inputs, n, count):
    """the flat, argument-major input table of the mv-lookup calls: one list of columns per argument -> (columns, n_inputs array)"""
    if len(compressed_inputs) != count:
        raise ValueError("mvlookup: %d input lists for %d tables" % (len(compressed_inputs), count))
    flat = [c for cols in compressed_inputs for c in cols]
    n_in = np.array([len(cols) for cols in compressed_inputs] or [0], dtype=np.uint32)
    return (_cols(flat, n, "compressed_inputs") if n is not None else flat), n_in


def mvlookup_multiplicities(k, compressed_inputs, compressed_tables, blinding_factors, partial=False):
    """The logUp (mv-lookup) argument's multiplicity columns (include/halo2hip.h states the definition): compressed_inputs[j] is the list
    of argument j's (2^k, 4) uint64 compressed input columns, compressed_tables[j] its table.  Returns the list of m columns, Montgomery
    form.  Raises H2HipLookupError when an input value is missing from its table -- unless partial=True, which returns (m, message or
    None): the engine writes the counts of the values it found either way."""
    n = 1 << int(k)
    t = _cols(compressed_tables, n, "compressed_tables")
    f, n_in = _mv_inputs(compressed_inputs, n, len(t))
    m = [np.zeros((n, 4), dtype=np.uint64) for _ in t]
    rc = lib().h2hip_mvlookup_multiplicities_bn254(k, _host_ptrs(f), _p(n_in), _host_ptrs(t), len(t),
                                                   blinding_factors, _host_ptrs(m))
    if partial and rc == H2HIP_ELOOKUP:
        return m, lib().h2hip_last_error().decode()
    _check_lookup(rc, "h2hip_mvlookup_multiplicities_bn254")
    return (m, None) if partial else m


def mvlookup_sums(k, beta, compressed_inputs, compressed_tables, m, blinding, blinding_factors):
    """The mv-lookup grand sums phi (include/halo2hip.h): inputs and tables as for mvlookup_multiplicities, m their multiplicity columns;
    blinding is (count * blinding_factors, 4).  Returns the list of phi columns."""
    n = 1 << int(k)
    t, mm = _cols(compressed_tables, n, "compressed_tables"), _cols(m, n, "m")
    if len(mm) != len(t):
        raise ValueError("mvlookup: m and tables differ in count")
    f, n_in = _mv_inputs(compressed_inputs, n, len(t))
    bl = _blinding(blinding, len(t), int(blinding_factors))
    phi = [np.zeros((n, 4), dtype=np.uint64) for _ in t]
    _check(lib().h2hip_mvlookup_sums_bn254(k, _p(_fe(beta)), _host_ptrs(f), _p(n_in), _host_ptrs(t), _host_ptrs(mm),
                                           len(t), _p(bl), blinding_factors, _host_ptrs(phi)),
           "h2hip_mvlookup_sums_bn254")
    return phi


def mvlookup_sum_rows(k, blinding_factors, count):
    """test hook: the rows one thread of the grand sum's scan takes in a call of `count` arguments (the code's own rule; no GPU)"""
    out = ctypes.c_uint32(0)
    _check(lib().h2hip_debug_mvlookup_sum_rows(k, blinding_factors, count, ctypes.byref(out)),
           "h2hip_debug_mvlookup_sum_rows")
    return out.value


def commit_mvlookup(params, domain, lookups, theta, beta, blinding, blinding_factors, blinds, fixed=(), advice=(), instance=(), challenges=()):
    """The mv-lookup prover steps for every argument of one instance, composed as commit_permuted is: compress every input tuple and the
    table tuple with theta, count the multiplicities, commit m in Lagrange form, build the grand sum phi with beta, commit phi, and
    take both to coefficient form, batched.  lookups: [([input_exprs, ...], table_exprs)] expression tuples, several inputs sharing one
    table; blinding as for mvlookup_sums (phi's rows); blinds[2j], blinds[2j + 1] the blinds of m_j and phi_j.  Returns one dict per
    argument: compressed_inputs / compressed_table, m / phi (Lagrange), m_poly / phi_poly (coefficients), m_commitment / phi_commitment."""
    from .evaluation import flatten_graph, lookup_compress_graphs
    k = int(domain.k)
    graphs, n_in = [], []
    for inputs, tab in lookups:
        for inp in inputs:
            graphs.append(flatten_graph(lookup_compress_graphs(inp, tab)[0]))
        graphs.append(flatten_graph(lookup_compress_graphs(inputs[0], tab)[1]))
        n_in.append(len(inputs))
    comp = lookup_compress(k, graphs, theta, fixed, advice, instance, challenges)
    f, t, at = [], [], 0
    for kj in n_in:
        f.append(comp[at:at + kj])
        t.append(comp[at + kj])
        at += kj + 1
    if len(blinds) != 2 * len(lookups):
        raise ValueError("blinds: expected two per argument")
    m = mvlookup_multiplicities(k, f, t, blinding_factors)
    m_commit = [params.commit_lagrange(m[j], blinds[2 * j]) for j in range(len(lookups))]
    phi = mvlookup_sums(k, beta, f, t, m, blinding, blinding_factors)
    polys = domain.lagrange_to_coeff_batch([c for j in range(len(lookups)) for c in (m[j], phi[j])])
    return [{"compressed_inputs": f[j], "compressed_table": t[j], "m": m[j], "phi": phi[j], "m_poly": polys[2 * j], "phi_poly": polys[2 * j + 1],
             "m_commitment": m_commit[j], "phi_commitment": params.commit_lagrange(phi[j], blinds[2 * j + 1])} for j in range(len(lookups))]


# ------------------------------------------------------------------ witness check: MockProver::verify's three column-wide loops
def _check_out(items, max_rows):
    max_rows = int(max_rows)
    counts = np.zeros(max(1, items), dtype=np.uint64)
    rows = np.full((max(1, items), max(1, max_rows)), 0xFFFFFFFF, dtype=np.uint32)
    return counts, rows, (_p(rows) if max_rows else None)


def _check_result(counts, rows, items, max_rows):
    return counts[:items], rows[:items, :int(max_rows)]


def check_gates(k, graphs, fixed=(), advice=(), instance=(), challenges=(), max_rows=16):
    """MockProver::verify's gate loop (dev.rs:676-746) over all 2^k rows: graphs are flattened evaluation.gate_check_graphs, columns
    (2^k, 4) uint64 Lagrange values.  Returns (counts, rows): counts[g] rows fail polynomial g, rows[g] holds the lowest max_rows of
    them in ascending order, then 0xFFFFFFFF."""
    n = 1 << int(k)
    fx, ad, ins = _cols(fixed, n, "fixed"), _cols(advice, n, "advice"), _cols(instance, n, "instance")
    from .evaluation import graph_array
    arr, keep = graph_array(graphs)
    ch, n_ch = _lookup_challenges(challenges)
    counts, rows, prow = _check_out(len(graphs), max_rows)
    _check(lib().h2hip_check_gates_bn254(k, _host_ptrs(fx), len(fx), _host_ptrs(ad), len(ad),
                                         _host_ptrs(ins), len(ins), _p(ch), n_ch, arr,
                                         len(graphs), max_rows, _p(counts), prow), "h2hip_check_gates_bn254")
    del keep
    return _check_result(counts, rows, len(graphs), max_rows)


def _check_mapping(mapping, n):
    mp = np.ascontiguousarray(mapping, dtype=np.uint32)
    if mp.ndim != 3 or mp.shape[1:] != (n, 2):
        raise ValueError("mapping: expected shape (m, %d, 2), got %s" % (n, mp.shape))
    return mp


def check_permutation(k, columns, mapping, max_rows=16):
    """MockProver::verify's copy-constraint loop (dev.rs:889-931): columns are the permutation argument's (2^k, 4) uint64 Lagrange
    columns, mapping the Assembly's (m, 2^k, 2) uint32 (column, row) pairs.  Returns (counts, rows) per column as check_gates does."""
    n = 1 << int(k)
    cols = _cols(columns, n, "columns")
    mp = _check_mapping(mapping, n)
    if mp.shape[0] != len(cols):
        raise ValueError("columns and mapping differ in count")
    maps = [mp[j] for j in range(len(cols))]
    counts, rows, prow = _check_out(len(cols), max_rows)
    _check(lib().h2hip_check_permutation_bn254(k, _host_ptrs(cols), _host_ptrs(maps), len(cols),
                                               max_rows, _p(counts), prow), "h2hip_check_permutation_bn254")
    return _check_result(counts, rows, len(cols), max_rows)


def check_lookups(k, compressed_inputs, compressed_tables, blinding_factors, max_rows=16):
    """MockProver::verify's lookup loop (dev.rs:751-886) on compressed columns (lookup_compress): input rows below u = 2^k -
    blinding_factors - 1 whose value no table row below u holds.  Returns (counts, rows) per lookup as check_gates does."""
    n = 1 << int(k)
    a, t = _cols(compressed_inputs, n, "compressed_inputs"), _cols(compressed_tables, n, "compressed_tables")
    if len(a) != len(t):
        raise ValueError("compressed inputs and tables differ in count")
    counts, rows, prow = _check_out(len(a), max_rows)
    _check(lib().h2hip_check_lookups_bn254(k, _host_ptrs(a), _host_ptrs(t), len(a),
                                           blinding_factors, max_rows, _p(counts), prow),
           "h2hip_check_lookups_bn254")
    return _check_result(counts, rows, len(a), max_rows)


def check_shuffles(k, compressed_inputs, compressed_shuffles, blinding_factors, max_rows=16):
    """The shuffle argument's witness check on compressed columns (lookup_compress): input rows below u = 2^k - blinding_factors - 1
    whose value occurs a different number of times among the input rows below u than among the shuffle rows below u.  Returns
    (counts, rows) per shuffle as check_gates does."""
    n = 1 << int(k)
    a, s = _cols(compressed_inputs, n, "compressed_inputs"), _cols(compressed_shuffles, n, "compressed_shuffles")
    if len(a) != len(s):
        raise ValueError("compressed inputs and shuffles differ in count")
    counts, rows, prow = _check_out(len(a), max_rows)
    _check(lib().h2hip_check_shuffles_bn254(k, _host_ptrs(a), _host_ptrs(s), len(a),
                                            blinding_factors, max_rows, _p(counts), prow),
           "h2hip_check_shuffles_bn254")
    return _check_result(counts, rows, len(a), max_rows)


def _failures(kind, counts, rows):
    return [(kind, j, int(r)) for j in range(len(counts)) for r in rows[j][:min(int(counts[j]), rows.shape[1])]]


def verify_witness(k, gate_polys, lookups, theta, blinding_factors, permutation_columns, mapping, fixed=(), advice=(), instance=(),
                   challenges=(), max_rows=64, shuffles=(), mvlookups=(), copies=None):
    """The three column-wide loops of MockProver::verify over one instance's columns: gate_polys are expression tuples (evaluation.py;
    every gate's polynomials in cs.gates order), lookups [(input_exprs, table_exprs)], compressed here with the caller's theta;
    permutation_columns [(kind, index)] with kind 'advice' / 'fixed' / 'instance' names the permutation argument's columns, mapping its
    Assembly's (m, 2^k, 2) uint32 pairs (None, or m = 0: no copy constraint).  Challenges and theta are the caller's: the engine draws
    nothing.  Returns the failures as ("gate", graph_index, row), ("lookup", lookup_index, row), ("permutation", column, row) tuples in
    verify's order (dev.rs:933-938), at most the max_rows lowest rows of each constraint; an empty list is a satisfied witness.
    shuffles [(input_exprs, shuffle_exprs)] (the argument of upstream PSE halo2) are compressed with the same theta and reported as
    ("shuffle", shuffle_index, row) after the lookups; the default checks none.  mvlookups [([input_exprs, ...], table_exprs)] (the
    logUp argument) go through the lookup check with the table repeated per input tuple and are reported after the shuffles as
    ("mvlookup", input_index, row), the input tuples counted over all arguments in order.  copies (a (C, 4) array or a CopyList) stands
    in for mapping, which is then None: the copy constraints themselves, turned into the ordered mapping by permutation_mapping."""
    from .evaluation import flatten_graph, gate_check_graphs, lookup_compress_graphs
    k = int(k)
    if copies is not None:
        if mapping is not None:
            raise ValueError("verify_witness: give mapping or copies, not both")
        if len(permutation_columns):
            mapping = permutation_mapping(k, len(permutation_columns), copies.array() if isinstance(copies, CopyList) else copies)
    out = []
    graphs = [flatten_graph(g) for g in gate_check_graphs(gate_polys)]
    if graphs:
        out += _failures("gate", *check_gates(k, graphs, fixed, advice, instance, challenges, max_rows))
    lg = []
    for inp, tab in lookups:
        gi, gt = lookup_compress_graphs(inp, tab)
        lg += [flatten_graph(gi), flatten_graph(gt)]
    if lg:
        comp = lookup_compress(k, lg, theta, fixed, advice, instance, challenges)
        out += _failures("lookup", *check_lookups(k, comp[0::2], comp[1::2], blinding_factors, max_rows))
    sg = []
    for inp, shf in shuffles:
        gi, gs = lookup_compress_graphs(inp, shf)
        sg += [flatten_graph(gi), flatten_graph(gs)]
    if sg:
        comp = lookup_compress(k, sg, theta, fixed, advice, instance, challenges)
        out += _failures("shuffle", *check_shuffles(k, comp[0::2], comp[1::2], blinding_factors, max_rows))
    mg, pairs = [], []  # pairs: (graph of an input tuple, graph of its argument's table) as indices into mg
    for inputs, tab in mvlookups:
        first = len(mg)
        mg += [flatten_graph(lookup_compress_graphs(inp, tab)[0]) for inp in inputs]
        mg.append(flatten_graph(lookup_compress_graphs(inputs[0], tab)[1]))
        pairs += [(first + t, len(mg) - 1) for t in range(len(inputs))]
    if mg:
        comp = lookup_compress(k, mg, theta, fixed, advice, instance, challenges)
        out += _failures("mvlookup", *check_lookups(k, [comp[i] for i, _ in pairs], [comp[t] for _, t in pairs], blinding_factors, max_rows))
    if mapping is not None and len(permutation_columns):
        pools = {"advice": advice, "fixed": fixed, "instance": instance}
        cols = [pools[kind][int(i)] for kind, i in permutation_columns]
        out += _failures("permutation", *check_permutation(k, cols, mapping, max_rows))
    return out


# ------------------------------------------------------------------ keygen: permutation key, batch_invert_assigned, l0 / l_last / l_active_row
FR_DELTA = pow(7, 1 << FR_S, FR_MODULUS)  # Fr::DELTA = MULTIPLICATIVE_GENERATOR^(2^S)


class PermutationAssembly:
    """permutation::keygen::Assembly (plonk/permutation/keygen.rs:16-103), a literal host port: `mapping`, `aux` and `sizes`, and
    `copy` merging the smaller cycle into the larger.  Columns are the permutation argument's column indices 0 .. n_columns - 1."""

    def __init__(self, n, n_columns):
        self.n, self.n_columns = int(n), int(n_columns)
        ident = np.zeros((self.n_columns, self.n, 2), dtype=np.uint32)         # :31-35: (i, j) for column i, row j
        ident[:, :, 0] = np.arange(self.n_columns, dtype=np.uint32)[:, None]
        ident[:, :, 1] = np.arange(self.n, dtype=np.uint32)[None, :]
        self.mapping = ident                                                   # :42
        self.aux = ident.copy()                                                # :43
        self.sizes = np.ones((self.n_columns, self.n), dtype=np.int64)         # :44

    def copy(self, left_column, left_row, right_column, right_row):
        lc, lr, rc, rr = int(left_column), int(left_row), int(right_column), int(right_row)
        if not (0 <= lc < self.n_columns and 0 <= rc < self.n_columns):        # :55-64 ColumnNotInPermutation
            raise ValueError("column not in the permutation")
        if not (0 <= lr < self.n and 0 <= rr < self.n):                        # :67-71 BoundsFailure
            raise ValueError("row out of bounds")
        mapping, aux, sizes = self.mapping, self.aux, self.sizes
        left = (int(aux[lc, lr, 0]), int(aux[lc, lr, 1]))                      # :75-76
        right = (int(aux[rc, rr, 0]), int(aux[rc, rr, 1]))
        if left == right:                                                      # :79-81
            return
        if sizes[left] < sizes[right]:                                         # :83-85
            left, right = right, left
        sizes[left] += sizes[right]                                            # :88
        i = right                                                              # :89-96
        while True:
            aux[i[0], i[1]] = left
            i = (int(mapping[i[0], i[1], 0]), int(mapping[i[0], i[1], 1]))
            if i == right:
                break
        tmp = mapping[lc, lr].copy()                                           # :98-100: the cells named in the call
        mapping[lc, lr] = mapping[rc, rr]
        mapping[rc, rr] = tmp


def _copies_array(copies):
    c = np.ascontiguousarray(np.asarray(copies, dtype=np.uint32).reshape(-1, 4))
    return c if c.shape[0] else np.zeros((0, 4), dtype=np.uint32)


def permutation_mapping(k, n_columns, copies):
    """The ordered permutation mapping of a circuit's copy constraints (include/halo2hip.h, "permutation mapping from copy
    constraints"): copies is a (C, 4) array of (left_column, left_row, right_column, right_row); every cell maps to the next cell of its
    connected component in ascending column * 2^k + row order, the last one to the least.  Returns the (m, 2^k, 2) uint32 array that
    permutation_keygen, check_permutation and verify_witness take.  The same cycles as PermutationAssembly.copy builds for these
    constraints, in an order of its own: valid, not byte-identical."""
    k, m = int(k), int(n_columns)
    c = _copies_array(copies)
    if not (0 <= k < 1 << 32 and 0 <= m < 1 << 32):
        raise ValueError("k and n_columns must fit 32 bits")
    # arguments beyond the limits go to the library, which names the limit: it reads no table then, so none of that size is made
    within = k <= 28 and m <= 65535 and (m << k) <= 1 << 32
    out = np.zeros((m, 1 << k, 2) if within else (min(m, 65536), 1, 2), dtype=np.uint32)
    _check(lib().h2hip_permutation_mapping(k, m, _p(c) if c.shape[0] else None, c.shape[0],
                                           _host_ptrs([out[j] for j in range(out.shape[0])])), "h2hip_permutation_mapping")
    return out


class CopyList:
    """The copy constraints of a circuit, recorded: `copy` makes PermutationAssembly.copy's column and row checks and appends, and
    `mapping()` builds the ordered mapping on the engine (permutation_mapping).  The order of the calls does not matter."""

    def __init__(self, n, n_columns):
        self.n, self.n_columns = int(n), int(n_columns)
        if self.n < 1 or self.n & (self.n - 1):
            raise ValueError("n must be a power of two")
        self.copies = []

    def copy(self, left_column, left_row, right_column, right_row):
        lc, lr, rc, rr = int(left_column), int(left_row), int(right_column), int(right_row)
        if not (0 <= lc < self.n_columns and 0 <= rc < self.n_columns):
            raise ValueError("column not in the permutation")
        if not (0 <= lr < self.n and 0 <= rr < self.n):
            raise ValueError("row out of bounds")
        self.copies.append((lc, lr, rc, rr))

    def array(self):
        return _copies_array(self.copies)

    def mapping(self):
        return permutation_mapping(self.n.bit_length() - 1, self.n_columns, self.array())


def _domain_args(domain):
    return (domain.k, _p(domain.omega), _p(domain.omega_inv), _p(domain.ifft_divisor), domain.extended_k,
            _p(domain.extended_omega), _p(domain.g_coset), _p(domain.g_coset_inv))


_KEYGEN_FORMS = ("permutations", "polys", "cosets")


def _keygen_want(want):
    want = tuple(want)
    for w in want:
        if w not in _KEYGEN_FORMS:
            raise ValueError("want: unknown form %r" % (w,))
    return want


def permutation_keygen(domain, mapping, want=_KEYGEN_FORMS, delta=None):
    """Assembly::build_vk / build_pk's columns (plonk/permutation/keygen.rs:105-242) from `mapping`, an (m, 2^k, 2) uint32 array of
    (column, row) pairs: a dict with the forms named in `want`, each a list of m columns -- permutations (2^k, 4), polys (2^k, 4),
    cosets (2^extended_k, 4).  delta defaults to Fr::DELTA."""
    want = _keygen_want(want)
    mp = np.ascontiguousarray(mapping, dtype=np.uint32)
    n = 1 << int(domain.k)
    if mp.ndim != 3 or mp.shape[1:] != (n, 2):
        raise ValueError("mapping: expected shape (m, %d, 2), got %s" % (n, mp.shape))
    m = mp.shape[0]
    rows = [mp[j] for j in range(m)]
    sizes = {"permutations": n, "polys": n, "cosets": domain.extended_len()}
    out = {w: [np.zeros((sizes[w], 4), dtype=np.uint64) for _ in range(m)] for w in want}
    tabs = [(_host_ptrs(out[w]) if w in out else None) for w in _KEYGEN_FORMS]
    d = fr_from_int(FR_DELTA) if delta is None else _fe(delta)
    _check(lib().h2hip_permutation_keygen_bn254(*_domain_args(domain), _p(d), _host_ptrs(rows), m, *tabs),
           "h2hip_permutation_keygen_bn254")
    return out


def _assigned_args(rat_rows, rat_denoms, m):
    rat_rows = [None] * m if rat_rows is None else list(rat_rows)
    rat_denoms = [None] * m if rat_denoms is None else list(rat_denoms)
    if len(rat_rows) != m or len(rat_denoms) != m:
        raise ValueError("rat_rows / rat_denoms: one entry per column")
    return rat_rows, rat_denoms


def batch_invert_assigned(k, numerators, rat_rows=None, rat_denoms=None, in_place=False):
    """batch_invert_assigned (poly.rs:180-209): numerators[j] (2^k, 4); rat_rows[j] the ascending uint32 rows of column j's Rational
    cells and rat_denoms[j] (count, 4) their denominators (None: none).  Returns the list of inverted columns; with in_place the
    numerators (contiguous uint64 arrays) are overwritten and returned (out == numerators at the ABI)."""
    n = 1 << int(k)
    nums = _cols(numerators, n, "numerators")
    m = len(nums)
    rat_rows, rat_denoms = _assigned_args(rat_rows, rat_denoms, m)
    rows, dens, counts = [], [], []
    for j in range(m):
        r = np.zeros(0, dtype=np.uint32) if rat_rows[j] is None else np.ascontiguousarray(rat_rows[j], dtype=np.uint32).reshape(-1)
        dn = np.zeros((0, 4), dtype=np.uint64) if rat_denoms[j] is None else np.ascontiguousarray(_u64(rat_denoms[j]).reshape(-1, 4))
        if r.shape[0] != dn.shape[0]:
            raise ValueError("column %d: %d rows but %d denominators" % (j, r.shape[0], dn.shape[0]))
        rows.append(r)
        dens.append(dn)
        counts.append(r.shape[0])
    if in_place:
        if any(a is not b for a, b in zip(nums, numerators)):
            raise ValueError("in_place needs contiguous uint64 numerators")
        outs = nums
    else:
        outs = [np.zeros((n, 4), dtype=np.uint64) for _ in range(m)]
    rp = (ctypes.c_void_p * max(1, m))(*[(r.ctypes.data if r.shape[0] else None) for r in rows])
    dp = (ctypes.c_void_p * max(1, m))(*[(d.ctypes.data if d.shape[0] else None) for d in dens])
    cnt = (ctypes.c_size_t * max(1, m))(*counts)
    _check(lib().h2hip_batch_invert_assigned_bn254(k, _host_ptrs(nums), rp, cnt, dp, m, _host_ptrs(outs)),
           "h2hip_batch_invert_assigned_bn254")
    return outs


def key_lagrange_columns(domain, blinding_factors):
    """pk.l0, pk.l_last, pk.l_active_row (plonk/keygen.rs:320-351): three (2^extended_k, 4) columns"""
    cols = [np.zeros((domain.extended_len(), 4), dtype=np.uint64) for _ in range(3)]
    _check(lib().h2hip_key_lagrange_columns_bn254(domain.k, _p(domain.omega_inv), _p(domain.ifft_divisor),
                                                  domain.extended_k, _p(domain.extended_omega), _p(domain.g_coset),
                                                  _p(domain.g_coset_inv), blinding_factors, _p(cols[0]), _p(cols[1]), _p(cols[2])),
           "h2hip_key_lagrange_columns_bn254")
    return tuple(cols)


def keygen_columns(params, domain, fixed, mapping, blinding_factors, delta=None, copies=None):
    """The columns of keygen_vk + keygen_pk (plonk/keygen.rs:203-367) that are data-parallel, composed from the calls above: `fixed` is
    a list of (2^k, 4) Lagrange columns (batch_invert_assigned and compress_selectors applied), or of
    (numerators, rat_rows, rat_denoms) triples, which are inverted here (:298); mapping is the assembly's.  Returns a dict under the names
    evaluation.py's describe() takes -- fixed_cosets, perm_cosets, l0, l_last, l_active_row -- plus fixed_values, fixed_polys,
    fixed_commitments, permutations (the list permutation_products takes), perm_polys, permutation_commitments (Jacobian (12,) uint64).
    copies (a CopyList, or an (n_columns, (C, 4) array) pair) stands in for mapping, which is then None: the permutation's columns come
    from permutation_keygen_from_copies, and the key is valid for the circuit, not byte-identical to the reference's."""
    k, n = int(domain.k), 1 << int(domain.k)
    if copies is not None and mapping is not None:
        raise ValueError("keygen_columns: give mapping or copies, not both")
    fixed = list(fixed)
    if fixed and isinstance(fixed[0], tuple):
        fixed_values = batch_invert_assigned(k, [f[0] for f in fixed], [f[1] for f in fixed], [f[2] for f in fixed])
    else:
        fixed_values = _cols(fixed, n, "fixed")
    fixed_polys = domain.lagrange_to_coeff_batch(fixed_values)                      # :306-309
    fixed_cosets = domain.coeff_to_extended_batch(fixed_polys)                      # :311-314
    if copies is None:
        perm = permutation_keygen(domain, mapping, delta=delta)                     # :316-318
    else:
        m_c, cp = (copies.n_columns, copies.array()) if isinstance(copies, CopyList) else copies
        perm = permutation_keygen_from_copies(domain, m_c, cp, delta=delta)
    l0, l_last, l_active_row = key_lagrange_columns(domain, blinding_factors)       # :320-351
    commit = lambda cols: list(best_multiexp_batch(cols, params.g_lagrange)) if cols else []
    return {"fixed_values": fixed_values, "fixed_polys": fixed_polys, "fixed_cosets": fixed_cosets,
            "fixed_commitments": commit(fixed_values),                              # keygen_vk :235-243
            "permutations": perm["permutations"], "perm_polys": perm["polys"], "perm_cosets": perm["cosets"],
            "permutation_commitments": commit(perm["permutations"]),                # build_vk :153-162
            "l0": l0, "l_last": l_last, "l_active_row": l_active_row}


# ------------------------------------------------------------------ opening: query evaluations and the KZG multiopen quotients
def _fes(values, what):
    """a list of field elements ((4,) uint64 Montgomery limbs each) or an (m, 4) array -> a contiguous (max(1, m), 4) array, and m"""
    a = np.ascontiguousarray(np.asarray(values, dtype=np.uint64).reshape(-1, 4)) if len(values) else np.zeros((0, 4), dtype=np.uint64)
    m = a.shape[0]
    return (a if m else np.zeros((1, 4), dtype=np.uint64)), m


def eval_polynomials(polys, query_poly, points):
    """eval_polynomial (arithmetic.rs:304-328) for every query in one call: polys is a list of (len_j, 4) uint64 coefficient arrays,
    query q evaluates polys[query_poly[q]] at points[q].  Returns (n_queries, 4) uint64."""
    ps = [_u64(a, 4) if len(a) else np.zeros((0, 4), dtype=np.uint64) for a in polys]
    lens = (ctypes.c_size_t * max(1, len(ps)))(*[a.shape[0] for a in ps])
    qp = np.ascontiguousarray(query_poly, dtype=np.uint32).reshape(-1)
    pts, nq = _fes(points, "points")
    if qp.shape[0] != nq:
        raise ValueError("query_poly and points differ in length")
    out = np.zeros((max(1, nq), 4), dtype=np.uint64)
    _check(lib().h2hip_eval_polynomials_bn254(_host_ptrs(ps) if ps else None, lens, len(ps), _p(qp if nq else np.zeros(1, np.uint32)),
                                              _p(pts), nq, _p(out)), "h2hip_eval_polynomials_bn254")
    return out[:nq]


def _combine_args(scalars, sub, roots, scale):
    sc, n_sc = _fes(scalars, "scalars")
    sb, n_sub = _fes(sub if sub is not None else [], "sub")
    rt, n_roots = _fes(roots, "roots")
    one = fr_from_int(1)
    sl = _fe(scale if scale is not None else one)
    return sc, n_sc, sb, n_sub, rt, n_roots, sl


def poly_combine(polys, scalars, sub=None, roots=(), scale=None, out=None, accumulate=False, out_len=None, remainder=False):
    """a = sum_j scalars[j] polys[j] - sub, divided by (X - r) for r in roots in order, times scale (h2hip_poly_combine_bn254_fr).
    polys: (L, 4) uint64 arrays of one length; sub: up to min(L, 16) low coefficients.  Without `out` the result is a new (out_len, 4)
    array (out_len defaults to L - len(roots)), zero past L - len(roots); with accumulate=True it is added to `out` in place.
    remainder=True returns (q, a(roots[0]))."""
    ps = [_u64(a, 4) for a in polys]
    L = ps[0].shape[0] if ps else 0
    for a in ps:
        if a.shape[0] != L:
            raise ValueError("poly_combine: polynomials differ in length")
    sc, n_sc, sb, n_sub, rt, n_roots, sl = _combine_args(scalars, sub, roots, scale)
    if n_sc != len(ps):
        raise ValueError("poly_combine: %d scalars for %d polynomials" % (n_sc, len(ps)))
    if out is None:
        out = np.zeros((max(0, L - n_roots) if out_len is None else int(out_len), 4), dtype=np.uint64)
    else:
        assert out.dtype == np.uint64 and out.flags["C_CONTIGUOUS"] and out.ndim == 2 and out.shape[1] == 4
    rem = np.zeros(4, dtype=np.uint64)
    _check(lib().h2hip_poly_combine_bn254_fr(_host_ptrs(ps) if ps else None, L, _p(sc), len(ps), _p(sb),
                                             n_sub, _p(rt), n_roots, _p(sl), 1 if accumulate else 0,
                                             _p(out) if out.shape[0] else None, out.shape[0], _p(rem) if remainder else None),
           "h2hip_poly_combine_bn254_fr")
    return (out, rem) if remainder else out


def kate_division(a, b):
    """arithmetic.rs:348-366: a(X) / (X - b) without the remainder; a is (L, 4) uint64 with L >= 1, the result (L - 1, 4)"""
    return poly_combine([a], [fr_from_int(1)], roots=[b])


def div_by_vanishing(a, roots):
    """shplonk/prover.rs:26-31: kate_division by each root in order; (L - len(roots), 4)"""
    return poly_combine([a], [fr_from_int(1)], roots=list(roots))


def _fr_powers(x, m):
    """powers() (poly/kzg/multiopen/shplonk.rs): 1, x, x^2, ... as integers"""
    out, acc = [], 1
    for _ in range(m):
        out.append(acc)
        acc = acc * x % FR_MODULUS
    return out


def _fr_lagrange_interpolate(points, evals):
    """arithmetic.rs:405-460 on integers: the polynomial of degree < len(points) through (points[i], evals[i])"""
    p, m = FR_MODULUS, len(points)
    final = [0] * m
    for j in range(m):
        basis, denom = [1], 1
        for k in range(m):
            if k == j:
                continue
            basis = [((basis[i - 1] if i else 0) - points[k] * (basis[i] if i < len(basis) else 0)) % p for i in range(len(basis) + 1)]
            denom = denom * (points[j] - points[k]) % p
        f = evals[j] * pow(denom, -1, p) % p
        for i in range(m):
            final[i] = (final[i] + f * basis[i]) % p
    return final


def _fr_eval(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % FR_MODULUS
    return acc


def _fr_vanishing(roots, z):
    """evaluate_vanishing_polynomial (arithmetic.rs): prod (z - r)"""
    acc = 1
    for r in roots:
        acc = acc * (z - r) % FR_MODULUS
    return acc


def _combine_any(polys, scalars, sub=None, roots=(), scale=None, out=None, accumulate=False):
    """poly_combine for host columns, poly_combine_device for torch CUDA tensors (the result a new (L - len(roots), 4) tensor unless
    `out` is given): what lets the multiopen compositions below serve a prover whose polynomials live in HBM"""
    if isinstance(polys[0], np.ndarray):
        return poly_combine(polys, scalars, sub=sub, roots=roots, scale=scale, out=out, accumulate=accumulate)
    import torch
    if out is None:
        L = polys[0].numel() * polys[0].element_size() // 32
        out = torch.zeros((max(0, L - len(roots)), 4), dtype=torch.int64, device=polys[0].device)
    poly_combine_device(polys, scalars, out, sub=sub, roots=roots, scale=scale, accumulate=accumulate)
    return out


def gwc_witnesses(polys, point_groups, v):
    """GWC's witness polynomials (poly/kzg/multiopen/gwc/prover.rs:61-89), one per point, as (n - 1, 4) arrays.  point_groups is
    construct_intermediate_sets' output in order: a list of (point, [(poly index, eval), ...]); evals and challenges are Montgomery limbs.
    polys: numpy arrays, or torch CUDA tensors (the witnesses are then tensors too, queued on the current stream)."""
    vv = fr_to_int(v)
    out = []
    for point, queries in point_groups:
        pw = _fr_powers(vv, len(queries))
        ev = sum(pw[i] * fr_to_int(e) for i, (_, e) in enumerate(queries)) % FR_MODULUS
        out.append(_combine_any([polys[j] for j, _ in queries], [fr_from_int(x) for x in pw], sub=[fr_from_int(ev)], roots=[point]))
    return out


def _shplonk_sets(rotation_sets):
    """(points as integers, [(poly index, [evals as integers])], interpolants) per rotation set"""
    out = []
    for points, commitments in rotation_sets:
        pts = [fr_to_int(x) for x in points]
        coms = [(j, [fr_to_int(e) for e in evs]) for j, evs in commitments]
        out.append((pts, coms, [_fr_lagrange_interpolate(pts, evs) for _, evs in coms]))
    return out


def shplonk_h(polys, rotation_sets, y, v):
    """SHPLONK's first quotient h_x (shplonk/prover.rs:138-203): rotation_sets in construct_intermediate_sets' order, each
    (points, [(poly index, [eval at each point]), ...]); polys are (n, 4) coefficient arrays, or torch CUDA tensors.  Returns h_x, (n, 4)."""
    yy, vv = fr_to_int(y), fr_to_int(v)
    n = polys[0].shape[0]
    if isinstance(polys[0], np.ndarray):
        h = np.zeros((n, 4), dtype=np.uint64)
    else:
        import torch
        h = torch.zeros((n, 4), dtype=torch.int64, device=polys[0].device)
    for i, (pts, coms, interp) in enumerate(_shplonk_sets(rotation_sets)):
        py = _fr_powers(yy, len(coms))
        sub = [sum(py[c] * interp[c][t] for c in range(len(coms))) % FR_MODULUS for t in range(len(pts))]
        _combine_any([polys[j] for j, _ in coms], [fr_from_int(x) for x in py], sub=[fr_from_int(x) for x in sub],
                     roots=[fr_from_int(x) for x in pts], scale=fr_from_int(pow(vv, i, FR_MODULUS)), out=h, accumulate=i > 0)
    return h


def shplonk_final(polys, rotation_sets, h_x, y, v, u):
    """SHPLONK's second quotient (shplonk/prover.rs:209-275): l_x over every polynomial and h_x, divided by (X - u) and normalised by
    z_diffs[0]^-1.  u is drawn by the caller after h_x is committed.  Returns (n - 1, 4)."""
    yy, vv, uu = fr_to_int(y), fr_to_int(v), fr_to_int(u)
    sets = _shplonk_sets(rotation_sets)
    super_set = []
    for pts, _, _ in sets:
        for x in pts:
            if x not in super_set:
                super_set.append(x)
    p = FR_MODULUS
    cols, scal, const, z0 = [], [], 0, None
    for i, (pts, coms, interp) in enumerate(sets):
        z_i = _fr_vanishing([x for x in super_set if x not in pts], uu)
        z0 = z_i if z0 is None else z0
        f = pow(vv, i, p) * z_i % p
        for c, (j, _) in enumerate(coms):
            w = f * pow(yy, c, p) % p
            cols.append(polys[j])
            scal.append(w)
            const = (const + w * _fr_eval(interp[c], uu)) % p
    cols.append(h_x)
    scal.append(-_fr_vanishing(super_set, uu) % p)
    return _combine_any(cols, [fr_from_int(x) for x in scal], sub=[fr_from_int(const)], roots=[u], scale=fr_from_int(pow(z0, -1, p)))




# ------------------------------------------------------------------ poly/domain.rs
class EvaluationDomain:
    """poly::EvaluationDomain<Fr> (poly/domain.rs:18-34): holds the constants `new` computes (:39-142) and routes the
    conversions through the fused device entry points.  `EvaluationDomain.new(j, k)` computes them here with Python
    integers (field inversions are not on the accelerated path)."""

    FIELDS = ("omega", "omega_inv", "extended_omega", "extended_omega_inv", "g_coset", "g_coset_inv",
              "ifft_divisor", "extended_ifft_divisor")

    def __init__(self, k, extended_k, quotient_poly_degree, t_evaluations=None, **consts):
        self.k, self.extended_k, self.quotient_poly_degree = int(k), int(extended_k), int(quotient_poly_degree)
        self.n = 1 << self.k
        for f in self.FIELDS:
            setattr(self, f, _fe(consts[f]))
        self.t_evaluations = None if t_evaluations is None else _u64(t_evaluations, 4)
        self.field = BN254_FR

    def _device_field(self):
        if self.field is not BN254_FR:
            raise H2HipError("the engine transforms bn256::Fr only (domain over %s)" % self.field.name)

    @classmethod
    def new(cls, j, k, field=None):
        """EvaluationDomain::new (poly/domain.rs:39-142), generic over the scalar field as the reference is (`G::Scalar`):
        `field` is a PrimeField (default BN254_FR, the only field the device entry points serve; PASTA_FP exists so that the
        constructor can be checked against the one domain constant the reference's own tests pin, tests/plonk_api.rs:629-632)."""
        field = BN254_FR if field is None else field
        r = field.modulus
        quotient_poly_degree = j - 1                                    # :41
        n = 1 << k                                                      # :44
        extended_k = k                                                  # :49-52
        while (1 << extended_k) < n * quotient_poly_degree:
            extended_k += 1
        if extended_k > field.S:
            raise ValueError("extended_k exceeds the 2-adicity of the field")
        extended_omega = field.root_of_unity                            # :54-61
        for _ in range(extended_k, field.S):
            extended_omega = extended_omega * extended_omega % r
        omega = extended_omega                                          # :70-73
        for _ in range(k, extended_k):
            omega = omega * omega % r
        g_coset = field.zeta                                            # :81
        g_coset_inv = g_coset * g_coset % r                             # :82
        orig = pow(field.zeta, n, r)                                    # :84-107
        step = pow(extended_omega, n, r)
        t_evaluations, cur = [], orig
        while True:
            t_evaluations.append(cur)
            cur = cur * step % r
            if cur == orig:
                break
        assert len(t_evaluations) == 1 << (extended_k - k)             # :98
        t_evaluations = [pow((c - 1) % r, -1, r) for c in t_evaluations]   # :101-103, batch_invert :117-124
        consts = {
            "omega": omega, "omega_inv": pow(omega, -1, r), "extended_omega": extended_omega,
            "extended_omega_inv": pow(extended_omega, -1, r), "g_coset": g_coset, "g_coset_inv": g_coset_inv,
            "ifft_divisor": pow(1 << k, -1, r), "extended_ifft_divisor": pow(1 << extended_k, -1, r),   # :109-110
        }
        d = cls(k, extended_k, quotient_poly_degree, t_evaluations=np.stack([field.from_int(c) for c in t_evaluations]),
                **{f: field.from_int(v) for f, v in consts.items()})
        d.barycentric_weight = field.from_int(pow(n, -1, r))            # :114
        d.field = field
        d.ints = dict(consts)  # the same constants as integers (canonical form)
        return d

    def extended_len(self):
        return 1 << self.extended_k

    def lagrange_to_coeff(self, a):
        """poly/domain.rs:226-236"""
        self._device_field()
        a = _u64(a, 4).copy()
        assert a.shape[0] == 1 << self.k
        _check(lib().h2hip_ifft_bn254_fr(_p(a), _p(self.omega_inv), self.k, _p(self.ifft_divisor)),
               "h2hip_ifft_bn254_fr")
        return a

    def coeff_to_extended(self, a):
        """poly/domain.rs:240-254"""
        self._device_field()
        a = _u64(a, 4)
        assert a.shape[0] == 1 << self.k
        out = np.zeros((self.extended_len(), 4), dtype=np.uint64)
        _check(lib().h2hip_coeff_to_extended_bn254_fr(_p(a), self.k, _p(out), self.extended_k,
                                                      _p(self.extended_omega), _p(self.g_coset), _p(self.g_coset_inv)),
               "h2hip_coeff_to_extended_bn254_fr")
        return out

    def coeff_to_extended_part(self, a, part):
        """upstream halo2's coeff_to_extended_part: rows j * P + part (P = 2^(extended_k - k)) of coeff_to_extended(a), 2^k elements"""
        self._device_field()
        a = _u64(a, 4)
        assert a.shape[0] == 1 << self.k
        out = np.zeros((1 << self.k, 4), dtype=np.uint64)
        _check(lib().h2hip_coeff_to_extended_part_bn254_fr(_p(a), self.k, self.extended_k, part,
                                                           _p(self.extended_omega), _p(self.g_coset), _p(self.g_coset_inv), _p(out)),
               "h2hip_coeff_to_extended_part_bn254_fr")
        return out

    def extended_to_coeff(self, a):
        """poly/domain.rs:281-303 (including the truncate at :299-300)"""
        self._device_field()
        a = _u64(a, 4).copy()
        assert a.shape[0] == self.extended_len()
        _check(lib().h2hip_extended_to_coeff_bn254_fr(_p(a), self.extended_k, _p(self.extended_omega_inv),
                                                      _p(self.extended_ifft_divisor), _p(self.g_coset), _p(self.g_coset_inv)),
               "h2hip_extended_to_coeff_bn254_fr")
        return a[: self.n * self.quotient_poly_degree]


    # the same conversions for a list of host columns, pipelined over PCIe inside one call (h2hip_*_batch): what a patched
    # prover calls where the reference maps the single-column method over its polynomials (plonk/prover.rs:476-490,
    # plonk/evaluation.rs:306-323)
    def lagrange_to_coeff_batch(self, polys):
        self._device_field()
        cols = [_u64(a, 4).copy() for a in polys]
        for a in cols:
            assert a.shape[0] == 1 << self.k
        if cols:
            _check(lib().h2hip_ifft_bn254_fr_batch(_host_ptrs(cols), len(cols), _p(self.omega_inv), self.k,
                                                   _p(self.ifft_divisor)), "h2hip_ifft_bn254_fr_batch")
        return cols

    def coeff_to_extended_batch(self, polys):
        self._device_field()
        cols = [_u64(a, 4) for a in polys]
        for a in cols:
            assert a.shape[0] == 1 << self.k
        outs = [np.empty((self.extended_len(), 4), dtype=np.uint64) for _ in cols]
        if cols:
            _check(lib().h2hip_coeff_to_extended_bn254_fr_batch(_host_ptrs(cols), self.k, _host_ptrs(outs), len(cols),
                                                                self.extended_k, _p(self.extended_omega), _p(self.g_coset),
                                                                _p(self.g_coset_inv)), "h2hip_coeff_to_extended_bn254_fr_batch")
        return outs

    def extended_to_coeff_batch(self, polys):
        self._device_field()
        cols = [_u64(a, 4).copy() for a in polys]
        for a in cols:
            assert a.shape[0] == self.extended_len()
        if cols:
            _check(lib().h2hip_extended_to_coeff_bn254_fr_batch(_host_ptrs(cols), len(cols), self.extended_k,
                                                                _p(self.extended_omega_inv), _p(self.extended_ifft_divisor), _p(self.g_coset),
                                                                _p(self.g_coset_inv)), "h2hip_extended_to_coeff_bn254_fr_batch")
        return [a[: self.n * self.quotient_poly_degree] for a in cols]

    def divide_by_vanishing_poly(self, a, t_evaluations=None):
        """poly/domain.rs:307-326"""
        self._device_field()
        a = _u64(a, 4).copy()
        t = self.t_evaluations if t_evaluations is None else _u64(t_evaluations, 4)
        assert a.shape[0] == self.extended_len()
        _check(lib().h2hip_divide_by_vanishing_poly_bn254_fr(_p(a), self.extended_k, _p(t), t.shape[0]),
               "h2hip_divide_by_vanishing_poly_bn254_fr")
        return a


# ------------------------------------------------------------------ helpers.rs (SerdeFormat), poly.rs:152-177
import enum  # noqa: E402


class SerdeFormat(enum.Enum):
    """helpers.rs:8-20"""
    Processed = 0           # curve points compressed (32 B per G1, 64 B per G2), field elements canonical; every element checked
    RawBytes = 1            # the in-memory Montgomery limbs; coordinates below the modulus and points on the curve checked
    RawBytesUnchecked = 2   # the same bytes, no checks


H2HIP_EENCODING = 5


class H2HipEncodingError(H2HipError):
    """an element fails its format's checks (H2HIP_EENCODING; the reference's io::Error "invalid point encoding" / "Invalid prime
    field point encoding").  count: invalid elements; index: the lowest of them; output: what the call wrote, invalid elements as zeros"""

    def __init__(self, what, rc, count, index, output=None):
        H2HipError.__init__(self, "%s failed (rc=%d): %s" % (what, rc, lib().h2hip_last_error().decode()))
        self.rc, self.count, self.index, self.output = rc, count, index, output


def _check_encoding(rc, what, invalid, output=None):
    if rc == H2HIP_EENCODING:
        raise H2HipEncodingError(what, rc, int(invalid[0]), int(invalid[1]), output)
    _check(rc, what)


def _bytes32(a, what):
    a = np.ascontiguousarray(np.frombuffer(a, dtype=np.uint8) if isinstance(a, (bytes, bytearray, memoryview)) else a)
    if a.dtype != np.uint8 or a.size % 32:
        raise ValueError("%s: expected uint8 data, 32 bytes per element" % what)
    return a.reshape(-1, 32)


def g1_from_bytes(data):
    """G1Affine::from_bytes over an array (SerdeFormat::Processed read): (n, 32) uint8 -> (n, 8) uint64 Montgomery points, on the GPU.
    H2HipEncodingError when an encoding is invalid."""
    data = _bytes32(data, "g1_from_bytes")
    n = data.shape[0]
    out, invalid = np.zeros((n, 8), dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    _check_encoding(lib().h2hip_g1_decompress_bn254(_p(data), n, _p(out), _p(invalid)), "h2hip_g1_decompress_bn254", invalid, out)
    return out


def g1_to_bytes(points):
    """G1Affine::to_bytes over an array (Processed write): (n, 8) uint64 -> (n, 32) uint8"""
    points = _u64(points, 8)
    n = points.shape[0]
    out = np.zeros((n, 32), dtype=np.uint8)
    _check(lib().h2hip_g1_compress_bn254(_p(points), n, _p(out)), "h2hip_g1_compress_bn254")
    return out


def g1_validate(points):
    """read_raw's checks (SerdeFormat::RawBytes read) on (n, 8) uint64 points; H2HipEncodingError when one fails"""
    points = _u64(points, 8)
    invalid = np.zeros(2, dtype=np.uint64)
    _check_encoding(lib().h2hip_g1_validate_bn254(_p(points), points.shape[0], _p(invalid)), "h2hip_g1_validate_bn254", invalid)


def fr_from_repr(data):
    """Fr::from_repr over an array: (n, 32) uint8 canonical little-endian -> (n, 4) uint64 Montgomery; H2HipEncodingError for a value >= r"""
    data = _bytes32(data, "fr_from_repr")
    n = data.shape[0]
    out, invalid = np.zeros((n, 4), dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    _check_encoding(lib().h2hip_fr_from_repr_bn254(_p(data), n, _p(out), _p(invalid)), "h2hip_fr_from_repr_bn254", invalid, out)
    return out


def fr_to_repr(a):
    """Fr::to_repr over an array: (n, 4) uint64 Montgomery -> (n, 32) uint8"""
    a = _u64(a, 4)
    out = np.zeros((a.shape[0], 32), dtype=np.uint8)
    _check(lib().h2hip_fr_to_repr_bn254(_p(a), a.shape[0], _p(out)), "h2hip_fr_to_repr_bn254")
    return out


# The two G2 points of a params file are converted on the host, in Python integers: Fq2 = Fq[u] / (u^2 + 1), the twist
# y^2 = x^3 + 3 / (9 + u).  Raw: x.c0 || x.c1 || y.c0 || y.c1, 32-B Montgomery each; compressed: x.c0 || x.c1 canonical little-endian
# with the low bit of canonical y.c0 in bit 7 of byte 63; all zero bytes: the identity.
def _fq2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % FQ_MODULUS, (a[0] * b[1] + a[1] * b[0]) % FQ_MODULUS)


_G2_B = _fq2_mul((3, 0), (9 * pow(82, -1, FQ_MODULUS) % FQ_MODULUS, -pow(82, -1, FQ_MODULUS) % FQ_MODULUS))  # 3 / (9 + u) = 3 (9 - u) / 82


def _fq_sqrt(a):
    y = pow(a, (FQ_MODULUS + 1) // 4, FQ_MODULUS)
    return y if y * y % FQ_MODULUS == a % FQ_MODULUS else None


def _fq2_sqrt(a):
    """a square root of a in Fq2 or None: with s^2 = a0^2 + a1^2, x0^2 = (a0 + s) / 2 or (a0 - s) / 2 and x1 = a1 / (2 x0)"""
    if a == (0, 0):
        return (0, 0)
    s = _fq_sqrt((a[0] * a[0] + a[1] * a[1]) % FQ_MODULUS)
    if s is None:
        return None
    half = pow(2, -1, FQ_MODULUS)
    for cand in ((a[0] + s) * half % FQ_MODULUS, (a[0] - s) * half % FQ_MODULUS):
        x0 = _fq_sqrt(cand)
        if x0:
            r = (x0, a[1] * pow(2 * x0, -1, FQ_MODULUS) % FQ_MODULUS)
            if _fq2_mul(r, r) == a:
                return r
    if a[1] == 0:  # a = -c^2 in Fq: the root is purely imaginary
        x1 = _fq_sqrt(-a[0] % FQ_MODULUS)
        if x1 is not None:
            return (0, x1)
    return None


def _g2_rhs(x):
    x3 = _fq2_mul(_fq2_mul(x, x), x)
    return ((x3[0] + _G2_B[0]) % FQ_MODULUS, (x3[1] + _G2_B[1]) % FQ_MODULUS)


def _g2_raw(data, check=False):
    """128 raw bytes of a G2 point (None: the identity); check: RawBytes' checks"""
    if data is None:
        return bytes(128)
    data = bytes(data)
    if len(data) != 128:
        raise ValueError("a raw G2 point is 128 bytes")
    if check and data != bytes(128):
        c = [int.from_bytes(data[32 * i:32 * i + 32], "little") for i in range(4)]
        if max(c) >= FQ_MODULUS:
            raise H2HipError("invalid point encoding: a G2 coordinate is not below q")
        rinv = pow(_FQ_R, -1, FQ_MODULUS)
        x, y = tuple(v * rinv % FQ_MODULUS for v in c[:2]), tuple(v * rinv % FQ_MODULUS for v in c[2:])
        if _fq2_mul(y, y) != _g2_rhs(x):
            raise H2HipError("invalid point encoding: the G2 point is not on the curve")
    return data


def g2_from_bytes(data):
    """G2Affine::from_bytes: 64 B compressed -> 128 B raw; H2HipError for an invalid encoding"""
    data = bytes(data)
    if len(data) != 64:
        raise ValueError("a compressed G2 point is 64 bytes")
    if data == bytes(64):
        return bytes(128)
    sign = data[63] >> 7
    x = (int.from_bytes(data[:32], "little"), int.from_bytes(data[32:63] + bytes([data[63] & 0x7f]), "little"))
    y = _fq2_sqrt(_g2_rhs(x)) if max(x) < FQ_MODULUS else None
    if y is None or x == (0, 0):
        raise H2HipError("invalid point encoding: not a compressed G2 point")
    if (y[0] & 1) != sign:
        y = (-y[0] % FQ_MODULUS, -y[1] % FQ_MODULUS)
    return b"".join((v * _FQ_R % FQ_MODULUS).to_bytes(32, "little") for v in x + y)


def g2_to_bytes(raw):
    """G2Affine::to_bytes: 128 B raw (reduced, on the curve) -> 64 B compressed"""
    raw = _g2_raw(raw)
    if raw == bytes(128):
        return bytes(64)
    rinv = pow(_FQ_R, -1, FQ_MODULUS)
    c = [int.from_bytes(raw[32 * i:32 * i + 32], "little") * rinv % FQ_MODULUS for i in range(4)]
    out = bytearray(c[0].to_bytes(32, "little") + c[1].to_bytes(32, "little"))
    out[63] |= (c[2] & 1) << 7
    return bytes(out)


def _read_exact(reader, n, what):
    buf = reader.read(n)
    if len(buf) != n:
        raise H2HipError("%s: short read" % what)
    return buf


def read_polynomial(reader, format):
    """Polynomial::read (poly.rs:152-165): a big-endian u32 length, then that many Fr in the format's encoding (SerdePrimeField,
    helpers.rs:61-93: Processed canonical, RawBytes* the Montgomery limbs, RawBytes checked to be below r) -> (len, 4) uint64"""
    format = SerdeFormat(format)
    n = int.from_bytes(_read_exact(reader, 4, "Polynomial::read"), "big")
    data = np.frombuffer(_read_exact(reader, 32 * n, "Polynomial::read"), dtype=np.uint8).reshape(n, 32)
    if format is SerdeFormat.Processed:
        return fr_from_repr(data)
    out = data.copy().view(np.uint64).reshape(n, 4)
    if format is SerdeFormat.RawBytes:
        top = np.array([(FR_MODULUS >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)
        ge = np.zeros(n, dtype=bool)   # limb-wise comparison with r, most significant limb last to decide
        for i in range(4):
            ge = np.where(out[:, i] != top[i], out[:, i] > top[i], ge)
        ge |= (out == top).all(axis=1)
        if ge.any():
            raise H2HipError("Invalid prime field point encoding: element %d is not below r" % int(np.argmax(ge)))
    return out


def write_polynomial(poly, writer, format):
    """Polynomial::write (poly.rs:167-177)"""
    format = SerdeFormat(format)
    poly = _u64(poly, 4)
    writer.write(int(poly.shape[0]).to_bytes(4, "big"))
    writer.write(fr_to_repr(poly).tobytes() if format is SerdeFormat.Processed else poly.tobytes())


def read_polynomial_vec(reader, format):
    """helpers.rs:116-127: a big-endian u32 count, then that many polynomials"""
    count = int.from_bytes(_read_exact(reader, 4, "read_polynomial_vec"), "big")
    return [read_polynomial(reader, format) for _ in range(count)]


def write_polynomial_slice(polys, writer, format):
    """helpers.rs:130-140"""
    writer.write(len(polys).to_bytes(4, "big"))
    for poly in polys:
        write_polynomial(poly, writer, format)


# ------------------------------------------------------------------ poly/kzg/commitment.rs
# EIP-197's generator of G2 as 128 raw bytes (x.c0 || x.c1 || y.c0 || y.c1, Montgomery): G2Affine::generator()
G2_GENERATOR = b"".join((c * _FQ_R % FQ_MODULUS).to_bytes(32, "little") for c in (
    0x1800deef121f1e76426a00665e5c4479674322d4f75edadd46debd5cd992f6ed, 0x198e9393920d483a7260bfb731fb5d25f1aa493335a9e71297e485b7aef312c2,
    0x12c85ea5db8c6deb4aab71808dcb408fe3d1e7690c43d37b4ce6cc0166fa7daa, 0x090689d0585ff075ec9e99ad690c3395bc4b313370b38ef355acdadcd122975b))


class ParamsStructure:
    """what ParamsKZG.check_structure found: `failed` names the relations that do not hold (of "identity", "subgroup", "pairing",
    "powers", "lagrange"); true when none failed"""

    def __init__(self, failed):
        self.failed = tuple(failed)
        self.ok = not self.failed

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return "ParamsStructure(ok)" if self.ok else "ParamsStructure(failed: %s)" % ", ".join(self.failed)


class ParamsKZG:
    """poly::kzg::commitment::ParamsKZG<Bn256> (poly/kzg/commitment.rs:22-30): g and g_lagrange
    are pinned on the GPU for the life of the object; commit / commit_lagrange are
    best_multiexp over them (:281-292, :327-334; the blind is ignored there too)."""

    def __init__(self, k, g, g_lagrange=None, g2=None, s_g2=None):
        """g_lagrange None: derived from g with g_to_lagrange, as downsize does (:274).  g2 / s_g2: the verifier's two G2 points, 128 raw
        bytes each (x.c0 || x.c1 || y.c0 || y.c1, Montgomery), which kzg.DualMSM.check pairs with; zeros (the identity) when not given"""
        self.k, self.n = int(k), 1 << int(k)
        self.g = _u64(g, 8).copy()
        self.g_lagrange = g_to_lagrange(self.g, self.k) if g_lagrange is None else _u64(g_lagrange, 8).copy()
        assert self.g.shape[0] == self.n and self.g_lagrange.shape[0] == self.n
        self.g2, self.s_g2 = _g2_raw(g2), _g2_raw(s_g2)
        self._d_g = self._d_g_lagrange = None  # read_custom: the device copies the points were converted or checked in, pinned as they lie
        bases_pin(self.g)
        bases_pin(self.g_lagrange)

    # ---- read / write (poly/kzg/commitment.rs:142-244): k as u32 LE, then g, g_lagrange, g2, s_g2 in the format's point encoding
    @classmethod
    def read(cls, reader):
        """Params::read = read_custom(reader, SerdeFormat::RawBytes) (:300-302)"""
        return cls.read_custom(reader, SerdeFormat.RawBytes)

    @classmethod
    def read_custom(cls, reader, format):
        """ParamsKZG::read_custom (:160-244).  Processed: 32 B per G1 point are uploaded, decompressed on the GPU (one square root each),
        that device copy is pinned for the commits (bases_pin_device) and the 64-B points come back for g / g_lagrange.  RawBytes: the
        uploaded copy is checked on the GPU (read_raw's checks) and pinned in the same way.  RawBytesUnchecked: no checks.  A short file
        or a point that fails its format's checks raises H2HipError, where the reference returns io::Error."""
        format = SerdeFormat(format)
        if device_count() < 1:
            raise H2HipError("ParamsKZG::read: no GPU (the points are converted and checked there; no CPU fallback exists)")
        import torch
        kb = reader.read(4)
        if len(kb) != 4:
            raise H2HipError("ParamsKZG::read: short read")
        k = int.from_bytes(kb, "little")
        if k > FR_S:
            raise H2HipError("ParamsKZG::read: k = %d > Fr::S" % k)
        n = 1 << k
        size = 32 if format is SerdeFormat.Processed else 64
        host, dev = [], []
        for what in ("g", "g_lagrange"):
            buf = reader.read(n * size)
            if len(buf) != n * size:
                raise H2HipError("ParamsKZG::read: short read")
            d_in = torch.from_numpy(np.frombuffer(buf, dtype=np.uint8).reshape(n, size).copy()).cuda()
            if format is SerdeFormat.Processed:
                d_pts = torch.empty((n, 8), dtype=torch.int64, device="cuda")
                g1_from_bytes_device(d_in, d_pts, n)
            else:
                d_pts = d_in.view(torch.int64)
                if format is SerdeFormat.RawBytes:
                    g1_validate_device(d_pts, n)
            dev.append(d_pts)
            host.append(to_numpy_u64(d_pts).copy())
        g2s = []
        for what in ("g2", "s_g2"):
            buf = reader.read(size * 2)
            if len(buf) != size * 2:
                raise H2HipError("ParamsKZG::read: short read")
            g2s.append(g2_from_bytes(buf) if format is SerdeFormat.Processed else _g2_raw(buf, check=format is SerdeFormat.RawBytes))
        self = cls.__new__(cls)
        self.k, self.n = k, n
        self.g, self.g_lagrange = host
        self.g2, self.s_g2 = g2s
        self._d_g = self._d_g_lagrange = None
        for name, d in zip(("_d_g", "_d_g_lagrange"), dev):
            bases_pin_device(d, n)
            setattr(self, name, d)
        return self

    def write(self, writer):
        """Params::write = write_custom(writer, SerdeFormat::RawBytes) (:296-298)"""
        self.write_custom(writer, SerdeFormat.RawBytes)

    def write_custom(self, writer, format):
        """ParamsKZG::write_custom (:142-157); Processed compresses the G1 points on the GPU"""
        format = SerdeFormat(format)
        writer.write(int(self.k).to_bytes(4, "little"))
        for pts in (self.g, self.g_lagrange):
            writer.write(g1_to_bytes(pts).tobytes() if format is SerdeFormat.Processed else pts.tobytes())
        for pt in (self.g2, self.s_g2):
            writer.write(g2_to_bytes(pt) if format is SerdeFormat.Processed else pt)

    def _msm(self, poly, host_bases, d_bases):
        size = poly.shape[0]
        if d_bases is None:
            out = np.zeros(12, dtype=np.uint64)
            _check(lib().h2hip_msm_bn254(_p(poly), _p(host_bases), size, _p(out)), "h2hip_msm_bn254")
            return out
        import torch
        return msm_device(torch.from_numpy(poly.view(np.int64)).cuda(), d_bases, size)

    @classmethod
    def setup(cls, k, secret):
        """ParamsKZG::setup (poly/kzg/commitment.rs:61-129) with the secret given (an int, or 4 Montgomery limbs) instead
        of drawn from an rng: g[i] = [s^i] G1, g_lagrange[i] = [l_i(s)] G1, computed on the GPU; g2 = the generator of G2 and
        s_g2 = [s] g2 (:118-119), on the host (h2hip_g2_mul_bn254)"""
        if not 0 <= int(k) <= FR_S:
            raise H2HipError("kzg_setup: assertion failed: k <= Fr::S")  # :64 (before any allocation of 2^k points)
        s = fr_from_int(secret) if isinstance(secret, int) else _fe(secret)
        n = 1 << int(k)
        g = np.zeros((n, 8), dtype=np.uint64)
        gl = np.zeros((n, 8), dtype=np.uint64)
        _check(lib().h2hip_kzg_setup_bn254(k, _p(s), _p(g), _p(gl)), "h2hip_kzg_setup_bn254")
        s_g2 = np.zeros(16, dtype=np.uint64)
        _check(lib().h2hip_g2_mul_bn254(_p(np.frombuffer(G2_GENERATOR, dtype=np.uint64)), _p(s), _p(s_g2)), "h2hip_g2_mul_bn254")
        return cls(k, g, gl, G2_GENERATOR, s_g2.tobytes())

    def commit_lagrange(self, poly, blind=None):
        poly = _u64(poly, 4)
        size = poly.shape[0]
        assert self.g_lagrange.shape[0] >= size  # assert!(bases.len() >= size), :290
        return self._msm(poly, self.g_lagrange, self._d_g_lagrange)

    def commit_lagrange_many(self, polys):
        """the advice-column loop of plonk/prover.rs:361-365 as one pipelined batch"""
        if self._d_g_lagrange is None:
            return best_multiexp_batch(polys, self.g_lagrange)
        return np.stack([self.commit_lagrange(p) for p in polys])

    def commit(self, poly, blind=None):
        poly = _u64(poly, 4)
        size = poly.shape[0]
        assert self.g.shape[0] >= size  # :332
        return self._msm(poly, self.g, self._d_g)

    def _resident_g(self):
        """g in HBM, pinned by its device pointer: read_custom's copy, or one uploaded at the first call and kept until close"""
        d_g = self._d_g
        if d_g is None:
            d_g = getattr(self, "_d_g_resident", None)
            if d_g is None:
                import torch
                d_g = torch.from_numpy(self.g.view(np.int64)).cuda()
                bases_pin_device(d_g, self.n)
                self._d_g_resident = d_g
        return d_g

    def commit_device(self, d_poly, n=None):
        """commit for a coefficient polynomial that lives in HBM (n x 32 B): an MSM over g resident in HBM and pinned by its device
        pointer -- read_custom's copy, or one uploaded at the first call and kept until close"""
        return msm_device(d_poly, self._resident_g(), n)

    def check_structure(self, seed, timings=None):
        """Is this a structured reference string?  A file's points are checked one by one when it is read; this checks the three
        relations between them, with randomness drawn from FrRng(seed) (32 bytes), and returns a ParamsStructure that names what
        failed.  The MSMs, the draws and the transform run on the GPU, the pairings on the host.
          (a) "identity": g[0], g2 or s_g2 is the identity; "subgroup": g2 or s_g2 is not on the twist or not in the subgroup of
              order r.  When (a) fails the pairing checks of (b) are not made (the library refuses such points).
          (b) "pairing": e(g[0], s_g2) != e(g[1], g2) -- s_g2 does not carry the s of g; "powers": with rho_i, i < n - 1, drawn in HBM,
              A = sum rho_i g[i] and B = sum rho_i g[i + 1] (two device MSMs), e(A, s_g2) != e(B, g2) -- g is not the powers of one s.
              "powers" is judged only when "pairing" holds.  B's bases are a device-to-device copy of g[1..n): the MSM takes its bases
              at a buffer's own alignment and that copy is not pinned.
          (c) "lagrange": with c of n elements drawn, commit_lagrange(c) != commit(lagrange_to_coeff(c)) -- g_lagrange is not g's
              Lagrange basis.
        At k = 0 there is no g[1]: (b) is vacuous, nothing ties s_g2 to g, and only (a) and (c) are checked.
        timings: a dict that receives the host-clock milliseconds of the "pairing" calls, of (b)'s draw and two "msm"s and of (c)'s
        "transform" and its two "commit"s (tools/pairing_bench.py)."""
        import ctypes
        import time
        import torch
        rng = FrRng(seed)
        spent = {"pairing": 0.0, "msm": 0.0, "transform": 0.0, "commit": 0.0}

        def clock(what, f):
            t = time.perf_counter()
            out = f()
            spent[what] += (time.perf_counter() - t) * 1e3
            return out
        n, failed = self.n, []
        g2s = [np.frombuffer(bytes(pt), dtype=np.uint64) for pt in (self.g2, self.s_g2)]
        if not self.g[0].any() or not all(pt.any() for pt in g2s):
            failed.append("identity")
        for pt in g2s:
            on, sub = ctypes.c_int(0), ctypes.c_int(0)
            rc = lib().h2hip_g2_check_bn254(_p(pt), ctypes.byref(on), ctypes.byref(sub))
            if (rc or not (on.value and sub.value)) and "subgroup" not in failed:
                failed.append("subgroup")
        if n > 1 and not failed:
            g2_pair = np.stack([g2s[1], g2s[0]])                      # s_g2, g2

            def holds(a, b):
                """e(a, s_g2) e(-b, g2) = 1; -b negates y, on Montgomery limbs as on the value"""
                pts = np.stack([a, b])
                y = int.from_bytes(pts[1, 4:].tobytes(), "little")
                pts[1, 4:] = np.frombuffer((-y % FQ_MODULUS).to_bytes(32, "little"), dtype=np.uint64)
                ok = ctypes.c_int(0)
                _check(clock("pairing", lambda: lib().h2hip_pairing_check_bn254(_p(pts), _p(g2_pair), 2, ctypes.byref(ok))),
                       "h2hip_pairing_check_bn254")
                return ok.value == 1
            if not holds(self.g[0], self.g[1]):
                failed.append("pairing")
            else:
                d_g = self._resident_g()
                d_shifted = d_g.reshape(-1)[8:8 * n].clone()          # g[1..n) at its own buffer's start
                d_rho = rng.draw_device(n - 1)
                a, b = clock("msm", lambda: (g1_to_affine(msm_device(d_rho, d_g, n - 1)), g1_to_affine(msm_device(d_rho, d_shifted, n - 1))))
                if not holds(a, b):
                    failed.append("powers")
        c = rng.draw(n)
        domain = EvaluationDomain.new(2, self.k)
        coeff = c if self.k == 0 else clock("transform", lambda: domain.lagrange_to_coeff(c))
        if not clock("commit", lambda: np.array_equal(g1_to_affine(self.commit_lagrange(c)), g1_to_affine(self.commit(coeff)))):
            failed.append("lagrange")
        if timings is not None:
            timings.update(spent)
        return ParamsStructure(failed)

    def downsize(self, k):
        """ParamsKZG::downsize (poly/kzg/commitment.rs:267-275)"""
        assert k <= self.k  # :268
        self.close()
        self.k, self.n = int(k), 1 << int(k)
        self.g = self.g[:self.n].copy()                       # self.g.truncate(self.n)
        self.g_lagrange = g_to_lagrange(self.g, self.k)       # :274
        bases_pin(self.g)
        bases_pin(self.g_lagrange)

    def close(self):
        """unpin both arrays (idempotent); also runs when the object is dropped or leaves a `with` block, so a dead
        ParamsKZG never leaves its device copies behind under host addresses numpy may hand out again"""
        for name in ("g", "g_lagrange"):
            b, d = getattr(self, name, None), getattr(self, "_d_" + name, None)
            if b is None:
                continue
            try:
                if d is None:
                    bases_unpin(b)
                else:
                    bases_unpin_device(d)
                    setattr(self, "_d_" + name, None)
            except H2HipError:
                pass
        d = getattr(self, "_d_g_resident", None)
        if d is not None:
            self._d_g_resident = None
            try:
                bases_unpin_device(d)
            except H2HipError:
                pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ device-resident entry points
def _dptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def msm_device(d_scalars, d_bases, n=None):
    """d_scalars / d_bases: torch CUDA tensors holding n x 32 B and n x 64 B (any dtype)"""
    nb = d_scalars.numel() * d_scalars.element_size()
    n = nb // 32 if n is None else int(n)
    out = np.zeros(12, dtype=np.uint64)
    _check(lib().h2hip_msm_bn254_device(_dptr(d_scalars), _dptr(d_bases), n, _p(out), _stream()), "h2hip_msm_bn254_device")
    return out


def msm_batch_device(d_scalars_list, d_bases, n=None):
    """count MSMs over the same device-resident bases; returns (count, 12) uint64"""
    count = len(d_scalars_list)
    if n is None:
        n = d_scalars_list[0].numel() * d_scalars_list[0].element_size() // 32
    ptrs = (ctypes.c_void_p * count)(*[t.data_ptr() for t in d_scalars_list])
    out = np.zeros((count, 12), dtype=np.uint64)
    _check(lib().h2hip_msm_bn254_batch_device(ptrs, _dptr(d_bases), n, count, _p(out), _stream()),
           "h2hip_msm_bn254_batch_device")
    return out


def ntt_device(d_a, omega, log_n):
    _check(lib().h2hip_ntt_bn254_fr_device(_dptr(d_a), _p(_fe(omega)), log_n, _stream()), "h2hip_ntt_bn254_fr_device")


def ifft_device(d_a, omega_inv, log_n, divisor):
    _check(lib().h2hip_ifft_bn254_fr_device(_dptr(d_a), _p(_fe(omega_inv)), log_n, _p(_fe(divisor)), _stream()),
           "h2hip_ifft_bn254_fr_device")


def coeff_to_extended_device(d_a, k, extended_k, extended_omega, g_coset, g_coset_inv):
    _check(lib().h2hip_coeff_to_extended_bn254_fr_device(_dptr(d_a), k, extended_k, _p(_fe(extended_omega)),
                                                         _p(_fe(g_coset)), _p(_fe(g_coset_inv)), _stream()),
           "h2hip_coeff_to_extended_bn254_fr_device")


def coeff_to_extended_part_device(d_a, k, extended_k, part, extended_omega, g_coset, g_coset_inv, d_out=None):
    """part `part` of coeff_to_extended(d_a) into d_out (2^k elements each; d_out None: in place); queued on the current stream"""
    d_out = d_a if d_out is None else d_out
    _check(lib().h2hip_coeff_to_extended_part_bn254_fr_device(_dptr(d_a), k, extended_k, part,
                                                              _p(_fe(extended_omega)), _p(_fe(g_coset)), _p(_fe(g_coset_inv)), _dptr(d_out),
                                                              _stream()), "h2hip_coeff_to_extended_part_bn254_fr_device")


def extended_to_coeff_device(d_a, extended_k, extended_omega_inv, extended_ifft_divisor, g_coset, g_coset_inv):
    _check(lib().h2hip_extended_to_coeff_bn254_fr_device(_dptr(d_a), extended_k, _p(_fe(extended_omega_inv)),
                                                         _p(_fe(extended_ifft_divisor)), _p(_fe(g_coset)), _p(_fe(g_coset_inv)), _stream()),
           "h2hip_extended_to_coeff_bn254_fr_device")


def _ptr_array(tensors):
    return (ctypes.c_void_p * max(1, len(tensors)))(*[t.data_ptr() for t in tensors])


def ntt_batch_device(d_list, omega, log_n):
    """the same NTT over every tensor of d_list, one launch per pass"""
    _check(lib().h2hip_ntt_bn254_fr_batch_device(_ptr_array(d_list), len(d_list), _p(_fe(omega)), log_n, _stream()),
           "h2hip_ntt_bn254_fr_batch_device")


def ifft_batch_device(d_list, omega_inv, log_n, divisor):
    _check(lib().h2hip_ifft_bn254_fr_batch_device(_ptr_array(d_list), len(d_list), _p(_fe(omega_inv)), log_n,
                                                  _p(_fe(divisor)), _stream()), "h2hip_ifft_bn254_fr_batch_device")


def coeff_to_extended_batch_device(d_list, k, extended_k, extended_omega, g_coset, g_coset_inv):
    _check(lib().h2hip_coeff_to_extended_bn254_fr_batch_device(_ptr_array(d_list), len(d_list), k,
                                                               extended_k, _p(_fe(extended_omega)), _p(_fe(g_coset)),
                                                               _p(_fe(g_coset_inv)), _stream()), "h2hip_coeff_to_extended_bn254_fr_batch_device")


def coeff_to_extended_part_batch_device(d_list, d_out_list, parts, k, extended_k, extended_omega, g_coset, g_coset_inv):
    """transform i: part parts[i] of coeff_to_extended(d_list[i]) into d_out_list[i], one launch per pass; a source may feed several
    transforms (all P parts of one polynomial), and an output may be its own source only where that source feeds no other transform"""
    assert len(d_list) == len(d_out_list) == len(parts)
    h_parts = (ctypes.c_uint32 * max(1, len(parts)))(*[int(p) for p in parts])
    _check(lib().h2hip_coeff_to_extended_part_bn254_fr_batch_device(_ptr_array(d_list), _ptr_array(d_out_list), h_parts, len(d_list),
                                                                    k, extended_k, _p(_fe(extended_omega)),
                                                                    _p(_fe(g_coset)), _p(_fe(g_coset_inv)), _stream()),
           "h2hip_coeff_to_extended_part_bn254_fr_batch_device")

def permutation_products_device(k, omega, delta, beta, gamma, d_columns, d_permutations, chunk_len, blinding, blinding_factors, d_z):
    """device form of permutation_products: torch CUDA tensors of 2^k x 32 B in, the n_sets tensors of d_z written; queued on the
    current stream, not waited for"""
    bl = _blinding(blinding, len(d_z), int(blinding_factors))
    _check(lib().h2hip_permutation_products_bn254_device(k, _p(_fe(omega)), _p(_fe(delta)), _p(_fe(beta)), _p(_fe(gamma)),
                                                         _ptr_array(d_columns), _ptr_array(d_permutations), len(d_columns),
                                                         chunk_len, _p(bl), blinding_factors, _ptr_array(d_z),
                                                         _stream()), "h2hip_permutation_products_bn254_device")


def lookup_products_device(k, beta, gamma, d_compressed_inputs, d_compressed_tables, d_permuted_inputs, d_permuted_tables, blinding,
                           blinding_factors, d_z):
    """device form of lookup_products; queued on the current stream, not waited for"""
    bl = _blinding(blinding, len(d_z), int(blinding_factors))
    _check(lib().h2hip_lookup_products_bn254_device(k, _p(_fe(beta)), _p(_fe(gamma)), _ptr_array(d_compressed_inputs),
                                                    _ptr_array(d_compressed_tables), _ptr_array(d_permuted_inputs), _ptr_array(d_permuted_tables),
                                                    len(d_z), _p(bl), blinding_factors, _ptr_array(d_z),
                                                    _stream()), "h2hip_lookup_products_bn254_device")


def shuffle_products_device(k, gamma, d_compressed_inputs, d_compressed_shuffles, blinding, blinding_factors, d_z):
    """device form of shuffle_products; queued on the current stream, not waited for"""
    bl = _blinding(blinding, len(d_z), int(blinding_factors))
    _check(lib().h2hip_shuffle_products_bn254_device(k, _p(_fe(gamma)), _ptr_array(d_compressed_inputs),
                                                     _ptr_array(d_compressed_shuffles), len(d_z), _p(bl),
                                                     blinding_factors, _ptr_array(d_z), _stream()),
           "h2hip_shuffle_products_bn254_device")


def mvlookup_multiplicities_device(k, d_compressed_inputs, d_compressed_tables, blinding_factors, d_m):
    """mvlookup_multiplicities over torch CUDA tensors (d_compressed_inputs[j]: the list of argument j's input tensors); queued on the
    current stream, which the call then waits for once (the verdict).  Raises H2HipLookupError when an input value is missing; d_m is
    written either way."""
    flat, n_in = _mv_inputs(d_compressed_inputs, None, len(d_compressed_tables))
    _check_lookup(lib().h2hip_mvlookup_multiplicities_bn254_device(k, _ptr_array(flat), _p(n_in), _ptr_array(d_compressed_tables),
                                                                   len(d_compressed_tables), blinding_factors,
                                                                   _ptr_array(d_m), _stream()), "h2hip_mvlookup_multiplicities_bn254_device")


def mvlookup_sums_device(k, beta, d_compressed_inputs, d_compressed_tables, d_m, blinding, blinding_factors, d_phi):
    """device form of mvlookup_sums; queued on the current stream, not waited for"""
    flat, n_in = _mv_inputs(d_compressed_inputs, None, len(d_compressed_tables))
    bl = _blinding(blinding, len(d_phi), int(blinding_factors))
    _check(lib().h2hip_mvlookup_sums_bn254_device(k, _p(_fe(beta)), _ptr_array(flat), _p(n_in), _ptr_array(d_compressed_tables),
                                                  _ptr_array(d_m), len(d_phi), _p(bl), blinding_factors,
                                                  _ptr_array(d_phi), _stream()), "h2hip_mvlookup_sums_bn254_device")


def batch_invert_device(d_a, n=None):
    """BatchInvert in place on a torch CUDA tensor of n x 32 B; queued on the current stream, not waited for"""
    n = d_a.numel() * d_a.element_size() // 32 if n is None else int(n)
    _check(lib().h2hip_batch_invert_bn254_fr_device(_dptr(d_a), n, _stream()), "h2hip_batch_invert_bn254_fr_device")


def eval_polynomials_device(d_polys, query_poly, points, lens=None):
    """eval_polynomials over torch CUDA tensors (len_j x 32 B each; lens defaults to their sizes); waits for the result, (n_queries, 4)"""
    lens = [t.numel() * t.element_size() // 32 for t in d_polys] if lens is None else [int(x) for x in lens]
    ln = (ctypes.c_size_t * max(1, len(lens)))(*lens)
    qp = np.ascontiguousarray(query_poly, dtype=np.uint32).reshape(-1)
    pts, nq = _fes(points, "points")
    out = np.zeros((max(1, nq), 4), dtype=np.uint64)
    _check(lib().h2hip_eval_polynomials_bn254_device(_ptr_array(d_polys), ln, len(lens), _p(qp if nq else np.zeros(1, np.uint32)),
                                                     _p(pts), nq, _p(out), _stream()), "h2hip_eval_polynomials_bn254_device")
    return out[:nq]


def poly_combine_device(d_polys, scalars, d_out, sub=None, roots=(), scale=None, accumulate=False, out_len=None, length=None, remainder=False):
    """poly_combine over torch CUDA tensors; d_out receives out_len elements (default: its size).  Queued on the current stream and not
    waited for, unless remainder=True, which returns a(roots[0]) as (4,) uint64."""
    L = (d_polys[0].numel() * d_polys[0].element_size() // 32 if d_polys else 0) if length is None else int(length)
    out_len = d_out.numel() * d_out.element_size() // 32 if out_len is None else int(out_len)
    sc, n_sc, sb, n_sub, rt, n_roots, sl = _combine_args(scalars, sub, roots, scale)
    rem = np.zeros(4, dtype=np.uint64)
    _check(lib().h2hip_poly_combine_bn254_fr_device(_ptr_array(d_polys), L, _p(sc), len(d_polys), _p(sb),
                                                    n_sub, _p(rt), n_roots, _p(sl),
                                                    1 if accumulate else 0, _dptr(d_out), out_len,
                                                    _p(rem) if remainder else None, _stream()), "h2hip_poly_combine_bn254_fr_device")
    return rem if remainder else None


def set_opening_tile(rows_per_thread=0, threads_per_tile=0):
    """test hook: force the opening kernels' tile shape (0, 0 = default)"""
    _check(lib().h2hip_debug_set_opening_tile(rows_per_thread, threads_per_tile), "h2hip_debug_set_opening_tile")




def lookup_compress_device(k, graphs, theta, d_out, d_fixed=(), d_advice=(), d_instance=(), challenges=()):
    """lookup_compress over torch CUDA tensors (2^k x 32 B each); d_out[g] receives graph g.  Queued on the current stream, not waited for"""
    from .evaluation import graph_array
    arr, keep = graph_array(graphs)
    ch, n_ch = _lookup_challenges(challenges)
    _check(lib().h2hip_lookup_compress_bn254_device(k, _ptr_array(d_fixed), len(d_fixed), _ptr_array(d_advice),
                                                    len(d_advice), _ptr_array(d_instance), len(d_instance), _p(ch),
                                                    n_ch, _p(_fe(theta)), arr, len(graphs), _ptr_array(d_out),
                                                    _stream()), "h2hip_lookup_compress_bn254_device")
    del keep


def lookup_permute_device(k, d_compressed_inputs, d_compressed_tables, blinding, blinding_factors, d_permuted_inputs, d_permuted_tables):
    """lookup_permute over torch CUDA tensors; queued on the current stream, which the call then waits for once (the not-found flags).
    Raises H2HipLookupError when an input value is missing from its table."""
    bl = _lookup_blinding(blinding, len(d_compressed_inputs), int(blinding_factors))
    _check_lookup(lib().h2hip_lookup_permute_bn254_device(k, _ptr_array(d_compressed_inputs), _ptr_array(d_compressed_tables),
                                                          len(d_compressed_inputs), _p(bl), blinding_factors,
                                                          _ptr_array(d_permuted_inputs), _ptr_array(d_permuted_tables), _stream()),
                  "h2hip_lookup_permute_bn254_device")


def check_gates_device(k, graphs, d_fixed=(), d_advice=(), d_instance=(), challenges=(), max_rows=16):
    """check_gates over torch CUDA tensors (2^k x 32 B each): queued on the current stream, which the call waits for once to deliver
    (counts, rows)"""
    from .evaluation import graph_array
    arr, keep = graph_array(graphs)
    ch, n_ch = _lookup_challenges(challenges)
    counts, rows, prow = _check_out(len(graphs), max_rows)
    _check(lib().h2hip_check_gates_bn254_device(k, _ptr_array(d_fixed), len(d_fixed), _ptr_array(d_advice),
                                                len(d_advice), _ptr_array(d_instance), len(d_instance), _p(ch),
                                                n_ch, arr, len(graphs), max_rows, _p(counts),
                                                prow, _stream()), "h2hip_check_gates_bn254_device")
    del keep
    return _check_result(counts, rows, len(graphs), max_rows)


def check_permutation_device(k, d_columns, d_mapping, max_rows=16):
    """check_permutation over torch CUDA tensors: d_mapping[j] holds 2^k (column, row) uint32 pairs (8 B per cell).  Queued on the
    current stream, waited for once; a pair out of range is not followed and raises H2HipError (H2HIP_EINVAL)."""
    counts, rows, prow = _check_out(len(d_columns), max_rows)
    _check(lib().h2hip_check_permutation_bn254_device(k, _ptr_array(d_columns), _ptr_array(d_mapping),
                                                      len(d_columns), max_rows, _p(counts), prow, _stream()),
           "h2hip_check_permutation_bn254_device")
    return _check_result(counts, rows, len(d_columns), max_rows)


def check_lookups_device(k, d_compressed_inputs, d_compressed_tables, blinding_factors, max_rows=16):
    """check_lookups over torch CUDA tensors; queued on the current stream, waited for once"""
    count = len(d_compressed_inputs)
    counts, rows, prow = _check_out(count, max_rows)
    _check(lib().h2hip_check_lookups_bn254_device(k, _ptr_array(d_compressed_inputs), _ptr_array(d_compressed_tables),
                                                  count, blinding_factors, max_rows, _p(counts),
                                                  prow, _stream()), "h2hip_check_lookups_bn254_device")
    return _check_result(counts, rows, count, max_rows)


def check_shuffles_device(k, d_compressed_inputs, d_compressed_shuffles, blinding_factors, max_rows=16):
    """check_shuffles over torch CUDA tensors; queued on the current stream, waited for once"""
    count = len(d_compressed_inputs)
    counts, rows, prow = _check_out(count, max_rows)
    _check(lib().h2hip_check_shuffles_bn254_device(k, _ptr_array(d_compressed_inputs), _ptr_array(d_compressed_shuffles),
                                                   count, blinding_factors, max_rows,
                                                   _p(counts), prow, _stream()), "h2hip_check_shuffles_bn254_device")
    return _check_result(counts, rows, count, max_rows)


def set_lookup_sort(lds_keys=0):
    """test hook: force the lookup sort's in-LDS block (a power of two in [4, 1024]; 0 = default)"""
    _check(lib().h2hip_debug_set_lookup_sort(lds_keys), "h2hip_debug_set_lookup_sort")


def lookup_sort_stats():
    """(block, merge passes) of the last lookup sort (a permute or a lookup-check call)"""
    out = (ctypes.c_uint32 * 2)()
    _check(lib().h2hip_debug_lookup_sort_stats(out), "h2hip_debug_lookup_sort_stats")
    return int(out[0]), int(out[1])


def copies_sort_plan(n_copies):
    """(block, merge passes) of permutation_mapping's sort for n_copies copies: the keys one workgroup sorts in LDS, and the passes after"""
    out = (ctypes.c_uint32 * 2)()
    _check(lib().h2hip_debug_copies_sort_plan(n_copies, out), "h2hip_debug_copies_sort_plan")
    return int(out[0]), int(out[1])


def _opt_ptr_array(tensors):
    return None if tensors is None else _ptr_array(tensors)


def permutation_keygen_device(domain, d_mapping, d_permutations=None, d_polys=None, d_cosets=None, delta=None):
    """permutation_keygen over torch CUDA tensors: d_mapping[j] holds 2^k (column, row) uint32 pairs (8 B per cell); each output is a list
    of m tensors (2^k x 32 B; cosets 2^extended_k x 32 B) or None.  Queued on the current stream, which the call waits for once at its end
    (the out-of-range flag)."""
    d = fr_from_int(FR_DELTA) if delta is None else _fe(delta)
    _check(lib().h2hip_permutation_keygen_bn254_device(*_domain_args(domain), _p(d), _ptr_array(d_mapping), len(d_mapping),
                                                       _opt_ptr_array(d_permutations), _opt_ptr_array(d_polys), _opt_ptr_array(d_cosets),
                                                       _stream()), "h2hip_permutation_keygen_bn254_device")


def permutation_mapping_device(k, n_columns, d_copies, d_mapping, n_copies=None):
    """permutation_mapping over torch CUDA tensors: d_copies holds n_copies x 16 B (None with no copy), d_mapping[j] receives 2^k
    (column, row) uint32 pairs (8 B per cell).  Queued on the current stream, which the call waits for once at its end (the flag of a
    copy out of range: H2HipError, the mapping of the valid copies written)."""
    if n_copies is None:
        n_copies = 0 if d_copies is None else d_copies.numel() * d_copies.element_size() // 16
    _check(lib().h2hip_permutation_mapping_device(k, n_columns, None if d_copies is None else _dptr(d_copies),
                                                  n_copies, _ptr_array(d_mapping), _stream()), "h2hip_permutation_mapping_device")


def permutation_keygen_from_copies(domain, n_columns, copies, want=_KEYGEN_FORMS, delta=None):
    """permutation_keygen from the copy constraints themselves: the copies are uploaded (16 B each), permutation_mapping_device builds
    the ordered mapping in device memory and permutation_keygen_device reads it there, so the 8-byte-per-cell mapping never crosses
    PCIe.  Returns what permutation_keygen(domain, permutation_mapping(k, n_columns, copies), want, delta) returns."""
    import torch
    want = _keygen_want(want)
    k, m = int(domain.k), int(n_columns)
    n = 1 << k
    c = _copies_array(copies)
    sizes = {"permutations": n, "polys": n, "cosets": domain.extended_len()}
    if m == 0:
        return {w: [] for w in want}
    d_copies = torch.from_numpy(c.view(np.int32)).cuda() if c.shape[0] else None
    d_map = [torch.empty((n, 2), dtype=torch.int32, device="cuda") for _ in range(m)]
    permutation_mapping_device(k, m, d_copies, d_map, c.shape[0])
    d_out = {w: [torch.empty((sizes[w], 4), dtype=torch.int64, device="cuda") for _ in range(m)] for w in want}
    permutation_keygen_device(domain, d_map, d_out.get("permutations"), d_out.get("polys"), d_out.get("cosets"), delta)
    return {w: [to_numpy_u64(t) for t in d_out[w]] for w in want}


def batch_invert_assigned_device(k, d_numerators, d_rat_rows, rat_counts, d_rat_denoms, d_out):
    """batch_invert_assigned over torch CUDA tensors; d_rat_rows[j] / d_rat_denoms[j] may be None where rat_counts[j] == 0; d_out[j] may
    be d_numerators[j].  Queued on the current stream, not waited for."""
    m = len(d_numerators)
    opt = lambda ts: (ctypes.c_void_p * max(1, m))(*[(None if t is None else t.data_ptr()) for t in ts])
    cnt = (ctypes.c_size_t * max(1, m))(*[int(x) for x in rat_counts])
    _check(lib().h2hip_batch_invert_assigned_bn254_device(k, _ptr_array(d_numerators), opt(d_rat_rows), cnt, opt(d_rat_denoms),
                                                          m, _ptr_array(d_out), _stream()),
           "h2hip_batch_invert_assigned_bn254_device")


def key_lagrange_columns_device(domain, blinding_factors, d_l0, d_l_last, d_l_active_row):
    """key_lagrange_columns into three torch CUDA tensors of 2^extended_k x 32 B; queued on the current stream, not waited for"""
    _check(lib().h2hip_key_lagrange_columns_bn254_device(domain.k, _p(domain.omega_inv), _p(domain.ifft_divisor),
                                                         domain.extended_k, _p(domain.extended_omega), _p(domain.g_coset),
                                                         _p(domain.g_coset_inv), blinding_factors, _dptr(d_l0), _dptr(d_l_last),
                                                         _dptr(d_l_active_row), _stream()), "h2hip_key_lagrange_columns_bn254_device")


def set_keygen_group(group_bytes=0):
    """test hook: the HBM one group of columns of a host-pointer keygen call takes (0 = default), so that small inputs run several groups"""
    _check(lib().h2hip_debug_set_keygen_group(group_bytes), "h2hip_debug_set_keygen_group")


def g1_from_bytes_device(d_bytes, d_points, n):
    """d_bytes: n x 32 B, d_points: n x 64 B (torch CUDA tensors); H2HipEncodingError when an encoding is invalid (d_points is written whole)"""
    invalid = np.zeros(2, dtype=np.uint64)
    _check_encoding(lib().h2hip_g1_decompress_bn254_device(_dptr(d_bytes), n, _dptr(d_points), _p(invalid), _stream()),
                    "h2hip_g1_decompress_bn254_device", invalid)


def g1_to_bytes_device(d_points, d_bytes, n):
    _check(lib().h2hip_g1_compress_bn254_device(_dptr(d_points), n, _dptr(d_bytes), _stream()), "h2hip_g1_compress_bn254_device")


def g1_validate_device(d_points, n):
    invalid = np.zeros(2, dtype=np.uint64)
    _check_encoding(lib().h2hip_g1_validate_bn254_device(_dptr(d_points), n, _p(invalid), _stream()),
                    "h2hip_g1_validate_bn254_device", invalid)


def fr_from_repr_device(d_repr, d_out, n):
    """d_out may be d_repr"""
    invalid = np.zeros(2, dtype=np.uint64)
    _check_encoding(lib().h2hip_fr_from_repr_bn254_device(_dptr(d_repr), n, _dptr(d_out), _p(invalid), _stream()),
                    "h2hip_fr_from_repr_bn254_device", invalid)


def fr_to_repr_device(d_in, d_repr, n):
    _check(lib().h2hip_fr_to_repr_bn254_device(_dptr(d_in), n, _dptr(d_repr), _stream()), "h2hip_fr_to_repr_bn254_device")


def gen_scalars_device(seed, n, start=0, device="cuda"):
    import torch
    out = torch.empty((n, 4), dtype=torch.int64, device=device)
    _check(lib().h2hip_gen_scalars_device(seed, start, n, _dptr(out), _stream()),
           "h2hip_gen_scalars_device")
    return out


def gen_points_device(seed, n, start=0, device="cuda"):
    import torch
    out = torch.empty((n, 8), dtype=torch.int64, device=device)
    _check(lib().h2hip_gen_points_device(seed, start, n, _dptr(out), _stream()),
           "h2hip_gen_points_device")
    return out


# ------------------------------------------------------------------ randomness (csrc/random.hip)
def _seed32(seed):
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("a seed is 32 bytes, got %d" % len(seed))
    return (ctypes.c_uint8 * 32).from_buffer_copy(seed)


def fr_random(seed, n, first_block=0, stream_id=0):
    """n draws of Fr::random from ChaCha20Rng::from_seed(seed) that has made first_block draws: element i is Fr::from_bytes_wide of
    ChaCha20 block first_block + i -> (n, 4) uint64 Montgomery.  Below HALO2_HIP_RANDOM_MIN_N elements this runs on the calling thread
    and needs no GPU.  The seed is as secret as the elements: the engine expands it and adds no entropy."""
    out = np.zeros((int(n), 4), dtype=np.uint64)
    _check(lib().h2hip_fr_random_bn254(_seed32(seed), stream_id, first_block, int(n), _p(out)),
           "h2hip_fr_random_bn254")
    return out


def fr_random_device(seed, n, first_block=0, stream_id=0, out=None):
    """the same draws left in HBM: a torch CUDA tensor (n, 4) int64, `out` when given (n x 32 B); the kernel is queued, not waited for"""
    if out is None:
        if device_count() < 1:
            raise H2HipError("fr_random_device: no GPU (no CPU fallback exists)")
        import torch
        out = torch.empty((int(n), 4), dtype=torch.int64, device="cuda")
    _check(lib().h2hip_fr_random_bn254_device(_seed32(seed), stream_id, first_block, int(n),
                                              _dptr(out), _stream()), "h2hip_fr_random_bn254_device")
    return out


def fr_from_bytes_wide(data):
    """Fr::from_bytes_wide over (n, 64) uint8: each 64 bytes as one little-endian integer mod r -> (n, 4) uint64 Montgomery"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    if data.ndim != 2 or data.shape[1] != 64:
        raise ValueError("fr_from_bytes_wide: expected shape (n,64), got %s" % (data.shape,))
    out = np.zeros((data.shape[0], 4), dtype=np.uint64)
    _check(lib().h2hip_fr_from_bytes_wide_bn254(_p(data), data.shape[0], _p(out)), "h2hip_fr_from_bytes_wide_bn254")
    return out


def fr_from_bytes_wide_device(d_bytes, d_out, n):
    """d_bytes: n x 64 B, d_out: n x 32 B (torch CUDA tensors, not overlapping); queued on the current stream"""
    _check(lib().h2hip_fr_from_bytes_wide_bn254_device(_dptr(d_bytes), n, _dptr(d_out), _stream()),
           "h2hip_fr_from_bytes_wide_bn254_device")


class FrRng:
    """ChaCha20Rng::from_seed(seed) as far as Fr::random uses it: every draw consumes one 64-byte block, so the state is the number of
    the next block.  draw / draw_device hand out consecutive blocks, which lets a mirror prover take all of a proof's draws from one
    stream in the reference's order, whichever of them are made on the GPU.  The seed is as secret as everything drawn from it; this
    object keeps it as Python bytes, which cannot be wiped (the library wipes its own copies, the C++ mirror's FrRng its seed)."""

    def __init__(self, seed, stream_id=0):
        self.seed, self.stream_id, self.block = bytes(seed), int(stream_id), 0
        _seed32(self.seed)

    def draw(self, n=1):
        out = fr_random(self.seed, n, self.block, self.stream_id)
        self.block += int(n)
        return out

    def draw_device(self, n, out=None):
        out = fr_random_device(self.seed, n, self.block, self.stream_id, out)
        self.block += int(n)
        return out


def vanishing_commit(params, domain, rng):
    """vanishing::Argument::commit (plonk/vanishing/prover.rs:36-67) with rng an FrRng: the random polynomial of 2^k coefficients is drawn
    into HBM (blocks [c, c + 2^k) of the stream), its blind is the next draw (block c + 2^k), and the commitment is the MSM over the
    resident, pinned g.  Returns (the device polynomial (2^k, 4), the blind (4,), the commitment (12,) Jacobian); nothing of 2^k
    elements crosses PCIe.  Writing the commitment to the transcript stays with the caller."""
    n = 1 << domain.k
    assert params.g.shape[0] >= n  # assert!(bases.len() >= size), poly/kzg/commitment.rs:332
    d_poly = rng.draw_device(n)
    blind = rng.draw(1)[0]
    return d_poly, blind, params.commit_device(d_poly, n)


def to_numpy_u64(t):
    return t.detach().cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------ tuning / measurement
def set_msm_window(c):
    _check(lib().h2hip_set_msm_window(c), "h2hip_set_msm_window")


def get_msm_window(n):
    return int(lib().h2hip_get_msm_window(n))


def get_msm_window_fixed_base(n):
    return int(lib().h2hip_get_msm_window_fixed_base(n))


def msm_min_n():
    return int(lib().h2hip_msm_min_n())


def ntt_min_log_n():
    return int(lib().h2hip_ntt_min_log_n())


def lazy_pin_after():
    """HALO2_HIP_LAZY_PIN: unpinned sightings of a host bases array after which the library pins it itself (0 = never)"""
    return int(lib().h2hip_lazy_pin_after())


def profile_enable(on=True):
    """True / 1: every stage; 2: only the dominant kernel, through its own dispatch (no gaps); False / 0: off"""
    _check(lib().h2hip_profile_enable(int(on)), "h2hip_profile_enable")


def profile_reset():
    _check(lib().h2hip_profile_reset(), "h2hip_profile_reset")


def profile_get(stage):
    ms = ctypes.c_double(0)
    cnt = ctypes.c_uint64(0)
    _check(lib().h2hip_profile_get(stage.encode(), ctypes.byref(ms), ctypes.byref(cnt)), "h2hip_profile_get")
    return ms.value, cnt.value
