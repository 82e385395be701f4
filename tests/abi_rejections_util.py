"""Calls that libhalo2hip.so rejects with H2HIP_EINVAL before the engine is entered, so that they answer the same with or without
a GPU: the candidate table (tests/golden/make_abi_rejections.py keeps the rows a build really rejects that way), and how a row
recorded in tests/golden/abi_rejections.json becomes a ctypes call (tests/test_abi_rejections.py).

A row is {"fn", "case", "args"}; an argument is one of the tokens below or {"u32" | "u64" | "size": value}.  Several entry points
return H2HIP_EINVAL without a text of their own for some mistakes (the batch transforms for a null scalar or k > extended_k); so that
what h2hip_last_error() then holds is defined, every call is preceded by PRIMER, a rejected call with a text of its own."""
import ctypes

H2HIP_EINVAL = 1
PRIMER = {"fn": "h2hip_g1_fold", "args": ["null", {"size": 1}, "null"], "rc": H2HIP_EINVAL, "error": "g1_fold: null argument"}
UNREDUCED = [0xFFFFFFFFFFFFFFFF] * 4  # 2^256 - 1
ONE = [1, 0, 0, 0]


def materialise(args, keep):
    """ctypes values for a row's arguments; `keep` collects the buffers they point into"""
    out = []
    for a in args:
        if isinstance(a, dict):
            (kind, v), = a.items()
            out.append({"u32": ctypes.c_uint32, "u64": ctypes.c_uint64, "size": ctypes.c_size_t}[kind](v))
            continue
        if a == "null":
            out.append(ctypes.c_void_p(None))
            continue
        if a == "buf":  # any non-null block: a rejected call reads none of it
            v = (ctypes.c_uint64 * 4096)()
        elif a == "one":
            v = (ctypes.c_uint64 * 4)(*ONE)
        elif a == "unreduced":
            v = (ctypes.c_uint64 * 4)(*UNREDUCED)
        elif a in ("cols", "cols_null1"):  # a table of two columns; cols_null1: the second one missing
            b = (ctypes.c_uint64 * 4096)()
            keep.append(b)
            v = (ctypes.c_void_p * 2)(ctypes.addressof(b), None if a == "cols_null1" else ctypes.addressof(b))
        elif a == "t2":  # two t_evaluations
            v = (ctypes.c_uint64 * 8)(*(ONE + ONE))
        elif a == "t2_unreduced":
            v = (ctypes.c_uint64 * 8)(*(ONE + UNREDUCED))
        else:
            raise ValueError(a)
        keep.append(v)
        out.append(v)
    return out


def call(L, row):
    """(return code, h2hip_last_error() text) of a row's call on library handle L, after the primer"""
    L.h2hip_last_error.restype = ctypes.c_char_p
    keep = []
    rc = getattr(L, PRIMER["fn"])(*materialise(PRIMER["args"], keep))
    assert (rc, L.h2hip_last_error().decode()) == (PRIMER["rc"], PRIMER["error"]), "the primer call itself answers differently"
    rc = getattr(L, row["fn"])(*materialise(row["args"], keep))
    return rc, L.h2hip_last_error().decode()


# ---- the candidate table -------------------------------------------------------------------------------------------------------
# an entry point's parameters in order: (name, kind, valid token).  Kinds: ptr (also tried NULL), fr (a scalar: also tried NULL and
# unreduced), log (a log2 size: also tried 29), cols (a table of columns: also tried NULL and with a null column), t (t_evaluations:
# also tried NULL and with an unreduced element), val (left alone)
U32 = lambda v: {"u32": v}
SIZE = lambda v: {"size": v}
STREAM = ("stream", "val", "null")
K, EK = ("k", "val", U32(3)), ("extended_k", "log", U32(4))
COSET = [("g_coset", "fr", "one"), ("g_coset_inv", "fr", "one")]
E2C = [("extended_omega_inv", "fr", "one"), ("extended_ifft_divisor", "fr", "one")] + COSET
C2E = [("extended_omega", "fr", "one")] + COSET
COUNT = ("count", "val", SIZE(2))
LOG_N = ("log_n", "log", U32(4))
GEN = [("seed", "val", {"u64": 1}), ("start", "val", {"u64": 0}), ("n", "val", SIZE(16)), ("d_out", "ptr", "buf"), STREAM]

ENTRY_POINTS = {
    # the NTT / domain family
    "h2hip_ntt_bn254_fr_device": [("d_a", "ptr", "buf"), ("omega", "fr", "one"), LOG_N, STREAM],
    "h2hip_ntt_bn254_fr": [("a", "ptr", "buf"), ("omega", "fr", "one"), LOG_N],
    "h2hip_ntt_bn254_fr_batch_device": [("d_a", "cols", "cols"), COUNT, ("omega", "fr", "one"), LOG_N, STREAM],
    "h2hip_ntt_bn254_fr_batch": [("a", "cols", "cols"), COUNT, ("omega", "fr", "one"), LOG_N],
    "h2hip_ifft_bn254_fr_device": [("d_a", "ptr", "buf"), ("omega_inv", "fr", "one"), LOG_N, ("divisor", "fr", "one"), STREAM],
    "h2hip_ifft_bn254_fr": [("a", "ptr", "buf"), ("omega_inv", "fr", "one"), LOG_N, ("divisor", "fr", "one")],
    "h2hip_ifft_bn254_fr_batch_device": [("d_a", "cols", "cols"), COUNT, ("omega_inv", "fr", "one"), LOG_N, ("divisor", "fr", "one"), STREAM],
    "h2hip_ifft_bn254_fr_batch": [("a", "cols", "cols"), COUNT, ("omega_inv", "fr", "one"), LOG_N, ("divisor", "fr", "one")],
    "h2hip_coeff_to_extended_bn254_fr_device": [("d_a", "ptr", "buf"), K, EK] + C2E + [STREAM],
    "h2hip_coeff_to_extended_bn254_fr": [("a", "ptr", "buf"), K, ("out", "ptr", "buf"), EK] + C2E,
    "h2hip_coeff_to_extended_bn254_fr_batch_device": [("d_a", "cols", "cols"), COUNT, K, EK] + C2E + [STREAM],
    "h2hip_coeff_to_extended_bn254_fr_batch": [("a", "cols", "cols"), K, ("out", "cols", "cols"), COUNT, EK] + C2E,
    "h2hip_extended_to_coeff_bn254_fr_device": [("d_a", "ptr", "buf"), EK] + E2C + [STREAM],
    "h2hip_extended_to_coeff_bn254_fr": [("a", "ptr", "buf"), EK] + E2C,
    "h2hip_extended_to_coeff_bn254_fr_batch": [("a", "cols", "cols"), COUNT, EK] + E2C,
    "h2hip_divide_by_vanishing_poly_bn254_fr_device": [("d_a", "ptr", "buf"), EK, ("t_evaluations", "t", "t2"), ("t_len", "val", U32(2)), STREAM],
    "h2hip_divide_by_vanishing_poly_bn254_fr": [("a", "ptr", "buf"), EK, ("t_evaluations", "t", "t2"), ("t_len", "val", U32(2))],
    # the entry points that live in their stage files
    "h2hip_g_to_lagrange_bn254_device": [("d_g_xy", "ptr", "buf"), ("k", "log", U32(3)), ("d_g_lagrange_xy", "ptr", "buf"), STREAM],
    "h2hip_g_to_lagrange_bn254": [("g_xy", "ptr", "buf"), ("k", "log", U32(3)), ("g_lagrange_xy", "ptr", "buf")],
    "h2hip_fft_bn254_g1_device": [("d_a_xyz", "ptr", "buf"), ("omega", "fr", "one"), LOG_N, STREAM],
    "h2hip_fft_bn254_g1": [("a_xyz", "ptr", "buf"), ("omega", "fr", "one"), LOG_N],
    "h2hip_kzg_setup_bn254_device": [("k", "log", U32(3)), ("secret", "fr", "one"), ("d_g_xy", "ptr", "buf"), ("d_g_lagrange_xy", "ptr", "buf"), STREAM],
    "h2hip_kzg_setup_bn254": [("k", "log", U32(3)), ("secret", "fr", "one"), ("g_xy", "ptr", "buf"), ("g_lagrange_xy", "ptr", "buf")],
    "h2hip_evaluate_h_bn254": [("desc", "ptr", "buf"), ("values", "ptr", "buf")],
    "h2hip_evaluate_h_bn254_device": [("desc", "ptr", "buf"), ("d_values", "ptr", "buf"), STREAM],
    "h2hip_gen_scalars_device": GEN,
    "h2hip_gen_points_device": GEN,
}


def candidate_rows():
    """Every mistake the table above describes, one at a time, plus the cases no single parameter expresses.  (evaluate_h's rows hand over
    a blank block as the description: both rows are rejected by the null check, before it is read.)"""
    rows = []
    for fn, params in ENTRY_POINTS.items():
        valid = [tok for _, _, tok in params]

        def add(case, i, tok):
            args = list(valid)
            args[i] = tok
            rows.append({"fn": fn, "case": case, "args": args})

        for i, (name, kind, _) in enumerate(params):
            if kind in ("ptr", "fr", "cols", "t"):
                add("null " + name, i, "null")
            if kind == "fr":
                add("unreduced " + name, i, "unreduced")
            if kind == "log":
                add(name + " = 29", i, U32(29))
            if kind == "cols":
                add("null column in " + name, i, "cols_null1")
            if kind == "t":
                add("unreduced element of " + name, i, "t2_unreduced")
        names = [name for name, _, _ in params]
        if "k" in names and "extended_k" in names:
            args = list(valid)
            args[names.index("k")] = U32(5)
            rows.append({"fn": fn, "case": "k > extended_k", "args": args})
        if "t_len" in names:
            args = list(valid)
            args[names.index("t_len")] = U32(0)
            rows.append({"fn": fn, "case": "t_len == 0", "args": args})
    for c in (1, 25):
        rows.append({"fn": "h2hip_set_msm_window", "case": "c = %d" % c, "args": [U32(c)]})
    return rows
