"""Serialisation on the GPU (csrc/serde.hip): SerdeFormat::Processed / RawBytes for params files and polynomial vectors, byte for byte
against the Python-integer reference of tests/serde_util.py.  CPU tests cover the reference itself, the fixture, the host build of the
per-element code (fu_sqrt with its bounds asserted) and the host-only G2 encoding; GPU tests cover the kernels, the C ABI's failure
reporting, ParamsKZG.read / write and the C++ mirror."""
import io
import os
import subprocess

import numpy as np
import pytest

import serde_util as ref
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden")
N_BIG = (1 << 12) + 1


def _raw():
    return open(os.path.join(GOLDEN, "kzg_6_params.rawbytes"), "rb").read()


def _processed():
    return open(os.path.join(GOLDEN, "kzg_6_params.processed"), "rb").read()


def _compressed(x, sign=0, bit254=0):
    b = bytearray(x.to_bytes(32, "little"))
    b[31] |= sign << 7 | bit254 << 6
    return bytes(b)


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_reference_converts_the_fixtures_both_ways():
    raw, proc = _raw(), _processed()
    assert len(proc) == 4 + 2 * 64 * 32 + 128
    assert ref.params_raw_to_processed(raw) == proc
    assert ref.params_processed_to_raw(proc) == raw


def test_known_encodings_of_the_generator():
    assert ref.g1_compress_one(1, 2) == bytes([1]) + bytes(31)
    assert ref.g1_compress_one(1, ref.Q - 2) == bytes([1]) + bytes(30) + bytes([0x80])
    assert ref.g1_decompress_one(bytes([1]) + bytes(31)) == (1, 2)
    assert ref.g1_decompress_one(bytes([1]) + bytes(30) + bytes([0x80])) == (1, ref.Q - 2)
    assert ref.g1_decompress_one(bytes(32)) == (0, 0)
    # the invalid encodings the GPU tests plant: non-residues, x >= q, the sign bit on x = 0
    for x in (4, 10, 12, 0):
        assert ref.sqrt_q((x ** 3 + 3) % ref.Q) is None
    assert ref.g1_decompress_one(_compressed(4)) is None and ref.g1_decompress_one(_compressed(0, sign=1)) is None
    assert ref.g1_decompress_one(ref.Q.to_bytes(32, "little")) is None and ref.g1_decompress_one(_compressed(1, bit254=1)) is None
    assert sum(ref.g1_decompress_one(_compressed(x)) is None for x in range(1, 2001)) == 982


def test_per_element_code_on_the_host(tmp_path):
    """csrc/serde_elem.h and fu_sqrt on the host against fe_pow, with -DH2_FU_CHECK asserting every product's limb bounds"""
    exe = str(tmp_path / "test_serde_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DH2_FU_CHECK", "-Wall", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_serde_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "serde host tests ok" in r.stdout, r.stdout + r.stderr


def test_g2_encoding_on_the_host(h2):
    """the G2 generator of EIP-197, its negation and the identity between 128 B raw and 64 B compressed; all on the twist"""
    x, y = ref.G2_GEN
    assert ref.g2_on_twist(x, y)
    neg = ((-y[0]) % ref.Q, (-y[1]) % ref.Q)
    for yy in (y, neg):
        raw = ref.g2_raw(x, yy)
        comp = ref.g2_compress(raw)
        assert len(comp) == 64 and comp[63] >> 7 == yy[0] & 1
        assert h2.g2_to_bytes(raw) == comp and h2.g2_from_bytes(comp) == raw and ref.g2_decompress(comp) == raw
        assert ref.g2_on_twist(*ref.g2_raw_to_plain(h2.g2_from_bytes(comp)))
        assert h2._g2_raw(raw, check=True) == raw
    assert ref.g2_compress(ref.g2_raw(x, y)) != ref.g2_compress(ref.g2_raw(x, neg))
    assert h2.g2_to_bytes(bytes(128)) == bytes(64) and h2.g2_from_bytes(bytes(64)) == bytes(128)
    assert h2._g2_raw(bytes(128), check=True) == bytes(128)
    bad = bytearray(ref.g2_raw(x, y))
    bad[64] ^= 1
    with pytest.raises(h2.H2HipError):
        h2._g2_raw(bytes(bad), check=True)
    with pytest.raises(h2.H2HipError):  # x.c1 = q
        h2.g2_from_bytes(bytes(32) + ref.Q.to_bytes(32, "little"))
    not_square = next(c for c in range(1, 50) if ref.g2_decompress(c.to_bytes(32, "little") + bytes(32)) is None)
    with pytest.raises(h2.H2HipError):
        h2.g2_from_bytes(not_square.to_bytes(32, "little") + bytes(32))


def test_interface_is_present(h2):
    assert [f.name for f in h2.SerdeFormat] == ["Processed", "RawBytes", "RawBytesUnchecked"]
    for name in ("read", "read_custom", "write", "write_custom"):
        assert callable(getattr(h2.ParamsKZG, name))
    L = h2.lib()
    for stem in ("g1_decompress", "g1_compress", "g1_validate", "fr_from_repr", "fr_to_repr"):
        assert hasattr(L, "h2hip_%s_bn254" % stem) and hasattr(L, "h2hip_%s_bn254_device" % stem)
    header = open(os.path.join(ROOT, "include", "halo2hip.h")).read()
    assert "#define H2HIP_EENCODING 5" in header and h2.H2HIP_EENCODING == 5


def test_raw_polynomials_need_no_gpu(h2):
    vals = [0, 1, ref.R - 1, ref.MONT % ref.R, 0x1234567890abcdef << 100]
    polys = [ref.limbs([v * ref.RR % ref.R for v in vals]), ref.limbs([7 * ref.RR % ref.R])]
    for fmt in (h2.SerdeFormat.RawBytes, h2.SerdeFormat.RawBytesUnchecked):
        w = io.BytesIO()
        h2.write_polynomial_slice(polys, w, fmt)
        assert w.getvalue() == (2).to_bytes(4, "big") + (5).to_bytes(4, "big") + polys[0].tobytes() + (1).to_bytes(4, "big") + polys[1].tobytes()
        back = h2.read_polynomial_vec(io.BytesIO(w.getvalue()), fmt)
        assert len(back) == 2 and all(np.array_equal(a, b) for a, b in zip(back, polys))
    bad = (1).to_bytes(4, "big") + ref.R.to_bytes(32, "little")
    with pytest.raises(h2.H2HipError):
        h2.read_polynomial(io.BytesIO(bad), h2.SerdeFormat.RawBytes)
    assert h2.read_polynomial(io.BytesIO(bad), h2.SerdeFormat.RawBytesUnchecked).shape == (1, 4)
    with pytest.raises(h2.H2HipError):
        h2.read_polynomial(io.BytesIO(bad[:20]), h2.SerdeFormat.RawBytes)


def test_no_gpu_means_loud_failure(h2):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(h2.H2HipError):
        h2.g1_from_bytes(np.zeros((1, 32), dtype=np.uint8))
    with pytest.raises(h2.H2HipError):
        h2.ParamsKZG.read(io.BytesIO(_raw()))


# ---------------------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def big(h2):
    """N_BIG valid points and their encodings, computed once: the fixture's 64 points, then h2hip_gen_points_device output; odd
    indices carry the other sign bit, so y and q - y both appear; identities at the first, the last and some interior indices"""
    h2.init(0)
    fix = np.frombuffer(_raw()[4:4 + 64 * 64], dtype=np.uint64).reshape(64, 8)
    pts = np.concatenate([fix, h2.to_numpy_u64(h2.gen_points_device(0x5EED5E2D, N_BIG - 64))])
    assert not ref.g1_invalid(pts)
    data = ref.g1_to_bytes(pts)
    data[1::2, 31] ^= 0x80
    want, bad = ref.g1_from_bytes(data)
    assert not bad and np.array_equal(want[0::2], pts[0::2]) and not np.array_equal(want[1::2], pts[1::2])
    return {"bytes": data, "points": want}


def _with_identities(big, n):
    data, want = big["bytes"][:n].copy(), big["points"][:n].copy()
    if n >= 4:  # n = 1 keeps its one point
        for i in {0, n - 1, n // 2, n // 3}:
            data[i], want[i] = 0, 0
    return data, want


def _device_decompress(h2, data):
    import torch
    n = data.shape[0]
    d_in, d_out = torch.from_numpy(data).cuda(), torch.full((n, 8), -1, dtype=torch.int64, device="cuda")
    h2.g1_from_bytes_device(d_in, d_out, n)
    return d_out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, N_BIG])
def test_decompress_matches_the_reference_and_compress_inverts_it(h2, big, n):
    import torch
    data, want = _with_identities(big, n)
    got = h2.g1_from_bytes(data)
    assert np.array_equal(got, want)
    assert np.array_equal(h2.g1_to_bytes(got), data)
    h2.g1_validate(got)
    d_pts = _device_decompress(h2, data)
    assert np.array_equal(h2.to_numpy_u64(d_pts), want)
    h2.g1_validate_device(d_pts, n)
    d_back = torch.full((n, 32), 0x55, dtype=torch.uint8, device="cuda")
    h2.g1_to_bytes_device(d_pts, d_back, n)
    torch.cuda.synchronize()
    assert np.array_equal(d_back.cpu().numpy(), data)


@pytest.mark.gpu
def test_the_generator_on_the_gpu(h2):
    h2.init(0)
    pts = ref.points([(1, 2), (1, ref.Q - 2), None])
    enc = h2.g1_to_bytes(pts)
    assert enc[0].tobytes() == bytes([1]) + bytes(31) and enc[1].tobytes() == bytes([1]) + bytes(30) + bytes([0x80]) and enc[2].tobytes() == bytes(32)
    assert np.array_equal(h2.g1_from_bytes(enc), pts)
    assert h2.g1_from_bytes(np.zeros((0, 32), dtype=np.uint8)).shape == (0, 8)  # n == 0 succeeds


INVALID = {"x=4": _compressed(4), "x=10": _compressed(10), "x=12,sign": _compressed(12, sign=1), "x=q": ref.Q.to_bytes(32, "little"),
           "x=1,bit254": _compressed(1, bit254=1), "x=0,sign": _compressed(0, sign=1)}


def _expect_invalid(h2, call, planted, want):
    """`call` must raise with H2HIP_EENCODING, the planted count and lowest index, zeros at the planted outputs and `want` elsewhere"""
    with pytest.raises(h2.H2HipEncodingError) as e:
        call()
    err = e.value
    assert err.rc == ref.H2HIP_EENCODING and (err.count, err.index) == (len(planted), min(planted))
    if want is not None:
        expect = want.copy()
        expect[sorted(planted)] = 0
        assert np.array_equal(err.output, expect)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(INVALID))
def test_one_invalid_encoding_is_counted_and_located(h2, big, case):
    n = 131  # three waves, the last one partial
    for at in (0, n - 1, 70):
        data, want = _with_identities(big, n)
        data[at] = np.frombuffer(INVALID[case], dtype=np.uint8)
        assert ref.g1_from_bytes(data)[1] == [at]
        _expect_invalid(h2, lambda: h2.g1_from_bytes(data), [at], want)


@pytest.mark.gpu
def test_three_invalid_encodings_and_the_device_form(h2, big):
    n = N_BIG
    planted = [4096, 777, 3000]
    data, want = _with_identities(big, n)
    for at, case in zip(planted, ("x=4", "x=q", "x=0,sign")):
        data[at] = np.frombuffer(INVALID[case], dtype=np.uint8)
    _expect_invalid(h2, lambda: h2.g1_from_bytes(data), planted, want)
    import torch
    d_in, d_out = torch.from_numpy(data).cuda(), torch.full((n, 8), -1, dtype=torch.int64, device="cuda")
    _expect_invalid(h2, lambda: h2.g1_from_bytes_device(d_in, d_out, n), planted, None)
    want[planted] = 0
    assert np.array_equal(h2.to_numpy_u64(d_out), want)


@pytest.mark.gpu
def test_mostly_invalid_input(h2):
    """x = 1 .. 2000 with the sign bit clear: 982 encodings are invalid.  Every element is converted, none is skipped."""
    h2.init(0)
    data = np.frombuffer(b"".join(_compressed(x) for x in range(1, 2001)), dtype=np.uint8).reshape(-1, 32)
    want, bad = ref.g1_from_bytes(data)
    assert len(bad) == 982
    _expect_invalid(h2, lambda: h2.g1_from_bytes(data), bad, want)


@pytest.mark.gpu
def test_validate_flags_what_read_raw_rejects(h2, big):
    n = 200
    pts = big["points"][:n].copy()
    pts[5] = 0                                             # (0, 0): the identity, accepted
    h2.g1_validate(pts)
    one, three = ref.QR, 3 * ref.QR % ref.Q
    bad = {0: (one, three), 64: None, 150: (0, one), n - 1: (one, three)}   # (1, 3); y = q; (0, 1); (1, 3) in the last place
    for at, xy in bad.items():
        pts[at] = ref.limbs(xy).reshape(8) if xy else np.concatenate([pts[at][:4], ref.limbs([ref.Q])[0]])
    assert ref.g1_invalid(pts) == sorted(bad)
    for planted in ([0], [64], [150], [n - 1], sorted(bad)):
        p = big["points"][:n].copy()
        p[planted] = pts[planted]
        _expect_invalid(h2, lambda: h2.g1_validate(p), planted, None)
    import torch
    d = torch.from_numpy(pts.view(np.int64)).cuda()
    _expect_invalid(h2, lambda: h2.g1_validate_device(d, n), sorted(bad), None)


@pytest.mark.gpu
def test_fr_conversions(h2):
    import torch
    h2.init(0)
    rng = np.random.default_rng(0x5E2D)
    vals = [0, 1, ref.R - 1, ref.MONT % ref.R] + [int.from_bytes(rng.bytes(32), "little") % ref.R for _ in range(300)]
    repr_ = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint8).reshape(-1, 32)
    mont = ref.limbs([v * ref.RR % ref.R for v in vals])
    assert np.array_equal(ref.fr_from_repr(repr_)[0], mont) and np.array_equal(ref.fr_to_repr(mont), repr_)
    assert np.array_equal(h2.fr_from_repr(repr_), mont)
    assert np.array_equal(h2.fr_to_repr(mont), repr_)
    assert np.array_equal(mont[3], ref.limbs([ref.RR * ref.RR % ref.R])[0])
    # in place on the device, both ways
    n = len(vals)
    d = torch.from_numpy(repr_.copy()).cuda()
    h2.fr_from_repr_device(d, d, n)
    assert np.array_equal(d.cpu().numpy().view(np.uint64).reshape(n, 4), mont)
    h2.fr_to_repr_device(d, d, n)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), repr_)
    # r and 2^256 - 1 are rejected with their indices; the other outputs stand
    bad = repr_.copy()
    bad[7] = np.frombuffer(ref.R.to_bytes(32, "little"), dtype=np.uint8)
    bad[n - 1] = 0xff
    _expect_invalid(h2, lambda: h2.fr_from_repr(bad), [7, n - 1], mont)
    bad[0] = 0xff
    _expect_invalid(h2, lambda: h2.fr_from_repr(bad), [0, 7, n - 1], mont)
    # polynomial vectors in the Processed format (poly.rs:152-177, helpers.rs:116-140)
    w = io.BytesIO()
    h2.write_polynomial_slice([mont, mont[:3]], w, h2.SerdeFormat.Processed)
    assert w.getvalue() == (2).to_bytes(4, "big") + n.to_bytes(4, "big") + repr_.tobytes() + (3).to_bytes(4, "big") + repr_[:3].tobytes()
    back = h2.read_polynomial_vec(io.BytesIO(w.getvalue()), h2.SerdeFormat.Processed)
    assert np.array_equal(back[0], mont) and np.array_equal(back[1], mont[:3])
    with pytest.raises(h2.H2HipError):
        h2.read_polynomial(io.BytesIO((1).to_bytes(4, "big") + ref.R.to_bytes(32, "little")), h2.SerdeFormat.Processed)


@pytest.mark.gpu
def test_params_files_in_all_formats(h2, golden):
    h2.init(0)
    raw, proc = _raw(), _processed()
    fmt = h2.SerdeFormat
    with h2.ParamsKZG.read(io.BytesIO(raw)) as a, h2.ParamsKZG.read_custom(io.BytesIO(proc), fmt.Processed) as b, \
            h2.ParamsKZG.read_custom(io.BytesIO(raw), fmt.RawBytesUnchecked) as c:
        for p in (a, b, c):
            assert p.k == 6 and np.array_equal(p.g, golden["kzg_6_g"]) and np.array_equal(p.g_lagrange, golden["kzg_6_g_lagrange"])
            assert p.g2 == bytes(128) and p.s_g2 == bytes(128)
            assert np.array_equal(h2.g1_to_affine(p.commit_lagrange(golden["kzg_6_poly_lagrange"])), golden["kzg_6_commit_lagrange"])
            assert np.array_equal(h2.g1_to_affine(p.commit(golden["kzg_6_poly_coeff"])), golden["kzg_6_commit_lagrange"])
            for f, want in ((fmt.RawBytes, raw), (fmt.RawBytesUnchecked, raw), (fmt.Processed, proc)):
                w = io.BytesIO()
                p.write_custom(w, f)
                assert w.getvalue() == want
            w = io.BytesIO()
            p.write(w)
            assert w.getvalue() == raw
        b.downsize(4)
        assert b.g.shape == (16, 8) and np.array_equal(b.g, golden["kzg_6_g"][:16])
    # non-trivial G2 points travel through both formats
    x, y = ref.G2_GEN
    g2, s_g2 = ref.g2_raw(x, y), ref.g2_raw(x, ((-y[0]) % ref.Q, (-y[1]) % ref.Q))
    with h2.ParamsKZG(6, golden["kzg_6_g"], golden["kzg_6_g_lagrange"], g2=g2, s_g2=s_g2) as p:
        w = io.BytesIO()
        p.write_custom(w, fmt.Processed)
        assert w.getvalue() == proc[:-128] + ref.g2_compress(g2) + ref.g2_compress(s_g2)
        with h2.ParamsKZG.read_custom(io.BytesIO(w.getvalue()), fmt.Processed) as back:
            assert back.g2 == g2 and back.s_g2 == s_g2 and np.array_equal(back.g_lagrange, p.g_lagrange)


@pytest.mark.gpu
def test_truncated_and_corrupted_files_raise(h2):
    h2.init(0)
    raw, proc = _raw(), _processed()
    fmt = h2.SerdeFormat
    for data, f in ((raw, fmt.RawBytes), (proc, fmt.Processed)):
        for cut in (2, 4 + 100, len(data) - 1):
            with pytest.raises(h2.H2HipError):
                h2.ParamsKZG.read_custom(io.BytesIO(data[:cut]), f)
    bad = bytearray(proc)
    bad[4 + 32 * 70:4 + 32 * 71] = _compressed(4)      # g_lagrange[6]: x^3 + 3 is not a square
    with pytest.raises(h2.H2HipEncodingError) as e:
        h2.ParamsKZG.read_custom(io.BytesIO(bytes(bad)), fmt.Processed)
    assert (e.value.count, e.value.index) == (1, 6)
    bad = bytearray(raw)
    bad[4 + 64 * 9 + 32] ^= 1                           # g[9].y
    with pytest.raises(h2.H2HipEncodingError) as e:
        h2.ParamsKZG.read(io.BytesIO(bytes(bad)))
    assert (e.value.count, e.value.index) == (1, 9)
    h2.ParamsKZG.read_custom(io.BytesIO(bytes(bad)), fmt.RawBytesUnchecked).close()   # no checks (helpers.rs:19-20)


@pytest.mark.gpu
def test_cpp_mirror_reads_and_writes_all_formats():
    exe = os.path.join(ROOT, "tests", "cpp", "test_serde_mirror")
    assert os.path.exists(exe), "tests/cpp/test_serde_mirror is not built (halo2-pse_amd/Makefile)"
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "serde mirror tests ok" in r.stdout, r.stdout + r.stderr
