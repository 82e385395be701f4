"""Fr::random over a column on the GPU (csrc/random.hip): ChaCha20Rng::from_seed(seed) followed by Fr::from_bytes_wide, limb for limb
against the numpy / Python-integer reference of tests/random_util.py.  CPU tests cover the reference itself (two published ChaCha20
blocks, one pinned draw), the host build of the per-element code with its limb bounds asserted, and the host forms of the C ABI, which
run on the calling thread below their threshold; GPU tests cover the kernels, the counter's edges, vanishing_commit and the C++ mirror."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import random_util as ref
from conftest import ROOT

SEED_ZERO = bytes(32)
SEED_RAMP = bytes(range(32))
SEED_RAND = np.random.default_rng(0x7A2D0).bytes(32)
SEEDS = {"zero": SEED_ZERO, "ramp": SEED_RAMP, "random": SEED_RAND}
STREAM = 0x0123456789abcdef
RFC_BLOCK = ("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4ed2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
PINNED = 0x1c59a59b6cff4308740943526ade1d8c09f71b337a67269cc89586bcdd6dfcba


# ---------------------------------------------------------------------------------------------------------------------------- CPU
def test_reference_chacha20_against_two_known_blocks():
    zero = ref.chacha20_blocks(SEED_ZERO, [0])[0].tobytes()
    assert zero.hex().startswith("76b8e0ada0f13d90405d6ae55386bd28") and zero.hex().endswith("b2ee6586")
    assert int.from_bytes(zero[:4], "little") == 0xade0b876          # rand_chacha's zero-seed vector, first word
    # RFC 7539 2.3.2: counter word 1, nonce 00000009 0000004a 00000000
    got = ref.chacha20_blocks(SEED_RAMP, [1 | 0x09000000 << 32], 0x4a000000)[0].tobytes()
    assert got.hex() == RFC_BLOCK
    # many blocks at once equal one at a time, in any order
    ctrs = [5, 0, (1 << 32) - 1, 1 << 32, (1 << 64) - 1]
    many = ref.chacha20_blocks(SEED_RAND, ctrs, STREAM)
    for i, c in enumerate(ctrs):
        assert np.array_equal(many[i], ref.chacha20_blocks(SEED_RAND, [c], STREAM)[0])
    assert len({many[i].tobytes() for i in range(len(ctrs))}) == len(ctrs)


def test_one_pinned_draw():
    assert int.from_bytes(ref.chacha20_blocks(SEED_ZERO, [0])[0].tobytes(), "little") % ref.R == PINNED
    want = ref.limbs([PINNED * ref.RR % ref.R])
    assert np.array_equal(ref.fr_random(SEED_ZERO, 1), want)


def test_per_element_code_on_the_host(tmp_path):
    """csrc/random_elem.h on the host against a schoolbook 512-bit remainder, with -DH2_FU_CHECK asserting the product's limb bounds"""
    exe = str(tmp_path / "test_random_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DH2_FU_CHECK", "-Wall", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_random_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "random host tests ok" in r.stdout, r.stdout + r.stderr


def test_per_element_code_under_asan_ubsan(tmp_path):
    """the same stand-alone program built with -fsanitize=address,undefined, as tests/test_host_cpu.py does for test_fieldu"""
    exe = str(tmp_path / "test_random_host_san")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.check_call(["g++", "-std=c++17", "-DH2_FU_CHECK", "-Wno-unknown-pragmas"] + san +
                          [os.path.join(ROOT, "tests", "cpp", "test_random_host.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "random host tests ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


@pytest.mark.parametrize("n", [0, 1, 5])
def test_host_forms_below_the_threshold_need_no_gpu(h2, n):
    for seed in SEEDS.values():
        for stream, first in ((0, 0), (STREAM, 7), (0, (1 << 32) - 2)):
            got = h2.fr_random(seed, n, first_block=first, stream_id=stream)
            assert got.shape == (n, 4) and np.array_equal(got, ref.fr_random(seed, n, first, stream))
    if n == 1:
        assert np.array_equal(h2.fr_random(SEED_ZERO, 1), ref.limbs([PINNED * ref.RR % ref.R]))


def test_from_bytes_wide_on_the_host(h2):
    data = np.concatenate([ref.crafted_wide(), np.frombuffer(np.random.default_rng(5).bytes(64 * 40), dtype=np.uint8).reshape(-1, 64)])
    assert np.array_equal(h2.fr_from_bytes_wide(data), ref.fr_from_bytes_wide(data))
    assert h2.fr_from_bytes_wide(np.zeros((0, 64), dtype=np.uint8)).shape == (0, 4)
    one = np.zeros((1, 64), dtype=np.uint8)
    one[0, 0] = 1
    assert np.array_equal(h2.fr_from_bytes_wide(one), ref.limbs([ref.RR]))
    with pytest.raises(ValueError):
        h2.fr_from_bytes_wide(np.zeros((2, 32), dtype=np.uint8))


def test_frrng_hands_out_consecutive_blocks(h2):
    rng = h2.FrRng(SEED_RAND, STREAM)
    got = np.concatenate([rng.draw(3), rng.draw(0), rng.draw(1), rng.draw(4)])
    assert rng.block == 8 and np.array_equal(got, ref.fr_random(SEED_RAND, 8, 0, STREAM))
    assert np.array_equal(h2.FrRng(SEED_RAND).draw(2), ref.fr_random(SEED_RAND, 2))
    with pytest.raises(ValueError):
        h2.FrRng(bytes(31))


def test_rejections_answer_einval_with_a_text(h2):
    L = h2.lib()
    seed = (ctypes.c_uint8 * 32)()
    out = np.zeros((3, 4), dtype=np.uint64)
    wide = np.zeros((1, 64), dtype=np.uint8)
    u64, sz = ctypes.c_uint64, ctypes.c_size_t
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    calls = {
        "null seed": lambda: L.h2hip_fr_random_bn254(None, u64(0), u64(0), sz(1), p(out)),
        "null output": lambda: L.h2hip_fr_random_bn254(seed, u64(0), u64(0), sz(1), None),
        "past 2^64": lambda: L.h2hip_fr_random_bn254(seed, u64(0), u64((1 << 64) - 2), sz(3), p(out)),
        "null seed, device": lambda: L.h2hip_fr_random_bn254_device(None, u64(0), u64(0), sz(1), p(out), None),
        "null output, device": lambda: L.h2hip_fr_random_bn254_device(seed, u64(0), u64(0), sz(1), None, None),
        "past 2^64, device": lambda: L.h2hip_fr_random_bn254_device(seed, u64(0), u64((1 << 64) - 2), sz(3), p(out), None),
        "null bytes": lambda: L.h2hip_fr_from_bytes_wide_bn254(None, sz(1), p(out)),
        "null wide output": lambda: L.h2hip_fr_from_bytes_wide_bn254(p(wide), sz(1), None),
        "null bytes, device": lambda: L.h2hip_fr_from_bytes_wide_bn254_device(None, sz(1), p(out), None),
        "null wide output, device": lambda: L.h2hip_fr_from_bytes_wide_bn254_device(p(wide), sz(1), None, None),
    }
    for name, call in calls.items():
        assert call() == ref.H2HIP_EINVAL, name
        text = L.h2hip_last_error().decode()
        assert text and ("null" in text or "2^64" in text), (name, text)
    with pytest.raises(h2.H2HipError, match="2\\^64"):
        h2.fr_random(SEED_ZERO, 3, first_block=(1 << 64) - 2)
    # n == 0 returns 0 and touches nothing, null pointers included; the last legal block is legal
    assert L.h2hip_fr_random_bn254(None, u64(0), u64(0), sz(0), None) == 0
    assert L.h2hip_fr_random_bn254_device(None, u64(0), u64(0), sz(0), None, None) == 0
    assert L.h2hip_fr_from_bytes_wide_bn254(None, sz(0), None) == 0 and L.h2hip_fr_from_bytes_wide_bn254_device(None, sz(0), None, None) == 0
    assert np.array_equal(h2.fr_random(SEED_RAMP, 2, first_block=(1 << 64) - 2), ref.fr_random(SEED_RAMP, 2, (1 << 64) - 2))


def test_interface_is_present(h2):
    L = h2.lib()
    for stem in ("fr_random", "fr_from_bytes_wide"):
        assert hasattr(L, "h2hip_%s_bn254" % stem) and hasattr(L, "h2hip_%s_bn254_device" % stem)
    for name in ("fr_random", "fr_random_device", "fr_from_bytes_wide", "fr_from_bytes_wide_device", "FrRng", "vanishing_commit"):
        assert callable(getattr(h2, name))
    header = open(os.path.join(ROOT, "include", "halo2hip.h")).read()
    assert "as secret as the polynomial" in header.lower() and "deterministic expander" in header


def test_no_gpu_means_loud_failure(h2):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(h2.H2HipError):
        h2.fr_random_device(SEED_ZERO, 4)
    with pytest.raises(h2.H2HipError):
        h2.FrRng(SEED_ZERO).draw_device(4)
    with pytest.raises(h2.H2HipError):  # from the threshold on the host form is the device's work too
        h2.fr_random(SEED_ZERO, 1 << 16)
    buf = np.zeros((64, 4), dtype=np.uint64)  # never dereferenced: the call fails before it reaches a device
    rc = h2.lib().h2hip_fr_from_bytes_wide_bn254_device(buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(1), buf.ctypes.data_as(ctypes.c_void_p), None)
    assert rc not in (0, ref.H2HIP_EINVAL) and h2.lib().h2hip_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------------------- GPU
N_HOST_DEVICE = (1 << 16) + 1   # the host form's device path (the threshold is far below)


@pytest.fixture(scope="module")
def want_big():
    """the reference's draws for the largest n of the parametrised test, per (seed, stream): computed once, sliced by every case"""
    cache = {}

    def get(seed_name, stream):
        key = (seed_name, stream)
        if key not in cache:
            cache[key] = ref.fr_random(SEEDS[seed_name], N_HOST_DEVICE, 0, stream)
            cache[key].setflags(write=False)
        return cache[key]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("stream", [0, STREAM])
@pytest.mark.parametrize("seed_name", sorted(SEEDS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, N_HOST_DEVICE])
def test_device_and_host_forms_match_the_reference(h2, want_big, n, seed_name, stream):
    h2.init(0)
    seed, want = SEEDS[seed_name], want_big(seed_name, stream)[:n]
    d = h2.fr_random_device(seed, n, stream_id=stream)
    assert np.array_equal(h2.to_numpy_u64(d), want)
    assert np.array_equal(h2.fr_random(seed, n, stream_id=stream), want)


@pytest.mark.gpu
@pytest.mark.parametrize("first", [(1 << 32) - 3, (1 << 64) - 8])
def test_counter_carry_and_the_last_legal_range(h2, first):
    """first_block = 2^32 - 3: the carry into state word 13; 2^64 - 8 with n = 8: the last legal range"""
    h2.init(0)
    for seed in (SEED_RAMP, SEED_RAND):
        want = ref.fr_random(seed, 8, first, STREAM)
        assert len({w.tobytes() for w in want}) == 8
        assert np.array_equal(h2.to_numpy_u64(h2.fr_random_device(seed, 8, first_block=first, stream_id=STREAM)), want)
        assert np.array_equal(h2.fr_random(seed, 8, first_block=first, stream_id=STREAM), want)
    with pytest.raises(h2.H2HipError, match="2\\^64"):
        h2.fr_random_device(SEED_RAMP, 9, first_block=(1 << 64) - 8)


@pytest.mark.gpu
def test_split_equality(h2):
    h2.init(0)
    n, m, first = 1000, 333, (1 << 32) - 500
    whole = h2.to_numpy_u64(h2.fr_random_device(SEED_RAND, n, first_block=first))
    a = h2.to_numpy_u64(h2.fr_random_device(SEED_RAND, m, first_block=first))
    b = h2.to_numpy_u64(h2.fr_random_device(SEED_RAND, n - m, first_block=first + m))
    assert np.array_equal(whole, np.concatenate([a, b]))
    assert np.array_equal(whole, ref.fr_random(SEED_RAND, n, first))
    rng = h2.FrRng(SEED_RAND)
    rng.block = first
    assert np.array_equal(np.concatenate([h2.to_numpy_u64(rng.draw_device(m)), rng.draw(7), h2.to_numpy_u64(rng.draw_device(n - m - 7))]), whole)


@pytest.mark.gpu
def test_a_million_elements_sampled(h2):
    h2.init(0)
    n = 1 << 20
    got = h2.to_numpy_u64(h2.fr_random_device(SEED_RAND, n, stream_id=STREAM))
    idx = np.unique(np.concatenate([[0, 1, 255, 256, n - 2, n - 1], np.random.default_rng(11).integers(0, n, 4090)]))[:4096]
    assert np.array_equal(got[idx], ref.fr_random_at(SEED_RAND, idx.tolist(), STREAM))
    assert not np.any(np.all(got[1:] == got[:-1], axis=1))       # no two consecutive elements are equal
    top = got[:, 3]
    assert int(top.max()) <= ref.R >> 192 and int(top.max()) > (ref.R >> 192) * 0.99   # reduced, and spread over the whole range


@pytest.mark.gpu
def test_from_bytes_wide_on_the_device(h2):
    import torch
    h2.init(0)
    data = np.concatenate([ref.crafted_wide(), np.frombuffer(np.random.default_rng(6).bytes(64 << 12), dtype=np.uint8).reshape(-1, 64)])
    n = data.shape[0]
    want = ref.fr_from_bytes_wide(data)
    d_in, d_out = torch.from_numpy(data).cuda(), torch.full((n, 4), -1, dtype=torch.int64, device="cuda")
    h2.fr_from_bytes_wide_device(d_in, d_out, n)
    assert np.array_equal(h2.to_numpy_u64(d_out), want)
    assert np.array_equal(h2.fr_from_bytes_wide(data), want)     # n > the threshold: the host form's device path
    # the generator's own blocks through the second kernel give the generator's elements
    blocks = ref.chacha20_blocks(SEED_RAMP, range(100, 300), STREAM)
    d_blocks, d_el = torch.from_numpy(blocks).cuda(), torch.empty((200, 4), dtype=torch.int64, device="cuda")
    h2.fr_from_bytes_wide_device(d_blocks, d_el, 200)
    assert np.array_equal(h2.to_numpy_u64(d_el), h2.to_numpy_u64(h2.fr_random_device(SEED_RAMP, 200, first_block=100, stream_id=STREAM)))


@pytest.mark.gpu
def test_profile_stages(h2):
    h2.init(0)
    h2.profile_enable(True)
    try:
        h2.profile_reset()
        h2.fr_random_device(SEED_ZERO, 300)
        h2.fr_from_bytes_wide(np.zeros((1 << 12, 64), dtype=np.uint8))
        import torch
        torch.cuda.synchronize()
        for stage in ("fr_random", "fr_from_wide"):
            total_ms, count = h2.profile_get(stage)
            assert count == 1 and total_ms > 0.0, stage
    finally:
        h2.profile_enable(False)


K = 10


@pytest.fixture(scope="module")
def vanishing(h2, oracle):
    """k = 10: pinned params, the reference's draws of blocks [c, c + 2^k] after c = 3 earlier draws, and the oracle's commitment"""
    h2.init(0)
    secret, c, n = 0x1234567 + K, 3, 1 << K
    draws = ref.fr_random(SEED_RAND, c + n + 1, 0, STREAM)
    params = h2.ParamsKZG.setup(K, secret)
    commit = oracle.g1_to_affine(oracle.best_multiexp(draws[c:c + n], params.g, 4))   # KZG commit = best_multiexp over g (commitment.rs:327-334)
    yield {"params": params, "secret": secret, "c": c, "draws": draws, "commit": commit}
    params.close()


@pytest.mark.gpu
def test_vanishing_commit(h2, vanishing):
    v = vanishing
    c, n = v["c"], 1 << K
    rng = h2.FrRng(SEED_RAND, STREAM)
    assert np.array_equal(rng.draw(c), v["draws"][:c])
    d_poly, blind, commitment = h2.vanishing_commit(v["params"], h2.EvaluationDomain.new(3, K), rng)
    assert d_poly.is_cuda and tuple(d_poly.shape) == (n, 4)
    assert np.array_equal(h2.to_numpy_u64(d_poly), v["draws"][c:c + n])
    assert np.array_equal(blind, v["draws"][c + n])              # the blind is block c + 2^k
    assert rng.block == c + n + 1
    assert np.array_equal(h2.g1_to_affine(commitment), v["commit"])
    # the host-side commit of the same coefficients agrees
    assert np.array_equal(h2.g1_to_affine(v["params"].commit(v["draws"][c:c + n])), v["commit"])


@pytest.mark.gpu
def test_cpp_mirror_draws_and_commits(h2, vanishing, tmp_path):
    v = vanishing
    exe = os.path.join(ROOT, "tests", "cpp", "test_random_mirror")
    assert os.path.exists(exe), "tests/cpp/test_random_mirror is not built (halo2-pse_amd/Makefile)"
    path = tmp_path / "vanishing_k10.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<II", K, v["c"]) + SEED_RAND + struct.pack("<Q", STREAM) + h2.fr_from_int(v["secret"]).tobytes())
        f.write(v["draws"].tobytes() + np.ascontiguousarray(v["commit"]).tobytes())
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "random mirror tests ok" in r.stdout, r.stdout + r.stderr
