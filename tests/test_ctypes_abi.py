"""The Python binding states every C entry point's prototype once, in halo2-pse_amd/_abi.py, which tools/gen_ctypes_abi.py translates from
include/halo2hip.h and include/halo2hip_debug.h and lib() applies to the loaded library:
  * the committed table is the translation of the headers, name for name and with the headers' arity;
  * lib() binds every exported name to its row;
  * ctypes then rejects a wrong argument count or a ctypes instance of the wrong width before C is reached, and carries a plain Python
    int at the declared width, in and out -- on the host (the stream ladder, the window widths) and, marked gpu, a device pointer and a
    stream handle."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_ctypes_abi  # noqa: E402
import gen_rust_extern  # noqa: E402


def _declared():
    """name -> parameter list, of both headers"""
    return {name: args for h in gen_ctypes_abi.HEADERS for _, name, args in gen_rust_extern.prototypes(h)}


def test_abi_table_is_the_translation_of_the_headers(h2):
    assert open(os.path.join(ROOT, "halo2-pse_amd", "_abi.py")).read() == gen_ctypes_abi.render()
    table, declared = sys.modules["halo2_pse_amd._abi"].PROTOTYPES, _declared()
    # the same names as tests/test_abi.py reads from the headers with a regex of its own
    names = set()
    for h in gen_ctypes_abi.HEADERS:
        names |= set(re.findall(r"^(?:int|void|size_t|uint32_t|uint64_t|const char\s*\*)\s+\*?\s*(h2hip_[a-z0-9_]+)\s*\(",
                                open(os.path.join(ROOT, "include", h)).read(), flags=re.M))
    assert set(table) == set(declared) == names and len(table) == 179
    for name, (restype, argtypes) in table.items():
        assert len(argtypes) == len(declared[name]), name
    assert table["h2hip_debug_set_msm_stream"] == (ctypes.c_int, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t])
    assert table["h2hip_last_error"] == (ctypes.c_char_p, []) and table["h2hip_shutdown"] == (None, [])
    assert table["h2hip_msm_bn254"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p])


def test_lib_binds_every_exported_name_to_its_row(h2):
    L, table = h2.lib(), sys.modules["halo2_pse_amd._abi"].PROTOTYPES
    for name, (restype, argtypes) in table.items():
        fn = getattr(L, name)  # tests/test_abi.py: the in-tree build exports every declared name
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_arity_and_width_are_enforced_before_c_is_reached(h2):
    L = h2.lib()
    with pytest.raises(TypeError):
        L.h2hip_get_msm_window()
    out = ctypes.c_size_t()
    with pytest.raises(TypeError):
        L.h2hip_evaluate_h_workspace_bytes(4, 6, 1, 1, 1, 1, 1, 1, 0, 0, ctypes.byref(out), 0)
    with pytest.raises(ctypes.ArgumentError):
        L.h2hip_debug_set_msm_stream(0, 0, ctypes.c_uint32(1))  # min_n is a size_t


def test_64_bits_arrive_and_come_back_without_a_cast(h2):
    L = h2.lib()
    n = (1 << 33) + 12345
    sizes = (ctypes.c_size_t * 32)()
    count = L.h2hip_debug_msm_stream_ladder(n, 0, 0, 0, sizes, 32)
    assert 1 <= count <= 32 and sum(sizes[:count]) == n
    assert L.h2hip_get_msm_window(1 << 33) == L.h2hip_get_msm_window(ctypes.c_size_t(1 << 33))
    assert L.h2hip_get_msm_window(1 << 33) != L.h2hip_get_msm_window(0)  # 2^33 did not arrive as its low 32 bits


@pytest.mark.gpu
def test_gpu_device_pointer_and_stream_pass_as_bare_ints(h2, oracle):
    import torch
    h2.init()
    L = h2.lib()
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert isinstance(t.data_ptr(), int) and isinstance(stream, int)
    src = np.arange(1, 65, dtype=np.uint8)
    back = np.zeros(64, dtype=np.uint8)
    assert L.h2hip_memcpy_h2d(t.data_ptr(), h2._p(src), 64, stream) == 0, L.h2hip_last_error()
    assert L.h2hip_stream_synchronize(stream) == 0, L.h2hip_last_error()
    assert L.h2hip_memcpy_d2h(h2._p(back), t.data_ptr(), 64, stream) == 0, L.h2hip_last_error()
    assert L.h2hip_stream_synchronize(stream) == 0, L.h2hip_last_error()
    assert np.array_equal(back, src)
    # one wrapper end to end: a 2^4 transform on a device tensor
    k = 4
    d, _ = oracle.domain_new(2, k)
    a = oracle.gen_scalars(0x5EED0003, 1 << k, num_threads=1)
    da = torch.from_numpy(a.copy()).cuda()
    h2.ntt_device(da, d.fe("omega"), k)
    torch.cuda.synchronize()
    assert np.array_equal(h2.to_numpy_u64(da), oracle.best_fft(a, d.fe("omega"), k, 1))
