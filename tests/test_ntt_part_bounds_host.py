"""CPU: the part mode of the NTT's first-pass load (csrc/ntt.hip, ntt_load<true>: coeff_to_extended_part's fused coset scaling) restated
on the host with every limb bound asserted (-DH2_FU_CHECK): the value it hands to the first butterfly round stays inside the bound that
round accepts for the zeta path, and whole tiles from that load equal a plain field.h transform (tests/cpp/test_ntt_part_bounds.cpp).
Built as a stand-alone program under AddressSanitizer and UBSan."""
import os
import subprocess

from conftest import ROOT


def test_ntt_part_load_bounds_host(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "test_ntt_part_bounds.cpp")
    exe = str(tmp_path / "test_ntt_part_bounds")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DH2_FU_CHECK", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-Wno-unknown-pragmas", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ntt part bounds ok" in r.stdout
    assert "runtime error" not in r.stderr
