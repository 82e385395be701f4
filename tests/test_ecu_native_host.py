"""The native table records of csrc/ecu.h on the host (tests/cpp/test_ecu_native.cpp): the record's mixed addition fuzzed against ec.h
with -DH2_FU_CHECK asserting every limb bound, the exceptional cases entry by entry, and the E-form <-> native conversion on edge
values.  A stand-alone program, built plain and with -fsanitize=address,undefined; no GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_ecu_native.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.parametrize("flags", [["-O2"], SAN], ids=["plain", "asan_ubsan"])
def test_native_records_on_the_host(tmp_path, flags):
    exe = str(tmp_path / "test_ecu_native")
    subprocess.check_call(["g++", "-std=c++17", "-DH2_FU_CHECK", "-Wall", "-Wno-unknown-pragmas"] + flags + [SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ecu native tests ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
