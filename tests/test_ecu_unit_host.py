"""The unit form of the mixed addition of csrc/ecu.h on the host (tests/cpp/test_ecu_unit.cpp): the addition onto an accumulator that is
a bucket's first record, fuzzed against ec.h and against the general form with -DH2_FU_CHECK asserting every limb bound; every
exceptional pairing on the second record (P + P, P + (-P), an identity record first or second); the bounds at coordinates 0, 1 and
p - 1; the state word the accumulate loops carry.  A stand-alone program, built plain and with -fsanitize=address,undefined; no GPU,
nothing loaded into Python."""
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_ecu_unit.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.parametrize("flags,divide", [(["-O2"], 2), (SAN, 10)], ids=["plain", "asan_ubsan"])
def test_unit_second_addition_on_the_host(tmp_path, flags, divide):
    """the plain build runs half of the random pairs and chains and the sanitised build a tenth; every exceptional case runs in both"""
    exe = str(tmp_path / "test_ecu_unit")
    subprocess.check_call(["g++", "-std=c++17", "-DH2_FU_CHECK", "-Wall", "-Wno-unknown-pragmas"] + flags + [SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(divide)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ecu unit tests ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
