"""CPU: what the C ABI rejects before the engine is entered, call by call -- return code and the whole h2hip_last_error() text -- for
the NTT / domain family, divide_by_vanishing_poly and the entry points that live in their stage files (g_to_lagrange, fft_g1,
kzg_setup, evaluate_h, gen_*, set_msm_window).  The table was recorded from the library as it was before these entry points were
regrouped (tests/golden/make_abi_rejections.py); such calls answer the same with or without a GPU.  HALO2_HIP_LIB points the test at
another build of the library."""
import ctypes
import json
import os

import abi_rejections_util as util
from conftest import ROOT


def test_rejected_calls_answer_as_recorded(h2):
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_rejections.json")))
    L = ctypes.CDLL(h2.LIB_PATH)  # a handle of its own: no argtypes but the ones a row states
    wrong = []
    for row in rows:
        assert row["rc"] == util.H2HIP_EINVAL
        got = util.call(L, row)
        if got != (row["rc"], row["error"]):
            wrong.append("%s, %s: got %r, recorded %r" % (row["fn"], row["case"], got, (row["rc"], row["error"])))
    assert not wrong, "\n".join(wrong)
    # every entry point of the table is rejected at least once, and every row of the fixture is a row the table still describes
    assert {r["fn"] for r in rows} == set(util.ENTRY_POINTS) | {"h2hip_set_msm_window"}
    described = [(r["fn"], r["case"], r["args"]) for r in util.candidate_rows()]
    assert all((r["fn"], r["case"], r["args"]) in described for r in rows)
