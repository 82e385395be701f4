"""The setter hooks (include/halo2hip_debug.h, plus h2hip_set_msm_window) need no GPU and leave an engine that is not running alone:
in a fresh process every one of them, called with the arguments that restore its default, returns 0, what the no-GPU queries report
is what it was before, and h2hip_num_devices() is still 0.  The list of hooks is read from the header, so a new hook without a row
in DEFAULTS fails here.  Also pinned: the three defaults the header states because a caller has to pass them to get them back."""
import json
import os
import re
import subprocess
import sys

from conftest import ROOT

# hook -> the arguments that restore its default: 0 where the hook takes 0 for that, else the default itself (the on / off switches
# are on by default; ntt_smax, ntt_twiddle_budget and evalh_max_local_slots have no reset value and take their default as stated in
# the header)
DEFAULTS = {
    "h2hip_set_msm_window": [0],
    "h2hip_debug_set_msm_stream": [0, 0, 0],
    "h2hip_debug_set_msm_max_chunk": [0],
    "h2hip_debug_set_table_records": [0],
    "h2hip_debug_set_msm_heavy_div": [0],
    "h2hip_debug_set_g2l_quad": [1],
    "h2hip_debug_set_msm_fuse_limits": [0, 0],
    "h2hip_debug_set_msm_rowcol": [0],
    "h2hip_debug_set_msm_split_buckets": [1],
    "h2hip_debug_set_msm_plane_tail": [1],
    "h2hip_debug_set_msm_quad_tail": [1],
    "h2hip_debug_set_msm_split_records": [1],
    "h2hip_debug_set_msm_bin_entries": [0],
    "h2hip_debug_set_msm_fuse_small": [1],
    "h2hip_debug_set_ntt_smax": [8],
    "h2hip_debug_set_lazy_pin": [0],
    "h2hip_debug_set_ntt_two_pass": [0, 0],
    "h2hip_debug_set_ntt_twiddle_budget": [4 << 30],
    "h2hip_debug_set_ntt_batch_bytes": [0],
    "h2hip_debug_set_ntt_two_pass_batch_wgs": [0],
    "h2hip_debug_set_ntt_full_max_log_m": [0],
    "h2hip_debug_set_ntt_fold_tables": [1],
    "h2hip_debug_set_ntt_host_batch": [0, 0],
    "h2hip_debug_set_ntt_two_pass_log_j": [-1],
    "h2hip_debug_set_evalh_max_local_slots": [256],
    "h2hip_debug_set_evalh_lookup_group_bytes": [0],
    "h2hip_debug_set_evalh_codegen": [1, 0],
    "h2hip_debug_set_opening_tile": [0, 0],
    "h2hip_debug_set_lookup_sort": [0],
    "h2hip_debug_set_keygen_group": [0],
    "h2hip_debug_set_random_min_n": [0],
}

CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
from __graft_entry__ import load_pkg
calls = json.loads(sys.argv[2])
L = load_pkg().lib()
CT = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "int": ctypes.c_int}

def observe():
    out = {}
    for log_n in (12, 17, 18, 19, 22, 23, 26):
        for count in (1, 16):
            r = (ctypes.c_uint32 * 4)()
            p = L.h2hip_debug_ntt_plan(ctypes.c_uint32(log_n), ctypes.c_size_t(count), r)
            out["plan %d x %d" % (count, log_n)] = list(r[:p])
    for n in ((1 << 20) - 1, 1 << 20):
        sz = (ctypes.c_size_t * 16)()
        k = L.h2hip_debug_msm_stream_ladder(ctypes.c_size_t(n), ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_int(0), sz, ctypes.c_size_t(16))
        out["ladder %d" % n] = list(sz[:k])
    for lg in (10, 16, 20, 24):
        out["window 2^%d" % lg] = [L.h2hip_get_msm_window(ctypes.c_size_t(1 << lg)), L.h2hip_get_msm_window_fixed_base(ctypes.c_size_t(1 << lg))]
    return out

before = observe()
rcs = {name: getattr(L, name)(*[CT[t](v) for t, v in args]) for name, args in calls}
print(json.dumps({"rcs": rcs, "before": before, "after": observe(), "devices": L.h2hip_num_devices()}))
"""


def _setters():
    """name -> parameter types, from the prototypes of the two headers"""
    found = {}
    for header, pattern in (("halo2hip_debug.h", r"^int (h2hip_debug_set_\w+)\(([^)]*)\);"), ("halo2hip.h", r"^int (h2hip_set_msm_window)\(([^)]*)\);")):
        text = open(os.path.join(ROOT, "include", header)).read()
        for name, params in re.findall(pattern, text, flags=re.M):
            found[name] = [p.strip().rsplit(" ", 1)[0] for p in params.split(",")]
    return found


def test_every_setter_restores_its_default_without_starting_the_engine():
    setters = _setters()
    assert len(setters) >= 30 and "h2hip_set_msm_window" in setters, sorted(setters)
    assert sorted(setters) == sorted(DEFAULTS), "a setter hook without a row in DEFAULTS (or a row without a hook)"
    calls = []
    for name, types in setters.items():
        assert len(types) == len(DEFAULTS[name]), name
        calls.append((name, list(zip(types, DEFAULTS[name]))))
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, json.dumps(calls)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["rcs"] == {name: 0 for name in setters}
    assert got["after"] == got["before"]
    assert got["before"]["plan 1 x 26"] == [9, 9, 8] and got["before"]["plan 1 x 23"] == [8, 8, 7]  # ntt_smax: 8, and 9 beyond 2^24
    assert got["devices"] == 0


def test_defaults_the_header_states_are_the_structs():
    """halo2hip_debug.h names three defaults -- those a caller passes to get them back -- and struct Tuning holds them"""
    header = open(os.path.join(ROOT, "include", "halo2hip_debug.h")).read()
    engine = open(os.path.join(ROOT, "halo2-pse_amd", "csrc", "engine.h")).read()
    for said, member in (("the default is 8,", "uint32_t ntt_smax = 8;"), ("the default is 4 GB", "uint64_t ntt_full_budget = (uint64_t)4 << 30;"),
                         ("the default is 256", "uint32_t evalh_max_local_slots = 256;")):
        assert said in header and member in engine, (said, member)
