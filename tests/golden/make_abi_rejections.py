#!/usr/bin/python3
"""The rejected calls of tests/golden/abi_rejections.json: every candidate of tests/abi_rejections_util.py is made on a build of the
library, and the rows it answers with H2HIP_EINVAL are kept, each with the return code and the full h2hip_last_error() text.  The
rest (a size the wrapper leaves to the engine, say) reaches the engine and answers by the machine it runs on; run this where there is
no GPU, so that such a call ends at the no-device error.

Run: HALO2_HIP_LIB=<the build to record> python tests/golden/make_abi_rejections.py   (writes tests/golden/abi_rejections.json)
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import abi_rejections_util as util


def main():
    lib = os.environ.get("HALO2_HIP_LIB") or os.path.join(os.path.dirname(os.path.dirname(HERE)), "halo2-pse_amd", "libhalo2hip.so")
    L = ctypes.CDLL(lib)
    rows, dropped = [], []
    for row in util.candidate_rows():
        rc, err = util.call(L, row)
        if rc == util.H2HIP_EINVAL:
            rows.append(dict(row, rc=rc, error=err))
        else:
            dropped.append((row["fn"], row["case"], rc))
    path = os.path.join(HERE, "abi_rejections.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    for d in dropped:
        print("not kept (rc %d): %s, %s" % (d[2], d[0], d[1]))
    print("wrote", path, len(rows), "rows of", len(rows) + len(dropped), "from", lib)


if __name__ == "__main__":
    main()
