#!/usr/bin/python3
"""Write tests/golden/kzg_6_params.processed: the k = 6 SRS of kzg_6_params.rawbytes in SerdeFormat::Processed
(ParamsKZG::write_custom, poly/kzg/commitment.rs:142-157: k u32 LE | g | g_lagrange as 32-B compressed points | g2 | s_g2 as 64-B
compressed points), derived with Python integers (tests/serde_util.py) from the committed raw file.
    python3 tests/golden/make_serde_golden.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import serde_util  # noqa: E402


def main():
    raw = open(os.path.join(HERE, "kzg_6_params.rawbytes"), "rb").read()
    proc = serde_util.params_raw_to_processed(raw)
    assert serde_util.params_processed_to_raw(proc) == raw
    path = os.path.join(HERE, "kzg_6_params.processed")
    with open(path, "wb") as f:
        f.write(proc)
    print("wrote", path, len(proc), "bytes")


if __name__ == "__main__":
    main()
