#!/usr/bin/env python3
"""Record what marllb_amd.trace.load_csv makes of the reference's rate_500 trace CSV (3.4 MB, too
large to keep here) into tests/golden/trace_rate_500.json: the row count, the rate and the SHA-256
of the gap_us (uint32) and work (float32) arrays' bytes.  tests/test_trace.py holds the built-in
npz (data/traces/, converted by tools/convert_trace.py) against these.

Usage:  python tests/golden/gen_trace.py --reference <reference root>
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
CSV = "data/trace/poisson_for_loop/rate_500.csv"
OUT = os.path.join(HERE, "trace_rate_500.json")


def digest(a: np.ndarray, dtype) -> str:
    a = np.ascontiguousarray(a)
    assert a.dtype == dtype and a.ndim == 1
    return hashlib.sha256(a.astype(a.dtype.newbyteorder("<")).tobytes()).hexdigest()


def record(t) -> dict:
    return {"rows": t.rows, "rate": t.rate, "gap_us_sha256": digest(t.gap_us, np.uint32),
            "work_sha256": digest(t.work, np.float32)}


def main():
    from marllb_amd import trace
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    rec = dict(record(trace.load_csv(os.path.join(ap.parse_args().reference, CSV))), csv=CSV)
    with open(OUT, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(OUT, rec)


if __name__ == "__main__":
    main()
