#!/usr/bin/env python3
"""Record what the reference's C reservoir twin (oracle/_ref/libref_reservoir.so, compiled by
oracle/ref_build.py where the reference tree is present) answers on the inputs of
tests/test_ref_twin.py, into tests/golden/ref_twin.npz.

Only inputs drawn here and the twin's outputs are stored: no reference source.  The test replays
these records where the twin is not built, and where it is built runs it again and also checks
that it still answers what is recorded.  The functions that drive the twin are shared with the
test, so both feed it the same calls.

Usage:  python tests/golden/gen_ref_twin.py     (after __graft_entry__.build() built the twin)
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "libref_reservoir.so")
OUT = os.path.join(HERE, "ref_twin.npz")
K = 128
ALGR_SEEDS = (0, 1, 20260109)
ALGR_ADDS = 3000
INCL_N, INCL_TRIALS = 512, 300
STAT_NOW_MS = 50_000


def load_twin(path=LIB):
    lib = ctypes.CDLL(path)
    lib.ref_reservoir_sizeof.restype = ctypes.c_size_t
    lib.ref_reservoir_init.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    lib.ref_reservoir_add.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_uint64]
    lib.ref_reservoir_add.restype = ctypes.c_int
    lib.ref_reservoir_count.argtypes = [ctypes.c_void_p]
    lib.ref_reservoir_count.restype = ctypes.c_uint64
    lib.ref_reservoir_values.argtypes = [ctypes.c_void_p]
    lib.ref_reservoir_values.restype = ctypes.POINTER(ctypes.c_float)
    lib.ref_reservoir_stats.argtypes = [ctypes.c_void_p, ctypes.c_float, ctypes.c_uint64,
                                        ctypes.c_void_p]
    return lib


def new_reservoir(lib, seed):
    buf = ctypes.create_string_buffer(lib.ref_reservoir_sizeof())
    lib.ref_reservoir_init(buf, seed)
    return buf


def algr_values(seed):
    return np.random.default_rng(seed).uniform(0.0, 100.0, ALGR_ADDS).astype(np.float32)


def stat_cases(rng):
    cases = []
    for n in (1, 5, 17, 64, 100, 128):
        for kind in range(3):
            if kind == 0:
                v = (rng.exponential(8e3, n).astype(np.int64) + 1).astype(np.float32) * np.float32(1e-6)
            elif kind == 1:
                v = rng.uniform(1.0, 50.0, n).astype(np.float32)
            else:
                v = rng.choice(np.float32([0.5, 1.0, 2.0, 4.0]), n)
            age_ms = rng.integers(0, 20000, n)
            cases.append((v.astype(np.float32), age_ms))
    return cases


def run_algr(lib, seed, vals):
    """Add vals[i] at timestamp i: (accepted flag, count after the add) per add, final values."""
    r = new_reservoir(lib, seed)
    accepted = np.zeros(len(vals), np.uint8)
    count = np.zeros(len(vals), np.uint64)
    for i, v in enumerate(vals):
        accepted[i] = bool(lib.ref_reservoir_add(r, float(v), i))
        count[i] = lib.ref_reservoir_count(r)
    final = np.ctypeslib.as_array(lib.ref_reservoir_values(r), shape=(K,)).copy()
    return accepted, count, final


def run_inclusion(lib):
    """How often each of INCL_N items (value = its index) ends in the reservoir over the trials."""
    hits = np.zeros(INCL_N)
    for t in range(INCL_TRIALS):
        r = new_reservoir(lib, 1000 + t)
        for i in range(INCL_N):
            lib.ref_reservoir_add(r, float(i), i)
        vals = np.ctypeslib.as_array(lib.ref_reservoir_values(r), shape=(K,)).astype(int)
        hits[vals] += 1
    return hits


def run_stats(lib, v, age_ms):
    """The twin's five statistics (mean, p90, std, mean_decay, p90_decay) of one case."""
    r = new_reservoir(lib, 3)
    ts_ms = (STAT_NOW_MS - age_ms).astype(np.uint32)
    for i in range(len(v)):
        lib.ref_reservoir_add(r, float(v[i]), int(ts_ms[i]) * 1000)  # us timestamps
    out = np.zeros(5, np.float32)
    lib.ref_reservoir_stats(r, 0.9, STAT_NOW_MS * 1000, out.ctypes.data)
    return out


def main():
    lib = load_twin()
    rec = {}
    for seed in ALGR_SEEDS:
        vals = algr_values(seed)
        acc, cnt, fin = run_algr(lib, seed, vals)
        rec[f"algr_vals_{seed}"], rec[f"algr_accepted_{seed}"] = vals, acc
        rec[f"algr_count_{seed}"], rec[f"algr_final_{seed}"] = cnt, fin
    rec["incl_hits"] = run_inclusion(lib)
    cases = stat_cases(np.random.default_rng(7))
    rec["stat_cases"] = np.array(len(cases))
    for i, (v, age) in enumerate(cases):
        rec[f"stat_v_{i}"], rec[f"stat_age_{i}"] = v, age.astype(np.int64)
        rec[f"stat_out_{i}"] = run_stats(lib, v, age)
    np.savez_compressed(OUT, **rec)
    print(f"{OUT}: {len(rec)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
