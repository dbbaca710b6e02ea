#!/usr/bin/env python3
"""Cost of workload tables (lbsim_set_workload_tables), DESIGN.md §3.15.

Two measurements, each one JSON line per result:

--bench PARENT_LIB: the headline bench.py on the parent commit's library (through LBSIM_LIBRARY)
  and on the in-tree build, alternating, --runs each: both medians and the parent's min - max.
  A handle without tables launches the kernels it launched before; their code did not change.

default: the dynamics launch at --shape on handles in one process, legs interleaved:
  a  no tables: the closed form, the handle's usual kernel
  e  no tables, duration_mode="service": a full handle for another reason, so the same kernel the
     table legs run (dynamics_group_full_kernel) with the closed form -- (e) against (a) is the
     price of being a full handle, (b) against (e) that of the lookups
  b  exponential tables for both words: the same law as (a), which isolates the price of the
     feature (the full kernel and the two lookups per arrival)
  c  bounded_pareto(1.5, 1000) work with exponential gaps
  d  hyperexp(2) gaps with exponential work (hyperexp(8)'s largest entry, 170, is above the 64 a
     gap table may hold)
  (c) and (d) also pay the lock-step cost of §3.10: a wave runs as long as its busiest env.
  Per leg: the dynamics launch time from the handle's own profiler and wall-clock env-steps/s,
  median over the rounds.

    python tools/workload_tables_ab.py [--shape 65536x4] [--steps 50] [--warmup 20] [--rounds 7]
    python tools/workload_tables_ab.py --bench marllb_amd/exp/liblbsim_parent.so [--runs 4]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_ab(parent_lib, runs, steps, warmup):
    parent_lib = os.path.abspath(parent_lib)
    vals = {"parent": [], "tree": []}
    for _ in range(runs):
        for which in ("parent", "tree"):
            env = dict(os.environ)
            env.pop("LBSIM_LIBRARY", None)
            if which == "parent":
                env["LBSIM_LIBRARY"] = parent_lib
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                                "--steps", str(steps), "--warmup", str(warmup),
                                "--no-cpu-baseline"],
                               cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"bench.py ({which}) failed:\n{r.stdout[-1000:]}{r.stderr[-2000:]}")
            line = json.loads(r.stdout.strip().splitlines()[-1])
            vals[which].append(float(line["value"]))
            print(json.dumps({"bench": "poisson", "library": which, "value": line["value"],
                              "unit": line.get("unit"), "metric": line.get("metric")}),
                  flush=True)
    p, t = vals["parent"], vals["tree"]
    print(json.dumps({"bench": "poisson", "runs": runs, "parent_median": statistics.median(p),
                      "parent_min_max": [min(p), max(p)], "tree_median": statistics.median(t),
                      "tree_min_max": [min(t), max(t)],
                      "tree_median_inside_parent_spread":
                          min(p) <= statistics.median(t) <= max(p)}), flush=True)


def legs(args):
    import numpy as np
    import torch
    from marllb_amd import VecLoadBalanceEnv, _lib, workload

    lib = _lib.load()
    NC = _lib.PROFILE_CLASSES
    B, S = (int(x) for x in args.shape.split("x"))
    tables = np.stack([workload.exponential_table(), workload.bounded_pareto_table(1.5, 1000.0),
                       workload.hyperexp_table(2.0)])
    pairs = {"b": (0, 0), "c": (0, 1), "d": (2, 0)}  # (gap table, work table)
    envs = {}
    for k in "aebcd":
        extra = {"duration_mode": "service"} if k == "e" else {}
        envs[k] = VecLoadBalanceEnv(B, S, device="cuda:0", seed=args.seed, autoreset=False,
                                    max_steps=10 ** 9, **extra)
        if k in pairs:
            envs[k].set_workload_tables(tables, *pairs[k])
    act = torch.randint(0, 3, (B, S), device="cuda:0")
    for e in envs.values():
        e.reset()
        for _ in range(args.warmup):
            e.step(act)
    torch.cuda.synchronize()
    dyn = {k: [] for k in envs}
    rate = {k: [] for k in envs}
    for _ in range(args.rounds):
        for k, e in envs.items():
            h = e.handle
            h.check(lib.lbsim_profile_begin(h.h, 4 * args.steps + 8))
            t0 = time.perf_counter()
            for _ in range(args.steps):
                e.step(act)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            ms = (ctypes.c_double * NC)()
            cnt = (ctypes.c_int64 * NC)()
            h.check(lib.lbsim_profile_end_ex(h.h, ms, cnt, NC))
            cls = 0 if cnt[0] > 0 else 4  # two launches, or the one-launch step
            dyn[k].append(ms[cls] / cnt[cls] * 1e3)
            rate[k].append(B * args.steps / el)
    names = {k: _lib.launch_names(e.handle).get(0, _lib.launch_names(e.handle).get(4, ""))
             for k, e in envs.items()}
    assert names["b"] == names["c"] == names["d"], "the table legs must run the same kernel"
    print(json.dumps({
        "shape": args.shape, "steps": args.steps, "rounds": args.rounds, "kernels": names,
        "legs": {k: {"dynamics_us_median": round(statistics.median(dyn[k]), 2),
                     "dynamics_us_min_max": [round(min(dyn[k]), 2), round(max(dyn[k]), 2)],
                     "env_steps_per_s_median": round(statistics.median(rate[k]))}
                 for k in envs}}), flush=True)
    for e in envs.values():
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench", metavar="PARENT_LIB", default=None)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--shape", default="65536x4")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    if args.bench:
        bench_ab(args.bench, args.runs, args.steps, args.warmup)
    else:
        legs(args)


if __name__ == "__main__":
    main()
