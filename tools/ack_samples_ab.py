#!/usr/bin/env python3
"""Cost of duration samples at every data ACK (lbsim_ack_samples_enable), one
process, legs interleaved.

Two measurements, each one JSON line per result:

--bench PARENT_LIB: the headline bench.py on the parent commit's library (through LBSIM_LIBRARY)
  and on the in-tree build, alternating, --runs each: a default handle must not pay (this tree's
  median inside the parent's own spread).

The legs (default), the dynamics launch of a step at --envs x --servers:
  a  a default handle (the plain kernels)
  b  a full FIFO handle (flow_stats=True: dynamics_group_full_kernel)
  c  ack_samples=True, max_acks=1   (dynamics_group_ack_kernel; one sample per flow)
  d  ack_samples=True, max_acks=8   (the default)
  e  ack_samples=True, max_acks=32
Per leg: the dynamics launch and the observe launch from the handle's profiler (classes 0 and 1)
and wall-clock us per step, median over the rounds, and the mean of observation column 0 (the
queues the launch walked).

    python tools/ack_samples_ab.py [--envs 65536] [--servers 4] [--steps 50] [--rounds 7]
    python tools/ack_samples_ab.py --bench marllb_amd/exp/liblbsim_parent.so [--runs 4]
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
            print(json.dumps({"bench": "headline", "library": which, "value": line["value"],
                              "unit": line.get("unit"), "metric": line.get("metric")}),
                  flush=True)
    p, t = vals["parent"], vals["tree"]
    print(json.dumps({"bench": "headline", "runs": runs, "parent_median": statistics.median(p),
                      "parent_min_max": [min(p), max(p)], "tree_median": statistics.median(t),
                      "tree_min_max": [min(t), max(t)],
                      "tree_median_inside_parent_spread":
                          min(p) <= statistics.median(t) <= max(p)}), flush=True)


def legs(args):
    import torch
    from marllb_amd import VecLoadBalanceEnv, _lib

    lib = _lib.load()
    NC = _lib.PROFILE_CLASSES
    B, S = args.envs, args.servers
    base = dict(device="cuda:0", seed=args.seed, autoreset=False, max_steps=10 ** 9)
    envs = {"a": VecLoadBalanceEnv(B, S, **base),
            "b": VecLoadBalanceEnv(B, S, flow_stats=True, **base),
            "c": VecLoadBalanceEnv(B, S, ack_samples=True, max_acks=1, **base),
            "d": VecLoadBalanceEnv(B, S, ack_samples=True, max_acks=8, **base),
            "e": VecLoadBalanceEnv(B, S, ack_samples=True, max_acks=32, **base)}
    act = torch.randint(0, 3, (B, S), device="cuda:0")
    last = {}
    for k, e in envs.items():
        e.reset()
        for _ in range(args.warmup):
            last[k] = e.step(act)
    torch.cuda.synchronize()
    dyn = {k: [] for k in envs}
    obs = {k: [] for k in envs}
    wall = {k: [] for k in envs}
    for _ in range(args.rounds):
        for k, e in envs.items():
            h = e.handle
            h.check(lib.lbsim_profile_begin(h.h, 4 * args.steps + 8))
            t0 = time.perf_counter()
            for _ in range(args.steps):
                last[k] = e.step(act)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            ms = (ctypes.c_double * NC)()
            cnt = (ctypes.c_int64 * NC)()
            h.check(lib.lbsim_profile_end_ex(h.h, ms, cnt, NC))
            dyn[k].append(ms[0] / args.steps * 1e3)
            obs[k].append(ms[1] / args.steps * 1e3)
            wall[k].append(el / args.steps * 1e6)
    print(json.dumps({
        "envs": B, "servers": S, "steps": args.steps, "rounds": args.rounds,
        "kernels": {k: _lib.launch_names(e.handle) for k, e in envs.items()},
        "mean_obs_column0": {k: float(last[k][0][:, :, 0].mean()) for k in envs},
        "legs": {k: {"dynamics_us_median": round(statistics.median(dyn[k]), 2),
                     "dynamics_us_min_max": [round(min(dyn[k]), 2), round(max(dyn[k]), 2)],
                     "observe_us_median": round(statistics.median(obs[k]), 2),
                     "wall_us_per_step_median": round(statistics.median(wall[k]), 2)}
                 for k in envs}}), flush=True)
    for e in envs.values():
        e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench", metavar="PARENT_LIB", default=None)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--servers", type=int, default=4)
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
