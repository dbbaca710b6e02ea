#!/usr/bin/env python3
"""Cost of scripted server availability (lbsim_set_server_avail), one process, legs interleaved.

Two measurements, each one JSON line per result:

--bench PARENT_LIB: the headline bench.py on the parent commit's library (through LBSIM_LIBRARY)
  and on the in-tree build, alternating, --runs each: a default handle must not pay (this tree's
  median inside the parent's own spread).

The legs (default), per shape:
  a  a default handle (the feature off)
  b  server_availability=True with an all-up table of P = 24 phases: identical observations and
     rewards (asserted), so the difference to (a) is the extra launch in front of the step -- and,
     at the small shape, the one-wave step kernel that an enabled handle gives up
  c  server_availability=True with marllb_amd.randomize.sample_cluster_sizes (min_servers = 1):
     absent servers take no flows, so the work itself changes (a finding, not a cost)
Per leg: the step's own launches from the handle's profiler (the launch in front is not among its
classes) and wall-clock us per step, median over the rounds.

    python tools/server_avail_ab.py [--shapes 65536x4,65536x8,4096x4] [--steps 50] [--rounds 7]
    python tools/server_avail_ab.py --bench marllb_amd/exp/liblbsim_parent.so [--runs 4]
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
    from marllb_amd.randomize import sample_cluster_sizes

    lib = _lib.load()
    NC = _lib.PROFILE_CLASSES
    P, H = args.phases, args.steps_per_phase
    for shape in args.shapes.split(","):
        B, S = (int(x) for x in shape.split("x"))
        envs = {k: VecLoadBalanceEnv(B, S, device="cuda:0", seed=args.seed, autoreset=False,
                                     max_steps=10 ** 9, server_availability=k != "a")
                for k in "abc"}
        envs["b"].set_server_availability(torch.ones((P, S), dtype=torch.uint8), steps_per_phase=H)
        envs["c"].set_cluster_sizes(sample_cluster_sizes(B, S, 1, seed=args.seed))
        act = torch.randint(0, 3, (B, S), device="cuda:0")
        last = {}
        for k, e in envs.items():
            e.reset()
            for _ in range(args.warmup):
                last[k] = e.step(act)
        torch.cuda.synchronize()
        own = {k: [] for k in envs}
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
                own[k].append(sum(ms[c] for c in (0, 1, 4)) / args.steps * 1e3)
                wall[k].append(el / args.steps * 1e6)
        assert torch.equal(last["a"][0], last["b"][0]) and torch.equal(last["a"][1], last["b"][1]), \
            "leg b must compute leg a's observations and rewards"
        print(json.dumps({
            "shape": shape, "steps": args.steps, "rounds": args.rounds, "phases": P,
            "steps_per_phase": H,
            "kernels": {k: _lib.launch_names(e.handle) for k, e in envs.items()},
            "servers_up_c": float(envs["c"].servers_up().float().mean()),
            "legs": {k: {"step_kernels_us_median": round(statistics.median(own[k]), 2),
                         "wall_us_per_step_median": round(statistics.median(wall[k]), 2),
                         "wall_us_per_step_min_max": [round(min(wall[k]), 2),
                                                      round(max(wall[k]), 2)]}
                     for k in envs}}), flush=True)
        for e in envs.values():
            e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench", metavar="PARENT_LIB", default=None)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--shapes", default="65536x4,65536x8,4096x4")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--phases", type=int, default=24)
    ap.add_argument("--steps-per-phase", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    if args.bench:
        bench_ab(args.bench, args.runs, args.steps, args.warmup)
    else:
        legs(args)


if __name__ == "__main__":
    main()
