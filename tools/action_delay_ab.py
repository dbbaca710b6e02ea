#!/usr/bin/env python3
"""Cost of action latency (lbsim_set_action_delay), one process, legs interleaved.

Two measurements, each one JSON line per result:

--bench PARENT_LIB: the headline bench.py on the parent commit's library (through LBSIM_LIBRARY)
  and on the in-tree build, alternating, --runs each: a default handle must not pay (this tree's
  median inside the parent's own spread).

--full-ab PARENT_LIB: leg (b) below, a full handle that does not enable the feature, on the
  parent's library and on the in-tree build, alternating child processes, --runs each: the other
  full handles must not pay either (this tree's median inside the parent's own spread).

The legs (default), per shape, the dynamics launch of a step:
  a  a default handle (the plain kernels)
  b  a full handle for another reason (duration_mode="service"): dynamics_group_full_kernel
  c  action_delay=True with every delay 0: (a)'s observations and rewards (asserted); against
     (b) the price of the prologue's reads, the ring store and the loop's test
  d  action_delay=True with marllb_amd.randomize.sample_action_delay over (0, dt): every env
     switches rows once inside the step; against (c) the price of the switch (and of routing on
     older weights: a slightly different workload)
The action batch changes every step (a fixed batch would make every row equal).
Per leg: the dynamics launch from the handle's profiler (class 0) and wall-clock us per step,
median over the rounds.

    python tools/action_delay_ab.py [--shapes 65536x4,65536x8] [--steps 50] [--rounds 7]
    python tools/action_delay_ab.py --bench marllb_amd/exp/liblbsim_parent.so [--runs 4]
    python tools/action_delay_ab.py --full-ab marllb_amd/exp/liblbsim_parent.so [--runs 4]
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


def full_ab(parent_lib, args):
    parent_lib = os.path.abspath(parent_lib)
    vals = {}
    for _ in range(args.runs):
        for which in ("parent", "tree"):
            env = dict(os.environ)
            env.pop("LBSIM_LIBRARY", None)
            if which == "parent":
                env["LBSIM_LIBRARY"] = parent_lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-legs", "b",
                                "--shapes", args.shapes, "--steps", str(args.steps), "--rounds",
                                str(args.rounds), "--warmup", str(args.warmup)],
                               cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"leg b ({which}) failed:\n{r.stdout[-1000:]}{r.stderr[-2000:]}")
            for line in r.stdout.strip().splitlines():
                d = json.loads(line)
                us = d["legs"]["b"]["dynamics_us_median"]
                vals.setdefault(d["shape"], {"parent": [], "tree": []})[which].append(us)
                print(json.dumps({"full_ab": d["shape"], "library": which, "leg_b_dynamics_us": us,
                                  "kernel": d["kernels"]["b"].get("0")}), flush=True)
    for shape, v in vals.items():
        p, t = v["parent"], v["tree"]
        print(json.dumps({"full_ab": shape, "runs": args.runs,
                          "parent_median": statistics.median(p), "parent_min_max": [min(p), max(p)],
                          "tree_median": statistics.median(t), "tree_min_max": [min(t), max(t)],
                          "tree_median_inside_parent_spread":
                              min(p) <= statistics.median(t) <= max(p)}), flush=True)


def legs(args):
    import torch
    from marllb_amd import VecLoadBalanceEnv, _lib
    from marllb_amd.randomize import sample_action_delay

    lib = _lib.load()
    NC = _lib.PROFILE_CLASSES
    for shape in args.shapes.split(","):
        B, S = (int(x) for x in shape.split("x"))
        extra = {"a": {}, "b": {"duration_mode": "service"}, "c": {"action_delay": True},
                 "d": {"action_delay": True}}
        envs = {k: VecLoadBalanceEnv(B, S, device="cuda:0", seed=args.seed, autoreset=False,
                                     max_steps=10 ** 9, **kw) for k, kw in extra.items()
                if k in args.only_legs}
        dt = float(next(iter(envs.values())).cfg.step_interval)
        delays = sample_action_delay(B, 0.0, dt, seed=args.seed)
        if "c" in envs:
            envs["c"].set_action_delay(0.0)
        if "d" in envs:
            envs["d"].set_action_delay(delays)
        g = torch.Generator(device="cuda:0").manual_seed(args.seed)
        acts = [torch.randint(0, 3, (B, S), device="cuda:0", generator=g) for _ in range(8)]
        last = {}
        for k, e in envs.items():
            e.reset()
            for i in range(args.warmup):
                last[k] = e.step(acts[i % 8])
        torch.cuda.synchronize()
        dyn = {k: [] for k in envs}
        wall = {k: [] for k in envs}
        for _ in range(args.rounds):
            for k, e in envs.items():
                h = e.handle
                h.check(lib.lbsim_profile_begin(h.h, 4 * args.steps + 8))
                t0 = time.perf_counter()
                for i in range(args.steps):
                    last[k] = e.step(acts[i % 8])
                torch.cuda.synchronize()
                el = time.perf_counter() - t0
                ms = (ctypes.c_double * NC)()
                cnt = (ctypes.c_int64 * NC)()
                h.check(lib.lbsim_profile_end_ex(h.h, ms, cnt, NC))
                dyn[k].append(ms[0] / args.steps * 1e3)
                wall[k].append(el / args.steps * 1e6)
        if "a" in envs and "c" in envs:
            assert torch.equal(last["a"][0], last["c"][0]) and \
                torch.equal(last["a"][1], last["c"][1]), \
                "leg c must compute leg a's observations and rewards"
        print(json.dumps({
            "shape": shape, "steps": args.steps, "rounds": args.rounds,
            "kernels": {k: _lib.launch_names(e.handle) for k, e in envs.items()},
            "mean_delay_s_d": float(delays.double().mean()),
            "mean_obs_column0": {k: float(last[k][0][:, :, 0].mean()) for k in envs},
            "legs": {k: {"dynamics_us_median": round(statistics.median(dyn[k]), 2),
                         "dynamics_us_min_max": [round(min(dyn[k]), 2), round(max(dyn[k]), 2)],
                         "wall_us_per_step_median": round(statistics.median(wall[k]), 2)}
                     for k in envs}}), flush=True)
        for e in envs.values():
            e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench", metavar="PARENT_LIB", default=None)
    ap.add_argument("--full-ab", metavar="PARENT_LIB", default=None)
    ap.add_argument("--only-legs", default="abcd", help="the legs to run (full-ab's children: b)")
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--shapes", default="65536x4,65536x8")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    if args.bench:
        bench_ab(args.bench, args.runs, args.steps, args.warmup)
    elif args.full_ab:
        full_ab(args.full_ab, args)
    else:
        legs(args)


if __name__ == "__main__":
    main()
