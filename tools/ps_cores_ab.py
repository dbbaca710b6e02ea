#!/usr/bin/env python3
"""Cost of per-server cores on processor-sharing handles (lbsim_set_ps_cores).

Two measurements, each one JSON line per result:

--bench PARENT_LIB: the headline bench.py on the parent commit's library (through LBSIM_LIBRARY)
  and on the in-tree build, alternating, --runs each: a default handle must not pay (this tree's
  median inside the parent's own spread).

--legs PARENT_LIB: the dynamics launch of a step at --envs x --servers on four legs, every one a
  handle with service_discipline="ps":
  a  the parent commit's library
  b  this tree, cores never set
  c  this tree, every count 1 (set_ps_cores(ones))
  d  this tree, counts drawn by sample_server_workers(choices=(1, 2, 4), keep_capacity=True) with
     the rate of one core set beside them: another workload (the flows of a c-core server run c
     at a time at rate mu / c each), so (d) mixes the workload's cost with the rule's
  One child process per (round, leg) -- a library is loaded once per process -- interleaved over
  --rounds rounds.  Per leg: the dynamics launch from the handle's profiler (class 0) and wall
  clock us per step, median over the rounds, and the mean of observation column 0.

    python tools/ps_cores_ab.py --legs marllb_amd/exp/liblbsim_parent.so [--envs 65536] [--servers 4]
    python tools/ps_cores_ab.py --bench marllb_amd/exp/liblbsim_parent.so [--runs 4]
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

from tools.processor_sharing_ab import bench_ab  # noqa: E402  (the same headline A/B)


def one_leg(args):
    """A child: one leg, one round -> one JSON line."""
    import torch
    from marllb_amd import VecLoadBalanceEnv, _lib, sample_server_workers

    lib = _lib.load()
    NC = _lib.PROFILE_CLASSES
    B, S = args.envs, args.servers
    env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=args.seed, autoreset=False,
                            max_steps=10 ** 9, service_discipline="ps")
    if args.leg == "c":
        env.set_ps_cores(torch.ones((B, S), dtype=torch.int32))
    elif args.leg == "d":
        base = [env.cfg.server_rate[s] for s in range(S)]
        counts, mu = sample_server_workers(B, S, (1, 2, 4), seed=args.seed, keep_capacity=True,
                                           server_rates=base)
        env.set_ps_cores(counts)
        env.set_rates(None, mu)
    act = torch.randint(0, 3, (B, S), device="cuda:0",
                        generator=torch.Generator("cuda:0").manual_seed(args.seed))
    env.reset()
    for _ in range(args.warmup):
        out = env.step(act)
    torch.cuda.synchronize()
    h = env.handle
    h.check(lib.lbsim_profile_begin(h.h, 4 * args.steps + 8))
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = env.step(act)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    ms = (ctypes.c_double * NC)()
    cnt = (ctypes.c_int64 * NC)()
    h.check(lib.lbsim_profile_end_ex(h.h, ms, cnt, NC))
    print(json.dumps({"leg": args.leg, "dynamics_us": ms[0] / args.steps * 1e3,
                      "wall_us_per_step": el / args.steps * 1e6,
                      "kernels": _lib.launch_names(h),
                      "mean_obs_column0": float(out[0][:, :, 0].mean())}), flush=True)
    env.close()


def legs(args):
    parent_lib = os.path.abspath(args.legs)
    res = {k: [] for k in "abcd"}
    for _ in range(args.rounds):
        for leg in "abcd":
            env = dict(os.environ)
            env.pop("LBSIM_LIBRARY", None)
            if leg == "a":
                env["LBSIM_LIBRARY"] = parent_lib
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg,
                                "--envs", str(args.envs), "--servers", str(args.servers),
                                "--steps", str(args.steps), "--warmup", str(args.warmup),
                                "--seed", str(args.seed)],
                               cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"leg {leg} failed:\n{r.stdout[-1000:]}{r.stderr[-2000:]}")
            res[leg].append(json.loads(r.stdout.strip().splitlines()[-1]))
    dyn = {k: [x["dynamics_us"] for x in v] for k, v in res.items()}
    print(json.dumps({
        "envs": args.envs, "servers": args.servers, "steps": args.steps, "rounds": args.rounds,
        "kernels": {k: v[-1]["kernels"] for k, v in res.items()},
        "mean_obs_column0": {k: v[-1]["mean_obs_column0"] for k, v in res.items()},
        "legs": {k: {"dynamics_us_median": round(statistics.median(dyn[k]), 2),
                     "dynamics_us_min_max": [round(min(dyn[k]), 2), round(max(dyn[k]), 2)],
                     "wall_us_per_step_median": round(statistics.median(
                         x["wall_us_per_step"] for x in res[k]), 2)} for k in res},
        "b_median_inside_a_min_max":
            min(dyn["a"]) <= statistics.median(dyn["b"]) <= max(dyn["a"])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench", metavar="PARENT_LIB", default=None)
    ap.add_argument("--legs", metavar="PARENT_LIB", default=None)
    ap.add_argument("--leg", choices="abcd", default=None, help="(a child of --legs)")
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--servers", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    if args.leg:
        one_leg(args)
    elif args.bench:
        bench_ab(args.bench, args.runs, args.steps, args.warmup)
    elif args.legs:
        legs(args)
    else:
        ap.error("one of --legs PARENT_LIB or --bench PARENT_LIB")


if __name__ == "__main__":
    main()
