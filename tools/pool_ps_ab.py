#!/usr/bin/env python3
"""Cost of shared server pools with processor-sharing servers (lbsim_server_pool_enable_ps,
DESIGN.md section 3.24), one process, legs interleaved.  Recorded with no target.

Two measurements, each one JSON line per result:

--bench PARENT_LIB: the headline bench.py on the parent commit's library (through LBSIM_LIBRARY)
  and on the in-tree build, alternating, --runs each: a default handle must not pay (this tree's
  median inside the parent's own min - max).

The legs (default), the dynamics launch of a step at --envs x --servers, every pool leg envs / 4
pools of 4 members, each member at a quarter of the config's arrival rate:
  a  a FIFO pool (dynamics_pool_kernel)
  b  a PS pool, cores never set (dynamics_pool_ps_kernel, a null cores pointer)
  c  a PS pool with sample_server_workers counts from (1, 2, 4) at equal capacity: a pool's server
     rates are the config's, so ONE row of counts is drawn for the S servers, the config's rates
     are divided by it and every pool gets that row
  d  a plain PS handle (dynamics_ps_kernel), envs independent balancers at the config's rate
Per leg: the dynamics launch from the handle's profiler (class 0) and wall-clock us per step,
median over the rounds.

    python tools/pool_ps_ab.py [--envs 65536] [--servers 4] [--steps 50] [--rounds 7]
    python tools/pool_ps_ab.py --bench marllb_amd/exp/liblbsim_parent.so [--runs 4]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.server_pool_ab import bench_ab  # noqa: E402  (the same alternating headline runs)


def legs(args):
    import torch
    from marllb_amd import VecLoadBalanceEnv, _lib
    from marllb_amd.randomize import sample_server_workers

    lib = _lib.load()
    NC = _lib.PROFILE_CLASSES
    B, S, A = args.envs, args.servers, args.balancers
    base = dict(device="cuda:0", seed=args.seed, autoreset=False, max_steps=10 ** 9)
    plain = VecLoadBalanceEnv(B, S, service_discipline="ps", **base)
    cfg = plain.cfg
    mu = [cfg.server_rate[s] for s in range(S)]
    pool = dict(balancers_per_pool=A, arrival_rate=cfg.arrival_rate / A, **base)
    counts, rate = sample_server_workers(1, S, (1, 2, 4), seed=args.seed, server_rates=mu)
    envs = {"a": VecLoadBalanceEnv(B, S, server_rates=mu, **pool),
            "b": VecLoadBalanceEnv(B, S, server_rates=mu, pool_discipline="ps", **pool),
            "c": VecLoadBalanceEnv(B, S, server_rates=[float(x) for x in rate[0]],
                                   pool_discipline="ps", pool_ps_cores=counts[0], **pool),
            "d": plain}
    act = torch.randint(0, 3, (B, S), device="cuda:0")
    last = {}
    for k, e in envs.items():
        e.reset()
        for _ in range(args.warmup):
            last[k] = e.step(act)
    torch.cuda.synchronize()
    dyn = {k: [] for k in envs}
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
            wall[k].append(el / args.steps * 1e6)
    phys = {"a": float(envs["a"].ground_truth()[:, :, 0].mean()),
            "b": float(envs["b"].pool_ps_state()[:, :, 0].mean()),
            "c": float(envs["c"].pool_ps_state()[:, :, 0].mean()),
            "d": float(envs["d"].ps_state()[:, :, 0].mean())}
    print(json.dumps({
        "envs": B, "servers": S, "balancers": A, "steps": args.steps, "rounds": args.rounds,
        "cores_c": [int(x) for x in counts[0]],
        "kernels": {k: _lib.launch_names(e.handle) for k, e in envs.items()},
        "mean_obs_column0": {k: float(last[k][0][:, :, 0].mean()) for k in envs},
        "mean_physical_queue": phys,
        "legs": {k: {"dynamics_us_median": round(statistics.median(dyn[k]), 2),
                     "dynamics_us_min_max": [round(min(dyn[k]), 2), round(max(dyn[k]), 2)],
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
    ap.add_argument("--balancers", type=int, default=4)
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
