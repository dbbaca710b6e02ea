#!/usr/bin/env python3
"""Cost of the exact flow statistics (lbsim_flow_stats_enable) at the headline shapes, one process,
legs interleaved.

  a  the default handle (the plain server-per-lane kernel)
  b  a full handle without statistics (duration_mode="service": dynamics_group_full_kernel and the
     duration plane) -- (b) against (a) is the price of the full kernel
  c  flow_stats=True (dynamics_group_full_kernel with the accumulation; no duration plane) --
     (c) against (b) is the accumulation itself, the histogram read-modify-write included

Per leg: the dynamics launch time from the handle's own profiler (lbsim_profile_begin / _end_ex)
and wall-clock env-steps/s, median and min-max over the rounds.  One JSON line per shape.

    python tools/flow_stats_ab.py [--shapes 65536x4,65536x8] [--steps 50] [--warmup 20] [--rounds 7]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = {"a": {}, "b": {"duration_mode": "service"}, "c": {"flow_stats": True}}


def main():
    import torch
    from marllb_amd import VecLoadBalanceEnv, _lib

    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x4,65536x8")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    lib = _lib.load()
    NC = _lib.PROFILE_CLASSES
    for shape in args.shapes.split(","):
        B, S = (int(x) for x in shape.split("x"))
        envs = {k: VecLoadBalanceEnv(B, S, device="cuda:0", seed=args.seed, autoreset=False,
                                     max_steps=10 ** 9, **kw) for k, kw in LEGS.items()}
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
        names = {k: _lib.launch_names(e.handle) for k, e in envs.items()}
        for k in "bc":
            assert names[k][0].startswith("dynamics_group_full_kernel<"), names[k]
        flows = int(envs["c"].flow_stats()["count"].sum())
        print(json.dumps({
            "shape": shape, "steps": args.steps, "rounds": args.rounds, "kernels": names,
            "flows_counted": flows,
            "legs": {k: {"dynamics_us_median": round(statistics.median(dyn[k]), 2),
                         "dynamics_us_min_max": [round(min(dyn[k]), 2), round(max(dyn[k]), 2)],
                         "env_steps_per_s_median": round(statistics.median(rate[k])),
                         "env_steps_per_s_min_max": [round(min(rate[k])), round(max(rate[k]))]}
                     for k in envs}}), flush=True)
        for e in envs.values():
            e.close()


if __name__ == "__main__":
    main()
