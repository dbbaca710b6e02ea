#!/usr/bin/env python3
"""Cost of a rate schedule (lbsim_set_rate_schedule) at the headline shape, one process, legs
interleaved.

  a  no schedule (the config's shared arrival_rate / server_rate[])
  b  a schedule of P = 24 phases that all hold the config's values: identical bits, so identical
     work -- the difference to (a) is the cost of the phase lookup (the episode-step load, the
     division, the table reads)
  c  marllb_amd.randomize.diurnal_schedule around the config's arrival rate, P = 24: the loads of
     a wave's envs differ, and a wave runs as long as the slowest of them, so a slowdown is
     expected (a finding, not a failure)

Per leg: the dynamics launch time from the handle's own profiler (lbsim_profile_begin / _end_ex)
and wall-clock env-steps/s, median over the rounds.  One JSON line per shape.

    python tools/rate_schedule_ab.py [--shapes 65536x4] [--steps 50] [--warmup 20] [--rounds 7]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from marllb_amd import VecLoadBalanceEnv, _lib, diurnal_schedule

    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x4")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--phases", type=int, default=24)
    ap.add_argument("--steps-per-phase", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    lib = _lib.load()
    NC = _lib.PROFILE_CLASSES
    P, H = args.phases, args.steps_per_phase
    for shape in args.shapes.split(","):
        B, S = (int(x) for x in shape.split("x"))
        envs = {k: VecLoadBalanceEnv(B, S, device="cuda:0", seed=args.seed, autoreset=False,
                                     max_steps=10 ** 9) for k in "abc"}
        cfg = envs["a"].cfg
        envs["b"].set_rate_schedule(torch.full((P,), cfg.arrival_rate),
                                    torch.tensor(cfg.server_rate[:S]).repeat(P, 1),
                                    steps_per_phase=H)
        gen = torch.Generator()
        gen.manual_seed(args.seed)
        envs["c"].set_rate_schedule(
            diurnal_schedule(torch.full((B,), cfg.arrival_rate), P, amplitude=(0.2, 0.8),
                             generator=gen), None, steps_per_phase=H)
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
        names = _lib.launch_names(envs["a"].handle)
        assert names == _lib.launch_names(envs["c"].handle), "the legs must run the same kernels"
        assert envs["a"].get_state() == envs["b"].get_state(), "leg b must compute leg a's bits"
        print(json.dumps({
            "shape": shape, "steps": args.steps, "rounds": args.rounds, "phases": P,
            "steps_per_phase": H, "kernels": names,
            "legs": {k: {"dynamics_us_median": round(statistics.median(dyn[k]), 2),
                         "dynamics_us_min_max": [round(min(dyn[k]), 2), round(max(dyn[k]), 2)],
                         "env_steps_per_s_median": round(statistics.median(rate[k]))}
                     for k in envs}}), flush=True)
        for e in envs.values():
            e.close()


if __name__ == "__main__":
    main()
