#!/usr/bin/env python3
"""Cost of trace banks (lbsim_set_trace_bank / lbsim_set_trace_schedule), DESIGN.md §3.14.

Two measurements, each one JSON line per result:

--bench PARENT_LIB: bench.py on the parent commit's library (through LBSIM_LIBRARY) and on the
  in-tree build, alternating, --runs each, for the existing TRACE path (--trace
  poisson_for_loop_rate_500 --servers 8) and for the Poisson headline (no arguments): both medians
  and the parent's min - max.  The TRACE instantiations now read a per-env descriptor behind a null
  test; no Poisson instantiation changed.

default: the dynamics launch at --shape (65536x8) on three handles in one process, legs interleaved:
  a  set_trace, as before
  b  a bank of four copies of that trace with random ids: identical bits, so identical work -- the
     difference to (a) is the gather launch and the per-env descriptor
  c  a bank of the trace rescaled to 0.5x, 1x and 1.5x its load with random ids: a wave runs as
     long as its busiest env (the lock-step cost of §3.10), so a slowdown is expected (a finding,
     not a failure)
  Per leg: the dynamics launch time from the handle's own profiler (the gather launch is not part
  of it) and wall-clock env-steps/s (it is), median over the rounds.

    python tools/trace_bank_ab.py [--shape 65536x8] [--steps 50] [--warmup 20] [--rounds 7]
    python tools/trace_bank_ab.py --bench marllb_amd/exp/liblbsim_parent.so [--runs 4]
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
    for tag, extra in (("trace", ["--trace", "poisson_for_loop_rate_500", "--servers", "8"]),
                       ("poisson", [])):
        vals = {"parent": [], "tree": []}
        for _ in range(runs):
            for which in ("parent", "tree"):
                env = dict(os.environ)
                env.pop("LBSIM_LIBRARY", None)
                if which == "parent":
                    env["LBSIM_LIBRARY"] = parent_lib
                r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                                    "--steps", str(steps), "--warmup", str(warmup),
                                    "--no-cpu-baseline", *extra],
                                   cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    sys.exit(f"bench.py ({which}, {tag}) failed:\n{r.stdout[-1000:]}{r.stderr[-2000:]}")
                line = json.loads(r.stdout.strip().splitlines()[-1])
                vals[which].append(float(line["value"]))
                print(json.dumps({"bench": tag, "library": which, "value": line["value"],
                                  "unit": line.get("unit"), "metric": line.get("metric")}),
                      flush=True)
        p, t = vals["parent"], vals["tree"]
        print(json.dumps({"bench": tag, "runs": runs, "parent_median": statistics.median(p),
                          "parent_min_max": [min(p), max(p)], "tree_median": statistics.median(t),
                          "tree_min_max": [min(t), max(t)],
                          "tree_median_inside_parent_spread":
                              min(p) <= statistics.median(t) <= max(p)}), flush=True)


def legs(args):
    import torch
    from marllb_amd import VecLoadBalanceEnv, _lib, trace
    from marllb_amd.randomize import sample_trace_ids

    lib = _lib.load()
    NC = _lib.PROFILE_CLASSES
    B, S = (int(x) for x in args.shape.split("x"))
    base = trace.builtin("poisson_for_loop_rate_500")
    banks = {"a": base, "b": [base] * 4,
             "c": [base, trace.rescaled(base, 0.5), trace.rescaled(base, 1.5)]}
    envs = {k: VecLoadBalanceEnv(B, S, device="cuda:0", seed=args.seed, autoreset=False,
                                 max_steps=10 ** 9, trace=banks[k]) for k in "abc"}
    envs["b"].set_env_trace(sample_trace_ids(B, 4, args.seed))
    envs["c"].set_env_trace(sample_trace_ids(B, 3, args.seed))
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
    ap.add_argument("--shape", default="65536x8")
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
