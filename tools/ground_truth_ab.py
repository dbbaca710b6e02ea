#!/usr/bin/env python3
"""Cost of the ground-truth read-out (lbsim_ground_truth), one JSON line per
result.  No target was set in advance: the figures are recorded as measured.

--bench PARENT_LIB: the headline bench.py on the parent commit's library (through LBSIM_LIBRARY)
  and on the in-tree build, alternating, --runs each: the default step launches nothing new, so
  this tree's median should lie inside the parent's own spread.

The call itself (default), per shape and handle kind:
  default        a default handle (the rates from the config: no optional array)
  workers_cross  server_workers plus cross_traffic at a share of 0.5, per-env rates: every
                 optional array but `down`
HIP events around --calls calls of ground_truth() into one reused buffer, the median of --rounds
rounds; the same around --calls steps of the handle, for the share of a step the call adds.
Bytes the rule must touch per server: the state words it reads (hc, and c, lost_on and the rate
where the handle has them), 8 per ring entry it reads (counted from the state: none from an empty
queue, two where 1 < c <= n) and the 32 it writes.

    python tools/ground_truth_ab.py [--shapes 65536x4,65536x8] [--calls 50] [--rounds 7]
    python tools/ground_truth_ab.py --bench marllb_amd/exp/liblbsim_parent.so [--runs 4]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

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


def timed(torch, fn, calls, rounds):
    """us per call: HIP events around `calls` calls, the median and the range of the rounds."""
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(calls):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls * 1e3)
    return round(statistics.median(out), 3), [round(min(out), 3), round(max(out), 3)]


def call_cost(args):
    import torch
    from marllb_amd import VecLoadBalanceEnv
    from marllb_amd.randomize import sample_server_workers

    for shape in args.shapes.split(","):
        B, S = (int(x) for x in shape.split("x"))
        for kind in ("default", "workers_cross"):
            extra = {}
            if kind == "workers_cross":
                extra = {"server_workers": True, "cross_traffic": True}
            env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=args.seed, autoreset=False,
                                    max_steps=10 ** 9, **extra)
            words = 4  # hc
            if kind == "workers_cross":
                w, mu = sample_server_workers(B, S, seed=args.seed,
                                              server_rates=float(env.cfg.server_rate[0]))
                env.set_server_workers(w)
                env.set_rates(None, mu)
                env.set_cross_traffic(0.5)
                words += 12  # c, lost_on, the per-env rate
            g = torch.Generator(device="cuda:0").manual_seed(args.seed)
            acts = [torch.randint(0, 3, (B, S), device="cuda:0", generator=g) for _ in range(8)]
            env.reset()
            for i in range(args.warmup):
                env.step(acts[i % 8])
            buf = torch.empty((B, S, 8), dtype=torch.float32, device="cuda:0")
            env.ground_truth(out=buf)
            torch.cuda.synchronize()
            step_us, step_rng = timed(torch, lambda i: env.step(acts[i % 8]), args.calls,
                                      args.rounds)
            call_us, call_rng = timed(torch, lambda i: env.ground_truth(out=buf), args.calls,
                                      args.rounds)
            t = env.ground_truth(out=buf)
            n = t[..., 0]
            c = env.get_server_workers().float() if kind == "workers_cross" else torch.ones_like(n)
            reads = (n > 0).float() + ((c > 1) & (n >= c)).float()
            ring = 8.0 * float(reads.mean())
            per_server = words + ring + 32.0
            total = per_server * B * S
            print(json.dumps({
                "shape": shape, "handle": kind, "calls": args.calls, "rounds": args.rounds,
                "call_us_median": call_us, "call_us_min_max": call_rng,
                "step_us_median": step_us, "step_us_min_max": step_rng,
                "call_share_of_step": round(call_us / step_us, 4),
                "bytes_per_server": {"state_words": words, "ring_entries_mean": round(ring, 2),
                                     "written": 32, "total": round(per_server, 2)},
                "bytes_total": int(total), "achieved_GBps": round(total / (call_us * 1e-6) / 1e9, 1),
                "mean_n_total": round(float(n.mean()), 3),
                "mean_n_hidden": round(float(t[..., 1].mean()), 3)}), flush=True)
            env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bench", metavar="PARENT_LIB", default=None)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--shapes", default="65536x4,65536x8")
    ap.add_argument("--steps", type=int, default=50, help="--bench: bench.py --steps")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    if args.bench:
        bench_ab(args.bench, args.runs, args.steps, args.warmup)
    else:
        call_cost(args)


if __name__ == "__main__":
    main()
