#!/usr/bin/env python3
"""Cost of the on-device snapshots (lbsim_state_save / lbsim_state_load) at the headline shapes,
one process, legs interleaved, HIP events.

  copy       the yardstick: torch.empty_like(buf).copy_(buf) on a buffer of the snapshot's size
             (the runtime's device-to-device copy)
  save       lbsim_state_save of every env
  load       lbsim_state_load of every env (src_env NULL)
  load_1_16  lbsim_state_load of a random 1/16 of the envs (the others: index -1, kept)
  load_bcast lbsim_state_load with src_env all 0 (every env takes saved env 0)
  host       lbsim_get_state + lbsim_set_state (the host round trip), wall clock, few rounds

Per leg: time per call over `rounds` rounds of `inner` calls each, median and min-max, the ratio
of the median to the yardstick's and the bytes the call reads plus writes over the median.  One
JSON line per shape, with the sections' bytes by path (whole-wave rows / lane-per-unit rows and
the unit width) so a miss can be read against where the bytes are.

    python tools/state_snapshot_ab.py [--shapes 65536x4,65536x8] [--rounds 9] [--inner 10]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROW_MIN = 256  # csrc/lbsim_snapshot.h kSnapRowMin


def section_table(env):
    """(name, bytes per env, path, unit width) per section, by the rules of snap_table_build for
    a 16-byte aligned buffer."""
    from tests import statelayout
    import numpy as np
    cfg = env.cfg
    B = cfg.num_envs
    secs = statelayout.sections(B, cfg.num_servers, cfg.queue_capacity, bool(cfg.normalize_obs),
                                cfg.fail_prob > 0, statelayout.has_leak(cfg),
                                statelayout.has_dur_plane(cfg), statelayout.split_p(cfg))
    out, off = [], 0
    for name, dt, n in secs:
        row = np.dtype(dt).itemsize * n // B
        wide = row % 16 == 0 and off % 16 == 0
        out.append((name, row, "wave" if row >= ROW_MIN else "lane", 16 if wide else 4))
        off += row * B
    return out


def main():
    import torch
    from marllb_amd import VecLoadBalanceEnv

    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="65536x4,65536x8")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--warm-steps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("state_snapshot_ab.py measures on a HIP device; none found")
    dev = torch.device("cuda:0")
    for shape in args.shapes.split(","):
        B, S = (int(x) for x in shape.split("x"))
        env = VecLoadBalanceEnv(B, S, device=dev, seed=args.seed, autoreset=False,
                                max_steps=10 ** 9)
        env.reset()
        act = torch.randint(0, 3, (B, S), device=dev)
        for _ in range(args.warm_steps):
            env.step(act)
        h = env.handle
        n = h.state_size()
        buf = torch.empty(n, dtype=torch.uint8, device=dev)
        h.state_save(buf)
        gen = torch.Generator(device=dev)
        gen.manual_seed(args.seed)
        ident = torch.arange(B, dtype=torch.int32, device=dev)
        pick = torch.rand(B, device=dev, generator=gen) < 1.0 / 16.0
        src_16 = torch.where(pick, ident, torch.full_like(ident, -1))
        src_0 = torch.zeros(B, dtype=torch.int32, device=dev)
        moved = int(pick.sum())
        legs = {
            "copy": (lambda: torch.empty_like(buf).copy_(buf), 2 * n),
            "save": (lambda: h.state_save(buf), 2 * n),
            "load": (lambda: h.state_load(buf), 2 * n),
            "load_1_16": (lambda: h.state_load(buf, src_16), 2 * n * moved // B),
            # every env reads saved env 0's rows: one env's bytes read, all written
            "load_bcast": (lambda: h.state_load(buf, src_0), n + n // B),
        }
        for fn, _ in legs.values():  # warm-up: code objects, the allocator's block for the copy
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in legs}
        for _ in range(args.rounds):
            for k, (fn, _) in legs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.inner):
                    fn()
                t1.record()
                t1.synchronize()
                us[k].append(t0.elapsed_time(t1) * 1e3 / args.inner)
        h.state_load(buf)  # the state the legs started from
        torch.cuda.synchronize()
        host = []
        for _ in range(args.host_rounds):
            t = time.perf_counter()
            data = h.state_bytes()
            h.load_state(data)
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t) * 1e6)
        yard = statistics.median(us["copy"])
        table = section_table(env)
        by_path = {}
        for _, row, path, width in table:
            key = f"{path}_{width}B"
            by_path[key] = by_path.get(key, 0) + row
        print(json.dumps({
            "shape": shape, "state_bytes": n, "bytes_per_env": n // B, "rounds": args.rounds,
            "inner": args.inner, "envs_in_1_16_mask": moved,
            "bytes_per_env_by_path": by_path,
            "sections": [{"name": nm, "row_bytes": row, "path": path, "unit": width}
                         for nm, row, path, width in table],
            "legs": {k: {"us_median": round(statistics.median(v), 1),
                         "us_min_max": [round(min(v), 1), round(max(v), 1)],
                         "x_copy": round(statistics.median(v) / yard, 3),
                         "moved_GBps": round(legs[k][1] / statistics.median(v) * 1e-3, 1)}
                     for k, v in us.items()},
            "host_get_set_us": {"median": round(statistics.median(host)),
                                "min_max": [round(min(host)), round(max(host))],
                                "x_copy": round(statistics.median(host) / yard, 1)},
        }), flush=True)
        env.close()
        del buf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
