"""bench.py's command line: a plain run is the headline alone, `--dump-outputs` writes what the
last timed step returned, and the same arguments give the same arrays.

One small bench process (2048 envs x 4 servers, 2 warm-up + 3 timed steps); the expected arrays
come from stepping the same env in this process from the same seeds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, W, K, SEED = 2048, 4, 2, 3, 77


def test_full_only_legs_need_full():
    """The legs that moved behind --full are refused, not silently dropped, without it (argparse
    exits before anything touches the GPU)."""
    for extra in (["--late-episode", "1000"], ["--async-groups", "4"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *extra],
                           cwd=ROOT, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-500:]


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    import torch

    from marllb_amd.env import VecLoadBalanceEnv
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", str(K), "--warmup", str(W), "--batch", str(B),
                        "--seed", str(SEED), "--prewarm-ms", "0", "--dump-outputs", d],
                       cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["steps"] == K and out["warmup"] == W and out["higher_is_better"] is True
    assert out["unit"] == "env-steps/s" and out["ms_per_step"] > 0
    assert abs(out["value"] - B / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    for leg in ("roofline", "graph", "cpu_baseline", "late_episode", "async_groups"):
        assert leg not in out, leg

    # the same env, seeds and action generator as bench.py's rollout workload
    dev = torch.device("cuda", 0)
    env = VecLoadBalanceEnv(B, S, max_steps=10000, device=dev, seed=SEED, env_id_offset=0,
                            autoreset=True, assign_policy="sed", trace=None, dyn_mapping="auto",
                            autoreset_mode="same_step")
    env.reset()
    gen = torch.Generator(device=dev)
    gen.manual_seed(SEED)
    for _ in range(W + K):
        obs, rew, done, info = env.step(
            torch.randint(0, 3, (B, S), device=dev, dtype=torch.int64, generator=gen))
    want = {"obs": obs, "reward": rew, "done": done,
            "info_episode_length": info["episode_length"],
            "info_episode_return": info["episode_return"]}
    got = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(got) == sorted(want) and sorted(out["dumped_outputs"]) == sorted(want)
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    for name, t in want.items():
        a = t.cpu().numpy()
        assert got[name].dtype == (np.float64 if a.dtype == np.float64 else np.float32), name
        assert got[name].shape == a.shape, name
        np.testing.assert_array_equal(got[name], a.astype(got[name].dtype), err_msg=name)
    assert got["obs"].shape == (B, S, 11) and np.abs(got["obs"]).sum() > 0
    env.close()
