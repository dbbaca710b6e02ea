"""The GPU-vs-oracle parity harness the test files share: the device guard, the action streams,
the per-step and whole-state comparisons (all bit for bit), the 12 + 4-step driver around them,
the child-process runner for settings the library reads once per process, and the kernel-name
check under those settings."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import statelayout

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV_LANE, GROUP, WAVE = 0, 1, 2  # lbsim_dyn_kernel


def _require_device():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a HIP device")


@pytest.fixture(scope="module")
def lib():
    _require_device()
    from marllb_amd import _lib
    return _lib


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    _require_device()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to("cuda:0") if dtype is None else t.to("cuda:0", dtype)


def simds():
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def actions(rng, B, S, kw, levels=False):
    """One step's actions for the config kwargs kw.  levels (tests/test_gpu_parity.py's stream):
    discrete actions range over kw's discrete_weights, and continuous ones always draw the NaN
    positions (kw's test option _nan_actions, a fraction) after the values."""
    if kw.get("action_type") == "continuous":
        a = rng.uniform(-1.0, 11.0, (B, S)).astype(np.float32)
        if levels:
            a[rng.random((B, S)) < kw.get("_nan_actions", 0.0)] = np.nan
        return a
    n = len(kw.get("discrete_weights", [1, 1.5, 2])) if levels else 3
    return rng.integers(-n, n, (B, S)).astype(np.int64)


def step_both(env, ref, a, k):
    """Step k of the env and of ref (OracleEnv's step(a) -> obs, reward, done, assign counts) with
    the same actions: the four outputs are equal.  Returns the reference's done."""
    og, rg, dg, info = env.step(torch.from_numpy(a), assign_counts=True)
    oo, ro, do, ao = ref.step(a)
    np.testing.assert_array_equal(info["assign_counts"].cpu().numpy(), ao, err_msg=f"assign step {k}")
    np.testing.assert_array_equal(og.cpu().numpy(), oo, err_msg=f"obs step {k}")
    np.testing.assert_array_equal(rg.cpu().numpy(), ro, err_msg=f"reward step {k}")
    np.testing.assert_array_equal(dg.cpu().numpy().astype(np.uint8), do, err_msg=f"done step {k}")
    return do


def _state(snap, cfg):
    """A state_bytes() snapshot of cfg.num_envs envs, or a list of one-env snapshots, parsed and
    concatenated section by section along the env axis; ring / pend by their live entries (stale
    slots beyond the counts are not state)."""
    parts, b = ([snap], cfg.num_envs) if isinstance(snap, bytes) else (snap, 1)
    S, Q, P = cfg.num_servers, cfg.queue_capacity, statelayout.split_p(cfg)
    out = {}
    for p in (statelayout.parse_cfg(s, cfg, B=b) for s in parts):
        p["_live_ring"] = statelayout.live_ring(p, b, S, Q)
        if P:
            p["_live_pend"] = statelayout.live_pend(p, b, S, P)
        for name, v in p.items():
            out.setdefault(name, []).append(v)
    return {name: np.concatenate(v) for name, v in out.items()}


def compare_state(handle, ref, cfg):
    """Every state word of handle.state_bytes() against ref.state_bytes() (one snapshot, or a list
    of one-env snapshots in env order).  Returns the parsed reference side."""
    g, o = _state(handle.state_bytes(), cfg), _state(ref.state_bytes(), cfg)
    assert list(g) == list(o)
    for name in g:
        if name not in ("ring", "pend"):
            np.testing.assert_array_equal(g[name], o[name], err_msg=name)
    return o


def run_vs_reference(env, ref, akw, seed, steps=12, post_steps=4, hook=None, levels=False):
    """Reset both and step them side by side on actions(default_rng(seed), ..., akw, levels):
    the outputs of every step, the whole state after `steps` steps (hook(env) first: the check of
    the kernel that ran) and again after a masked reset of every third env and `post_steps` more
    steps.  Returns the reference state after `steps` steps; closes nothing."""
    B, S = env.cfg.num_envs, env.cfg.num_servers
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    rng = np.random.default_rng(seed)
    for k in range(steps):
        step_both(env, ref, actions(rng, B, S, akw, levels), k)
    if hook is not None:
        hook(env)
    mid = compare_state(env.handle, ref, env.cfg)
    mask = (np.arange(B) % 3 == 0).astype(np.uint8)
    og = env.reset(mask=torch.from_numpy(mask)).cpu().numpy()
    np.testing.assert_array_equal(og, ref.reset(mask=mask, obs=og.copy()))
    for k in range(post_steps):
        step_both(env, ref, actions(rng, B, S, akw, levels), steps + k)
    compare_state(env.handle, ref, env.cfg)
    return mid


def run_cases_in_child(test_file, test_ids, env_over, timeout=600):
    """Tests of tests/<test_file> in a child pytest with env_over in its environment (settings the
    library reads once per process).  test_ids: the ids to run, or a string, a -k expression over
    the whole file."""
    path = os.path.join(ROOT, "tests", test_file)
    select = [path, "-k", test_ids] if isinstance(test_ids, str) else [path + "::" + k for k in test_ids]
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p",
                        "no:cacheprovider"] + select,
                       cwd=ROOT, env={**os.environ, **env_over}, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def check_dispatch(lib, env, default, forced_group=None, forced_wave=False):
    """The kernel form that ran, by lbsim_dynamics_kernel and the launch names of the last step.
    In a child run under LBSIM_DYN_GROUP_LANES the handle steps with groups of that width if
    forced_group is not None and its servers fit: forced_group names the dynamics kernel ("" for
    a one-launch step: only the form is checked).  Under LBSIM_DYN_WAVE=1 it steps one wave per
    env if forced_wave.  Otherwise default(kern, names), the case's own expectation."""
    kern = lib.load().lbsim_dynamics_kernel(env.handle.h)
    names = lib.launch_names(env.handle)
    lanes, wave = os.environ.get("LBSIM_DYN_GROUP_LANES"), os.environ.get("LBSIM_DYN_WAVE")
    if lanes and forced_group is not None and int(lanes) >= env.cfg.num_servers:
        assert kern == GROUP, (kern, names)
        if forced_group:
            assert names.get(0, "").startswith(f"{forced_group}<{lanes},"), names
    elif wave == "1" and forced_wave:
        assert kern == WAVE, (kern, names)
        assert (names.get(0, "").startswith("dynamics_wave_kernel<")
                or names.get(4, "").startswith("step_wave_kernel<")), names
    else:
        default(kern, names)
