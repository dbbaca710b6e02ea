"""Scripted server availability (lbsim_set_server_avail, VecLoadBalanceEnv.set_server_availability;
DESIGN.md §3.16).

The reference is the unmodified oracle created with fail_prob = 1e-9 and recover_prob = 0: it has
the down section, thresholds of 0 (it never draws a change) and honours the flags.  Before every
oracle step the test takes each env's phase from the oracle's own ep_step, applies the transition
rule to the oracle's snapshot in numpy (apply_rule) and loads the snapshot back; the GPU handle
(fail_prob = 0, enabled) gets the table once.  Observations, rewards, done flags, assignment
counts and the whole state are compared word for word, the GPU state parsed with the oracle's
config.

apply_rule is itself pinned on the CPU against the oracle's own failure branch
(test_numpy_rule_is_the_oracles_failure), and the kernel's body runs on the host between guard
bytes under the address and undefined-behaviour sanitizers (test_kernel_body_on_the_host).
"""
import os
import subprocess

import numpy as np
import pytest

from marllb_amd.randomize import (outage_schedule, rolling_restart_schedule,
                                  sample_cluster_sizes, schedule_phase)
from tests import parity, statelayout
from tests.parity import ENV_LANE, GROUP, actions, lib, step_both  # noqa: F401

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K = 128
LAST_NONE = -(1 << 30)


# ------------------------------------------------------------------ the rule, in numpy

def views(buf: bytearray, cfg, B=None):
    """Writable arrays over the sections of a snapshot held in a bytearray (tests/statelayout.py
    names), parsed with cfg's flags."""
    B = cfg.num_envs if B is None else B
    secs = statelayout.sections(B, cfg.num_servers, cfg.queue_capacity, bool(cfg.normalize_obs),
                                cfg.fail_prob > 0, statelayout.has_leak(cfg),
                                statelayout.has_dur_plane(cfg), statelayout.split_p(cfg))
    out, off = {}, 0
    for name, dt, n in secs:
        out[name] = np.frombuffer(buf, dtype=dt, count=n, offset=off)
        off += np.dtype(dt).itemsize * n
    assert off == len(buf), (off, len(buf))
    return out


def apply_rule(v, B, S, want_up, res_vpp, skip=None):
    """The transition of DESIGN.md §3.16 on the arrays v: server (b, s) is brought to want_up[b, s]
    (envs with skip[b] are left alone).  up -> down is the oracle's failure branch; down -> up
    clears the flag.  Returns the (B, S) mask of the servers that failed."""
    want_up = np.asarray(want_up, bool).reshape(B, S)
    live = np.ones((B, 1), bool) if skip is None else ~np.asarray(skip, bool).reshape(B, 1)
    down = v["down"].reshape(B, S)
    fail = (down == 0) & ~want_up & live
    back = (down != 0) & want_up & live
    hc = v["hc"].reshape(B, S)
    v["dropped"] += ((hc >> 16) * fail).sum(axis=1).astype(np.uint32)
    hc[fail] &= 0x7FFF  # the head: count 0, no big flag
    v["last_tc"].reshape(B, S)[fail] = LAST_NONE
    v["res_count"].reshape(B, S)[fail] = 0
    for name in ("lost_on", "res_count_dur", "pend_hc"):
        if name in v:
            v[name].reshape(B, S)[fail] = 0
    if res_vpp:
        v["res"].reshape(B, S, 2 * K)[fail] = 0
        for name in ("res_dur", "res_dur2"):
            if name in v:
                v[name].reshape(B, S, -1)[fail] = 0
    v["fcache"].reshape(B, S, 10)[fail] = 0.0
    down[fail] = 1
    down[back] = 0
    return fail


def ref_config(cfg):
    """cfg with the reference's failure settings: the down section, thresholds of 0."""
    c = type(cfg).from_buffer_copy(cfg)
    c.fail_prob, c.recover_prob = 1e-9, 0.0
    return c


def expand_table(up, B, S):
    """(P, S) shared or (B, P, S) -> (B, P, S) bool; None stays None."""
    if up is None:
        return None
    t = np.asarray(up.cpu() if hasattr(up, "cpu") else up) != 0
    t = np.broadcast_to(t[None], (B,) + t.shape) if t.ndim == 2 else t
    assert t.shape[0] == B and t.shape[2] == S
    return t


class AvailRef:
    """The oracle under an availability table.  inner: an OracleEnv of B envs made with
    ref_config, or an object with .envs, a list of B one-env oracles (ScheduledOracles)."""

    def __init__(self, inner, cfg, table=None, H=1, wrap=True):
        self.inner, self.cfg = inner, cfg
        self.B, self.S = cfg.num_envs, cfg.num_servers
        self.set_table(table, H, wrap)

    def set_table(self, table, H=1, wrap=True):
        self.table, self.H, self.wrap = expand_table(table, self.B, self.S), H, wrap

    def _pieces(self):
        envs = getattr(self.inner, "envs", None)
        return [(self.inner, 0, self.B)] if envs is None else [(o, b, 1) for b, o in enumerate(envs)]

    def want(self, ep_step, lo=0):
        """(want (n, S), skip (n,), phase (n,)) of the envs lo .. lo + n at episode steps ep_step."""
        n = len(ep_step)
        skip = (ep_step >= self.cfg.max_steps) if self.cfg.next_step_reset else np.zeros(n, bool)
        if self.table is None:
            return np.ones((n, self.S), bool), skip, np.zeros(n, np.int64)
        ph = schedule_phase(np.asarray(ep_step), self.table.shape[1], self.H, self.wrap)
        ph = np.where(skip, 0, ph)
        w = self.table[np.arange(lo, lo + n), ph]
        return np.where(skip[:, None], True, w), skip, ph

    def want_all(self):
        """What lbsim_get_server_avail reports: (want (B, S), up_now (B, S), phase (B,))."""
        w, u, p = [], [], []
        for o, lo, n in self._pieces():
            v = views(bytearray(o.state_bytes()), self.cfg, n)
            wi, _, pi = self.want(v["ep_step"], lo)
            w.append(wi), u.append(v["down"].reshape(n, self.S) == 0), p.append(pi)
        return np.concatenate(w), np.concatenate(u), np.concatenate(p)

    def apply(self):
        for o, lo, n in self._pieces():
            buf = bytearray(o.state_bytes())
            v = views(buf, self.cfg, n)
            w, skip, _ = self.want(v["ep_step"], lo)
            apply_rule(v, n, self.S, w, self.cfg.reservoir_mode == 1, skip)
            o.load_state(bytes(buf))

    def reset(self, mask=None, obs=None):
        return self.inner.reset(mask=mask, obs=obs)

    def step(self, a):
        self.apply()
        return self.inner.step(a)

    def state_bytes(self):
        return self.inner.state_bytes()

    def load_state(self, data):
        self.inner.load_state(data)

    def close(self):
        self.inner.close()


def make_table(B, S, P, seed, p_up=0.65):
    """(B, P, S) uint8, each server up with probability p_up per phase."""
    return (np.random.default_rng(seed).random((B, P, S)) < p_up).astype(np.uint8)


# ------------------------------------------------------------------ CPU: the rule, the helpers

LOST_FIN = {"lost_fin_prob": 0.3, "flow_timeout": 0.4}
RULE_CASES = {
    "s4": (4, {}),
    "s5-q8-900": (5, {"queue_capacity": 8, "arrival_rate": 900.0}),
    "s8-alias-700": (8, {"assign_policy": "alias", "action_type": "continuous",
                         "arrival_rate": 700.0}),
    "lost-fin": (4, LOST_FIN),
    "lost-fin-nflow-vpp": (4, {**LOST_FIN, "n_flow_on_mode": "vpp"}),
    "res-vpp": (4, {"reservoir_mode": "vpp"}),
    "res-vpp-lost-fin": (4, {**LOST_FIN, "reservoir_mode": "vpp"}),
    "service": (4, {"duration_mode": "service"}),
    "normalize": (4, {"normalize_obs": True}),
}


@pytest.mark.parametrize("case", list(RULE_CASES))
def test_numpy_rule_is_the_oracles_failure(oracle_mod, case):
    """Oracle A (fail_prob = recover_prob = 1) fails every server inside its even steps and
    recovers it inside the odd ones; oracle B (the reference handle) is edited all-down / all-up
    by apply_rule before each step.  From B's reset state, 6 envs and 10 steps: the outputs and
    every state section are equal, but for bit 0 of chg word 0 of the servers that failed (set by
    a failure inside the step, not by an edit before it)."""
    from marllb_amd.env import make_config
    S, kw = RULE_CASES[case]
    B = 6
    base = make_config(B, S, seed=40 + S, **kw)
    cb = ref_config(base)
    ca = type(base).from_buffer_copy(base)
    ca.fail_prob, ca.recover_prob = 1.0, 1.0
    a, b = oracle_mod.OracleEnv(ca), oracle_mod.OracleEnv(cb)
    a.reset()
    b.reset()
    a.load_state(b.state_bytes())
    ref = AvailRef(b, cb)
    rng = np.random.default_rng(3)
    lost = 0
    for k in range(10):
        failing = k % 2 == 0
        ref.set_table(np.full((1, S), 0 if failing else 1, np.uint8))
        before = int(views(bytearray(b.state_bytes()), cb)["dropped"].sum())
        act = actions(rng, B, S, kw)
        ra, rb = a.step(act), ref.step(act)
        for x, y, name in zip(ra, rb, ("obs", "reward", "done", "assign")):
            np.testing.assert_array_equal(x, y, err_msg=f"{name} step {k}")
        va, vb = views(bytearray(a.state_bytes()), cb), views(bytearray(b.state_bytes()), cb)
        lost += int(vb["dropped"].sum()) - before
        assert list(va) == list(vb)
        for name in va:
            if name == "chg":
                diff = (va[name] ^ vb[name]).reshape(B * S, 4)
                np.testing.assert_array_equal(diff[:, 0], 1 if failing else 0, err_msg=f"chg {k}")
                assert not diff[:, 1:].any()
            else:
                np.testing.assert_array_equal(va[name], vb[name], err_msg=f"{name} step {k}")
        np.testing.assert_array_equal(vb["down"], 1 if failing else 0)
    assert lost > 0  # queued flows were lost to the failures
    a.close()
    b.close()


def _probe_case(rng, B, S, split, res_vpp, has_lost, dur_words, P, H, wrap, next_reset, max_steps,
                has_table):
    BS = B * S
    v = {"ep_step": rng.integers(-1, max_steps + 3, B).astype(np.int32),
         "dropped": rng.integers(0, 1000, B).astype(np.uint32),
         "hc": (rng.integers(0, 32, BS) | (rng.integers(0, 2, BS) << 15)
                | (rng.integers(0, 33, BS) << 16)).astype(np.uint32),
         "last_tc": rng.integers(-1000, 10 ** 6, BS).astype(np.int32),
         "res_count": rng.integers(0, 1000, BS).astype(np.uint32),
         "res": rng.integers(1, 2 ** 32, BS * K * 2, dtype=np.uint64).astype(np.uint32),
         "fcache": rng.random(BS * 10).astype(np.float32) + 1.0,
         "down": (rng.random(BS) < 0.4).astype(np.uint32) * rng.integers(1, 3, BS).astype(np.uint32)}
    if has_lost:
        v["lost_on"] = rng.integers(1, 50, BS).astype(np.uint32)
    if dur_words:
        v["res_dur2" if dur_words == 2 else "res_dur"] = rng.integers(
            1, 2 ** 32, BS * K * dur_words, dtype=np.uint64).astype(np.uint32)
    if split:
        v["res_count_dur"] = rng.integers(1, 1000, BS).astype(np.uint32)
        v["pend_hc"] = rng.integers(1, 2 ** 20, BS).astype(np.uint32)
    table = None
    if has_table:  # any nonzero byte is up
        table = ((rng.random((B, P, S)) < 0.6) * rng.integers(1, 256, (B, P, S))).astype(np.uint8)
    head = np.zeros(16, np.int32)
    head[:12] = [B, S, split, res_vpp, has_lost, dur_words, P, H, wrap, next_reset, max_steps,
                 has_table]
    return head, v, table


PROBE_CASES = [
    # B, S, split, res_vpp, lost_on, dur words, P, H, wrap, next_reset, max_steps, table
    (24, 4, 0, 0, 0, 0, 3, 2, 1, 0, 10000, 1),
    (7, 3, 0, 0, 0, 0, 3, 2, 0, 0, 10000, 1),
    (5, 5, 1, 0, 1, 2, 4, 1, 1, 0, 10000, 1),
    (5, 7, 1, 1, 0, 2, 2, 3, 1, 1, 6, 1),
    (3, 20, 0, 1, 0, 1, 1, 1, 1, 0, 10000, 1),
    (4, 6, 0, 1, 0, 0, 5, 1, 0, 1, 6, 1),
    (9, 4, 0, 0, 0, 1, 3, 2, 1, 1, 6, 0),
    (1, 64, 0, 0, 0, 0, 4096, 1, 1, 0, 10000, 1),
]


def test_kernel_body_on_the_host(tmp_path):
    """csrc/lbsim_avail.h as host C++ (tests/avail_probe.cpp, address and undefined-behaviour
    sanitizers): every thread of a launch, on sections between guard bytes, writes what apply_rule
    writes -- split and reservoir_mode VPP layouts, S no power of two, clamped and cyclic tables,
    next-step resets, no table -- and a launch that only reports writes no state."""
    from marllb_amd import build
    exe = str(tmp_path / "avail_probe")
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "avail_probe.cpp")], check=True)
    rng = np.random.default_rng(11)
    order = ("ep_step", "dropped", "hc", "last_tc", "res_count", "res", "fcache", "down", "lost_on",
             "res_dur", "res_dur2", "res_count_dur", "pend_hc")
    for case in PROBE_CASES:
        B, S, split, res_vpp, _, _, P, H, wrap, next_reset, max_steps, has_table = case
        head, v, table = _probe_case(rng, *case)
        names = [n for n in order if n in v]
        fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(fin, "wb") as f:
            f.write(head.tobytes())
            for n in names:
                f.write(v[n].tobytes())
            if table is not None:
                f.write(table.tobytes())
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, (case, r.stderr[-3000:])
        raw = open(fout, "rb").read()
        want = np.frombuffer(raw, np.uint8, B * S).reshape(B, S)
        now = np.frombuffer(raw, np.uint8, B * S, B * S).reshape(B, S)
        phase = np.frombuffer(raw, np.int32, B, 2 * B * S)
        off = 2 * B * S + 4 * B
        got = {}
        for n in names:
            got[n] = np.frombuffer(raw, v[n].dtype, v[n].size, off)
            off += v[n].nbytes
        assert off == len(raw)
        # the expectation: schedule_phase and apply_rule
        skip = (v["ep_step"] >= max_steps) if next_reset else np.zeros(B, bool)
        ph = np.where(skip, 0, schedule_phase(v["ep_step"], P, H, bool(wrap))) if has_table else 0
        w = table[np.arange(B), ph] != 0 if has_table else np.ones((B, S), bool)
        w = np.where(skip[:, None], True, w)
        np.testing.assert_array_equal(want, w, err_msg=str(case))
        np.testing.assert_array_equal(now, v["down"].reshape(B, S) == 0, err_msg=str(case))
        np.testing.assert_array_equal(phase, np.broadcast_to(ph, (B,)), err_msg=str(case))
        exp = {n: x.copy() for n, x in v.items()}
        failed = apply_rule(exp, B, S, w, bool(res_vpp), skip)
        assert failed.any() == bool(has_table) and (~failed).any()
        assert (exp["down"] != v["down"]).any()
        for n in names:
            np.testing.assert_array_equal(got[n], exp[n], err_msg=f"{case} {n}")


def test_randomize_helpers():
    n = sample_cluster_sizes(500, 8, 2, seed=3)
    assert n.dtype == torch.int32 and tuple(n.shape) == (500,)
    assert int(n.min()) == 2 and int(n.max()) == 8
    assert torch.equal(n, sample_cluster_sizes(500, 8, 2, seed=3))
    assert not torch.equal(n, sample_cluster_sizes(500, 8, 2, seed=4))
    up = outage_schedule(40, 6, 10, 2, 3, 4, seed=5)
    assert up.dtype == torch.uint8 and tuple(up.shape) == (40, 10, 6)
    u = up.numpy().astype(bool)
    assert u[:, :3].all() and u[:, 7:].all()
    assert ((~u[:, 3:7]).sum(axis=2) == 2).all()
    for b in range(40):  # one block of consecutive servers (cyclically), the same in every phase
        d = np.flatnonzero(~u[b, 3])
        assert (d[1] - d[0]) % 6 in (1, 5)
        assert (u[b, 3:7] == u[b, 3]).all()
    assert len({tuple(np.flatnonzero(~u[b, 3])) for b in range(40)}) > 2
    assert torch.equal(up, outage_schedule(40, 6, 10, 2, 3, 4, seed=5))
    r = rolling_restart_schedule(4, 7).numpy()
    assert r.shape == (7, 4) and r[0].all()
    np.testing.assert_array_equal(np.argmin(r[1:], axis=1), [1, 2, 3, 0, 1, 2])
    assert (r[1:].sum(axis=1) == 3).all()
    with pytest.raises(ValueError):
        sample_cluster_sizes(4, 4, 5)
    with pytest.raises(ValueError):
        outage_schedule(4, 4, 3, 5, 0, 1)


def test_header_and_binding_agree():
    from marllb_amd import _lib
    names = {"lbsim_server_avail_enable", "lbsim_set_server_avail", "lbsim_clear_server_avail",
             "lbsim_get_server_avail"}
    assert names <= set(_lib.header_functions())
    assert names <= set(_lib._SIGNATURES)


# ------------------------------------------------------------------ GPU

def compare_state(env, ref):
    """Every state word of the GPU handle against the reference's, both parsed with the
    reference's config (the GPU handle's own fail_prob is 0)."""
    g = parity._state(env.handle.state_bytes(), ref.cfg)
    o = parity._state(ref.state_bytes(), ref.cfg)
    assert list(g) == list(o)
    for name in g:
        if name not in ("ring", "pend"):
            np.testing.assert_array_equal(g[name], o[name], err_msg=name)
    return o


def make_pair(oracle_mod, B, S, kw, env_kw=None, table=None, H=1, wrap=True):
    """A GPU env with server_availability=True and its reference, the table installed in both."""
    from marllb_amd.env import VecLoadBalanceEnv
    env = VecLoadBalanceEnv(B, S, device="cuda:0", server_availability=True,
                            **{"autoreset": False, **(env_kw or {})}, **kw)
    cfg = ref_config(env.cfg)
    ref = AvailRef(oracle_mod.OracleEnv(cfg), cfg, table, H, wrap)
    if table is not None:
        env.set_server_availability(table, steps_per_phase=H, wrap=wrap)
    return env, ref


def step_auto(env, ref, a, k):
    """step_both for an env that auto-resets in the same step: the reference resets its done envs
    after the step, and the GPU's observation holds their reset rows."""
    og, rg, dg, _ = env.step(torch.from_numpy(a))
    oo, ro, do, _ = ref.step(a)
    if do.any():
        oo = ref.reset(mask=do, obs=oo.copy())
    np.testing.assert_array_equal(og.cpu().numpy(), oo, err_msg=f"obs step {k}")
    np.testing.assert_array_equal(rg.cpu().numpy(), ro, err_msg=f"reward step {k}")
    np.testing.assert_array_equal(dg.cpu().numpy().astype(np.uint8), do, err_msg=f"done step {k}")


def drive(env, ref, kw, seed, steps=12, post=4, same_step=False):
    """Reset both, `steps` steps side by side, the whole state; then (post > 0) a masked reset of
    every third env, which puts the envs out of step, `post` more steps and the state again."""
    B, S = env.cfg.num_envs, env.cfg.num_servers
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    rng = np.random.default_rng(seed)
    one = step_auto if same_step else step_both
    for k in range(steps):
        one(env, ref, actions(rng, B, S, kw), k)
    mid = compare_state(env, ref)
    if post:
        mask = (np.arange(B) % 3 == 0).astype(np.uint8)
        og = env.reset(mask=torch.from_numpy(mask)).cpu().numpy()
        np.testing.assert_array_equal(og, ref.reset(mask=mask, obs=og.copy()))
        for k in range(post):
            one(env, ref, actions(rng, B, S, kw), steps + k)
        compare_state(env, ref)
    return mid


ALIAS = {"assign_policy": "alias", "action_type": "continuous"}
SPLIT = {"lost_fin_prob": 0.3, "flow_timeout": 0.4}
CYCLE = (3, 2, True, False)  # P, H, wrap, shared
# id: (B, S, config kwargs, VecLoadBalanceEnv kwargs, table, the dynamics kernel expected)
CASES = {
    "group-24x4": (24, 4, {}, {}, CYCLE, GROUP),
    "group-24x8": (24, 8, {}, {}, CYCLE, GROUP),
    "group-12x20": (12, 20, {}, {}, CYCLE, GROUP),
    "env-70x4": (70, 4, {"dyn_mapping": "env"}, {}, CYCLE, ENV_LANE),
    "fused-24x4": (24, 4, {"dyn_mapping": "server", "step_kernel": "fused"}, {}, CYCLE, GROUP),
    "lsq2-24x4": (24, 4, {"assign_policy": "lsq2"}, {}, CYCLE, GROUP),
    "alias-24x4": (24, 4, ALIAS, {}, CYCLE, GROUP),
    "shared-clamped-24x4": (24, 4, {}, {}, (3, 2, False, True), GROUP),
    "lost-fin-24x4": (24, 4, SPLIT, {}, CYCLE, GROUP),
    "lost-fin-pend4-24x4": (24, 4, {**SPLIT, "lost_fin_pending": 4}, {}, CYCLE, GROUP),
    "res-vpp-24x4": (24, 4, {"reservoir_mode": "vpp"}, {}, CYCLE, GROUP),
    "nflow-vpp-24x4": (24, 4, {**SPLIT, "n_flow_on_mode": "vpp"}, {}, CYCLE, GROUP),
    "normalize-24x4": (24, 4, {"normalize_obs": True}, {}, CYCLE, GROUP),
    "flow-stats-24x4": (24, 4, {}, {"flow_stats": True}, CYCLE, GROUP),
}


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_bit_exact(lib, oracle_mod, case):
    """P = 3, H = 2 tables on every dynamics form, policy and state layout: 12 steps, a masked
    reset of every third env, 4 more steps."""
    B, S, kw, env_kw, (P, H, wrap, shared), kern = CASES[case]
    idx = list(CASES).index(case)
    kw = {"seed": 300 + idx, **kw}
    table = make_table(B, S, P, 50 + idx)
    table = table[0] if shared else table
    env, ref = make_pair(oracle_mod, B, S, kw, env_kw, table, H, wrap)
    mid = drive(env, ref, kw, idx)
    if not os.environ.get("LBSIM_DYN_GROUP_LANES"):
        assert lib.load().lbsim_dynamics_kernel(env.handle.h) == kern
    else:
        names = lib.launch_names(env.handle)
        assert names.get(0, "").startswith("dynamics_group") and "<4," in names[0], names
    if case.startswith("fused"):
        assert lib.launch_names(env.handle).get(4, "").startswith("fused_step_kernel"), \
            lib.launch_names(env.handle)
    st = views(bytearray(ref.state_bytes()), ref.cfg)
    assert 0 < int(st["down"].sum()) < B * S and int(mid["dropped"].sum()) > 0
    if env_kw.get("flow_stats"):  # a failing server keeps its accumulators
        want, now, _ = env.handle.server_avail()
        failing = (now != 0) & (want == 0)
        before = env.handle.flow_stats()
        step_both(env, ref, np.zeros((B, S), np.int64), 16)
        after = env.handle.flow_stats()
        assert bool(failing.any()) and int(before[0][failing].max()) > 0
        for x, y in zip(before, after):
            assert torch.equal(x[failing], y[failing])
        assert int((after[0] - before[0]).sum()) > 0  # the servers that stayed up went on counting
    ref.close()
    env.close()


@gpu
def test_four_lane_groups_bit_exact():
    """LBSIM_DYN_GROUP_LANES=4: the headline 4-lane groups, 16 envs per wave, the second wave
    partial (the setting is read once per process, so a child runs the case)."""
    parity.run_cases_in_child("test_server_avail.py", ["test_bit_exact[group-24x4]"],
                              {"LBSIM_DYN_GROUP_LANES": "4"})


@gpu
def test_cluster_sizes(lib, oracle_mod):
    """P = 1: sample_cluster_sizes, the first n[b] servers of env b up; the absent servers are
    zero rows from the first step on."""
    B, S = 24, 8
    kw = {"seed": 21}
    n = sample_cluster_sizes(B, S, 1, seed=2)
    up = (np.arange(S)[None, :] < n.numpy()[:, None]).astype(np.uint8)
    env, ref = make_pair(oracle_mod, B, S, kw)
    env.set_cluster_sizes(n)
    ref.set_table(up[:, None, :])
    drive(env, ref, kw, 5)
    obs, _, _, _ = env.step(torch.zeros((B, S), dtype=torch.int64))
    ref.step(np.zeros((B, S), np.int64))
    assert len(set(n.tolist())) > 3
    assert not obs.cpu().numpy()[up == 0].any()
    np.testing.assert_array_equal(env.servers_up().cpu().numpy(), up != 0)
    ref.close()
    env.close()


@gpu
@pytest.mark.parametrize("mode", ["same_step", "next_step"])
def test_episode_ends(lib, oracle_mod, mode):
    """max_steps = 6 over three episode ends: a reset brings every server up and the first step
    of the episode applies phase 0; under next-step auto-reset the launch that resets an env
    leaves it alone."""
    B, S, (P, H, wrap, _) = 24, 4, CYCLE
    kw = {"seed": 31, "max_steps": 6}
    table = make_table(B, S, P, 77)
    env, ref = make_pair(oracle_mod, B, S, kw, {"autoreset": True, "autoreset_mode": mode},
                         table, H, wrap)
    assert bool(ref.cfg.next_step_reset) == (mode == "next_step")
    drive(env, ref, kw, 9, steps=21, post=0, same_step=mode == "same_step")
    assert int(views(bytearray(ref.state_bytes()), ref.cfg)["episode"].min()) >= 3
    want, now, phase = (x.cpu().numpy() for x in env.handle.server_avail())
    rw, rn, rp = ref.want_all()
    np.testing.assert_array_equal(want != 0, rw)
    np.testing.assert_array_equal(now != 0, rn)
    np.testing.assert_array_equal(phase, rp)
    ref.close()
    env.close()


@gpu
def test_beside_a_rate_schedule(lib, oracle_mod):
    """A per-env server-rate schedule of other P and H beside the availability table: the
    reference is the chained one-env oracles of tests/test_rate_schedule.py, each edited by the
    rule before its step."""
    from marllb_amd.env import VecLoadBalanceEnv, make_config
    from tests.test_rate_schedule import ScheduledOracles, make_schedule
    B, S, (P, H, wrap, _) = 12, 4, CYCLE
    kw = {"seed": 41}
    _, srv = make_schedule(B, S, 2, 17)
    table = make_table(B, S, P, 78)

    class Chain(ScheduledOracles):
        def _make(self, b, ph):
            cfg = ref_config(make_config(1, self.S, env_id_offset=b,
                                         server_rates=self.srv[b, ph].tolist(), **self.kw))
            return self.mod.OracleEnv(cfg)

    env = VecLoadBalanceEnv(B, S, device="cuda:0", server_availability=True, autoreset=False, **kw)
    env.set_rate_schedule(server=srv, steps_per_phase=3)
    env.set_server_availability(table, steps_per_phase=H, wrap=wrap)
    ref = AvailRef(Chain(oracle_mod, B, S, kw, None, srv, 3, True), ref_config(env.cfg), table, H,
                   wrap)
    drive(env, ref, kw, 13)
    assert ref.inner.handoffs > B
    ref.close()
    env.close()


@gpu
def test_installed_and_cleared_mid_run(lib, oracle_mod):
    """No table for 4 steps, a table installed for 6, cleared for 4: the clear brings every
    server up at the next step.  And a run under an all-ones table equals the run with no table
    bit for bit."""
    B, S, (P, H, wrap, _) = 24, 4, CYCLE
    kw = {"seed": 51}
    env, ref = make_pair(oracle_mod, B, S, kw)
    ones, _ = make_pair(oracle_mod, B, S, kw)
    ones.set_server_availability(np.ones((B, P, S), np.uint8), steps_per_phase=H)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    ones.reset()
    rng = np.random.default_rng(8)
    table = make_table(B, S, P, 79)
    for k in range(14):
        if k == 4:
            assert ones.get_state() == env.get_state()
            env.set_server_availability(table, steps_per_phase=H, wrap=wrap)
            ref.set_table(table, H, wrap)
        if k == 10:
            assert not env.servers_up().all()
            env.clear_server_availability()
            ref.set_table(None)
        a = actions(rng, B, S, kw)
        step_both(env, ref, a, k)
        if k < 4:
            oo, ro, do, _ = ones.step(torch.from_numpy(a))
            np.testing.assert_array_equal(oo.cpu().numpy(), env._last_obs.cpu().numpy())
        if k == 10:
            assert bool(env.servers_up().all())
    compare_state(env, ref)
    for e in (env, ones):
        e.close()
    ref.close()


@gpu
def test_graph_replay(lib):
    """One captured step replayed equals eager stepping; a table of the same P written between
    replays is seen without a new capture."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, (P, H, wrap, _) = 24, 4, CYCLE
    t0, t1 = make_table(B, S, P, 61), make_table(B, S, P, 62)
    eager = VecLoadBalanceEnv(B, S, device="cuda:0", seed=8, max_steps=5, server_availability=True)
    graph = VecLoadBalanceEnv(B, S, device="cuda:0", seed=8, max_steps=5, graph_mode=True,
                              server_availability=True)
    for e in (eager, graph):
        e.set_server_availability(t0, steps_per_phase=H)
        e.reset()
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1)
    acts = [torch.randint(0, 3, (B, S), device="cuda:0", generator=gen) for _ in range(13)]
    a_static = acts[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up step (eager, graph_mode buffers)
        graph.step(a_static)
    torch.cuda.current_stream().wait_stream(side)
    eager.step(acts[0])
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):  # the capture records the step, it does not run it
        obs, rew, done, info = graph.step(a_static)
    for k in range(1, 13):
        if k == 7:  # after six replays: a new table of the same shape, no new capture
            for e in (eager, graph):
                e.set_server_availability(t1, steps_per_phase=H)
        a_static.copy_(acts[k])
        cg.replay()
        eo, er, ed, _ = eager.step(acts[k])
        assert torch.equal(obs, eo), k
        assert torch.equal(rew, er) and torch.equal(done, ed), k
    assert graph.get_state() == eager.get_state()
    assert torch.equal(graph.servers_up(), eager.servers_up())
    assert not bool(eager.servers_up().all())
    eager.close()
    graph.close()


@gpu
def test_shard_invariance(lib):
    """Two uneven shards, each with env_id_offset = lo and its own rows of the table, together
    equal the whole batch."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, (P, H, wrap, _) = 50, 4, CYCLE
    table = make_table(B, S, P, 63)
    bounds = [0, 19, B]
    full = VecLoadBalanceEnv(B, S, device="cuda:0", seed=9, autoreset=False,
                             server_availability=True)
    full.set_server_availability(table, steps_per_phase=H)
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        e = VecLoadBalanceEnv(hi - lo, S, device="cuda:0", seed=9, autoreset=False,
                              env_id_offset=lo, server_availability=True)
        e.set_server_availability(table[lo:hi], steps_per_phase=H)
        parts.append(e)
    assert torch.equal(full.reset(), torch.cat([e.reset() for e in parts]))
    rng = np.random.default_rng(B)
    for _ in range(8):
        a = torch.from_numpy(rng.integers(0, 3, (B, S)))
        fo, fr, fd, _ = full.step(a)
        po = [e.step(a[lo:hi]) for e, lo, hi in zip(parts, bounds[:-1], bounds[1:])]
        assert torch.equal(fo, torch.cat([x[0] for x in po]))
        assert torch.equal(fr, torch.cat([x[1] for x in po]))
        assert torch.equal(fd, torch.cat([x[2] for x in po]))
    assert torch.equal(full.servers_up(), torch.cat([e.servers_up() for e in parts]))
    for e in [full, *parts]:
        e.close()


@gpu
def test_fork_is_reconciled_with_the_slots_table(lib, oracle_mod):
    """restore(snap, src=...) from envs with other servers down: the down flags travel with the
    state, the table stays with the slot, and the next step applies the rule to the difference."""
    B, S, (P, H, wrap, _) = 24, 4, CYCLE
    kw = {"seed": 71}
    table = make_table(B, S, P, 64)
    env, ref = make_pair(oracle_mod, B, S, kw, None, table, H, wrap)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    rng = np.random.default_rng(4)
    for k in range(5):
        step_both(env, ref, actions(rng, B, S, kw), k)
    snap = env.snapshot()
    src = np.roll(np.arange(B), 5).astype(np.int32)
    up_before = env.servers_up().cpu().numpy()
    assert (up_before[src] != up_before).any()
    env.restore(snap, src=torch.from_numpy(src))
    raw = ref.state_bytes()
    buf, off = bytearray(raw), 0
    for name, dt, n in statelayout.sections(B, S, ref.cfg.queue_capacity, False, True):
        nb = np.dtype(dt).itemsize * n
        rows = np.frombuffer(raw, np.uint8, nb, off).reshape(B, -1)
        buf[off:off + nb] = rows[src].tobytes()
        off += nb
    assert off == len(raw)
    ref.load_state(bytes(buf))
    np.testing.assert_array_equal(env.servers_up().cpu().numpy(), up_before[src])
    for k in range(5, 10):
        step_both(env, ref, actions(rng, B, S, kw), k)
    compare_state(env, ref)
    ref.close()
    env.close()


@gpu
def test_servers_up_and_get(lib, oracle_mod):
    """lbsim_get_server_avail on envs out of step, cyclic and clamped: the set the next step will
    enforce, the servers up now, the phase; any output may be NULL."""
    import ctypes
    B, S, P, H = 24, 4, 3, 2
    for wrap in (True, False):
        kw = {"seed": 81}
        table = make_table(B, S, P, 65)
        env, ref = make_pair(oracle_mod, B, S, kw, None, table, H, wrap)
        drive(env, ref, kw, 6, steps=5, post=2)
        want, now, phase = (x.cpu().numpy() for x in env.handle.server_avail())
        rw, rn, rp = ref.want_all()
        np.testing.assert_array_equal(want != 0, rw)
        np.testing.assert_array_equal(now != 0, rn)
        np.testing.assert_array_equal(phase, rp)
        assert len(set(rp.tolist())) > 1
        np.testing.assert_array_equal(env.servers_up().cpu().numpy(), rn)
        np.testing.assert_array_equal(env.availability_phase.cpu().numpy(), rp)
        only = torch.full((B,), -1, dtype=torch.int32, device="cuda:0")
        L = lib.load()
        assert L.lbsim_get_server_avail(env.handle.h, None, None, ctypes.c_void_p(only.data_ptr()),
                                        None) == 0
        assert L.lbsim_get_server_avail(env.handle.h, None, None, None, None) == 0
        torch.cuda.synchronize()
        np.testing.assert_array_equal(only.cpu().numpy(), rp)
        ref.close()
        env.close()


@gpu
def test_multi_agent_facade(lib, oracle_mod):
    """VecMultiAgentLoadBalanceEnv forwards the calls: 4 agents of 4 servers, a rolling restart;
    its state equals a VecLoadBalanceEnv's of the same config under the same actions."""
    from marllb_amd.env import VecLoadBalanceEnv
    from marllb_amd.multi_agent import VecMultiAgentLoadBalanceEnv
    B, A, spa = 6, 4, 4
    S = A * spa
    table = rolling_restart_schedule(S, 5)
    ma = VecMultiAgentLoadBalanceEnv(B, A, spa, device="cuda:0", seed=5, server_availability=True)
    vec = VecLoadBalanceEnv(B, S, device="cuda:0", seed=5, server_availability=True,
                            action_type=ma.vec.action_type, max_steps=int(ma.vec.cfg.max_steps))
    for e in (ma, vec):
        e.set_server_availability(table, steps_per_phase=1, wrap=True)
    ma.reset()
    vec.reset()
    rng = np.random.default_rng(2)
    for k in range(6):
        a = rng.integers(0, 3, (B, A, spa))
        ma.step(torch.from_numpy(a))
        vec.step(torch.from_numpy(a.reshape(B, S)))
        up = ma.servers_up().cpu().numpy()
        assert torch.equal(ma.servers_up(), vec.servers_up())
        np.testing.assert_array_equal(up, np.broadcast_to(table.numpy()[k % 5] != 0, (B, S)))
    assert ma.vec.get_state() == vec.get_state()
    ma.clear_server_availability()
    ma.set_cluster_sizes(np.full(B, 7))
    ma.step(torch.from_numpy(rng.integers(0, 3, (B, A, spa))))
    assert int(ma.servers_up().sum()) == 7 * B
    ma.close()
    vec.close()


@gpu
def test_error_paths(lib):
    from marllb_amd.env import Handle, VecLoadBalanceEnv, make_config
    B, S = 8, 4
    up = torch.ones((B, 2, S), dtype=torch.uint8, device="cuda:0")
    h = Handle(make_config(B, S, seed=1), 0)
    with pytest.raises(lib.LbsimError) as e:  # set without enable
        h.set_server_avail(up, rows=B, phases=2)
    assert e.value.code == lib.ENOTSUP
    with pytest.raises(lib.LbsimError) as e:
        h.server_avail()
    assert e.value.code == lib.ENOTSUP
    size0 = h.state_size()
    h.enable_server_avail()
    h.enable_server_avail()  # a second call is a no-op
    assert h.state_size() == size0 + 4 * B * S  # the down section, as a fail_prob handle's
    hf = Handle(make_config(B, S, seed=1, fail_prob=0.1), 0)
    assert hf.state_size() == h.state_size()
    with pytest.raises(lib.LbsimError) as e:  # random failures beside a script
        hf.enable_server_avail()
    assert e.value.code == lib.ENOTSUP
    hf.close()
    with pytest.raises(lib.LbsimError) as e:
        h.set_server_avail(up, rows=2, phases=2)
    assert e.value.code == lib.ESHAPE
    for P in (0, 4097):
        with pytest.raises(ValueError):
            h.set_server_avail(up, rows=1, phases=P)
    with pytest.raises(ValueError):
        h.set_server_avail(up, rows=B, phases=2, steps_per_phase=0)
    with pytest.raises(ValueError):
        h.set_server_avail(None, rows=B, phases=2)
    big = Handle(make_config(300000, 2, seed=1), 0)
    big.enable_server_avail()
    with pytest.raises(lib.LbsimError) as e:  # 300000 * 4096 * 2 entries
        big.set_server_avail(up, rows=1, phases=4096)
    assert e.value.code == lib.ENOMEM
    big.close()
    h.set_server_avail(up, rows=B, phases=2)
    h.close()
    env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=1)
    env.reset()
    with pytest.raises(ValueError):  # enable after the first reset
        env.handle.enable_server_avail()
    env.close()
    env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=1, server_availability=True)
    for bad in (np.ones((B, 2, S + 1)), np.ones((B + 1, 2, S)), np.ones(S), np.ones((2, 0, S))):
        with pytest.raises(ValueError):
            env.set_server_availability(bad)
    with pytest.raises(ValueError):
        env.set_cluster_sizes(np.ones(B + 1, np.int64))
    env.close()


@gpu
def test_single_env_facade(lib):
    """LoadBalanceEnv(server_availability=True) forwards the calls to its one env: a rolling
    restart, a cluster size, and the clear."""
    from marllb_amd.env import LoadBalanceEnv
    S = 4
    env = LoadBalanceEnv(num_servers=S, seed=3, step_interval=0, server_availability=True)
    env.set_server_availability(rolling_restart_schedule(S, 3).numpy())
    env.reset()
    assert env.servers_up() == [True] * S
    a = np.zeros(S, np.int64)
    for k in range(4):  # the step after k completed steps runs at phase k % 3
        obs = np.asarray(env.step(a)[0]).reshape(S, 11)
        assert env.servers_up() == [s != k % 3 or k % 3 == 0 for s in range(S)], k
        if k % 3:
            assert not obs[k % 3].any() and obs[0].any()
    env.set_cluster_size(2)
    env.step(a)
    assert env.servers_up() == [True, True, False, False]
    env.clear_server_availability()
    env.step(a)
    assert env.servers_up() == [True] * S
    with pytest.raises(ValueError):
        env.set_server_availability(np.ones((1, 2, S)))
    env.close()
