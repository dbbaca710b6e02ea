"""Ground-truth server state: lbsim_ground_truth and what sits on it.

The reference is tests/truth_ref.ground_truth, numpy written from the rule's table over a parsed
state snapshot and the existing getters.

Not gpu: the reference against the independent simulators' queues (oracle states for the plain
cases of test_flowsim_ref.CASES, states laid out from WorkerSim's and CrossSim's queues for the
other two), what the device scenarios reach (on the oracle and the simulators alone), the rule's
header compiled as host C++ under the address and undefined-behaviour sanitizers against a brute
force, and the one-env facade's defaults.  gpu: ground_truth() equals the reference bit for bit
after the reset and after every step, on every kind of handle.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from marllb_amd import build
from marllb_amd.env import make_config
from marllb_amd.randomize import schedule_phase
from tests import crosstraffic_ref as cr
from tests import statelayout
from tests import test_cross_traffic as ct
from tests import test_flowsim_ref as fr
from tests import test_server_workers as wsw
from tests import truth_ref as tr
from tests.parity import lib  # noqa: F401  (the fixture: fails a gpu test run without a device)

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = fr.CASES
gpu = pytest.mark.gpu
F32 = np.float32
B = fr.GPU_B  # 67: B * S = 335 at S = 5 leaves a partial last block
STEPS = 12


def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def seconds(us):
    return F32(max(0, int(us))) * F32(1e-6)


# ------------------------------------------------------------------ not gpu: against the simulators

def state_of_queues(queues, base, Q, rng, hidden=False):
    """A state dict laid out as the handle's from the simulators' queues (queues[b][s]: entries
    whose [0] is tc in absolute us, [2] the hidden flag), times relative to `base[b]`, every ring
    at a random head with poison in the slots that are not live."""
    nB, S = len(queues), len(queues[0])
    hc = np.zeros((nB, S), np.uint32)
    ring = np.full((nB, S, Q, 2), 0x7F0F0F0F, np.int32)
    lost = np.zeros((nB, S), np.int32)
    for b in range(nB):
        for s in range(S):
            q = queues[b][s]
            head = int(rng.integers(Q))
            hc[b, s] = head | (len(q) << 16) | (0x8000 if rng.integers(2) else 0)
            for i, e in enumerate(q):
                ring[b, s, (head + i) % Q] = (e[0] - base[b], 0)
            lost[b, s] = -sum(1 for e in q if hidden and e[2])
    d = {"hc": hc.reshape(-1), "ring": ring.reshape(-1)}
    if hidden:
        d["lost_on"] = lost.reshape(-1).view(np.uint32)
    return d


@pytest.mark.parametrize("case", list(CASES))
def test_reference_on_oracle_states(oracle_mod, case):
    """Plain handles: on the oracle's states n_total is the length of the independent simulator's
    queue, backlog its largest tc, and with one worker the wait is the backlog."""
    from tests.flowsim_ref import FlowSim
    nB = fr.HOST_B
    S, kw = fr.config_kwargs(case)
    cfg = make_config(nB, S, **kw)
    Q, dt = cfg.queue_capacity, int(round(cfg.step_interval * 1e6))
    sims = [FlowSim(kw["seed"], cfg.env_id_offset + b, S, Q, kw.get("assign_policy", "sed"),
                    cfg.arrival_rate, [cfg.server_rate[s] for s in range(S)],
                    dt=cfg.step_interval, warmup_steps=cfg.warmup_steps, trace=kw.get("trace"))
            for b in range(nB)]
    back = fr.OracleBackend(oracle_mod, cfg, kw)
    mu = np.tile(np.array([cfg.server_rate[s] for s in range(S)], F32), (nB, 1))
    seen = {"flows": 0}

    def check():
        d = statelayout.parse_cfg(back.ora.state_bytes(), cfg)
        t = tr.ground_truth(d, nB, S, Q, mu)
        for b in range(nB):
            base = sims[b].step_no * dt
            for s in range(S):
                q = sims[b].queues[s]
                assert t[b, s, 0] == len(q), ("n_total", b, s)
                want = seconds(max(tc for tc, _ in q) - base) if q else F32(0)
                assert t[b, s, 5] == want, ("backlog", b, s)
                assert t[b, s, 4] == want, ("wait at c = 1", b, s)
                assert t[b, s, 2] == min(len(q), 1) == t[b, s, 3]
                seen["flows"] += len(q)
        assert (t[..., 1] == 0).all() and (t[..., 6] == 1).all()
        np.testing.assert_array_equal(t[..., 7], mu)
        assert (t >= 0).all()

    acts = fr.actions_of(case, nB)
    back.reset(None)
    for m in sims:
        m.reset()
    check()
    for k in range(fr.STEPS):
        if k == fr.RESET_AT:  # the masked reset of every third env: a second episode
            mask = np.arange(nB) % 3 == 0
            back.reset(mask.astype(np.uint8))
            for b in np.flatnonzero(mask):
                sims[b].reset()
            check()
        back.step(acts[k])
        wts = fr.weights_of(acts[k], kw)
        for b, m in enumerate(sims):
            m.step(wts[b])
        check()
    assert seen["flows"] > nB
    back.ora.close()


@pytest.mark.parametrize("case", list(CASES))
def test_reference_against_explicit_workers(case):
    """Multi-worker servers: the wait is WorkerSim's explicit earliest-free-worker time (formulation
    (a), per-worker free times), on states laid out from its queues."""
    nB = fr.HOST_B
    S, kw = fr.config_kwargs(case)
    cfg = make_config(nB, S, **kw)
    Q, dt = cfg.queue_capacity, int(round(cfg.step_interval * 1e6))
    workers = wsw.workers_of(case, nB)
    mus = wsw.rates_of(case, nB, workers)
    sims = wsw.make_sims(case, nB, workers, mus, explicit=True)
    rng = np.random.default_rng(5)
    acts = fr.actions_of(case, nB)
    seen = {"multi": 0, "busy_all": 0}

    def check():
        base = [m.step_no * dt for m in sims]
        queues = [m.queues for m in sims]
        d = state_of_queues(queues, base, Q, rng)
        t = tr.ground_truth(d, nB, S, Q, mus, workers)
        for b, m in enumerate(sims):
            for s in range(S):
                q, c = m.queues[s], int(workers[b, s])
                assert t[b, s, 0] == len(q)
                assert t[b, s, 2] == min(len(q), c)
                assert t[b, s, 3] == F32(min(len(q), c)) / F32(c)
                assert t[b, s, 4] == seconds(min(m.free[s]) - base[b]), ("wait", b, s)
                assert t[b, s, 5] == (seconds(max(e[0] for e in q) - base[b]) if q else 0)
                assert t[b, s, 7] == F32(c) * mus[b, s]
                seen["multi"] += c > 1 and len(q) > c
                seen["busy_all"] += len(q) >= c

    for m in sims:
        m.reset()
    check()
    for k in range(fr.STEPS):
        wts = fr.weights_of(acts[k], kw)
        for b, m in enumerate(sims):
            m.step(wts[b])
        check()
    assert seen["busy_all"] > 0
    if case in ("s4-q64-deep", "s3-lsq-q6-overload", "s1-q3-drops"):
        assert seen["multi"] > 0  # a wait read from a position that is neither first nor last


@pytest.mark.parametrize("case", list(CASES))
def test_reference_counts_the_hidden_entries(case):
    """Cross traffic: n_hidden is the number of hidden entries in crosstraffic_ref's queues, and
    n_total counts them with the visible ones."""
    nB = fr.HOST_B
    S, kw = fr.config_kwargs(case)
    cfg = make_config(nB, S, **kw)
    Q, dt = cfg.queue_capacity, int(round(cfg.step_interval * 1e6))
    share, w = ct.cross_params(case, nB)
    sims = [cr.CrossSim(kw["seed"], cfg.env_id_offset + b, S, Q, kw.get("assign_policy", "sed"),
                        cfg.arrival_rate, [cfg.server_rate[s] for s in range(S)],
                        dt=cfg.step_interval, warmup_steps=cfg.warmup_steps, trace=kw.get("trace"),
                        share=share[b], weights=w[b]) for b in range(nB)]
    mu = np.tile(np.array([cfg.server_rate[s] for s in range(S)], F32), (nB, 1))
    rng = np.random.default_rng(6)
    acts = fr.actions_of(case, nB)
    hidden_seen = 0
    for m in sims:
        m.reset()
    for k in range(fr.STEPS):
        wts = fr.weights_of(acts[k], kw)
        for b, m in enumerate(sims):
            m.step(wts[b])
        d = state_of_queues([m.queues for m in sims], [m.step_no * dt for m in sims], Q, rng,
                            hidden=True)
        t = tr.ground_truth(d, nB, S, Q, mu, hidden=True)
        hid = np.array([m.hidden_in_flight() for m in sims])
        vis = np.array([m.in_flight() for m in sims])
        np.testing.assert_array_equal(t[..., 1], hid.astype(F32))
        np.testing.assert_array_equal(t[..., 0], (hid + vis).astype(F32))
        assert tr.reach(d, nB, S, Q, hidden=True)["hidden"] == int((hid > 0).sum())
        hidden_seen += int(hid.sum())
    assert hidden_seen > 0


# ------------------------------------------------------------------ the device scenarios

SHAPES = [(S, Q) for S in (1, 5, 16) for Q in (3, 8, 32)]
SEED = 8200


def scenario_kw(S, Q, **extra):
    """Load 0.95 on equal servers, ten arrivals per server and step: queues of every depth."""
    return {"queue_capacity": Q, "arrival_rate": 40.0 * S, "load": 0.95, "warmup_steps": 2,
            "seed": SEED + 16 * S + Q, **extra}


def scenario_actions(S, steps=STEPS, nB=B):
    rng = np.random.default_rng(S)
    return [rng.integers(0, 3, (nB, S)).astype(np.int64) for _ in range(steps)]


# What each plain shape must reach over the reset and its 12 steps (checked on the oracle below,
# and again on the device, whose states are the oracle's): an empty server and a queue that wraps
# its ring at every shape, a full server where Q <= 8 (rings of 32 do not fill at this load).
EXPECT = {(S, Q): {"empty", "wraps"} | ({"full"} if Q <= 8 else set()) for S, Q in SHAPES}


def add_reach(total, r):
    for k, v in r.items():
        total[k] = total.get(k, 0) + v
    return total


@pytest.mark.parametrize("S,Q", SHAPES)
def test_plain_scenario_reaches_on_the_oracle(oracle_mod, S, Q):
    """The plain device scenario on the oracle alone: the shapes together reach an empty server, a
    full one and a queue that wraps its ring; each shape what EXPECT says."""
    kw = scenario_kw(S, Q)
    cfg = make_config(B, S, **kw)
    ora = oracle_mod.OracleEnv(cfg, threads=4)
    ora.reset()
    total = add_reach({}, tr.reach(statelayout.parse_cfg(ora.state_bytes(), cfg), B, S, Q))
    for a in scenario_actions(S):
        ora.step(a)
        add_reach(total, tr.reach(statelayout.parse_cfg(ora.state_bytes(), cfg), B, S, Q))
    ora.close()
    print(f"REACH S={S} Q={Q}: {total}")
    for k in EXPECT[(S, Q)]:
        assert total[k] > 0, (k, total)


def test_failures_reach_a_down_server_on_the_oracle(oracle_mod):
    S, Q = 5, 8
    kw = scenario_kw(S, Q, fail_prob=0.15, recover_prob=0.4)
    cfg = make_config(B, S, **kw)
    ora = oracle_mod.OracleEnv(cfg, threads=4)
    ora.reset()
    total = {}
    for a in scenario_actions(S):
        ora.step(a)
        d = statelayout.parse_cfg(ora.state_bytes(), cfg)
        add_reach(total, tr.reach(d, B, S, Q))
        t = tr.ground_truth(d, B, S, Q, np.ones((B, S), F32))
        down = d["down"].reshape(B, S) != 0
        assert (t[down][:, :6] == 0).all() and (t[down][:, 6] == 0).all()
        assert (t[~down][:, 6] == 1).all()
    ora.close()
    assert total["down"] > 0 and total["wraps"] > 0


W_S, W_Q = 5, 8


def scenario_workers(nB=B, S=W_S):
    """Worker counts cycling 1, 2, 3, 4 over envs and servers, and the rates divided by them."""
    w = (1 + (np.arange(nB)[:, None] + np.arange(S)[None, :]) % 4).astype(np.int32)
    cfg = make_config(nB, S, **scenario_kw(S, W_Q))
    mu = (F32(cfg.server_rate[0]) / w.astype(F32)).astype(F32)
    return w, mu


def test_workers_and_cross_scenario_reaches_on_the_simulators():
    """The workers plus cross-traffic scenario on CrossWorkerSim alone (12 envs of the 67): a wait
    read from position n - c > 0 with c > 1, a full server, an empty one, hidden flows."""
    nB, S, Q = 12, W_S, W_Q
    kw = scenario_kw(S, Q)
    cfg = make_config(nB, S, **kw)
    w, mu = scenario_workers(nB)
    sims = [wsw.wr.CrossWorkerSim(kw["seed"], b, S, Q, "sed", cfg.arrival_rate,
                                  [float(x) for x in mu[b]], dt=cfg.step_interval,
                                  warmup_steps=cfg.warmup_steps, workers=w[b], share=0.5,
                                  weights=np.ones(S, F32)) for b in range(nB)]
    rng = np.random.default_rng(7)
    dt = int(round(cfg.step_interval * 1e6))
    total = {}
    for m in sims:
        m.reset()
    for a in scenario_actions(S, nB=nB):
        wts = fr.weights_of(a, kw)
        for b, m in enumerate(sims):
            m.step(wts[b])
        d = state_of_queues([m.queues for m in sims], [m.step_no * dt for m in sims], Q, rng,
                            hidden=True)
        add_reach(total, tr.reach(d, nB, S, Q, w, hidden=True))
    print(f"REACH workers + cross: {total}")
    for k in ("multi_wait", "full", "empty", "hidden"):
        assert total[k] > 0, (k, total)


# ------------------------------------------------------------------ not gpu: the header, the facade

def test_rule_against_a_brute_force(tmp_path):
    """tests/truth_probe.cpp: csrc/lbsim_truth.h on a plain array, for every c in 1..64, Q in {3,
    8, 9, 32, 64}, every n in 0..Q and every head, under the address and undefined-behaviour
    sanitizers."""
    exe = str(tmp_path / "truth_probe")
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "truth_probe.cpp")], check=True)
    for seed in (1, 2):
        r = subprocess.run([exe, str(seed)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        rows = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert [(c, q) for c, q, *_ in rows] == [(c, q) for c in range(1, 65)
                                                 for q in (3, 8, 9, 32, 64)]
        for c, q, n_rows, wrapped, two, multi in rows:
            assert n_rows == (q + 1) * q and wrapped == q * (q - 1) // 2
            # two reads exactly where 1 < c <= n
            assert two == multi == (q * max(0, q - c + 1) if c > 1 else 0)


def test_facade_defaults_and_abi():
    """ground_truth_source="reference" (the default) leaves the one-env facade as it was: a
    (S, 14) space, (S, 11) arrays, the reference plumbing's values; a bad value raises, and so
    does "sim" where there is no simulator."""
    from marllb_amd import GROUND_TRUTH_COLUMNS, LoadBalanceEnv, _lib
    assert GROUND_TRUTH_COLUMNS == tr.NAMES and len(GROUND_TRUTH_COLUMNS) == tr.COLS
    plain = LoadBalanceEnv(num_servers=3, reference_plumbing=True, seed=11)
    wide = LoadBalanceEnv(num_servers=3, reference_plumbing=True, seed=11, use_ground_truth=True)
    named = LoadBalanceEnv(num_servers=3, reference_plumbing=True, seed=11, use_ground_truth=True,
                           ground_truth_source="reference")
    assert wide.observation_space.shape == (3, 14) and plain.observation_space.shape == (3, 11)
    o = [e.reset() for e in (plain, wide, named)]
    assert o[0].shape == (3, 11) and o[0].dtype == np.float32
    for x in o[1:]:
        assert bits(x).tolist() == bits(o[0]).tolist()
    for _ in range(3):
        r = [e.step(np.zeros(3, np.int64)) for e in (plain, wide, named)]
        for x in r[1:]:
            assert x[0].shape == (3, 11) and bits(x[0]).tolist() == bits(r[0][0]).tolist()
            assert x[1] == r[0][1]
    with pytest.raises(ValueError):
        LoadBalanceEnv(num_servers=3, reference_plumbing=True, ground_truth_source="oracle")
    with pytest.raises(ValueError):
        LoadBalanceEnv(num_servers=3, reference_plumbing=True, use_ground_truth=True,
                       ground_truth_source="sim")
    with pytest.raises(ValueError):
        LoadBalanceEnv(num_servers=3, use_shm=True, shm_name="lbsim-no-such-region",
                       use_ground_truth=True, ground_truth_source="sim")
    with pytest.raises(RuntimeError):
        plain.ground_truth()
    header = open(os.path.join(os.path.dirname(HERE), "include", "lbsim.h")).read()
    assert "int lbsim_ground_truth(lbsim_t* h, float* truth_out, void* stream);" in header
    assert "#define LBSIM_TRUTH_COLS 8" in header and "#define LBSIM_ABI_VERSION 10 " in header
    assert len(_lib._SIGNATURES["lbsim_ground_truth"][1]) == 3
    assert _lib.load().lbsim_ground_truth_cols() == 8
    assert _lib.load().lbsim_ground_truth(None, None, None) == _lib.EINVAL


# ------------------------------------------------------------------ the device

def make_env(S, Q, nB=B, **extra):
    from marllb_amd.env import VecLoadBalanceEnv
    kw = scenario_kw(S, Q)
    kw.update(extra)
    kw.setdefault("autoreset", False)
    return VecLoadBalanceEnv(nB, S, device="cuda:0", **kw)


class Checker:
    """ground_truth() against the reference, bit for bit; collects what the states reach."""

    def __init__(self, env, cross=False, workers=False, getter_rates=True):
        self.env, self.opt = env, dict(cross=cross, workers=workers, getter_rates=getter_rates)
        self.total, self.calls = {}, 0

    def __call__(self, who=""):
        env = self.env
        c = env.cfg
        got = env.ground_truth().cpu().numpy()  # first: the getters below may allocate rate arrays
        want, d = tr.of_env(env, **self.opt)
        assert got.shape == want.shape == (c.num_envs, c.num_servers, 8) and got.dtype == F32
        bad = np.argwhere(bits(got) != bits(want))
        assert len(bad) == 0, (who, bad[:5].tolist(), got[tuple(bad[0][:2])], want[tuple(bad[0][:2])])
        assert np.array_equal(bits(got), bits(want))
        assert (got >= 0).all()
        w = env.get_server_workers().cpu().numpy() if self.opt["workers"] else None
        add_reach(self.total, tr.reach(d, c.num_envs, c.num_servers, c.queue_capacity, w,
                                       hidden=self.opt["cross"]))
        self.calls += 1
        return got


def run_scenario(env, chk, steps=STEPS, before_step=None):
    import torch
    S = env.num_servers
    env.reset()
    chk("reset")
    for k, a in enumerate(scenario_actions(S, steps, env.num_envs)):
        if before_step is not None:
            before_step(k)
        env.step(torch.from_numpy(a))
        chk(f"step {k}")
    return chk


MAPPED = [(S, Q, m) for S, Q in SHAPES for m in ("auto", "env", "server")]


@gpu
@pytest.mark.parametrize("S,Q,mapping", MAPPED)
def test_default_handles(lib, S, Q, mapping):
    """Default handles under every dyn_mapping: the rates come from the config (no rate array is
    ever allocated), every optional array is absent."""
    env = make_env(S, Q, dyn_mapping=mapping)
    chk = run_scenario(env, Checker(env, getter_rates=False))
    for k in EXPECT[(S, Q)]:
        assert chk.total[k] > 0, (k, chk.total)
    env.close()


@gpu
def test_server_workers(lib):
    w, mu = scenario_workers()
    env = make_env(W_S, W_Q, server_workers=w)
    env.set_rates(None, mu)
    chk = run_scenario(env, Checker(env, workers=True))
    assert chk.total["multi_wait"] > 0 and chk.total["full"] > 0, chk.total
    got = env.ground_truth().cpu().numpy()
    np.testing.assert_array_equal(got[..., 7], w.astype(F32) * mu)
    env.close()


@gpu
def test_cross_traffic_at_half_share(lib):
    env = make_env(W_S, W_Q, cross_traffic=True)
    env.set_cross_traffic(0.5)
    chk = run_scenario(env, Checker(env, cross=True))
    assert chk.total["hidden"] > 0, chk.total
    env.close()


@gpu
def test_workers_with_cross_traffic(lib):
    w, mu = scenario_workers()
    env = make_env(W_S, W_Q, server_workers=w, cross_traffic=True)
    env.set_rates(None, mu)
    env.set_cross_traffic(0.5)
    chk = run_scenario(env, Checker(env, cross=True, workers=True))
    for k in ("multi_wait", "full", "empty", "hidden"):
        assert chk.total[k] > 0, (k, chk.total)
    env.close()


@gpu
def test_scripted_outage(lib):
    """A (P, S) availability table: `up` is lbsim_get_server_avail's up_now after every step, a
    down server's columns 0-5 are zero, and some server is down."""
    S, Q = W_S, W_Q
    env = make_env(S, Q, server_availability=True)
    table = np.ones((4, S), np.uint8)
    table[1, 1] = table[2, 1] = table[2, 3] = 0
    env.set_server_availability(table, steps_per_phase=1, wrap=True)
    chk = Checker(env)
    seen = {"down": 0}

    def after():
        got = chk()
        up = env.servers_up().cpu().numpy()
        np.testing.assert_array_equal(got[..., 6], up.astype(F32))
        assert (got[~up][:, :6] == 0).all()
        seen["down"] += int((~up).sum())

    import torch
    env.reset()
    after()
    for a in scenario_actions(S):
        env.step(torch.from_numpy(a))
        after()
    assert seen["down"] > 0 and chk.total["down"] == seen["down"]
    env.close()


@gpu
def test_random_failures(lib):
    env = make_env(W_S, W_Q, fail_prob=0.15, recover_prob=0.4)
    chk = run_scenario(env, Checker(env, getter_rates=False))
    assert chk.total["down"] > 0 and chk.total["wraps"] > 0, chk.total
    env.close()


def rate_tables(S, P, seed):
    rng = np.random.default_rng(seed)
    per_env = rng.uniform(30.0, 90.0, (B, S)).astype(F32)
    sched = rng.uniform(30.0, 90.0, (B, P, S)).astype(F32)
    return per_env, sched


@gpu
@pytest.mark.parametrize("wrap", [True, False])
def test_per_env_rates_and_a_rate_schedule(lib, wrap):
    """Per-env rates, then a per-env server schedule of 3 phases held 2 steps each: capacity is the
    table's row at schedule_phase of the steps the env has completed."""
    import torch
    S, Q, P, H = W_S, W_Q, 3, 2
    per_env, sched = rate_tables(S, P, 31)
    env = make_env(S, Q)
    env.set_rates(None, per_env)
    chk = Checker(env)
    env.reset()
    np.testing.assert_array_equal(chk("per-env rates")[..., 7], per_env)
    acts = scenario_actions(S)
    env.step(torch.from_numpy(acts[0]))
    np.testing.assert_array_equal(chk()[..., 7], per_env)
    env.set_rate_schedule(None, sched, steps_per_phase=H, wrap=wrap)
    phases = set()
    for k in range(1, STEPS):
        ph = int(schedule_phase(k, P, H, wrap))
        np.testing.assert_array_equal(chk(f"before step {k}")[..., 7], sched[:, ph])
        phases.add(ph)
        env.step(torch.from_numpy(acts[k]))
    assert phases == {0, 1, 2}
    env.clear_rate_schedule()
    cfg_mu = F32(env.cfg.server_rate[0])
    assert (chk("cleared")[..., 7] == cfg_mu).all()
    env.close()


@gpu
def test_lost_fin_handle(lib):
    """Lost-FIN with n_flow_on_mode="vpp": the handle's lost_on words count lost flows, not hidden
    ones, and n_hidden stays 0."""
    env = make_env(W_S, W_Q, lost_fin_prob=0.3, flow_timeout=0.4, n_flow_on_mode="vpp",
                   lost_fin_pending=64)
    chk = Checker(env, getter_rates=False)
    run_scenario(env, chk)
    d = tr.parse_env(env)
    assert d["lost_on"].sum() > 0
    assert (env.ground_truth()[..., 1] == 0).all()
    env.close()


@gpu
def test_trace_handle(lib):
    from marllb_amd import trace
    S, Q = 8, 8
    env = make_env(S, Q, trace=trace.synthetic(37, 300.0, seed=7), server_rates=[40.0] * S,
                   step_interval=0.1)
    chk = run_scenario(env, Checker(env, getter_rates=False))
    assert chk.total["empty"] > 0 and chk.total["empty"] < chk.calls * B * S
    env.close()


@gpu
def test_next_step_auto_reset_across_an_episode_end(lib):
    """max_steps = 3 with next-step auto-reset and a rate schedule: after the episode's last step
    the rows describe its final state at the rate of phase 0 (the next launch resets the env), and
    after that launch the new episode."""
    import torch
    S, Q, P = W_S, W_Q, 3
    _, sched = rate_tables(S, P, 32)
    env = make_env(S, Q, autoreset=True, autoreset_mode="next_step", max_steps=3)
    env.set_rate_schedule(None, sched, steps_per_phase=1, wrap=False)
    chk = Checker(env)
    env.reset()
    chk("reset")
    for k, a in enumerate(scenario_actions(S, 9)):
        _, _, done, _ = env.step(torch.from_numpy(a))
        got = chk(f"step {k}")
        completed = (k % 4) + 1 if k % 4 != 3 else 0  # steps of the episode behind each env
        assert bool(done.all()) == (completed == 3)
        want_phase = 0 if completed in (0, 3) else completed
        np.testing.assert_array_equal(got[..., 7], sched[:, want_phase])
    env.close()


@gpu
def test_same_step_auto_reset_describes_the_new_episode(lib):
    import torch
    S, Q = W_S, W_Q
    env = make_env(S, Q, autoreset=True, max_steps=2)
    twin = make_env(S, Q)
    chk = Checker(env, getter_rates=False)
    env.reset()
    twin.reset()
    first = twin.ground_truth().cpu().numpy()
    acts = scenario_actions(S, 2)
    env.step(torch.from_numpy(acts[0]))
    chk()
    _, _, done, _ = env.step(torch.from_numpy(acts[1]))
    assert bool(done.all())
    got = chk("after the auto-reset")
    # the second episode starts as the first did except for its arrivals: every server up, the
    # shapes equal, and the rows are those of the state that reset left
    assert got.shape == first.shape and (got[..., 6] == 1).all()
    env.close()
    twin.close()


@gpu
def test_snapshot_restore_and_fork(lib):
    import torch
    w, mu = scenario_workers()
    env = make_env(W_S, W_Q, server_workers=w, cross_traffic=True)
    env.set_rates(None, mu)
    env.set_cross_traffic(0.5)
    chk = Checker(env, cross=True, workers=True)
    acts = [torch.from_numpy(a) for a in scenario_actions(W_S)]
    env.reset()
    for k in range(4):
        env.step(acts[k])
    at_snap = chk("snapshot").copy()
    snap = env.snapshot()
    for k in range(4, 7):
        env.step(acts[k])
    assert not np.array_equal(chk("moved on"), at_snap)
    env.restore(snap)
    assert np.array_equal(bits(chk("restored")), bits(at_snap))
    src = int(at_snap[..., 0].sum(1).argmax())
    env.restore(snap, src=torch.full((B,), src, dtype=torch.int32))
    forked = chk("forked")
    # the queue's columns are the source's in every env; busy, cpu, the wait and the capacity
    # follow each env's own workers and rates
    for col in (0, 1, 5, 6):
        assert (forked[..., col] == forked[src][None, :, col]).all(), col
    np.testing.assert_array_equal(forked[..., 7], w.astype(F32) * mu)
    env.close()


@gpu
def test_two_uneven_shards(lib):
    import torch
    w, mu = scenario_workers()
    acts = scenario_actions(W_S, 5)

    def run(lo, n):
        env = make_env(W_S, W_Q, nB=n, server_workers=w[lo:lo + n], cross_traffic=True,
                       env_id_offset=lo)
        env.set_rates(None, mu[lo:lo + n])
        env.set_cross_traffic(0.5)
        env.reset()
        out = [env.ground_truth().cpu().numpy()]
        for a in acts:
            env.step(torch.from_numpy(a[lo:lo + n]))
            out.append(env.ground_truth().cpu().numpy())
        env.close()
        return out

    whole = run(0, B)
    lo = 0
    for n in (26, 41):
        for x, y in zip(run(lo, n), whole):
            assert np.array_equal(bits(x), bits(y[lo:lo + n]))
        lo += n
    assert lo == B


@gpu
def test_graph_capture_of_step_plus_ground_truth(lib):
    """One torch.cuda.graph capture of step() plus ground_truth(), replayed three times: each
    replay's rows equal the reference of the state it left, and an eager twin's."""
    import torch
    w, mu = scenario_workers()

    def make(**kw):
        e = make_env(W_S, W_Q, server_workers=w, cross_traffic=True, **kw)
        e.set_rates(None, mu)
        e.set_cross_traffic(0.5)
        e.reset()
        return e

    eager, graph = make(), make(graph_mode=True)
    acts = [torch.from_numpy(a).to("cuda:0") for a in scenario_actions(W_S, 5)]
    a_static = acts[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up (eager, the graph_mode buffers)
        graph.step(a_static)
        graph.ground_truth()
    torch.cuda.current_stream().wait_stream(side)
    eager.step(acts[0])
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        graph.step(a_static)
        truth = graph.ground_truth()
    for k in range(1, 4):
        a_static.copy_(acts[k])
        cg.replay()
        eager.step(acts[k])
        got = truth.cpu().numpy()
        want, _ = tr.of_env(graph, cross=True, workers=True)
        assert np.array_equal(bits(got), bits(want)), k
        assert torch.equal(truth, eager.ground_truth()), k
    eager.close()
    graph.close()


@gpu
def test_one_env_facade(lib):
    from marllb_amd.env import LoadBalanceEnv
    S, Q = 4, 8
    kw = dict(num_servers=S, seed=5, use_ground_truth=True, queue_capacity=Q, arrival_rate=160.0,
              load=0.95, warmup_steps=2, server_workers=[1, 2, 3, 4])
    env = LoadBalanceEnv(ground_truth_source="sim", **kw)
    ref = LoadBalanceEnv(**kw)
    assert env.observation_space.shape == (S, 14)

    def check(o, o_ref):
        assert o.shape == (S, 14) and o.dtype == np.float32 and (o >= 0).all()
        assert o_ref.shape == (S, 11)
        assert np.array_equal(bits(o[:, :11]), bits(o_ref))
        t = env.ground_truth()
        want, _ = tr.of_env(env._vec, workers=True)
        assert t.shape == (S, 8) and np.array_equal(bits(t), bits(want[0]))
        assert np.array_equal(bits(o[:, 11]), bits(t[:, 3]))
        assert np.array_equal(bits(o[:, 12]), bits(t[:, 0] / F32(Q)))
        assert np.array_equal(bits(o[:, 13]), bits(t[:, 2]))
        return t

    check(env.reset(), ref.reset())
    busy = 0
    rng = np.random.default_rng(3)
    for _ in range(8):
        a = rng.integers(0, 3, S)
        (o, r, d, _), (o2, r2, d2, _) = env.step(a), ref.step(a)
        assert r == r2 and d == d2
        busy += int(check(o, o2)[:, 2].sum())
    assert busy > 0
    snap = env.snapshot()
    before = env.ground_truth()
    env.step(np.zeros(S, np.int64))
    o = env.restore(snap)
    assert o.shape == (S, 14) and np.array_equal(bits(env.ground_truth()), bits(before))
    env.close()
    ref.close()


@gpu
def test_multi_agent_true_state(lib):
    import torch
    from marllb_amd.multi_agent import VecMultiAgentLoadBalanceEnv
    A, k, nB = 2, 3, 9
    ma = VecMultiAgentLoadBalanceEnv(nB, num_agents=A, servers_per_agent=k, action_type="discrete",
                                     cross_traffic=True, autoreset=False,
                                     **scenario_kw(A * k, 8))
    ma.set_cross_traffic(0.5)
    ma.reset()
    hidden = 0
    for a in scenario_actions(A * k, 6, nB):
        ma.step(torch.from_numpy(a))
        state = ma.get_state()
        assert state.shape == (nB, 4 * A * k + 10) and not state[:, :4 * A * k].any()
        ts = ma.true_state()
        assert ts.shape == (nB, 8 * A * k) and ts.dtype == torch.float32
        want, _ = tr.of_env(ma.vec, cross=True)
        assert np.array_equal(bits(ts.cpu().numpy()), bits(want.reshape(nB, -1)))
        hidden += float(ts.view(nB, A * k, 8)[..., 1].sum())
    assert hidden > 0
    ma.vec.close()


@gpu
def test_error_paths(lib):
    import torch
    env = make_env(W_S, W_Q)
    with pytest.raises(RuntimeError):
        env.ground_truth()  # before the first reset
    out = torch.zeros((B, W_S, 8), dtype=torch.float32, device="cuda:0")
    with pytest.raises(ValueError):  # the library's own check: a handle without state
        env.handle.ground_truth(out)
    env.reset()
    h = env.handle
    assert h.lib.lbsim_ground_truth(h.h, None, None) == lib.EINVAL
    assert b"NULL" in h.lib.lbsim_last_error(h.h)
    flat = torch.zeros(B * W_S * 8 + 1, dtype=torch.float32, device="cuda:0")
    assert h.lib.lbsim_ground_truth(h.h, ctypes.c_void_p(flat.data_ptr() + 4), None) == lib.EINVAL
    assert not flat.any()
    for bad in (torch.zeros((B, W_S, 7), device="cuda:0"),
                torch.zeros((B, W_S, 8), dtype=torch.float64, device="cuda:0"),
                torch.zeros((B, W_S, 8)), flat[1:].view(B, W_S, 8)[:, :, ::1].transpose(0, 1)):
        with pytest.raises(ValueError):
            env.ground_truth(out=bad)
    assert env.ground_truth(out=out) is out and bool((out[..., 6] == 1).all())
    env.close()
