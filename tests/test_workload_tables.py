"""Workload tables (lbsim_set_workload_tables, VecLoadBalanceEnv.set_workload_tables,
marllb_amd.workload).

The reference is the unmodified oracle in TRACE mode.  Its draw_arrival computes the same Philox
block (arr_idx, gid, episode, 1 << 24) on a TRACE handle as on a Poisson one and sends z and w to
next_u2 / next_u3; only the gap and the work come from the trace, at row
(gid * 7919 + (e - 1) * 1000003 + k) mod R.  So env gid of a table handle equals a one-env TRACE
oracle (env_id_offset = gid) whose trace this file builds on the host: for each episode e and
arrival k it writes, at that row,

    gap_us = max(1, int32(f32(tab_g[bin(d0)]) * f32(mean_gap)))      work = tab_w[bin(d1)]

with d = tests/policy_ref.philox4x32_10.  R = 65536 and 1000003 mod 65536 = 16963, so episodes
1..3 with fewer than 16963 arrivals each occupy disjoint rows: host_trace asserts that no row is
written twice, and the tests assert from the final state that arr_idx stayed below the bound.
The oracle's config is the handle's with arrival_source switched to TRACE (the arrival rate is
kept: lost-FIN's bucket wait reads it).  Every change -- tables installed mid-run, new ids, a new
arrival-rate phase, new server rates -- is an oracle hand-off: a new oracle with the new trace or
config loads the old one's state.  The host tests show first, with the closed form written into
such traces, that this construction equals one unbroken Poisson oracle bit for bit.  Every GPU
comparison is bit for bit, through tests/parity.run_vs_reference.

The bank: exponential, bounded_pareto(1.5, 1000), hyperexp(8), constant -- and, because the
library rejects a gap table with an entry above 64 (the largest entries of bounded_pareto(1.5,
1000) and hyperexp(8) are 344 and 170: the error-path test shows them refused as gap tables),
two heavy-tailed tables that pass as gap tables, bounded_pareto(1.5, 100) and hyperexp(2).  Every
table is some env's work table, every table that may be a gap table is some env's gap table.

A handle with tables is a full handle: whatever mapping a case asks for, its
steps and resets run dynamics_group_full_kernel, and that is the form each case checks.
"""
import os
import subprocess

import numpy as np
import pytest

from marllb_amd import _lib, flowstats, trace, workload
from tests import parity, statelayout
from tests.parity import lib  # noqa: F401
from tests.policy_ref import philox4x32_10

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K = 128

R = 65536        # rows of a host-built trace
KMAX = 16963     # 1000003 mod R: arrivals per episode that keep episodes 1..3 on disjoint rows
EPISODES = (1, 2, 3)
ALIAS = {"assign_policy": "alias", "action_type": "continuous"}
NEXT_STEP = {"autoreset": True, "autoreset_mode": "next_step"}

_BANK = None
EXP, BP1000, HX8, CONST, BP100, HX2 = range(6)
GAP_OK = (EXP, CONST, BP100, HX2)  # the tables with every entry <= 64


def bank():
    """(6, 896) f32: the four tables the issue names, then the two gap-safe heavy-tailed ones."""
    global _BANK
    if _BANK is None:
        _BANK = np.stack([workload.exponential_table(), workload.bounded_pareto_table(1.5, 1000.0),
                          workload.hyperexp_table(8.0), workload.constant_table(),
                          workload.bounded_pareto_table(1.5, 100.0), workload.hyperexp_table(2.0)])
    return _BANK


def make_ids(B, seed):
    """Per-env (gap_id, work_id): every table is some env's work table, every gap-safe table some
    env's gap table; env 0 has a heavy-tailed gap, env 1 a heavy-tailed work."""
    rng = np.random.default_rng(seed)
    g = np.asarray(GAP_OK)[rng.integers(0, len(GAP_OK), B)].astype(np.int32)
    w = rng.integers(0, 6, B).astype(np.int32)
    g[:4] = (HX2, EXP, BP100, CONST)
    w[:6] = (EXP, BP1000, HX8, CONST, BP100, HX2)[:min(6, B)]
    return g, w


def draws(seed, gid, episode, n=KMAX):
    """The Philox blocks (n, 4) of arrivals 0 .. n - 1 of env gid's episode."""
    ctr = np.zeros((n, 4), np.uint64)
    ctr[:, 0] = np.arange(n)
    ctr[:, 1], ctr[:, 2], ctr[:, 3] = gid, episode, 1 << 24
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64))


def mean_gap_of(rate):
    """derive_params' mean gap: 1e6 / rate divided in f64 and rounded once to f32."""
    return np.float32(1e6 / float(np.float32(rate)))


def host_trace(seed, gid, rate, gap_of, work_of, n=KMAX):
    """The R-row trace that makes a one-env TRACE oracle draw gap_of(d0) / work_of(d1)."""
    gap = np.zeros(R, np.uint32)
    work = np.zeros(R, np.float32)
    written = np.zeros(R, bool)
    for e in EPISODES:
        rows = (gid * 7919 + (e - 1) * 1000003 + np.arange(n, dtype=np.int64)) % R
        assert not written[rows].any() and len(set(rows.tolist())) == n, "a row written twice"
        written[rows] = True
        d = draws(seed, gid, e, n)
        gap[rows] = gap_of(d[:, 0])
        work[rows] = work_of(d[:, 1])
    return trace.Trace(gap, work, float(rate), f"host-{gid}")


def table_trace(seed, gid, rate, tab_g, tab_w):
    mg = mean_gap_of(rate)

    def gap_of(d0):
        g = (tab_g[workload.table_bin(d0)].astype(np.float32) * mg).astype(np.int32)
        return np.maximum(g, 1).astype(np.uint32)
    return host_trace(seed, gid, rate, gap_of, lambda d1: tab_w[workload.table_bin(d1)])


class TableOracles:
    """B chained one-env oracles.  Env b runs the oracle of its spec -- (tables on?, gap_id,
    work_id, arrival rate, server rates) -- and at every change of spec (set_tables, set_ids,
    clear, set_rates, a new phase of an arrival schedule) a new oracle is created, with a new host
    trace where the gap or work changes and a new config where a rate does, and loads the old
    one's state.  arr_sched (B, P) with hold H is tests/test_rate_schedule.py's phase rule: a
    reset runs at phase 0, and with next_step the step after a done is that reset."""

    def __init__(self, oracle_mod, B, S, kw, tables=None, gap_id=None, work_id=None, arr=None,
                 srv=None, arr_sched=None, H=1, next_step=False, offset=0):
        self.mod, self.B, self.S, self.offset = oracle_mod, B, S, offset
        self.kw = dict(kw)
        if next_step:
            self.kw["next_step_reset"] = True
        self.next_step = next_step
        self.tables = tables
        self.gap_id = None if gap_id is None else np.broadcast_to(gap_id, (B,)).copy()
        self.work_id = None if work_id is None else np.broadcast_to(work_id, (B,)).copy()
        self.arr, self.srv, self.arr_sched, self.H = arr, srv, arr_sched, H
        self.k = np.zeros(B, np.int64)
        self.prev_done = np.zeros(B, bool)
        self.handoffs = 0
        self.cache = {}
        self.spec = [None] * B
        self.envs = [None] * B
        for b in range(B):
            self._sync(b, 0)

    def _spec(self, b, phase):
        rate = float(self.kw.get("arrival_rate", 400.0))
        if self.arr is not None:
            rate = float(self.arr[b])
        if self.arr_sched is not None:
            rate = float(self.arr_sched[b, phase])
        mu = None if self.srv is None else tuple(float(x) for x in self.srv[b])
        on = self.tables is not None
        return (on, int(self.gap_id[b]) if on else -1, int(self.work_id[b]) if on else -1, rate, mu)

    def _make(self, b, spec):
        from marllb_amd.env import make_config
        on, g, w, rate, mu = spec
        if mu is None:  # the handle's own server rates, whatever the env's arrival rate is now
            base = make_config(1, self.S, **self.kw)
            mu = [float(base.server_rate[s]) for s in range(self.S)]
        rk = {"arrival_rate": rate, "server_rates": list(mu)}
        cfg = make_config(1, self.S, env_id_offset=self.offset + b, **{**self.kw, **rk})
        if not on:
            return self.mod.OracleEnv(cfg)
        key = (b, g, w, rate)
        if key not in self.cache:
            self.cache[key] = table_trace(int(cfg.seed), self.offset + b, rate, self.tables[g],
                                          self.tables[w])
        cfg.arrival_source = _lib.ARRIVAL_TRACE
        return self.mod.OracleEnv(cfg, trace=self.cache[key])

    def _sync(self, b, phase):
        spec = self._spec(b, phase)
        if spec == self.spec[b]:
            return
        new = self._make(b, spec)
        if self.envs[b] is not None:
            new.load_state(self.envs[b].state_bytes())
            self.envs[b].close()
            self.handoffs += 1
        self.envs[b], self.spec[b] = new, spec

    def phases_next(self):
        if self.arr_sched is None:
            return np.zeros(self.B, np.int64)
        ph = (self.k // self.H) % self.arr_sched.shape[1]
        return np.where(self.next_step & self.prev_done, 0, ph)

    # the handle's calls
    def set_tables(self, tables, gap_id, work_id):
        self.tables = tables
        self.gap_id = np.broadcast_to(gap_id, (self.B,)).copy()
        self.work_id = np.broadcast_to(work_id, (self.B,)).copy()

    def set_ids(self, gap_id=None, work_id=None):
        if gap_id is not None:
            self.gap_id = np.asarray(gap_id).copy()
        if work_id is not None:
            self.work_id = np.asarray(work_id).copy()

    def clear(self):
        self.tables = None

    def set_rates(self, arr=None, srv=None):
        self.arr = self.arr if arr is None else arr
        self.srv = self.srv if srv is None else srv

    def reset(self, mask=None, obs=None):
        out = None if mask is None else obs.copy()
        rows = []
        for b in range(self.B):
            if mask is not None and not mask[b]:
                continue
            self._sync(b, 0)
            self.k[b], self.prev_done[b] = 0, False
            if mask is None:
                rows.append(self.envs[b].reset())
            else:
                out[b:b + 1] = self.envs[b].reset(mask=np.ones(1, np.uint8), obs=out[b:b + 1].copy())
        return np.concatenate(rows) if mask is None else out

    def step(self, a):
        nxt = self.phases_next()
        res = []
        for b in range(self.B):
            self._sync(b, int(nxt[b]))
            res.append(self.envs[b].step(a[b:b + 1]))
            restarted = self.next_step and self.prev_done[b]
            self.k[b] = 0 if restarted else self.k[b] + 1
            self.prev_done[b] = bool(res[-1][2][0])
        return tuple(np.concatenate([x[i] for x in res]) for i in range(4))

    def state_bytes(self):
        return [o.state_bytes() for o in self.envs]

    def close(self):
        for o in self.envs:
            o.close()


def check_bounds(env):
    """The run stayed inside the host traces: episodes 1..3, fewer than KMAX arrivals each."""
    st = statelayout.parse_cfg(env.get_state(), env.cfg)
    assert int(st["arr_idx"].max()) < KMAX - 1, int(st["arr_idx"].max())
    assert 1 <= int(st["episode"].min()) and int(st["episode"].max()) <= EPISODES[-1]


def check_full_kernel(lib, env):
    """A table handle's dynamics: dynamics_group_full_kernel, of the forced width in a child run
    under LBSIM_DYN_GROUP_LANES when the servers fit."""
    kern = lib.load().lbsim_dynamics_kernel(env.handle.h)
    names = lib.launch_names(env.handle)
    assert kern == parity.GROUP, (kern, names)
    lanes = os.environ.get("LBSIM_DYN_GROUP_LANES")
    pre = "dynamics_group_full_kernel<"
    if lanes and int(lanes) >= env.cfg.num_servers:
        pre += f"{lanes},"
    assert names.get(0, "").startswith(pre), names


# id: (B, S, mapping, config kwargs, VecLoadBalanceEnv kwargs): test_trace_bank.py's shapes, the
# smallest that reach every mapping, every group width and a partial last wave
CASES = {
    "auto-67x4": (67, 4, "auto", {}, None),
    "env-35x8": (35, 8, "env", {}, None),
    "server-19x16": (19, 16, "server", {}, None),
    "alias-67x4": (67, 4, "server", ALIAS, None),
    "fused-35x8-fail": (35, 8, "server-fused", {"fail_prob": 0.05}, None),
    "auto-67x4-nextstep": (67, 4, "auto", {"max_steps": 5}, NEXT_STEP),
    "alias-67x4-nextstep": (67, 4, "server", {"max_steps": 5, **ALIAS}, NEXT_STEP),
    "full-19x16-service": (19, 16, "server", {"duration_mode": "service"}, None),
}
SEED = 2100
HOST_B = 5


def make_env(B, S, mapping="auto", env_kw=None, **kw):
    from marllb_amd.env import VecLoadBalanceEnv
    kw = dict(kw)
    if mapping == "server-fused":
        mapping, kw["step_kernel"] = "server", "fused"
    return VecLoadBalanceEnv(B, S, device="cuda:0", dyn_mapping=mapping,
                             **{"autoreset": False, **(env_kw or {})}, **kw)


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_bit_exact_vs_trace_oracles(lib, oracle_mod, case):
    """Every mapping and config form with per-env tables against the one-env TRACE oracles."""
    B, S, mapping, kw, env_kw = CASES[case]
    idx = list(CASES).index(case)
    kw = {"seed": SEED + idx, **kw}
    g, w = make_ids(B, SEED + S)
    assert set(w.tolist()) == set(range(6)) and set(g.tolist()) == set(GAP_OK)
    env = make_env(B, S, mapping, env_kw, **kw)
    env.set_workload_tables(bank(), torch.from_numpy(g).to("cuda:0"), w)
    ref = TableOracles(oracle_mod, B, S, kw, bank(), g, w, next_step=env.next_step)
    parity.run_vs_reference(env, ref, kw, idx, steps=10, post_steps=4,
                            hook=lambda e: check_full_kernel(lib, e))
    check_bounds(env)
    eg, ew = env.env_workload
    np.testing.assert_array_equal(eg.cpu().numpy(), g)
    np.testing.assert_array_equal(ew.cpu().numpy(), w)
    ref.close()
    env.close()


def _child(env_over):
    ks = [f"test_bit_exact_vs_trace_oracles[{c}]" for c, v in CASES.items() if v[1] <= 4]
    assert len(ks) == 4
    parity.run_cases_in_child("test_workload_tables.py", ks, env_over)


@gpu
def test_four_lane_groups_bit_exact():
    """LBSIM_DYN_GROUP_LANES=4: the 4-lane full kernel on the S <= 4 cases."""
    _child({"LBSIM_DYN_GROUP_LANES": "4"})


@gpu
def test_under_forced_wave_dynamics_bit_exact():
    """LBSIM_DYN_WAVE=1: a table handle stays a full handle; the S <= 4 cases still agree."""
    _child({"LBSIM_DYN_WAVE": "1"})


# ------------------------------------------------------------------ composition

@gpu
def test_with_per_env_rates(lib, oracle_mod):
    """Per-env arrival and server rates from sample_rates under per-env tables."""
    from marllb_amd.randomize import sample_rates
    B, S, kw = 35, 4, {"seed": SEED + 20}
    gen = torch.Generator()
    gen.manual_seed(7)
    arr, srv = sample_rates(B, S, rate=(200.0, 1500.0), load=(0.3, 1.2), server_skew=(1.0, 3.0),
                            generator=gen)
    g, w = make_ids(B, 31)
    env = make_env(B, S, **kw)
    env.set_rates(arr, srv)
    env.set_workload_tables(bank(), g, w)
    ref = TableOracles(oracle_mod, B, S, kw, bank(), g, w, arr=arr.numpy(), srv=srv.numpy())
    parity.run_vs_reference(env, ref, kw, 21, steps=10, post_steps=4,
                            hook=lambda e: check_full_kernel(lib, e))
    check_bounds(env)
    ref.close()
    env.close()


@gpu
def test_with_arrival_schedule(lib, oracle_mod):
    """An arrival-rate schedule, P = 3, H = 2: every phase scales the gaps of the same tables."""
    B, S, P, H, kw = 35, 4, 3, 2, {"seed": SEED + 21}
    sched = np.random.default_rng(5).uniform(150.0, 900.0, (B, P)).astype(np.float32)
    g, w = make_ids(B, 32)
    env = make_env(B, S, **kw)
    env.set_workload_tables(bank(), g, w)
    env.set_rate_schedule(sched, None, steps_per_phase=H, wrap=True)
    ref = TableOracles(oracle_mod, B, S, kw, bank(), g, w, arr_sched=sched, H=H)
    parity.run_vs_reference(env, ref, kw, 22, steps=10, post_steps=4)
    check_bounds(env)
    assert ref.handoffs > 2 * B
    ref.close()
    env.close()


@gpu
def test_on_lost_fin_handle(lib, oracle_mod):
    """A lost-FIN handle (flow_timeout 0.4 s) with per-env server rates and tables."""
    from marllb_amd.randomize import sample_rates
    B, S = 35, 4
    kw = {"seed": SEED + 22, "lost_fin_prob": 0.2, "flow_timeout": 0.4, "lost_fin_pending": 8}
    gen = torch.Generator()
    gen.manual_seed(9)
    _, srv = sample_rates(B, S, rate=(400.0, 400.0), load=(0.4, 1.1), server_skew=(1.0, 3.0),
                          generator=gen)
    g, w = make_ids(B, 33)
    env = make_env(B, S, **kw)
    env.set_rates(None, srv)
    env.set_workload_tables(bank(), g, w)
    ref = TableOracles(oracle_mod, B, S, kw, bank(), g, w, srv=srv.numpy())
    parity.run_vs_reference(env, ref, kw, 23, steps=10, post_steps=4,
                            hook=lambda e: check_full_kernel(lib, e))
    check_bounds(env)
    ref.close()
    env.close()


def oracle_counts(ref):
    cnt, rec = [], []
    for o in ref.envs:
        d = statelayout.parse(o.state_bytes(), 1, ref.S, 32, False)
        cnt.append(d["res_count"].astype(np.int64))
        rec.append(d["res_fct"].reshape(ref.S, K))
    return np.stack(cnt), np.stack(rec)


@gpu
def test_flow_stats_handle(lib, oracle_mod):
    """A flow_stats=True handle at a tenth of the load (no oracle reservoir passes its 128 slots,
    tests/test_flow_stats.py's bound): outputs, state, and statistics equal to those the oracles'
    records imply."""
    B, S = 67, 4
    kw = {"seed": SEED + 23, "warmup_steps": 2, "arrival_rate": 40.0}
    g, w = make_ids(B, 34)
    env = make_env(B, S, env_kw={"flow_stats": True}, **kw)
    env.set_workload_tables(bank(), g, w)
    ref = TableOracles(oracle_mod, B, S, kw, bank(), g, w)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    count = np.zeros((B, S), np.uint32)
    sum_us = np.zeros((B, S), np.uint64)
    max_us = np.zeros((B, S), np.uint32)
    hist = np.zeros((B, S, flowstats.NBINS), np.uint32)
    c0, _ = oracle_counts(ref)
    rng = np.random.default_rng(61)
    for k in range(12):
        parity.step_both(env, ref, parity.actions(rng, B, S, kw), k)
        c1, rec = oracle_counts(ref)
        assert c1.max() <= K, "the oracle's reservoirs wrapped: lower the load of this test"
        for b, s in zip(*np.nonzero(c1 > c0)):
            v = rec[b, s, c0[b, s]:c1[b, s]].astype(np.int64)
            count[b, s] += v.size
            sum_us[b, s] += np.uint64(v.sum())
            max_us[b, s] = max(int(max_us[b, s]), int(v.max()))
            np.add.at(hist[b, s], flowstats.bin_of(v), 1)
        c0 = c1
    check_full_kernel(lib, env)
    parity.compare_state(env.handle, ref, env.cfg)
    cnt, sm, mx, h = env.handle.flow_stats(hist=True)
    np.testing.assert_array_equal(cnt.cpu().numpy().view(np.uint32), count)
    np.testing.assert_array_equal(sm.cpu().numpy().view(np.uint64), sum_us)
    np.testing.assert_array_equal(mx.cpu().numpy().view(np.uint32), max_us)
    np.testing.assert_array_equal(h.cpu().numpy().view(np.uint32), hist)
    assert count.sum() > 10 * B
    ref.close()
    env.close()


@gpu
def test_installed_mid_run(lib, oracle_mod):
    """5 Poisson steps, set_workload_tables, 5 steps, set_env_workload with new ids, 5 steps: the
    arrival in flight keeps its time and work at both changes (the hand-off carries it)."""
    B, S, kw = 67, 4, {"seed": SEED + 24}
    g0, w0 = make_ids(B, 35)
    g1, w1 = make_ids(B, 36)
    g1, w1 = np.roll(g1, 7), np.roll(w1, 11)
    env = make_env(B, S, **kw)
    ref = TableOracles(oracle_mod, B, S, kw)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    rng = np.random.default_rng(3)

    def in_flight():
        st = statelayout.parse_cfg(env.get_state(), env.cfg)
        return st["next_arr"].copy(), st["next_work"].copy()

    def five(k0):
        for k in range(k0, k0 + 5):
            parity.step_both(env, ref, parity.actions(rng, B, S, kw), k)
        parity.compare_state(env.handle, ref, env.cfg)

    five(0)
    before = in_flight()
    env.set_workload_tables(bank(), g0, w0)
    ref.set_tables(bank(), g0, w0)
    for x, y in zip(before, in_flight()):
        np.testing.assert_array_equal(x, y)
    five(5)
    check_full_kernel(lib, env)
    before = in_flight()
    env.set_env_workload(g1, torch.from_numpy(w1).to("cuda:0"))
    ref.set_ids(g1, w1)
    for x, y in zip(before, in_flight()):
        np.testing.assert_array_equal(x, y)
    five(10)
    assert ref.handoffs >= B + (np.logical_or(g0 != g1, w0 != w1)).sum()
    check_bounds(env)
    ref.close()
    env.close()


# ------------------------------------------------------------------ equivalences, GPU twins

def run_twins(envs, steps=8, seed=4, reset=True):
    B, S = envs[0].num_envs, envs[0].num_servers
    outs = [[e.reset()] if reset else [] for e in envs]
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        a = torch.from_numpy(rng.integers(0, 3, (B, S)))
        for e, o in zip(envs, outs):
            obs, rew, done, info = e.step(a, assign_counts=True)
            o += [obs, rew, done, info["assign_counts"]]
    return outs, [e.get_state() for e in envs]


def same(x, y):
    return len(x) == len(y) and all(torch.equal(a, b) for a, b in zip(x, y))


@gpu
def test_equivalences(lib):
    """A shared id equals the same id given per env; clear_workload_tables() followed by steps
    equals a handle that never had tables, loaded with the same state; the accessors return what
    was set."""
    B, S = 67, 4
    shared, per_env, cleared, plain = (make_env(B, S, seed=5) for _ in range(4))
    shared.set_workload_tables(bank(), HX2, BP1000)
    per_env.set_workload_tables(bank(), np.full(B, HX2), np.full(B, BP1000))
    o, s = run_twins([shared, per_env])
    assert same(o[0], o[1]) and s[0] == s[1]
    for e in (shared, per_env):
        gg, ww = e.env_workload
        assert (gg == HX2).all() and (ww == BP1000).all() and gg.dtype == torch.int32
    g, w = make_ids(B, 40)
    shared.set_env_workload(work_id=w)  # None: the gap ids stay
    gg, ww = shared.env_workload
    assert (gg == HX2).all() and np.array_equal(ww.cpu().numpy(), w)
    shared.set_env_workload(gap_id=g)
    gg, ww = shared.env_workload
    assert np.array_equal(gg.cpu().numpy(), g) and np.array_equal(ww.cpu().numpy(), w)

    cleared.set_workload_tables(bank(), g, w)
    oc, sc = run_twins([cleared], steps=4)
    plain.reset()
    oe, se = run_twins([plain], steps=4)
    assert sc[0] != se[0]  # the tables were read
    cleared.clear_workload_tables()
    with pytest.raises(ValueError, match="no workload tables"):
        cleared.env_workload
    plain.set_state(sc[0])
    o, s = run_twins([cleared, plain], steps=6, seed=9, reset=False)
    assert same(o[0], o[1]) and s[0] == s[1]
    names = lib.launch_names(cleared.handle)
    assert not names.get(0, "").startswith("dynamics_group_full_kernel<"), names
    for e in (shared, per_env, cleared, plain):
        e.close()


@gpu
def test_graph_replay(lib):
    """A step captured after the first set_workload_tables and replayed: ids rewritten between
    replays (same T, so in place) are seen without a new capture."""
    B, S = 67, 4
    g0, w0 = make_ids(B, 41)
    g1, w1 = np.roll(g0, 5), np.roll(w0, 9)
    eager = make_env(B, S, seed=8, max_steps=5, env_kw={"autoreset": True})
    graph = make_env(B, S, seed=8, max_steps=5, env_kw={"autoreset": True, "graph_mode": True})
    for e in (eager, graph):
        e.set_workload_tables(bank(), g0, w0)
        e.reset()
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1)
    acts = [torch.randint(0, 3, (B, S), device="cuda:0", generator=gen) for _ in range(13)]
    a_static = acts[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graph.step(a_static)
    torch.cuda.current_stream().wait_stream(side)
    eager.step(acts[0])
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        obs, rew, done, info = graph.step(a_static)
    for k in range(1, 13):
        if k == 7:
            for e in (eager, graph):
                e.set_env_workload(g1, w1)
        a_static.copy_(acts[k])
        cg.replay()
        eo, er, ed, _ = eager.step(acts[k])
        assert torch.equal(obs, eo), k
        assert torch.equal(rew, er) and torch.equal(done, ed), k
    assert graph.get_state() == eager.get_state()
    assert np.array_equal(graph.env_workload[0].cpu().numpy(), g1)
    eager.close()
    graph.close()


@gpu
def test_shard_invariance(lib):
    """B = 131 in two uneven shards (env_id_offset = lo, ids[lo:hi]) equal the whole batch."""
    B, S = 131, 4
    g, w = make_ids(B, 42)
    bounds = [0, 47, B]
    full = make_env(B, S, seed=9)
    full.set_workload_tables(bank(), g, w)
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        e = make_env(hi - lo, S, seed=9, env_id_offset=lo)
        e.set_workload_tables(bank(), g[lo:hi], w[lo:hi])
        parts.append(e)
    assert torch.equal(full.reset(), torch.cat([e.reset() for e in parts]))
    rng = np.random.default_rng(B)
    for _ in range(7):
        a = torch.from_numpy(rng.integers(0, 3, (B, S)))
        fo, fr, fd, fi = full.step(a, assign_counts=True)
        po = [e.step(a[lo:hi], assign_counts=True) for e, lo, hi in zip(parts, bounds[:-1], bounds[1:])]
        assert torch.equal(fo, torch.cat([p[0] for p in po]))
        assert torch.equal(fr, torch.cat([p[1] for p in po]))
        assert torch.equal(fd, torch.cat([p[2] for p in po]))
        assert torch.equal(fi["assign_counts"], torch.cat([p[3]["assign_counts"] for p in po]))
    for e in [full] + parts:
        e.close()


@gpu
def test_snapshot_restore_with_src(lib, oracle_mod):
    """A restore with src forks env states across slots: the forked env draws from the tables of
    the slot it lands in (the TRACE oracle of slot b, loaded with the state of env src[b])."""
    B, S, kw = 19, 4, {"seed": SEED + 25}
    g, w = make_ids(B, 43)
    env = make_env(B, S, **kw)
    env.set_workload_tables(bank(), g, w)
    ref = TableOracles(oracle_mod, B, S, kw, bank(), g, w)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    rng = np.random.default_rng(6)
    for k in range(4):
        parity.step_both(env, ref, parity.actions(rng, B, S, kw), k)
    snap = env.snapshot()
    src = np.random.default_rng(8).integers(0, B, B).astype(np.int32)
    src[0] = 0
    states = ref.state_bytes()
    env.restore(snap, src=torch.from_numpy(src).to("cuda:0"))
    for b in range(B):
        # the one-env state of env src[b], with slot b's own env id, into slot b's oracle
        ref.envs[b].load_state(states[int(src[b])])
    assert (src != np.arange(B)).sum() > B // 2
    for k in range(4, 10):
        parity.step_both(env, ref, parity.actions(rng, B, S, kw), k)
    parity.compare_state(env.handle, ref, env.cfg)
    check_bounds(env)
    env.close()
    ref.close()


@gpu
def test_multi_agent_forwards(lib):
    from marllb_amd.multi_agent import VecMultiAgentLoadBalanceEnv
    B = 9
    ma = VecMultiAgentLoadBalanceEnv(B, num_agents=2, servers_per_agent=2, device="cuda:0", seed=3)
    g, w = make_ids(B, 44)
    ma.set_workload_tables(bank(), g, w)
    gg, ww = ma.env_workload
    assert np.array_equal(gg.cpu().numpy(), g) and np.array_equal(ww.cpu().numpy(), w)
    ma.set_env_workload(work_id=np.roll(w, 1))
    assert np.array_equal(ma.vec.env_workload[1].cpu().numpy(), np.roll(w, 1))
    ma.clear_workload_tables()
    with pytest.raises(ValueError):
        ma.env_workload
    ma.close()


@gpu
def test_errors_leave_the_tables_in_force(lib, oracle_mod):
    """Each error leaves the tables in force untouched, and steps stay equal to the reference."""
    B, S, kw = 19, 4, {"seed": SEED + 26}
    g, w = make_ids(B, 45)
    env = make_env(B, S, **kw)
    env.set_workload_tables(bank(), g, w)
    ref = TableOracles(oracle_mod, B, S, kw, bank(), g, w)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    rng = np.random.default_rng(2)
    k = 0

    def still_equal():
        nonlocal k
        for _ in range(2):
            parity.step_both(env, ref, parity.actions(rng, B, S, kw), k)
            k += 1
        eg, ew = env.env_workload
        assert np.array_equal(eg.cpu().numpy(), g) and np.array_equal(ew.cpu().numpy(), w)

    def bad(i, v):
        t = bank().copy()
        t[EXP, i] = v
        return t

    zeros = bank().copy()
    zeros[CONST] = 0.0
    mu = float(env.cfg.server_rate[0])
    over = bank().copy()  # a work table over wmax * (1e6 / mu) * Q <= 2^30 for the config's mu
    over[BP1000] *= np.float32(1.01 * 2.0 ** 30 * mu / (1e6 * env.cfg.queue_capacity) / over[BP1000].max())
    for tables, gi, wi, msg in (
            (bad(100, np.nan), g, w, "offender"), (bad(0, -1.0), g, w, "offender"),
            (bad(3, 65.0), g, w, "offender"),         # table EXP is some env's gap table
            (bank(), np.full(B, HX8), w, "offender"),  # hyperexp(8) as a gap table: entries > 64
            (zeros, g, w, "offender"),                # a gap table of zeros: mean < 1/16
            (bank(), np.where(np.arange(B) == 3, 6, g), w, "offender"),  # an id equal to T
            (over, g, w, "2\\^30")):
        with pytest.raises(ValueError, match=msg):
            env.set_workload_tables(tables, gi, wi)
        still_equal()
    with pytest.raises(ValueError, match="offender"):
        env.set_env_workload(work_id=np.where(np.arange(B) == 5, -1, w))
    still_equal()
    h = env.handle
    dev_t = torch.from_numpy(bank()).to("cuda:0")
    ids = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError, match="n_tables"):  # T = 0
        h.check(h.lib.lbsim_set_workload_tables(h.h, dev_t.data_ptr(), 0, ids.data_ptr(),
                                                ids.data_ptr(), B, None))
    with pytest.raises(lib.LbsimError, match="rows") as ei:  # rows = 2
        h.check(h.lib.lbsim_set_workload_tables(h.h, dev_t.data_ptr(), 6, ids.data_ptr(),
                                                ids.data_ptr(), 2, None))
    assert ei.value.code == lib.ESHAPE
    still_equal()
    # a set_rates whose server rate falls under the floor the tables in force impose
    wmax = float(bank()[[BP1000, HX8]].max())
    floor = wmax * env.cfg.queue_capacity * 1e6 / 2.0 ** 30
    assert 1.0 < floor < mu
    low = np.full((B, S), mu, np.float32)
    low[7, 2] = np.float32(0.9 * floor)
    with pytest.raises(ValueError, match="out of range"):
        env.set_rates(None, low)
    with pytest.raises(ValueError, match="out of range"):
        env.set_rate_schedule(None, low[:, None, :].repeat(2, axis=1))
    still_equal()
    check_bounds(env)
    env.close()
    ref.close()
    # a TRACE handle
    tr = make_env(B, S, seed=1, trace=trace.synthetic(97, 300.0, seed=1))
    with pytest.raises(ValueError, match="TRACE"):
        tr.set_workload_tables(bank(), 0, 0)
    tr.close()


# ------------------------------------------------------------------ host tests (no GPU)

def edge_words():
    e = workload.bin_edges()
    return np.concatenate([e[:-1], e[1:] - np.uint64(1)]).astype(np.uint64)


def test_bin_rule():
    """table_bin at every bin's first and last word; monotone; the masses sum to 2^32."""
    e = workload.bin_edges()
    assert e.shape == (workload.TABLE_BINS + 1,) and int(e[0]) == 0 and int(e[-1]) == 2 ** 32
    k = np.arange(workload.TABLE_BINS)
    np.testing.assert_array_equal(workload.table_bin(e[:-1]), k)
    np.testing.assert_array_equal(workload.table_bin(e[1:] - np.uint64(1)), k)
    assert workload.table_bin(0) == 0 and workload.table_bin(31) == 31 and workload.table_bin(32) == 32
    assert workload.table_bin(2 ** 32 - 1) == workload.TABLE_BINS - 1 == 895
    v = np.sort(np.random.default_rng(0).integers(0, 2 ** 32, 20000, dtype=np.uint64))
    assert (np.diff(workload.table_bin(v)) >= 0).all()
    m = workload.bin_mass()
    assert int(m.sum()) == 2 ** 32 and (m[:32] == 1).all()
    np.testing.assert_array_equal(m[32:], np.uint64(1) << (k[32:] // 32 - 1).astype(np.uint64))
    # the issue's formula, word by word, on the edge words
    for x in (int(t) for t in edge_words()[::37]):
        ee = x.bit_length() - 1
        assert workload.table_bin(x) == (x if x < 32 else 32 * (ee - 4) + ((x >> (ee - 5)) & 31))
    assert "#define LBSIM_TABLE_BINS 896" in open(_lib.HEADER_PATH).read()


def test_header_table_bin_as_host_cpp(tmp_path):
    """csrc/lbsim_table.h compiled as host C++ (tests/workload_probe.cpp): the same bins."""
    exe = str(tmp_path / "workload_probe")
    subprocess.run(["c++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe,
                    os.path.join(HERE, "workload_probe.cpp")], check=True)
    words = edge_words()
    r = subprocess.run([exe], input="\n".join(str(int(x)) for x in words) + "\n",
                       capture_output=True, text=True, check=True)
    lines = r.stdout.split()
    assert lines[0] == str(workload.TABLE_BINS)
    np.testing.assert_array_equal(np.array(lines[1:], np.int64), workload.table_bin(words))


BUILDERS = {
    "exponential": workload.exponential_table,
    "bounded_pareto": lambda: workload.bounded_pareto_table(1.5, 1000.0),
    "lognormal": lambda: workload.lognormal_table(1.0),
    "hyperexp": lambda: workload.hyperexp_table(8.0),
    "weibull": lambda: workload.weibull_table(0.5),
    "constant": workload.constant_table,
    "empirical": lambda: workload.empirical_table(trace.builtin().work),
}


@pytest.mark.parametrize("name", list(BUILDERS))
def test_builders_have_mean_one(name):
    t = BUILDERS[name]()
    assert t.dtype == np.float32 and t.shape == (workload.TABLE_BINS,)
    assert np.isfinite(t).all() and (t >= 0).all()
    assert abs(workload.table_mean(t) - 1.0) <= 1e-6
    assert (np.diff(t.astype(np.float64)) <= 0).all()  # small words are the tail


def test_builder_moments():
    assert abs(workload.table_cv2(workload.exponential_table()) - 1.0) < 1e-3
    assert abs(workload.table_cv2(workload.hyperexp_table(8.0)) - 8.0) < 1e-2
    assert abs(workload.table_cv2(workload.weibull_table(0.5)) - 5.0) < 1e-2
    assert workload.table_cv2(workload.constant_table()) == 0.0
    ids = workload.sample_table_ids(1000, [1, 3], 5)
    assert ids.dtype == np.int32 and set(ids.tolist()) == {1, 3}
    assert np.array_equal(ids, workload.sample_table_ids(1000, [1, 3], 5))


def test_bounded_pareto_table():
    """Non-increasing in k, largest entry <= its bound after scaling, and the survival function at
    bin edges equals the analytic one."""
    alpha, bound = 1.5, 1000.0
    t = workload.bounded_pareto_table(alpha, bound).astype(np.float64)
    assert (np.diff(t) <= 0).all()
    # mean of the law on [1, bound]: alpha / (alpha - 1) * (1 - bound^(1 - alpha)) / (1 - bound^-alpha)
    mean = alpha / (alpha - 1.0) * (1.0 - bound ** (1.0 - alpha)) / (1.0 - bound ** -alpha)
    assert t.max() <= bound / mean * (1 + 1e-6) and t.min() >= 1.0 / mean * (1 - 1e-6)
    # P(X > x) analytic at the level between two bins = the mass of the bins above it
    e = workload.bin_edges().astype(np.float64)
    c = 1.0 - bound ** -alpha
    for k in (40, 200, 500, 800, 890):
        x = ((1.0 - (1.0 - e[k] / 2.0 ** 32) * c) ** (-1.0 / alpha)) / mean  # ppf at the edge
        assert t[k - 1] >= x * (1 - 1e-6) >= t[k] * (1 - 2e-6), k
        surv = ((x * mean) ** -alpha - bound ** -alpha) / c
        assert abs(surv - e[k] / 2.0 ** 32) <= 1e-9 * max(1.0, e[k] / 2.0 ** 32) + 1e-12, k


def test_empirical_table_reproduces_quantiles():
    x = np.sort(trace.builtin().work.astype(np.float64))
    t = workload.empirical_table(x).astype(np.float64) * x.mean()
    e = workload.bin_edges().astype(np.float64)
    n = x.size
    for k in range(0, workload.TABLE_BINS, 29):
        # every word of bin k maps to an order statistic between those of the bin's two edges
        q_hi, q_lo = 1.0 - e[k] / 2.0 ** 32, 1.0 - e[k + 1] / 2.0 ** 32
        lo = x[int(np.clip(np.ceil(q_lo * n) - 1, 0, n - 1))]
        hi = x[int(np.clip(np.ceil(q_hi * n) - 1, 0, n - 1))]
        assert lo * (1 - 1e-5) <= t[k] <= hi * (1 + 1e-5), k


def host_kw(case):
    kw = dict(CASES[case][3])
    kw["seed"] = SEED + list(CASES).index(case)
    if CASES[case][4] is NEXT_STEP:
        kw["next_step_reset"] = True
    return kw


HOST_N = 4096  # arrivals per episode of the host chains (the closed form is slow on the host)


@pytest.mark.parametrize("case", list(CASES) + ["lost-fin", "flow-load"])
def test_closed_form_traces_equal_poisson_oracle(oracle_mod, case):
    """The reference scheme itself, for every config the GPU cases use, on 5 envs: host traces
    built from the closed form make the one-env TRACE oracles equal one unbroken Poisson oracle,
    over reset, 10 steps, a masked reset and 4 more steps."""
    from marllb_amd.env import make_config
    if case == "lost-fin":
        S, kw = 4, {"seed": SEED + 22, "lost_fin_prob": 0.2, "flow_timeout": 0.4,
                    "lost_fin_pending": 8}
    elif case == "flow-load":
        S, kw = 4, {"seed": SEED + 23, "warmup_steps": 2, "arrival_rate": 40.0}
    else:
        S, kw = CASES[case][1], host_kw(case)
    B = HOST_B
    olib = oracle_mod.load()
    logf = np.vectorize(lambda x: olib.oracle_logf(float(x)), otypes=[np.float32])

    def u01(d):
        return ((d >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24)

    whole = oracle_mod.OracleEnv(make_config(B, S, **kw))
    rate = float(whole.cfg.arrival_rate)
    mg = mean_gap_of(rate)
    ones = []
    for b in range(B):
        cfg = make_config(1, S, env_id_offset=b, **kw)
        cfg.arrival_source = _lib.ARRIVAL_TRACE
        tr = host_trace(int(cfg.seed), b, rate,
                        lambda d0: ((-logf(u01(d0))).astype(np.float32) * mg).astype(np.int32).astype(np.uint32),
                        lambda d1: (-logf(u01(d1))).astype(np.float32), n=HOST_N)
        ones.append(oracle_mod.OracleEnv(cfg, trace=tr))

    def stacked(fn):
        return np.concatenate([fn(b, o) for b, o in enumerate(ones)])

    np.testing.assert_array_equal(whole.reset(), stacked(lambda b, o: o.reset()))
    rng = np.random.default_rng(1)
    for k in range(14):
        if k == 10:
            mask = (np.arange(B) % 3 == 0).astype(np.uint8)
            ow = whole.reset(mask=mask, obs=np.zeros((B, S, 11), np.float32))
            for b, o in enumerate(ones):
                if mask[b]:
                    np.testing.assert_array_equal(ow[b:b + 1], o.reset())
        a = parity.actions(rng, B, S, kw)
        rw = whole.step(a)
        ro = [o.step(a[b:b + 1]) for b, o in enumerate(ones)]
        for i in range(4):
            np.testing.assert_array_equal(rw[i], np.concatenate([r[i] for r in ro]), err_msg=f"{k}/{i}")
    pw = statelayout.parse_cfg(whole.state_bytes(), whole.cfg)
    assert int(pw["arr_idx"].max()) < HOST_N - 1 and int(pw["episode"].max()) <= EPISODES[-1]
    for b, o in enumerate(ones):
        po = statelayout.parse_cfg(o.state_bytes(), o.cfg, B=1)
        for name in po:
            if name not in ("ring", "pend"):
                np.testing.assert_array_equal(po[name], pw[name][b:b + 1] if pw[name].shape[0] == B
                                              else pw[name].reshape(B, -1)[b].reshape(po[name].shape),
                                              err_msg=name)
        o.close()
    whole.close()


def test_signature_table_declares_the_exports():
    for name, nargs in (("lbsim_set_workload_tables", 7), ("lbsim_set_env_workload", 4),
                        ("lbsim_get_env_workload", 4), ("lbsim_clear_workload_tables", 1)):
        assert name in _lib._SIGNATURES and len(_lib._SIGNATURES[name][1]) == nargs, name
    hdr = open(_lib.HEADER_PATH).read()
    for name in ("lbsim_set_workload_tables", "lbsim_set_env_workload", "lbsim_get_env_workload",
                 "lbsim_clear_workload_tables"):
        assert f"int {name}(" in hdr
