"""Trace banks (lbsim_set_trace_bank / lbsim_set_trace_schedule, VecLoadBalanceEnv.set_trace_bank /
set_env_trace / set_trace_schedule).

The reference is tests/test_rate_schedule.py's scheme with traces in place of rates: B chained
one-env oracles, env b with env_id_offset = b and the trace of its phase; at every change of phase
its oracle is replaced by one created with the new phase's trace that loads the old one's state
(the arrival already drawn, arr_idx and episode carry over; every later arrival reads the new
trace).  The host tests first show that such a chain over one and the same trace equals an
unbroken oracle for every config used.  Every GPU comparison is bit for bit: observations,
rewards, done flags, assignment counts and the device state.

The bank: trace.synthetic(R, rate, seed) with (R, rate) = (7, 400), (97, 250), (500, 400),
(1031, 650).  R = 7 is below every group width, so one draw-ahead refill wraps the trace several
times; R = 97 wraps about once per 0.25 s step; the unequal rates make the envs of one wave run
unequal iteration counts.  The flow-statistics case replays the same rows at a tenth of the load
(trace.rescaled): its check reads every completed flow from the oracle's reservoirs, which hold
128 per server (tests/test_rate_schedule.py::test_flow_stats_handle, the same bound).
"""
import hashlib

import numpy as np
import pytest

from marllb_amd import flowstats, trace
from marllb_amd.randomize import diurnal_trace_schedule, sample_trace_ids, schedule_phase
from tests import parity, statelayout
from tests.parity import GROUP, actions, compare_state, lib, step_both  # noqa: F401
from tests.test_env_rates import PerEnvOracles, check_kernel
from tests.test_rate_schedule import (ALIAS, NEXT_STEP, oracle_counts, run_twins, same,
                                      server_only_schedule)

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
K = 128

BANK_SPEC = ((7, 400.0), (97, 250.0), (500, 400.0), (1031, 650.0))


def make_bank(scale=1.0):
    ts = [trace.synthetic(R, rate, seed=11 + i) for i, (R, rate) in enumerate(BANK_SPEC)]
    return ts if scale == 1.0 else [trace.rescaled(t, scale) for t in ts]


def make_ids(B, P, T, seed, shared=False):
    """(B, P) int32 ids over all T traces; shared: env 0's row for every env."""
    ids = np.random.default_rng(seed).integers(0, T, (B, P)).astype(np.int32)
    ids[:T, 0] = np.arange(T)[:min(T, B)]  # every trace is some env's phase 0 (a reset's trace)
    return np.repeat(ids[:1], B, axis=0) if shared else ids


class TraceOracles:
    """B chained one-env oracles under the trace schedule ids (B, P) over `bank`, and optionally a
    server-rate schedule srv (B, Ps, S) with its own hold and wrap: env b runs the oracle of its
    pair of phases, handed the previous one's state at every change of either (also between two
    phases naming the same trace: the hand-off itself is under test).  A reset runs at phase 0;
    with next_step the step after a done is that reset."""

    def __init__(self, oracle_mod, B, S, kw, bank, ids, H, wrap, next_step=False, offset=0,
                 srv=None, srv_H=1, srv_wrap=True):
        self.mod, self.B, self.S = oracle_mod, B, S
        self.kw = {k: v for k, v in kw.items() if k != "trace"}
        if next_step:
            self.kw["next_step_reset"] = True
        self.bank, self.ids, self.H, self.wrap, self.offset = bank, ids, H, wrap, offset
        self.srv, self.srv_H, self.srv_wrap = srv, srv_H, srv_wrap
        self.P = ids.shape[1]
        self.next_step = next_step
        self.k = np.zeros(B, np.int64)  # steps completed in the episode (the device's ep_step)
        self.phase = [(0, 0)] * B
        self.prev_done = np.zeros(B, bool)
        self.handoffs = 0
        self.envs = [self._make(b, (0, 0)) for b in range(B)]

    def _make(self, b, ph):
        from marllb_amd.env import make_config
        rk = {} if self.srv is None else {"server_rates": self.srv[b, ph[1]].tolist()}
        # the handle's own config (its arrival_rate is the first trace's), the phase's trace
        cfg = make_config(1, self.S, env_id_offset=self.offset + b, trace=self.bank[0],
                          **{**self.kw, **rk})
        return self.mod.OracleEnv(cfg, trace=self.bank[int(self.ids[b, ph[0]])])

    def _to_phase(self, b, ph):
        if ph == self.phase[b]:
            return
        new = self._make(b, ph)
        new.load_state(self.envs[b].state_bytes())
        self.envs[b].close()
        self.envs[b], self.phase[b] = new, ph
        self.handoffs += 1

    def reset(self, mask=None, obs=None):
        out = None if mask is None else obs.copy()
        rows = []
        for b in range(self.B):
            if mask is not None and not mask[b]:
                continue
            self._to_phase(b, (0, 0))
            self.k[b], self.prev_done[b] = 0, False
            if mask is None:
                rows.append(self.envs[b].reset())
            else:
                out[b:b + 1] = self.envs[b].reset(mask=np.ones(1, np.uint8), obs=out[b:b + 1].copy())
        return np.concatenate(rows) if mask is None else out

    def phases_next(self):
        """The trace phase each env's next step runs at (what trace_phase reports)."""
        ph = schedule_phase(self.k, self.P, self.H, self.wrap)
        return np.where(self.next_step & self.prev_done, 0, ph)

    def srv_phases_next(self):
        if self.srv is None:
            return np.zeros(self.B, np.int64)
        ph = schedule_phase(self.k, self.srv.shape[1], self.srv_H, self.srv_wrap)
        return np.where(self.next_step & self.prev_done, 0, ph)

    def ids_next(self):
        """The trace each env's next step replays (what env_trace reports)."""
        return self.ids[np.arange(self.B), self.phases_next()]

    def step(self, a):
        nxt, snxt = self.phases_next(), self.srv_phases_next()
        res = []
        for b in range(self.B):
            self._to_phase(b, (int(nxt[b]), int(snxt[b])))
            res.append(self.envs[b].step(a[b:b + 1]))
            restarted = self.next_step and self.prev_done[b]  # this step reset the env instead
            self.k[b] = 0 if restarted else self.k[b] + 1
            self.prev_done[b] = bool(res[-1][2][0])
        return tuple(np.concatenate([x[i] for x in res]) for i in range(4))

    def state_bytes(self):
        return [o.state_bytes() for o in self.envs]

    def close(self):
        for o in self.envs:
            o.close()


# id: (B, S, mapping, config kwargs, kernel form expected by default, VecLoadBalanceEnv kwargs,
#      (P, H, wrap, shared), steps before the masked reset of every third env)
CYCLE = (3, 2, True, False)
CASES = {
    "wave-67x4": (67, 4, "auto", {}, "step_wave", None, CYCLE, 10),
    "env-35x8": (35, 8, "env", {}, "env_lane", None, CYCLE, 10),
    "group-19x16": (19, 16, "server", {}, "group", None, CYCLE, 10),
    "group-67x4-alias": (67, 4, "server", ALIAS, "group", None, CYCLE, 10),
    "fused-35x8-fail": (35, 8, "server-fused", {"fail_prob": 0.05}, "fused", None, CYCLE, 10),
    "wave-67x4-shared": (67, 4, "auto", {}, "step_wave", None, (3, 2, True, True), 10),
    "wave-67x4-clamped": (67, 4, "auto", {}, "step_wave", None, (3, 2, False, False), 10),
    "wave-67x3-warmup3-h1": (67, 3, "auto", {"warmup_steps": 3}, "step_wave", None,
                             (3, 1, True, False), 10),
    # envs out of step: the masked reset comes after step 5, mid-cycle
    "wave-67x4-reset-after-5": (67, 4, "auto", {}, "step_wave", None, CYCLE, 5),
    "group-67x4-alias-reset-after-5": (67, 4, "server", ALIAS, "group", None, CYCLE, 5),
    # next-step auto-reset: max_steps = 5 ends the episode inside phase 2 of the cycle
    "wave-67x4-nextstep": (67, 4, "auto", {"max_steps": 5}, "wave_split", NEXT_STEP, CYCLE, 10),
    "env-67x4-nextstep": (67, 4, "env", {"max_steps": 5}, "env_lane", NEXT_STEP, CYCLE, 10),
    "group-67x4-alias-nextstep": (67, 4, "server", {"max_steps": 5, **ALIAS}, "group", NEXT_STEP,
                                  CYCLE, 10),
    # the full group kernel
    # the full group kernel (S = 16: no wave form, so the duration plane's handle runs it)
    "full-19x16-service": (19, 16, "server", {"duration_mode": "service"}, "group", None, CYCLE, 10),
}
FULL = ("full-19x16-service",)
SEED = 1400
HOST_B = 5  # the host-side chain checks run the same configs on fewer envs


def case_ids(case, B=None):
    Bc, S, _, _, _, _, (P, H, wrap, shared), _ = CASES[case]
    return make_ids(Bc if B is None else B, P, len(BANK_SPEC), SEED + S, shared)


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_bit_exact_vs_chained_oracles(lib, oracle_mod, case):
    """Every dynamics form under a per-env trace schedule over the four-trace bank."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, mapping, kw, expect, env_kw, (P, H, wrap, shared), steps = CASES[case]
    idx = list(CASES).index(case)
    kw = {"seed": 1700 + idx, **kw}
    bank, ids = make_bank(), case_ids(case)
    assert len(set(ids.ravel().tolist())) == len(bank) or shared
    ekw = dict(kw)
    if mapping == "server-fused":
        mapping, ekw["step_kernel"] = "server", "fused"
    env = VecLoadBalanceEnv(B, S, device="cuda:0", dyn_mapping=mapping, trace=bank,
                            **{"autoreset": False, **(env_kw or {})}, **ekw)
    ref = TraceOracles(oracle_mod, B, S, kw, bank, ids, H, wrap, next_step=env.next_step)
    if shared:
        env.set_trace_schedule(ids[0], steps_per_phase=H, wrap=wrap)
    else:
        env.set_trace_schedule(torch.from_numpy(ids).to("cuda:0"), steps_per_phase=H, wrap=wrap)

    def hook(e):
        check_kernel(lib, e, mapping, ekw, expect)
        if case in FULL:
            assert lib.launch_names(e.handle).get(0, "").startswith("dynamics_group_full_kernel<")

    parity.run_vs_reference(env, ref, kw, idx, steps=steps, post_steps=14 - steps, hook=hook)
    st = statelayout.parse_cfg(env.get_state(), env.cfg)
    np.testing.assert_array_equal(st["clock"].astype(np.int64), env.cfg.warmup_steps + st["ep_step"])
    assert len(set(st["ep_step"].tolist())) > 1  # the envs are out of step
    np.testing.assert_array_equal(env.trace_phase.cpu().numpy(), ref.phases_next())
    np.testing.assert_array_equal(env.env_trace.cpu().numpy(), ref.ids_next())
    assert ref.handoffs > 2 * B  # the phases did change
    ref.close()
    env.close()


def _child(env_over):
    """This file's S <= 4 cases in a child process (the overrides are read once per process)."""
    ks = [f"test_bit_exact_vs_chained_oracles[{c}]" for c, v in CASES.items()
          if v[1] <= 4 and c not in FULL]  # (a full handle has one kernel form: nothing to force)
    assert len(ks) >= 8
    parity.run_cases_in_child("test_trace_bank.py", ks, env_over)


@gpu
def test_headline_four_lane_groups_bit_exact():
    """LBSIM_DYN_GROUP_LANES=4: the headline kernel (4-lane groups) on the S <= 4 cases."""
    _child({"LBSIM_DYN_GROUP_LANES": "4"})


@gpu
def test_wave_dynamics_bit_exact():
    """LBSIM_DYN_WAVE=1: the one-wave-per-env dynamics on every S <= 4 case it applies to."""
    _child({"LBSIM_DYN_WAVE": "1"})


FLOW_KW = {"warmup_steps": 2}
FLOW_SCALE = 0.1  # the bank at a tenth of the load: no oracle reservoir passes its 128 slots


@gpu
def test_flow_stats_handle(lib, oracle_mod):
    """A flow_stats=True handle (the full group kernel) under a trace schedule: outputs and state
    as above, and statistics equal to those the chained oracles' records imply."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, (P, H, wrap) = 67, 4, (3, 2, True)
    kw = {"seed": 1761, **FLOW_KW}
    bank, ids = make_bank(FLOW_SCALE), make_ids(B, P, len(BANK_SPEC), SEED + 7)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=False, flow_stats=True, trace=bank, **kw)
    ref = TraceOracles(oracle_mod, B, S, kw, bank, ids, H, wrap)
    env.set_trace_schedule(ids, steps_per_phase=H, wrap=wrap)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    count = np.zeros((B, S), np.uint32)
    sum_us = np.zeros((B, S), np.uint64)
    max_us = np.zeros((B, S), np.uint32)
    hist = np.zeros((B, S, flowstats.NBINS), np.uint32)
    c0, _ = oracle_counts(ref)
    rng = np.random.default_rng(61)
    for k in range(14):
        step_both(env, ref, actions(rng, B, S, kw), k)
        c1, rec = oracle_counts(ref)
        assert c1.max() <= K, "the oracle's reservoirs wrapped: lower the load of this test"
        for b, s in zip(*np.nonzero(c1 > c0)):
            v = rec[b, s, c0[b, s]:c1[b, s]].astype(np.int64)
            count[b, s] += v.size
            sum_us[b, s] += np.uint64(v.sum())
            max_us[b, s] = max(int(max_us[b, s]), int(v.max()))
            np.add.at(hist[b, s], flowstats.bin_of(v), 1)
        c0 = c1
    names = lib.launch_names(env.handle)
    kern = lib.load().lbsim_dynamics_kernel(env.handle.h)
    assert kern == GROUP and names.get(0, "").startswith("dynamics_group_full_kernel<"), names
    compare_state(env.handle, ref, env.cfg)
    cnt, sm, mx, h = env.handle.flow_stats(hist=True)
    np.testing.assert_array_equal(cnt.cpu().numpy().view(np.uint32), count)
    np.testing.assert_array_equal(sm.cpu().numpy().view(np.uint64), sum_us)
    np.testing.assert_array_equal(mx.cpu().numpy().view(np.uint32), max_us)
    np.testing.assert_array_equal(h.cpu().numpy().view(np.uint32), hist)
    assert count.sum() > 20 * B
    np.testing.assert_array_equal(env.env_trace.cpu().numpy(), ref.ids_next())
    assert ref.handoffs > 2 * B
    ref.close()
    env.close()


# ------------------------------------------------------------------ equivalences, GPU twins

@gpu
def test_equivalences(lib):
    """A bank of one trace is set_trace; every env on id t is set_trace of trace t; set_env_trace
    is a one-phase schedule; a schedule whose phases all name one id is that constant id;
    clear_trace_schedule, set_trace_bank and set_trace put every env back on trace 0."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, P = 67, 4, 3
    bank = make_bank()
    T = len(bank)
    ids = sample_trace_ids(B, T, seed=3)

    def make(tr):
        return VecLoadBalanceEnv(B, S, device="cuda:0", seed=5, autoreset=False, trace=tr,
                                 server_rates=[40.0, 60.0, 80.0, 100.0])

    single, bank1, plain0, cleared, rebanked = make(bank[0]), make([bank[0]]), make(bank), make(bank), make(bank)
    cleared.set_trace_schedule(make_ids(B, P, T, 1), steps_per_phase=2)
    cleared.clear_trace_schedule()
    rebanked.set_env_trace(ids)
    rebanked.set_trace_bank(trace.TraceBank(bank))
    outs, states = run_twins([single, bank1, plain0, cleared, rebanked])
    for i in range(1, 5):
        assert same(outs[0], outs[i]) and states[0] == states[i], i
    assert not cleared.env_trace.any() and not cleared.trace_phase.any()
    for t in range(T):
        alone, const, sched = make(bank[t]), make(bank), make(bank)
        const.set_env_trace(np.full(B, t))
        sched.set_trace_schedule(np.full((B, P), t), steps_per_phase=2, wrap=False)
        o, s = run_twins([alone, const, sched])
        assert same(o[0], o[1]) and s[0] == s[1], t
        assert same(o[0], o[2]) and s[0] == s[2], t
        assert (const.env_trace == t).all()
        for e in (alone, const, sched):
            e.close()
    per_env, one_phase = make(bank), make(bank)
    per_env.set_env_trace(ids)
    one_phase.set_trace_schedule(ids.numpy()[:, None], steps_per_phase=5)
    o, s = run_twins([per_env, one_phase])
    assert same(o[0], o[1]) and s[0] == s[1]
    assert s[0] != states[0]  # and the selection is read
    assert torch.equal(per_env.env_trace.cpu(), ids)
    # set_trace on a handle with a selection: back to one trace for every env
    per_env.handle.set_trace(bank[0])
    assert not per_env.env_trace.any()
    for e in (single, bank1, plain0, cleared, rebanked, per_env, one_phase):
        e.close()


@gpu
def test_rate_and_trace_schedules_together(lib, oracle_mod):
    """A server-rate schedule (P = 3, H = 2) beside a trace schedule (P = 2, H = 3): each follows
    its own phases, equal to chained oracles that follow both."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S = 35, 4
    bank = make_bank()
    kw = {"seed": 1741}
    ids = make_ids(B, 2, len(bank), SEED + 31)
    srv = server_only_schedule(B, S, 3, bank[0].rate)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=False, trace=bank, **kw)
    ref = TraceOracles(oracle_mod, B, S, kw, bank, ids, 3, True, srv=srv, srv_H=2, srv_wrap=True)
    env.set_rate_schedule(None, srv, steps_per_phase=2, wrap=True)
    env.set_trace_schedule(ids, steps_per_phase=3, wrap=True)
    parity.run_vs_reference(env, ref, kw, 5, steps=10, post_steps=4)
    np.testing.assert_array_equal(env.trace_phase.cpu().numpy(), ref.phases_next())
    np.testing.assert_array_equal(env.rate_phase.cpu().numpy(), ref.srv_phases_next())
    np.testing.assert_array_equal(env.env_trace.cpu().numpy(), ref.ids_next())
    assert ref.handoffs > 2 * B
    ref.close()
    env.close()


# ------------------------------------------------------------------ graphs, shards, errors

@gpu
def test_graph_replay(lib):
    """A step captured after the first set_trace_schedule and replayed across phase boundaries
    equals eager stepping; ids of the same P written between replays are seen without a new
    capture."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, P, H = 67, 4, 3, 2
    bank = make_bank()
    i0, i1 = make_ids(B, P, len(bank), 61), make_ids(B, P, len(bank), 62)
    eager = VecLoadBalanceEnv(B, S, device="cuda:0", seed=8, max_steps=5, trace=bank)
    graph = VecLoadBalanceEnv(B, S, device="cuda:0", seed=8, max_steps=5, trace=bank, graph_mode=True)
    for e in (eager, graph):
        e.set_trace_schedule(i0, steps_per_phase=H)
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
        if k == 7:  # after six replays: new ids of the same shape, no new capture
            for e in (eager, graph):
                e.set_trace_schedule(i1, steps_per_phase=H)
        a_static.copy_(acts[k])
        cg.replay()
        eo, er, ed, _ = eager.step(acts[k])
        assert torch.equal(obs, eo), k
        assert torch.equal(rew, er) and torch.equal(done, ed), k
    assert graph.get_state() == eager.get_state()
    assert torch.equal(graph.env_trace, eager.env_trace)
    assert torch.equal(graph.trace_phase, eager.trace_phase)
    eager.close()
    graph.close()


@gpu
def test_shard_invariance(lib):
    """B = 131 in two uneven shards, each with env_id_offset = lo and its own rows of the ids,
    together equal the full handle."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, P, H = 131, 4, 3, 2
    bank = make_bank()
    ids = make_ids(B, P, len(bank), 54)
    bounds = [0, 47, B]
    full = VecLoadBalanceEnv(B, S, device="cuda:0", seed=9, autoreset=False, trace=bank)
    full.set_trace_schedule(ids, steps_per_phase=H)
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        e = VecLoadBalanceEnv(hi - lo, S, device="cuda:0", seed=9, autoreset=False, trace=bank,
                              env_id_offset=lo)
        e.set_trace_schedule(ids[lo:hi], steps_per_phase=H)
        parts.append(e)
    assert torch.equal(full.reset(), torch.cat([e.reset() for e in parts]))
    rng = np.random.default_rng(B)
    for _ in range(7):
        a = torch.from_numpy(rng.integers(0, 3, (B, S)))
        fo, fr, fd, fi = full.step(a, assign_counts=True)
        po = [e.step(a[lo:hi], assign_counts=True) for e, lo, hi in zip(parts, bounds[:-1], bounds[1:])]
        assert torch.equal(fo, torch.cat([x[0] for x in po]))
        assert torch.equal(fr, torch.cat([x[1] for x in po]))
        assert torch.equal(fd, torch.cat([x[2] for x in po]))
        assert torch.equal(fi["assign_counts"], torch.cat([x[3]["assign_counts"] for x in po]))
    assert torch.equal(full.env_trace, torch.cat([e.env_trace for e in parts]))
    for e in [full, *parts]:
        e.close()


@gpu
def test_multi_agent_forwards_selection(lib):
    from marllb_amd import VecMultiAgentLoadBalanceEnv
    B, A, k = 8, 2, 2
    bank = make_bank()
    ids = make_ids(B, 3, len(bank), 81)
    env = VecMultiAgentLoadBalanceEnv(B, A, k, device="cuda:0", seed=1, trace=bank)
    env.set_trace_schedule(ids, steps_per_phase=2, wrap=False)
    np.testing.assert_array_equal(env.env_trace.cpu().numpy(), ids[:, 0])
    assert not env.trace_phase.any()
    env.set_env_trace(ids[:, 1])
    np.testing.assert_array_equal(env.vec.env_trace.cpu().numpy(), ids[:, 1])
    env.clear_trace_schedule()
    assert not env.env_trace.any()
    env.close()


@gpu
def test_errors(lib):
    """Each rejection returns its code, and a rejected call leaves the selection in force: the
    handle keeps stepping with its twin."""
    import ctypes
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, P, H = 19, 4, 3, 2
    bank = make_bank()
    T = len(bank)
    ids = make_ids(B, P, T, 91)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=3, autoreset=False, trace=bank)
    twin = VecLoadBalanceEnv(B, S, device="cuda:0", seed=3, autoreset=False, trace=bank)
    for e in (env, twin):
        e.set_trace_schedule(ids, steps_per_phase=H)
        e.reset()
    act = torch.from_numpy(np.random.default_rng(0).integers(0, 3, (B, S)))
    for e in (env, twin):
        e.step(act)
    for bad in (-1, T, 2**31 - 1):
        ib = ids.copy()
        ib[7, 1] = bad
        with pytest.raises(ValueError, match="1 id"):
            env.set_trace_schedule(ib, steps_per_phase=H)
        ib[5, 2] = bad
        with pytest.raises(ValueError, match="2 id"):
            env.set_trace_schedule(ib, steps_per_phase=H)
        with pytest.raises(ValueError, match="1 id"):
            env.set_trace_schedule(ib[:, :2], steps_per_phase=H)  # another P: a new table
        with pytest.raises(ValueError, match="1 id"):
            env.set_env_trace(ib[:, 1])
    # shapes and parameters
    with pytest.raises(ValueError, match="expected"):
        env.set_trace_schedule(ids[:-1])
    with pytest.raises(ValueError, match="expected"):
        env.set_env_trace(ids[:-1, 0])
    with pytest.raises(ValueError, match="integers"):
        env.set_trace_schedule(ids.astype(np.float32))
    with pytest.raises(ValueError, match="steps_per_phase"):
        env.set_trace_schedule(ids, steps_per_phase=0)
    with pytest.raises(ValueError, match="phases"):
        env.set_trace_schedule(np.zeros(4097, np.int32))
    h = env.handle
    dev_ids = torch.from_numpy(ids).to("cuda:0")

    def raw(handle, rows, phases, hold):
        return handle.lib.lbsim_set_trace_schedule(handle.h, ctypes.c_void_p(dev_ids.data_ptr()),
                                                   rows, phases, hold, 1, None)

    assert raw(h, 2, P, H) == lib.ESHAPE and raw(h, 0, P, H) == lib.ESHAPE
    assert raw(h, B, 0, H) == lib.EINVAL and raw(h, B, 4097, H) == lib.EINVAL
    assert raw(h, B, P, 0) == lib.EINVAL
    # arrival rates and arrival schedules on a TRACE handle stay ENOTSUP
    with pytest.raises(lib.LbsimError, match="TRACE") as ei:
        env.set_rates(np.full(B, 300.0, np.float32), None)
    assert ei.value.code == lib.ENOTSUP
    with pytest.raises(lib.LbsimError, match="TRACE") as ei:
        env.set_rate_schedule(np.full((B, P), 300.0, np.float32), None)
    assert ei.value.code == lib.ENOTSUP
    # a Poisson handle: EINVAL; a lost-FIN handle: ENOTSUP, but a bank on trace 0 is allowed
    poisson = VecLoadBalanceEnv(B, S, device="cuda:0", seed=3, autoreset=False)
    assert raw(poisson.handle, B, P, H) == lib.EINVAL
    with pytest.raises(ValueError, match="TRACE"):
        poisson.set_trace_bank(bank)
    lost = VecLoadBalanceEnv(B, S, device="cuda:0", seed=3, autoreset=False, trace=bank,
                             lost_fin_prob=0.2, flow_timeout=0.5, lost_fin_pending=8)
    with pytest.raises(lib.LbsimError, match="lost-FIN") as ei:
        lost.set_env_trace(ids[:, 0])
    assert ei.value.code == lib.ENOTSUP
    with pytest.raises(lib.LbsimError, match="lost-FIN") as ei:
        lost.set_trace_schedule(ids, steps_per_phase=H)
    assert ei.value.code == lib.ENOTSUP
    lost.reset()
    lost.step(act)
    assert not lost.env_trace.any()
    # a malformed bank
    begin = np.array([0, 7, 7], np.int64)
    g = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    w = torch.ones(8, dtype=torch.float32, device="cuda:0")

    def raw_bank(b, n):
        return h.lib.lbsim_set_trace_bank(h.h, ctypes.c_void_p(g.data_ptr()),
                                          ctypes.c_void_p(w.data_ptr()),
                                          b.ctypes.data_as(ctypes.c_void_p), n, None)

    assert raw_bank(begin, 2) == lib.EINVAL  # an empty trace
    assert raw_bank(begin, 0) == lib.EINVAL and raw_bank(begin, 4097) == lib.EINVAL
    assert raw_bank(np.array([1, 7], np.int64), 1) == lib.EINVAL
    # the selection set at the start is still the one in force
    assert torch.equal(env.env_trace, twin.env_trace)
    np.testing.assert_array_equal(env.env_trace.cpu().numpy(), ids[:, 0])  # one step done: k = 1
    for _ in range(5):
        x, y = env.step(act, assign_counts=True), twin.step(act, assign_counts=True)
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
        assert torch.equal(x[3]["assign_counts"], y[3]["assign_counts"])
    assert env.get_state() == twin.get_state()
    assert env.trace_phase.cpu().numpy().tolist() == [schedule_phase(6, P, H, True)] * B
    for e in (env, twin, poisson, lost):
        e.close()


# ------------------------------------------------------------------ host (no GPU)

def host_kw(case):
    """The config kwargs, the next-step flag, the schedule and the reset step of a GPU case."""
    if case == "flow-stats":
        return 4, {"seed": 1761, **FLOW_KW}, False, (3, 2, True), 10
    if case == "both-schedules":
        return 4, {"seed": 1741}, False, (2, 3, True), 10
    _, S, _, kw, _, env_kw, (P, H, wrap, _), steps = CASES[case]
    return S, {"seed": 1700 + list(CASES).index(case), **kw}, bool(env_kw), (P, H, wrap), steps


@pytest.mark.parametrize("case", [*CASES, "flow-stats", "both-schedules"])
def test_chain_over_one_trace_equals_unbroken_oracle(oracle_mod, case):
    """The reference's premise, per config: handing an env's state to a new oracle holding the
    SAME trace at every phase change (and at every reset) changes nothing."""
    S, kw, next_step, (P, H, wrap), steps = host_kw(case)
    B = HOST_B
    bank = make_bank(FLOW_SCALE if case == "flow-stats" else 1.0)
    for t in (0, 1):  # the 7-row trace, which wraps inside a step, and the 97-row one
        ids = np.full((B, P), t, np.int32)
        okw = {**kw, "next_step_reset": True} if next_step else kw
        from marllb_amd.env import make_config
        whole = PerEnvOracles.__new__(PerEnvOracles)
        whole.B, whole.S = B, S
        whole.envs = [oracle_mod.OracleEnv(make_config(1, S, env_id_offset=b, trace=bank[0], **okw),
                                           trace=bank[t]) for b in range(B)]
        chain = TraceOracles(oracle_mod, B, S, kw, bank, ids, H, wrap, next_step=next_step)
        np.testing.assert_array_equal(chain.reset(), whole.reset())
        rng = np.random.default_rng(1)
        mask = (np.arange(B) % 3 == 0).astype(np.uint8)
        for k in range(14):
            if k == steps:
                obs = np.zeros((B, S, 11), np.float32)
                np.testing.assert_array_equal(chain.reset(mask=mask, obs=obs),
                                              whole.reset(mask=mask, obs=obs))
            a = actions(rng, B, S, kw)
            for x, y in zip(chain.step(a), whole.step(a)):
                np.testing.assert_array_equal(x, y, err_msg=f"step {k}")
        assert chain.state_bytes() == whole.state_bytes()
        assert chain.handoffs >= 2 * B
        chain.close()
        whole.close()


def test_chained_reference_follows_the_trace(oracle_mod):
    """The reference does depend on the ids: two chains over different ids part ways, and a chain
    whose env changes trace keeps the arrival already drawn."""
    B, S, P, H = 3, 4, 2, 2
    bank = make_bank()
    kw = {"seed": 3}
    a_ids = np.array([[1, 2]] * B, np.int32)
    b_ids = np.array([[1, 3]] * B, np.int32)
    x, y = (TraceOracles(oracle_mod, B, S, kw, bank, i, H, True) for i in (a_ids, b_ids))
    np.testing.assert_array_equal(x.reset(), y.reset())
    act = np.zeros((B, S), np.int64)
    for k in range(2):  # phase 0: the same trace
        for u, v in zip(x.step(act), y.step(act)):
            np.testing.assert_array_equal(u, v)
    before = statelayout.parse(x.envs[0].state_bytes(), 1, S, 32, False)
    # a hand-off keeps the drawn arrival: an oracle of the next trace loads next_arr / next_work,
    # arr_idx and episode as they were
    fresh = x._make(0, (1, 0))
    fresh.load_state(x.envs[0].state_bytes())
    after = statelayout.parse(fresh.state_bytes(), 1, S, 32, False)
    for name in ("next_arr", "next_work", "arr_idx", "episode"):
        np.testing.assert_array_equal(before[name], after[name], err_msg=name)
    fresh.close()
    x.step(act), y.step(act)  # phase 1: traces 2 and 3
    assert x.state_bytes() != y.state_bytes()
    x.close()
    y.close()


def test_trace_bank_concatenation():
    ts = make_bank()
    bank = trace.TraceBank(ts)
    assert len(bank) == 4 and bank.rows == 7 + 97 + 500 + 1031
    np.testing.assert_array_equal(bank.row_begin, [0, 7, 104, 604, 1635])
    assert bank.row_begin.dtype == np.int64
    assert bank.gap_us.dtype == np.uint32 and bank.work.dtype == np.float32
    for t, tr in enumerate(ts):
        lo, hi = bank.row_begin[t], bank.row_begin[t + 1]
        np.testing.assert_array_equal(bank.gap_us[lo:hi], tr.gap_us)
        np.testing.assert_array_equal(bank.work[lo:hi], tr.work)
        assert bank.rate[t] == tr.rate and bank.name[t] == tr.name and bank[t] is tr
    one = trace.TraceBank(ts[0])
    assert len(one) == 1 and one.rows == 7
    with pytest.raises(ValueError):
        trace.TraceBank([])
    with pytest.raises(ValueError):
        trace.TraceBank([ts[0]] * 4097)
    from marllb_amd.env import make_config
    assert make_config(2, 4, trace=ts).arrival_rate == np.float32(ts[0].rate)
    assert make_config(2, 4, trace=bank).arrival_rate == make_config(2, 4, trace=ts[0]).arrival_rate


def test_rescaled():
    t = trace.synthetic(500, 400.0, seed=13)
    for f in (0.5, 1.0, 1.5):
        r = trace.rescaled(t, f)
        np.testing.assert_array_equal(r.gap_us, np.rint(t.gap_us.astype(np.float64) / f).astype(np.uint32))
        np.testing.assert_array_equal(r.work, t.work)
        assert r.rows == t.rows and r.rate == t.rate * f
        assert r.name != t.name or f == 1.0
        assert abs(r.gap_us[1:].astype(np.float64).mean() * f / t.gap_us[1:].mean() - 1.0) < 0.01
    assert trace.rescaled(t, 1.0).gap_us.tobytes() == t.gap_us.tobytes()
    assert trace.rescaled(t, 2.0).work is not t.work
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            trace.rescaled(t, bad)


# sha256 of gap_us then work of trace.synthetic(rows, rate, seed) as it was before it gained its
# work= option (first 16 hex digits)
SYNTHETIC_HASHES = {
    (7, 400, 1): "875fd0a145e14dfd",
    (97, 250, 2): "7673edcf32a9cd90",
    (500, 400, 3): "e4f4cada87a0fdd1",
    (1031, 650, 4): "098bff0008467264",
    (64, 500.0, 0): "60f73ec951a3bb5a",
}


def test_synthetic_defaults_unchanged_and_pareto():
    for (rows, rate, seed), digest in SYNTHETIC_HASHES.items():
        t = trace.synthetic(rows, rate, seed)
        assert hashlib.sha256(t.gap_us.tobytes() + t.work.tobytes()).hexdigest()[:16] == digest
        assert t.name == f"synthetic-{rows}-{rate}"
        u = trace.synthetic(rows, rate, seed, work="lognormal")
        assert u.work.tobytes() == t.work.tobytes()
    p = trace.synthetic(4000, 500.0, seed=2, work="pareto", alpha=1.5, bound=100.0)
    q = trace.synthetic(4000, 500.0, seed=2)
    np.testing.assert_array_equal(p.gap_us, q.gap_us)  # the same arrival times
    assert abs(float(p.work.mean()) - 1.0) < 1e-4 and p.work.min() > 0
    assert p.work.max() / p.work.min() <= 100.0 * (1 + 1e-6)  # bounded
    assert p.work.max() / p.work.min() > 30.0 and np.median(p.work) < 0.7  # heavy-tailed
    assert "pareto" in p.name
    for bad in ({"work": "uniform"}, {"work": "pareto", "alpha": 0.0},
                {"work": "pareto", "bound": 1.0}):
        with pytest.raises(ValueError):
            trace.synthetic(10, 100.0, **bad)


def test_helpers_shapes_seed_and_ranges():
    B, T, P = 300, 4, 24
    ids = sample_trace_ids(B, T, seed=7)
    assert ids.shape == (B,) and ids.dtype == torch.int32
    assert ids.min() == 0 and ids.max() == T - 1
    assert torch.equal(ids, sample_trace_ids(B, T, seed=7))
    assert not torch.equal(ids, sample_trace_ids(B, T, seed=8))
    assert not sample_trace_ids(B, 1, seed=7).any()
    rates = np.array([100.0, 200.0, 300.0, 400.0, 500.0])
    d = diurnal_trace_schedule(rates, P, B, amplitude=(0.3, 0.6), seed=7)
    assert d.shape == (B, P) and d.dtype == torch.int32
    assert d.min() >= 0 and d.max() <= len(rates) - 1
    assert torch.equal(d, diurnal_trace_schedule(rates, P, B, amplitude=(0.3, 0.6), seed=7))
    assert not torch.equal(d, diurnal_trace_schedule(rates, P, B, amplitude=(0.3, 0.6), seed=8))
    # mean 300, swing at least 0.3 * 300 = 90 either way: every env reaches 200 and 400
    assert (d.min(dim=1).values <= 1).all() and (d.max(dim=1).values >= 3).all()
    assert len(set(d.argmax(dim=1).tolist())) > 6  # per-env offsets
    # no amplitude: the trace nearest to the mean, every phase; a fixed phase offset: one row
    flat = diurnal_trace_schedule(rates, P, B, amplitude=(0.0, 0.0), seed=1)
    assert (flat == 2).all()
    fixed = diurnal_trace_schedule(rates, P, B, amplitude=(0.6, 0.6), phase=(0.25, 0.25), seed=1)
    assert (fixed == fixed[0]).all() and fixed[0, 0] == 4  # sin(pi / 2): the peak, 480 -> 500
    assert fixed[0, P // 2] == 0  # and the trough, 120 -> 100
    near = diurnal_trace_schedule([100.0, 1000.0], 8, 5, amplitude=(0.1, 0.1), seed=0)
    assert ((near == 0) | (near == 1)).all()
    for call in (lambda: sample_trace_ids(0, 4), lambda: sample_trace_ids(4, 0),
                 lambda: diurnal_trace_schedule(rates, 0, B),
                 lambda: diurnal_trace_schedule(rates, P, B, amplitude=(0.5, 1.0)),
                 lambda: diurnal_trace_schedule([], P, B),
                 lambda: diurnal_trace_schedule([0.0], P, B)):
        with pytest.raises(ValueError):
            call()


def test_shard_rows():
    from marllb_amd.dist import Shard
    ids = np.arange(12)
    assert Shard(1, 3, 4).rows(ids).tolist() == [4, 5, 6, 7]
    with pytest.raises(ValueError):
        Shard(0, 3, 4).rows(ids[:5])


def test_signature_table_declares_the_exports():
    from marllb_amd import _lib
    declared = _lib.header_functions()
    for name, nargs in (("lbsim_set_trace_bank", 6), ("lbsim_set_trace_schedule", 7),
                        ("lbsim_clear_trace_schedule", 1), ("lbsim_env_trace", 4)):
        assert name in _lib._SIGNATURES and name in declared
        assert len(_lib._SIGNATURES[name][1]) == nargs
