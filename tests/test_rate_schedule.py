"""Rate schedules (lbsim_set_rate_schedule, VecLoadBalanceEnv.set_rate_schedule).

The reference is B chained one-env oracles.  A phase change acts as a mid-run set_rates, so
whenever an env's phase changes its oracle is replaced by one created with the new phase's rates
that loads the old one's state (PerEnvOracles.with_rates does the same for a whole batch); each env
tracks its own episode step and takes its phase from randomize.schedule_phase.  The host tests
first show that such a chain at identical rates equals an unbroken oracle for every config used.
Every GPU comparison is bit for bit: observations, rewards, done flags, assignment counts and the
device state.
"""
import numpy as np
import pytest

from marllb_amd import flowstats
from marllb_amd.randomize import burst_schedule, diurnal_schedule, schedule_phase
from tests import parity, statelayout
from tests.parity import GROUP, actions, compare_state, lib, step_both  # noqa: F401
from tests.test_env_rates import PerEnvOracles, check_kernel, make_rates

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
K = 128


def make_schedule(B, S, P, seed):
    """arrival (B, P) and server (B, P, S) f32: make_rates of another seed for every phase."""
    per = [make_rates(B, S, seed + 101 * j) for j in range(P)]
    return (np.stack([r for r, _ in per], axis=1).copy(),
            np.stack([mu for _, mu in per], axis=1).copy())


class ScheduledOracles:
    """B chained one-env oracles under the schedule arr (B, P) / srv (B, P, S) (None: the rates of
    kw): env b runs the oracle of its phase, handed the previous one's state at every phase change
    (also at a change between two phases of identical rates: the hand-off itself is under test).
    A reset runs at phase 0; with next_step the step after a done is that reset."""

    def __init__(self, oracle_mod, B, S, kw, arr, srv, H, wrap, next_step=False, offset=0):
        self.mod, self.B, self.S, self.kw = oracle_mod, B, S, dict(kw)
        if next_step:
            self.kw["next_step_reset"] = True
        self.arr, self.srv, self.H, self.wrap, self.offset = arr, srv, H, wrap, offset
        self.P = (arr if arr is not None else srv).shape[1]
        self.next_step = next_step
        self.k = np.zeros(B, np.int64)  # steps completed in the episode (the device's ep_step)
        self.phase = np.zeros(B, np.int64)
        self.prev_done = np.zeros(B, bool)
        self.handoffs = 0
        self.envs = [self._make(b, 0) for b in range(B)]

    def _make(self, b, ph):
        from marllb_amd.env import make_config
        rk = {}
        if self.arr is not None:
            rk["arrival_rate"] = float(self.arr[b, ph])
        if self.srv is not None:
            rk["server_rates"] = self.srv[b, ph].tolist()
        cfg = make_config(1, self.S, env_id_offset=self.offset + b, **{**self.kw, **rk})
        return self.mod.OracleEnv(cfg, trace=self.kw.get("trace"))

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
            self._to_phase(b, 0)
            self.k[b], self.prev_done[b] = 0, False
            if mask is None:
                rows.append(self.envs[b].reset())
            else:
                out[b:b + 1] = self.envs[b].reset(mask=np.ones(1, np.uint8), obs=out[b:b + 1].copy())
        return np.concatenate(rows) if mask is None else out

    def phases_next(self):
        """The phase each env's next step runs at (what rate_phase reports)."""
        ph = schedule_phase(self.k, self.P, self.H, self.wrap)
        return np.where(self.next_step & self.prev_done, 0, ph)

    def step(self, a):
        nxt = self.phases_next()
        res = []
        for b in range(self.B):
            self._to_phase(b, int(nxt[b]))
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


ALIAS = {"assign_policy": "alias", "action_type": "continuous"}
NEXT_STEP = {"autoreset": True, "autoreset_mode": "next_step"}
LOST_FIN = {"lost_fin_prob": 0.2, "flow_timeout": 0.5, "lost_fin_pending": 8}
# id: (B, S, mapping, config kwargs, kernel form expected by default, VecLoadBalanceEnv kwargs,
#      (P, H, wrap, shared), steps before the masked reset of every third env)
CYCLE = (3, 2, True, False)
CASES = {
    "wave-67x4": (67, 4, "auto", {}, "step_wave", None, CYCLE, 10),
    "env-35x8": (35, 8, "env", {}, "env_lane", None, CYCLE, 10),
    "group-19x16": (19, 16, "server", {}, "group", None, CYCLE, 10),
    "group-67x4-alias": (67, 4, "server", ALIAS, "group", None, CYCLE, 10),
    "fused-35x8-fail": (35, 8, "server-fused", {"fail_prob": 0.05}, "fused", None, CYCLE, 10),
    "env-67x4-norm": (67, 4, "env", {"normalize_obs": True}, "env_lane", None, CYCLE, 10),
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
}
SEED = 900
HOST_B = 5  # the host-side chain checks run the same configs on fewer envs


def case_schedule(case, B=None):
    Bc, S, _, kw, _, env_kw, (P, H, wrap, shared), _ = CASES[case]
    B = Bc if B is None else B
    arr, srv = make_schedule(B, S, P, SEED + S)
    if shared:  # one schedule for every env: env 0's rows
        arr, srv = np.repeat(arr[:1], B, axis=0), np.repeat(srv[:1], B, axis=0)
    return arr, srv


def drive(env, ref, kw, seed, steps, post, hook=None):
    """parity.run_vs_reference: reset, `steps` steps, the state, a masked reset of every third env,
    `post` more steps, the state (14 steps in all)."""
    return parity.run_vs_reference(env, ref, kw, seed, steps=steps, post_steps=post, hook=hook)


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_bit_exact_vs_chained_oracles(lib, oracle_mod, case):
    """Every dynamics form under a per-env schedule of arrival and server rates."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, mapping, kw, expect, env_kw, (P, H, wrap, shared), steps = CASES[case]
    idx = list(CASES).index(case)
    kw = {"seed": 700 + idx, **kw}
    arr, srv = case_schedule(case)
    ekw = dict(kw)
    if mapping == "server-fused":
        mapping, ekw["step_kernel"] = "server", "fused"
    env = VecLoadBalanceEnv(B, S, device="cuda:0", dyn_mapping=mapping,
                            **{"autoreset": False, **(env_kw or {})}, **ekw)
    ref = ScheduledOracles(oracle_mod, B, S, kw, arr, srv, H, wrap, next_step=env.next_step)
    if shared:
        env.set_rate_schedule(arr[0], torch.from_numpy(srv[0]), steps_per_phase=H, wrap=wrap)
    else:
        env.set_rate_schedule(torch.from_numpy(arr).to("cuda:0"), srv, steps_per_phase=H, wrap=wrap)
    drive(env, ref, kw, idx, steps, 14 - steps, hook=lambda e: check_kernel(lib, e, mapping, ekw, expect))
    # the invariant behind reading the phase from the episode step: every env's clock word is its
    # warm-up plus its episode step (envs are out of step after the masked reset)
    st = statelayout.parse_cfg(env.get_state(), env.cfg)
    np.testing.assert_array_equal(st["clock"].astype(np.int64), env.cfg.warmup_steps + st["ep_step"])
    assert len(set(st["ep_step"].tolist())) > 1
    np.testing.assert_array_equal(env.rate_phase.cpu().numpy(), ref.phases_next())
    assert ref.handoffs > 2 * B  # the phases did change
    ref.close()
    env.close()


def _child(env_over):
    """This file's S <= 4 cases in a child process (the overrides are read once per process)."""
    ks = [f"test_bit_exact_vs_chained_oracles[{c}]" for c, v in CASES.items() if v[1] <= 4]
    assert len(ks) >= 8
    parity.run_cases_in_child("test_rate_schedule.py", ks, env_over)


@gpu
def test_headline_four_lane_groups_bit_exact():
    """LBSIM_DYN_GROUP_LANES=4: the headline 65536 x 4 kernel (4-lane groups) on the S <= 4 cases."""
    _child({"LBSIM_DYN_GROUP_LANES": "4"})


@gpu
def test_wave_dynamics_bit_exact():
    """LBSIM_DYN_WAVE=1: the one-wave-per-env dynamics on every S <= 4 case it applies to."""
    _child({"LBSIM_DYN_WAVE": "1"})


# ------------------------------------------------------------------ flow statistics

FLOW_KW = {"warmup_steps": 2}


def flow_schedule(B, S, P):
    """Light loads (25-55 flows/s): a server's reservoir count stays below its 128 slots over the
    run, so the oracle's records list every completed flow."""
    arr, srv = make_schedule(B, S, P, SEED + 7)
    scale = (np.random.default_rng(5).uniform(25.0, 55.0, (B, P)) / arr).astype(np.float32)
    arr, srv = (arr * scale).astype(np.float32), (srv * scale[:, :, None]).astype(np.float32)
    assert srv.min() >= 1.0
    return arr, srv


def oracle_counts(ref):
    """(reservoir counts (B, S), records (B, S, K) us) of the chained one-env oracles."""
    cnt, rec = [], []
    for o in ref.envs:
        d = statelayout.parse(o.state_bytes(), 1, ref.S, 32, False)
        cnt.append(d["res_count"].astype(np.int64))
        rec.append(d["res_fct"].reshape(ref.S, K))
    return np.stack(cnt), np.stack(rec)


@gpu
def test_flow_stats_handle(lib, oracle_mod):
    """A flow_stats=True handle (the full group kernel) under a schedule: outputs and state as
    above, and statistics equal to those the chained oracles' records imply."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, (P, H, wrap) = 67, 4, (3, 2, True)
    kw = {"seed": 761, **FLOW_KW}
    arr, srv = flow_schedule(B, S, P)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=False, flow_stats=True, **kw)
    ref = ScheduledOracles(oracle_mod, B, S, kw, arr, srv, H, wrap)
    env.set_rate_schedule(arr, srv, steps_per_phase=H, wrap=wrap)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    count = np.zeros((B, S), np.uint32)
    sum_us = np.zeros((B, S), np.uint64)
    max_us = np.zeros((B, S), np.uint32)
    hist = np.zeros((B, S, flowstats.NBINS), np.uint32)
    c0, _ = oracle_counts(ref)
    rng = np.random.default_rng(61)
    for k in range(12):
        step_both(env, ref, actions(rng, B, S, kw), k)
        c1, rec = oracle_counts(ref)
        assert c1.max() <= K, "the oracle's reservoirs wrapped: lower the rates of this test"
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
    ref.close()
    env.close()


# ------------------------------------------------------------------ restricted handles

def restricted(which):
    from marllb_amd import trace
    if which == "lost_fin":
        return dict(LOST_FIN), 400.0, "group"
    kw = {"trace": trace.synthetic(37, 300.0, seed=7)}
    return kw, kw["trace"].rate, "step_wave"


def server_only_schedule(B, S, P, shared_rate):
    """Server schedules whose per-env loads are make_rates's at the handle's own arrival rate."""
    arr, srv = make_schedule(B, S, P, SEED + 13)
    srv = (srv * (shared_rate / arr)[:, :, None]).astype(np.float32)
    assert srv.min() >= 1.0
    return srv


@gpu
@pytest.mark.parametrize("which", ["lost_fin", "trace"])
def test_server_schedule_on_restricted_handles(lib, oracle_mod, which):
    """Lost-FIN and TRACE handles take a server-only schedule; an arrival schedule is ENOTSUP."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, (P, H, wrap) = 35, 4, (3, 2, True)
    rkw, shared_rate, expect = restricted(which)
    kw = {"seed": 741, **rkw}
    srv = server_only_schedule(B, S, P, shared_rate)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=False, **kw)
    ref = ScheduledOracles(oracle_mod, B, S, kw, None, srv, H, wrap)
    arr = np.full((B, P), 300.0, np.float32)
    for a, m in ((arr, None), (arr, srv), (arr[0], None)):
        with pytest.raises(lib.LbsimError, match="lost-FIN" if which == "lost_fin" else "TRACE") as ei:
            env.set_rate_schedule(a, m, steps_per_phase=H)
        assert ei.value.code == lib.ENOTSUP
    assert not env.rate_phase.any()
    env.set_rate_schedule(None, srv, steps_per_phase=H, wrap=wrap)
    drive(env, ref, kw, 5, 10, 4, hook=lambda e: check_kernel(lib, e, "auto", kw, expect))
    assert ref.handoffs > 2 * B
    ref.close()
    env.close()


# ------------------------------------------------------------------ equivalences, by state

def run_twins(envs, steps=8, seed=4):
    """Reset and step the envs on the same actions; returns the (obs, reward, done, assign) lists
    of every env and their final states."""
    B, S = envs[0].num_envs, envs[0].num_servers
    outs = [[e.reset()] for e in envs]
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
    """A one-phase schedule is set_rates; a schedule whose every phase holds the config's rates is
    a plain handle; set_rates after a schedule drops the schedule; so does clear_rate_schedule."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, P = 67, 4, 3
    r, mu = make_rates(B, S, 31)
    arr, srv = make_schedule(B, S, P, 32)
    envs = [VecLoadBalanceEnv(B, S, device="cuda:0", seed=5, autoreset=False) for _ in range(7)]
    plain, rates, one_phase, config_sched, dropped, cleared, sched = envs
    cfg = plain.cfg
    rates.set_rates(r, mu)
    one_phase.set_rate_schedule(r[:, None], mu[:, None, :], steps_per_phase=3)
    config_sched.set_rate_schedule(np.full(P, cfg.arrival_rate, np.float32),
                                   np.tile(np.array(cfg.server_rate[:S], np.float32), (P, 1)))
    dropped.set_rate_schedule(arr, srv)
    dropped.set_rates(r, mu)
    cleared.set_rate_schedule(arr, srv)
    cleared.clear_rate_schedule()
    sched.set_rate_schedule(arr, srv)
    outs, states = run_twins(envs)
    assert same(outs[1], outs[2]) and states[1] == states[2]  # P = 1 == set_rates
    assert same(outs[0], outs[3]) and states[0] == states[3]  # the config's rates == plain
    assert same(outs[1], outs[4]) and states[1] == states[4]  # set_rates dropped the schedule
    assert same(outs[0], outs[5]) and states[0] == states[5]  # cleared == plain
    assert not dropped.rate_phase.any() and not cleared.rate_phase.any()
    # and the schedule is read: it differs from its own phase-0 rates held constant
    phase0 = VecLoadBalanceEnv(B, S, device="cuda:0", seed=5, autoreset=False)
    phase0.set_rates(arr[:, 0], srv[:, 0])
    o0, s0 = run_twins([phase0])
    assert torch.equal(o0[0][0], outs[6][0]) and torch.equal(o0[0][1], outs[6][1])  # reset, step 0
    assert s0[0] != states[6]
    np.testing.assert_array_equal(sched.rate_phase.cpu().numpy(), np.full(B, 8 % P))
    for e in [*envs, phase0]:
        e.close()


@gpu
def test_null_argument_keeps_the_rates_in_force(lib):
    """server=None keeps the per-env server rates set before (constant over the phases) and
    arrival=None the arrival rates: equal to the schedule with those rates written out."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, P = 35, 4, 3
    r, mu = make_rates(B, S, 33)
    arr, srv = make_schedule(B, S, P, 34)
    envs = [VecLoadBalanceEnv(B, S, device="cuda:0", seed=6, autoreset=False) for _ in range(4)]
    a_null, a_full, s_null, s_full = envs
    a_null.set_rates(r, mu)
    a_null.set_rate_schedule(arr, None, steps_per_phase=2)
    a_full.set_rate_schedule(arr, np.repeat(mu[:, None, :], P, axis=1), steps_per_phase=2)
    s_null.set_rates(r, mu)
    s_null.set_rate_schedule(None, srv, steps_per_phase=2)
    s_full.set_rate_schedule(np.repeat(r[:, None], P, axis=1), srv, steps_per_phase=2)
    outs, states = run_twins(envs)
    assert same(outs[0], outs[1]) and states[0] == states[1]
    assert same(outs[2], outs[3]) and states[2] == states[3]
    assert states[0] != states[2]
    for e in envs:
        e.close()


# ------------------------------------------------------------------ graphs, shards, accessors

@gpu
def test_graph_replay(lib):
    """One captured step replayed 12 times equals eager stepping, each env at its own phase; a
    schedule of the same P written between replays is seen without a new capture."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, P, H = 67, 4, 3, 2
    a0, s0 = make_schedule(B, S, P, 61)
    a1, s1 = make_schedule(B, S, P, 62)
    eager = VecLoadBalanceEnv(B, S, device="cuda:0", seed=8, max_steps=5)
    graph = VecLoadBalanceEnv(B, S, device="cuda:0", seed=8, max_steps=5, graph_mode=True)
    for e in (eager, graph):
        e.set_rate_schedule(a0, s0, steps_per_phase=H)
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
        if k == 7:  # after six replays: new tables of the same shape, no new capture
            for e in (eager, graph):
                e.set_rate_schedule(a1, s1, steps_per_phase=H)
        a_static.copy_(acts[k])
        cg.replay()
        eo, er, ed, _ = eager.step(acts[k])
        assert torch.equal(obs, eo), k
        assert torch.equal(rew, er) and torch.equal(done, ed), k
    assert graph.get_state() == eager.get_state()
    assert torch.equal(graph.rate_phase, eager.rate_phase)
    eager.close()
    graph.close()


@gpu
def test_shard_invariance(lib):
    """B = 200 in three uneven shards, each with env_id_offset = lo and its own rows of the
    schedule, together equal the full handle."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, P, H = 200, 4, 3, 2
    arr, srv = make_schedule(B, S, P, 54)
    rng = np.random.default_rng(B)
    cuts = np.sort(rng.choice(np.arange(1, B), 2, replace=False))
    bounds = [0, *cuts.tolist(), B]
    full = VecLoadBalanceEnv(B, S, device="cuda:0", seed=9, autoreset=False)
    full.set_rate_schedule(arr, srv, steps_per_phase=H)
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        e = VecLoadBalanceEnv(hi - lo, S, device="cuda:0", seed=9, autoreset=False, env_id_offset=lo)
        e.set_rate_schedule(arr[lo:hi], srv[lo:hi], steps_per_phase=H)
        parts.append(e)
    assert torch.equal(full.reset(), torch.cat([e.reset() for e in parts]))
    for _ in range(7):
        a = torch.from_numpy(rng.integers(0, 3, (B, S)))
        fo, fr, fd, fi = full.step(a, assign_counts=True)
        po = [e.step(a[lo:hi], assign_counts=True) for e, lo, hi in zip(parts, bounds[:-1], bounds[1:])]
        assert torch.equal(fo, torch.cat([x[0] for x in po]))
        assert torch.equal(fr, torch.cat([x[1] for x in po]))
        assert torch.equal(fd, torch.cat([x[2] for x in po]))
        assert torch.equal(fi["assign_counts"], torch.cat([x[3]["assign_counts"] for x in po]))
    for e in [full, *parts]:
        e.close()


@gpu
@pytest.mark.parametrize("wrap", [True, False])
def test_rate_phase_and_rates_out_of_step(lib, wrap):
    """rate_phase and rates of a scheduled handle whose envs are at different episode steps equal
    schedule_phase of each env's step and that phase's rows of the tables."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, P, H = 67, 4, 3, 2
    arr, srv = make_schedule(B, S, P, 71)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=3, autoreset=False)
    env.set_rate_schedule(arr, srv, steps_per_phase=H, wrap=wrap)
    env.reset()
    k = np.zeros(B, np.int64)
    a = torch.zeros((B, S), dtype=torch.int64)
    rows = np.arange(B)
    for step in range(9):
        if step in (3, 4, 7):  # masked resets put the envs out of step
            mask = (rows % 3 == step % 3).astype(np.uint8)
            env.reset(mask=torch.from_numpy(mask))
            k[mask != 0] = 0
        ph = schedule_phase(k, P, H, wrap)
        np.testing.assert_array_equal(env.rate_phase.cpu().numpy(), ph)
        ra, rm = env.rates
        np.testing.assert_array_equal(ra.cpu().numpy(), arr[rows, ph])
        np.testing.assert_array_equal(rm.cpu().numpy(), srv[rows, ph])
        env.step(a)
        k += 1
    assert len(set(k.tolist())) > 2
    st = statelayout.parse_cfg(env.get_state(), env.cfg)
    np.testing.assert_array_equal(st["ep_step"], k)
    env.close()


@gpu
def test_multi_agent_forwards_schedule(lib):
    from marllb_amd import VecMultiAgentLoadBalanceEnv
    B, A, k, P = 8, 2, 2, 3
    arr, srv = make_schedule(B, A * k, P, 81)
    env = VecMultiAgentLoadBalanceEnv(B, A, k, device="cuda:0", seed=1)
    env.set_rate_schedule(arr, srv, steps_per_phase=2, wrap=False)
    np.testing.assert_array_equal(env.rates[0].cpu().numpy(), arr[:, 0])
    np.testing.assert_array_equal(env.vec.rates[1].cpu().numpy(), srv[:, 0])
    assert not env.rate_phase.any()
    env.clear_rate_schedule()
    assert (env.rates[0].cpu().numpy() == np.float32(env.vec.cfg.arrival_rate)).all()
    env.close()


@gpu
def test_errors(lib):
    """A rejected call leaves the schedule in force: the handle keeps stepping with its twin."""
    import ctypes
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, P, H = 19, 4, 3, 2
    arr, srv = make_schedule(B, S, P, 91)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=3, autoreset=False)
    twin = VecLoadBalanceEnv(B, S, device="cuda:0", seed=3, autoreset=False)
    for e in (env, twin):
        e.set_rate_schedule(arr, srv, steps_per_phase=H)
        e.reset()
    act = torch.from_numpy(np.random.default_rng(0).integers(0, 3, (B, S)))
    for e in (env, twin):
        e.step(act)
    for bad in (0.0, float("nan"), 1e9):
        ab, sb = arr.copy(), srv.copy()
        ab[7, 1] = bad
        with pytest.raises(ValueError, match="1 value"):
            env.set_rate_schedule(ab, None, steps_per_phase=H)
        sb[5, 2, 3] = bad
        with pytest.raises(ValueError, match="2 value"):
            env.set_rate_schedule(ab, sb, steps_per_phase=H)
        with pytest.raises(ValueError, match="1 value"):
            env.set_rate_schedule(None, sb[:, 1:], steps_per_phase=H)  # another P: a new table
        with pytest.raises(ValueError, match="1 value"):
            env.set_rates(ab[:, 1], None)  # a rejected set_rates keeps the schedule too
    # shapes and parameters
    with pytest.raises(ValueError, match="arrival"):
        env.set_rate_schedule(arr[:-1], None)
    with pytest.raises(ValueError, match="server"):
        env.set_rate_schedule(None, srv[:, :, :-1])
    with pytest.raises(ValueError, match="phases"):
        env.set_rate_schedule(arr, srv[:, :2])
    with pytest.raises(ValueError, match="arrival and / or server"):
        env.set_rate_schedule()
    with pytest.raises(ValueError, match="steps_per_phase"):
        env.set_rate_schedule(arr, srv, steps_per_phase=0)
    with pytest.raises(ValueError, match="phases"):
        env.set_rate_schedule(np.full(4097, 300.0, np.float32), None)
    h = env.handle
    dev_arr = torch.from_numpy(arr).to("cuda:0")

    def raw(rows, phases, hold):
        return h.lib.lbsim_set_rate_schedule(h.h, ctypes.c_void_p(dev_arr.data_ptr()), None, rows,
                                             phases, hold, 1, None)

    assert raw(2, P, H) == lib.ESHAPE and raw(0, P, H) == lib.ESHAPE
    assert raw(B, 0, H) == lib.EINVAL and raw(B, 4097, H) == lib.EINVAL
    assert raw(B, P, 0) == lib.EINVAL
    # the schedule set at the start is still the one in force
    np.testing.assert_array_equal(env.rate_phase.cpu().numpy(), twin.rate_phase.cpu().numpy())
    np.testing.assert_array_equal(env.rates[0].cpu().numpy(), arr[:, 0])  # one step done: k = 1
    for _ in range(5):
        x, y = env.step(act, assign_counts=True), twin.step(act, assign_counts=True)
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
        assert torch.equal(x[3]["assign_counts"], y[3]["assign_counts"])
    assert env.get_state() == twin.get_state()
    assert env.rate_phase.cpu().numpy().tolist() == [schedule_phase(6, P, H, True)] * B
    env.close()
    twin.close()


# ------------------------------------------------------------------ host (no GPU)

def host_kw(case):
    """The config kwargs and the next-step flag of a GPU case above."""
    if case in CASES:
        _, S, _, kw, _, env_kw, (P, H, wrap, _), steps = CASES[case]
        return S, {"seed": 700 + list(CASES).index(case), **kw}, bool(env_kw), (P, H, wrap), steps
    if case == "flow-stats":
        return 4, {"seed": 761, **FLOW_KW}, False, (3, 2, True), 10
    rkw, _, _ = restricted(case)
    return 4, {"seed": 741, **rkw}, False, (3, 2, True), 10


@pytest.mark.parametrize("case", [*CASES, "flow-stats", "lost_fin", "trace"])
def test_chain_at_identical_rates_equals_unbroken_oracle(oracle_mod, case):
    """The reference's premise, per config: handing an env's state to a new oracle of the SAME
    rates at every phase change (and at every reset) changes nothing."""
    S, kw, next_step, (P, H, wrap), steps = host_kw(case)
    B = HOST_B
    r, mu = make_rates(B, S, SEED + S)
    if "lost_fin_prob" in kw or "trace" in kw:  # (no per-env arrival rates on these)
        shared = 400.0 if "lost_fin_prob" in kw else kw["trace"].rate
        mu, r = (mu * (shared / r)[:, None]).astype(np.float32), None
    arr = None if r is None else np.repeat(r[:, None], P, axis=1)
    srv = np.repeat(mu[:, None, :], P, axis=1)
    okw = {**kw, "next_step_reset": True} if next_step else kw
    whole = PerEnvOracles(oracle_mod, B, S, okw, r, mu)
    chain = ScheduledOracles(oracle_mod, B, S, kw, arr, srv, H, wrap, next_step=next_step)
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
    assert chain.handoffs >= 2 * B  # (a clamped schedule: two changes per env, then none)
    chain.close()
    whole.close()


def test_schedule_phase_edges():
    assert [schedule_phase(k, 3, 1, True) for k in range(7)] == [0, 1, 2, 0, 1, 2, 0]
    assert [schedule_phase(k, 3, 1, False) for k in range(7)] == [0, 1, 2, 2, 2, 2, 2]
    assert [schedule_phase(k, 3, 2, True) for k in range(8)] == [0, 0, 1, 1, 2, 2, 0, 0]
    assert [schedule_phase(k, 3, 2, False) for k in range(8)] == [0, 0, 1, 1, 2, 2, 2, 2]
    assert [schedule_phase(k, 1, 5, w) for k in (0, 4, 5, 99) for w in (True, False)] == [0] * 8
    assert schedule_phase(-1, 3, 2, True) == 0 and schedule_phase(-7, 3, 2, False) == 0
    assert schedule_phase(2**31 - 1, 4096, 1, True) == (2**31 - 1) % 4096
    assert schedule_phase(2**31 - 1, 4096, 7, False) == 4095
    k = np.array([-1, 0, 1, 5, 6, 11, 12])
    np.testing.assert_array_equal(schedule_phase(k, 3, 2, True), [0, 0, 0, 2, 0, 2, 0])
    np.testing.assert_array_equal(schedule_phase(k, 3, 2, False), [0, 0, 0, 2, 2, 2, 2])
    t = schedule_phase(torch.from_numpy(k), 3, 2, True)
    assert t.tolist() == [0, 0, 0, 2, 0, 2, 0]
    for bad in ((0, 1), (3, 0)):
        with pytest.raises(ValueError):
            schedule_phase(1, *bad)


def test_schedule_helpers_shapes_seed_and_ranges():
    B, P = 300, 24
    base = torch.linspace(50.0, 2000.0, B)
    g = torch.Generator()
    g.manual_seed(7)
    d = diurnal_schedule(base, P, amplitude=(0.2, 0.8), generator=g)
    b = burst_schedule(base, P, factor=4.0, p_on=0.2, p_off=0.5, generator=g)
    for t in (d, b):
        assert t.shape == (B, P) and t.dtype == torch.float32
        assert t.min() >= 0.1 and t.max() <= 1.0e6
    rel = d.double() / base.double()[:, None]
    assert rel.min() >= 0.2 - 1e-6 and rel.max() <= 1.8 + 1e-6
    swing = rel.max(dim=1).values - rel.min(dim=1).values
    assert swing.min() > 0.3 and swing.max() > 1.2  # every env moves; amplitudes differ
    assert torch.allclose(rel.mean(dim=1), torch.ones(B, dtype=torch.float64), atol=1e-6)
    assert len(set(rel.argmax(dim=1).tolist())) > 6  # per-env offsets
    on = b != base[:, None]
    assert not on[:, 0].any()  # phase 0, the phase of a reset, is calm
    assert torch.equal(b[on], (base[:, None] * 4.0).expand(B, P)[on])
    frac = on[:, 1:].double().mean().item()
    assert 0.15 < frac < 0.40  # the chain's stationary share of bursts is 0.2 / 0.7 = 0.29
    g.manual_seed(7)
    assert torch.equal(d, diurnal_schedule(base, P, amplitude=(0.2, 0.8), generator=g))
    assert torch.equal(b, burst_schedule(base, P, factor=4.0, p_on=0.2, p_off=0.5, generator=g))
    assert not torch.equal(d, diurnal_schedule(base, P, amplitude=(0.2, 0.8), generator=g))
    # clamped to the valid range, never out of it
    top = burst_schedule(torch.tensor([9.0e5]), 50, factor=10.0, p_on=1.0, p_off=0.0, generator=g)
    assert top.max() == 1.0e6 and top[0, 0] == 9.0e5
    assert diurnal_schedule(torch.tensor([0.1]), 8, amplitude=(0.9, 0.9), generator=g).min() >= 0.1
    for call in (lambda: diurnal_schedule(base, P, amplitude=(0.5, 1.0)),
                 lambda: diurnal_schedule(base, 0),
                 lambda: diurnal_schedule(torch.tensor([0.0]), 4),
                 lambda: burst_schedule(base, P, p_on=1.5),
                 lambda: burst_schedule(base, P, factor=0.0)):
        with pytest.raises(ValueError):
            call()


def test_signature_table_declares_the_exports():
    from marllb_amd import _lib
    declared = _lib.header_functions()
    for name, nargs in (("lbsim_set_rate_schedule", 8), ("lbsim_clear_rate_schedule", 1),
                        ("lbsim_rate_phase", 3)):
        assert name in _lib._SIGNATURES and name in declared
        assert len(_lib._SIGNATURES[name][1]) == nargs
