"""The flow dynamics against an independent event simulator (tests/flowsim_ref.py), exactly.

Every other dynamics test compares a kernel with oracle/lbsim_oracle.c, which was written beside
the kernels and shares their construction (int32 times relative to the step start, rebased every
step; a ring per server; one drawn arrival carried across steps).  The reference here is written
from DESIGN.md §3.2, §3.3, §3.6 and §3.7 in absolute int64 us with plain lists, so a misreading
of the text that the oracle and the kernels share does not pass.

One scenario per case, the same for every check: reset, 6 steps, a masked reset of every third
env (their episode 2), 6 more steps.  The rates keep every reservoir count at or below 128, so
Algorithm R has put completion c into slot c and the records [c0, c1) of a step list its
completions in order (asserted).  Not gpu: the reference against the oracle.  gpu: against plain
handles under every dyn_mapping through their state, and against a flow_stats handle through its
exact count / sum / maximum / histogram after every step.
"""
import numpy as np
import pytest

from marllb_amd import flowstats, trace
from marllb_amd.env import make_config
from tests import statelayout
from tests.flowsim_ref import FlowSim
from tests.parity import lib  # noqa: F401  (the fixture: fails a gpu test run without a device)
from tests.test_parity_coverage import window

K = 128
STEPS, RESET_AT = 12, 6
CONT = {"action_type": "continuous"}
# id: (S, config kwargs, what the case must reach)
CASES = {
    "s1-default": (1, {"arrival_rate": 20.0, "server_rates": [40.0], "warmup_steps": 4}, ()),
    "s1-q3-drops": (1, {"arrival_rate": 30.0, "server_rates": [20.0], "queue_capacity": 3,
                        "warmup_steps": 2}, ("drops",)),
    "s3-lsq-q6-overload": (3, {"assign_policy": "lsq", "queue_capacity": 6, "arrival_rate": 60.0,
                               "load": 1.3, "warmup_steps": 2}, ("drops",)),
    "s4-sed-levels": (4, {"discrete_weights": [0.5, 1.0, 8.0], "arrival_rate": 60.0,
                          "warmup_steps": 2}, ()),
    "s4-sed-continuous": (4, {**CONT, "arrival_rate": 60.0, "warmup_steps": 2}, ()),
    "s5-lsq2-unequal": (5, {"assign_policy": "lsq2", "arrival_rate": 70.0, "warmup_steps": 2,
                            "server_rates": [10.0, 15.0, 20.0, 30.0, 40.0]}, ()),
    "s8-sed2-rate500": (8, {"assign_policy": "sed2", "arrival_rate": 500.0, "warmup_steps": 4,
                            "step_interval": 0.05}, ()),
    "s4-alias-zero-level": (4, {"assign_policy": "alias", "discrete_weights": [0.0, 1.0, 3.0],
                                "arrival_rate": 60.0, "warmup_steps": 2}, ("drops", "zero-rows")),
    "s6-alias-continuous": (6, {"assign_policy": "alias", **CONT, "min_weight": 0.0,
                                "arrival_rate": 90.0, "warmup_steps": 2}, ()),
    "s16-lsq-continuous": (16, {"assign_policy": "lsq", **CONT, "arrival_rate": 160.0,
                                "warmup_steps": 2}, ()),
    "s20-sed2": (20, {"assign_policy": "sed2", "arrival_rate": 200.0, "warmup_steps": 2}, ()),
    "s8-trace37": (8, {"_trace": True, "warmup_steps": 2, "step_interval": 0.1}, ()),
    "s4-q64-deep": (4, {"queue_capacity": 64, "arrival_rate": 200.0, "server_rates": [40.0] * 4,
                        "warmup_steps": 2, "step_interval": 0.15}, ("deep",)),
    # node.c:442-460 takes the alias only if the fraction EXCEEDS odd[bucket].  Weights (1, 3)
    # give odd[0] = 0.5 in f32, and under seed 7113 arrival 25 of global env 93407 (local env 5)
    # draws the hash word 0x400000f2: U = 0.25, rn = 0.5 exactly.  Found by a search over Philox
    # counters; the case asserts that the reference met the tie.
    "s2-alias-tie": (2, {"assign_policy": "alias", "discrete_weights": [1.0, 3.0],
                         "arrival_rate": 40.0, "warmup_steps": 0, "seed": 7113,
                         "env_id_offset": 93402},
                     ("tie",)),
}


def config_kwargs(case):
    S, kw, _ = CASES[case]
    kw = {"seed": 7100 + list(CASES).index(case), **kw}
    if kw.pop("_trace", False):
        kw["trace"] = trace.synthetic(37, 300.0, seed=7)
    return S, kw


def actions_of(case, B):
    """The action batch of every step, drawn once per case."""
    S, kw = config_kwargs(case)
    rng = np.random.default_rng(list(CASES).index(case))
    out = []
    for k in range(STEPS):
        if kw.get("action_type") == "continuous":
            a = rng.uniform(-1.0, 11.0, (B, S)).astype(np.float32)
        else:
            n = len(kw.get("discrete_weights", [1.0, 1.5, 2.0]))
            a = rng.integers(-n, n, (B, S)).astype(np.int64)
            if "zero-rows" in CASES[case][2] and k % 3 == 1:
                a[k % 5::5] = 0  # every server at the level 0.0: no active server
            if "tie" in CASES[case][2]:
                a[:] = [0, 1]  # weights (1, 3) in every env and step
        out.append(a)
    return out


def weights_of(a, kw):
    """a level by Python list indexing, or the f32 clip."""
    if kw.get("action_type") == "continuous":
        lo, hi = kw.get("min_weight", 0.1), kw.get("max_weight", 10.0)
        return np.clip(a, np.float32(lo), np.float32(hi))
    levels = [np.float32(x) for x in kw.get("discrete_weights", [1.0, 1.5, 2.0])]
    return np.array([[levels[int(i)] for i in row] for row in a], np.float32)


class Event:
    """What the reference says the state is after a reset (mask: the envs reset) or a step."""

    def __init__(self, B, S):
        self.mask = None
        self.assigned = np.zeros((B, S), np.int64)
        self.new = [[([], []) for _ in range(S)] for _ in range(B)]  # (fct us, tc us) completed


_RUNS = {}


def reference_run(case, B):
    """The scenario on B reference envs -> (config, its kwargs, the actions of every step, the
    Events).  Computed once per (case, B) and shared by the tests."""
    if (case, B) in _RUNS:
        return _RUNS[(case, B)]
    S, kw = config_kwargs(case)
    cfg = make_config(B, S, **kw)
    sims = [FlowSim(kw["seed"], cfg.env_id_offset + b, S, cfg.queue_capacity,
                    kw.get("assign_policy", "sed"), cfg.arrival_rate,
                    [cfg.server_rate[s] for s in range(S)],
                    dt=cfg.step_interval, warmup_steps=cfg.warmup_steps, trace=kw.get("trace"))
            for b in range(B)]
    drops = np.zeros(B, np.int64)
    acts = actions_of(case, B)
    events = []

    def snapshot(ev):
        ev.dropped = drops.copy()
        ev.in_flight = np.array([m.in_flight() for m in sims])
        ev.arr_idx = np.array([m.k for m in sims])
        ev.next_abs = np.array([m.next_arrival() for m in sims])
        ev.steps = np.array([m.step_no for m in sims])
        events.append(ev)

    def reset(mask):
        ev = Event(B, S)
        ev.mask = mask
        for b in np.flatnonzero(mask):
            drops[b] = 0
            for r in sims[b].reset():  # the warm-up's flows are records and drops like any other
                drops[b] += r.dropped
                for s in range(S):
                    ev.new[b][s][0].extend(r.fct(s))
                    ev.new[b][s][1].extend(r.tc(s))
        snapshot(ev)

    reset(np.ones(B, bool))
    for k in range(STEPS):
        if k == RESET_AT:
            reset(np.arange(B) % 3 == 0)
        w = weights_of(acts[k], kw)
        ev = Event(B, S)
        for b in range(B):
            r = sims[b].step(w[b])
            ev.assigned[b] = r.assigned
            drops[b] += r.dropped
            ev.new[b] = [(r.fct(s), r.tc(s)) for s in range(S)]
        snapshot(ev)
    events[-1].alias_ties = sum(m.alias_ties for m in sims)
    _RUNS[(case, B)] = (cfg, kw, acts, events)
    return _RUNS[(case, B)]


def drive(case, B, backend, check):
    """The scenario on `backend` (reset(mask or None), step(a) -> assign counts): check(event,
    assign or None) after every reset and step."""
    cfg, kw, acts, events = reference_run(case, B)
    it = iter(events)
    backend.reset(None)
    check(next(it), None)
    for k in range(STEPS):
        if k == RESET_AT:
            backend.reset((np.arange(B) % 3 == 0).astype(np.uint8))
            check(next(it), None)
        check(next(it), backend.step(acts[k]))
    return events


class StateCheck:
    """An Event against a state snapshot (the oracle's or a handle's: one layout)."""

    def __init__(self, cfg, read):
        self.cfg, self.read = cfg, read
        self.B, self.S = cfg.num_envs, cfg.num_servers
        self.dt = int(round(cfg.step_interval * 1e6))
        self.count = np.zeros((self.B, self.S), np.int64)
        self.peak = self.deepest = 0

    def __call__(self, ev, assign):
        B, S = self.B, self.S
        d = statelayout.parse_cfg(self.read(), self.cfg)
        if assign is not None:
            np.testing.assert_array_equal(assign, ev.assigned, err_msg="assignments")
        np.testing.assert_array_equal(d["dropped"], ev.dropped, err_msg="dropped")
        queued = (d["hc"].reshape(B, S) >> 16).astype(np.int64)
        np.testing.assert_array_equal(queued, ev.in_flight, err_msg="flows in flight")
        np.testing.assert_array_equal(d["arr_idx"], ev.arr_idx, err_msg="arrival index")
        np.testing.assert_array_equal(d["clock"], ev.steps, err_msg="clock")
        next_abs = d["next_arr"].astype(np.int64) + ev.steps * self.dt
        np.testing.assert_array_equal(next_abs, ev.next_abs, err_msg="next arrival")
        c1 = d["res_count"].reshape(B, S).astype(np.int64)
        fct, ts = d["res_fct"].reshape(B, S, K), d["res_ts"].reshape(B, S, K)
        if ev.mask is not None:
            self.count[ev.mask] = 0
        self.peak = max(self.peak, int(c1.max()))
        assert self.peak <= K, "a reservoir wrapped: its records no longer list every flow"
        self.deepest = max(self.deepest, int(queued.max()))
        for b in range(B):
            for s in range(S):
                want_fct, want_tc = ev.new[b][s]
                c0 = int(self.count[b, s])
                assert int(c1[b, s]) == c0 + len(want_fct), ("completions", b, s)
                if want_fct:
                    assert fct[b, s, c0:c1[b, s]].tolist() == want_fct, ("fct records", b, s)
                    assert ts[b, s, c0:c1[b, s]].tolist() == [t // 1000 for t in want_tc], (
                        "record timestamps", b, s)
        self.count = c1


def check_reaches(case, events, deepest, B):
    """The case is not vacuous."""
    S, reach = CASES[case][0], CASES[case][2]
    recorded = sum(len(ev.new[b][s][0]) for ev in events if ev.mask is None
                   for b in range(B) for s in range(S))
    assert recorded > 20 * B, recorded
    assert any(ev.mask is not None and not ev.mask.all() for ev in events)  # episode 2 was run
    if "drops" in reach:
        assert events[-1].dropped.sum() > 0
    if "zero-rows" in reach:
        idle = [ev for ev in events if ev.mask is None and (ev.assigned.sum(1) == 0).any()]
        assert idle  # some env had no active server for a whole step
    if "tie" in reach:
        assert events[-1].alias_ties >= 1
    if "deep" in reach:
        assert deepest > window(S), deepest


class OracleBackend:
    def __init__(self, oracle_mod, cfg, kw):
        self.ora = oracle_mod.OracleEnv(cfg, threads=2, trace=kw.get("trace"))

    def reset(self, mask):
        self.ora.reset(mask=mask)

    def step(self, a):
        return self.ora.step(a)[3]


HOST_B = 12


@pytest.mark.parametrize("case", list(CASES))
def test_reference_equals_the_oracle(oracle_mod, case):
    cfg, kw, _, _ = reference_run(case, HOST_B)
    back = OracleBackend(oracle_mod, cfg, kw)
    chk = StateCheck(cfg, back.ora.state_bytes)
    events = drive(case, HOST_B, back, chk)
    check_reaches(case, events, chk.deepest, HOST_B)
    back.ora.close()


# ------------------------------------------------------------------ the device

gpu = pytest.mark.gpu
GPU_B = 67  # odd, and more than one wave of 4-lane groups


class DeviceBackend:
    def __init__(self, S, kw, **extra):
        import torch
        from marllb_amd.env import VecLoadBalanceEnv
        self.torch = torch
        self.env = VecLoadBalanceEnv(GPU_B, S, device="cuda:0", autoreset=False, **extra, **kw)

    def reset(self, mask):
        self.env.reset(mask=None if mask is None else self.torch.from_numpy(mask))

    def step(self, a):
        info = self.env.step(self.torch.from_numpy(a), assign_counts=True)[3]
        return info["assign_counts"].cpu().numpy()


# (one lane per env takes at most 16 servers: make_config refuses S = 20 under "env")
PLAIN = [(c, m) for c in CASES for m in ("auto", "env", "server")
         if m != "env" or CASES[c][0] <= 16]


@gpu
@pytest.mark.parametrize("case,mapping", PLAIN)
def test_plain_handles_equal_the_reference(lib, case, mapping):
    S, kw = config_kwargs(case)
    back = DeviceBackend(S, kw, dyn_mapping=mapping)
    chk = StateCheck(back.env.cfg, back.env.handle.state_bytes)
    events = drive(case, GPU_B, back, chk)
    check_reaches(case, events, chk.deepest, GPU_B)
    back.env.close()


class StatsCheck:
    """An Event against a flow_stats handle: the exact statistics of every flow completed by a
    step (a reset's warm-up counts nothing), and the counts that need no reservoir."""

    def __init__(self, env):
        B, S = env.cfg.num_envs, env.cfg.num_servers
        self.env, self.B, self.S = env, B, S
        self.count = np.zeros((B, S), np.uint32)
        self.sum_us = np.zeros((B, S), np.uint64)
        self.max_us = np.zeros((B, S), np.uint32)
        self.hist = np.zeros((B, S, flowstats.NBINS), np.uint32)
        self.peak = 0

    def __call__(self, ev, assign):
        env = self.env
        d = statelayout.parse_cfg(env.handle.state_bytes(), env.cfg)
        np.testing.assert_array_equal(d["dropped"], ev.dropped, err_msg="dropped")
        if assign is not None:
            np.testing.assert_array_equal(assign, ev.assigned, err_msg="assignments")
            for b in range(self.B):
                for s in range(self.S):
                    v = np.array(ev.new[b][s][0], np.int64)
                    if len(v):
                        self.count[b, s] += len(v)
                        self.sum_us[b, s] += np.uint64(v.sum())
                        self.max_us[b, s] = max(int(self.max_us[b, s]), int(v.max()))
                        np.add.at(self.hist[b, s], flowstats.bin_of(v), 1)
        cnt, sm, mx, h = (t.cpu().numpy() for t in env.handle.flow_stats(hist=True))
        np.testing.assert_array_equal(cnt.view(np.uint32), self.count, err_msg="count")
        np.testing.assert_array_equal(sm.view(np.uint64), self.sum_us, err_msg="sum_us")
        np.testing.assert_array_equal(mx.view(np.uint32), self.max_us, err_msg="max_us")
        np.testing.assert_array_equal(h.view(np.uint32), self.hist, err_msg="hist")
        self.peak = max(self.peak, int((d["hc"] >> 16).max()))


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_flow_statistics_equal_the_reference(lib, case):
    S, kw = config_kwargs(case)
    back = DeviceBackend(S, kw, flow_stats=True)
    chk = StatsCheck(back.env)
    events = drive(case, GPU_B, back, chk)
    check_reaches(case, events, chk.peak, GPU_B)
    assert int(chk.count.sum()) > 20 * GPU_B
    back.env.close()
