"""Shared server pools: several balancers in front of one set of servers.

The reference is tests/pool_ref.PoolSim, written from §3.21's text on top of
tests/flowsim_ref.FlowSim (absolute times, plain lists, entries that carry their owner).  One
scenario per case: reset, 12 steps, a masked reset in the middle whose mask names ONE member of
every third pool, so whole pools restart.  The rates keep every (member, server) reservoir count
at or below 128, so completion c of a member at a server is record c (asserted on the CPU).

Not gpu: PoolSim with one member against FlowSim; one server against a hand merge of the members'
streams; what the scenario reaches; lbsim_pool.h's rule as a host program under the address and
undefined-behaviour sanitizers against numpy; the argument rules that need no device.
gpu: enabled handles against PoolSim after every reset and step through their state and outputs,
one-member pools against the C oracle, the ground truth of the physical servers, a mid-run rate
change, state round trips, graph replay, shards, normalize_obs, the VPP export and the MARL view.
"""
import os
import subprocess

import numpy as np
import pytest

import oracle
from marllb_amd import _lib as lbffi
from marllb_amd import build, dist, pools
from marllb_amd.env import make_config
from tests import parity, statelayout
from tests import test_flowsim_ref as fr
from tests.flowsim_ref import FlowSim
from tests.parity import lib  # noqa: F401  (the fixture: fails a gpu test run without a device)
from tests.pool_ref import PoolSim

HERE = os.path.dirname(os.path.abspath(__file__))
K = 128
STEPS, RESET_AT, CHANGE_AT = 12, 6, 3
POOL_KERNEL = 3  # LBSIM_DYN_KERNEL_POOL
gpu = pytest.mark.gpu
CONT = {"action_type": "continuous"}

# id: (pools C, balancers A, servers S, config kwargs, member rate spread or None, what it reaches)
# The shapes: pools spanning two waves with a partly filled last wave at every group width
# (22 x 3 and 33 x 2 on 4 lanes: 16 pools per wave; 9 x 8 and 10 x 5 on 8 lanes: 8 per wave; 5 x 2
# on 16 lanes: 4 per wave; 35 x 1 and 37 x 2 on 2 lanes: 32 per wave), A above and below S, S in
# {1, 2, 3, 4, 6, 16}, Q in {3, 6, 32}, the four policies, both action types, unequal member rates.
CASES = {
    "a3-s4-sed-levels": (22, 3, 4, {"discrete_weights": [0.5, 1.0, 8.0], "arrival_rate": 20.0,
                                    "server_rates": [17.0] * 4, "warmup_steps": 2}, None,
                         ("carried",)),
    "a2-s3-lsq-q6-overload": (33, 2, 3, {"assign_policy": "lsq", "queue_capacity": 6,
                                         "arrival_rate": 30.0, "server_rates": [16.0] * 3,
                                         "warmup_steps": 2}, (0.6, 1.4),
                              ("drops", "carried")),
    "a8-s6-sed2-continuous": (9, 8, 6, {"assign_policy": "sed2", **CONT, "arrival_rate": 300.0,
                                        "server_rates": [450.0] * 6, "warmup_steps": 2,
                                        "step_interval": 0.05}, None, ("ties", "carried")),
    "a4-s1-q3-drops": (17, 4, 1, {"queue_capacity": 3, "arrival_rate": 8.0,
                                  "server_rates": [25.0], "warmup_steps": 2}, (0.5, 1.5),
                       ("drops", "own-zero", "carried")),
    "a2-s16-lsq2-continuous": (5, 2, 16, {"assign_policy": "lsq2", **CONT, "arrival_rate": 80.0,
                                          "server_rates": [11.0] * 16, "warmup_steps": 2}, None, ()),
    "a5-s3-sed-unequal": (10, 5, 3, {"arrival_rate": 12.0, "server_rates": [15.0, 22.0, 30.0],
                                     "warmup_steps": 2}, (0.4, 1.6), ("carried",)),
    "a1-s1-sed": (35, 1, 1, {"arrival_rate": 20.0, "server_rates": [30.0], "warmup_steps": 4}, None,
                  ()),
    # two members on the narrowest group: every forced width (4, 8, 16) is above its own
    "a2-s2-lsq2-levels": (37, 2, 2, {"assign_policy": "lsq2", "arrival_rate": 15.0,
                                     "server_rates": [18.0, 16.0], "warmup_steps": 2}, None, ()),
}


def case_kwargs(case):
    C, A, S, kw, spread, _ = CASES[case]
    return C, A, S, {"seed": 8100 + list(CASES).index(case), **kw}


def member_rates(case, variant=0):
    """(C, A) f32 arrival rates of the members: the config's rate, or spread over `spread` times
    it (an unequal ECMP split)."""
    C, A, S, kw = case_kwargs(case)
    spread = CASES[case][4]
    base = np.float32(kw["arrival_rate"])
    if spread is None and not variant:
        return None
    lo, hi = spread or (0.7, 1.3)
    rng = np.random.default_rng(900 + 7 * list(CASES).index(case) + variant)
    return (base * rng.uniform(lo, hi, (C, A))).astype(np.float32)


def actions_of(case):
    C, A, S, kw = case_kwargs(case)
    rng = np.random.default_rng(50 + list(CASES).index(case))
    out = []
    for _ in range(STEPS):
        if kw.get("action_type") == "continuous":
            out.append(rng.uniform(-1.0, 11.0, (C * A, S)).astype(np.float32))
        else:
            n = len(kw.get("discrete_weights", [1.0, 1.5, 2.0]))
            out.append(rng.integers(-n, n, (C * A, S)).astype(np.int64))
    return out


def reset_mask(case):
    """One member (the last) of every third pool."""
    C, A, _, _ = case_kwargs(case)
    b = np.arange(C * A)
    return ((b // A) % 3 == 0) & (b % A == A - 1)


def make_pools(case, cfg, kw, rates):
    C, A, S, _ = case_kwargs(case)
    r = rates if rates is not None else np.full((C, A), np.float32(cfg.arrival_rate))
    return [PoolSim(kw["seed"], cfg.env_id_offset + c * A, A, S, cfg.queue_capacity,
                    kw.get("assign_policy", "sed"), r[c], [cfg.server_rate[s] for s in range(S)],
                    dt=cfg.step_interval, warmup_steps=cfg.warmup_steps) for c in range(C)]


class Event(fr.Event):
    """fr.Event per env (a member), plus the physical queues per pool."""


_RUNS = {}


def reference_run(case, change=False):
    """The scenario on the case's PoolSims -> (cfg, kw, actions, events, rates, changed rates,
    what was reached).  Computed once per (case, change)."""
    if (case, change) in _RUNS:
        return _RUNS[(case, change)]
    C, A, S, kw = case_kwargs(case)
    B = C * A
    cfg = make_config(B, S, **kw)
    rates, changed = member_rates(case), member_rates(case, variant=1)
    sims = make_pools(case, cfg, kw, rates)
    drops = np.zeros(B, np.int64)
    acts = actions_of(case)
    events = []
    reach = {"carried_behind_other": 0, "drop_own_below_q": 0, "own_zero_at_full": 0,
             "partial_mask": 0}

    def record(c, r, ev, step_lo):
        for a in range(A):
            b = c * A + a
            for s in range(S):
                ev.new[b][s][0].extend(r.fct(a, s))
                ev.new[b][s][1].extend(r.tc(a, s))
        Q = cfg.queue_capacity
        for (ta, a, s, phys, own) in sims[c].events:  # the drops of this step
            full = [x for x in range(S) if phys[x] >= Q]
            reach["drop_own_below_q"] += int(any(own[x] < Q for x in full))
            reach["own_zero_at_full"] += int(any(own[x] == 0 for x in full))
        # a flow that arrived in an earlier step and completed in this one, queued behind another
        # member's flow: its start was that flow's completion, start = tc - svc > ta; the queue
        # order shows it as a completion (ta < step_lo) right after another owner's on its server
        for s in range(S):
            seq = [(ta, tc, own) for (sv, ta, tc, own) in r.completed if sv == s]
            for prev, cur in zip(seq, seq[1:]):
                if cur[0] < step_lo and prev[2] != cur[2] and prev[1] > cur[0]:
                    reach["carried_behind_other"] += 1

    def snapshot(ev):
        ev.dropped = drops.copy()
        ev.in_flight = np.array([row for m in sims for row in m.in_flight()])
        ev.arr_idx = np.array([x.k for m in sims for x in m.members])
        ev.next_abs = np.array([x.next_arrival() for m in sims for x in m.members])
        ev.steps = np.array([m.step_no for m in sims for _ in range(A)])
        ev.queues = [[list(q) for q in m.queues] for m in sims]
        events.append(ev)

    def reset(mask):
        ev = Event(B, S)
        ev.given = mask
        pool = mask.reshape(C, A).any(1)  # a pool resets iff any member's byte is set
        ev.mask = np.repeat(pool, A)
        reach["partial_mask"] += int((mask.reshape(C, A).sum(1) == 1).any() and A > 1)
        for c in np.flatnonzero(pool):
            drops[c * A:(c + 1) * A] = 0
            for k, r in enumerate(sims[c].reset()):
                drops[c * A:(c + 1) * A] += r.dropped
                record(c, r, ev, k * sims[c].dt)
        snapshot(ev)

    reset(np.ones(B, bool))
    for k in range(STEPS):
        if k == RESET_AT:
            reset(reset_mask(case))
        if change and k == CHANGE_AT:
            for c in range(C):
                for a in range(A):
                    sims[c].set_rate(a, changed[c, a])
        w = fr.weights_of(acts[k], kw).reshape(C, A, S)
        ev = Event(B, S)
        for c in range(C):
            lo = sims[c].step_no * sims[c].dt
            r = sims[c].step(w[c])
            ev.assigned[c * A:(c + 1) * A] = r.assigned
            drops[c * A:(c + 1) * A] += r.dropped
            record(c, r, ev, lo)
        snapshot(ev)
    reach["ties"] = sum(m.ties for m in sims)
    _RUNS[(case, change)] = (cfg, kw, acts, events, rates, changed, reach)
    return _RUNS[(case, change)]


def drive(case, backend, check, change=False):
    _, _, acts, events, _, changed, _ = reference_run(case, change)
    it = iter(events)
    check(next(it), backend.reset(None))
    for k in range(STEPS):
        if k == RESET_AT:
            check(next(it), backend.reset(reset_mask(case).astype(np.uint8)))
        if change and k == CHANGE_AT:
            backend.set_rates(changed)
        check(next(it), backend.step(acts[k]))
    return events


# ------------------------------------------------------------------ not gpu: the reference

FLOWSIM_CASES = [c for c, v in fr.CASES.items()
                 if v[1].get("assign_policy", "sed") != "alias" and not v[1].get("_trace")]


@pytest.mark.parametrize("case", FLOWSIM_CASES)
def test_pool_of_one_equals_flowsim(case):
    """(a) PoolSim with A = 1 is FlowSim event for event, on every FlowSim case whose policy and
    arrival source a pool has (no ALIAS, no trace)."""
    S, kw = fr.config_kwargs(case)
    cfg = make_config(4, S, **kw)
    acts = fr.actions_of(case, 4)
    mu = [cfg.server_rate[s] for s in range(S)]
    for b in range(4):
        opt = dict(dt=cfg.step_interval, warmup_steps=cfg.warmup_steps)
        plain = FlowSim(kw["seed"], cfg.env_id_offset + b, S, cfg.queue_capacity,
                        kw.get("assign_policy", "sed"), cfg.arrival_rate, mu, **opt)
        pool = PoolSim(kw["seed"], cfg.env_id_offset + b, 1, S, cfg.queue_capacity,
                       kw.get("assign_policy", "sed"), [cfg.arrival_rate], mu, **opt)

        def same(ra, rb):
            np.testing.assert_array_equal(ra.assigned, rb.assigned[0])
            assert ra.dropped == rb.dropped[0]
            assert ra.completed == [(s, ta, tc) for (s, ta, tc, own) in rb.completed]
            assert all(own == 0 for (_, _, _, own) in rb.completed)
            assert plain.in_flight() == pool.in_flight()[0] == pool.physical()
            assert plain.k == pool.members[0].k
            assert plain.next_arrival() == pool.members[0].next_arrival()

        for ra, rb in zip(plain.reset(), pool.reset()):
            same(ra, rb)
        for k in range(fr.STEPS):
            if k == fr.RESET_AT and b % 3 == 0:
                for ra, rb in zip(plain.reset(), pool.reset()):
                    same(ra, rb)
            wt = fr.weights_of(acts[k], kw)[b]
            same(plain.step(wt), pool.step(wt[None]))


@pytest.mark.parametrize("A,Q,rate,mu", [(2, 32, 20.0, 50.0), (4, 3, 9.0, 25.0), (8, 6, 6.0, 40.0)])
def test_one_server_equals_a_hand_merge(A, Q, rate, mu):
    """(b) S = 1: the pool's completions equal an independent merge of the A members' FlowSim
    arrival streams into one FIFO (sorted by (time, member); a full queue drops)."""
    seed, gid0, steps, warm = 991 + A, 40 * A, 10, 2
    rates = [rate * (1 + 0.2 * a) for a in range(A)]
    pool = PoolSim(seed, gid0, A, 1, Q, "sed", rates, [mu], warmup_steps=warm)
    got, got_drops = [], np.zeros(A, np.int64)
    for r in pool.reset():
        got += r.completed
        got_drops += r.dropped
    for _ in range(steps):
        r = pool.step(np.ones((A, 1), np.float32))
        got += r.completed
        got_drops += r.dropped
    end = (steps + warm) * pool.dt
    # the hand merge: every member's arrivals before `end`, from FlowSims of their own
    arr = []
    scale = None
    for a in range(A):
        m = FlowSim(seed, gid0 + a, 1, Q, "sed", rates[a], [mu], warmup_steps=0)
        m.reset()
        scale = m.svc_scale[0]
        k = 0
        while m._arrival(k) < end:
            arr.append((m._ta[k], a, m._work[k]))
            k += 1
    arr.sort(key=lambda e: (e[0], e[1]))
    queue, want, drops, tail = [], [], np.zeros(A, np.int64), None
    for ta, a, work in arr:
        while queue and queue[0][0] <= ta:
            tc, t0, own = queue.pop(0)
            want.append((0, t0, tc, own))
        if len(queue) >= Q:
            drops[a] += 1
            continue
        start = max(ta, queue[-1][0]) if queue else ta
        queue.append((start + max(1, int(np.float32(work) * scale)), ta, a))
    want += [(0, t0, tc, own) for (tc, t0, own) in queue if tc <= end]
    assert got == want and len(want) > 10 * A
    np.testing.assert_array_equal(got_drops, drops)
    assert len({own for (_, _, _, own) in want}) == A


def check_reaches(case):
    """(c) The scenario is not vacuous, and its records list every completion."""
    C, A, S, _ = case_kwargs(case)
    _, _, _, events, _, _, reach = reference_run(case)
    B = C * A
    count = np.zeros((B, S), np.int64)
    peak = 0
    for ev in events:
        if ev.mask is not None:
            count[ev.mask] = 0
        count += np.array([[len(ev.new[b][s][0]) for s in range(S)] for b in range(B)])
        peak = max(peak, int(count.max()))
    assert peak <= K, "a reservoir wrapped: its records no longer list every flow of its owner"
    recorded = sum(len(ev.new[b][s][0]) for ev in events for b in range(B) for s in range(S))
    assert recorded > 10 * B
    return peak, reach


@pytest.mark.parametrize("case", list(CASES))
def test_scenario_reaches(case):
    peak, reach = check_reaches(case)
    tags = CASES[case][5]
    print(f"REACH {case}: peak reservoir count {peak}, {reach}")
    if "ties" in tags:
        assert reach["ties"] > 0
    if "carried" in tags:
        assert reach["carried_behind_other"] > 0
    if "drops" in tags:
        assert reach["drop_own_below_q"] > 0
    if "own-zero" in tags:
        assert reach["own_zero_at_full"] > 0
    if CASES[case][1] > 1:
        assert reach["partial_mask"] > 0


def test_scenarios_reach_everything_between_them():
    """Every situation the issue names is met by some GPU case at its GPU batch size."""
    total = {}
    for case in CASES:
        for k, v in check_reaches(case)[1].items():
            total[k] = total.get(k, 0) + v
    assert all(total[k] > 0 for k in ("ties", "carried_behind_other", "drop_own_below_q",
                                      "own_zero_at_full", "partial_mask")), total


# ------------------------------------------------------------------ not gpu: lbsim_pool.h

@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/pool_probe.cpp, the rule of csrc/lbsim_pool.h as a host program built with the
    address and undefined-behaviour sanitizers: probe(lines) -> its output lines."""
    exe = str(tmp_path_factory.mktemp("pool") / "pool_probe")
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "pool_probe.cpp")], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


def test_rule_small_functions(probe):
    """(d) The enable check, the group width, the next member and the service time against
    numpy."""
    rng = np.random.default_rng(3)
    checks = [(B, off, A) for B in (1, 6, 8, 24, 66) for off in (0, 3, 8, 24) for A in range(0, 11)]
    out = probe([f"check {B} {off} {A}" for B, off, A in checks])
    for (B, off, A), line in zip(checks, out):
        want = 1 if not 1 <= A <= 8 else 2 if B % A else 3 if off % A else 0
        assert int(line) == want, (B, off, A)
    lanes = [(S, A, f) for S in range(1, 17) for A in range(1, 9) for f in (0, 2, 4, 8, 16, 32)]
    out = probe([f"lanes {S} {A} {f}" for S, A, f in lanes])
    for (S, A, f), line in zip(lanes, out):
        need = max(S, A)
        want = f if f in (4, 8, 16) and f >= need else max(2, 1 << (need - 1).bit_length())
        assert int(line) == want and int(line) >= need, (S, A, f)
    rows = [rng.integers(-5, 5, A) * int(rng.integers(1, 1000)) for A in range(1, 9) for _ in range(40)]
    rows += [np.array([2 ** 31 - 1] * 3), np.array([-2 ** 31, 0, -2 ** 31])]
    out = probe([f"next {len(t)} " + " ".join(map(str, t.tolist())) for t in rows])
    for t, line in zip(rows, out):
        assert int(line) == int(np.argmin(t)), t  # argmin: the first of equal minima
    work = np.concatenate([rng.exponential(1.0, 200), [0.0, 1e-9, 16.6]]).astype(np.float32)
    scale = (1e6 / rng.uniform(1.0, 1e4, len(work))).astype(np.float32)
    out = probe([f"svc {int(w.view(np.uint32))} {int(s.view(np.uint32))}"
                 for w, s in zip(work, scale)])
    for w, s, line in zip(work, scale, out):
        assert int(line) == max(1, int(np.float32(w * s))), (w, s)


@pytest.mark.parametrize("Q", [1, 3, 6, 32, 64])
def test_rule_physical_fifo(probe, Q):
    """(d) One physical FIFO on a ring of exactly Q entries, from every head position, against a
    list: completions with their owners in order, drops at a full queue, the ring word."""
    rng = np.random.default_rng(Q)
    lines, wants = [], []
    for head in sorted({0, Q // 2, Q - 1}):
        for load in (0.5, 1.0, 2.0):
            n = 6 * Q + 10
            ta = np.cumsum(rng.integers(0, 200, n)).tolist()
            svc = rng.integers(1, int(200 * load) + 2, n).tolist()
            own = rng.integers(0, 8, n).tolist()
            lines.append(f"fifo {Q} {head} {n} " +
                         " ".join(f"{a} {b} {c}" for a, b, c in zip(ta, svc, own)))
            q, out, h = [], [], head
            for a, b, c in zip(ta, svc, own):
                while q and q[0][0] <= a:
                    tc, t0, o = q.pop(0)
                    h = (h + 1) % Q
                    out += ["c", tc, t0, o]
                if len(q) >= Q:
                    out += ["d", a, c]
                    continue
                q.append(((max(a, q[-1][0]) if q else a) + b, a, c))
            word = h | len(q) << 16
            for tc, t0, o in q:
                out += ["c", tc, t0, o]
            wants.append(" ".join(map(str, out + ["w", word])))
    got = probe(lines)
    assert [g.strip() for g in got] == wants
    assert any(" d " in w for w in wants) or Q == 64


# ------------------------------------------------------------------ not gpu: the argument rules

def refused_configs():
    """What the enable rule names -> config kwargs that have it (S: the server count)."""
    from marllb_amd import trace
    return {
        "num_servers > 16": dict(S=20),
        "assign_policy ALIAS": dict(assign_policy="alias"),
        "arrival_source TRACE": dict(trace=trace.synthetic(37, 300.0, seed=7)),
        "lost_fin_prob > 0": dict(lost_fin_prob=0.1),
        "fail_prob > 0": dict(fail_prob=0.01),
        "reservoir_mode VPP": dict(reservoir_mode="vpp"),
        "n_flow_on_mode VPP": dict(n_flow_on_mode="vpp"),
        "duration_mode SERVICE": dict(duration_mode="service"),
        "next_step_reset": dict(next_step_reset=True),
    }


REFUSED_OPTIONS = {"flow statistics": dict(flow_stats=True),
                   "server availability": dict(server_availability=True),
                   "cross traffic": dict(cross_traffic=True),
                   "server workers": dict(server_workers=True),
                   "action delay": dict(action_delay=True)}


def test_enable_rule_without_a_device():
    """(e) check_pool_config: what lbsim_server_pool_enable accepts, before any handle exists."""
    ok = make_config(24, 4, seed=1)
    for A in (1, 2, 3, 4, 6, 8):
        pools.check_pool_config(ok, A)
    for A in (0, -1, 9, 5, 7):
        with pytest.raises(ValueError):
            pools.check_pool_config(ok, A)
    with pytest.raises(ValueError, match="env_id_offset"):
        pools.check_pool_config(make_config(24, 4, seed=1, env_id_offset=10), 4)
    pools.check_pool_config(make_config(24, 4, seed=1, env_id_offset=48), 4)
    for what, kw in refused_configs().items():
        kw = dict(kw)
        cfg = make_config(24, kw.pop("S", 4), seed=1, **kw)
        with pytest.raises(lbffi.LbsimError, match=what) as e:
            pools.check_pool_config(cfg, 2)
        assert e.value.code == lbffi.ENOTSUP
    for what, kw in REFUSED_OPTIONS.items():
        with pytest.raises(lbffi.LbsimError, match=what) as e:
            pools.check_pool_config(ok, 2, **kw)
        assert e.value.code == lbffi.ENOTSUP


def test_shape_errors_precede_the_device():
    """(e) VecLoadBalanceEnv / VecServerPoolEnv refuse a bad pool size before creating a handle."""
    from marllb_amd import VecLoadBalanceEnv, VecServerPoolEnv
    with pytest.raises(ValueError, match="multiple"):
        VecLoadBalanceEnv(10, 4, balancers_per_pool=4, seed=1)
    with pytest.raises(ValueError, match=r"\[1, 8\]"):
        VecLoadBalanceEnv(18, 4, balancers_per_pool=9, seed=1)
    with pytest.raises(lbffi.LbsimError, match="ALIAS"):
        VecLoadBalanceEnv(8, 4, balancers_per_pool=2, seed=1, assign_policy="alias")
    with pytest.raises(lbffi.LbsimError, match="cross traffic"):
        VecLoadBalanceEnv(8, 4, balancers_per_pool=2, seed=1, cross_traffic=True)
    for bad in ((0, 2, 4), (3, 0, 4), (3, 9, 4)):
        with pytest.raises(ValueError):
            VecServerPoolEnv(*bad, seed=1)
    with pytest.raises(ValueError, match="num_balancers"):
        VecServerPoolEnv(3, 2, 4, balancers_per_pool=2, seed=1)


def test_sampler_shards_and_abi():
    import torch
    from marllb_amd import sample_pool_arrival_rates
    r = sample_pool_arrival_rates(200, 4, total=(100.0, 300.0), skew=(1.0, 3.0), seed=5)
    assert r.shape == (800,) and r.dtype == torch.float32
    tot = r.double().view(200, 4).sum(1)
    assert 100.0 - 1e-3 <= float(tot.min()) and float(tot.max()) <= 300.0 + 1e-3
    srt = r.double().view(200, 4).sort(dim=1, descending=True).values
    ratio = srt[:, :-1] / srt[:, 1:]
    assert torch.allclose(ratio, ratio[:, :1].expand_as(ratio), rtol=1e-5)
    assert 1.0 - 1e-6 <= float(ratio.min()) and float(ratio.max()) <= 3.0 * (1 + 1e-5)
    assert torch.equal(r, sample_pool_arrival_rates(200, 4, total=(100.0, 300.0), skew=(1.0, 3.0),
                                                    seed=5))
    eq = sample_pool_arrival_rates(3, 4, total=(400.0, 400.0)).view(3, 4)
    assert torch.allclose(eq, torch.full((3, 4), 100.0))
    for bad in (dict(total=(0.0, 5.0)), dict(total=(9.0, 5.0)), dict(skew=(0.5, 2.0)),
                dict(skew=(3.0, 2.0)), dict(total=(0.2, 0.3), skew=(5.0, 5.0))):
        with pytest.raises(ValueError):
            sample_pool_arrival_rates(4, 4, **bad)
    # shards keep pools whole
    sh = dist.pool_shard(1, 3, pools_per_rank=5, balancers_per_pool=4)
    assert sh.envs_per_rank == 20 and sh.env_id_offset == 20 and sh.env_id_offset % 4 == 0
    assert list(sh.pools(4)) == [5, 6, 7, 8, 9] and sh.check_pools(4) is sh
    with pytest.raises(ValueError, match="straddle"):
        dist.Shard(1, 2, 10).check_pools(4)
    header = open(os.path.join(os.path.dirname(HERE), "include", "lbsim.h")).read()
    for name, nargs in (("lbsim_server_pool_enable", 2), ("lbsim_server_pool_size", 1)):
        assert f"int {name}(" in header
        assert len(lbffi._SIGNATURES[name][1]) == nargs
    assert "LBSIM_DYN_KERNEL_POOL = 3" in header and "#define LBSIM_ABI_VERSION 10 " in header


# ------------------------------------------------------------------ the device

def pool_state(env):
    """The state of an enabled handle: every section where a default handle has it, then pool_hc
    (C, S) and pool_owner (C, S, Q)."""
    c = env.cfg
    B, S, Q, A = c.num_envs, c.num_servers, c.queue_capacity, env.balancers_per_pool
    C = B // A
    buf = env.handle.state_bytes()
    tail = C * S * 4 + C * S * Q
    d = statelayout.parse_cfg(buf[:len(buf) - tail], c)
    d["pool_hc"] = np.frombuffer(buf[len(buf) - tail:len(buf) - C * S * Q], np.uint32).reshape(C, S)
    d["pool_owner"] = np.frombuffer(buf[len(buf) - C * S * Q:], np.uint8).reshape(C, S, Q)
    return d


class DeviceBackend:
    """reset / step -> (obs, reward or None, assign counts or None), numpy."""

    def __init__(self, case, rates=None, **extra):
        import torch
        from marllb_amd.env import VecLoadBalanceEnv
        C, A, S, kw = case_kwargs(case)
        self.torch = torch
        self.env = VecLoadBalanceEnv(C * A, S, device="cuda:0", autoreset=False,
                                     balancers_per_pool=A, **extra, **kw)
        if rates is not None:
            self.set_rates(rates)

    def set_rates(self, rates):
        self.env.set_rates(arrival_rate=np.ascontiguousarray(rates, np.float32).reshape(-1))

    def reset(self, mask):
        obs = self.env.reset(mask=None if mask is None else self.torch.from_numpy(mask))
        return obs.cpu().numpy(), None, None

    def step(self, a):
        obs, rew, _, info = self.env.step(self.torch.from_numpy(a), assign_counts=True)
        return obs.cpu().numpy(), rew.cpu().numpy(), info["assign_counts"].cpu().numpy()


def check_features(env, d, obs, rew, who):
    """Columns 1-10 are oracle.features of the state's records and the reward is oracle.rewards of
    the observation, bit for bit (tests/test_cross_traffic.py's check)."""
    B, S = env.cfg.num_envs, env.cfg.num_servers
    val = d["res_fct"].view(np.int32).astype(np.float32) * np.float32(1e-6)
    f = oracle.features(val, d["res_ts"], d["res_count"]).reshape(B, S, 5)
    np.testing.assert_array_equal(obs[:, :, 1:6], f, err_msg=f"{who}: fct features")
    np.testing.assert_array_equal(obs[:, :, 6:11], f, err_msg=f"{who}: duration features")
    if rew is not None:
        want = oracle.rewards(obs, env.cfg.reward_metric, env.cfg.reward_field)
        np.testing.assert_array_equal(rew, want, err_msg=f"{who}: reward")


class PoolCheck:
    """An Event of the reference against an enabled handle's state and outputs."""

    def __init__(self, env):
        self.env, self.cfg = env, env.cfg
        self.B, self.S, self.A = env.cfg.num_envs, env.cfg.num_servers, env.balancers_per_pool
        self.dt = int(round(env.cfg.step_interval * 1e6))
        self.count = np.zeros((self.B, self.S), np.int64)

    def __call__(self, ev, out):
        B, S, A, Q = self.B, self.S, self.A, self.cfg.queue_capacity
        obs, rew, assign = out
        d = pool_state(self.env)
        if assign is not None:
            np.testing.assert_array_equal(assign, ev.assigned, err_msg="assign_counts")
        np.testing.assert_array_equal(d["dropped"], ev.dropped, err_msg="dropped")
        np.testing.assert_array_equal(d["arr_idx"], ev.arr_idx, err_msg="arrival index")
        np.testing.assert_array_equal(d["clock"], ev.steps, err_msg="clock")
        np.testing.assert_array_equal(d["next_arr"].astype(np.int64) + ev.steps * self.dt,
                                      ev.next_abs, err_msg="next arrival")
        own = (d["hc"].reshape(B, S) >> 16).astype(np.int64)
        np.testing.assert_array_equal(own, ev.in_flight, err_msg="own counts (hc >> 16)")
        np.testing.assert_array_equal(obs[:, :, 0], ev.in_flight.astype(np.float32),
                                      err_msg="observation column 0")
        # the physical queue: count, {tc, ta} and owners by position from the head
        ring = d["ring"].reshape(B, S, Q, 2).astype(np.int64)
        for c, queues in enumerate(ev.queues):
            base = int(ev.steps[c * A]) * self.dt
            for s, q in enumerate(queues):
                w = int(d["pool_hc"][c, s])
                h, n = w & 0x7FFF, w >> 16
                assert n == len(q), ("physical count", c, s)
                pos = [(h + i) % Q for i in range(n)]
                got = [(int(ring[c * A, s, p, 0]) + base, int(ring[c * A, s, p, 1]) + base,
                        int(d["pool_owner"][c, s, p])) for p in pos]
                assert got == q, ("physical queue", c, s)
        assert (own.reshape(-1, A, S).sum(1) == (d["pool_hc"] >> 16)).all()
        c1 = d["res_count"].reshape(B, S).astype(np.int64)
        fct, ts = d["res_fct"].reshape(B, S, K), d["res_ts"].reshape(B, S, K)
        if ev.mask is not None:
            self.count[ev.mask] = 0
        new = np.array([[len(ev.new[b][s][0]) for s in range(S)] for b in range(B)])
        np.testing.assert_array_equal(c1, self.count + new, err_msg="res_count")
        assert c1.max() <= K
        for b in range(B):
            for s in range(S):
                want_fct, want_tc = ev.new[b][s]
                c0 = int(self.count[b, s])
                if want_fct:
                    assert fct[b, s, c0:c1[b, s]].tolist() == want_fct, ("fct records", b, s)
                    assert ts[b, s, c0:c1[b, s]].tolist() == [t // 1000 for t in want_tc], (
                        "record timestamps", b, s)
        self.count = c1
        check_features(self.env, d, obs, rew, "pool handle")


def check_pool_kernel(lib, env, reset=False):
    names = lib.launch_names(env.handle, 1 if reset else 0)
    assert lib.load().lbsim_dynamics_kernel(env.handle.h) == POOL_KERNEL, names
    name = names.get(2 if reset else 0, "")
    assert name.startswith("dynamics_pool_kernel<"), names
    assert lib.load().lbsim_server_pool_size(env.handle.h) == env.balancers_per_pool
    lanes = os.environ.get("LBSIM_DYN_GROUP_LANES")
    need = max(env.cfg.num_servers, env.balancers_per_pool)
    if lanes and int(lanes) >= need:
        assert name.startswith(f"dynamics_pool_kernel<{lanes},"), names


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_enabled_handles_equal_the_reference(lib, case):
    rates = reference_run(case)[4]
    back = DeviceBackend(case, rates=rates)
    drive(case, back, PoolCheck(back.env))
    check_pool_kernel(lib, back.env)
    check_pool_kernel(lib, back.env, reset=True)
    check_reaches(case)
    back.env.close()


def pools_width(S, A):
    """A pool's own group width: pow2 >= max(S, A), at least 2."""
    return max(2, 1 << (max(S, A) - 1).bit_length())


FORCED = {4: [c for c, v in CASES.items() if max(v[1], v[2]) <= 4],
          8: ["a2-s2-lsq2-levels", "a4-s1-q3-drops"],
          16: ["a2-s2-lsq2-levels", "a3-s4-sed-levels", "a8-s6-sed2-continuous"]}


@gpu
@pytest.mark.parametrize("lanes", list(FORCED))
def test_forced_group_widths(lanes):
    """LBSIM_DYN_GROUP_LANES = 4, 8, 16: groups wider than max(S, A) asks for, with one member and
    with several (the lanes past S and A hold neither a server nor a member); the child checks
    the launched kernel's width."""
    ks = [f"test_enabled_handles_equal_the_reference[{c}]" for c in FORCED[lanes]]
    own = {c: pools_width(CASES[c][2], CASES[c][1]) for c in FORCED[lanes]}
    assert any(CASES[c][1] > 1 and own[c] < lanes for c in FORCED[lanes]), own
    parity.run_cases_in_child("test_server_pools.py", ks, {"LBSIM_DYN_GROUP_LANES": str(lanes)})


@gpu
@pytest.mark.parametrize("case", ["a3-s4-sed-levels", "a4-s1-q3-drops", "a8-s6-sed2-continuous"])
def test_mid_run_rate_change(lib, case):
    """set_rates(arrival_rate) before step 3: the arrival already drawn keeps its time, every later
    gap of every member follows its new rate."""
    rates = reference_run(case, change=True)[4]
    back = DeviceBackend(case, rates=rates)
    drive(case, back, PoolCheck(back.env), change=True)
    back.env.close()


def _parity_configs():
    """tests/test_gpu_parity.py's CONFIGS inside the supported set."""
    from tests.test_gpu_parity import CONFIGS
    out = []
    for i, c in enumerate(CONFIGS):
        kw = c["kw"]
        if c["S"] > 16 or kw.get("assign_policy") == "alias" or "trace" in kw or "_trace" in kw:
            continue
        if any(kw.get(k) for k in ("lost_fin_prob", "fail_prob", "next_step_reset")):
            continue
        if kw.get("reservoir_mode", "algr") != "algr" or kw.get("n_flow_on_mode", "queue") != "queue":
            continue
        if kw.get("duration_mode", "age") != "age":
            continue
        out.append(i)
    return out


@gpu
@pytest.mark.parametrize("idx", _parity_configs())
def test_pools_of_one_equal_the_oracle(lib, oracle_mod, idx):
    """A = 1 on an enabled handle: every output and every state section equal the C oracle's, the
    pool sections repeat the env's own queue words, and the pool kernel ran."""
    from marllb_amd.env import VecLoadBalanceEnv
    from tests.test_gpu_parity import CONFIGS, resolve_kw
    c = CONFIGS[idx]
    B, S, kw = c["B"], c["S"], resolve_kw(c["kw"])
    kw.setdefault("seed", 1000 + idx)
    try:
        pools.check_pool_config(make_config(B, S, **kw), 1)
    except lbffi.LbsimError:
        pytest.fail(f"CONFIGS[{idx}] was listed as supported")
    env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=False, balancers_per_pool=1, **kw)
    ora = oracle_mod.OracleEnv(make_config(B, S, **kw), threads=4)

    class Trimmed:  # the handle's snapshot without the two pool sections
        def state_bytes(self):
            buf = env.handle.state_bytes()
            return buf[:len(buf) - B * S * 4 - B * S * env.cfg.queue_capacity]

    real = env.handle
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ora.reset())
    rng = np.random.default_rng(idx)
    import torch
    for k in range(8):
        parity.step_both(env, ora, parity.actions(rng, B, S, dict(c["kw"]), levels=True), k)
    parity.compare_state(Trimmed(), ora, env.cfg)
    d = pool_state(env)
    np.testing.assert_array_equal(d["pool_hc"].reshape(-1) & 0xFFFF7FFF, d["hc"] & 0xFFFF7FFF)
    assert not d["pool_owner"].any()
    mask = (np.arange(B) % 3 == 0).astype(np.uint8)
    og = env.reset(mask=torch.from_numpy(mask)).cpu().numpy()
    np.testing.assert_array_equal(og, ora.reset(mask=mask, obs=og.copy()))
    for k in range(4):
        parity.step_both(env, ora, parity.actions(rng, B, S, dict(c["kw"]), levels=True), 8 + k)
    parity.compare_state(Trimmed(), ora, env.cfg)
    assert env.handle is real
    check_pool_kernel(lib, env)
    ora.close()
    env.close()


def run_steps(env, acts, upto=None):
    import torch
    outs = []
    for a in acts[:upto]:
        o, r, dn, info = env.step(torch.from_numpy(a), assign_counts=True)
        outs.append((o.cpu().numpy(), r.cpu().numpy(), dn.cpu().numpy(),
                     info["assign_counts"].cpu().numpy()))
    return outs


def same_outputs(xs, ys):
    assert len(xs) == len(ys)
    for k, (x, y) in enumerate(zip(xs, ys)):
        for u, v, name in zip(x, y, ("obs", "reward", "done", "assign")):
            np.testing.assert_array_equal(u, v, err_msg=f"{name} step {k}")


@gpu
@pytest.mark.parametrize("case", ["a3-s4-sed-levels", "a2-s3-lsq-q6-overload", "a4-s1-q3-drops"])
def test_ground_truth_describes_the_physical_servers(lib, case):
    """Every member's row: n_total the physical queue, n_hidden = physical - own, wait and backlog
    of the physical FIFO (its last completion), busy / cpu of one pipe, up 1, capacity mu."""
    C, A, S, kw = case_kwargs(case)
    cfg, _, acts, events, rates, _, _ = reference_run(case)
    back = DeviceBackend(case, rates=rates)
    it = iter(events)
    dt = int(round(cfg.step_interval * 1e6))

    def check(ev):
        gt = back.env.ground_truth().cpu().numpy().reshape(C, A, S, 8)
        for c, queues in enumerate(ev.queues):
            now = int(ev.steps[c * A]) * dt
            for s, q in enumerate(queues):
                n = len(q)
                last = np.float32(max(q[-1][0] - now, 0)) * np.float32(1e-6) if q else np.float32(0)
                for a in range(A):
                    own = sum(1 for e in q if e[2] == a)
                    want = [n, n - own, min(n, 1), float(min(n, 1)), last, last, 1.0,
                            np.float32(cfg.server_rate[s])]
                    np.testing.assert_array_equal(gt[c, a, s], np.array(want, np.float32),
                                                  err_msg=f"truth row {(c, a, s)}")

    back.reset(None)
    check(next(it))
    hidden = 0
    for k in range(RESET_AT):
        back.step(acts[k])
        ev = next(it)
        check(ev)
        hidden += sum(len(q) for qs in ev.queues for q in qs)
    assert hidden > 0
    back.env.close()


@gpu
@pytest.mark.parametrize("case", ["a3-s4-sed-levels", "a8-s6-sed2-continuous"])
def test_state_round_trip_continues_identically(lib, case):
    """get_state -> set_state into a fresh handle: the pool sections travel, the run continues bit
    for bit; a snapshot of another format is refused by its size."""
    import torch
    _, _, acts, _, rates, _, _ = reference_run(case)
    a, b = DeviceBackend(case, rates=rates), DeviceBackend(case, rates=rates)
    a.reset(None)
    run_steps(a.env, acts, 5)
    snap = a.env.handle.state_bytes()
    b.env.reset()
    b.env.handle.load_state(snap)
    assert b.env.handle.state_bytes() == snap
    same_outputs(run_steps(a.env, acts[5:]), run_steps(b.env, acts[5:]))
    assert a.env.handle.state_bytes() == b.env.handle.state_bytes()
    C, A, S, kw = case_kwargs(case)
    from marllb_amd.env import VecLoadBalanceEnv
    plain = VecLoadBalanceEnv(C * A, S, device="cuda:0", autoreset=False, **kw)
    assert plain.handle.state_size() < len(snap)
    with pytest.raises(lbffi.LbsimError):
        plain.handle.load_state(snap)
    with pytest.raises(lbffi.LbsimError) as e:  # a per-env fork would tear a pool apart
        a.env.handle.state_save(torch.zeros(len(snap) + 16, dtype=torch.uint8, device="cuda:0"))
    assert e.value.code == lbffi.ENOTSUP
    for env in (a.env, b.env, plain):
        env.close()


@gpu
def test_opt_ins_are_refused_on_an_enabled_handle(lib):
    """ENOTSUP from the library itself: the other opt-ins after the pools, the pools after one of
    them, per-env server rates; EINVAL for a second size and for enabling after the first reset."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    env = VecLoadBalanceEnv(12, 4, device="cuda:0", autoreset=False, balancers_per_pool=3, seed=5)
    h = env.handle
    for fn in (h.enable_flow_stats, h.enable_server_avail, h.enable_cross_traffic,
               h.enable_server_workers, h.enable_action_delay):
        with pytest.raises(lbffi.LbsimError) as e:
            fn()
        assert e.value.code == lbffi.ENOTSUP and "server pools" in str(e.value)
    with pytest.raises(lbffi.LbsimError) as e:
        env.set_rates(server_rates=torch.full((12, 4), 100.0))
    assert e.value.code == lbffi.ENOTSUP
    env.set_rates(arrival_rate=torch.full((12,), 100.0))
    h.enable_server_pool(3)  # the same value: a no-op
    with pytest.raises(ValueError, match="already on"):
        h.enable_server_pool(2)
    env.close()
    plain = VecLoadBalanceEnv(12, 4, device="cuda:0", autoreset=False, seed=5, flow_stats=True)
    with pytest.raises(lbffi.LbsimError, match="flow statistics") as e:
        plain.handle.enable_server_pool(2)
    assert e.value.code == lbffi.ENOTSUP and plain.handle.server_pool_size() == 0
    plain.close()
    late = VecLoadBalanceEnv(12, 4, device="cuda:0", autoreset=False, seed=5)
    for bad in (0, 9, 5):
        with pytest.raises(ValueError):
            late.handle.enable_server_pool(bad)
    late.reset()
    with pytest.raises(ValueError, match="first"):
        late.handle.enable_server_pool(2)
    late.close()
    off = VecLoadBalanceEnv(12, 4, device="cuda:0", autoreset=False, seed=5, env_id_offset=8)
    with pytest.raises(ValueError, match="env_id_offset"):
        off.handle.enable_server_pool(3)
    off.handle.enable_server_pool(4)
    off.close()


@gpu
@pytest.mark.parametrize("case", ["a3-s4-sed-levels", "a5-s3-sed-unequal"])
def test_captured_step_replays_equal_eager_steps(lib, case):
    """One step captured into a graph and replayed N times equals N eager steps."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    C, A, S, kw = case_kwargs(case)
    _, _, acts, _, rates, _, _ = reference_run(case)
    eager = DeviceBackend(case, rates=rates)
    eager.reset(None)
    g = VecLoadBalanceEnv(C * A, S, device="cuda:0", autoreset=False, balancers_per_pool=A,
                          graph_mode=True, **kw)
    if rates is not None:
        g.set_rates(arrival_rate=rates.reshape(-1))
    g.reset()
    a_buf = torch.from_numpy(acts[0]).to("cuda:0")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = g.step(a_buf)  # warm the buffers
        torch.cuda.synchronize()
    eager.step(acts[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = g.step(a_buf)
    N = 5
    for k in range(1, 1 + N):  # (capture runs nothing)
        a_buf.copy_(torch.from_numpy(acts[k]))
        graph.replay()
        torch.cuda.synchronize()
        o, r, _ = eager.step(acts[k])
        np.testing.assert_array_equal(out[0].cpu().numpy(), o, err_msg=f"obs replay {k}")
        np.testing.assert_array_equal(out[1].cpu().numpy(), r, err_msg=f"reward replay {k}")
    assert g.handle.state_bytes() == eager.env.handle.state_bytes()
    g.close()
    eager.env.close()


@gpu
def test_two_shards_equal_one_handle(lib):
    """Pools 0-12 and 13-21 of the 22 x 3 case on two handles (env_id_offset a multiple of A) equal
    the one handle, outputs and state."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    case = "a3-s4-sed-levels"
    C, A, S, kw = case_kwargs(case)
    _, _, acts, _, _, _, _ = reference_run(case)
    whole = DeviceBackend(case)
    whole.reset(None)
    ref = run_steps(whole.env, acts, 6)
    cut = 13 * A
    parts = [VecLoadBalanceEnv(n, S, device="cuda:0", autoreset=False, balancers_per_pool=A,
                               env_id_offset=off, **kw) for off, n in ((0, cut), (cut, C * A - cut))]
    for p in parts:
        p.reset()
    got = [run_steps(p, [a[lo:hi] for a in acts], 6)
           for p, (lo, hi) in zip(parts, ((0, cut), (cut, C * A)))]
    for k in range(6):
        for i, name in enumerate(("obs", "reward", "done", "assign")):
            np.testing.assert_array_equal(np.concatenate([got[0][k][i], got[1][k][i]]), ref[k][i],
                                          err_msg=f"{name} step {k}")
    d = pool_state(whole.env)
    ds = [pool_state(p) for p in parts]
    for name in ("hc", "res_count", "next_arr", "arr_idx", "dropped", "pool_hc", "res"):
        np.testing.assert_array_equal(np.concatenate([x[name].reshape(-1) for x in ds]),
                                      d[name].reshape(-1), err_msg=name)
    for e in (whole.env, *parts):
        e.close()


@gpu
def test_normalize_obs_and_vpp_export(lib):
    """normalize_obs on a pool handle: the raw rows are the un-normalised handle's and the
    normalised ones are finite and differ from them (their values are the untouched observe
    kernels'; test_pools_of_one_equal_the_oracle pins them on the normalize_obs configs).
    lbsim_vpp_export's n_flow_on is observation column 0."""
    import torch
    case = "a3-s4-sed-levels"
    C, A, S, kw = case_kwargs(case)
    B = C * A
    _, _, acts, _, _, _, _ = reference_run(case)
    plain, norm = DeviceBackend(case), DeviceBackend(case, normalize_obs=True)
    o0 = plain.env.reset().cpu().numpy()
    norm.env.reset()
    for k in range(4):
        o, _, _, _ = plain.env.step(torch.from_numpy(acts[k]))
        on, _, _, info = norm.env.step(torch.from_numpy(acts[k]), raw_obs=True)
        np.testing.assert_array_equal(info["raw_obs"].cpu().numpy(), o.cpu().numpy())
        assert np.isfinite(on.cpu().numpy()).all()
    assert not np.array_equal(on.cpu().numpy(), o.cpu().numpy()) and o0.shape == (B, S, 11)
    tv = torch.empty((B, S, 2, 128, 2), dtype=torch.float32, device="cuda:0")
    nfo = torch.empty((B, S), dtype=torch.int32, device="cuda:0")
    ts = torch.empty(B, dtype=torch.float32, device="cuda:0")
    h = plain.env.handle
    h.check(h.lib.lbsim_vpp_export(h.h, 0, B, tv.data_ptr(), nfo.data_ptr(), ts.data_ptr(),
                                   plain.env._stream()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(nfo.cpu().numpy().astype(np.float32), o.cpu().numpy()[:, :, 0])
    assert nfo.sum() > 0
    plain.env.close()
    norm.env.close()


@gpu
def test_marl_view_shapes_and_values(lib):
    """VecServerPoolEnv: (C, A, S, 11) observations, (C, A) rewards, (C,) done, the team reward,
    the physical true state and the others' load, all equal to the flat env's."""
    import torch
    from marllb_amd import VecServerPoolEnv
    case = "a3-s4-sed-levels"
    C, A, S, kw = case_kwargs(case)
    _, _, acts, events, _, _, _ = reference_run(case)
    flat = DeviceBackend(case)
    view = VecServerPoolEnv(C, A, S, device="cuda:0", autoreset=False, max_steps=3, **kw)
    o = view.reset()
    assert tuple(o.shape) == (C, A, S, 11)
    np.testing.assert_array_equal(o.cpu().numpy().reshape(C * A, S, 11), flat.reset(None)[0])
    with pytest.raises(ValueError, match="shape"):
        view.step(torch.zeros((C * A, S), dtype=torch.int64))
    for k in range(3):
        obs, rew, done, info = view.step(torch.from_numpy(acts[k]).view(C, A, S),
                                         assign_counts=True)
        fo, fr_, fa = flat.step(acts[k])
        assert tuple(obs.shape) == (C, A, S, 11) and tuple(rew.shape) == (C, A)
        assert tuple(done.shape) == (C,) and tuple(info["assign_counts"].shape) == (C, A, S)
        np.testing.assert_array_equal(obs.cpu().numpy().reshape(C * A, S, 11), fo)
        np.testing.assert_array_equal(rew.cpu().numpy().reshape(-1), fr_)
        assert torch.equal(info["team_reward"], rew.mean(1))
        np.testing.assert_allclose(info["team_reward"].cpu().numpy(),
                                   rew.cpu().numpy().astype(np.float64).mean(1), rtol=1e-6)
        assert bool(done.all()) == (k == 2) and bool(done.any()) == (k == 2)
    ts, ol = view.true_state().cpu().numpy(), view.others_load().cpu().numpy()
    assert ts.shape == (C, S, 8) and ol.shape == (C, A, S)
    ev = events[3]
    phys = np.array([[len(q) for q in qs] for qs in ev.queues], np.float32)
    np.testing.assert_array_equal(ts[:, :, 0], phys)
    assert not ts[:, :, 1].any() and (ts[:, :, 6] == 1).all()
    np.testing.assert_array_equal(ol, phys[:, None, :] - ev.in_flight.reshape(C, A, S))
    assert ol.sum() > 0
    o2 = view.reset(pool_mask=np.arange(C) % 2 == 0)
    assert tuple(o2.shape) == (C, A, S, 11)
    steps = pool_state(view.env)["ep_step"].reshape(C, A)
    assert (steps[0::2] == 0).all() and (steps[1::2] == 3).all()
    view.close()
    flat.env.close()


@gpu
def test_library_refuses_what_check_pool_config_refuses(lib):
    """lbsim_server_pool_enable and marllb_amd.pools.check_pool_config state one rule twice: every
    config and every option the Python rule refuses, the library refuses with the same words and
    code, on a handle made without pools."""
    from marllb_amd.env import VecLoadBalanceEnv
    cases = [(what, dict(kw), {}) for what, kw in refused_configs().items()]
    cases += [(what, {}, dict(opt)) for what, opt in REFUSED_OPTIONS.items()]
    for what, kw, opt in cases:
        S = kw.pop("S", 4)
        with pytest.raises(lbffi.LbsimError, match=what):
            pools.check_pool_config(make_config(24, S, seed=1, **kw), 2, **opt)
        env = VecLoadBalanceEnv(24, S, device="cuda:0", autoreset=False, seed=1, **kw, **opt)
        with pytest.raises(lbffi.LbsimError, match=what) as e:
            env.handle.enable_server_pool(2)
        assert e.value.code == lbffi.ENOTSUP and env.handle.server_pool_size() == 0, what
        env.close()
    # per-env rates in force: refused, and clear_rates() is the way out
    import torch
    env = VecLoadBalanceEnv(24, 4, device="cuda:0", autoreset=False, seed=1)
    env.set_rates(arrival_rate=torch.full((24,), 100.0))
    with pytest.raises(lbffi.LbsimError, match="per-env rates") as e:
        env.handle.enable_server_pool(2)
    assert e.value.code == lbffi.ENOTSUP
    env.clear_rates()
    env.handle.enable_server_pool(2)
    env.set_rates(arrival_rate=torch.full((24,), 100.0))
    assert env.handle.server_pool_size() == 2
    env.close()


def episode_stats(env):
    """lbsim_episode_stats -> (length (B,) int32, return (B,) float64), numpy."""
    import torch
    B = env.cfg.num_envs
    ln = torch.full((B,), -7, dtype=torch.int32, device="cuda:0")
    rt = torch.full((B,), -7.0, dtype=torch.float64, device="cuda:0")
    h = env.handle
    h.check(h.lib.lbsim_episode_stats(h.h, ln.data_ptr(), rt.data_ptr(), env._stream()))
    torch.cuda.synchronize()
    return ln.cpu().numpy(), rt.cpu().numpy()


@gpu
@pytest.mark.parametrize("case", ["a3-s4-sed-levels", "a5-s3-sed-unequal"])
def test_episode_stats_follow_each_member(lib, case):
    """lbsim_episode_stats and lbsim_step_ex's episode outputs on an enabled handle with A > 1:
    the length is the step count and the return the float64 running sum of the member's own
    rewards -- of the float64 reward the observe kernel computes before it rounds the step's
    output to float32 (oracle.rewards(..., f64=True) of the member's observation, whose float32
    rounding is the step's reward), exactly; after a reset whose mask names ONE member of every third pool both are 0 for EVERY
    member of those pools (also the members whose byte was not set) and unchanged for the other
    pools; then they count on from there."""
    import torch
    C, A, S, kw = case_kwargs(case)
    B = C * A
    _, _, acts, _, rates, _, _ = reference_run(case)
    back = DeviceBackend(case, rates=rates)
    env = back.env
    env.reset()
    ln, rt = episode_stats(env)
    assert not ln.any() and not rt.any()
    total = np.zeros(B, np.float64)
    steps = np.zeros(B, np.int64)

    def step(k):
        obs, rew, _, info = env.step(torch.from_numpy(acts[k]))
        r64 = oracle.rewards(obs.cpu().numpy(), env.cfg.reward_metric, env.cfg.reward_field,
                             f64=True)
        np.testing.assert_array_equal(r64.astype(np.float32), rew.cpu().numpy())
        total[:] = total + r64
        steps[:] = steps + 1
        ln, rt = episode_stats(env)
        np.testing.assert_array_equal(ln, steps, err_msg=f"episode length step {k}")
        np.testing.assert_array_equal(rt, total, err_msg=f"episode return step {k}")
        np.testing.assert_array_equal(info["episode_length"].cpu().numpy(), steps)
        np.testing.assert_array_equal(info["episode_return"].cpu().numpy(), total)

    for k in range(5):
        step(k)
    assert (total != 0).all() and len(np.unique(total.reshape(C, A), axis=1)[0]) > 1
    given = reset_mask(case)
    pool = np.repeat(given.reshape(C, A).any(1), A)
    assert given.sum() * A == pool.sum() and 0 < pool.sum() < B and A > 1
    env.reset(mask=torch.from_numpy(given.astype(np.uint8)))
    total[pool], steps[pool] = 0.0, 0
    ln, rt = episode_stats(env)
    np.testing.assert_array_equal(ln, steps, err_msg="episode length after the masked reset")
    np.testing.assert_array_equal(rt, total, err_msg="episode return after the masked reset")
    assert (ln[pool] == 0).all() and (rt[pool] == 0).all() and (ln[~pool] == 5).all()
    for k in range(5, 8):
        step(k)
    env.close()


@gpu
def test_same_step_autoreset_resets_whole_pools(lib):
    """autoreset=True with max_steps reached: the done mask of the step goes to the reset of a
    pool handle.  Equal, outputs and state, to stepping without autoreset and resetting by hand
    with the step's done mask; done is equal across a pool."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    case = "a3-s4-sed-levels"
    C, A, S, kw = case_kwargs(case)
    _, _, acts, _, _, _, _ = reference_run(case)
    opt = dict(device="cuda:0", balancers_per_pool=A, max_steps=3, **kw)
    auto = VecLoadBalanceEnv(C * A, S, autoreset=True, **opt)
    hand = VecLoadBalanceEnv(C * A, S, autoreset=False, **opt)
    np.testing.assert_array_equal(auto.reset().cpu().numpy(), hand.reset().cpu().numpy())
    resets = 0
    for k in range(7):
        a = torch.from_numpy(acts[k])
        oa, ra, da, ia = auto.step(a)
        oh, rh, dh, ih = hand.step(a)
        np.testing.assert_array_equal(da.cpu().numpy(), dh.cpu().numpy(), err_msg=f"done {k}")
        done = dh.cpu().numpy().reshape(C, A)
        assert (done == done[:, :1]).all()
        if done.any():
            oh = hand.reset(mask=dh)
            resets += 1
        np.testing.assert_array_equal(oa.cpu().numpy(), oh.cpu().numpy(), err_msg=f"obs {k}")
        np.testing.assert_array_equal(ra.cpu().numpy(), rh.cpu().numpy(), err_msg=f"reward {k}")
        np.testing.assert_array_equal(ia["episode_length"].cpu().numpy(),
                                      ih["episode_length"].cpu().numpy())
    assert resets == 2
    assert auto.handle.state_bytes() == hand.handle.state_bytes()
    assert (pool_state(auto)["ep_step"] == 1).all()
    auto.close()
    hand.close()
