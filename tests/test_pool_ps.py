"""Shared server pools of processor-sharing servers.

The reference is tests/pool_ps_ref.PoolPSSim, written from §3.24's text on top of PoolSim's member
streams with PSCoresSim's server restated over entries that carry their owner (absolute int64 us,
plain sorted lists; the §3.23 invariants asserted at every event).  One scenario per case: reset,
12 steps, a masked reset in the middle whose mask names ONE member of every third pool.

Not gpu: PoolPSSim with one member against PSCoresSim event for event; one server against
PSCoresSim fed a hand merge of the members' streams; what the scenarios reach; the accessor with
owners over csrc/lbsim_ps.h as a host program under the address and undefined-behaviour sanitizers
against a naive array model, its operations replayed through PoolPSSim; check_pool_config, the
argument rules and the plan; FIFO against PS completions on the references.
gpu: enabled handles against PoolPSSim after every reset and step through their state, outputs and
pool_ps_state(); the identities (A = 1 is a plain PS handle, cores all 1 is cores never set);
mid-run changes, a state round trip, graph replay across a rewrite of the cores, shards, auto-reset,
normalize_obs, the MARL view, every refusal; and the closed forms of queueing theory per member.
"""
import math
import os
import subprocess

import numpy as np
import pytest

from marllb_amd import _lib as lbffi
from marllb_amd import build, pools
from marllb_amd.env import make_config
from tests import parity
from tests import ps_cores_ref as pcr
from tests import test_flowsim_ref as fr
from tests import test_processor_sharing as tp
from tests import test_ps_cores as tc_
from tests import test_queueing_theory as qt
from tests import test_server_pools as tsp
from tests.parity import lib  # noqa: F401  (the fixture: fails a gpu test run without a device)
from tests.pool_ps_ref import REACH, PoolPSSim
from tests.pool_ref import PoolSim

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K = 128
STEPS, RESET_AT, CHANGE_AT = 12, 6, 3
POOL_PS_KERNEL = 5  # LBSIM_DYN_KERNEL_POOL_PS
gpu = pytest.mark.gpu
CONT = {"action_type": "continuous"}

# id: (pools C, balancers A, servers S, config kwargs, member rate spread or None)
# Pools x members 22 x 3, 33 x 2, 9 x 8, 17 x 4, 35 x 1 (two waves and a partly filled last one at
# every group width); S in {1, 2, 3, 4, 6, 16}; Q in {3, 8, 64}; the four policies, both action
# types, unequal member rates.  The rates put the one-core pools near or above saturation (full
# queues, drops, carries with n > c) and leave the pools with more cores lightly loaded; every
# (member, server) reservoir count stays at or below 128 (test_past_128_samples goes beyond).
CASES = {
    "a3-s4-sed-q8-levels": (22, 3, 4, {"discrete_weights": [0.5, 1.0, 8.0], "queue_capacity": 8,
                                       "arrival_rate": 20.0, "server_rates": [14.0] * 4,
                                       "warmup_steps": 2}, None),
    "a2-s3-lsq-q8-overload": (33, 2, 3, {"assign_policy": "lsq", "queue_capacity": 8,
                                         "arrival_rate": 30.0, "server_rates": [16.0] * 3,
                                         "warmup_steps": 2}, (0.6, 1.4)),
    "a8-s6-sed2-q64-continuous": (9, 8, 6, {"assign_policy": "sed2", **CONT, "queue_capacity": 64,
                                            "arrival_rate": 300.0, "server_rates": [380.0] * 6,
                                            "warmup_steps": 2, "step_interval": 0.05}, None),
    "a4-s1-q3-drops": (17, 4, 1, {"queue_capacity": 3, "arrival_rate": 8.0,
                                  "server_rates": [25.0], "warmup_steps": 2}, (0.5, 1.5)),
    "a1-s16-sed-q8-continuous": (35, 1, 16, {**CONT, "queue_capacity": 8, "arrival_rate": 160.0,
                                             "server_rates": [11.0] * 16, "warmup_steps": 2}, None),
    "a2-s2-lsq2-q8-fast": (33, 2, 2, {"assign_policy": "lsq2", "queue_capacity": 8,
                                      "arrival_rate": 12000.0, "server_rates": [20000.0, 12000.0],
                                      "warmup_steps": 2, "step_interval": 0.0005}, (0.7, 1.3)),
}
DEEP, FAST = "a8-s6-sed2-q64-continuous", "a2-s2-lsq2-q8-fast"
# beyond 128 samples per (member, server): 50 flows per step on each (test_past_128_samples)
PAST = {"a3-s2-sed-q64-past128": (5, 3, 2, {"queue_capacity": 64, "arrival_rate": 400.0,
                                            "server_rates": [700.0, 600.0], "warmup_steps": 2},
                                  None)}
ALL = {**CASES, **PAST}


def case_kwargs(case):
    C, A, S, kw, _ = ALL[case]
    return C, A, S, {"seed": 8400 + list(ALL).index(case), **kw}


def cores_of(C, S):
    """(C, S) counts: rows cycle 1, 2, 3, 4 by pool; pool 1's last server has 64."""
    c = np.repeat(1 + np.arange(C)[:, None] % 4, S, axis=1).astype(np.int32)
    if C > 1:
        c[1, S - 1] = 64
    return c


def member_rates(case, variant=0):
    C, A, S, kw = case_kwargs(case)
    spread = ALL[case][4]
    base = np.float32(kw["arrival_rate"])
    if spread is None and not variant:
        return None
    lo, hi = spread or (0.7, 1.3)
    rng = np.random.default_rng(1900 + 7 * list(ALL).index(case) + variant)
    return (base * rng.uniform(lo, hi, (C, A))).astype(np.float32)


def actions_of(case, steps=STEPS):
    C, A, S, kw = case_kwargs(case)
    rng = np.random.default_rng(150 + list(ALL).index(case))
    out = []
    for _ in range(steps):
        if kw.get("action_type") == "continuous":
            out.append(rng.uniform(-1.0, 11.0, (C * A, S)).astype(np.float32))
        else:
            n = len(kw.get("discrete_weights", [1.0, 1.5, 2.0]))
            out.append(rng.integers(-n, n, (C * A, S)).astype(np.int64))
    return out


def reset_mask(C, A):
    """One member (the last) of every third pool."""
    b = np.arange(C * A)
    return ((b // A) % 3 == 0) & (b % A == A - 1)


def make_pools(cfg, C, A, S, kw, rates, cores, cls=PoolPSSim):
    r = rates if rates is not None else np.full((C, A), np.float32(cfg.arrival_rate))
    extra = {} if cores is None else None
    return [cls(kw["seed"], cfg.env_id_offset + c * A, A, S, cfg.queue_capacity,
                kw.get("assign_policy", "sed"), r[c], [cfg.server_rate[s] for s in range(S)],
                dt=cfg.step_interval, warmup_steps=cfg.warmup_steps,
                **(extra if extra is not None else {"cores": cores[c]})) for c in range(C)]


class Snap:
    """What the reference says the state is after a reset (mask: the envs reset) or a step."""


def snapshot(sims, A, S, drops, mask=None, assigned=None):
    ev = Snap()
    ev.mask, ev.assigned, ev.dropped = mask, assigned, drops.copy()
    ev.in_flight = np.array([row for m in sims for row in m.in_flight()])
    ev.arr_idx = np.array([x.k for m in sims for x in m.members])
    ev.next_abs = np.array([x.next_arrival() for m in sims for x in m.members])
    ev.steps = np.array([m.step_no for m in sims for _ in range(A)])
    ev.queues = [[m.remaining(s) for s in range(S)] for m in sims]
    ev.acc = np.array([m.acc for m in sims])
    ev.res_count = np.array([m.res_count[a] for m in sims for a in range(A)])
    ev.res = [[list(m.res[a][s]) for s in range(S)] for m in sims for a in range(A)]
    ev.big = np.array([m.big[a] for m in sims for a in range(A)])
    ev.state = np.array([[m.state_row(a, s) for s in range(S)] for m in sims for a in range(A)],
                        np.float32)
    return ev


_RUNS = {}


def reference_run(case, cores="default", change=None, steps=STEPS):
    """The scenario on the case's PoolPSSims -> (cfg, kw, acts, snaps, rates, sims).  cores: (C, S)
    counts, None (never set) or "default" (cores_of).  change = ("cores", counts) or ("rates",
    rates): applied before step CHANGE_AT.  Computed once per key."""
    key = (case, cores if isinstance(cores, str) or cores is None else "given",
           change and change[0], steps)
    if key in _RUNS:
        return _RUNS[key]
    C, A, S, kw = case_kwargs(case)
    B = C * A
    cfg = make_config(B, S, **kw)
    rates = member_rates(case)
    if isinstance(cores, str):
        cores = cores_of(C, S)
    sims = make_pools(cfg, C, A, S, kw, rates, cores)
    drops = np.zeros(B, np.int64)
    acts = actions_of(case, steps)
    snaps = []

    def reset(mask):
        pool = mask.reshape(C, A).any(1)  # a pool resets iff any member's byte is set
        for c in np.flatnonzero(pool):
            drops[c * A:(c + 1) * A] = 0
            for r in sims[c].reset():
                drops[c * A:(c + 1) * A] += r.dropped
        snaps.append(snapshot(sims, A, S, drops, mask=np.repeat(pool, A)))

    reset(np.ones(B, bool))
    for k in range(steps):
        if k == RESET_AT:
            reset(reset_mask(C, A))
        if change is not None and k == CHANGE_AT:
            for c in range(C):
                if change[0] == "cores":
                    sims[c].set_cores(change[1][c])
                else:
                    for a in range(A):
                        sims[c].set_rate(a, change[1][c, a])
        w = fr.weights_of(acts[k], kw).reshape(C, A, S)
        assigned = np.zeros((B, S), np.int64)
        for c in range(C):
            r = sims[c].step(w[c])
            assigned[c * A:(c + 1) * A] = r.assigned
            drops[c * A:(c + 1) * A] += r.dropped
        snaps.append(snapshot(sims, A, S, drops, assigned=assigned))
    _RUNS[key] = (cfg, kw, acts, snaps, rates, sims)
    return _RUNS[key]


# ------------------------------------------------------------------ not gpu: the identities

@pytest.mark.parametrize("policy", tp.SCORE_POLICIES)
@pytest.mark.parametrize("case", list(fr.CASES))
def test_pool_of_one_equals_pscoressim(case, policy):
    """PoolPSSim with A = 1 is PSCoresSim event for event on every case of test_flowsim_ref.CASES
    under the four policies: completions, assignments, drops, queues, clock words, reservoirs."""
    S, kw = tp.ps_case_of(case, policy)
    cfg = make_config(tp.HOST_B, S, **kw)
    acts = fr.actions_of(case, tp.HOST_B)
    mu = [cfg.server_rate[s] for s in range(S)]
    flows = 0
    for b in range(tp.HOST_B):
        cores = [1 + (b + s) % 4 for s in range(S)]
        opt = dict(dt=cfg.step_interval, warmup_steps=cfg.warmup_steps, cores=cores)
        plain = pcr.PSCoresSim(kw["seed"], cfg.env_id_offset + b, S, cfg.queue_capacity, policy,
                               cfg.arrival_rate, mu, **opt)
        pool = PoolPSSim(kw["seed"], cfg.env_id_offset + b, 1, S, cfg.queue_capacity, policy,
                         [cfg.arrival_rate], mu, **opt)

        def same(ra, rb):
            np.testing.assert_array_equal(ra.assigned, rb.assigned[0])
            assert ra.dropped == rb.dropped[0]
            assert ra.completed == [(s, ta, tc) for (s, ta, tc, own) in rb.completed]
            assert plain.queues == [[(t, ta) for t, ta, _ in q] for q in pool.queues]
            assert (plain.V, plain.acc, plain.t_last) == (pool.V, pool.acc, pool.t_last)
            assert plain.res == pool.res[0] and plain.res_count == pool.res_count[0]
            assert plain.k == pool.members[0].k
            for s in range(S):
                assert plain.state_row(s) == [x for i, x in enumerate(pool.state_row(0, s))
                                              if i != 1]
                assert pool.state_row(0, s)[1] == 0
            return len(ra.completed)

        for ra, rb in zip(plain.reset(), pool.reset()):
            flows += same(ra, rb)
        for k in range(fr.STEPS):
            if k == fr.RESET_AT and b % 3 == 0:
                for ra, rb in zip(plain.reset(), pool.reset()):
                    same(ra, rb)
            wt = fr.weights_of(acts[k], kw)[b]
            flows += same(plain.step(wt), pool.step(wt[None]))
    assert flows > 10 * tp.HOST_B


@pytest.mark.parametrize("policy", ("sed", "lsq2"))
def test_more_cores_than_queue_slots_give_fct_equal_svc(policy):
    """c >= Q: no flow ever shares a core, so every flow of every member completes at ta + svc."""
    A, S, Q = 3, 2, 8
    pool = PoolPSSim(8802, 12, A, S, Q, policy, [40.0, 25.0, 60.0], [30.0, 45.0],
                     warmup_steps=2, cores=[64, 8])
    want, got = [], []
    rng = np.random.default_rng(5)
    for r in pool.reset():
        got += r.completed
    steps = 2
    for _ in range(10):
        want_step = pool.step(rng.uniform(0.5, 4.0, (A, S)).astype(np.float32))
        got += want_step.completed
        want += [(s, ta, ta + svc, a) for s, ta, svc, a in pool.assigned_log]
        steps += 1
        assert pool.acc == [0] * S
    end = steps * pool.dt
    # (the warm-up's flows were not logged: compare the flows that arrived after it)
    t0 = 2 * pool.dt
    assert sorted(x for x in got if x[1] >= t0) == sorted(x for x in want if x[2] <= end)
    assert len(want) > 100 and len({x[3] for x in want}) == A


class MergedPS(pcr.PSCoresSim):
    """PSCoresSim of one server fed a given arrival list instead of its own stream."""

    def feed(self, arr):
        self._ta = [t for t, _, _ in arr] + [1 << 60]
        self._work = [w for _, _, w in arr] + [np.float32(1.0)]
        self._u2 = [0] * (len(arr) + 1)

    def _draw_block(self):
        raise AssertionError("the merged list is the whole stream")


@pytest.mark.parametrize("A,Q,c,rate,mu", [(2, 64, 1, 20.0, 50.0), (4, 3, 2, 9.0, 12.0),
                                           (8, 8, 3, 6.0, 14.0)])
def test_one_server_equals_a_hand_merge(A, Q, c, rate, mu):
    """S = 1: the pool's completions equal PSCoresSim fed an independent merge of the A members'
    FlowSim arrival streams (sorted by (time, member); a full server drops)."""
    from tests.flowsim_ref import FlowSim
    seed, gid0, steps, warm = 1991 + A, 40 * A, 10, 2
    rates = [rate * (1 + 0.2 * a) for a in range(A)]
    pool = PoolPSSim(seed, gid0, A, 1, Q, "sed", rates, [mu], warmup_steps=warm, cores=[c])
    got, got_drops = [], np.zeros(A, np.int64)
    for r in pool.reset() + [pool.step(np.ones((A, 1), np.float32)) for _ in range(steps)]:
        got += r.completed
        got_drops += r.dropped
    end = (steps + warm) * pool.dt
    arr = []
    for a in range(A):
        m = FlowSim(seed, gid0 + a, 1, Q, "sed", rates[a], [mu], warmup_steps=0)
        m.reset()
        k = 0
        while m._arrival(k) < end:
            arr.append((m._ta[k], a, m._work[k]))
            k += 1
    arr.sort(key=lambda e: (e[0], e[1]))
    one = MergedPS(seed, gid0, 1, Q, "sed", rates[0], [mu], warmup_steps=0, cores=[c])
    one.reset()
    one.feed(arr)
    owner = {}
    for ta, a, _ in arr:
        owner.setdefault(ta, []).append(a)
    want, dropped_at = [], []
    for _ in range(steps + warm):
        k0 = one.k
        r = one.step(np.ones(1, np.float32))
        want += r.completed
        taken = {ta for _, ta, _, _ in one.assigned_log}
        dropped_at += [i for i in range(k0, one.k) if arr[i][0] not in taken]
    assert len({t for t, _, _ in arr}) == len(arr), "a tie in the merge: pick another seed"
    assert [(s, ta, tc) for s, ta, tc, _ in got] == want and len(want) > 10 * A
    assert all(own == owner[ta][0] for _, ta, _, own in got)
    drops = np.zeros(A, np.int64)
    for i in dropped_at:
        drops[arr[i][1]] += 1
    np.testing.assert_array_equal(got_drops, drops)
    assert len({own for (_, _, _, own) in got}) == A


def total_reach(cases=CASES):
    total = {k: 0 for k in REACH}
    for case in cases:
        sims = reference_run(case)[5]
        for m in sims:
            for k in REACH:
                total[k] += int(m.reach[k])
    return total


def test_scenarios_reach_everything_between_them():
    """Every situation §3.24's tests name is met by the GPU cases at their GPU batch sizes: two
    members' arrivals in one us, an insert at the head in front of another member's entry, a move
    of more than 8 entries of mixed owners, equal tags of different owners completing in one us in
    queue order, a drop at a physically full server where the member's own count is 0, a carry
    across a step boundary with n > c, a completion at exactly ta and at exactly dt; and no
    (member, server) reservoir passes 128 samples, so record c is completion c."""
    total = total_reach()
    print("REACH", total)
    assert all(total[k] > 0 for k in REACH), total
    for case in CASES:
        snaps = reference_run(case)[3]
        assert max(int(ev.res_count.max()) for ev in snaps) <= K, case
        assert sum(int(ev.res_count.sum()) for ev in snaps[-1:]) > 0


def test_fifo_and_ps_pools_differ_in_the_recorded_completions():
    """One seed, the same members, rates and weights: PoolSim (FIFO) and PoolPSSim with one core
    assign differently once a queue forms and complete the flows at other times."""
    args = (8801, 0, 3, 1, 64, "sed", [10.0, 6.0, 4.0], [40.0])
    fifo, ps = PoolSim(*args, warmup_steps=0), PoolPSSim(*args, warmup_steps=0)
    fifo.reset(), ps.reset()
    a, b = [], []
    ones = np.ones((3, 1), np.float32)
    for _ in range(40):
        a += fifo.step(ones).completed
        b += ps.step(ones).completed
    assert len(a) > 100 and abs(len(a) - len(b)) <= 64
    assert sorted(x[1] for x in a)[:100] == sorted(x[1] for x in b)[:100]  # the same arrivals
    fa, fb = {ta: tc for _, ta, tc, _ in a}, {ta: tc for _, ta, tc, _ in b}
    both = [ta for ta in fa if ta in fb]
    assert sum(fa[t] != fb[t] for t in both) > len(both) // 4
    assert any(fa[t] < fb[t] for t in both) and any(fa[t] > fb[t] for t in both)


# ------------------------------------------------------------------ not gpu: the accessor

def test_accessor_with_owners_against_a_naive_model(tmp_path):
    """tests/pool_ps_probe.cpp: the ring accessor whose entries carry their owner over
    csrc/lbsim_ps.h for Q in {3, 8, 9, 32, 64}, c in {1, 2, 3, 64}, A in {1, 3, 8} against a naive
    array model, under the address and undefined-behaviour sanitizers (a program of its own, run
    directly, as tests/test_ps_cores.py runs its probe); then its printed operations replayed
    through PoolPSSim."""
    exe = str(tmp_path / "pool_ps_probe")
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "pool_ps_probe.cpp")], check=True)
    r = subprocess.run([exe, "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert [tuple(row[:3]) for row in rows] == [(q, c, a) for q in (3, 8, 9, 32, 64)
                                                for c in (1, 2, 3, 64) for a in (1, 3, 8)]
    tot = np.zeros(5, np.int64)
    for q, c, a, *counts in rows:
        assert counts[0] > 100 and counts[1] > 100, (q, c, a)
        if a == 1:
            assert counts[2] == counts[3] == counts[4] == 0
        elif q >= 32 and c < 64:
            assert counts[2] > 0 and counts[3] > 0 and counts[4] > 0, (q, c, a, counts)
        tot += counts
    assert tot.min() > 0, tot
    r = subprocess.run([exe, "1", "trace"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    seen = replay_probe_trace(r.stdout.splitlines())
    assert seen["Q"] == [(q, c, a) for q in (3, 8, 9, 32, 64) for c in (1, 2, 3, 64)
                         for a in (1, 3, 8)]
    assert min(seen[k] for k in ("A", "C", "D", "E")) > 100, seen


def replay_probe_trace(lines, dt=50000):
    """Every operation the probe did, done again by PoolPSSim's own methods: the completions it
    pops before each operation are the probe's (times, order and owners), an insert lands at the
    probe's position with its owner, and at a step end the carry, the entries {remaining, ta,
    owner}, the work and the drain are the probe's."""
    seen = {"Q": [], "A": 0, "C": 0, "D": 0, "E": 0}
    sim, base, pending = None, 0, []

    def pops(t, at_arrival=True):
        done = []
        sim._pop_due(t, done, at_arrival)
        assert [(tc - base, ta - base, own) for _, ta, tc, own in done] == pending, (done, pending)
        seen["C"] += len(pending)
        pending.clear()

    for line in lines:
        op, *v = line.split()
        v = [int(x) for x in v]
        if op == "Q":
            assert not pending
            sim = PoolPSSim(7700, 0, v[2], 1, v[0], "lsq", [10.0] * v[2], [10.0], dt=dt * 1e-6,
                            warmup_steps=0, cores=[v[1]])
            sim.reset()
            base = 0
            seen["Q"].append((v[0], v[1], v[2]))
        elif op == "C":
            pending.append((v[0], v[1], v[2]))
        elif op == "A":
            pops(base + v[0])
            sim._insert(0, base + v[0], v[1], v[3])
            assert sim.queues[0][v[2]] == (sim.V[0] + v[1], base + v[0], v[3]), ("position", line)
            seen["A"] += 1
        elif op == "D":
            pops(base + v[0])
            assert len(sim.queues[0]) == sim.Q
            seen["D"] += 1
        elif op == "E":
            pops(base + dt, at_arrival=False)
            sim._advance(0, base + dt)
            sim.step_no += 1
            base += dt
            assert sim.acc[0] == v[0] and len(sim.queues[0]) == v[1], line
            assert sim.server_state(0)[2:] == (v[2], v[3]), (line, sim.server_state(0))
            want = [(v[4 + 3 * i], v[5 + 3 * i], v[6 + 3 * i]) for i in range(v[1])]
            assert [(rem, ta - base, own) for rem, ta, own in sim.remaining(0)] == want, line
            seen["E"] += 1
    return seen


# ------------------------------------------------------------------ not gpu: rules and the plan

def test_check_pool_config_and_the_interface():
    """check_pool_config(pool_discipline="ps") accepts what "fifo" accepts and refuses what it
    refuses, with the same words; any other discipline is a ValueError; the constructor's
    argument rules come before a device; the header declares the entry points and ctypes knows
    them; the ABI version stays."""
    from marllb_amd.env import VecLoadBalanceEnv
    ok = make_config(24, 4, assign_policy="lsq2", arrival_rate=50.0)
    pools.check_pool_config(ok, 3, pool_discipline="ps")
    pools.check_pool_config(ok, 3, pool_discipline="fifo")
    pools.check_pool_config(ok, 3)
    with pytest.raises(ValueError, match="pool_discipline"):
        pools.check_pool_config(ok, 3, pool_discipline="lifo")
    for what, kw in tsp.refused_configs().items():
        kw = dict(kw)
        S = kw.pop("S", 4)
        for disc in ("fifo", "ps"):
            with pytest.raises(lbffi.LbsimError, match=what) as e:
                pools.check_pool_config(make_config(24, S, seed=1, **kw), 2, pool_discipline=disc)
            assert e.value.code == lbffi.ENOTSUP
    for what, opt in tsp.REFUSED_OPTIONS.items():
        with pytest.raises(lbffi.LbsimError, match=what):
            pools.check_pool_config(ok, 2, pool_discipline="ps", **opt)
    for bad in (0, 9, 5):
        with pytest.raises(ValueError):
            pools.check_pool_config(ok, bad, pool_discipline="ps")
    # the constructor, before a device is touched (device index 99 does not exist)
    with pytest.raises(ValueError, match="pool_discipline"):
        VecLoadBalanceEnv(24, 4, device="cuda:99", balancers_per_pool=3, pool_discipline="lifo")
    with pytest.raises(ValueError, match="balancers_per_pool"):
        VecLoadBalanceEnv(24, 4, device="cuda:99", pool_discipline="ps")
    with pytest.raises(lbffi.LbsimError, match="lbsim_server_pool_enable_ps") as e:
        VecLoadBalanceEnv(24, 4, device="cuda:99", balancers_per_pool=3, pool_ps_cores=[1] * 4)
    assert e.value.code == lbffi.ENOTSUP
    with pytest.raises(lbffi.LbsimError) as e:  # the old refusal, unchanged
        VecLoadBalanceEnv(24, 4, device="cuda:99", balancers_per_pool=3, service_discipline="ps")
    assert e.value.code == lbffi.ENOTSUP
    header = open(os.path.join(ROOT, "include", "lbsim.h")).read()
    for name, nargs in (("lbsim_server_pool_enable_ps", 2), ("lbsim_server_pool_discipline", 1),
                        ("lbsim_set_pool_ps_cores", 4), ("lbsim_get_pool_ps_cores", 3),
                        ("lbsim_clear_pool_ps_cores", 2), ("lbsim_pool_ps_state", 3)):
        assert f"int {name}(" in header and len(lbffi._SIGNATURES[name][1]) == nargs
    assert "size_t lbsim_pool_ps_state_cols(void);" in header
    assert "#define LBSIM_ABI_VERSION 10 " in header and "LBSIM_DYN_KERNEL_POOL_PS = 5" in header
    assert "#define LBSIM_POOL_PS_STATE_COLS 5" in header
    from marllb_amd import env as envmod
    assert envmod.POOL_PS_STATE_COLUMNS == ("n", "n_others", "busy_cores", "work_s", "drain_s")


PLAN_PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include "marllb_amd/csrc/lbsim_plan.h"
int main(int argc, char** argv) {
  lbk::PlanInput in{};
  in.B = std::atoi(argv[1]), in.S = std::atoi(argv[2]), in.Q = std::atoi(argv[3]);
  in.policy = std::atoi(argv[4]);
  in.dyn_mapping = LBSIM_DYN_AUTO, in.step_kernel = std::atoi(argv[5]), in.simds = 1024;
  in.pool = std::atoi(argv[6]);
  in.pool_ps = std::atoi(argv[7]) != 0;
  const lbk::StepPlan p = lbk::make_plan(in, lbk::Overrides::from_env());
  std::printf("%d %d %d %u %u %d %d %d %u %d %d\n", p.form, p.dyn.kernel, p.dyn.width, p.dyn.grid,
              p.dyn.block, p.reset_dyn.kernel, p.reset_dyn.width, p.obs.form, p.obs.grid,
              (int)p.nr, p.dyn.epw);
  return 0;
}
"""


def test_plan_of_a_ps_pool_input(tmp_path):
    """make_plan (csrc/lbsim_plan.h, compiled alone): pool_ps plans exactly as the FIFO pool does
    -- groups of pow2 >= max(S, A) lanes, 64 / G pools per wave, the two-launch step with the
    ordinary paired observe -- but for the kernel it names; pool_ps = false is the plan of
    before."""
    src, exe = tmp_path / "pool_ps_plan_probe.cpp", str(tmp_path / "pool_ps_plan_probe")
    src.write_text(PLAN_PROBE)
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", f"-I{ROOT}", "-o",
                    exe, str(src)], check=True)

    def plan(B, S, A, ps, Q=8, step_kernel=0, env=None):
        e = {k: v for k, v in os.environ.items() if not k.startswith("LBSIM_")}
        e.update(env or {})
        out = subprocess.run([exe] + [str(x) for x in (B, S, Q, 0, step_kernel, A, ps)],
                             capture_output=True, text=True, check=True, env=e).stdout.split()
        return dict(zip(("form", "kernel", "width", "grid", "block", "rkernel", "rwidth", "obs",
                         "obs_grid", "nr", "epw"), map(int, out)))

    TWO_LAUNCH, OBS_PAIR = 2, 0  # kStepTwoLaunch, kObsPair
    for C in (22, 4096):
        for S, A, g in ((1, 1, 2), (4, 3, 4), (3, 2, 4), (6, 8, 8), (1, 4, 4), (16, 1, 16),
                        (2, 8, 8)):
            for sk in (0, 1, 2):
                ps = plan(C * A, S, A, 1, step_kernel=sk)
                fifo = plan(C * A, S, A, 0, step_kernel=sk)
                assert ps["kernel"] == ps["rkernel"] == POOL_PS_KERNEL
                assert fifo["kernel"] == fifo["rkernel"] == tsp.POOL_KERNEL
                assert {k: v for k, v in ps.items() if "kernel" not in k} == \
                    {k: v for k, v in fifo.items() if "kernel" not in k}
                assert ps["form"] == TWO_LAUNCH and ps["width"] == ps["rwidth"] == g
                assert ps["block"] == 64 and ps["grid"] == -(-C // (64 // g))
                if S <= 8:
                    assert ps["obs"] == OBS_PAIR
    assert plan(66, 3, 2, 1, env={"LBSIM_DYN_GROUP_LANES": "8"})["width"] == 8
    assert plan(66, 3, 8, 1, env={"LBSIM_DYN_GROUP_LANES": "4"})["width"] == 8  # too narrow
    assert plan(66, 3, 2, 1, env={"LBSIM_DYN_WAVE": "1"})["kernel"] == POOL_PS_KERNEL
    assert plan(2048, 4, 0, 0, Q=32)["kernel"] == parity.WAVE  # no pools: the plans of before


# ------------------------------------------------------------------ the device

class DeviceBackend:
    """reset / step -> (obs, reward or None, assign counts or None), numpy."""

    def __init__(self, case, cores="default", rates="default", **extra):
        import torch
        from marllb_amd.env import VecLoadBalanceEnv
        C, A, S, kw = case_kwargs(case)
        self.torch = torch
        if isinstance(cores, str):
            cores = cores_of(C, S)
        self.env = VecLoadBalanceEnv(C * A, S, device="cuda:0", autoreset=False,
                                     balancers_per_pool=A, pool_discipline="ps",
                                     pool_ps_cores=cores, **{**kw, **extra})
        if isinstance(rates, str):
            rates = member_rates(case)
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


class PoolPSCheck:
    """A Snap of the reference against an enabled handle's state, outputs and pool_ps_state()."""

    def __init__(self, env):
        self.env, self.cfg = env, env.cfg
        self.B, self.S, self.A = env.cfg.num_envs, env.cfg.num_servers, env.balancers_per_pool
        self.dt = int(round(env.cfg.step_interval * 1e6))

    def __call__(self, ev, out):
        B, S, A, Q = self.B, self.S, self.A, self.cfg.queue_capacity
        obs, rew, assign = out
        d = tsp.pool_state(self.env)
        if assign is not None:
            np.testing.assert_array_equal(assign, ev.assigned, err_msg="assign_counts")
        np.testing.assert_array_equal(d["dropped"], ev.dropped, err_msg="dropped")
        np.testing.assert_array_equal(d["arr_idx"], ev.arr_idx, err_msg="arrival index")
        np.testing.assert_array_equal(d["clock"], ev.steps, err_msg="clock")
        np.testing.assert_array_equal(d["next_arr"].astype(np.int64) + ev.steps * self.dt,
                                      ev.next_abs, err_msg="next arrival")
        hc = d["hc"].reshape(B, S)
        own = (hc >> 16).astype(np.int64)
        np.testing.assert_array_equal(own, ev.in_flight, err_msg="own counts (hc >> 16)")
        np.testing.assert_array_equal(obs[:, :, 0], ev.in_flight.astype(np.float32),
                                      err_msg="observation column 0")
        np.testing.assert_array_equal((hc & 0x8000) != 0, ev.big, err_msg="big flags")
        # the physical server: count, {remaining tag, ta} and owners by position from the head
        ring = d["ring"].reshape(B, S, Q, 2).astype(np.int64)
        for c, queues in enumerate(ev.queues):
            base = int(ev.steps[c * A]) * self.dt
            for s, q in enumerate(queues):
                w = int(d["pool_hc"][c, s])
                h, n = w & 0x7FFF, w >> 16
                assert n == len(q), ("physical count", c, s)
                assert all((int(x) & 0x7FFF) == h for x in hc[c * A:(c + 1) * A, s])
                pos = [(h + i) % Q for i in range(n)]
                got = [(int(ring[c * A, s, p, 0]), int(ring[c * A, s, p, 1]) + base,
                        int(d["pool_owner"][c, s, p])) for p in pos]
                assert got == q, ("physical entries", c, s)
        assert (own.reshape(-1, A, S).sum(1) == (d["pool_hc"] >> 16)).all()
        np.testing.assert_array_equal(d["last_tc"].reshape(B // A, A, S),
                                      np.repeat(ev.acc[:, None, :], A, 1), err_msg="last_tc == acc")
        np.testing.assert_array_equal(d["res_count"].reshape(B, S), ev.res_count,
                                      err_msg="res_count")
        fct, ts = d["res_fct"].reshape(B, S, K), d["res_ts"].reshape(B, S, K)
        for b in range(B):
            for s in range(S):
                for k, rec in enumerate(ev.res[b][s]):
                    if rec is not None:
                        assert (int(fct[b, s, k]), int(ts[b, s, k])) == rec, ("record", b, s, k)
        tsp.check_features(self.env, d, obs, rew, "PS pool handle")
        st = self.env.pool_ps_state().cpu().numpy()
        np.testing.assert_array_equal(st, ev.state, err_msg="pool_ps_state")


def check_pool_ps_kernel(lib, env):
    for reset in (False, True):
        names = lib.launch_names(env.handle, 1 if reset else 0)
        assert lib.load().lbsim_dynamics_kernel(env.handle.h) == POOL_PS_KERNEL, names
        name = names.get(2 if reset else 0, "")
        assert name.startswith("dynamics_pool_ps_kernel<"), names
        lanes = os.environ.get("LBSIM_DYN_GROUP_LANES")
        need = max(env.cfg.num_servers, env.balancers_per_pool)
        if lanes and int(lanes) >= need:
            assert name.startswith(f"dynamics_pool_ps_kernel<{lanes},"), names
    h = env.handle
    assert h.server_pool_size() == env.balancers_per_pool and h.server_pool_discipline() == 1
    assert not h.processor_sharing()


def drive(back, check, acts, snaps, change=None, steps=STEPS):
    C, A = back.env.num_envs // back.env.balancers_per_pool, back.env.balancers_per_pool
    it = iter(snaps)
    check(next(it), back.reset(None))
    for k in range(steps):
        if k == RESET_AT:
            check(next(it), back.reset(reset_mask(C, A).astype(np.uint8)))
        if change is not None and k == CHANGE_AT:
            change(back)
        check(next(it), back.step(acts[k]))


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_enabled_handles_equal_the_reference(lib, case):
    """After every reset and each of 12 steps, with a one-member masked reset in the middle: the
    members' counters and own counts, the physical entries with owners in order, last_tc == acc,
    res_count, every record and timestamp, columns 1-10 and the reward, and pool_ps_state(),
    exact."""
    _, _, acts, snaps, _, _ = reference_run(case)
    back = DeviceBackend(case)
    drive(back, PoolPSCheck(back.env), acts, snaps)
    check_pool_ps_kernel(lib, back.env)
    np.testing.assert_array_equal(back.env.get_pool_ps_cores().cpu().numpy(),
                                  cores_of(*case_kwargs(case)[0:3:2]))
    back.env.close()


FORCED = {4: ["a2-s2-lsq2-q8-fast", "a3-s4-sed-q8-levels", "a2-s3-lsq-q8-overload"],
          8: ["a2-s2-lsq2-q8-fast", "a4-s1-q3-drops", "a8-s6-sed2-q64-continuous"],
          16: ["a2-s2-lsq2-q8-fast", "a3-s4-sed-q8-levels"]}


@gpu
@pytest.mark.parametrize("lanes", list(FORCED))
def test_forced_group_widths(lanes):
    """LBSIM_DYN_GROUP_LANES = 4, 8, 16: groups at and above what max(S, A) asks for (the lanes
    past S and A hold neither a server nor a member); the child checks the launched width."""
    ks = [f"test_enabled_handles_equal_the_reference[{c}]" for c in FORCED[lanes]]
    own = {c: tsp.pools_width(CASES[c][2], CASES[c][1]) for c in FORCED[lanes]}
    assert any(CASES[c][1] > 1 and own[c] < lanes for c in FORCED[lanes]), own
    parity.run_cases_in_child("test_pool_ps.py", ks, {"LBSIM_DYN_GROUP_LANES": str(lanes)})


@gpu
def test_past_128_samples(lib):
    """More than 128 completions per (member, server): the slots follow the owner's reservoir
    stream at the owner's count."""
    case = "a3-s2-sed-q64-past128"
    _, _, acts, snaps, _, sims = reference_run(case)
    assert min(min(min(r) for r in m.res_count) for m in sims) > K
    back = DeviceBackend(case)
    drive(back, PoolPSCheck(back.env), acts, snaps)
    back.env.close()


def run_steps(env, acts, lo=0, hi=None):
    import torch
    outs = []
    for a in acts[lo:hi]:
        o, r, dn, info = env.step(torch.from_numpy(a), assign_counts=True)
        outs.append((o.cpu().numpy(), r.cpu().numpy(), dn.cpu().numpy(),
                     info["assign_counts"].cpu().numpy()))
    return outs


@gpu
@pytest.mark.parametrize("case", ["a1-s16-sed-q8-continuous", "a4-s1-q3-drops"])
def test_pool_of_one_is_a_plain_ps_handle(lib, case):
    """A = 1 against service_discipline="ps" with the same cores, bit for bit: observation,
    reward, assign counts, every state section the plain handle has, and the privileged view."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    C, A, S, kw = case_kwargs(case)
    B = C * A  # (the 17 x 4 case runs as 68 pools of one)
    cores = cores_of(B, S)
    acts = actions_of(case)
    opt = dict(device="cuda:0", autoreset=False, **kw)
    pool = VecLoadBalanceEnv(B, S, balancers_per_pool=1, pool_discipline="ps", pool_ps_cores=cores,
                             **opt)
    plain = VecLoadBalanceEnv(B, S, service_discipline="ps", ps_cores=cores, **opt)

    def same_state():
        a, b = pool.handle.state_bytes(), plain.handle.state_bytes()
        assert a[:len(b)] == b and len(a) == len(b) + B * S * 4 + B * S * kw["queue_capacity"]
        st = pool.pool_ps_state().cpu().numpy()
        np.testing.assert_array_equal(st[:, :, [0, 2, 3, 4]], plain.ps_state().cpu().numpy())
        assert not st[:, :, 1].any()

    np.testing.assert_array_equal(pool.reset().cpu().numpy(), plain.reset().cpu().numpy())
    same_state()
    for k in range(STEPS):
        if k == RESET_AT:
            m = torch.from_numpy((np.arange(B) % 3 == 0).astype(np.uint8))
            np.testing.assert_array_equal(pool.reset(mask=m).cpu().numpy(),
                                          plain.reset(mask=m).cpu().numpy())
        tsp.same_outputs(run_steps(pool, acts, k, k + 1), run_steps(plain, acts, k, k + 1))
        same_state()
    assert lib.load().lbsim_dynamics_kernel(pool.handle.h) == POOL_PS_KERNEL
    assert lib.load().lbsim_dynamics_kernel(plain.handle.h) == tp.PS_KERNEL
    pool.close()
    plain.close()


@gpu
def test_all_ones_is_a_handle_that_never_set_cores(lib):
    """Cores all 1 (set), set and cleared, and never set: the same outputs and state bytes, and
    the reference run with no cores given."""
    case = "a3-s4-sed-q8-levels"
    C, A, S, kw = case_kwargs(case)
    acts = actions_of(case)
    never = DeviceBackend(case, cores=None)
    ones = DeviceBackend(case, cores=np.ones((C, S), np.int32))
    cleared = DeviceBackend(case, cores=cores_of(C, S))
    cleared.env.clear_pool_ps_cores()
    assert (cleared.env.get_pool_ps_cores().cpu().numpy() == 1).all()
    assert (never.env.get_pool_ps_cores().cpu().numpy() == 1).all()
    envs = [never.env, ones.env, cleared.env]
    obs = [e.reset().cpu().numpy() for e in envs]
    np.testing.assert_array_equal(obs[0], obs[1])
    np.testing.assert_array_equal(obs[0], obs[2])
    outs = [run_steps(e, acts, 0, 6) for e in envs]
    tsp.same_outputs(outs[0], outs[1])
    tsp.same_outputs(outs[0], outs[2])
    assert never.env.handle.state_bytes() == ones.env.handle.state_bytes() \
        == cleared.env.handle.state_bytes()
    # the reference with cores never given is the same run
    _, _, racts, snaps, _, _ = reference_run(case, cores=None)
    chk = DeviceBackend(case, cores=None)
    drive(chk, PoolPSCheck(chk.env), racts, snaps)
    for e in envs + [chk.env]:
        e.close()


@gpu
@pytest.mark.parametrize("what", ["cores", "rates"])
def test_mid_run_change(lib, what):
    """set_pool_ps_cores / set_rates(arrival_rate) before step 3: queued flows keep their
    remaining tags and the carry, the arrival already drawn keeps its time."""
    case = "a3-s4-sed-q8-levels" if what == "cores" else "a2-s3-lsq-q8-overload"
    C, A, S, kw = case_kwargs(case)
    new = np.roll(cores_of(C, S), 1, axis=0) if what == "cores" else member_rates(case, variant=1)
    _, _, acts, snaps, _, _ = reference_run(case, change=(what, new))
    back = DeviceBackend(case)

    def change(b):
        if what == "cores":
            b.env.set_pool_ps_cores(new)
        else:
            b.set_rates(new)

    drive(back, PoolPSCheck(back.env), acts, snaps, change=change)
    back.env.close()


@gpu
def test_state_round_trip_continues_identically(lib):
    """get_state -> set_state into a fresh handle: the run continues bit for bit; a FIFO pool's
    snapshot has the same size (no new section) and a plain handle's another."""
    case = DEEP
    acts = actions_of(case)
    a, b = DeviceBackend(case), DeviceBackend(case)
    a.reset(None)
    run_steps(a.env, acts, 0, 5)
    snap = a.env.handle.state_bytes()
    b.env.reset()
    b.env.handle.load_state(snap)
    assert b.env.handle.state_bytes() == snap
    tsp.same_outputs(run_steps(a.env, acts, 5), run_steps(b.env, acts, 5))
    assert a.env.handle.state_bytes() == b.env.handle.state_bytes()
    np.testing.assert_array_equal(a.env.pool_ps_state().cpu().numpy(),
                                  b.env.pool_ps_state().cpu().numpy())
    from marllb_amd.env import VecLoadBalanceEnv
    C, A, S, kw = case_kwargs(case)
    fifo = VecLoadBalanceEnv(C * A, S, device="cuda:0", autoreset=False, balancers_per_pool=A, **kw)
    assert fifo.handle.state_size() == len(snap)
    for env in (a.env, b.env, fifo):
        env.close()


@gpu
def test_replayed_graph_across_a_rewrite_of_the_cores(lib):
    """One step captured into a graph and replayed five times equals five eager steps, with the
    cores rewritten in place between the second and the third replay."""
    import torch
    case = "a3-s4-sed-q8-levels"
    C, A, S, kw = case_kwargs(case)
    acts = actions_of(case)
    new = np.roll(cores_of(C, S), 2, axis=0)
    eager = DeviceBackend(case)
    g = DeviceBackend(case, graph_mode=True)
    eager.reset(None)
    g.env.reset()
    a_buf = torch.from_numpy(acts[0]).to("cuda:0")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = g.env.step(a_buf)  # warm the buffers
        torch.cuda.synchronize()
    eager.step(acts[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        out = g.env.step(a_buf)
    for k in range(1, 6):  # (capture runs nothing)
        if k == 3:
            g.env.set_pool_ps_cores(new)
            eager.env.set_pool_ps_cores(new)
        a_buf.copy_(torch.from_numpy(acts[k]))
        graph.replay()
        torch.cuda.synchronize()
        o, r, _ = eager.step(acts[k])
        np.testing.assert_array_equal(out[0].cpu().numpy(), o, err_msg=f"obs replay {k}")
        np.testing.assert_array_equal(out[1].cpu().numpy(), r, err_msg=f"reward replay {k}")
    assert g.env.handle.state_bytes() == eager.env.handle.state_bytes()
    g.env.close()
    eager.env.close()


@gpu
def test_two_uneven_shards_equal_one_handle(lib):
    """Pools 0-12 and 13-21 of the 22 x 3 case on two handles (env_id_offset a multiple of A, each
    passing its own rows of the cores) equal the one handle, outputs and state."""
    from marllb_amd.env import VecLoadBalanceEnv
    case = "a3-s4-sed-q8-levels"
    C, A, S, kw = case_kwargs(case)
    acts = actions_of(case)
    cores = cores_of(C, S)
    whole = DeviceBackend(case)
    whole.reset(None)
    ref = run_steps(whole.env, acts, 0, 6)
    cut = 13
    parts = [VecLoadBalanceEnv(n * A, S, device="cuda:0", autoreset=False, balancers_per_pool=A,
                               pool_discipline="ps", pool_ps_cores=cores[lo:lo + n],
                               env_id_offset=lo * A, **kw) for lo, n in ((0, cut), (cut, C - cut))]
    for p in parts:
        p.reset()
    got = [run_steps(p, [a[lo * A:hi * A] for a in acts], 0, 6)
           for p, (lo, hi) in zip(parts, ((0, cut), (cut, C)))]
    for k in range(6):
        for i, name in enumerate(("obs", "reward", "done", "assign")):
            np.testing.assert_array_equal(np.concatenate([got[0][k][i], got[1][k][i]]), ref[k][i],
                                          err_msg=f"{name} step {k}")
    d = tsp.pool_state(whole.env)
    ds = [tsp.pool_state(p) for p in parts]
    for name in ("hc", "res_count", "next_arr", "arr_idx", "dropped", "pool_hc", "res", "last_tc",
                 "pool_owner"):
        np.testing.assert_array_equal(np.concatenate([x[name].reshape(-1) for x in ds]),
                                      d[name].reshape(-1), err_msg=name)
    np.testing.assert_array_equal(
        np.concatenate([p.pool_ps_state().cpu().numpy() for p in parts]),
        whole.env.pool_ps_state().cpu().numpy())
    for e in (whole.env, *parts):
        e.close()


@gpu
def test_same_step_autoreset_resets_whole_pools(lib):
    """autoreset=True with max_steps reached equals stepping without it and resetting by hand with
    the step's done mask; done is equal across a pool."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    case = "a3-s4-sed-q8-levels"
    C, A, S, kw = case_kwargs(case)
    acts = actions_of(case)
    opt = dict(device="cuda:0", balancers_per_pool=A, pool_discipline="ps",
               pool_ps_cores=cores_of(C, S), max_steps=3, **kw)
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
    assert resets == 2 and auto.handle.state_bytes() == hand.handle.state_bytes()
    ln, _ = tsp.episode_stats(auto)
    assert (ln == 1).all()
    auto.close()
    hand.close()


@gpu
def test_normalize_obs_vpp_export_and_the_marl_view(lib):
    """normalize_obs: the raw rows are the un-normalised handle's.  lbsim_vpp_export's n_flow_on is
    column 0.  VecServerPoolEnv(pool_discipline="ps"): the flat env's outputs reshaped, true_state()
    (C, S, 5) the leader's rows with column 1 zero, others_load() column 1, the cores forwarded."""
    import torch
    from marllb_amd import VecServerPoolEnv
    case = "a3-s4-sed-q8-levels"
    C, A, S, kw = case_kwargs(case)
    B = C * A
    _, _, acts, snaps, _, _ = reference_run(case)
    plain, norm = DeviceBackend(case), DeviceBackend(case, normalize_obs=True)
    view = VecServerPoolEnv(C, A, S, device="cuda:0", autoreset=False, pool_discipline="ps",
                            pool_ps_cores=cores_of(C, S), **kw)
    o0 = plain.env.reset().cpu().numpy()
    norm.env.reset()
    v0 = view.reset()
    assert tuple(v0.shape) == (C, A, S, 11)
    np.testing.assert_array_equal(v0.cpu().numpy().reshape(B, S, 11), o0)
    for k in range(4):
        o, r, _, _ = plain.env.step(torch.from_numpy(acts[k]))
        on, _, _, info = norm.env.step(torch.from_numpy(acts[k]), raw_obs=True)
        np.testing.assert_array_equal(info["raw_obs"].cpu().numpy(), o.cpu().numpy())
        assert np.isfinite(on.cpu().numpy()).all()
        vo, vr, vd, _ = view.step(torch.from_numpy(acts[k]).view(C, A, S))
        np.testing.assert_array_equal(vo.cpu().numpy().reshape(B, S, 11), o.cpu().numpy())
        np.testing.assert_array_equal(vr.cpu().numpy().reshape(-1), r.cpu().numpy())
        assert tuple(vd.shape) == (C,)
    assert not np.array_equal(on.cpu().numpy(), o.cpu().numpy())
    tv = torch.empty((B, S, 2, 128, 2), dtype=torch.float32, device="cuda:0")
    nfo = torch.empty((B, S), dtype=torch.int32, device="cuda:0")
    ts = torch.empty(B, dtype=torch.float32, device="cuda:0")
    h = plain.env.handle
    h.check(h.lib.lbsim_vpp_export(h.h, 0, B, tv.data_ptr(), nfo.data_ptr(), ts.data_ptr(),
                                   plain.env._stream()))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(nfo.cpu().numpy().astype(np.float32), o.cpu().numpy()[:, :, 0])
    assert nfo.sum() > 0
    st, ol = view.true_state().cpu().numpy(), view.others_load().cpu().numpy()
    assert st.shape == (C, S, 5) and ol.shape == (C, A, S)
    want = snaps[4].state.reshape(C, A, S, 5)  # after the reset and four steps
    np.testing.assert_array_equal(st[:, :, [0, 2, 3, 4]], want[:, 0][:, :, [0, 2, 3, 4]])
    assert not st[:, :, 1].any()
    np.testing.assert_array_equal(ol, want[..., 1])
    assert ol.sum() > 0
    np.testing.assert_array_equal(view.get_pool_ps_cores().cpu().numpy(), cores_of(C, S))
    view.clear_pool_ps_cores()
    assert (view.get_pool_ps_cores().cpu().numpy() == 1).all()
    view.set_pool_ps_cores([2] * S)
    assert (view.pool_ps_state().cpu().numpy().shape) == (B, S, 5)
    for e in (plain.env, norm.env):
        e.close()
    view.close()


@gpu
def test_refusals(lib):
    """The old refusals, walked unchanged on the handles they were written for, and the new ones by
    name."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    L = lib.load()
    def mk(**kw):
        return VecLoadBalanceEnv(12, 4, device="cuda:0", autoreset=False, seed=5, **kw)

    env = mk(balancers_per_pool=3, pool_discipline="ps")
    h = env.handle
    assert h.server_pool_discipline() == 1 and h.server_pool_size() == 3
    assert not h.processor_sharing()
    # every refusal of a pool handle holds
    for fn in (h.enable_flow_stats, h.enable_server_avail, h.enable_cross_traffic,
               h.enable_server_workers, h.enable_action_delay):
        with pytest.raises(lbffi.LbsimError) as e:
            fn()
        assert e.value.code == lbffi.ENOTSUP and "server pools" in str(e.value)
    with pytest.raises(lbffi.LbsimError) as e:
        env.set_rates(server_rates=torch.full((12, 4), 100.0))
    assert e.value.code == lbffi.ENOTSUP
    with pytest.raises(lbffi.LbsimError, match="server pools") as e:
        h.enable_processor_sharing()
    assert e.value.code == lbffi.ENOTSUP
    # it is not a lbsim_processor_sharing_enable handle
    c4 = torch.ones((1, 4), dtype=torch.int32, device="cuda:0")
    for fn in (lambda: h.set_ps_cores(c4, rows=1), h.ps_cores, h.clear_ps_cores,
               lambda: h.ps_server_state(torch.zeros((12, 4, 4), device="cuda:0"))):
        with pytest.raises(lbffi.LbsimError, match="lbsim_processor_sharing_enable") as e:
            fn()
        assert e.value.code == lbffi.ENOTSUP
    # the other way round
    h.enable_server_pool_ps(3)  # the same value: a no-op
    with pytest.raises(ValueError, match="already on"):
        h.enable_server_pool_ps(2)
    with pytest.raises(ValueError, match="processor-sharing"):
        h.enable_server_pool(3)
    env.reset()
    with pytest.raises(lbffi.LbsimError, match="lbsim_pool_ps_state") as e:
        env.ground_truth()
    assert e.value.code == lbffi.ENOTSUP
    with pytest.raises(lbffi.LbsimError) as e:  # a per-env fork would tear a pool apart
        h.state_save(torch.zeros(h.state_size() + 16, dtype=torch.uint8, device="cuda:0"))
    assert e.value.code == lbffi.ENOTSUP
    # the cores' argument rules: a bad count leaves what was in force
    env.set_pool_ps_cores([1, 2, 3, 64])
    for bad in ([0, 1, 1, 1], [1, 1, 65, 1]):
        with pytest.raises(ValueError, match="outside"):
            env.set_pool_ps_cores(bad)
    with pytest.raises(ValueError, match="shape"):
        env.set_pool_ps_cores(np.ones((12, 4)))
    with pytest.raises(ValueError, match="integers"):
        env.set_pool_ps_cores([1.5, 1, 1, 1])
    with pytest.raises(lbffi.LbsimError) as e:
        h.set_pool_ps_cores(torch.ones((3, 4), dtype=torch.int32, device="cuda:0"), rows=3)
    assert e.value.code == lbffi.ESHAPE
    assert env.get_pool_ps_cores().cpu().tolist() == [[1, 2, 3, 64]] * 4
    assert L.lbsim_pool_ps_state_cols() == 5
    env.close()
    # FIFO pools, plain PS and plain handles: the new calls name lbsim_server_pool_enable_ps
    fifo, ps, plain = mk(balancers_per_pool=3), mk(service_discipline="ps"), mk()
    for e_ in (fifo, ps, plain):
        e_.reset()
        hh = e_.handle
        assert hh.server_pool_discipline() == 0
        for fn in (lambda: hh.set_pool_ps_cores(c4, rows=1), lambda: hh.pool_ps_cores(4),
                   hh.clear_pool_ps_cores,
                   lambda: hh.pool_ps_state(torch.zeros((12, 4, 5), device="cuda:0"))):
            with pytest.raises(lbffi.LbsimError, match="lbsim_server_pool_enable_ps") as e:
                fn()
            assert e.value.code == lbffi.ENOTSUP
        for name in ("set_pool_ps_cores", "get_pool_ps_cores", "clear_pool_ps_cores",
                     "pool_ps_state"):
            with pytest.raises(lbffi.LbsimError, match="lbsim_server_pool_enable_ps"):
                getattr(e_, name)(*([[1] * 4] if name == "set_pool_ps_cores" else []))
    with pytest.raises(ValueError, match="FIFO"):
        fifo.handle.enable_server_pool_ps(3)
    with pytest.raises(lbffi.LbsimError, match="server pools") as e:  # PS, then pools: refused
        ps.handle.enable_server_pool_ps(3)
    assert e.value.code == lbffi.ENOTSUP
    with pytest.raises(ValueError, match="first"):
        plain.handle.enable_server_pool_ps(3)
    assert fifo.ground_truth().shape == (12, 4, 8)
    with pytest.raises(lbffi.LbsimError) as e:
        ps.ground_truth()
    assert e.value.code == lbffi.ENOTSUP and "lbsim_pool_ps_state" not in str(e.value)
    for e_ in (fifo, ps, plain):
        e_.close()
    # what lbsim_server_pool_enable refuses, lbsim_server_pool_enable_ps refuses with its words
    late = mk(flow_stats=True)
    with pytest.raises(lbffi.LbsimError, match="flow statistics") as e:
        late.handle.enable_server_pool_ps(2)
    assert e.value.code == lbffi.ENOTSUP and late.handle.server_pool_size() == 0
    for bad in (0, 9, 5):
        with pytest.raises(ValueError):
            late.handle.enable_server_pool_ps(bad)
    late.close()


# ------------------------------------------------------------------ theory on the device

# S = 1, three members with unequal rates summing to load 1 / 2 of the capacity c mu = 40.
TH_LAMS, TH_CAP, TH_POOLS, TH_REC = (10.0, 6.0, 4.0), 40.0, 2048, 600


class TheoryRun:
    pass


def theory_run(seed, c, ps=True):
    """Burn in, then TH_REC steps.  Algorithm R keeps every flow a (member, server) completed since
    the reset with the same probability, by draws that do not depend on the flow, so the records
    stamped after the burn-in are a uniform sample of the flows completed after it: their mean
    estimates the stationary mean sojourn time.  Column 0 is summed at the recorded step ends."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    A, C = len(TH_LAMS), TH_POOLS
    B = C * A
    lam = sum(TH_LAMS)
    kw = dict(pool_discipline="ps", pool_ps_cores=[c]) if ps else {}
    env = VecLoadBalanceEnv(B, 1, device="cuda:0", autoreset=False, seed=seed, warmup_steps=0,
                            queue_capacity=qt.Q, step_interval=qt.DT, action_type="continuous",
                            max_steps=1 << 30, arrival_rate=lam / A, server_rates=[TH_CAP / c],
                            balancers_per_pool=A, **kw)
    env.set_rates(arrival_rate=np.tile(np.array(TH_LAMS, np.float32), C))
    env.reset()
    a = torch.ones((B, 1), dtype=torch.float32, device="cuda:0")
    burn = qt.burn_steps(qt.relaxation(TH_CAP, lam))
    for _ in range(burn):
        env.step(a)
    in_flight = torch.zeros(B, dtype=torch.float64, device="cuda:0")
    for _ in range(TH_REC):
        obs, _, _, _ = env.step(a)
        in_flight += obs[:, 0, 0].to(torch.float64)
    d = tsp.pool_state(env)
    r = TheoryRun()
    assert int(d["dropped"].sum()) == 0
    fct = d["res_fct"].reshape(B, K).astype(np.float64) * 1e-6
    ts = d["res_ts"].reshape(B, K).astype(np.int64)
    cnt = d["res_count"].reshape(B).astype(np.int64)
    assert cnt.min() > K  # every reservoir is full: all 128 slots hold records
    keep = ts >= int(burn * qt.DT * 1000)
    r.sum_s = (fct * keep).sum(1).reshape(C, A)
    r.count = keep.sum(1).astype(np.float64).reshape(C, A)
    r.n_mean = (in_flight.cpu().numpy() / TH_REC).reshape(C, A)
    env.close()
    return r


def theory_checks(r, c, name):
    w = tc_.mmc_ps(c, TH_CAP / c, sum(TH_LAMS))
    out = []
    for a, lam in enumerate(TH_LAMS):
        out.append(qt.Check(f"{name} member {a} mean sojourn time",
                            *qt.ratio(r.sum_s[:, a], r.count[:, a]), w))
        out.append(qt.Check(f"{name} member {a} Little: mean column 0 against lambda_a W",
                            r.n_mean[:, a].mean(),
                            r.n_mean[:, a].std(ddof=1) / math.sqrt(len(r.n_mean)),
                            lambda k, lam=lam: lam * w(k)))
    return out


@pytest.fixture(scope="module")
def theory_runs(lib):
    return {"ps-1": theory_run(9501, 1), "ps-2": theory_run(9502, 2),
            "fifo-1": theory_run(9503, 1, ps=False)}


def test_theory_formulas_restated():
    assert tc_.mmc_ps(1, 40.0, 20.0)(1.0) == pytest.approx(1.0 / (40.0 - 20.0))
    assert tc_.mmc_ps(2, 20.0, 20.0)(1.0) == pytest.approx(1.0 / 20.0 + (1.0 / 3.0) / 20.0)


@gpu
@pytest.mark.parametrize("key", ["ps-1", "ps-2", "fifo-1"])
def test_theory_per_member(theory_runs, key):
    """c = 1: every member's mean FCT is 1 / (mu - sum lambda); c = 2: the M/M/c-PS value of
    §3.23; Little's law per member on column 0.  A FIFO pool passes the c = 1 checks too
    (exponential sizes give the same mean).  Every check fails with mu scaled by 1.03.

    The confidence rule is tests/test_queueing_theory.py's: |estimate - theory| <= 5 SE + 0.1 %
    and SE <= 0.5 % of the theory value."""
    c = int(key.split("-")[1])
    checks = theory_checks(theory_runs[key], c, f"pool {key}")
    qt.assert_checks(checks)
    for chk in checks:
        assert not chk.ok(1.03), f"does not discriminate: {chk}"
