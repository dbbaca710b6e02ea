"""Processor-sharing servers with several cores: per-(env, server) core counts on
a processor-sharing handle, and its privileged view of the servers.

The reference is tests/ps_cores_ref.PSCoresSim, tests/ps_ref.PSSim with §3.23 added from its text.
The scenario and the cases are tests/test_processor_sharing.py's (reset, 6 steps, a masked reset of
every third env, 6 steps; S in {1, 2, 3, 4, 8, 16}, Q in {8, 64}, the four score policies) with
cores_of's counts: rows cycling 1, 2, 3, 4 by env, env 4 mixed, one server of env 5 with 64 cores,
each server's rate divided by its count where that is at most 4.

Not gpu: all counts 1 against PSSim and 64 cores against fct == svc on every case of
test_flowsim_ref.CASES; the scenario against an exact c-core server in fractions (largest
difference printed; the ledger and V == tag_head are asserted inside the reference at every
event); what the scenario reaches; a mid-run change; the c-core functions of csrc/lbsim_ps.h as
host C++ under the sanitizers and replayed through the reference; the privileged view's
definitions; check_ps_config; M/M/c-PS theory on the reference.
gpu: handles with cores against the reference exactly, after every reset and step, the
compositions, the refusals, and theory at 4096 envs.
"""
import copy
import math
import os
import subprocess

import numpy as np
import pytest

from marllb_amd import _lib, build
from marllb_amd.env import make_config
from marllb_amd.ps import check_ps_config
from tests import parity, ps_ref, statelayout
from tests import ps_cores_ref as pcr
from tests import test_flowsim_ref as fr
from tests import test_processor_sharing as tp
from tests import test_queueing_theory as qt
from tests.parity import lib  # noqa: F401  (the fixture: fails a gpu test run without a device)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
gpu = pytest.mark.gpu
STEPS, RESET_AT = tp.STEPS, tp.RESET_AT
CASES, DEEP, FAST = tp.CASES, tp.DEEP, tp.FAST
HOST_B, GPU_B = 8, fr.GPU_B
MIXED = (2, 3, 1, 4)


def cores_of(B, S):
    """(B, S) counts: rows cycle 1, 2, 3, 4 by env; env 4 is mixed; env 5's last server has 64."""
    c = np.repeat(1 + np.arange(B)[:, None] % 4, S, axis=1).astype(np.int32)
    if B > 4:
        c[4] = [MIXED[s % 4] for s in range(S)]
    if B > 5:
        c[5, S - 1] = 64
    return c


def rates_of(case, B, cores):
    """(B, S) f32 server rates: the case's, each divided by the server's count where it is <= 4
    (equal capacity); a 64-core server keeps its core's rate."""
    S, kw = tp.config_kwargs(case)
    cfg = make_config(B, S, **kw)
    base = np.array([cfg.server_rate[s] for s in range(S)], np.float64)
    return (base[None, :] / np.where(cores <= 4, cores, 1)).astype(np.float32)


def make_sims(case, B, cores, mus, lams=None, tables=None, offset=0):
    S, kw = tp.config_kwargs(case)
    cfg = make_config(B, S, **kw)
    return [pcr.PSCoresSim(kw["seed"], cfg.env_id_offset + offset + b, S, cfg.queue_capacity,
                           kw.get("assign_policy", "sed"),
                           cfg.arrival_rate if lams is None else float(lams[b]),
                           [float(x) for x in mus[b]], dt=cfg.step_interval,
                           warmup_steps=cfg.warmup_steps, cores=cores[b],
                           arrivals=None if tables is None else tables[b])
            for b in range(B)]


def snapshot(sims, drops, **kw):
    ev = tp.snapshot(sims, drops, **kw)
    ev.state = np.array([[m.state_row(s) for s in range(m.S)] for m in sims], np.float32)
    return ev


_RUNS = {}


def reference_run(case, B, steps=STEPS, cores=None, mus=None, change=None, schedule=None,
                  key=None, **sim_kw):
    """The scenario on B PSCoresSim envs -> (acts, snapshots, sims), once per key.  cores / mus:
    default cores_of / rates_of.  change = (k, counts): set_cores(counts) before step k.
    schedule: as tests.test_processor_sharing.reference_run's."""
    S, kw = tp.config_kwargs(case)
    cores = cores_of(B, S) if cores is None else cores
    mus = rates_of(case, B, cores) if mus is None else mus
    if key is not None and (case, B, steps, key) in _RUNS:
        return _RUNS[(case, B, steps, key)]
    sims = make_sims(case, B, cores, mus, **sim_kw)
    drops, ep_step = np.zeros(B, np.int64), np.zeros(B, np.int64)
    acts = tp.actions_of(case, B, steps)
    snaps = []

    def phase(b, j):
        if schedule is not None:
            sims[b].set_rates(float(schedule[0][b, j]), [float(x) for x in schedule[1][b, j]])

    def reset(mask):
        for b in np.flatnonzero(mask):
            phase(b, 0)
            drops[b] = sum(r.dropped for r in sims[b].reset())
            ep_step[b] = 0
        snaps.append(snapshot(sims, drops, mask=mask))

    reset(np.ones(B, bool))
    for k in range(steps):
        if k == RESET_AT:
            reset(np.arange(B) % 3 == 0)
        if change is not None and k == change[0]:
            for b in range(B):
                sims[b].set_cores(change[1][b])
        if schedule is not None:
            for b in range(B):
                phase(b, tp.schedule_phase(int(ep_step[b]), schedule))
        ep_step += 1
        wts = fr.weights_of(acts[k], kw)
        rs = [sims[b].step(wts[b]) for b in range(B)]
        drops += np.array([r.dropped for r in rs])
        snaps.append(snapshot(sims, drops, assigned=np.array([r.assigned for r in rs]),
                              new=[[r.fct(s) for s in range(S)] for r in rs]))
    out = (acts, snaps, sims)
    if key is not None:
        _RUNS[(case, B, steps, key)] = out
    return out


# ------------------------------------------------------------------ not gpu: the two identities

def host_sims(case, policy, cls, **extra):
    S, kw = tp.ps_case_of(case, policy)
    cfg = make_config(tp.HOST_B, S, **kw)
    return S, kw, [cls(kw["seed"], cfg.env_id_offset + b, S, cfg.queue_capacity, policy,
                       cfg.arrival_rate, [cfg.server_rate[s] for s in range(S)],
                       dt=cfg.step_interval, warmup_steps=0, **extra) for b in range(tp.HOST_B)]


@pytest.mark.parametrize("policy", tp.SCORE_POLICIES)
@pytest.mark.parametrize("case", list(fr.CASES))
def test_one_core_is_pssim_and_64_cores_is_an_infinite_server(case, policy):
    """All counts 1: PSCoresSim equals PSSim event for event (completions, assignments, drops,
    queues, carries).  All counts 64 >= Q: every flow's fct is its svc exactly."""
    S, kw, plain = host_sims(case, policy, ps_ref.PSSim)
    _, _, ones = host_sims(case, policy, pcr.PSCoresSim, cores=[1] * S)
    _, _, wide = host_sims(case, policy, pcr.PSCoresSim, cores=[64] * S)
    acts = fr.actions_of(case, tp.HOST_B)
    flows = 0
    for b in range(tp.HOST_B):
        p, o, w = plain[b], ones[b], wide[b]
        assert w.Q <= 64
        for m in (p, o, w):
            m.reset()
        want, got = [], []
        for k in range(STEPS):
            wt = fr.weights_of(acts[k], kw)[b]
            rp, ro, rw = p.step(wt), o.step(wt), w.step(wt)
            assert rp.completed == ro.completed and rp.dropped == ro.dropped, (b, k)
            np.testing.assert_array_equal(rp.assigned, ro.assigned)
            assert p.queues == o.queues and p.acc == o.acc and p.V == o.V
            want += [(s, ta, ta + svc) for s, ta, svc, _ in w.assigned_log]
            got += rw.completed
            assert all(a == 0 for a in w.acc)
        end = STEPS * w.dt
        assert sorted(got) == sorted(x for x in want if x[2] <= end), ("fct == svc", b)
        flows += len(got)
    assert flows > 10 * tp.HOST_B


# ------------------------------------------------------------------ not gpu: the scenario

def host_run(case):
    return reference_run(case, HOST_B, key="host")


@pytest.mark.parametrize("case", list(CASES))
def test_scenario_against_exact_c_core_processor_sharing(case):
    """Each server's assigned (ta, svc) fed to ExactCoresPS, exact c-core processor sharing in
    fractions; the largest completion-time difference is printed (DESIGN.md §3.23 records it).

    No bound on it is asserted: §3.22's 2 k n_max argument needs the unfinished work of the two to
    agree at every arrival, and with c > 1 it does not (the service rate min(n, c) depends on n, so
    a completion that differs by a us changes the rate for that us, and the rule drops a carry of
    less than c core-us at each fall to n <= c).  What is exact is asserted, inside PSCoresSim, at
    every event of this run: V == tag_head at each completion with 0 <= acc < c, the completion at
    the smallest such us, and the ledger (sum(tag - V) - acc falls by min(n, c) d, plus the dropped
    carry).  Here: one-core servers still end their busy periods at the exact us (§3.22), and
    servers with c >= Q complete every flow at the exact time."""
    S, kw = tp.config_kwargs(case)
    B = HOST_B
    cores = cores_of(B, S)
    mus = rates_of(case, B, cores)
    sims = make_sims(case, B, cores, mus)
    acts = tp.actions_of(case, B)
    worst = {}
    exact_checked = 0
    for b, sim in enumerate(sims):
        sim.warmup_steps = 0
        sim.reset()
        exact = [pcr.ExactCoresPS(cores[b, s]) for s in range(S)]
        completions = []
        for k in range(STEPS):
            sim.step(fr.weights_of(acts[k], kw)[b])
            for s, ta, svc, _ in sim.assigned_log:
                exact[s].arrive(ta, svc)
            completions.extend(sim.completion_log)
        by_ta = []
        for s in range(S):
            exact[s].finish()
            d = {}
            for ta, tc in exact[s].done:
                d.setdefault(ta, []).append(tc)
            by_ta.append(d)
        for s, ta, tc, _, ends_busy in completions:
            c = int(cores[b, s])
            cand = by_ta[s][ta]
            e = min(cand, key=lambda x: abs(x - tc))
            cand.remove(e)
            if c >= sim.Q or (c == 1 and ends_busy):
                assert tc == e, ("exact completion", b, s, ta, tc, e)
                exact_checked += 1
            worst[c] = max(worst.get(c, 0), abs(tc - e))
    assert exact_checked > 0
    print(f"PS-CORES-EXACT {case}: largest |tc - exact| by c = "
          + ", ".join(f"{c}: {float(v):.3f} us" for c, v in sorted(worst.items())))


REACHES = ("acc_left", "rem_dropped", "zero_delta", "found_n_eq_c", "carried_n_gt_c",
           "full_drops_multicore")


def test_scenario_reaches():
    """The scenario meets what the rule adds: a completion leaving acc > 0, a carry dropped at a
    fall to n <= c, a completion at t_last with n > c (equal tags), an arrival finding n == c, a
    carry across a step boundary with n > c, and a drop with every queue full on a multi-core
    env."""
    total = {}
    for case in CASES:
        _, snaps, sims = host_run(case)
        r = tp.reach_of(sims)
        print(f"REACH {case}: {r}")
        for k, v in r.items():
            total[k] = total.get(k, 0) + v
    for k in REACHES + ("equal_tags", "at_head", "at_ta", "at_dt", "same_us"):
        assert total[k] > 0, k
    multi = sum(m.reach["full_drops_multicore"] for case in CASES
                for m in host_run(case)[2] if max(m.cores) > 1)
    assert multi > 0


def test_mid_run_change_on_the_reference():
    """set_cores from the next step on, in both directions (c -> 5 - c): entries keep their
    remaining tags, and the run differs from the unchanged one only from that step on."""
    S, _ = tp.config_kwargs(DEEP)
    cores = cores_of(HOST_B, S)
    mus = rates_of(DEEP, HOST_B, cores)
    new = np.where(cores <= 4, 5 - cores, cores)
    _, base, _ = reference_run(DEEP, HOST_B, cores=cores, mus=mus)
    _, snaps, sims = reference_run(DEEP, HOST_B, cores=cores, mus=mus, change=(3, new))
    for k, (a, b) in enumerate(zip(base, snaps)):
        same = a.rings == b.rings and (a.acc == b.acc).all()
        assert same or k > 3, k  # snapshots 0..3: the reset and steps 0..2
    assert snaps[-1].rings != base[-1].rings
    assert all(m.cores == list(new[b]) and m.cores_changed for b, m in enumerate(sims))
    # the step before the change left entries behind on servers that gained and that lost cores
    n3 = base[3].in_flight
    assert ((n3 > 0) & (new > cores)).any() and ((n3 > 0) & (new < cores)).any()


def test_server_state_definitions():
    """The privileged view on the reference: a copy run forward with no arrivals completes its
    last flow at now + drain; the work is the sum of the remaining tags less the carry where
    n > c; one-core servers have work == drain; c >= n servers drain in their largest tag."""
    seen = {"n_gt_c": 0, "one": 0, "wide": 0}
    for case in (DEEP, FAST, "s1-sed-q8-drops"):
        _, _, sims = host_run(case)
        for m in sims:
            now = m.step_no * m.dt
            fwd = copy.deepcopy(m)
            done = []
            fwd._pop_due(1 << 60, done)
            for s in range(m.S):
                n, busy, work, drain = m.server_state(s)
                rem = [r for r, _ in m.remaining(s)]
                c = m.cores[s]
                assert n == len(rem) and busy == min(n, c)
                assert work == sum(rem) - (m.acc[s] if n > c else 0)
                last = max([tc for sv, _, tc in done if sv == s], default=now)
                assert last - now == drain, (case, s, last - now, drain)
                if c == 1:
                    assert work == drain
                    seen["one"] += n > 1
                if n and c >= n:
                    assert drain == max(rem)
                    seen["wide"] += 1
                seen["n_gt_c"] += n > c > 1
                row = m.state_row(s)
                assert row[2] == np.float32(work) * np.float32(1e-6)
    assert min(seen.values()) > 0, seen


# ------------------------------------------------------------------ not gpu: the helpers

def test_helpers_against_a_naive_model(tmp_path):
    """tests/ps_cores_probe.cpp: the c-core advance, next completion, completion shortcut and
    ps_server_state of csrc/lbsim_ps.h for every c in 1..64 and Q in {3, 8, 9, 32, 64} against the
    rule in 64 bits, under the address and undefined-behaviour sanitizers; then the probe's
    operations replayed through PSCoresSim."""
    exe = str(tmp_path / "ps_cores_probe")
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "ps_cores_probe.cpp")], check=True)
    r = subprocess.run([exe, "1"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
    assert [(row[0], row[1]) for row in rows] == [(c, q) for c in range(1, 65)
                                                  for q in (3, 8, 9, 32, 64)]
    tot = np.zeros(7, np.int64)
    shared = {c: np.zeros(7, np.int64) for c in range(2, 64)}
    for c, q, *counts in rows:
        inserts, completions, acc_left, rem_dropped, zero_delta, n_eq_c, carried = counts
        assert inserts > 100 and completions > 100, (c, q)
        if 1 < c < q:  # the cores are shared at times
            shared[c] += counts
        if c == 1 or c >= q:
            assert acc_left == 0 and rem_dropped == 0, (c, q)
        tot += counts
    assert tot.min() > 0, tot
    for c, t in shared.items():  # every c below 64 shared its cores and fell back to n <= c
        acc_left, rem_dropped, n_eq_c = t[2], t[3], t[5]
        assert min(acc_left, rem_dropped) > 0 and n_eq_c > 1, (c, t)
    r = subprocess.run([exe, "1", "trace"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    seen = replay_probe_trace(r.stdout.splitlines())
    assert seen["Q"] == [(q, c) for c in (1, 2, 3, 5, 8, 64) for q in (3, 8, 9, 32, 64)]
    assert min(seen[k] for k in ("A", "C", "D", "E")) > 100, seen


def replay_probe_trace(lines, dt=50000):
    """Every operation csrc/lbsim_ps.h did in ps_cores_probe, done again by PSCoresSim's own
    methods: the completions it pops before each operation are the probe's (times and order), an
    insert lands at the probe's position, and at a step end the carry, the entries {remaining,
    ta}, the work and the drain are the probe's."""
    seen = {"Q": [], "A": 0, "C": 0, "D": 0, "E": 0}
    sim, base, pending = None, 0, []

    def pops(t, at_arrival=True):
        done = []
        sim._pop_due(t, done, at_arrival)
        assert [(tc - base, ta - base) for _, ta, tc in done] == pending, (done, pending, base)
        seen["C"] += len(pending)
        pending.clear()

    for line in lines:
        op, *v = line.split()
        v = [int(x) for x in v]
        if op == "Q":
            assert not pending
            sim = pcr.PSCoresSim(7600, 0, 1, v[0], "lsq", 10.0, [10.0], dt=dt * 1e-6,
                                 warmup_steps=0, cores=[v[1]])
            sim.reset()
            base = 0
            seen["Q"].append((v[0], v[1]))
        elif op == "C":
            pending.append((v[0], v[1]))
        elif op == "A":
            pops(base + v[0])
            sim._insert(0, base + v[0], v[1])
            tag = sim.V[0] + v[1]
            assert sim.queues[0][v[2]] == (tag, base + v[0]), ("position", line)
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
            want = [(v[4 + 2 * i], v[5 + 2 * i]) for i in range(v[1])]
            assert [(rem, ta - base) for rem, ta in sim.remaining(0)] == want, line
            seen["E"] += 1
    return seen


def test_check_ps_config_and_the_interface():
    """check_ps_config(ps_cores=True) passes where the config passes and refuses what it refused;
    the header declares the entry points, the ABI version stays, ctypes knows them."""
    from marllb_amd import trace
    ok = make_config(8, 4, assign_policy="lsq2", arrival_rate=50.0)
    check_ps_config(ok, ps_cores=True)
    check_ps_config(ok, ps_cores=False)
    for cfg_kw, opts in ((dict(assign_policy="alias"), {}), (dict(fail_prob=0.1), {}),
                         (dict(trace=trace.synthetic(37, 300.0, seed=7)), {}),
                         ({}, dict(server_workers=True)), ({}, dict(balancers_per_pool=2))):
        for pc in (False, True):
            with pytest.raises(_lib.LbsimError) as e:
                check_ps_config(make_config(8, 4, **cfg_kw), ps_cores=pc, **opts)
            assert e.value.code == _lib.ENOTSUP
    header = open(os.path.join(ROOT, "include", "lbsim.h")).read()
    for name, nargs in (("lbsim_set_ps_cores", 4), ("lbsim_get_ps_cores", 3),
                        ("lbsim_clear_ps_cores", 2), ("lbsim_ps_server_state", 3)):
        assert f"int {name}(" in header and len(_lib._SIGNATURES[name][1]) == nargs
    assert "#define LBSIM_ABI_VERSION 10 " in header and "#define LBSIM_PS_STATE_COLS 4" in header
    import marllb_amd
    assert marllb_amd.PS_STATE_COLUMNS == ("n", "busy_cores", "work_s", "drain_s")


# ------------------------------------------------------------------ theory, on the reference

# the arrival rate and the capacity c mu of every server: load 1 / 2, as test_processor_sharing's,
# at rates where one of two cores (24 flows/s) still keeps §3.15's bound on the largest service
# time under the Pareto sizes (344.2 x 1e6 / mu x 64 <= 2^30 needs mu >= 20.6).  More flows per
# step than at (40, 20): the recorded steps sized there (tp.TH_REC) give a smaller SE here, and
# test_theory_sizes_on_the_reference checks it.
TH_LAM, TH_CAP = 24.0, 48.0


def erlang_c(c, a):
    """The probability that an arrival of M/M/c with offered load a = lambda / mu < c waits."""
    top = a ** c / math.factorial(c) * c / (c - a)
    return top / (sum(a ** k / math.factorial(k) for k in range(c)) + top)


def mmc_ps(c, mu, lam):
    """The mean sojourn time of M/M/c-PS (each of n flows served at rate min(1, c / n) mu): the
    number in system is M/M/c's birth-death chain, so by Little's law it is M/M/c's,
    1 / mu + C(c, lambda / mu) / (c mu - lambda); theory(k): with mu scaled by k."""
    return lambda k: 1.0 / (k * mu) + erlang_c(c, lam / (k * mu)) / (c * k * mu - lam)


def test_erlang_c_restated():
    assert erlang_c(1, 0.5) == pytest.approx(0.5)  # M/M/1: rho
    assert mmc_ps(1, 40.0, 20.0)(1.0) == pytest.approx(qt.mm1(40.0, 20.0)(1.0))
    assert erlang_c(2, 1.0) == pytest.approx(1.0 / 3.0)  # 2 rho^2 / (1 + rho) at rho = 1 / 2
    # the chain itself: p_n of M/M/c summed directly
    for c, a in ((2, 1.0), (4, 2.0), (3, 2.5)):
        p = [a ** n / math.factorial(n) if n <= c else
             a ** c / math.factorial(c) * (a / c) ** (n - c) for n in range(4000)]
        assert sum(p[c:]) / sum(p) == pytest.approx(erlang_c(c, a), rel=1e-9)
        mean_n = sum(n * x for n, x in enumerate(p)) / sum(p)
        assert mean_n == pytest.approx(a * mmc_ps(c, 1.0, a)(1.0), rel=1e-9)


@pytest.mark.parametrize("c,sizes", [(2, "exp"), (4, "exp"), (2, "pareto")])
def test_theory_sizes_on_the_reference(c, sizes):
    """The reference alone, at reduced size, meets the M/M/c-PS mean whatever the size
    distribution, and 1 / sqrt(n) scaling of its SE puts the device run under the cap."""
    envs, rec = 48, 40
    tabs = tp.pareto_tables() if sizes == "pareto" else None
    count, sum_us = np.zeros(envs), np.zeros(envs)
    for b in range(envs):
        sim = pcr.PSCoresSim(9420 + c, b, 1, qt.Q, "sed", TH_LAM, [TH_CAP / c], dt=qt.DT,
                             warmup_steps=0, arrivals=tabs, cores=[c])
        sim.reset()
        for _ in range(tp.th_burn()):
            sim.step([1.0])
        for _ in range(rec):
            for _, ta, tc in sim.step([1.0]).completed:
                count[b] += 1
                sum_us[b] += tc - ta
    est, se = qt.ratio(sum_us * 1e-6, count)
    chk = qt.Check(f"reference M/G/{c}-PS mean ({sizes})", est, se, mmc_ps(c, TH_CAP / c, TH_LAM))
    scaled = se * math.sqrt(envs * rec / (qt.B * tp.TH_REC[sizes]))
    print(chk, f"-> device SE {100 * scaled / chk.theory(1.0):.3f} %")
    assert chk.ok()
    assert scaled <= qt.CAP * chk.theory(1.0)


# ------------------------------------------------------------------ the device

class CoresCheck(tp.PSCheck):
    """PSCheck, and ps_state() against the reference's four columns, exact."""

    def __call__(self, ev, out):
        super().__call__(ev, out)
        got = self.env.ps_state().cpu().numpy()
        np.testing.assert_array_equal(got, ev.state, err_msg="ps_state")
        self.compared["state"] = self.compared.get("state", 0) + int((ev.state[:, :, 0] > 0).sum())


def backend(case, B, cores, mus, **extra):
    S, kw = tp.config_kwargs(case)
    return tp.DeviceBackend(B, S, kw, mus=mus, ps_cores=cores, **extra)


def drive(back, check, run, B, steps=STEPS, change=None):
    acts, snaps, sims = run
    it = iter(snaps)
    check(next(it), back.reset(None))
    for k in range(steps):
        if k == RESET_AT:
            check(next(it), back.reset((np.arange(B) % 3 == 0).astype(np.uint8)))
        if change is not None and k == change[0]:
            back.env.set_ps_cores(change[1])
        check(next(it), back.step(acts[k]))
    return snaps, sims


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_handles_with_cores_equal_the_reference(lib, case):
    """After every reset and step: everything test_processor_sharing's PSCheck compares (the
    counters, hc, res_count, every record and timestamp, the live ring entries in order, last_tc
    == acc, columns 1-10, the reward) and ps_state()'s four columns, all exact."""
    S, _ = tp.config_kwargs(case)
    cores = cores_of(GPU_B, S)
    mus = rates_of(case, GPU_B, cores)
    back = backend(case, GPU_B, cores, mus)
    np.testing.assert_array_equal(back.env.get_ps_cores().cpu().numpy(), cores)
    chk = CoresCheck(back.env)
    snaps, sims = drive(back, chk, reference_run(case, GPU_B, key="gpu"), GPU_B)
    tp.check_ps_kernel(lib, back.env)
    assert chk.compared["entries"] > GPU_B and chk.compared["records"] > 10 * GPU_B
    assert chk.compared["state"] > GPU_B
    r = tp.reach_of(sims)
    assert r["found_n_eq_c"] > 0 and r["all_own_core"] > 0
    if case == FAST:
        assert min(r[k] for k in ("acc_left", "rem_dropped", "zero_delta", "carried_n_gt_c")) > 0
        assert chk.compared["acc"] > 0
    back.env.close()


@gpu
def test_forced_four_lane_groups():
    """LBSIM_DYN_GROUP_LANES=4: the 4-lane groups on every case of at most 4 servers."""
    ks = [f"test_handles_with_cores_equal_the_reference[{c}]" for c, v in CASES.items()
          if v[0] <= 4]
    assert len(ks) >= 5
    parity.run_cases_in_child("test_ps_cores.py", ks, {"LBSIM_DYN_GROUP_LANES": "4"})


@gpu
def test_all_ones_is_a_handle_that_never_set_cores(lib):
    """Every count 1 -- set, or cleared after other counts were in force for a reset that is then
    repeated -- against a handle that never set cores: outputs and state bytes, bit for bit, and
    the same kernel names."""
    for case in (DEEP, FAST, "s16-lsq-q64"):
        S, kw = tp.config_kwargs(case)
        B = 24
        never = tp.DeviceBackend(B, S, kw)
        ones = tp.DeviceBackend(B, S, kw, ps_cores=np.ones((B, S), np.int32))
        cleared = tp.DeviceBackend(B, S, kw, ps_cores=[3] * S)
        cleared.env.clear_ps_cores()
        acts = tp.actions_of(case, B)
        outs = [e.reset(None) for e in (never, ones, cleared)]
        for k in range(STEPS):
            for o in outs[1:]:
                np.testing.assert_array_equal(o[0], outs[0][0])
            outs = [e.step(acts[k]) for e in (never, ones, cleared)]
            for o in outs[1:]:
                for x, y in zip(o, outs[0]):
                    np.testing.assert_array_equal(x, y)
        ref = never.env.handle.state_bytes()
        names = lib.launch_names(never.env.handle)
        for e in (ones, cleared):
            assert e.env.handle.state_bytes() == ref
            assert lib.launch_names(e.env.handle) == names
            assert bool((e.env.get_ps_cores() == 1).all())
        assert bool((never.env.get_ps_cores() == 1).all())
        # one-core servers: the drain is the work
        st = never.env.ps_state().cpu().numpy()
        np.testing.assert_array_equal(st[:, :, 2], st[:, :, 3])
        np.testing.assert_array_equal(st, ones.env.ps_state().cpu().numpy())
        assert st[:, :, 0].max() > 1
        for e in (never, ones, cleared):
            e.env.close()


@gpu
def test_past_128_samples(lib):
    """Every reservoir past 128 samples, on shared cores."""
    steps, B = 40, 24
    S, _ = tp.config_kwargs(FAST)
    cores = cores_of(B, S)
    mus = rates_of(FAST, B, cores)
    back = backend(FAST, B, cores, mus)
    snaps, _ = drive(back, CoresCheck(back.env), reference_run(FAST, B, steps), B, steps)
    assert int(snaps[-1].res_count.min()) > tp.K + 20
    back.env.close()


@gpu
def test_per_env_rates_and_flow_statistics(lib):
    B = 24
    S, _ = tp.config_kwargs(DEEP)
    rng = np.random.default_rng(15)
    cores = cores_of(B, S)
    lams = rng.uniform(100.0, 220.0, B).astype(np.float32)
    mus = (rng.uniform(25.0, 60.0, (B, S)) / np.minimum(cores, 4)).astype(np.float32)
    S, kw = tp.config_kwargs(DEEP)
    back = tp.DeviceBackend(B, S, kw, mus=mus, lams=lams, flow_stats=True, ps_cores=cores)
    chk = CoresCheck(back.env, stats=True)
    drive(back, chk, reference_run(DEEP, B, cores=cores, mus=mus, lams=lams), B)
    assert int(chk.fs[0].sum()) > 5 * B
    back.env.close()


@gpu
def test_workload_tables_with_a_heavy_tail(lib):
    """Workload tables: exponential gaps and, on every other env, bounded-Pareto sizes.  The
    servers keep the case's rates (a quarter of them would break §3.15's bound on the largest
    service time under these sizes), so a server of c cores has c times the capacity."""
    B = 24
    S, kw = tp.config_kwargs(DEEP)
    cores = cores_of(B, S)
    mus = rates_of(DEEP, B, np.ones_like(cores))
    bank = np.stack(tp.pareto_tables())
    work_id = (np.arange(B) % 2).astype(np.int32)
    tables = [(bank[0], bank[w]) for w in work_id]
    back = tp.DeviceBackend(B, S, kw, mus=mus, tables=(bank, 0, work_id), flow_stats=True,
                            ps_cores=cores)
    chk = CoresCheck(back.env, stats=True)
    _, sims = drive(back, chk, reference_run(DEEP, B, cores=cores, mus=mus, tables=tables), B)
    assert tp.reach_of(sims)["at_head"] > 0
    back.env.close()


@gpu
def test_rate_schedule(lib):
    """A P = 3, H = 2 cyclic rate schedule, per env, under cores."""
    B, P, H = 24, 3, 2
    S, kw = tp.config_kwargs(DEEP)
    cores = cores_of(B, S)
    rng = np.random.default_rng(16)
    lam = rng.uniform(90.0, 230.0, (B, P)).astype(np.float32)
    mu = (rng.uniform(25.0, 60.0, (B, P, S)) / np.minimum(cores, 4)[:, None, :]).astype(np.float32)
    back = tp.DeviceBackend(B, S, kw, flow_stats=True, ps_cores=cores)
    back.env.set_rate_schedule(lam, mu, steps_per_phase=H, wrap=True)
    chk = CoresCheck(back.env, stats=True)
    drive(back, chk, reference_run(DEEP, B, cores=cores, mus=mu[:, 0], schedule=(lam, mu, H, True)),
          B)
    back.env.close()


@gpu
def test_same_step_auto_reset(lib):
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    B, case = 12, "s4-sed2-q8-continuous"
    S, kw = tp.config_kwargs(case)
    cores = cores_of(B, S)
    mus = rates_of(case, B, cores)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", service_discipline="ps", ps_cores=cores,
                            max_steps=3, **kw)
    env.set_rates(None, mus)
    chk = CoresCheck(env)
    sims = make_sims(case, B, cores, mus)
    drops = np.array([sum(r.dropped for r in m.reset()) for m in sims], np.int64)
    obs = env.reset()
    chk(snapshot(sims, drops, mask=np.ones(B, bool)), (obs.cpu().numpy(), None, None))
    acts = tp.actions_of(case, B)
    for k in range(7):
        obs, rew, done, info = env.step(torch.from_numpy(acts[k]), assign_counts=True)
        wts = fr.weights_of(acts[k], kw)
        rs = [m.step(wts[b]) for b, m in enumerate(sims)]
        drops += np.array([r.dropped for r in rs])
        ends = k % 3 == 2
        assert bool(done.all()) == ends
        if ends:
            drops = np.array([sum(r.dropped for r in m.reset()) for m in sims], np.int64)
        chk(snapshot(sims, drops, assigned=np.array([r.assigned for r in rs])),
            (obs.cpu().numpy(), None if ends else rew.cpu().numpy(),
             info["assign_counts"].cpu().numpy()))
    assert chk.compared["entries"] > B
    env.close()


@gpu
def test_snapshot_restore_fork_and_state_round_trip(lib):
    """The layout is unchanged and the counts are no part of it: a snapshot restores byte for
    byte, a fork copies rings and carries, and a state set into a fresh handle with the same
    counts steps as the first."""
    import torch
    B = 24
    S, kw = tp.config_kwargs(DEEP)
    cores = cores_of(B, S)
    mus = rates_of(DEEP, B, cores)
    back = backend(DEEP, B, cores, mus)
    env = back.env
    plain = tp.DeviceBackend(B, S, kw)
    assert len(plain.env.handle.state_bytes()) == len(env.handle.state_bytes())
    plain.env.close()
    acts = tp.actions_of(DEEP, B)
    back.reset(None)
    for k in range(4):
        back.step(acts[k])
    snap = env.snapshot()
    before = env.handle.state_bytes()
    for k in range(4, 7):
        back.step(acts[k])
    env.restore(snap)
    assert env.handle.state_bytes() == before
    np.testing.assert_array_equal(env.get_ps_cores().cpu().numpy(), cores)
    d = statelayout.parse_cfg(before, env.cfg)
    src = int((d["hc"].reshape(B, S) >> 16).sum(1).argmax())
    env.restore(snap, src=torch.full((B,), src, dtype=torch.int32))
    f = statelayout.parse_cfg(env.handle.state_bytes(), env.cfg)
    for name in ("hc", "last_tc", "res_count"):
        rows = f[name].reshape(B, S)
        assert (rows == rows[src]).all(), name
    st = env.ps_state().cpu().numpy()
    assert (st[:, :, 0] == st[src, :, 0]).all()  # the same flows; busy cores by each env's counts
    np.testing.assert_array_equal(st[:, :, 1], np.minimum(st[:, :, 0], cores))
    env.restore(snap)
    third = backend(DEEP, B, cores, mus)
    third.reset(None)
    third.env.set_state(env.get_state())
    assert third.env.handle.state_bytes() == env.handle.state_bytes()
    for k in range(4, 6):
        for x, y in zip(back.step(acts[k]), third.step(acts[k])):
            np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(env.ps_state().cpu().numpy(), third.env.ps_state().cpu().numpy())
    for e in (third.env, env):
        e.close()


@gpu
def test_shards_at_uneven_sizes(lib):
    """Shards of 5, 12 and 7 envs, each passing its own rows of the counts and the rates."""
    B = 24
    S, kw = tp.config_kwargs(DEEP)
    cores = cores_of(B, S)
    mus = rates_of(DEEP, B, cores)
    whole = backend(DEEP, B, cores, mus)
    acts = tp.actions_of(DEEP, B)
    whole.reset(None)
    outs = [whole.step(acts[k]) for k in range(4)]
    dw = statelayout.parse_cfg(whole.env.handle.state_bytes(), whole.env.cfg)
    sw = whole.env.ps_state().cpu().numpy()
    lo = 0
    for n in (5, 12, 7):
        part = tp.DeviceBackend(n, S, {**kw, "env_id_offset": lo}, mus=mus[lo:lo + n],
                                ps_cores=cores[lo:lo + n])
        part.reset(None)
        for k in range(4):
            for x, y in zip(part.step(acts[k][lo:lo + n]), outs[k]):
                np.testing.assert_array_equal(x, y[lo:lo + n])
        dp = statelayout.parse_cfg(part.env.handle.state_bytes(), part.env.cfg)
        for name in ("hc", "last_tc", "res_count"):
            np.testing.assert_array_equal(dp[name].reshape(n, S),
                                          dw[name].reshape(B, S)[lo:lo + n], err_msg=name)
        np.testing.assert_array_equal(part.env.ps_state().cpu().numpy(), sw[lo:lo + n])
        part.env.close()
        lo += n
    whole.env.close()


@gpu
def test_replayed_graph_across_a_rewrite_of_the_cores(lib):
    """A captured step (with ps_state) replayed equals an eager twin step for step, and a
    set_ps_cores between two replays, which rewrites the array in place, is seen by the next."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    B = 24
    S, kw = tp.config_kwargs(DEEP)
    cores = cores_of(B, S)
    new = np.where(cores <= 4, 5 - cores, cores)
    mk = dict(device="cuda:0", service_discipline="ps", ps_cores=cores, **kw)
    eager = VecLoadBalanceEnv(B, S, **mk)
    graph = VecLoadBalanceEnv(B, S, graph_mode=True, **mk)
    for e in (eager, graph):
        e.reset()
    acts = [torch.from_numpy(a).to("cuda:0") for a in tp.actions_of(DEEP, B)[:7]]
    a_static = acts[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up step (eager, graph_mode buffers)
        graph.step(a_static)
        graph.ps_state()
    torch.cuda.current_stream().wait_stream(side)
    eager.step(acts[0])
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):  # the capture records the step, it does not run it
        obs, rew, done, info = graph.step(a_static)
        st = graph.ps_state()
    for k in range(1, 7):
        if k == 4:
            for e in (eager, graph):
                e.set_ps_cores(new)
        a_static.copy_(acts[k])
        cg.replay()
        eo, er, ed, _ = eager.step(acts[k])
        assert torch.equal(obs, eo) and torch.equal(rew, er) and torch.equal(done, ed), k
        assert torch.equal(st, eager.ps_state()), k
    assert graph.handle.state_bytes() == eager.handle.state_bytes()
    # the rewrite mattered: a twin that kept the old counts has parted from them
    keep = VecLoadBalanceEnv(B, S, **mk)
    keep.reset()
    for k in range(7):
        keep.step(acts[k])
    assert keep.handle.state_bytes() != eager.handle.state_bytes()
    for e in (eager, graph, keep):
        e.close()


@gpu
def test_mid_run_change(lib):
    """set_ps_cores between two steps, c -> 5 - c: from the next launch on, against the
    reference's set_cores."""
    B = 24
    S, _ = tp.config_kwargs(DEEP)
    cores = cores_of(B, S)
    mus = rates_of(DEEP, B, cores)
    new = np.where(cores <= 4, 5 - cores, cores)
    back = backend(DEEP, B, cores, mus)
    chk = CoresCheck(back.env)
    drive(back, chk, reference_run(DEEP, B, cores=cores, mus=mus, change=(3, new)), B,
          change=(3, new))
    np.testing.assert_array_equal(back.env.get_ps_cores().cpu().numpy(), new)
    back.env.close()


@gpu
def test_facades_and_the_sampler(lib):
    import torch
    from marllb_amd import sample_server_workers
    from marllb_amd.env import LoadBalanceEnv, VecLoadBalanceEnv
    from marllb_amd.multi_agent import MultiAgentLoadBalanceEnv, VecMultiAgentLoadBalanceEnv
    one = LoadBalanceEnv(num_servers=4, service_discipline="ps", ps_cores=[1, 2, 3, 4], seed=3)
    assert one.get_ps_cores() == [1, 2, 3, 4]
    one.reset()
    one.step(np.zeros(4, np.int64))
    st = one.ps_state()
    assert st.shape == (4, 4) and st.dtype == np.float32
    assert (st[:, 1] == np.minimum(st[:, 0], [1, 2, 3, 4])).all()
    one.set_ps_cores([4, 3, 2, 1])
    assert one.get_ps_cores() == [4, 3, 2, 1]
    one.clear_ps_cores()
    assert one.get_ps_cores() == [1, 1, 1, 1]
    with pytest.raises(ValueError):
        one.set_ps_cores([1, 2])
    one.close()
    ma1 = MultiAgentLoadBalanceEnv(num_agents=2, servers_per_agent=2, service_discipline="ps",
                                   ps_cores=[2, 2, 1, 1])
    assert ma1.get_ps_cores() == [2, 2, 1, 1]
    ma1.reset()
    assert ma1.ps_state().shape == (4, 4)
    ma1.set_ps_cores([1, 1, 2, 2])
    ma1.clear_ps_cores()
    ma1.close()
    ma = VecMultiAgentLoadBalanceEnv(6, num_agents=2, servers_per_agent=2,
                                     service_discipline="ps", ps_cores=[1, 2, 3, 4])
    ma.reset()
    assert ma.get_ps_cores().cpu().tolist() == [[1, 2, 3, 4]] * 6
    assert tuple(ma.ps_state().shape) == (6, 4, 4)
    ma.set_ps_cores(np.full((6, 4), 2))
    ma.clear_ps_cores()
    assert bool((ma.get_ps_cores() == 1).all())
    ma.vec.close()
    # the sampler: counts and the rate of one core at equal capacity
    B, S = 16, 4
    counts, mu = sample_server_workers(B, S, (1, 2, 4), seed=5, keep_capacity=True,
                                       server_rates=80.0)
    vec = VecLoadBalanceEnv(B, S, device="cuda:0", service_discipline="ps")
    vec.set_ps_cores(counts)
    vec.set_rates(None, mu)
    assert torch.equal(vec.get_ps_cores().cpu(), counts.cpu())
    np.testing.assert_allclose((counts.double() * mu.double()).numpy(), 80.0, rtol=1e-6)
    vec.reset()
    vec.step(torch.zeros((B, S), dtype=torch.int64))
    st = vec.ps_state()
    assert bool((st[:, :, 1] == torch.minimum(st[:, :, 0], counts.to(st))).all())
    out = torch.empty((B, S, 4), dtype=torch.float32, device="cuda:0")
    assert vec.ps_state(out) is out and torch.equal(out, st)
    vec.close()


@gpu
def test_refusals(lib):
    """Every refusal, each leaving what was in force."""
    import torch
    from marllb_amd.env import Handle, VecLoadBalanceEnv
    L = lib.load()
    assert L.lbsim_set_ps_cores(None, None, 1, None) == _lib.EINVAL
    assert L.lbsim_get_ps_cores(None, None, None) == _lib.EINVAL
    assert L.lbsim_clear_ps_cores(None, None) == _lib.EINVAL
    assert L.lbsim_ps_server_state(None, None, None) == _lib.EINVAL
    assert L.lbsim_ps_server_state_cols() == 4
    # ps_cores without "ps": ENOTSUP before any device is touched
    with pytest.raises(_lib.LbsimError) as e:
        VecLoadBalanceEnv(8, 4, device="cuda:99", ps_cores=[1, 2, 3, 4])
    assert e.value.code == _lib.ENOTSUP and "lbsim_processor_sharing_enable" in str(e.value)
    # a FIFO handle: the four entry points refuse, naming the enable
    fifo = VecLoadBalanceEnv(8, 4, device="cuda:0")
    fifo.reset()
    dev = torch.device("cuda:0")
    c = torch.ones((8, 4), dtype=torch.int32, device=dev)
    buf = torch.empty((8, 4, 4), dtype=torch.float32, device=dev)
    for call in (lambda: fifo.handle.set_ps_cores(c, rows=8), fifo.handle.ps_cores,
                 fifo.handle.clear_ps_cores, lambda: fifo.handle.ps_server_state(buf),
                 lambda: fifo.set_ps_cores([1, 1, 1, 1]), fifo.get_ps_cores, fifo.clear_ps_cores,
                 fifo.ps_state):
        with pytest.raises(_lib.LbsimError) as e:
            call()
        assert e.value.code == _lib.ENOTSUP and "lbsim_processor_sharing_enable" in str(e.value)
    fifo.step(torch.zeros((8, 4), dtype=torch.int64))
    fifo.close()
    # server_workers with PS stays refused, in both orders and in the facade, cores or not
    h = Handle(make_config(8, 4), 0)
    h.enable_processor_sharing()
    h.set_ps_cores(c, rows=8)
    with pytest.raises(_lib.LbsimError) as e:
        h.enable_server_workers()
    assert e.value.code == _lib.ENOTSUP
    h.close()
    with pytest.raises(_lib.LbsimError) as e:
        VecLoadBalanceEnv(8, 4, device="cuda:0", service_discipline="ps", server_workers=True,
                          ps_cores=[1, 2, 3, 4])
    assert e.value.code == _lib.ENOTSUP
    env = VecLoadBalanceEnv(8, 4, device="cuda:0", service_discipline="ps")
    with pytest.raises(RuntimeError):
        env.ps_state()  # before reset()
    with pytest.raises(ValueError):
        env.handle.ps_server_state(buf)  # the C entry point: EINVAL before the first reset
    env.reset()
    # counts out of range: EINVAL, and before the first valid call nothing is in force but ones
    for bad in ([0, 1, 1, 1], [1, 65, 1, 1], [1, 1, -3, 1], [1, 1, 1, 1000]):
        with pytest.raises(ValueError):
            env.set_ps_cores(bad)
        assert bool((env.get_ps_cores() == 1).all())
    env.set_ps_cores([1, 2, 3, 64])
    for bad in ([0, 1, 1, 1], [1, 65, 1, 1], [1.5, 1, 1, 1], [float("nan"), 1, 1, 1],
                [True, True, True, True]):
        with pytest.raises(ValueError):
            env.set_ps_cores(bad)
        assert env.get_ps_cores().cpu().tolist() == [[1, 2, 3, 64]] * 8  # what was in force stays
    for shape in ((3,), (2, 4), (8, 3)):
        with pytest.raises(ValueError):
            env.set_ps_cores(np.ones(shape, np.int64))
    with pytest.raises(_lib.LbsimError) as e:  # the C entry point: rows other than 1 or B
        env.handle.set_ps_cores(c, rows=2)
    assert e.value.code == _lib.ESHAPE
    assert L.lbsim_set_ps_cores(env.handle.h, None, 1, None) == _lib.EINVAL
    with pytest.raises(ValueError):
        env.ps_state(torch.empty((8, 4, 3), dtype=torch.float32, device=dev))
    # ground_truth stays refused with the FIFO message
    with pytest.raises(_lib.LbsimError) as e:
        env.ground_truth()
    assert e.value.code == _lib.ENOTSUP and "FIFO" in str(e.value)
    env.step(torch.zeros((8, 4), dtype=torch.int64))
    assert env.get_ps_cores().cpu().tolist() == [[1, 2, 3, 64]] * 8
    env.close()


# ---- theory on the device

def cores_run(seed, c, tables=None, fifo=False):
    rec = tp.TH_REC["pareto" if tables is not None else "exp"]
    kw = dict(server_workers=[c]) if fifo else dict(service_discipline="ps", ps_cores=[c])
    r = qt.device_run(1, [1.0], tp.th_burn(), rec, seed, tables=tables, arrival_rate=TH_LAM,
                      server_rates=[TH_CAP / c], **kw)
    assert r.drops == 0 or fifo
    assert r.count.sum() > 0.9 * qt.B * rec * TH_LAM * qt.DT
    return r


@pytest.fixture(scope="module")
def theory_runs(lib):
    return {"exp-2": cores_run(9430, 2), "exp-4": cores_run(9431, 4),
            "pareto-2": cores_run(9432, 2, tables=tp.pareto_tables()),
            "fifo-pareto-2": cores_run(9432, 2, tables=tp.pareto_tables(), fifo=True)}


def cores_checks(r, c, name):
    w = mmc_ps(c, TH_CAP / c, TH_LAM)
    n_mean = r.in_flight.sum(1) / r.rec
    return [qt.Check(f"{name} mean sojourn time", *qt.server_mean(r, 0), w),
            qt.Check(f"{name} Little: mean column 0 against lambda W", n_mean.mean(),
                     n_mean.std(ddof=1) / math.sqrt(qt.B), lambda k: TH_LAM * w(k))]


@gpu
@pytest.mark.parametrize("key", ["exp-2", "exp-4", "pareto-2"])
def test_theory_mmc_ps(theory_runs, key):
    """M/M/c-PS at c = 2 and 4, and M/G/2-PS with bounded-Pareto(1.5, 1000) sizes: the mean
    sojourn time is 1 / mu + C(c, lambda / mu) / (c mu - lambda) whatever the size distribution
    (equally shared state-dependent-rate PS is insensitive), and by Little's law the mean of
    column 0 is lambda times it.  Both fail with mu scaled by 1.03."""
    c = int(key.split("-")[1])
    checks = cores_checks(theory_runs[key], c, f"M/G/{c}-PS ({key})")
    qt.assert_checks(checks)
    for chk in checks:
        assert not chk.ok(1.03), f"does not discriminate: {chk}"


@gpu
def test_theory_discriminates_the_discipline(theory_runs):
    """The same Pareto run on a FIFO handle with server_workers = 2 fails the check."""
    chk = cores_checks(theory_runs["fifo-pareto-2"], 2, "FIFO, 2 workers, Pareto sizes")[0]
    print(chk)
    assert not chk.ok(), f"a FIFO server would pass: {chk}"
