"""Multi-worker servers: per-server worker counts in the flow dynamics.

The reference is tests/workers_ref.WorkerSim, tests/flowsim_ref.FlowSim with §3.18 added from its
text, in two formulations: explicit per-worker free times and the sorted-queue rule.  The scenario,
cases, actions and weights are tests/test_flowsim_ref.py's (reset, 6 steps, a masked reset of every
third env, 6 steps).  The worker rows cycle through 1, 2, 3, 4 by env; env 0 is all 1 and env 5
mixes the counts over its servers.  Each server's rate is divided by its count, so the queues stay
as deep as in the plain cases.

Not gpu: the two formulations against each other, c = 1 against plain FlowSim (which
test_flowsim_ref pins to the oracle), what the scenario reaches, the helpers of
csrc/lbsim_workers.h compiled as host C++ under the address and undefined-behaviour sanitizers
against a naive model, the sampler, the ABI and the theory test's sizes.  gpu: enabled handles
against the reference exactly, all counts 1 against the unmodified oracle, the ring contents, the
interplay with the other domains, and the M/M/c closed forms.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import oracle
from marllb_amd import build, flowstats
from marllb_amd.env import make_config
from tests import parity, statelayout
from tests import test_flowsim_ref as fr
from tests import test_queueing_theory as qt
from tests import workers_ref as wr
from tests.flowsim_ref import FlowSim
from tests.parity import lib  # noqa: F401  (the fixture: fails a gpu test run without a device)

HERE = os.path.dirname(os.path.abspath(__file__))
K = 128
CASES = fr.CASES
STEPS, RESET_AT = fr.STEPS, fr.RESET_AT
gpu = pytest.mark.gpu
MIXED_ENV = 5


# ------------------------------------------------------------------ the scenario's parameters

def workers_of(case, B, variant=0):
    """(B, S) worker counts: env b has 1 + (b + variant) % 4 workers on every server; env 0 is
    all 1 (variant 0) and env MIXED_ENV cycles 1, 2, 3, 4 over its servers."""
    S = CASES[case][0]
    w = np.repeat((1 + (np.arange(B) + variant) % 4)[:, None], S, axis=1)
    if B > MIXED_ENV:
        w[MIXED_ENV] = 1 + (np.arange(S) + variant) % 4
    return w.astype(np.int32)


def rates_of(case, B, workers):
    """(B, S) f32 per-worker server rates: the case's rate divided by the server's count."""
    S, kw = fr.config_kwargs(case)
    cfg = make_config(B, S, **kw)
    base = np.array([cfg.server_rate[s] for s in range(S)], np.float32)
    return (base[None, :] / workers.astype(np.float32)).astype(np.float32)


def make_sims(case, B, workers, mus, explicit=False, cls=wr.WorkerSim):
    S, kw = fr.config_kwargs(case)
    cfg = make_config(B, S, **kw)
    return [cls(kw["seed"], cfg.env_id_offset + b, S, cfg.queue_capacity,
                kw.get("assign_policy", "sed"), cfg.arrival_rate, [float(x) for x in mus[b]],
                dt=cfg.step_interval, warmup_steps=cfg.warmup_steps, trace=kw.get("trace"),
                workers=workers[b], explicit=explicit) for b in range(B)]


_RUNS = {}
CHANGE_AT = 3  # variant "change": new worker counts before step 3 (and they stay)


def reference_run(case, B, explicit=False, change=False, ones=False):
    """The scenario on B WorkerSim envs -> (cfg, kwargs, actions, events, workers, mus, sims).
    An Event also carries the raw StepResults (ev.results[b]: a list) and the queues after it
    (ev.queues[b][s]: [(tc, ta)] absolute us).  Computed once per key."""
    key = (case, B, explicit, change, ones)
    if key in _RUNS:
        return _RUNS[key]
    S, kw = fr.config_kwargs(case)
    cfg = make_config(B, S, **kw)
    workers = np.ones((B, S), np.int32) if ones else workers_of(case, B)
    mus = rates_of(case, B, workers_of(case, B))
    sims = make_sims(case, B, workers, mus, explicit)
    drops = np.zeros(B, np.int64)
    acts = fr.actions_of(case, B)
    events = []

    def snapshot(ev):
        ev.dropped = drops.copy()
        ev.in_flight = np.array([m.in_flight() for m in sims])
        ev.arr_idx = np.array([m.k for m in sims])
        ev.next_abs = np.array([m.next_arrival() for m in sims])
        ev.steps = np.array([m.step_no for m in sims])
        ev.queues = [[list(q) for q in m.queues] for m in sims]
        events.append(ev)

    def reset(mask):
        ev = fr.Event(B, S)
        ev.mask = mask
        ev.results = [[] for _ in range(B)]
        for b in np.flatnonzero(mask):
            drops[b] = 0
            for r in sims[b].reset():
                drops[b] += r.dropped
                ev.results[b].append(r)
                for s in range(S):
                    ev.new[b][s][0].extend(r.fct(s))
                    ev.new[b][s][1].extend(r.tc(s))
        snapshot(ev)

    reset(np.ones(B, bool))
    for k in range(STEPS):
        if k == RESET_AT:
            reset(np.arange(B) % 3 == 0)
        if change and k == CHANGE_AT:
            for b, m in enumerate(sims):
                m.set_workers(workers_of(case, B, variant=1)[b])
        wts = fr.weights_of(acts[k], kw)
        ev = fr.Event(B, S)
        ev.results = [[] for _ in range(B)]
        for b in range(B):
            r = sims[b].step(wts[b])
            ev.results[b].append(r)
            ev.assigned[b] = r.assigned
            drops[b] += r.dropped
            ev.new[b] = [(r.fct(s), r.tc(s)) for s in range(S)]
        snapshot(ev)
    _RUNS[key] = (cfg, kw, acts, events, workers, mus, sims)
    return _RUNS[key]


def drive(case, B, backend, check, change=False, ones=False):
    """The scenario on `backend`: check(event, outputs) after every reset and step."""
    events = reference_run(case, B, change=change, ones=ones)[3]
    acts = fr.actions_of(case, B)
    it = iter(events)
    check(next(it), backend.reset(None))
    for k in range(STEPS):
        if k == RESET_AT:
            check(next(it), backend.reset((np.arange(B) % 3 == 0).astype(np.uint8)))
        if change and k == CHANGE_AT:
            backend.env.set_server_workers(workers_of(case, B, variant=1))
        check(next(it), backend.step(acts[k]))
    return events


# ------------------------------------------------------------------ not gpu: the reference

HOST_B = 12


@pytest.mark.parametrize("case", list(CASES))
def test_explicit_workers_equal_the_sorted_queue_rule(case):
    """Formulation (a), per-worker free times, and (b), the start from sorted position n - c, are
    the same process event for event at constant c."""
    a = reference_run(case, HOST_B, explicit=True)[3]
    b = reference_run(case, HOST_B)[3]
    assert len(a) == len(b)
    for ea, eb in zip(a, b):
        np.testing.assert_array_equal(ea.assigned, eb.assigned)
        np.testing.assert_array_equal(ea.dropped, eb.dropped)
        np.testing.assert_array_equal(ea.next_abs, eb.next_abs)
        assert ea.queues == eb.queues
        for ra, rb in zip(ea.results, eb.results):
            assert len(ra) == len(rb)
            for x, y in zip(ra, rb):
                assert x.completed == y.completed and x.records == y.records


@pytest.mark.parametrize("case", list(CASES))
def test_one_worker_is_flowsim(case):
    """WorkerSim with every count 1 is FlowSim event for event, records in FIFO order; through
    test_flowsim_ref's OracleBackend test that is the oracle."""
    S, kw = fr.config_kwargs(case)
    B = 4
    cfg = make_config(B, S, **kw)
    acts = fr.actions_of(case, B)
    for b in range(B):
        args = (kw["seed"], cfg.env_id_offset + b, S, cfg.queue_capacity,
                kw.get("assign_policy", "sed"), cfg.arrival_rate,
                [cfg.server_rate[s] for s in range(S)])
        opt = dict(dt=cfg.step_interval, warmup_steps=cfg.warmup_steps, trace=kw.get("trace"))
        plain, one = FlowSim(*args, **opt), wr.WorkerSim(*args, workers=[1] * S, **opt)

        def same(ra, rb):
            np.testing.assert_array_equal(ra.assigned, rb.assigned)
            assert ra.dropped == rb.dropped and ra.completed == rb.completed
            for s in range(S):
                assert ra.fct(s) == rb.fct(s) and ra.tc(s) == rb.tc(s)
            assert plain.in_flight() == one.in_flight() and plain.k == one.k
            assert plain.queues == one.queues

        for ra, rb in zip(plain.reset(), one.reset()):
            same(ra, rb)
        for k in range(STEPS):
            if k == RESET_AT and b % 3 == 0:
                for ra, rb in zip(plain.reset(), one.reset()):
                    same(ra, rb)
            wt = fr.weights_of(acts[k], kw)[b]
            same(plain.step(wt), one.step(wt))
        assert one.reach["out_of_order"] == 0


def reach_of(case, B):
    sims = reference_run(case, B)[6]
    return {k: sum(m.reach[k] for m in sims) for k in sims[0].reach}


def check_reaches(case, B):
    """The scenario is not vacuous (asserted on the reference alone)."""
    _, _, _, events, workers, _, _ = reference_run(case, B)
    S = CASES[case][0]
    count = np.zeros((B, S), np.int64)
    peak = 0
    for ev in events:
        if ev.mask is not None:
            count[ev.mask] = 0
        count += np.array([[len(ev.new[b][s][0]) for s in range(S)] for b in range(B)])
        peak = max(peak, int(count.max()))
    assert peak <= K, "a reservoir wrapped: its records no longer list every flow"
    assert any(ev.mask is not None and not ev.mask.all() for ev in events)
    r = reach_of(case, B)
    assert r["pushes"] > 20 * B
    if workers.max() > 1:
        assert r["out_of_order"] > 0 and r["max_shift"] > 0
    return peak, r


def test_scenario_reaches():
    total = {}
    for case in CASES:
        peak, r = check_reaches(case, HOST_B)
        print(f"REACH {case}: peak reservoir count {peak}, {r}")
        for k, v in r.items():
            total[k] = total.get(k, 0) + v
    # an out-of-order insert, an insert at position 0 of a non-empty queue, an insert that
    # shifts c - 1 entries, carried-in completions out of arrival order, a drop at full queues
    # with c > 1
    for k in ("out_of_order", "at_head", "max_shift", "carried_out_of_order", "multi_drop"):
        assert total[k] > 0, k
    # the window / ring boundary: an entry moved from position 7 to 8, and a start taken from an
    # entry in the ring part, both on s4-q64-deep, whose envs with c >= 2 queue that deep
    deep = reach_of("s4-q64-deep", HOST_B)
    assert deep["cross_window"] > 0 and deep["ring_start"] > 0, deep
    for case in ("s1-q3-drops", "s3-lsq-q6-overload"):
        assert reach_of(case, HOST_B)["multi_drop"] > 0, case


# ------------------------------------------------------------------ not gpu: the helpers

def test_helpers_against_a_naive_model(tmp_path):
    """tests/workers_probe.cpp: the position arithmetic, the start rule and the sorted insert of
    csrc/lbsim_workers.h on a window plus ring, for every c in 1..64 and Q in {3, 8, 9, 32, 64},
    under the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "workers_probe")
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "workers_probe.cpp")], check=True)
    for seed in (1, 2):
        r = subprocess.run([exe, str(seed)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        rows = [[int(x) for x in line.split()] for line in r.stdout.splitlines()]
        assert [(c, q) for c, q, *_ in rows] == [(c, q) for c in range(1, 65)
                                                 for q in (3, 8, 9, 32, 64)]
        for c, q, pushes, ooo, shift, ring in rows:
            assert pushes > 50 and shift <= min(c, q) - 1
            assert (ooo == 0) == (c == 1)
        # the largest shift is reached, and starts are read from the ring part
        assert max(shift for c, *_, shift, _ in rows if c == 4) == 3
        assert max(shift for *_, shift, _ in rows) == 63
        assert sum(ring for c, q, *_, ring in rows if q >= 32 and 2 <= c <= 8) > 0


def test_sampler_and_abi():
    import torch
    from marllb_amd import _lib, sample_server_workers
    w, mu = sample_server_workers(300, 6, seed=4, server_rates=120.0)
    assert w.shape == (300, 6) and w.dtype == torch.int32
    assert mu.shape == (300, 6) and mu.dtype == torch.float32
    assert set(w.unique().tolist()) == {1, 2, 4}
    assert torch.equal(mu, (120.0 / w.double()).float())  # equal capacity c * mu
    w2, mu2 = sample_server_workers(300, 6, seed=4, server_rates=120.0)
    assert torch.equal(w, w2) and torch.equal(mu, mu2)
    assert not torch.equal(w, sample_server_workers(300, 6, seed=5)[0])
    w3, mu3 = sample_server_workers(8, 3, choices=(1, 64), keep_capacity=False,
                                    server_rates=[10.0, 20.0, 30.0])
    assert set(w3.unique().tolist()) <= {1, 64}
    assert torch.equal(mu3, torch.tensor([10.0, 20.0, 30.0]).expand(8, 3))
    lo = sample_server_workers(50, 2, choices=(64,), server_rates=2.0)[1]
    assert float(lo.min()) == 1.0  # clamped to the valid range of a server rate
    for bad in (dict(choices=(0, 1)), dict(choices=(65,)), dict(choices=()),
                dict(choices=(1.5,)), dict(server_rates=-1.0)):
        with pytest.raises(ValueError):
            sample_server_workers(4, 4, **bad)
    header = open(os.path.join(os.path.dirname(HERE), "include", "lbsim.h")).read()
    for name, nargs in (("lbsim_server_workers_enable", 1), ("lbsim_set_server_workers", 4),
                        ("lbsim_get_server_workers", 3), ("lbsim_clear_server_workers", 2)):
        assert f"int {name}(" in header
        assert len(_lib._SIGNATURES[name][1]) == nargs
    assert "#define LBSIM_ABI_VERSION 10 " in header


# ------------------------------------------------------------------ theory: M/M/c

TH_MU, TH_RHO = 40.0, 0.7
TH_C = (2, 4)
TH_REC = {2: 160, 4: 100}  # recorded steps of the device runs, sized on the reference below


def th_lam(c):
    return TH_RHO * c * TH_MU


def erlang_c(c, a):
    """P(wait) of M/M/c at offered load a = lambda / mu < c."""
    rho = a / c
    top = a ** c / math.factorial(c) / (1.0 - rho)
    return top / (sum(a ** k / math.factorial(k) for k in range(c)) + top)


def mmc(c, mu, lam):
    """Mean sojourn time of M/M/c, mu scaled by k."""
    return lambda k: 1.0 / (k * mu) + erlang_c(c, lam / (k * mu)) / (c * k * mu - lam)


def th_burn(c):
    # the decay rate of M/M/c at this load is that of M/M/1 at rate c mu
    return qt.burn_steps(qt.relaxation(c * TH_MU, th_lam(c)))


def test_theory_formulas():
    assert abs(erlang_c(1, 0.5) - 0.5) < 1e-15  # M/M/1: P(wait) = rho
    assert abs(mmc(1, 40.0, 20.0)(1.0) - qt.mm1(40.0, 20.0)(1.0)) < 1e-15
    assert abs(erlang_c(2, 1.4) - 0.98 / 0.3 / (2.4 + 0.98 / 0.3)) < 1e-12


@pytest.mark.parametrize("c", TH_C)
def test_theory_sizes_on_the_reference(c):
    """The reference alone, at reduced size, meets the M/M/c mean and Little's law, and
    1 / sqrt(n) scaling of its standard errors puts the device run under the cap."""
    envs, rec = 64, 30
    lam = th_lam(c)
    count, sum_us, in_flight = np.zeros(envs), np.zeros(envs), np.zeros(envs)
    for b in range(envs):
        sim = wr.WorkerSim(9300 + c, b, 1, qt.Q, "lsq", lam, [TH_MU], dt=qt.DT, warmup_steps=0,
                           workers=[c])
        sim.reset()
        for _ in range(th_burn(c)):
            sim.step([1.0])
        for _ in range(rec):
            for _, ta, tc in sim.step([1.0]).completed:
                count[b] += 1
                sum_us[b] += tc - ta
            in_flight[b] += sim.in_flight()[0]
    scale = math.sqrt(envs * rec / (qt.B * TH_REC[c]))
    est, se = qt.ratio(sum_us * 1e-6, count)
    w = mmc(c, TH_MU, lam)
    n_mean = in_flight / rec
    for chk in (qt.Check(f"reference M/M/{c} mean", est, se, w),
                qt.Check(f"reference M/M/{c} Little", n_mean.mean(),
                         n_mean.std(ddof=1) / math.sqrt(envs), lambda k: lam * w(k))):
        print(chk)
        assert chk.ok()
        assert chk.se * scale <= qt.CAP * chk.theory(1.0)


# ------------------------------------------------------------------ the device

GPU_B = fr.GPU_B


def workers_state(env):
    c = env.cfg
    return statelayout.parse(env.handle.state_bytes(), c.num_envs, c.num_servers, c.queue_capacity,
                             bool(c.normalize_obs), c.fail_prob > 0 or env.server_availability,
                             leak=False, dur_plane=statelayout.has_dur_plane(c))


class DeviceBackend:
    """reset / step -> (obs, reward or None, assign counts or None), numpy."""

    def __init__(self, B, S, kw, workers=None, mus=None, **extra):
        import torch
        from marllb_amd.env import VecLoadBalanceEnv
        self.torch = torch
        self.env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=False, **extra, **kw)
        if workers is not None:
            self.env.set_server_workers(workers)
        if mus is not None:
            self.env.set_rates(None, mus)

    def reset(self, mask):
        obs = self.env.reset(mask=None if mask is None else self.torch.from_numpy(mask))
        return obs.cpu().numpy(), None, None

    def step(self, a):
        obs, rew, _, info = self.env.step(self.torch.from_numpy(a), assign_counts=True)
        return obs.cpu().numpy(), rew.cpu().numpy(), info["assign_counts"].cpu().numpy()


def check_features(env, d, obs, rew, who):
    """Columns 1-10 are oracle.features of the state's records and the reward is oracle.rewards of
    the observation, bit for bit."""
    B, S = env.cfg.num_envs, env.cfg.num_servers
    val = d["res_fct"].view(np.int32).astype(np.float32) * np.float32(1e-6)
    f = oracle.features(val, d["res_ts"], d["res_count"]).reshape(B, S, 5)
    np.testing.assert_array_equal(obs[:, :, 1:6], f, err_msg=f"{who}: fct features")
    np.testing.assert_array_equal(obs[:, :, 6:11], f, err_msg=f"{who}: duration features")
    if rew is not None:
        want = oracle.rewards(obs, env.cfg.reward_metric, env.cfg.reward_field)
        np.testing.assert_array_equal(rew, want, err_msg=f"{who}: reward")


class WorkersCheck:
    """An Event of the reference against an enabled handle's state and outputs."""

    def __init__(self, env, stats=False, rings=True):
        self.env, self.cfg = env, env.cfg
        self.B, self.S = env.cfg.num_envs, env.cfg.num_servers
        self.dt = int(round(env.cfg.step_interval * 1e6))
        self.count = np.zeros((self.B, self.S), np.int64)
        self.stats, self.rings = stats, rings
        self.sorted_rings = self.inversions = 0
        self.fs = [np.zeros((self.B, self.S), np.uint32), np.zeros((self.B, self.S), np.uint64),
                   np.zeros((self.B, self.S), np.uint32),
                   np.zeros((self.B, self.S, flowstats.NBINS), np.uint32)]

    def __call__(self, ev, out):
        B, S = self.B, self.S
        obs, rew, assign = out
        d = workers_state(self.env)
        if assign is not None:
            np.testing.assert_array_equal(assign, ev.assigned, err_msg="assign_counts")
        np.testing.assert_array_equal(d["dropped"], ev.dropped, err_msg="dropped")
        np.testing.assert_array_equal(d["arr_idx"], ev.arr_idx, err_msg="arrival index")
        np.testing.assert_array_equal(d["clock"], ev.steps, err_msg="clock")
        np.testing.assert_array_equal(d["next_arr"].astype(np.int64) + ev.steps * self.dt,
                                      ev.next_abs, err_msg="next arrival")
        queued = (d["hc"].reshape(B, S) >> 16).astype(np.int64)
        np.testing.assert_array_equal(queued, ev.in_flight, err_msg="hc count")
        np.testing.assert_array_equal(obs[:, :, 0], ev.in_flight.astype(np.float32),
                                      err_msg="observation column 0")
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
        check_features(self.env, d, obs, rew, "server-workers handle")
        if self.rings:
            self.check_rings(ev, d)
        if self.stats:
            self.check_stats(ev, assign is not None)

    def check_rings(self, ev, d):
        """Each server's live ring entries, from the head: non-decreasing tc, and equal to the
        reference's queue (times relative to the next step's start)."""
        B, S, Q = self.B, self.S, self.cfg.queue_capacity
        hc = d["hc"].reshape(B, S)
        ring = d["ring"].view(np.int32).reshape(B, S, Q, 2).astype(np.int64)
        for b in range(B):
            base = int(ev.steps[b]) * self.dt
            for s in range(S):
                h, n = int(hc[b, s] & 0x7FFF), int(hc[b, s] >> 16)
                got = [(int(ring[b, s, (h + i) % Q, 0]), int(ring[b, s, (h + i) % Q, 1]))
                       for i in range(n)]
                tcs = [t for t, _ in got]
                assert tcs == sorted(tcs), ("ring order", b, s)
                assert got == [(tc - base, ta - base) for tc, ta in ev.queues[b][s]], (
                    "ring contents", b, s)
                tas = [a for _, a in got]
                self.sorted_rings += n > 1
                self.inversions += tas != sorted(tas)

    def check_stats(self, ev, is_step):
        if is_step:
            for b in range(self.B):
                for s in range(self.S):
                    v = np.array(ev.new[b][s][0], np.int64)
                    if len(v):
                        self.fs[0][b, s] += len(v)
                        self.fs[1][b, s] += np.uint64(v.sum())
                        self.fs[2][b, s] = max(int(self.fs[2][b, s]), int(v.max()))
                        np.add.at(self.fs[3][b, s], flowstats.bin_of(v), 1)
        cnt, sm, mx, h = (t.cpu().numpy() for t in self.env.handle.flow_stats(hist=True))
        np.testing.assert_array_equal(cnt.view(np.uint32), self.fs[0], err_msg="flow count")
        np.testing.assert_array_equal(sm.view(np.uint64), self.fs[1], err_msg="flow sum_us")
        np.testing.assert_array_equal(mx.view(np.uint32), self.fs[2], err_msg="flow max_us")
        np.testing.assert_array_equal(h.view(np.uint32), self.fs[3], err_msg="flow hist")


def check_full_kernel(lib, env):
    names = lib.launch_names(env.handle)
    assert lib.load().lbsim_dynamics_kernel(env.handle.h) == parity.GROUP, names
    assert names.get(0, "").startswith("dynamics_group_full_kernel<"), names


MAPPED = [(c, m) for c in CASES for m in ("auto", "env", "server")
          if m != "env" or CASES[c][0] <= 16]


@gpu
@pytest.mark.parametrize("case,mapping", MAPPED)
def test_enabled_handles_equal_the_reference(lib, case, mapping):
    S, kw = fr.config_kwargs(case)
    _, _, _, _, workers, mus, _ = reference_run(case, GPU_B)
    back = DeviceBackend(GPU_B, S, kw, workers=workers, mus=mus, server_workers=True,
                         dyn_mapping=mapping)
    chk = WorkersCheck(back.env)
    drive(case, GPU_B, back, chk)
    check_full_kernel(lib, back.env)
    check_reaches(case, GPU_B)
    assert chk.inversions > 0  # rings whose arrival times are out of order were compared
    np.testing.assert_array_equal(back.env.get_server_workers().cpu().numpy(), workers)
    back.env.close()


@gpu
def test_forced_four_lane_groups():
    """LBSIM_DYN_GROUP_LANES=4: the headline shape's 4-lane full kernel on the S <= 4 cases."""
    ks = [f"test_enabled_handles_equal_the_reference[{c}-auto]" for c, v in CASES.items()
          if v[0] <= 4]
    assert len(ks) >= 6
    parity.run_cases_in_child("test_server_workers.py", ks, {"LBSIM_DYN_GROUP_LANES": "4"})


def _parity_configs():
    from tests.test_gpu_parity import CONFIGS
    return [i for i, c in enumerate(CONFIGS)
            if "lost_fin_prob" not in c["kw"] and c["kw"].get("duration_mode") != "service"]


@gpu
@pytest.mark.parametrize("idx", _parity_configs())
def test_all_counts_one_equals_the_oracle(lib, oracle_mod, idx):
    """An enabled handle whose counts are all 1 (set explicitly, through the in-place rewrite):
    every output and every state section equal the unmodified oracle's, on the full kernel."""
    from marllb_amd.env import VecLoadBalanceEnv
    from tests.test_gpu_parity import CONFIGS, resolve_kw
    c = CONFIGS[idx]
    B, S, kw = c["B"], c["S"], resolve_kw(c["kw"])
    kw.setdefault("seed", 1000 + idx)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=False, server_workers=True, **kw)
    env.set_server_workers(np.ones(S, np.int64))
    ora = oracle_mod.OracleEnv(make_config(B, S, **kw), threads=4, trace=kw.get("trace"))
    parity.run_vs_reference(env, ora, dict(c["kw"]), idx, steps=8, post_steps=4,
                            hook=lambda e: check_full_kernel(lib, e), levels=True)
    ora.close()
    env.close()


# ---- each of the following once

ONCE = "s4-q64-deep"  # Q = 64, queues past the window: the ring part takes part in every test


def small_pair(case=ONCE, B=24, **extra):
    S, kw = fr.config_kwargs(case)
    workers = workers_of(case, B)
    mus = rates_of(case, B, workers)
    back = DeviceBackend(B, S, kw, workers=workers, mus=mus, server_workers=True, **extra)
    return back, S, kw, workers, mus


def assert_matches_sims(env, sims, drops):
    B, S = env.cfg.num_envs, env.cfg.num_servers
    d = workers_state(env)
    np.testing.assert_array_equal(d["hc"].reshape(B, S) >> 16,
                                  np.array([m.in_flight() for m in sims]))
    np.testing.assert_array_equal(d["arr_idx"], np.array([m.k for m in sims]))
    np.testing.assert_array_equal(d["dropped"], drops)
    return d


@gpu
@pytest.mark.parametrize("case", ["s4-sed-levels", "s3-lsq-q6-overload", "s8-trace37",
                                  "s6-alias-continuous"])
def test_mid_run_change(lib, case):
    """New counts before step 3, against formulation (b): arrivals assigned from that launch on
    start by the new c, queued flows keep their tc.  (Not s4-q64-deep: with more workers at
    unchanged rates its reservoirs pass 128 records, 130 on the reference, and no longer list
    every flow; three of these cases queue past the window.)"""
    S, kw = fr.config_kwargs(case)
    _, _, _, _, workers, mus, _ = reference_run(case, GPU_B, change=True)
    back = DeviceBackend(GPU_B, S, kw, workers=workers, mus=mus, server_workers=True)
    drive(case, GPU_B, back, WorkersCheck(back.env), change=True)
    back.env.close()


@gpu
@pytest.mark.parametrize("case", ["s4-q64-deep", "s5-lsq2-unequal"])
def test_flow_statistics(lib, case):
    S, kw = fr.config_kwargs(case)
    _, _, _, _, workers, mus, _ = reference_run(case, GPU_B)
    back = DeviceBackend(GPU_B, S, kw, workers=workers, mus=mus, server_workers=True,
                         flow_stats=True)
    chk = WorkersCheck(back.env, stats=True)
    drive(case, GPU_B, back, chk)
    assert int(chk.fs[0].sum()) > 5 * GPU_B
    back.env.close()


@gpu
def test_per_env_rates_through_the_sampler(lib):
    """sample_server_workers's counts and equal-capacity rates on the device, against the
    reference run at the same values."""
    from marllb_amd import sample_server_workers
    case, B = "s4-sed-levels", 24
    S, kw = fr.config_kwargs(case)
    w, mu = sample_server_workers(B, S, seed=3, server_rates=20.0)
    workers, mus = w.numpy(), mu.numpy()
    back = DeviceBackend(B, S, kw, workers=w, mus=mu, server_workers=True)
    sims = make_sims(case, B, workers, mus)
    drops = np.array([sum(r.dropped for r in m.reset()) for m in sims])
    back.reset(None)
    acts = fr.actions_of(case, B)
    for k in range(6):
        assert_matches_sims(back.env, sims, drops)
        wts = fr.weights_of(acts[k], kw)
        _, _, assign = back.step(acts[k])
        rs = [m.step(wts[b]) for b, m in enumerate(sims)]
        drops += np.array([r.dropped for r in rs])
        np.testing.assert_array_equal(assign, np.array([r.assigned for r in rs]))
    assert_matches_sims(back.env, sims, drops)
    assert sum(m.reach["out_of_order"] for m in sims) > 0
    back.env.close()


@gpu
def test_scripted_outage_frees_the_workers(lib):
    """Server 1 of every env scripted down for one step: its queue is dropped and its workers are
    idle when it comes back (the reference empties the queue, frees the workers and keeps the
    server full of flows that never complete while it is down)."""
    B, J = 24, 1
    back, S, kw, workers, mus = small_pair(ONCE, B, server_availability=True)
    env, Q = back.env, back.env.cfg.queue_capacity
    sims = make_sims(ONCE, B, workers, mus)
    drops = np.array([sum(r.dropped for r in m.reset()) for m in sims])
    back.reset(None)
    acts = fr.actions_of(ONCE, B)

    def both_step(k):
        nonlocal drops
        wts = fr.weights_of(acts[k], kw)
        _, _, assign = back.step(acts[k])
        rs = [m.step(wts[b]) for b, m in enumerate(sims)]
        drops = drops + np.array([r.dropped for r in rs])
        np.testing.assert_array_equal(assign, np.array([r.assigned for r in rs]))

    for k in range(3):
        both_step(k)
    assert_matches_sims(env, sims, drops)
    assert sum(len(m.queues[J]) for m in sims) > B
    up = np.ones((1, S), np.uint8)
    up[0, J] = 0
    env.set_server_availability(up)
    never = 1 << 60
    for b, m in enumerate(sims):
        drops[b] += m.fail(J)
        m.queues[J] = [(never, 0)] * Q
    both_step(3)
    for m in sims:
        assert len(m.queues[J]) == Q
        m.queues[J] = []
    d = assert_matches_sims(env, sims, drops)
    assert (d["down"].reshape(B, S)[:, J] != 0).all() and d["down"].sum() == B
    env.set_server_availability(np.ones((1, S), np.uint8))
    for k in range(4, 8):  # the server is back with idle workers: both go on alike
        both_step(k)
    assert_matches_sims(env, sims, drops)
    env.close()


@gpu
def test_random_failures_keep_the_rings_sorted(lib):
    """fail_prob > 0 with c > 1: after every step each live ring is in tc order, a down server's
    queue is empty, and flows are served out of arrival order (identities)."""
    B = 24
    S, kw = fr.config_kwargs(ONCE)
    workers = workers_of(ONCE, B)
    back = DeviceBackend(B, S, {**kw, "fail_prob": 0.2, "recover_prob": 0.5}, workers=workers,
                         mus=rates_of(ONCE, B, workers), server_workers=True)
    back.reset(None)
    acts = fr.actions_of(ONCE, B)
    Q = back.env.cfg.queue_capacity
    seen_down = inversions = 0
    for k in range(8):
        back.step(acts[k])
        d = workers_state(back.env)
        hc = d["hc"].reshape(B, S)
        ring = d["ring"].view(np.int32).reshape(B, S, Q, 2)
        down = d["down"].reshape(B, S) != 0
        assert not (hc >> 16)[down].any()
        seen_down += int(down.sum())
        for b in range(B):
            for s in range(S):
                h, n = int(hc[b, s] & 0x7FFF), int(hc[b, s] >> 16)
                e = [ring[b, s, (h + i) % Q] for i in range(n)]
                assert [int(x[0]) for x in e] == sorted(int(x[0]) for x in e), (k, b, s)
                inversions += [int(x[1]) for x in e] != sorted(int(x[1]) for x in e)
    assert seen_down > 0 and inversions > 0
    back.env.close()


@gpu
def test_hidden_cross_traffic_with_workers(lib):
    """Cross traffic on multi-worker servers, against the reference with §3.17 layered on: the
    visible and hidden counts, drops and assignments after every step; in every state lost_on is
    minus the number of flagged ring entries (a flag moves with its entry through the sorted
    insert) and the ring, flags included, is the reference's queue."""
    from tests import test_cross_traffic as ct
    B = 24
    S, kw = fr.config_kwargs(ONCE)
    workers = workers_of(ONCE, B)
    mus = rates_of(ONCE, B, workers)
    share, w = ct.cross_params(ONCE, B)
    back = DeviceBackend(B, S, kw, workers=workers, mus=mus, server_workers=True,
                         cross_traffic=True)
    back.env.set_cross_traffic(share, w)
    cfg = back.env.cfg
    sims = [wr.CrossWorkerSim(kw["seed"], cfg.env_id_offset + b, S, cfg.queue_capacity,
                              kw.get("assign_policy", "sed"), cfg.arrival_rate,
                              [float(x) for x in mus[b]], dt=cfg.step_interval,
                              warmup_steps=cfg.warmup_steps, workers=workers[b], share=share[b],
                              weights=w[b]) for b in range(B)]
    drops = np.array([sum(r.dropped for r in m.reset()) for m in sims])
    back.reset(None)
    acts = fr.actions_of(ONCE, B)
    Q, dt = cfg.queue_capacity, int(round(cfg.step_interval * 1e6))
    flag = np.iinfo(np.int32).min
    flagged_mid = 0
    for k in range(8):
        wts = fr.weights_of(acts[k], kw)
        obs, _, assign = back.step(acts[k])
        rs = [m.step(wts[b]) for b, m in enumerate(sims)]
        drops += np.array([r.dropped for r in rs])
        np.testing.assert_array_equal(assign, np.array([r.assigned for r in rs]))
        ct.assert_matches_sims(back.env, sims, drops)
        d, hid = ct.hidden_queued(back.env)
        np.testing.assert_array_equal(ct.ring_flags(back.env, d), hid)
        hc = d["hc"].reshape(B, S)
        np.testing.assert_array_equal(obs[:, :, 0], ((hc >> 16) - hid).astype(np.float32))
        ring = d["ring"].view(np.int32).reshape(B, S, Q, 2).astype(np.int64)
        for b in range(B):
            base = sims[b].step_no * dt
            for s in range(S):
                h, n = int(hc[b, s] & 0x7FFF), int(hc[b, s] >> 16)
                got = [(int(ring[b, s, (h + i) % Q, 0]), int(ring[b, s, (h + i) % Q, 1]))
                       for i in range(n)]
                want = [(tc - base, flag if hidden else ta - base)
                        for tc, ta, hidden in sims[b].queues[s]]
                assert got == want, ("ring contents and flags", k, b, s)
                flags = [e[2] for e in sims[b].queues[s]]
                # a hidden flow that is neither first nor last: it sits among visible ones
                flagged_mid += any(flags[1:-1]) and not all(flags)
    assert hid.sum() > 0 and flagged_mid > 0
    assert sum(m.reach["out_of_order"] for m in sims) > 0
    back.env.close()


@gpu
def test_next_step_auto_reset_across_an_episode_end(lib):
    """max_steps = 3 with next-step auto-reset: the step after an episode's end resets in place
    (the warm-up at the counts in force), against the reference."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    case, B = ONCE, 24
    S, kw = fr.config_kwargs(case)
    workers = workers_of(case, B)
    mus = rates_of(case, B, workers)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=True, autoreset_mode="next_step",
                            server_workers=workers, max_steps=3, **kw)
    env.set_rates(None, mus)
    sims = make_sims(case, B, workers, mus)
    drops = np.array([sum(r.dropped for r in m.reset()) for m in sims])
    env.reset()
    acts = fr.actions_of(case, B)
    for k in range(9):
        assert_matches_sims(env, sims, drops)
        wts = fr.weights_of(acts[k], kw)
        _, _, done, info = env.step(torch.from_numpy(acts[k]), assign_counts=True)
        if k % 4 == 3:  # the step after the third: every env resets instead of stepping
            drops = np.array([sum(r.dropped for r in m.reset()) for m in sims])
            assert not info["assign_counts"].any()
        else:
            rs = [m.step(wts[b]) for b, m in enumerate(sims)]
            drops += np.array([r.dropped for r in rs])
            np.testing.assert_array_equal(info["assign_counts"].cpu().numpy(),
                                          np.array([r.assigned for r in rs]))
            assert bool(done.all()) == (k % 4 == 2)
    assert_matches_sims(env, sims, drops)
    env.close()


@gpu
def test_snapshot_restore_and_fork(lib):
    """The layout is unchanged: a snapshot restores byte for byte, a fork copies the sorted rings,
    and restored envs step as a twin that never took the detour."""
    import torch
    B = 24
    back, S, kw, workers, mus = small_pair(ONCE, B)
    env = back.env
    size = env.handle.state_bytes()
    plain = DeviceBackend(B, S, kw)
    assert len(plain.env.handle.state_bytes()) == len(size)  # lbsim_state_size is unchanged
    plain.env.close()
    back.reset(None)
    acts = fr.actions_of(ONCE, B)
    for k in range(4):
        back.step(acts[k])
    snap = env.snapshot()
    before = env.handle.state_bytes()
    for k in range(4, 7):
        back.step(acts[k])
    env.restore(snap)
    assert env.handle.state_bytes() == before
    src = int((workers_state(env)["hc"].reshape(B, S) >> 16).sum(1).argmax())
    env.restore(snap, src=torch.full((B,), src, dtype=torch.int32))
    d = workers_state(env)
    hc = d["hc"].reshape(B, S)
    assert (hc == hc[src]).all()
    env.restore(snap)
    twin = DeviceBackend(B, S, kw, workers=workers, mus=mus, server_workers=True)
    twin.reset(None)
    for k in range(4):
        twin.step(acts[k])
    for k in range(4, 8):
        for x, y in zip(back.step(acts[k]), twin.step(acts[k])):
            np.testing.assert_array_equal(x, y)
    assert env.handle.state_bytes() == twin.env.handle.state_bytes()
    twin.env.close()
    env.close()


@gpu
def test_replayed_graph_sees_an_in_place_rewrite(lib):
    """A step captured before set_server_workers rewrites the array in place reads the new counts
    on replay: equal to an eager twin given the same counts at the same step."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    case, B = ONCE, 24
    S, kw = fr.config_kwargs(case)
    first, second = workers_of(case, B), workers_of(case, B, variant=2)
    mus = rates_of(case, B, first)
    eager = VecLoadBalanceEnv(B, S, device="cuda:0", server_workers=True, **kw)
    graph = VecLoadBalanceEnv(B, S, device="cuda:0", server_workers=True, graph_mode=True, **kw)
    for e in (eager, graph):
        e.set_server_workers(first)
        e.set_rates(None, mus)
        e.reset()
    acts = [torch.from_numpy(a).to("cuda:0") for a in fr.actions_of(case, B)[:7]]
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
    for k in range(1, 7):
        if k == 4:  # after three replays: new counts, no new capture
            for e in (eager, graph):
                e.set_server_workers(second)
        a_static.copy_(acts[k])
        cg.replay()
        eo, er, ed, _ = eager.step(acts[k])
        assert torch.equal(obs, eo), k
        assert torch.equal(rew, er) and torch.equal(done, ed), k
    assert graph.handle.state_bytes() == eager.handle.state_bytes()
    np.testing.assert_array_equal(graph.get_server_workers().cpu().numpy(), second)
    eager.close()
    graph.close()


@gpu
def test_shards_at_uneven_sizes(lib):
    """Shards of 5, 12 and 7 envs with their own rows equal the 24-env handle's rows."""
    case, B = ONCE, 24
    S, kw = fr.config_kwargs(case)
    workers = workers_of(case, B)
    mus = rates_of(case, B, workers)
    whole = DeviceBackend(B, S, kw, workers=workers, mus=mus, server_workers=True)
    acts = fr.actions_of(case, B)
    whole.reset(None)
    outs = [whole.step(acts[k]) for k in range(4)]
    dw = workers_state(whole.env)
    lo = 0
    for n in (5, 12, 7):
        part = DeviceBackend(n, S, {**kw, "env_id_offset": kw.get("env_id_offset", 0) + lo},
                             workers=workers[lo:lo + n], mus=mus[lo:lo + n], server_workers=True)
        part.reset(None)
        for k in range(4):
            got = part.step(acts[k][lo:lo + n])
            for x, y in zip(got, outs[k]):
                np.testing.assert_array_equal(x, y[lo:lo + n])
        dp = workers_state(part.env)
        np.testing.assert_array_equal(dp["hc"].reshape(n, S), dw["hc"].reshape(B, S)[lo:lo + n])
        np.testing.assert_array_equal(dp["dropped"], dw["dropped"][lo:lo + n])
        part.env.close()
        lo += n
    whole.env.close()


@gpu
def test_facades_forward(lib):
    """LoadBalanceEnv and VecMultiAgentLoadBalanceEnv set, read back and clear the counts."""
    from marllb_amd.env import LoadBalanceEnv
    from marllb_amd.multi_agent import VecMultiAgentLoadBalanceEnv
    one = LoadBalanceEnv(num_servers=4, server_workers=[1, 2, 2, 4], seed=3)
    assert one.get_server_workers() == [1, 2, 2, 4]
    one.reset()
    one.step(np.zeros(4, np.int64))
    one.set_server_workers([4, 1, 1, 1])
    assert one.get_server_workers() == [4, 1, 1, 1]
    with pytest.raises(ValueError):
        one.set_server_workers([1, 2])
    one.clear_server_workers()
    assert one.get_server_workers() == [1, 1, 1, 1]
    one.close()
    ma = VecMultiAgentLoadBalanceEnv(6, num_agents=2, servers_per_agent=2, server_workers=True)
    rows = 1 + (np.arange(24).reshape(6, 4) % 4)
    ma.set_server_workers(rows)
    np.testing.assert_array_equal(ma.get_server_workers().cpu().numpy(), rows)
    ma.reset()
    ma.set_server_workers([2, 2, 1, 1])
    np.testing.assert_array_equal(ma.get_server_workers().cpu().numpy(),
                                  np.tile([2, 2, 1, 1], (6, 1)))
    ma.clear_server_workers()
    assert (ma.get_server_workers() == 1).all()
    ma.vec.close()


@gpu
def test_error_paths(lib):
    import torch
    from marllb_amd import _lib
    from marllb_amd.env import VecLoadBalanceEnv
    for bad in (dict(lost_fin_prob=0.2), dict(duration_mode="service")):
        with pytest.raises(_lib.LbsimError) as e:
            VecLoadBalanceEnv(8, 4, device="cuda:0", server_workers=True, **bad)
        assert e.value.code == _lib.ENOTSUP
    late = VecLoadBalanceEnv(8, 4, device="cuda:0")
    with pytest.raises(ValueError):
        late.set_server_workers([1, 2, 1, 2])  # not enabled: EINVAL
    with pytest.raises(ValueError):
        late.get_server_workers()
    late.reset()
    with pytest.raises(ValueError):
        late.handle.enable_server_workers()  # after the first reset
    late.close()
    env = VecLoadBalanceEnv(8, 4, device="cuda:0", server_workers=True)
    assert (env.get_server_workers() == 1).all()
    env.set_server_workers([1, 64, 2, 3])
    before = env.get_server_workers().cpu().numpy().copy()
    np.testing.assert_array_equal(before, np.tile([1, 64, 2, 3], (8, 1)))
    three = torch.ones((3, 4), dtype=torch.int32, device="cuda:0")
    with pytest.raises(_lib.LbsimError) as e:  # rows neither 1 nor B
        env.handle.set_server_workers(three, rows=3)
    assert e.value.code == _lib.ESHAPE
    with pytest.raises(ValueError):
        env.set_server_workers(np.ones((3, 4), np.int64))
    rows = np.ones((8, 4), np.int64)
    rows[6, 2] = 65
    for bad in ([0, 1, 1, 1], [1, 1, 65, 1], [1, -3, 1, 1], [1, 1.5, 1, 1],
                [1, np.nan, 1, 1], [1, 1, 1, 2 ** 40], rows):
        with pytest.raises(ValueError):
            env.set_server_workers(bad)
        np.testing.assert_array_equal(env.get_server_workers().cpu().numpy(), before)
    env.reset()
    env.step(torch.zeros((8, 4), dtype=torch.int64))
    env.close()


# ---- theory

@pytest.fixture(scope="module")
def mmc_runs(lib):
    """One server of c workers at a per-worker utilisation of 0.7, at test_queueing_theory's run
    shape (4096 envs, flow statistics, no warm-up, Q = 64)."""
    out = {}
    for c in TH_C:
        lam = th_lam(c)
        r = qt.device_run(1, [1.0], th_burn(c), TH_REC[c], 9310 + c, assign_policy="lsq",
                          arrival_rate=lam, server_rates=[TH_MU], server_workers=[c])
        assert r.drops == 0 and r.count.sum() > 0.9 * qt.B * TH_REC[c] * lam * qt.DT
        out[c] = r
    return out


def mmc_checks(r, c, theory=None):
    lam = th_lam(c)
    w = mmc(c, TH_MU, lam) if theory is None else theory
    n_mean = r.in_flight.sum(1) / r.rec
    return [qt.Check(f"M/M/{c} mean sojourn time", *qt.server_mean(r, 0), w),
            qt.Check(f"M/M/{c} Little: mean column 0 against lambda W", n_mean.mean(),
                     n_mean.std(ddof=1) / math.sqrt(qt.B), lambda k: lam * w(k))]


@gpu
@pytest.mark.parametrize("c", TH_C)
def test_theory_mmc(mmc_runs, c):
    """The mean sojourn time is 1 / mu + C(c, lambda / mu) / (c mu - lambda) with Erlang C, and by
    Little's law the mean of column 0 is lambda times it.  Both fail with mu scaled by 1.03, and
    against M/M/1 at rate c mu: the workers are real."""
    checks = mmc_checks(mmc_runs[c], c)
    qt.assert_checks(checks)
    for chk in checks:
        assert not chk.ok(1.03), f"does not discriminate: {chk}"
    for chk in mmc_checks(mmc_runs[c], c, theory=qt.mm1(c * TH_MU, th_lam(c))):
        print(f"against M/M/1 at rate c mu: {chk}")
        assert not chk.ok(), f"one fast server would pass: {chk}"
