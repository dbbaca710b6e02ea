"""Hidden cross traffic: flows on the servers that the balancer cannot see.

The reference is tests/crosstraffic_ref.CrossSim, tests/flowsim_ref.FlowSim with §3.17 added from
its text.  The scenario, cases, actions and weights are tests/test_flowsim_ref.py's (reset, 6
steps, a masked reset of every third env, 6 steps); the shares are 0, 0.25, 0.5, 0.75 and 1 for
envs 0-4, then uniform in [0.2, 0.7]; the hidden weights alternate between uniform and skewed rows
with zero entries.

Not gpu: the reference at share 0 against plain FlowSim (which test_flowsim_ref pins to the
oracle), what the scenario reaches, the conversion rule of csrc/lbsim_cross.h compiled as host C++
under the address and undefined-behaviour sanitizers against the numpy rule, and the theory test's
sizes.  gpu: enabled handles against the reference exactly, share 0 against the unmodified oracle,
share 1, the interplay with the other per-env domains, and the closed forms of two superposed
Poisson streams.
"""
import math
import os
import subprocess

import numpy as np
import pytest

import oracle
from marllb_amd import build, flowstats
from marllb_amd.env import make_config
from tests import crosstraffic_ref as cr
from tests import parity, statelayout
from tests import test_flowsim_ref as fr
from tests import test_queueing_theory as qt
from tests.flowsim_ref import FlowSim
from tests.parity import lib  # noqa: F401  (the fixture: fails a gpu test run without a device)

HERE = os.path.dirname(os.path.abspath(__file__))
K = 128
CASES = fr.CASES
STEPS, RESET_AT = fr.STEPS, fr.RESET_AT
gpu = pytest.mark.gpu


# ------------------------------------------------------------------ the scenario's parameters

def cross_params(case, B, variant=0):
    """(share (B,), weights (B, S)) f32 of the case: shares 0, .25, .5, .75, 1 then uniform in
    [0.2, 0.7]; even rows uniform weights, odd rows skewed with zero entries."""
    S = CASES[case][0]
    rng = np.random.default_rng(4200 + 17 * list(CASES).index(case) + variant)
    share = np.concatenate([[0.0, 0.25, 0.5, 0.75, 1.0], rng.uniform(0.2, 0.7, B)])[:B]
    if variant:
        share = share[::-1].copy()
    w = np.ones((B, S), np.float32)
    for b in range(1 - variant % 2, B, 2):
        w[b] = rng.uniform(0.2, 4.0, S)
        w[b, rng.random(S) < 0.3] = 0.0
        if w[b].sum() == 0:
            w[b, b % S] = 1.0
    return share.astype(np.float32), w


_RUNS = {}
CHANGE_AT = 3  # variant "change": new shares and weights before step 3 (and they stay)


def reference_run(case, B, change=False):
    """The scenario on B CrossSim envs -> (cfg, kwargs, actions, events, (share, weights)[, the
    changed pair]).  Computed once per (case, B, change)."""
    key = (case, B, change)
    if key in _RUNS:
        return _RUNS[key]
    S, kw = fr.config_kwargs(case)
    cfg = make_config(B, S, **kw)
    share, w = cross_params(case, B)
    sims = [cr.CrossSim(kw["seed"], cfg.env_id_offset + b, S, cfg.queue_capacity,
                        kw.get("assign_policy", "sed"), cfg.arrival_rate,
                        [cfg.server_rate[s] for s in range(S)], dt=cfg.step_interval,
                        warmup_steps=cfg.warmup_steps, trace=kw.get("trace"),
                        share=share[b], weights=w[b]) for b in range(B)]
    drops = np.zeros(B, np.int64)
    tot = {"hidden_assigned": np.zeros(B, np.int64), "hidden_dropped": np.zeros(B, np.int64),
           "hidden_in_step": np.zeros(B, np.int64), "hidden_carried": np.zeros(B, np.int64),
           "visible_done": np.zeros(B, np.int64)}
    acts = fr.actions_of(case, B)
    events = []

    def account(b, r):
        tot["hidden_assigned"][b] += int(r.hidden_assigned.sum())
        tot["hidden_dropped"][b] += r.hidden_dropped
        tot["hidden_in_step"][b] += sum(1 for e in r.hidden_completed if e[2])
        tot["hidden_carried"][b] += sum(1 for e in r.hidden_completed if not e[2])
        tot["visible_done"][b] += len(r.completed)

    def snapshot(ev):
        ev.dropped = drops.copy()
        ev.in_flight = np.array([m.in_flight() for m in sims])
        ev.hidden = np.array([m.hidden_in_flight() for m in sims])
        ev.arr_idx = np.array([m.k for m in sims])
        ev.next_abs = np.array([m.next_arrival() for m in sims])
        ev.steps = np.array([m.step_no for m in sims])
        events.append(ev)

    def reset(mask):
        ev = fr.Event(B, S)
        ev.mask = mask
        for b in np.flatnonzero(mask):
            drops[b] = 0
            for r in sims[b].reset():
                drops[b] += r.dropped
                account(b, r)
                for s in range(S):
                    ev.new[b][s][0].extend(r.fct(s))
                    ev.new[b][s][1].extend(r.tc(s))
        snapshot(ev)

    changed = cross_params(case, B, variant=1)
    reset(np.ones(B, bool))
    for k in range(STEPS):
        if k == RESET_AT:
            reset(np.arange(B) % 3 == 0)
        if change and k == CHANGE_AT:
            for b in range(B):
                sims[b].set_cross(changed[0][b], changed[1][b])
        wts = fr.weights_of(acts[k], kw)
        ev = fr.Event(B, S)
        for b in range(B):
            r = sims[b].step(wts[b])
            account(b, r)
            ev.assigned[b] = r.assigned
            drops[b] += r.dropped
            ev.new[b] = [(r.fct(s), r.tc(s)) for s in range(S)]
        snapshot(ev)
    events[-1].totals = tot
    _RUNS[key] = (cfg, kw, acts, events, (share, w), changed)
    return _RUNS[key]


def drive(case, B, backend, check, change=False):
    """The scenario on `backend`: check(event, outputs) after every reset and step."""
    _, _, acts, events, _, changed = reference_run(case, B, change)
    it = iter(events)
    check(next(it), backend.reset(None))
    for k in range(STEPS):
        if k == RESET_AT:
            check(next(it), backend.reset((np.arange(B) % 3 == 0).astype(np.uint8)))
        if change and k == CHANGE_AT:
            backend.set_cross(*changed)
        check(next(it), backend.step(acts[k]))
    return events


# ------------------------------------------------------------------ not gpu: the reference

HOST_B = 12


@pytest.mark.parametrize("case", list(CASES))
def test_reference_at_share_zero_equals_flowsim(case):
    """CrossSim with share 0 (and skewed hidden weights) is FlowSim event for event; through
    test_flowsim_ref's OracleBackend test that is the oracle."""
    S, kw = fr.config_kwargs(case)
    cfg = make_config(4, S, **kw)
    acts = fr.actions_of(case, 4)
    _, w = cross_params(case, 4)
    for b in range(4):
        args = (kw["seed"], cfg.env_id_offset + b, S, cfg.queue_capacity,
                kw.get("assign_policy", "sed"), cfg.arrival_rate,
                [cfg.server_rate[s] for s in range(S)])
        opt = dict(dt=cfg.step_interval, warmup_steps=cfg.warmup_steps, trace=kw.get("trace"))
        plain, cross = FlowSim(*args, **opt), cr.CrossSim(*args, share=0.0, weights=w[b], **opt)

        def same(ra, rb):
            np.testing.assert_array_equal(ra.assigned, rb.assigned)
            assert ra.dropped == rb.dropped and ra.completed == rb.completed
            assert rb.hidden_assigned.sum() == 0 and not rb.hidden_completed
            assert plain.in_flight() == cross.in_flight() and plain.k == cross.k
            assert plain.next_arrival() == cross.next_arrival()

        for ra, rb in zip(plain.reset(), cross.reset()):
            same(ra, rb)
        for k in range(STEPS):
            if k == RESET_AT and b % 3 == 0:
                for ra, rb in zip(plain.reset(), cross.reset()):
                    same(ra, rb)
            wt = fr.weights_of(acts[k], kw)[b]
            same(plain.step(wt), cross.step(wt))


# The drop cases whose drops come from full queues: a hidden flow is dropped only at a full (or
# down) server.  s4-alias-zero-level's drops come from all-zero visible weights, which a hidden
# flow ignores.
HIDDEN_DROPS = ("s1-q3-drops", "s3-lsq-q6-overload", "s6-alias-continuous")
# envs of the not-gpu reach test: s6-alias-continuous (Q = 32, load 0.8) fills a queue only where
# a skewed row of hidden weights piles the hidden flows on one server, in none of its first 12 envs
# and in several of 67
REACH_B = {"s6-alias-continuous": 67}


def check_reaches(case, B):
    """The scenario is not vacuous (asserted on the reference alone)."""
    _, _, _, events, (share, _), _ = reference_run(case, B)
    S, reach = CASES[case][0], CASES[case][2]
    count = np.zeros((B, S), np.int64)
    peak = 0
    for ev in events:
        if ev.mask is not None:
            count[ev.mask] = 0
        count += np.array([[len(ev.new[b][s][0]) for s in range(S)] for b in range(B)])
        peak = max(peak, int(count.max()))
    assert peak <= K, "a reservoir wrapped: its records no longer list every visible flow"
    tot = events[-1].totals
    mid = (share > 0) & (share < 1)
    assert mid.sum() >= B - 3
    assert (tot["visible_done"][mid] > 0).all() and (tot["hidden_assigned"][mid] > 0).all()
    assert tot["hidden_assigned"][share == 0].sum() == 0
    assert tot["visible_done"][share == 1].sum() == 0
    assert tot["hidden_in_step"].sum() > 0 and tot["hidden_carried"].sum() > 0
    if case in HIDDEN_DROPS:
        assert tot["hidden_dropped"].sum() > 0
    assert any(ev.mask is not None and not ev.mask.all() for ev in events)
    return peak, tot


@pytest.mark.parametrize("case", list(CASES))
def test_scenario_reaches(case):
    peak, tot = check_reaches(case, REACH_B.get(case, HOST_B))
    print(f"REACH {case}: peak reservoir count {peak}, visible completions per env "
          f"{tot['visible_done'].tolist()}, hidden drops {int(tot['hidden_dropped'].sum())}")


# ------------------------------------------------------------------ not gpu: the conversion rule

@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/cross_probe.cpp, the rule of csrc/lbsim_cross.h as a host program built with the
    address and undefined-behaviour sanitizers: probe(lines) -> its output lines."""
    exe = str(tmp_path_factory.mktemp("cross") / "cross_probe")
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "cross_probe.cpp")], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


def bits(x):
    return [int(v) for v in np.asarray(x, np.float32).reshape(-1).view(np.uint32)]


def test_threshold_rule(probe):
    shares = np.array([0.0, 1.0, 1e-45, 1e-39, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), 1),
                       2.0 ** -24, 0.25, 0.5, 0.3, 0.7, np.nextafter(np.float32(1), 0), -0.0],
                      np.float32)
    bad = np.array([np.nan, -1e-45, np.nextafter(np.float32(1), 2), np.inf, -np.inf, -1.0],
                   np.float32)
    out = probe([f"thr {b}" for b in bits(shares)] + [f"thr {b}" for b in bits(bad)])
    for sh, line in zip(shares, out):
        assert line.split() == ["1", str(cr.threshold(sh))], (sh, line)
    assert cr.threshold(0.0) == 0 and cr.threshold(1.0) == cr.ONE and cr.threshold(1e-45) == 0
    for line in out[len(shares):]:
        assert line.split()[0] == "0"


def test_edges_rule_every_width(probe):
    rng = np.random.default_rng(77)
    rows = []
    for S in range(1, 65):
        rows.append(rng.uniform(0.0, 5.0, S).astype(np.float32))
        z = rng.uniform(0.0, 5.0, S).astype(np.float32)
        z[rng.random(S) < 0.4] = 0.0
        z[rng.integers(S)] = np.float32(1e-30) if S % 2 else np.float32(3e38)
        rows.append(z)
        rows.append((10.0 ** rng.uniform(-30, 30, S)).astype(np.float32))
    out = probe([f"edges {len(w)} " + " ".join(map(str, bits(w))) for w in rows])
    for w, line in zip(rows, out):
        got = [int(x) for x in line.split()]
        assert got[0] == 1, w
        want = cr.edges(w, len(w))
        assert got[1:] == want.tolist(), w
        assert got[-1] == cr.ONE and (np.diff(want) >= 0).all()
    uni = probe([f"uniform {S}" for S in range(1, 65)])
    for S, line in zip(range(1, 65), uni):
        assert [int(x) for x in line.split()] == cr.edges(None, S).tolist()
    bad = [[0.0, 0.0, 0.0], [1.0, -1e-45, 1.0], [1.0, np.nan], [np.inf, 1.0], [-0.0]]
    for w, line in zip(bad, probe([f"edges {len(w)} " + " ".join(map(str, bits(w))) for w in bad])):
        assert line.split()[0] == "0", w


def test_pick_at_every_24_bit_word(probe):
    """One table with zero weights (equal edges) and a denormal one: cross_pick of all 2^24 words
    against numpy's count of the edges at or below the word."""
    w = np.array([3.0, 0.0, 1.0, 1e-40, 0.0, 2.5, 0.0], np.float32)
    cum = cr.edges(w, len(w))
    line = probe([f"sweep {len(w)} " + " ".join(map(str, cum.tolist()))])[0].split()
    want = np.searchsorted(cum, np.arange(cr.ONE, dtype=np.int64), side="right")
    assert want.max() < len(w)  # cum[S-1] = 2^24 is above every word
    at = np.flatnonzero(np.diff(want)) + 1
    runs = [int(want[0])] + [v for x in at for v in (int(x), int(want[x]))]
    assert [int(v) for v in line] == runs
    # the servers of weight 0 (the last one included) and the denormal one are never picked
    assert set(want.tolist()) == {0, 2, 5}


def test_hash_rule(probe):
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 2 ** 32, (200, 6), dtype=np.uint64)
    rows[:, 5] %= cr.ONE + 1
    out = probe(["hash " + " ".join(map(str, r.tolist())) for r in rows])
    for r, line in zip(rows.tolist(), out):
        k0, k1, gid, ep, k, thr = r
        slt = cr.salt((k0, k1), gid, ep)
        h = cr.mix(k ^ slt ^ 0x3C6EF372)
        assert [int(v) for v in line.split()] == [slt, h, int((h >> 8) < thr),
                                                  cr.mix(h ^ 0x6A09E667) >> 8]


def test_sampler_and_abi():
    """sample_cross_traffic: shares inside their range, each row of weights a permutation of a
    geometric ladder with ratio in `skew`, deterministic for a seeded generator; the four entry
    points are declared in include/lbsim.h and bound in _lib."""
    import torch
    from marllb_amd import _lib, sample_cross_traffic
    g = torch.Generator().manual_seed(3)
    share, w = sample_cross_traffic(500, 6, share=(0.1, 0.6), skew=(1.0, 3.0), generator=g)
    assert share.shape == (500,) and w.shape == (500, 6) and w.dtype == torch.float32
    assert 0.1 <= float(share.min()) and float(share.max()) <= 0.6
    assert float(share.max()) - float(share.min()) > 0.4
    srt = w.double().sort(dim=1, descending=True).values
    ratio = srt[:, :-1] / srt[:, 1:]
    assert torch.allclose(ratio, ratio[:, :1].expand_as(ratio), rtol=1e-5)
    assert 1.0 <= float(ratio.min()) and float(ratio.max()) <= 3.0 * (1 + 1e-5)
    assert (srt[:, 0] == 1.0).all() and len({tuple(r) for r in w.argsort(dim=1).tolist()}) > 100
    s2, w2 = sample_cross_traffic(500, 6, share=(0.1, 0.6), skew=(1.0, 3.0),
                                  generator=torch.Generator().manual_seed(3))
    assert torch.equal(share, s2) and torch.equal(w, w2)
    for bad in (dict(share=(-0.1, 0.5)), dict(share=(0.2, 1.5)), dict(share=(0.6, 0.2)),
                dict(skew=(0.5, 2.0)), dict(skew=(3.0, 2.0))):
        with pytest.raises(ValueError):
            sample_cross_traffic(4, 4, **bad)
    header = open(os.path.join(os.path.dirname(HERE), "include", "lbsim.h")).read()
    for name, nargs in (("lbsim_cross_traffic_enable", 1), ("lbsim_set_cross_traffic", 5),
                        ("lbsim_get_cross_traffic", 4), ("lbsim_clear_cross_traffic", 2)):
        assert f"int {name}(" in header
        assert len(_lib._SIGNATURES[name][1]) == nargs
    assert "#define LBSIM_ABI_VERSION 10 " in header


# ------------------------------------------------------------------ theory: sizes on the reference

TH_A, TH_C, TH_P = [1.0, 2.0, 3.0, 4.0], [2.0, 3.0, 3.0, 2.0], 0.5
TH_MU, TH_LAM, TH_REC = [12.5, 25.0, 37.5, 50.0], 50.0, 200


def theory_rates():
    """Per server: (total arrival rate, visible arrival rate)."""
    tot = [TH_LAM * ((1 - TH_P) * a / sum(TH_A) + TH_P * c / sum(TH_C))
           for a, c in zip(TH_A, TH_C)]
    vis = [TH_LAM * (1 - TH_P) * a / sum(TH_A) for a in TH_A]
    return tot, vis


def theory_burn():
    tot, _ = theory_rates()
    return qt.burn_steps(max(qt.relaxation(m, l) for m, l in zip(TH_MU, tot)))


def test_theory_sizes_on_the_reference():
    """The reference alone, at reduced size, meets the superposition's closed forms, and
    1 / sqrt(n) scaling of its standard errors puts the device run under the cap."""
    envs, rec = 64, 40
    tot, vis = theory_rates()
    assert all(l < 0.8 * m for l, m in zip(tot, TH_MU))
    count, sum_us = np.zeros((envs, 4)), np.zeros((envs, 4))
    for b in range(envs):
        sim = cr.CrossSim(9201, b, 4, qt.Q, "alias", TH_LAM, TH_MU, dt=qt.DT, warmup_steps=0,
                          share=TH_P, weights=TH_C)
        sim.reset()
        for _ in range(theory_burn()):
            sim.step(TH_A)
        for _ in range(rec):
            for s, ta, tc in sim.step(TH_A).completed:
                count[b, s] += 1
                sum_us[b, s] += tc - ta
    for s in range(4):
        est, se = qt.ratio(sum_us[:, s] * 1e-6, count[:, s])
        c = qt.Check(f"reference cross-traffic mean, server {s}", est, se, qt.mm1(TH_MU[s], tot[s]))
        print(c)
        assert c.ok()
        assert se * math.sqrt(envs * rec / (qt.B * TH_REC)) <= qt.CAP * c.theory(1.0)
        rate, rse = qt.ratio(count[:, s], np.full(envs, rec * qt.DT))
        assert abs(rate - vis[s]) <= qt.NSE * rse + qt.SLACK * vis[s]


# ------------------------------------------------------------------ the device

GPU_B = fr.GPU_B


def cross_state(env):
    """The state of an enabled handle: the lost_on section at the position a leak handle has it."""
    c = env.cfg
    return statelayout.parse(env.handle.state_bytes(), c.num_envs, c.num_servers, c.queue_capacity,
                             bool(c.normalize_obs), c.fail_prob > 0 or env.server_availability,
                             leak=True, dur_plane=statelayout.has_dur_plane(c))


class DeviceBackend:
    """reset / step -> (obs, reward or None, assign counts or None), numpy."""

    def __init__(self, B, S, kw, cross=None, **extra):
        import torch
        from marllb_amd.env import VecLoadBalanceEnv
        self.torch = torch
        self.env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=False, **extra, **kw)
        if cross is not None:
            self.set_cross(*cross)

    def set_cross(self, share, w):
        self.env.set_cross_traffic(share, w)

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


class CrossCheck:
    """An Event of the reference against an enabled handle's state and outputs."""

    def __init__(self, env, stats=False):
        self.env, self.cfg = env, env.cfg
        self.B, self.S = env.cfg.num_envs, env.cfg.num_servers
        self.dt = int(round(env.cfg.step_interval * 1e6))
        self.count = np.zeros((self.B, self.S), np.int64)
        self.stats = stats
        self.fs = [np.zeros((self.B, self.S), np.uint32), np.zeros((self.B, self.S), np.uint64),
                   np.zeros((self.B, self.S), np.uint32),
                   np.zeros((self.B, self.S, flowstats.NBINS), np.uint32)]

    def __call__(self, ev, out):
        B, S = self.B, self.S
        obs, rew, assign = out
        d = cross_state(self.env)
        if assign is not None:
            np.testing.assert_array_equal(assign, ev.assigned, err_msg="assign_counts")
        np.testing.assert_array_equal(d["dropped"], ev.dropped, err_msg="dropped")
        np.testing.assert_array_equal(d["arr_idx"], ev.arr_idx, err_msg="arrival index")
        np.testing.assert_array_equal(d["clock"], ev.steps, err_msg="clock")
        np.testing.assert_array_equal(d["next_arr"].astype(np.int64) + ev.steps * self.dt,
                                      ev.next_abs, err_msg="next arrival")
        queued = (d["hc"].reshape(B, S) >> 16).astype(np.int64)
        np.testing.assert_array_equal(queued, ev.in_flight + ev.hidden, err_msg="hc count")
        np.testing.assert_array_equal(d["lost_on"].view(np.int32).reshape(B, S), -ev.hidden,
                                      err_msg="lost_on")
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
        check_features(self.env, d, obs, rew, "cross-traffic handle")
        if self.stats:
            self.check_stats(ev, assign is not None)

    def check_stats(self, ev, is_step):
        """count / sum / maximum / histogram of the visible flows completed by the steps."""
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


def default_handle_first(S, kw, mapping, acts):
    """The features / reward comparison on a default handle, so a mismatch on the enabled one is
    the cross traffic's."""
    back = DeviceBackend(GPU_B, S, kw, dyn_mapping=mapping)
    obs, _, _ = back.reset(None)
    d = statelayout.parse_cfg(back.env.handle.state_bytes(), back.env.cfg)
    check_features(back.env, d, obs, None, "default handle")
    for a in acts[:2]:
        obs, rew, _ = back.step(a)
        d = statelayout.parse_cfg(back.env.handle.state_bytes(), back.env.cfg)
        check_features(back.env, d, obs, rew, "default handle")
    back.env.close()


MAPPED = [(c, m) for c in CASES for m in ("auto", "env", "server")
          if m != "env" or CASES[c][0] <= 16]


@gpu
@pytest.mark.parametrize("case,mapping", MAPPED)
def test_enabled_handles_equal_the_reference(lib, case, mapping):
    S, kw = fr.config_kwargs(case)
    _, _, acts, _, cross, _ = reference_run(case, GPU_B)
    if mapping == "auto":
        default_handle_first(S, kw, mapping, acts)
    back = DeviceBackend(GPU_B, S, kw, cross=cross, cross_traffic=True, dyn_mapping=mapping)
    drive(case, GPU_B, back, CrossCheck(back.env))
    check_full_kernel(lib, back.env)
    check_reaches(case, GPU_B)
    back.env.close()


@gpu
def test_forced_four_lane_groups():
    """LBSIM_DYN_GROUP_LANES=4: the headline shape's 4-lane full kernel on the S <= 4 cases."""
    ks = [f"test_enabled_handles_equal_the_reference[{c}-auto]" for c, v in CASES.items()
          if v[0] <= 4]
    assert len(ks) >= 6
    parity.run_cases_in_child("test_cross_traffic.py", ks, {"LBSIM_DYN_GROUP_LANES": "4"})


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_flow_statistics_count_the_visible_flows(lib, case):
    S, kw = fr.config_kwargs(case)
    cross = reference_run(case, GPU_B)[4]
    back = DeviceBackend(GPU_B, S, kw, cross=cross, cross_traffic=True, flow_stats=True)
    chk = CrossCheck(back.env, stats=True)
    drive(case, GPU_B, back, chk)
    assert int(chk.fs[0].sum()) > 5 * GPU_B
    back.env.close()


@gpu
@pytest.mark.parametrize("case", ["s4-sed-levels", "s3-lsq-q6-overload", "s6-alias-continuous",
                                  "s8-trace37", "s4-q64-deep"])
def test_mid_run_change(lib, case):
    """New shares and weights before step 3: arrivals assigned from that launch on follow them,
    and the flows already queued keep their flag (the reference's queues say which)."""
    S, kw = fr.config_kwargs(case)
    cross = reference_run(case, GPU_B, change=True)[4]
    back = DeviceBackend(GPU_B, S, kw, cross=cross, cross_traffic=True)
    drive(case, GPU_B, back, CrossCheck(back.env), change=True)
    back.env.close()


# ---- share 0 on an enabled handle: the unmodified oracle

def _parity_configs():
    from tests.test_gpu_parity import CONFIGS
    return [i for i, c in enumerate(CONFIGS) if "lost_fin_prob" not in c["kw"]]


@gpu
@pytest.mark.parametrize("idx", _parity_configs())
def test_share_zero_equals_the_oracle(lib, oracle_mod, idx):
    """An enabled handle whose shares are all 0 (hidden weights skewed): every output and every
    state section equal the oracle's, and lost_on stays zero."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    from tests.test_gpu_parity import CONFIGS, resolve_kw
    c = CONFIGS[idx]
    B, S, kw = c["B"], c["S"], resolve_kw(c["kw"])
    kw.setdefault("seed", 1000 + idx)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=False, cross_traffic=True, **kw)
    env.set_cross_traffic(0.0, np.arange(1, S + 1, dtype=np.float32))
    ora = oracle_mod.OracleEnv(make_config(B, S, **kw), threads=4, trace=kw.get("trace"))

    def same_state():
        g = cross_state(env)
        o = statelayout.parse_cfg(ora.state_bytes(), env.cfg)
        assert not g["lost_on"].any()
        g["ring"] = statelayout.live_ring(g, B, S, env.cfg.queue_capacity)
        o["ring"] = statelayout.live_ring(o, B, S, env.cfg.queue_capacity)
        assert set(g) == set(o) | {"lost_on"}
        for name in o:
            np.testing.assert_array_equal(g[name], o[name], err_msg=name)

    np.testing.assert_array_equal(env.reset().cpu().numpy(), ora.reset())
    rng = np.random.default_rng(idx)
    for k in range(8):
        parity.step_both(env, ora, parity.actions(rng, B, S, dict(c["kw"]), levels=True), k)
    same_state()
    mask = (np.arange(B) % 3 == 0).astype(np.uint8)
    og = env.reset(mask=torch.from_numpy(mask)).cpu().numpy()
    np.testing.assert_array_equal(og, ora.reset(mask=mask, obs=og.copy()))
    for k in range(4):
        parity.step_both(env, ora, parity.actions(rng, B, S, dict(c["kw"]), levels=True), 8 + k)
    same_state()
    check_full_kernel(lib, env)
    ora.close()
    env.close()


# ---- share 1

@gpu
@pytest.mark.parametrize("case", ["s4-sed-levels", "s1-q3-drops", "s6-alias-continuous"])
def test_share_one(lib, case):
    """Every arrival hidden: zero observation rows, no assignments, empty reservoirs; the queues
    and drops are what the reference says."""
    S, kw = fr.config_kwargs(case)
    cfg = make_config(GPU_B, S, **kw)
    B = 16
    _, w = cross_params(case, B)
    back = DeviceBackend(B, S, kw, cross=(1.0, w), cross_traffic=True)
    sims = [cr.CrossSim(kw["seed"], cfg.env_id_offset + b, S, cfg.queue_capacity,
                        kw.get("assign_policy", "sed"), cfg.arrival_rate,
                        [cfg.server_rate[s] for s in range(S)], dt=cfg.step_interval,
                        warmup_steps=cfg.warmup_steps, share=1.0, weights=w[b]) for b in range(B)]
    drops = np.array([sum(r.dropped for r in m.reset()) for m in sims])
    obs, _, _ = back.reset(None)
    acts = fr.actions_of(case, B)
    for k in range(6):
        d = cross_state(back.env)
        assert not obs.any() and not d["res_count"].any()
        np.testing.assert_array_equal(d["dropped"], drops)
        hid = np.array([m.hidden_in_flight() for m in sims])
        np.testing.assert_array_equal((d["hc"].reshape(B, S) >> 16), hid)
        np.testing.assert_array_equal(d["lost_on"].view(np.int32).reshape(B, S), -hid)
        wts = fr.weights_of(acts[k], kw)
        obs, rew, assign = back.step(acts[k])
        assert not assign.any()
        drops += np.array([m.step(wts[b]).dropped for b, m in enumerate(sims)])
    assert hid.sum() > 0
    if "drops" in CASES[case][2]:
        assert drops.sum() > 0
    back.env.close()


# ---- interplay

def small_pair(case="s4-sed-levels", B=24, **extra):
    """An enabled env of B envs with the case's config and its reference sims (shares and weights
    of cross_params)."""
    S, kw = fr.config_kwargs(case)
    share, w = cross_params(case, B)
    back = DeviceBackend(B, S, kw, cross=(share, w), cross_traffic=True, **extra)
    return back, S, kw, share, w


def hidden_queued(env):
    d = cross_state(env)
    B, S = env.cfg.num_envs, env.cfg.num_servers
    return d, -d["lost_on"].view(np.int32).reshape(B, S).astype(np.int64)


def ring_flags(env, d):
    """Per server, the number of live ring entries that carry the hidden flag."""
    B, S, Q = env.cfg.num_envs, env.cfg.num_servers, env.cfg.queue_capacity
    hc = d["hc"].reshape(B, S)
    ring = d["ring"].reshape(B, S, Q, 2)
    out = np.zeros((B, S), np.int64)
    for b in range(B):
        for s in range(S):
            h, c = int(hc[b, s] & 0x7FFF), int(hc[b, s] >> 16)
            out[b, s] = sum(ring[b, s, (h + i) % Q, 1] == np.iinfo(np.int32).min for i in range(c))
    return out


@gpu
def test_flags_and_counter_travel_together(lib):
    """In every state, lost_on is minus the number of flagged ring entries -- after steps, after
    a snapshot / restore into another env and a fork (identity, no reference needed)."""
    import torch
    back, S, kw, share, w = small_pair("s3-lsq-q6-overload", 24)
    env = back.env
    back.reset(None)
    acts = fr.actions_of("s3-lsq-q6-overload", 24)
    for k in range(4):
        back.step(acts[k])
        d, hid = hidden_queued(env)
        np.testing.assert_array_equal(ring_flags(env, d), hid)
    assert hid.sum() > 0
    snap = env.snapshot()
    before = env.handle.state_bytes()
    for k in range(4, 7):
        back.step(acts[k])
    env.restore(snap)
    assert env.handle.state_bytes() == before
    d, hid = hidden_queued(env)
    np.testing.assert_array_equal(ring_flags(env, d), hid)
    # a fork: every env takes the saved state of the env with the most hidden flows queued
    src = int(hid.sum(1).argmax())
    env.restore(snap, src=torch.full((24,), src, dtype=torch.int32))
    d, forked = hidden_queued(env)
    np.testing.assert_array_equal(forked, np.tile(hid[src], (24, 1)))
    np.testing.assert_array_equal(ring_flags(env, d), forked)
    env.restore(snap)
    # the restored envs step as the reference says envs stepped without the detour do
    twin = DeviceBackend(24, S, kw, cross=(share, w), cross_traffic=True)
    twin.reset(None)
    for k in range(4):
        twin.step(acts[k])
    for k in range(4, 8):
        a, b = back.step(acts[k]), twin.step(acts[k])
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    assert env.handle.state_bytes() == twin.env.handle.state_bytes()
    twin.env.close()
    env.close()


@gpu
def test_failure_and_outage_drop_hidden_flows(lib):
    """A scripted outage of every server with hidden flows queued: lost_on back to 0 and dropped
    grows by the whole queue, hidden flows included."""
    case = "s4-q64-deep"
    back, S, kw, share, w = small_pair(case, 24, server_availability=True)
    env = back.env
    back.reset(None)
    acts = fr.actions_of(case, 24)
    for k in range(3):
        back.step(acts[k])
    d0, hid = hidden_queued(env)
    assert hid.sum() > 0
    queued = (d0["hc"].reshape(24, S) >> 16).astype(np.int64)
    env.set_server_availability(np.zeros((1, S), np.uint8))
    obs, _, assign = back.step(acts[3])
    d1, hid1 = hidden_queued(env)
    assert not hid1.any() and not (d1["hc"] >> 16).any() and not assign.any()
    arrivals = d1["arr_idx"].astype(np.int64) - d0["arr_idx"].astype(np.int64)
    np.testing.assert_array_equal(d1["dropped"].astype(np.int64) - d0["dropped"].astype(np.int64),
                                  queued.sum(1) + arrivals)
    env.close()


@gpu
def test_failure_of_every_server_drops_hidden_flows(lib):
    """fail_prob = 1 and recover_prob = 1: every server alternates down and up, so the reset's two
    warm-up steps leave the servers up with flows queued, hidden ones among them, and the first
    step fails all of them: lost_on back to 0, the queues empty, and dropped grows by the whole
    queue, visible and hidden, plus the step's arrivals (no server takes a flow)."""
    case, B = "s4-q64-deep", 24
    S, kw = fr.config_kwargs(case)
    assert kw["warmup_steps"] == 2
    share, w = cross_params(case, B)
    back = DeviceBackend(B, S, {**kw, "fail_prob": 1.0, "recover_prob": 1.0}, cross=(share, w),
                         cross_traffic=True)
    back.reset(None)
    acts = fr.actions_of(case, B)
    for k in range(0, 4, 2):  # a failing step, then a step with every server back up
        d0, hid0 = hidden_queued(back.env)
        assert not d0["down"].any()
        queued = (d0["hc"].reshape(B, S) >> 16).astype(np.int64)
        assert hid0.sum() > 0 and (queued - hid0).sum() > 0  # hidden and visible flows queued
        _, _, assign = back.step(acts[k])
        d1, hid1 = hidden_queued(back.env)
        assert d1["down"].all() and not hid1.any() and not (d1["hc"] >> 16).any()
        assert not assign.any() and not d1["res_count"].any()
        arrivals = d1["arr_idx"].astype(np.int64) - d0["arr_idx"].astype(np.int64)
        assert (arrivals > 0).all()
        np.testing.assert_array_equal(
            d1["dropped"].astype(np.int64) - d0["dropped"].astype(np.int64),
            queued.sum(1) + arrivals)
        back.step(acts[k + 1])  # every server recovers at the step's start and takes flows
    back.env.close()


@gpu
def test_one_server_outage_against_the_reference(lib):
    """Server 1 of every env scripted down for one step, the others up: its queue, hidden flows
    included, is dropped; a hidden flow aimed at it is dropped while the pick still counts every
    edge, so the hidden flows of the other servers go where the reference says.  The reference
    has no down servers: for that step its server 1 is emptied (its flows dropped) and filled
    with Q flows that never complete, which makes it ineligible for visible and hidden flows
    alike, as a down server is."""
    case, B, J = "s4-sed-levels", 24, 1
    back, S, kw, share, w = small_pair(case, B, server_availability=True)
    env, Q = back.env, back.env.cfg.queue_capacity
    sims = reference_sims(case, B, share, w)
    drops = np.array([sum(r.dropped for r in m.reset()) for m in sims])
    back.reset(None)
    acts = fr.actions_of(case, B)

    def both_step(k):
        nonlocal drops
        wts = fr.weights_of(acts[k], kw)
        _, _, assign = back.step(acts[k])
        rs = [m.step(wts[b]) for b, m in enumerate(sims)]
        drops = drops + np.array([r.dropped for r in rs])
        np.testing.assert_array_equal(assign, np.array([r.assigned for r in rs]))
        return rs

    for k in range(3):
        both_step(k)
    assert_matches_sims(env, sims, drops)
    lost_hidden = sum(sum(1 for e in m.queues[J] if e[2]) for m in sims)
    assert lost_hidden > 0  # hidden flows are queued at the server that goes down
    up = np.ones((1, S), np.uint8)
    up[0, J] = 0
    env.set_server_availability(up)
    never = 1 << 60
    for b, m in enumerate(sims):
        drops[b] += len(m.queues[J])
        m.queues[J] = [(never, 0, False, -1)] * Q
    rs = both_step(3)
    assert sum(r.hidden_dropped for r in rs) > 0  # hidden flows aimed at the down server
    assert sum(int(r.hidden_assigned.sum()) for r in rs) > 0  # and others queued elsewhere
    for m in sims:
        assert len(m.queues[J]) == Q
        m.queues[J] = []
    assert_matches_sims(env, sims, drops)
    d = cross_state(env)
    assert (d["down"].reshape(B, S)[:, J] != 0).all() and d["down"].sum() == B
    env.set_server_availability(np.ones((1, S), np.uint8))
    for k in range(4, 7):  # the server is back: both go on alike
        both_step(k)
    assert_matches_sims(env, sims, drops)
    env.close()


@gpu
def test_random_failures_keep_counter_and_flags_together(lib):
    """fail_prob > 0: a failing server loses its hidden flows with its queue, so lost_on stays
    minus the number of flagged ring entries in every state (identity)."""
    S, kw = fr.config_kwargs("s4-q64-deep")
    share, w = cross_params("s4-q64-deep", 24)
    back = DeviceBackend(24, S, {**kw, "fail_prob": 0.3, "recover_prob": 0.5}, cross=(share, w),
                         cross_traffic=True)
    back.reset(None)
    acts = fr.actions_of("s4-q64-deep", 24)
    seen_down = seen_hidden = 0
    for k in range(8):
        back.step(acts[k])
        d, hid = hidden_queued(back.env)
        np.testing.assert_array_equal(ring_flags(back.env, d), hid)
        assert not hid[d["down"].reshape(24, S) != 0].any()
        seen_down += int((d["down"] != 0).sum())
        seen_hidden += int(hid.sum())
    assert seen_down > 0 and seen_hidden > 0
    back.env.close()


def reference_sims(case, B, share, w, rates=None):
    S, kw = fr.config_kwargs(case)
    cfg = make_config(B, S, **kw)
    out = []
    for b in range(B):
        lam = cfg.arrival_rate if rates is None else rates[0][b]
        mus = [cfg.server_rate[s] for s in range(S)] if rates is None else list(rates[1][b])
        out.append(cr.CrossSim(kw["seed"], cfg.env_id_offset + b, S, cfg.queue_capacity,
                               kw.get("assign_policy", "sed"), lam, mus, dt=cfg.step_interval,
                               warmup_steps=cfg.warmup_steps, share=share[b], weights=w[b]))
    return out


def assert_matches_sims(env, sims, drops):
    B, S = env.cfg.num_envs, env.cfg.num_servers
    d, hid = hidden_queued(env)
    np.testing.assert_array_equal(hid, np.array([m.hidden_in_flight() for m in sims]))
    np.testing.assert_array_equal((d["hc"].reshape(B, S) >> 16) - hid,
                                  np.array([m.in_flight() for m in sims]))
    np.testing.assert_array_equal(d["arr_idx"], np.array([m.k for m in sims]))
    np.testing.assert_array_equal(d["dropped"], drops)


@gpu
def test_per_env_rates(lib):
    """Per-env arrival and server rates under cross traffic, against the reference."""
    case, B = "s4-sed-levels", 24
    back, S, kw, share, w = small_pair(case, B)
    rng = np.random.default_rng(9)
    lam = rng.uniform(30.0, 120.0, B).astype(np.float32)
    mus = rng.uniform(10.0, 60.0, (B, S)).astype(np.float32)
    back.env.set_rates(lam, mus)
    sims = reference_sims(case, B, share, w, rates=(lam, mus))
    drops = np.array([sum(r.dropped for r in m.reset()) for m in sims])
    back.reset(None)
    acts = fr.actions_of(case, B)
    for k in range(5):
        assert_matches_sims(back.env, sims, drops)
        wts = fr.weights_of(acts[k], kw)
        _, _, assign = back.step(acts[k])
        rs = [m.step(wts[b]) for b, m in enumerate(sims)]
        drops += np.array([r.dropped for r in rs])
        np.testing.assert_array_equal(assign, np.array([r.assigned for r in rs]))
    assert_matches_sims(back.env, sims, drops)
    back.env.close()


@gpu
def test_server_rate_schedule(lib):
    """A per-env server-rate schedule (3 phases of 2 steps, cyclic) under cross traffic: a flow's
    service time uses the rates of the phase it is assigned in, hidden or not; the reset and its
    warm-up run at phase 0.  Against the reference, whose svc_scale follows the phase."""
    case, B, P, H = "s4-sed-levels", 24, 3, 2
    back, S, kw, share, w = small_pair(case, B)
    rng = np.random.default_rng(11)
    mus = rng.uniform(10.0, 60.0, (B, P, S)).astype(np.float32)
    back.env.set_rate_schedule(None, mus, steps_per_phase=H, wrap=True)
    sims = reference_sims(case, B, share, w)

    def at_phase(ph):
        for b, m in enumerate(sims):
            m.svc_scale = [np.float32(1e6 / float(x)) for x in mus[b, ph]]

    at_phase(0)
    drops = np.array([sum(r.dropped for r in m.reset()) for m in sims])
    back.reset(None)
    acts = fr.actions_of(case, B)
    for k in range(8):
        assert_matches_sims(back.env, sims, drops)
        at_phase((k // H) % P)
        wts = fr.weights_of(acts[k], kw)
        _, _, assign = back.step(acts[k])
        rs = [m.step(wts[b]) for b, m in enumerate(sims)]
        drops += np.array([r.dropped for r in rs])
        np.testing.assert_array_equal(assign, np.array([r.assigned for r in rs]))
    assert_matches_sims(back.env, sims, drops)
    back.env.close()


@gpu
def test_arrival_schedule_of_equal_phases(lib):
    """An arrival-rate schedule whose phases all hold the per-env rates R is set_rates(R): the
    schedule's gather in front of the launch composes with cross traffic (identity)."""
    case, B = "s4-sed-levels", 24
    sched, S, kw, share, w = small_pair(case, B)
    plain = small_pair(case, B)[0]
    lam = np.random.default_rng(12).uniform(30.0, 120.0, B).astype(np.float32)
    sched.env.set_rate_schedule(np.repeat(lam[:, None], 3, axis=1), None, steps_per_phase=2)
    plain.env.set_rates(lam, None)
    acts = fr.actions_of(case, B)
    for x, y in zip(sched.reset(None)[:1], plain.reset(None)[:1]):
        np.testing.assert_array_equal(x, y)
    for k in range(7):
        for x, y in zip(sched.step(acts[k]), plain.step(acts[k])):
            np.testing.assert_array_equal(x, y)
    assert sched.env.handle.state_bytes() == plain.env.handle.state_bytes()
    assert hidden_queued(sched.env)[1].sum() > 0
    sched.env.close()
    plain.env.close()


@gpu
def test_next_step_auto_reset_across_an_episode_end(lib):
    """max_steps = 3 with next-step auto-reset: the step after an episode's end resets in place
    (episode 2's salt, its warm-up with hidden flows), against the reference."""
    case, B = "s4-sed-levels", 24
    S, kw = fr.config_kwargs(case)
    share, w = cross_params(case, B)
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=True, autoreset_mode="next_step",
                            cross_traffic=True, max_steps=3, **kw)
    env.set_cross_traffic(share, w)
    sims = reference_sims(case, B, share, w)
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
def test_replayed_graph_sees_an_in_place_rewrite(lib):
    """A step captured before set_cross_traffic rewrites the arrays in place reads the new values
    on replay: equal to an eager twin given the same values at the same step."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    case, B = "s4-sed-levels", 24
    S, kw = fr.config_kwargs(case)
    first, second = cross_params(case, B), cross_params(case, B, variant=1)
    eager = VecLoadBalanceEnv(B, S, device="cuda:0", cross_traffic=True, **kw)
    graph = VecLoadBalanceEnv(B, S, device="cuda:0", cross_traffic=True, graph_mode=True, **kw)
    for e in (eager, graph):
        e.set_cross_traffic(*first)
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
        if k == 4:  # after three replays: new shares and weights, no new capture
            for e in (eager, graph):
                e.set_cross_traffic(*second)
        a_static.copy_(acts[k])
        cg.replay()
        eo, er, ed, _ = eager.step(acts[k])
        assert torch.equal(obs, eo), k
        assert torch.equal(rew, er) and torch.equal(done, ed), k
    assert graph.handle.state_bytes() == eager.handle.state_bytes()
    d, hid = hidden_queued(graph)
    assert hid.sum() > 0
    eager.close()
    graph.close()


@gpu
def test_shards_at_uneven_sizes(lib):
    """Shards of 5, 12 and 7 envs with their own rows equal the 24-env handle's rows."""
    case, B = "s4-sed-levels", 24
    S, kw = fr.config_kwargs(case)
    share, w = cross_params(case, B)
    whole = DeviceBackend(B, S, kw, cross=(share, w), cross_traffic=True)
    acts = fr.actions_of(case, B)
    whole.reset(None)
    outs = [whole.step(acts[k]) for k in range(4)]
    dw, hw = hidden_queued(whole.env)
    lo = 0
    for n in (5, 12, 7):
        part = DeviceBackend(n, S, {**kw, "env_id_offset": kw.get("env_id_offset", 0) + lo},
                             cross=(share[lo:lo + n], w[lo:lo + n]), cross_traffic=True)
        part.reset(None)
        for k in range(4):
            got = part.step(acts[k][lo:lo + n])
            for x, y in zip(got, outs[k]):
                np.testing.assert_array_equal(x, y[lo:lo + n])
        dp, hp = hidden_queued(part.env)
        np.testing.assert_array_equal(hp, hw[lo:lo + n])
        np.testing.assert_array_equal(dp["dropped"], dw["dropped"][lo:lo + n])
        part.env.close()
        lo += n
    assert hw.sum() > 0
    whole.env.close()


@gpu
def test_facades_forward(lib):
    """LoadBalanceEnv and VecMultiAgentLoadBalanceEnv set, read back and clear the values."""
    from marllb_amd.env import LoadBalanceEnv
    from marllb_amd.multi_agent import VecMultiAgentLoadBalanceEnv
    one = LoadBalanceEnv(num_servers=4, cross_traffic=True, seed=3)
    one.set_cross_traffic(0.25, [1.0, 0.0, 1.0, 2.0])
    sh, wt = one.cross_traffic
    assert sh == 0.25 and np.allclose(wt, [0.25, 0.0, 0.25, 0.5], atol=2.0 ** -23)
    one.reset()
    one.step(np.zeros(4, np.int64))
    one.clear_cross_traffic()
    assert one.cross_traffic[0] == 0.0
    one.close()
    ma = VecMultiAgentLoadBalanceEnv(6, num_agents=2, servers_per_agent=2, cross_traffic=True)
    ma.set_cross_traffic(np.linspace(0.0, 1.0, 6), [1.0, 1.0, 2.0, 0.0])
    sh, wt = ma.cross_traffic
    np.testing.assert_allclose(sh.cpu().numpy(), np.linspace(0.0, 1.0, 6), atol=2.0 ** -24)
    np.testing.assert_allclose(wt.cpu().numpy(), np.tile([0.25, 0.25, 0.5, 0.0], (6, 1)),
                               atol=2.0 ** -23)
    ma.reset()
    ma.clear_cross_traffic()
    assert not ma.cross_traffic[0].any()
    ma.vec.close()


@gpu
def test_error_paths(lib):
    import torch
    from marllb_amd import _lib
    from marllb_amd.env import VecLoadBalanceEnv
    with pytest.raises(_lib.LbsimError) as e:
        VecLoadBalanceEnv(8, 4, device="cuda:0", cross_traffic=True, lost_fin_prob=0.2)
    assert e.value.code == _lib.ENOTSUP
    late = VecLoadBalanceEnv(8, 4, device="cuda:0")
    with pytest.raises(_lib.LbsimError) as e:
        late.set_cross_traffic(0.5)  # not enabled
    assert e.value.code == _lib.ENOTSUP
    late.reset()
    with pytest.raises(ValueError):
        late.handle.enable_cross_traffic()  # after the first reset
    late.close()
    env = VecLoadBalanceEnv(8, 4, device="cuda:0", cross_traffic=True)
    env.set_cross_traffic(0.5, [1.0, 2.0, 0.0, 1.0])
    before = [t.cpu().numpy().copy() for t in env.handle.cross_traffic()]
    sh3 = torch.full((3,), 0.5, device="cuda:0")
    with pytest.raises(_lib.LbsimError) as e:  # rows neither 1 nor B
        env.handle.set_cross_traffic(sh3, None, rows=3)
    assert e.value.code == _lib.ESHAPE
    with pytest.raises(ValueError):
        env.set_cross_traffic(np.full(3, 0.5))
    for share, w in [(np.nan, None), (-0.01, None), (1.01, None),
                     (0.5, [1.0, np.nan, 1.0, 1.0]), (0.5, [1.0, -1.0, 1.0, 1.0]),
                     (0.5, [0.0, 0.0, 0.0, 0.0]), (0.5, [1.0, np.inf, 1.0, 1.0]),
                     (np.array([0.1] * 7 + [2.0]), None)]:
        with pytest.raises(ValueError):
            env.set_cross_traffic(share, w)
        after = [t.cpu().numpy() for t in env.handle.cross_traffic()]
        for x, y in zip(before, after):  # what was in force is untouched
            np.testing.assert_array_equal(x, y)
    env.close()


# ---- theory

@pytest.fixture(scope="module")
def theory_run(lib):
    """ALIAS with visible weights TH_A, hidden weights TH_C != TH_A and share 0.5, at
    test_queueing_theory's run shape (4096 envs, flow statistics, no warm-up, Q = 64)."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    env = VecLoadBalanceEnv(qt.B, 4, device="cuda:0", autoreset=False, flow_stats=True,
                            cross_traffic=True, seed=9202, warmup_steps=0, queue_capacity=qt.Q,
                            step_interval=qt.DT, action_type="continuous", max_steps=1 << 30,
                            assign_policy="alias", arrival_rate=TH_LAM, server_rates=TH_MU)
    env.set_cross_traffic(TH_P, TH_C)
    env.reset()
    a = torch.tensor(TH_A, dtype=torch.float32, device="cuda:0").expand(qt.B, 4).contiguous()
    for _ in range(theory_burn()):
        env.step(a)
    env.clear_flow_stats()
    in_flight = torch.zeros((qt.B, 4), dtype=torch.float64, device="cuda:0")
    for _ in range(TH_REC):
        obs = env.step(a)[0]
        in_flight += obs[:, :, 0].to(torch.float64)
    cnt, sm, _ = env.handle.flow_stats()
    r = qt.Run()
    r.count = cnt.cpu().numpy().view(np.uint32).astype(np.float64)
    r.sum_s = sm.cpu().numpy().view(np.uint64).astype(np.float64) * 1e-6
    r.in_flight = in_flight.cpu().numpy()
    r.dropped = int(cross_state(env)["dropped"].astype(np.int64).sum())
    env.close()
    return r


def theory_checks(r):
    tot, vis = theory_rates()
    means = [qt.Check(f"cross traffic: visible mean fct, server {s}", *qt.server_mean(r, s),
                      qt.mm1(TH_MU[s], tot[s])) for s in range(4)]
    t = TH_REC * qt.DT
    # (the completion rate's "mu scaled by k" scales the rate itself, as the arrival test does)
    rates = [qt.Check(f"cross traffic: visible completion rate, server {s}",
                      *qt.ratio(r.count[:, s], np.full(qt.B, t)), lambda k, s=s: k * vis[s])
             for s in range(4)]
    n_mean = r.in_flight.sum(1) / TH_REC
    rate_times_fct = r.sum_s.sum(1) / t
    d = n_mean - rate_times_fct
    little = [qt.Check("cross traffic: Little, column 0 against visible rate x mean fct",
                       n_mean.mean(), d.std(ddof=1) / math.sqrt(qt.B),
                       lambda k: k * rate_times_fct.mean())]
    return means, rates, little


@gpu
def test_theory_superposed_streams(theory_run):
    """Server s is M/M/1 at lambda ((1-p) a_s / sum a + p c_s / sum c): the visible flows' mean
    FCT meets it (PASTA), their completion rate is (1-p) lambda a_s / sum a, and Little's law
    holds between column 0 and the visible flow statistics.  Scaled by 1.03 each must fail."""
    assert theory_run.dropped == 0
    means, rates, little = theory_checks(theory_run)
    qt.assert_checks(means + rates + little)
    for c in means + rates + little:
        assert not c.ok(1.03), f"does not discriminate: {c}"
