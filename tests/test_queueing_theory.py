"""The simulated queues against closed forms of queueing theory, on the device.

The exact tests (tests/test_flowsim_ref.py) show that the kernels compute what DESIGN.md §3
describes; these show that what it describes is the process it claims to be: Poisson arrivals,
FIFO M/M/1 and M/G/1 servers, Poisson thinning under ALIAS, Little's law between the observation
and the flow statistics, and the order LSQ < LSQ2 < random assignment.

Every device run: B = 4096 envs, flow_stats=True, warmup_steps=0 (the warm-up runs at weights 1.0,
which is another system), queue_capacity=64, a burn-in of at least 10 relaxation times
tau = 1 / (mu (1 - sqrt(rho))^2) of the slowest server at the test's own weights, then
clear_flow_stats() and the recorded steps.

Estimator: sum of sum_us over sum of count, over envs.  The envs are independent, so its standard
error comes from the across-env residuals of the ratio.  Rule, for every check:

    |estimate - theory| <= 5 SE + 0.001 theory      and      SE <= 0.005 theory.

The 0.1 % covers the known biases: gaps and service times are truncated to whole us (< 1e-4 at
means >= 20 ms), the uniforms sit on a 24-bit grid (~2^-25), a queue of 64 truncates rho^64, the
tabled exponential gaps of the M/G/1 runs have cv^2 = 0.99996.  The cap on the SE is a condition,
not a measurement: a noisy or degenerate run fails instead of passing, and the allowed deviation
is at most 2.6 %.  A theory value scaled by mu -> 1.03 mu must fail (checked for every test by
test_checks_discriminate; the arrival test scales lambda, Little's law the measured rate).
The measured values are in DESIGN.md §6.
"""
import math

import numpy as np
import pytest

from marllb_amd import flowstats, workload
from tests import statelayout
from tests.flowsim_ref import FlowSim
from tests.parity import lib  # noqa: F401  (the fixture: fails a gpu test run without a device)

gpu = pytest.mark.gpu
B, DT, Q = 4096, 0.25, 64
NSE, SLACK, CAP = 5.0, 1e-3, 5e-3


class Check:
    """One estimate against theory(k), the closed form with mu scaled by k."""

    def __init__(self, name, est, se, theory):
        self.name, self.est, self.se, self.theory = name, float(est), float(se), theory

    def ok(self, k=1.0):
        t = self.theory(k)
        return abs(self.est - t) <= NSE * self.se + SLACK * t

    def capped(self):
        return self.se <= CAP * self.theory(1.0)

    def __str__(self):
        t = self.theory(1.0)
        return (f"THEORY {self.name}: estimate {self.est:.6g} theory {t:.6g} SE {self.se:.3g} "
                f"({100 * self.se / t:.3f} %) deviation {(self.est - t) / self.se:+.2f} SE")


def assert_checks(checks):
    for c in checks:
        print(c)
    for c in checks:
        assert c.capped(), f"SE above the cap: {c}"
        assert c.ok(), str(c)


def ratio(num, den):
    """sum(num) / sum(den) over independent envs, and its standard error from the residuals."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    est = num.sum() / den.sum()
    r = num - est * den
    n = len(num)
    return est, math.sqrt(n / (n - 1.0) * float((r * r).sum())) / den.sum()


def relaxation(mu, lam):
    return 1.0 / (mu * (1.0 - math.sqrt(lam / mu)) ** 2)


def burn_steps(tau):
    return int(math.ceil(10.0 * tau / DT))


def mm1(mu, lam):
    return lambda k: 1.0 / (k * mu - lam)


def pollaczek_khinchine(mu, lam, cv2):
    def t(k):
        m = k * mu
        return 1.0 / m + lam * (1.0 + cv2) / (2.0 * m * m * (1.0 - lam / m))
    return t


# ------------------------------------------------------------------ sizes, on the reference

REC_MM1, REC_THIN = 160, 100  # recorded steps of the device runs sized here
THIN_W, THIN_MU, THIN_LAM = [1.0, 2.0, 3.0, 4.0], [12.5, 25.0, 37.5, 50.0], 50.0


def reference_run(envs, S, policy, lam, mus, weights, burn, rec, seed):
    """count and sum_us (envs, S) of the flows completed in `rec` steps after `burn` steps."""
    count, sum_us = np.zeros((envs, S)), np.zeros((envs, S))
    for b in range(envs):
        sim = FlowSim(seed, b, S, Q, policy, lam, mus, dt=DT, warmup_steps=0)
        sim.reset()
        for _ in range(burn):
            sim.step(weights)
        for _ in range(rec):
            for s, ta, tc in sim.step(weights).completed:
                count[b, s] += 1
                sum_us[b, s] += tc - ta
    return count, sum_us


def test_sizes_on_the_reference():
    """The reference alone, at reduced size, meets the closed forms, and 1 / sqrt(n) scaling of
    its standard errors puts the device runs (4096 envs x the recorded steps) under the cap."""
    envs, rec = 96, 40
    count, sum_us = reference_run(envs, 1, "sed", 20.0, [40.0], [1.0],
                                  burn_steps(relaxation(40.0, 20.0)), rec, 9001)
    est, se = ratio(sum_us[:, 0] * 1e-6, count[:, 0])
    c = Check("reference M/M/1 mean", est, se, mm1(40.0, 20.0))
    print(c)
    assert c.ok()
    assert se * math.sqrt(envs * rec / (B * REC_MM1)) <= CAP * 0.05
    envs, rec = 64, 40
    count, sum_us = reference_run(envs, 4, "alias", THIN_LAM, THIN_MU, THIN_W,
                                  burn_steps(relaxation(12.5, 5.0)), rec, 9002)
    for s in range(4):
        est, se = ratio(sum_us[:, s] * 1e-6, count[:, s])
        c = Check(f"reference thinning server {s}", est, se,
                  mm1(THIN_MU[s], THIN_LAM * THIN_W[s] / sum(THIN_W)))
        print(c)
        assert c.ok()
        assert se * math.sqrt(envs * rec / (B * REC_THIN)) <= CAP * c.theory(1.0)


# ------------------------------------------------------------------ the device runs

class Run:
    pass


def dropped_and_index(env):
    d = statelayout.parse_cfg(env.handle.state_bytes(), env.cfg)
    return d["dropped"].astype(np.int64), d["arr_idx"].astype(np.int64)


def device_run(S, weights, burn, rec, seed, tables=None, **kw):
    """Burn in, clear the statistics, record: the per-(env, server) statistics, the assignments,
    the per-env sums of arrivals and their squares, and the sum of obs column 0 at step ends."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=False, flow_stats=True, seed=seed,
                            warmup_steps=0, queue_capacity=Q, step_interval=DT,
                            action_type="continuous", max_steps=1 << 30, **kw)
    if tables is not None:
        env.set_workload_tables(np.stack(tables), 0, 1)  # gaps from table 0, work from table 1
    env.reset()
    a = torch.tensor(weights, dtype=torch.float32, device="cuda:0").expand(B, S).contiguous()
    for _ in range(burn):
        env.step(a)
    env.clear_flow_stats()
    drop0, idx0 = dropped_and_index(env)
    f64 = dict(dtype=torch.float64, device="cuda:0")
    assigned, in_flight = torch.zeros((B, S), **f64), torch.zeros((B, S), **f64)
    arr, arr2 = torch.zeros(B, **f64), torch.zeros(B, **f64)
    for _ in range(rec):
        obs, _, _, info = env.step(a, assign_counts=True)
        n = info["assign_counts"].to(torch.float64)
        assigned += n
        arr += n.sum(1)
        arr2 += n.sum(1) ** 2
        in_flight += obs[:, :, 0].to(torch.float64)
    r = Run()
    cnt, sm, _, hist = env.handle.flow_stats(hist=True)
    r.count = cnt.cpu().numpy().view(np.uint32).astype(np.float64)
    r.sum_s = sm.cpu().numpy().view(np.uint64).astype(np.float64) * 1e-6
    r.hist = hist.cpu().numpy().view(np.uint32).astype(np.int64)
    r.assigned, r.in_flight = assigned.cpu().numpy(), in_flight.cpu().numpy()
    r.arr, r.arr2, r.rec = arr.cpu().numpy(), arr2.cpu().numpy(), rec
    drop1, idx1 = dropped_and_index(env)
    r.drops = int((drop1 - drop0).sum())
    # arrivals are assignments plus drops: the arrival index says the same
    np.testing.assert_array_equal(idx1 - idx0, r.assigned.sum(1) + (drop1 - drop0))
    env.close()
    return r


def server_mean(r, s):
    return ratio(r.sum_s[:, s], r.count[:, s])


# bin edges (flowstats.bin_lower_us) near 0.4, 1 and 2 mean sojourn times: bins 98, 108, 116
TAIL_EDGES = {98: 20480, 108: 49152, 116: 98304}


@pytest.fixture(scope="module")
def mm1_checks(lib):
    mu, lam = 40.0, 20.0
    r = device_run(1, [1.0], burn_steps(relaxation(mu, lam)), REC_MM1, 9101,
                   arrival_rate=lam, server_rates=[mu])
    assert r.drops == 0 and r.count.sum() > 0.9 * B * REC_MM1 * lam * DT
    checks = [Check("M/M/1 mean", *server_mean(r, 0), mm1(mu, lam))]
    lower = flowstats.bin_lower_us()
    for k, edge in TAIL_EDGES.items():
        assert lower[k] == edge
        n = r.count[:, 0]
        p, se = ratio(r.hist[:, 0, k:].sum(-1), n)
        inflation = se * se / (p * (1.0 - p) / n.sum())  # across-env over binomial variance
        print(f"tail >= {edge} us: variance inflation {inflation:.2f}")
        se = math.sqrt(p * (1.0 - p) / n.sum() * inflation)
        checks.append(Check(f"M/M/1 P(T >= {edge} us)", p, se,
                            lambda k, e=edge: math.exp(-(k * mu - lam) * e * 1e-6)))
    return checks


@gpu
def test_mm1_mean_and_tail(mm1_checks):
    assert_checks(mm1_checks)


@pytest.fixture(scope="module")
def thinning_checks(lib):
    lam_s = [THIN_LAM * w / sum(THIN_W) for w in THIN_W]
    r = device_run(4, THIN_W, burn_steps(relaxation(THIN_MU[0], lam_s[0])), REC_THIN, 9102,
                   assign_policy="alias", arrival_rate=THIN_LAM, server_rates=THIN_MU)
    assert r.drops == 0
    means = [Check(f"thinning mean, server {s}", *server_mean(r, s), mm1(THIN_MU[s], lam_s[s]))
             for s in range(4)]
    shares = [Check(f"thinning share, server {s}", *ratio(r.assigned[:, s], r.assigned.sum(1)),
                    lambda k, s=s: THIN_W[s] / sum(THIN_W)) for s in range(4)]
    return means, shares


@gpu
def test_poisson_thinning(thinning_checks):
    assert_checks(thinning_checks[0] + thinning_checks[1])


@pytest.fixture(scope="module")
def arrival_checks(lib):
    lam, rec = 100.0, 80
    r = device_run(4, [1.0] * 4, 4, rec, 9103, arrival_rate=lam, load=0.5)
    assert r.drops == 0  # so the assignments of a step are its arrivals
    mean = Check("arrivals per step, mean", *ratio(r.arr, np.full(B, float(rec))),
                 lambda k: k * lam * DT)  # k scales lambda here
    m = mean.est
    d = (r.arr2 - 2.0 * m * r.arr + rec * m * m) / (rec * m)  # per env: sum (n - m)^2 / (rec m)
    disp = Check("arrivals per step, variance / mean", d.mean() * B * rec / (B * rec - 1.0),
                 d.std(ddof=1) / math.sqrt(B), lambda k: 1.0)
    return [mean, disp]


@gpu
def test_arrival_process(arrival_checks):
    assert_checks(arrival_checks)


WORK_TABLES = {"M/D/1 constant": (workload.constant_table, 200),
               "M/H2/1 hyperexp(2)": (lambda: workload.hyperexp_table(2.0), 200),
               "M/G/1 bounded Pareto(1.5, 100)": (lambda: workload.bounded_pareto_table(1.5, 100.0),
                                                  400)}


@pytest.fixture(scope="module")
def pk_checks(lib):
    mu, lam = 40.0, 20.0
    gaps = workload.exponential_table()  # the staircase of Exp(1): Poisson arrivals to 4e-5
    assert abs(workload.table_cv2(gaps) - 1.0) < 1e-4
    assert abs(workload.table_mean(gaps) - 1.0) < 1e-6
    out = {}
    for i, (name, (make, rec)) in enumerate(WORK_TABLES.items()):
        work = make()
        r = device_run(1, [1.0], 48, rec, 9110 + i, tables=[gaps, work], arrival_rate=lam,
                       server_rates=[mu])
        assert r.drops == 0
        cv2 = workload.table_cv2(work)  # of the installed table: its quantisation is in the theory
        out[name] = [Check(f"{name} mean (cv2 {cv2:.4f})", *server_mean(r, 0),
                           pollaczek_khinchine(mu, lam, cv2))]
    return out


@gpu
@pytest.mark.parametrize("name", list(WORK_TABLES))
def test_pollaczek_khinchine(pk_checks, name):
    assert_checks(pk_checks[name])


@pytest.fixture(scope="module")
def little_checks(lib):
    S, lam, load, rec = 4, 100.0, 0.7, 100
    mu = lam / (load * S)
    r = device_run(S, [1.0] * S, burn_steps(relaxation(mu, lam / S)), rec, 9120,
                   arrival_rate=lam, load=load)
    assert r.drops == 0
    n_mean = r.in_flight.sum(1) / rec          # per env: flows in flight, mean over step ends
    # (completions / s) x (mean fct) = the sojourn time completed per second
    rate_times_fct = r.sum_s.sum(1) / (rec * DT)
    d = n_mean - rate_times_fct
    return [Check("Little: mean obs column 0 against rate x mean fct (per env, all servers)",
                  n_mean.mean(), d.std(ddof=1) / math.sqrt(B),
                  lambda k: k * rate_times_fct.mean())]  # k scales the measured rate here


@gpu
def test_littles_law(little_checks):
    assert_checks(little_checks)


@pytest.fixture(scope="module")
def ordering_checks(lib):
    S, mu, lam, rec = 8, 25.0, 160.0, 200
    burn = burn_steps(relaxation(mu, lam / S))  # the random-assignment leg is the slowest
    out = {}
    for i, policy in enumerate(["lsq", "lsq2", "alias"]):
        r = device_run(S, [1.0] * S, burn, rec, 9130 + i, assign_policy=policy, arrival_rate=lam,
                       server_rates=[mu] * S)
        # rho^64 = 6e-7 of the random leg's arrivals meet a full queue; each would have stayed
        # about Q + 1 service times: the sojourn time lost to drops is under 1e-4 of the total
        assert r.drops * (Q + 1) / mu <= 1e-4 * r.sum_s.sum()
        out[policy] = ratio(r.sum_s.sum(1), r.count.sum(1))
        print(f"THEORY ordering: {policy} mean fct {out[policy][0]:.6g} SE {out[policy][1]:.3g}")
    out["check"] = Check("uniform ALIAS mean, S = 8", *out["alias"], mm1(mu, lam / S))
    return out


@gpu
def test_policy_ordering(ordering_checks):
    o = ordering_checks
    assert_checks([o["check"]])
    for better, worse in (("lsq", "lsq2"), ("lsq2", "alias")):
        gap = o[worse][0] - o[better][0]
        assert gap > NSE * math.hypot(o[worse][1], o[better][1]), (better, worse, gap)


@gpu
def test_checks_discriminate(mm1_checks, thinning_checks, arrival_checks, pk_checks, little_checks,
                             ordering_checks):
    """Every theory test fails when its theoretical mu is scaled by 1.03."""
    groups = {"mm1 mean": mm1_checks[:1], "mm1 tail": mm1_checks[1:],
              "thinning": thinning_checks[0], "arrivals": arrival_checks[:1],
              "little": little_checks, "ordering": [ordering_checks["check"]], **pk_checks}
    for name, checks in groups.items():
        assert all(not c.ok(1.03) for c in checks), name
