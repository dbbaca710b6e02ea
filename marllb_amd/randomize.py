"""Domain randomisation of the per-env workload (VecLoadBalanceEnv.set_rates).

sample_rates draws one arrival rate and one set of server rates per env, so one handle trains a
policy across light, heavy and overloaded clusters with fast, slow and heterogeneous servers.
diurnal_schedule and burst_schedule draw per-env arrival schedules whose load moves inside an
episode (VecLoadBalanceEnv.set_rate_schedule); schedule_phase states the phase rule.
sample_trace_ids and diurnal_trace_schedule are their counterparts for a TRACE handle's bank of
traces (VecLoadBalanceEnv.set_env_trace / set_trace_schedule).
Pure torch; deterministic for a seeded generator.
"""
from __future__ import annotations

import math

import numpy as np


def sample_rates(num_envs: int, num_servers: int, *, rate=(100.0, 1000.0), load=(0.3, 1.2),
                 server_skew=(1.0, 4.0), generator=None, device=None):
    """-> (arrival (B,), server (B, S)) float32 tensors, flows/s.

    rate (lo, hi): each env's arrival rate, log-uniform in [lo, hi].
    load (lo, hi): each env's utilisation arrival / sum(server), uniform in [lo, hi]; the env's
    capacity is arrival / load.
    server_skew (lo, hi): each server's multiplier, uniform in [lo, hi]; an env's capacity is split
    over its servers in proportion to them (renormalised), so two servers of one env differ by at
    most hi / lo.
    generator: a torch.Generator (the draws are made on its device, then moved to `device`).
    """
    import torch

    B, S = int(num_envs), int(num_servers)
    for name, (lo, hi) in (("rate", rate), ("load", load), ("server_skew", server_skew)):
        if not (0.0 < float(lo) <= float(hi)) or not math.isfinite(float(hi)):
            raise ValueError(f"{name}: need 0 < lo <= hi (got {lo}, {hi})")
    gdev = generator.device if generator is not None else torch.device("cpu")

    def uniform(shape, lo, hi):
        u = torch.rand(shape, generator=generator, device=gdev, dtype=torch.float64)
        return float(lo) + (float(hi) - float(lo)) * u

    arrival = torch.exp(uniform((B,), math.log(rate[0]), math.log(rate[1])))
    arrival = arrival.clamp(float(rate[0]), float(rate[1]))  # exp(log(x)) may miss x by an ulp
    rho = uniform((B,), load[0], load[1])
    skew = uniform((B, S), server_skew[0], server_skew[1])
    server = (arrival / rho).unsqueeze(1) * skew / skew.sum(dim=1, keepdim=True)
    return (arrival.to(device=device, dtype=torch.float32),
            server.to(device=device, dtype=torch.float32))


# ---- rate schedules (VecLoadBalanceEnv.set_rate_schedule): non-stationary workloads

ARRIVAL_RANGE = (0.1, 1.0e6)  # flows/s, make_config's range for arrival_rate


def schedule_phase(k, phases: int, steps_per_phase: int = 1, wrap: bool = True):
    """The phase a step runs at when the env has completed k steps of its episode: with
    j = k // steps_per_phase, j % phases when cyclic (wrap), else min(j, phases - 1).  k: an int,
    a numpy array or a torch tensor (k < 0 counts as 0).  The host statement of the rule the
    dynamics kernels apply per env; a reset (warm-up included) always runs at phase 0."""
    P, H = int(phases), int(steps_per_phase)
    if P < 1 or H < 1:
        raise ValueError(f"need phases >= 1 and steps_per_phase >= 1 (got {phases}, "
                         f"{steps_per_phase})")
    if isinstance(k, (int, np.integer)):
        j = max(int(k), 0) // H
        return j % P if wrap else min(j, P - 1)
    if isinstance(k, np.ndarray):
        j = np.maximum(k.astype(np.int64), 0) // H
        return j % P if wrap else np.minimum(j, P - 1)
    j = k.long().clamp(min=0) // H
    return j % P if wrap else j.clamp(max=P - 1)


def _arrival_rows(arrival, generator):
    import torch

    gdev = generator.device if generator is not None else torch.device("cpu")
    a = torch.as_tensor(arrival, dtype=torch.float64).reshape(-1).to(gdev)
    if a.numel() < 1 or not bool(((a >= ARRIVAL_RANGE[0]) & (a <= ARRIVAL_RANGE[1])).all()):
        raise ValueError(f"arrival: need (B,) rates in [{ARRIVAL_RANGE[0]}, {ARRIVAL_RANGE[1]}]")
    return a, gdev


def diurnal_schedule(arrival, phases: int, *, amplitude=(0.2, 0.8), generator=None, device=None):
    """-> arrival schedule (B, phases) float32, flows/s: a day of rising and falling load,
    arrival[b] * (1 + a_b * sin(2 pi (j / phases + phi_b))) for phase j, with each env's relative
    amplitude a_b uniform in amplitude = (lo, hi), 0 <= lo <= hi < 1, and its phase offset phi_b
    uniform in [0, 1).  arrival: (B,) base rates (a scalar: one env).  Clamped to make_config's
    arrival range; deterministic for a seeded generator."""
    import torch

    P = int(phases)
    lo, hi = float(amplitude[0]), float(amplitude[1])
    if P < 1 or not (0.0 <= lo <= hi < 1.0):
        raise ValueError(f"need phases >= 1 and 0 <= lo <= hi < 1 (got {phases}, {amplitude})")
    a, gdev = _arrival_rows(arrival, generator)
    B = a.numel()
    amp = lo + (hi - lo) * torch.rand(B, generator=generator, device=gdev, dtype=torch.float64)
    phi = torch.rand(B, generator=generator, device=gdev, dtype=torch.float64)
    j = torch.arange(P, device=gdev, dtype=torch.float64) / P
    sched = a[:, None] * (1.0 + amp[:, None] * torch.sin(2.0 * math.pi * (j[None, :] + phi[:, None])))
    return sched.clamp(*ARRIVAL_RANGE).to(device=device, dtype=torch.float32)


def burst_schedule(arrival, phases: int, *, factor: float = 4.0, p_on: float = 0.1,
                   p_off: float = 0.5, generator=None, device=None):
    """-> arrival schedule (B, phases) float32, flows/s: bursts from a two-state Markov chain per
    env, sampled once here.  Every env starts calm (phase 0, the phase of a reset); a calm phase is
    followed by a burst with probability p_on, a burst by a calm phase with probability p_off;
    a burst phase runs at arrival[b] * factor, a calm one at arrival[b].  Clamped to make_config's
    arrival range; deterministic for a seeded generator."""
    import torch

    P = int(phases)
    if P < 1 or not (float(factor) > 0.0 and math.isfinite(float(factor))):
        raise ValueError(f"need phases >= 1 and a finite factor > 0 (got {phases}, {factor})")
    for name, v in (("p_on", p_on), ("p_off", p_off)):
        if not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"{name}: a probability (got {v})")
    a, gdev = _arrival_rows(arrival, generator)
    B = a.numel()
    u = torch.rand((B, P), generator=generator, device=gdev, dtype=torch.float64)
    on = torch.zeros((B, P), dtype=torch.bool, device=gdev)
    for j in range(1, P):
        prev = on[:, j - 1]
        on[:, j] = torch.where(prev, u[:, j] >= float(p_off), u[:, j] < float(p_on))
    sched = a[:, None] * torch.where(on, float(factor), 1.0)
    return sched.clamp(*ARRIVAL_RANGE).to(device=device, dtype=torch.float32)


# ---- trace banks (VecLoadBalanceEnv.set_env_trace / set_trace_schedule): the TRACE counterpart

def sample_trace_ids(num_envs: int, num_traces: int, seed: int = 0, *, device=None):
    """-> (B,) int32 trace ids, uniform over the bank's T traces: domain randomisation over the
    load of a TRACE handle (VecLoadBalanceEnv.set_env_trace).  Deterministic for a seed."""
    import torch

    B, T = int(num_envs), int(num_traces)
    if B < 1 or T < 1:
        raise ValueError(f"need num_envs >= 1 and num_traces >= 1 (got {num_envs}, {num_traces})")
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(0, T, (B,), generator=g, dtype=torch.int64).to(device=device,
                                                                        dtype=torch.int32)


def diurnal_trace_schedule(bank_rates, phases: int, num_envs: int, *, amplitude=(0.2, 0.8),
                           phase=(0.0, 1.0), seed: int = 0, device=None):
    """-> (B, phases) int32 trace ids: diurnal_schedule over a bank.  With mean the mean of
    bank_rates (the bank's per-trace arrival rates, TraceBank.rate), env b's target load in phase
    j is mean * (1 + a_b * sin(2 pi (j / phases + phi_b))), a_b uniform in amplitude = (lo, hi),
    0 <= lo <= hi < 1, phi_b uniform in phase = (lo, hi); the id is that of the bank trace whose
    rate is nearest to the target (the first of equals).  Deterministic for a seed."""
    import torch

    P, B = int(phases), int(num_envs)
    lo, hi = float(amplitude[0]), float(amplitude[1])
    plo, phi_hi = float(phase[0]), float(phase[1])
    if P < 1 or B < 1 or not (0.0 <= lo <= hi < 1.0) or not plo <= phi_hi:
        raise ValueError(f"need phases >= 1, num_envs >= 1, 0 <= lo <= hi < 1 and an ordered "
                         f"phase range (got {phases}, {num_envs}, {amplitude}, {phase})")
    rates = torch.as_tensor(np.asarray(bank_rates, np.float64)).reshape(-1)
    if rates.numel() < 1 or not bool((rates > 0).all()):
        raise ValueError("bank_rates: need (T,) positive rates")
    g = torch.Generator().manual_seed(int(seed))
    amp = lo + (hi - lo) * torch.rand(B, generator=g, dtype=torch.float64)
    phi = plo + (phi_hi - plo) * torch.rand(B, generator=g, dtype=torch.float64)
    j = torch.arange(P, dtype=torch.float64) / P
    target = rates.mean() * (1.0 + amp[:, None] * torch.sin(2.0 * math.pi * (j[None, :] + phi[:, None])))
    ids = (target[:, :, None] - rates[None, None, :]).abs().argmin(dim=2)
    return ids.to(device=device, dtype=torch.int32)


# ---- server availability (VecLoadBalanceEnv.set_cluster_sizes / set_server_availability)

def sample_cluster_sizes(num_envs: int, num_servers: int, min_servers: int = 1, seed: int = 0, *,
                         device=None):
    """-> (B,) int32 cluster sizes, uniform in [min_servers, num_servers]: cluster size as a
    randomised domain inside one fixed-width batch (VecLoadBalanceEnv.set_cluster_sizes: env b
    has its first n[b] servers up).  Deterministic for a seed."""
    import torch

    B, S, lo = int(num_envs), int(num_servers), int(min_servers)
    if B < 1 or S < 1 or not 0 <= lo <= S:
        raise ValueError(f"need num_envs >= 1 and 0 <= min_servers <= num_servers (got "
                         f"{num_envs}, {min_servers}, {num_servers})")
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(lo, S + 1, (B,), generator=g, dtype=torch.int64).to(device=device,
                                                                             dtype=torch.int32)


def outage_schedule(num_envs: int, num_servers: int, phases: int, n_down: int, start: int,
                    length: int, seed: int = 0, *, device=None):
    """-> (B, phases, S) uint8 availability table (1 = up): per env one correlated outage, a
    block of n_down consecutive servers (wrapping past the last one) whose first server is
    uniform over the S servers, down over the phases [start, start + length) and up otherwise
    (VecLoadBalanceEnv.set_server_availability).  Deterministic for a seed."""
    import torch

    B, S, P = int(num_envs), int(num_servers), int(phases)
    n, lo, ln = int(n_down), int(start), int(length)
    if B < 1 or S < 1 or P < 1 or not 0 <= n <= S or lo < 0 or ln < 0:
        raise ValueError(f"need num_envs, num_servers, phases >= 1, 0 <= n_down <= num_servers, "
                         f"start >= 0 and length >= 0 (got {num_envs}, {num_servers}, {phases}, "
                         f"{n_down}, {start}, {length})")
    g = torch.Generator().manual_seed(int(seed))
    first = torch.randint(0, S, (B,), generator=g, dtype=torch.int64)
    hit = ((torch.arange(S)[None, :] - first[:, None]) % S) < n          # (B, S)
    j = torch.arange(P)
    during = (j >= lo) & (j < lo + ln)                                   # (P,)
    up = ~(hit[:, None, :] & during[None, :, None])
    return up.to(device=device, dtype=torch.uint8)


def rolling_restart_schedule(num_servers: int, phases: int, *, device=None):
    """-> (phases, S) uint8 availability table (1 = up), shared by every env: a rolling restart,
    server j % S down in phase j for j = 1 .. phases - 1; phase 0 (the phase of an episode's
    first steps) has every server up."""
    import torch

    S, P = int(num_servers), int(phases)
    if S < 1 or P < 1:
        raise ValueError(f"need num_servers >= 1 and phases >= 1 (got {num_servers}, {phases})")
    j = torch.arange(P)
    down = (torch.arange(S)[None, :] == (j % S)[:, None]) & (j > 0)[:, None]
    return (~down).to(device=device, dtype=torch.uint8)


# ---- hidden cross traffic (VecLoadBalanceEnv.set_cross_traffic)

def sample_cross_traffic(num_envs: int, num_servers: int, *, share=(0.0, 0.5), skew=(1.0, 4.0),
                         generator=None, device=None):
    """-> (share (B,), weights (B, S)) float32 tensors for VecLoadBalanceEnv.set_cross_traffic.

    share (lo, hi): each env's hidden share, uniform in [lo, hi], 0 <= lo <= hi <= 1.
    skew (lo, hi): each env's ratio r, uniform in [lo, hi], 1 <= lo <= hi; its hidden weights are
    a random permutation of the geometric ladder 1, 1/r, ..., r^-(S-1) (another balancer favouring
    some servers; r = 1: uniform).
    generator: a torch.Generator (the draws are made on its device, then moved to `device`).
    The visible arrival rate of env b is (1 - share[b]) * its arrival rate: to keep it at `rate`,
    give set_rates the arrival rate rate / (1 - share).
    """
    import torch

    B, S = int(num_envs), int(num_servers)
    if B < 1 or S < 1:
        raise ValueError(f"need num_envs >= 1 and num_servers >= 1 (got {num_envs}, {num_servers})")
    if not 0.0 <= float(share[0]) <= float(share[1]) <= 1.0:
        raise ValueError(f"share: need 0 <= lo <= hi <= 1 (got {share[0]}, {share[1]})")
    if not (1.0 <= float(skew[0]) <= float(skew[1])) or not math.isfinite(float(skew[1])):
        raise ValueError(f"skew: need 1 <= lo <= hi (got {skew[0]}, {skew[1]})")
    gdev = generator.device if generator is not None else torch.device("cpu")

    def uniform(shape, lo, hi):
        u = torch.rand(shape, generator=generator, device=gdev, dtype=torch.float64)
        return float(lo) + (float(hi) - float(lo)) * u

    sh = uniform((B,), share[0], share[1]).clamp(0.0, 1.0)
    r = uniform((B,), skew[0], skew[1])
    rank = torch.rand((B, S), generator=generator, device=gdev).argsort(dim=1).to(torch.float64)
    w = torch.pow(r.unsqueeze(1), -rank)
    return (sh.to(device=device, dtype=torch.float32), w.to(device=device, dtype=torch.float32))


# ---- multi-worker servers (VecLoadBalanceEnv.set_server_workers)

SERVER_RANGE = (1.0, 1.0e7)  # flows/s, make_config's range for a server rate


def sample_server_workers(num_envs: int, num_servers: int, choices=(1, 2, 4), seed: int = 0,
                          keep_capacity: bool = True, *, server_rates=None, device=None):
    """-> (workers (B, S) int32, server_rate (B, S) float32) for
    VecLoadBalanceEnv.set_server_workers and set_rates(None, server_rate); on an env with
    service_discipline="ps" the same pair gives the servers' cores:
    vec.set_ps_cores(workers); vec.set_rates(None, server_rate).

    workers: each server's count, uniform over `choices` (integers in [1, 64]).
    server_rate: the rate of ONE worker.  server_rates (a scalar, (S,) or (B, S), flows/s; default
    100) is each server's rate before the split; with keep_capacity it is divided by the server's
    count, so "one fast core against several slow ones" is compared at equal capacity c * mu;
    without, every worker keeps it and a server of c workers has c times the capacity.  Clamped to
    make_config's range for a server rate.  Deterministic for a seed."""
    import torch

    B, S = int(num_envs), int(num_servers)
    ch = [int(c) for c in choices]
    if B < 1 or S < 1:
        raise ValueError(f"need num_envs >= 1 and num_servers >= 1 (got {num_envs}, {num_servers})")
    if not ch or any(c != x for c, x in zip(ch, choices)) or min(ch) < 1 or max(ch) > 64:
        raise ValueError(f"choices: need integers in [1, 64] (got {tuple(choices)})")
    g = torch.Generator().manual_seed(int(seed))
    pick = torch.randint(0, len(ch), (B, S), generator=g, dtype=torch.int64)
    workers = torch.tensor(ch, dtype=torch.int64)[pick]
    base = torch.as_tensor(100.0 if server_rates is None else server_rates).to(
        device="cpu", dtype=torch.float64)
    if tuple(base.shape) not in ((), (S,), (B, S)) or not bool((base > 0).all()):
        raise ValueError(f"server_rates: need positive rates, a scalar, ({S},) or ({B}, {S})")
    rate = base.expand(B, S) / workers.to(torch.float64) if keep_capacity else base.expand(B, S)
    rate = rate.clamp(*SERVER_RANGE)
    return (workers.to(device=device, dtype=torch.int32),
            rate.to(device=device, dtype=torch.float32).contiguous())


# ---- action latency (VecLoadBalanceEnv.set_action_delay)


def sample_action_delay(num_envs: int, low: float = 0.0, high: float = 0.25, seed: int = 0, *,
                        max_delay: float | None = None, device=None):
    """-> (B,) float32 seconds for VecLoadBalanceEnv.set_action_delay: each env's control delay,
    uniform over [low, high], clamped to the valid range [0, max_delay] (max_delay: the env's
    max_delay_steps * step_interval; default `high`).  Deterministic for a seed."""
    import torch

    B = int(num_envs)
    if B < 1:
        raise ValueError(f"need num_envs >= 1 (got {num_envs})")
    lo, hi = float(low), float(high)
    if not (0.0 <= lo <= hi) or hi != hi or hi == float("inf"):
        raise ValueError(f"need 0 <= low <= high, finite (got {low}, {high})")
    top = hi if max_delay is None else float(max_delay)
    if not top >= 0.0:
        raise ValueError(f"max_delay: need a value >= 0 (got {max_delay})")
    g = torch.Generator().manual_seed(int(seed))
    u = torch.rand(B, generator=g, dtype=torch.float64)
    # (clamped in f64: the f32 of the bound is within half an ulp of it, far below the half
    # microsecond that the conversion to whole us rounds away)
    d = (lo + (hi - lo) * u).clamp(0.0, top)
    return d.to(device=device, dtype=torch.float32).contiguous()


# ---- ACK intervals (VecLoadBalanceEnv.set_ack_interval)


def sample_ack_interval(num_envs: int, lo_us: int = 250, hi_us: int = 4000, seed: int = 0, *,
                        device=None):
    """-> (B,) int32 microseconds for VecLoadBalanceEnv.set_ack_interval: each env's ACK interval,
    log-uniform over [lo_us, hi_us] (1 <= lo_us <= hi_us <= 2^30), rounded to whole us and kept
    inside the bounds.  Deterministic for a seed."""
    import math

    import torch

    B = int(num_envs)
    if B < 1:
        raise ValueError(f"need num_envs >= 1 (got {num_envs})")
    lo, hi = int(lo_us), int(hi_us)
    if lo != lo_us or hi != hi_us or not 1 <= lo <= hi <= 1 << 30:
        raise ValueError(f"need integers 1 <= lo_us <= hi_us <= 2^30 (got {lo_us}, {hi_us})")
    g = torch.Generator().manual_seed(int(seed))
    u = torch.rand(B, generator=g, dtype=torch.float64)
    v = torch.exp(math.log(lo) + (math.log(hi) - math.log(lo)) * u).round().clamp(lo, hi)
    return v.to(device=device, dtype=torch.int32).contiguous()


def sample_pool_arrival_rates(num_pools: int, num_balancers: int, total=(200.0, 400.0),
                              skew=(1.0, 1.0), seed: int = 0, *, generator=None, device=None):
    """-> (num_pools * num_balancers,) float32 flows/s for set_rates(arrival_rate=...) of an env
    with balancers_per_pool = num_balancers: the ECMP split of each pool's
    traffic.  A pool's total rate is uniform over `total` = (lo, hi); its members' shares are a
    geometric ladder 1, 1/q, 1/q^2, ... with q uniform over `skew` = (lo >= 1, hi), in a random
    order, scaled to sum to the total (q = 1: equal shares).  Every rate must stay inside the
    config's range [0.1, 1e6].  Deterministic for a seed or a seeded generator."""
    import torch

    C, A = int(num_pools), int(num_balancers)
    if C < 1 or A < 1:
        raise ValueError(f"need num_pools >= 1 and num_balancers >= 1 (got {num_pools}, "
                         f"{num_balancers})")
    tlo, thi = (float(x) for x in total)
    qlo, qhi = (float(x) for x in skew)
    if not (0.0 < tlo <= thi) or thi == float("inf"):
        raise ValueError(f"total: need 0 < lo <= hi, finite (got {total})")
    if not (1.0 <= qlo <= qhi) or qhi == float("inf"):
        raise ValueError(f"skew: need 1 <= lo <= hi, finite (got {skew})")
    g = generator if generator is not None else torch.Generator().manual_seed(int(seed))
    tot = tlo + (thi - tlo) * torch.rand(C, generator=g, dtype=torch.float64)
    q = qlo + (qhi - qlo) * torch.rand(C, generator=g, dtype=torch.float64)
    order = torch.rand(C, A, generator=g, dtype=torch.float64).argsort(dim=1)
    share = q.unsqueeze(1) ** (-order.to(torch.float64))
    rates = tot.unsqueeze(1) * share / share.sum(dim=1, keepdim=True)
    if float(rates.min()) < 0.1 or float(rates.max()) > 1.0e6:
        raise ValueError("a member's rate leaves [0.1, 1e6] flows/s: narrow `total` or `skew`")
    return rates.reshape(-1).to(device=device, dtype=torch.float32).contiguous()
