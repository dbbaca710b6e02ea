"""Domain randomisation of the per-env workload (VecLoadBalanceEnv.set_rates).

sample_rates draws one arrival rate and one set of server rates per env, so one handle trains a
policy across light, heavy and overloaded clusters with fast, slow and heterogeneous servers.
Pure torch; deterministic for a seeded generator.
"""
from __future__ import annotations

import math


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
