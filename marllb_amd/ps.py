"""Processor-sharing servers: VecLoadBalanceEnv(..., service_discipline="ps").

Every server has one worker that the flows queued on it share equally, as an application host
with more worker processes than cores shares its CPU; ps_cores=... gives a server several cores
(§3.23).  check_ps_config states, without a device,
what lbsim_processor_sharing_enable accepts.
"""
from __future__ import annotations

from . import _lib


def check_ps_config(cfg, *, server_availability=False, cross_traffic=False, server_workers=False,
                    action_delay=False, balancers_per_pool=0, ps_cores=False) -> None:
    """lbsim_processor_sharing_enable's rule on a config, before any handle exists: LbsimError
    (code ENOTSUP) naming the option the processor-sharing dynamics have no code for.  ps_cores
    (per-server core counts) refuses nothing: they compose with everything a
    processor-sharing handle accepts."""
    no = None
    if cfg.assign_policy == _lib.POLICIES.index("alias"):
        no = "assign_policy ALIAS"
    elif cfg.arrival_source == _lib.ARRIVAL_TRACE:
        no = "arrival_source TRACE"
    elif cfg.lost_fin_prob > 0:
        no = "lost_fin_prob > 0"
    elif cfg.fail_prob > 0:
        no = "fail_prob > 0"
    elif cfg.reservoir_mode != 0:
        no = "reservoir_mode VPP"
    elif cfg.n_flow_on_mode != 0:
        no = "n_flow_on_mode VPP"
    elif cfg.duration_mode != 0:
        no = "duration_mode SERVICE"
    elif cfg.next_step_reset:
        no = "next_step_reset"
    elif server_availability:
        no = "server availability"
    elif cross_traffic:
        no = "cross traffic"
    elif server_workers:
        no = "server workers"
    elif action_delay:
        no = "action delay"
    elif balancers_per_pool:
        no = "server pools"
    if no is not None:
        raise _lib.LbsimError(_lib.ENOTSUP, f"processor sharing with {no}: not supported")
