"""Duration samples at every data ACK: VecLoadBalanceEnv(..., ack_samples=True).

The data plane records a flow_duration sample on every pure ACK after the handshake; with
ack_samples a flow offers its server's duration reservoir one sample per data ACK, its age at that
packet, at times spread evenly over its service interval, instead of one sample at its completion.
check_ack_config states, without a device, what lbsim_ack_samples_enable accepts.
"""
from __future__ import annotations

from . import _lib

MAX_ACKS_LIMIT = 32          # max_acks in [1, 32]
ACK_INTERVAL_LIMIT = 1 << 30  # ack_interval_us in [1, 2^30]
DEFAULT_MAX_ACKS = 8
DEFAULT_ACK_INTERVAL_US = 1000


def ack_count(svc_us: int, ack_us: int, max_acks: int) -> int:
    """k: the data ACKs of a flow of svc_us of service (the rule of csrc/lbsim_acks.h)."""
    return min(int(max_acks), max(1, int(svc_us) // int(ack_us)))


def ack_times(t0: int, svc_us: int, ack_us: int, max_acks: int):
    """The times of a flow's ACKs: t_j = t0 + (svc j) // k, j = 1..k; the last is its completion."""
    k = ack_count(svc_us, ack_us, max_acks)
    return [int(t0) + (int(svc_us) * j) // k for j in range(1, k + 1)]


def check_ack_config(cfg, *, max_acks=DEFAULT_MAX_ACKS, flow_stats=False, server_availability=False,
                     cross_traffic=False, server_workers=False, action_delay=False,
                     balancers_per_pool=0, service_discipline="fifo", workload_tables=False,
                     trace_bank=False, trace_schedule=False) -> None:
    """lbsim_ack_samples_enable's rule on a config, before any handle exists: LbsimError (code
    ENOTSUP) naming the option the ACK dynamics have no code for, or (code EINVAL) max_acks out of
    [1, 32]."""
    if not 1 <= int(max_acks) <= MAX_ACKS_LIMIT:
        raise _lib.LbsimError(_lib.EINVAL, f"ack samples: max_acks must be in [1, {MAX_ACKS_LIMIT}] "
                                           f"(got {int(max_acks)})")
    no = None
    if cfg.lost_fin_prob > 0:
        no = "lost_fin_prob > 0"
    elif cfg.fail_prob > 0:
        no = "fail_prob > 0"
    elif cfg.duration_mode != 0:
        no = "duration_mode SERVICE"
    elif cfg.reservoir_mode != 0:
        no = "reservoir_mode VPP"
    elif cfg.n_flow_on_mode != 0:
        no = "n_flow_on_mode VPP"
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
    elif service_discipline != "fifo":
        no = "processor sharing"
    elif flow_stats:
        no = "flow statistics"
    elif workload_tables:
        no = "workload tables"
    elif trace_bank:
        no = "a trace bank"
    elif trace_schedule:
        no = "a trace schedule"
    if no is not None:
        raise _lib.LbsimError(_lib.ENOTSUP, f"ack samples with {no}: not supported")
