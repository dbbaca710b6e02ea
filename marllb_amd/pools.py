"""Shared server pools: several learning balancers in front of one set of servers.

VecLoadBalanceEnv(B, S, balancers_per_pool=A) keeps the flat (B, S, ...) shapes: env cA + a is
balancer a of pool c.  VecServerPoolEnv is the thin MARL view of the same env, shaped
(pools, balancers, servers): one observation, action row and reward per balancer, one done flag per
pool, the physical servers' true state for a centralised critic, and what the other balancers put
on every server.  check_pool_config states, without a device, what lbsim_server_pool_enable
accepts.
"""
from __future__ import annotations

from . import _lib

MAX_BALANCERS = 8   # kPoolMaxBalancers
MAX_SERVERS = 16    # kPoolMaxServers


def check_pool_config(cfg, balancers: int, *, flow_stats=False, server_availability=False,
                      cross_traffic=False, server_workers=False, action_delay=False,
                      pool_discipline="fifo") -> None:
    """lbsim_server_pool_enable's rule on a config, before any handle exists: ValueError for a
    pool size outside [1, 8] or one that does not divide num_envs and env_id_offset; LbsimError
    (code ENOTSUP) naming the option the pool dynamics have no code for.  pool_discipline "ps"
    (lbsim_server_pool_enable_ps) accepts exactly the same configs; any other
    value than "fifo" or "ps" is a ValueError."""
    if pool_discipline not in ("fifo", "ps"):
        raise ValueError(f"Unknown pool_discipline: {pool_discipline}")
    A = int(balancers)
    if A < 1 or A > MAX_BALANCERS:
        raise ValueError(f"server pools: balancers must be in [1, {MAX_BALANCERS}] (got {A})")
    if cfg.num_envs % A != 0:
        raise ValueError(f"server pools: num_envs = {cfg.num_envs} is no multiple of balancers = {A}")
    if cfg.env_id_offset % A != 0:
        raise ValueError(f"server pools: env_id_offset = {cfg.env_id_offset} is no multiple of "
                         f"balancers = {A} (a pool never straddles a shard)")
    no = None
    if cfg.num_servers > MAX_SERVERS:
        no = "num_servers > 16"
    elif cfg.assign_policy == _lib.POLICIES.index("alias"):
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
    elif flow_stats:
        no = "flow statistics"
    elif server_availability:
        no = "server availability"
    elif cross_traffic:
        no = "cross traffic"
    elif server_workers:
        no = "server workers"
    elif action_delay:
        no = "action delay"
    if no is not None:
        raise _lib.LbsimError(_lib.ENOTSUP, f"server pools with {no}: not supported")


class VecServerPoolEnv:
    """num_pools pools of num_balancers balancers, each pool in front of its own num_servers
    physical FIFO servers, stepped together on one GPU.

    reset()        -> obs (C, A, S, 11) f32 cuda tensor
    step(actions)  -> obs, rewards (C, A) f32, done (C,) bool, info; actions (C, A, S) as
                      VecLoadBalanceEnv's; info['team_reward'] = rewards.mean(1)
    true_state()   -> (C, S, 8): the physical servers (ground-truth columns; column 1 is 0)
    others_load()  -> (C, A, S): the flows the OTHER balancers have on each server
    Every other keyword goes to VecLoadBalanceEnv; .env is that env (set_rates, seed, ...).
    pool_discipline="ps" (DESIGN.md §3.24): the physical servers are processor-sharing ones
    (pool_ps_cores=..., set_pool_ps_cores / get_pool_ps_cores / clear_pool_ps_cores /
    pool_ps_state forwarded); true_state() is then (C, S, 5), the leader's pool_ps_state() rows
    with column 1 set to 0, and others_load() their column 1.
    """

    def __init__(self, num_pools: int, num_balancers: int, num_servers: int = 4, **kwargs):
        from .env import VecLoadBalanceEnv
        C, A, S = int(num_pools), int(num_balancers), int(num_servers)
        if C < 1:
            raise ValueError(f"need num_pools >= 1 (got {num_pools})")
        if A < 1 or A > MAX_BALANCERS:
            raise ValueError(f"num_balancers must be in [1, {MAX_BALANCERS}] (got {num_balancers})")
        if "balancers_per_pool" in kwargs:
            raise ValueError("balancers_per_pool is num_balancers here")
        self.num_pools, self.num_balancers, self.num_servers = C, A, S
        self.env = VecLoadBalanceEnv(C * A, S, balancers_per_pool=A, **kwargs)

    def _actions(self, actions):
        import torch
        a = torch.as_tensor(actions)
        want = (self.num_pools, self.num_balancers, self.num_servers)
        if tuple(a.shape) != want:
            raise ValueError(f"actions: expected shape {want}, got {tuple(a.shape)}")
        return a.reshape(self.num_pools * self.num_balancers, self.num_servers)

    def _view(self, obs):
        return obs.view(self.num_pools, self.num_balancers, self.num_servers, obs.shape[-1])

    def reset(self, pool_mask=None):
        """Reset every pool, or those with pool_mask[c] true ((C,) bool / uint8)."""
        if pool_mask is None:
            return self._view(self.env.reset())
        import torch
        m = torch.as_tensor(pool_mask)
        if m.numel() != self.num_pools:
            raise ValueError(f"pool_mask must have num_pools={self.num_pools} entries, got "
                             f"{m.numel()}")
        m = m.reshape(-1, 1).to(torch.uint8).expand(-1, self.num_balancers).reshape(-1)
        return self._view(self.env.reset(mask=m))

    def step(self, actions, **kwargs):
        obs, rew, done, info = self.env.step(self._actions(actions), **kwargs)
        C, A = self.num_pools, self.num_balancers
        rewards = rew.view(C, A)
        info = dict(info)
        info["team_reward"] = rewards.mean(1)
        for k in ("episode_length", "episode_return"):
            if k in info:
                info[k] = info[k].view(C, A)
        if "assign_counts" in info:
            info["assign_counts"] = info["assign_counts"].view(C, A, self.num_servers)
        # ep_step is equal across a pool, so its members are done together
        return self._view(obs), rewards, done.view(C, A)[:, 0], info

    def true_state(self):
        """(C, S, 8) f32: the pool leader's ground-truth rows -- the physical queue length, busy,
        cpu, wait_s, backlog_s, up, capacity -- with column 1 (n_hidden, a per-member number:
        others_load) set to 0.  On a pool of processor-sharing servers (pool_discipline="ps"):
        (C, S, 5) f32, the leader's pool_ps_state() rows -- n, n_others, busy_cores, work_s,
        drain_s (env.POOL_PS_STATE_COLUMNS) -- with column 1 (n_others) set to 0."""
        gt = self._truth()
        t = gt.view(self.num_pools, self.num_balancers, self.num_servers, gt.shape[-1])[:, 0].clone()
        t[:, :, 1] = 0.0
        return t

    def _truth(self):
        # a PS pool's privileged rows are pool_ps_state()'s (C, S, 5): n, n_others, busy_cores,
        # work_s, drain_s -- column 1 the per-member number there too
        if self.env.pool_discipline == "ps":
            return self.env.pool_ps_state()
        return self.env.ground_truth()

    # ---- pools of processor-sharing servers (pool_discipline="ps"): VecLoadBalanceEnv's
    def set_pool_ps_cores(self, cores) -> None:
        self.env.set_pool_ps_cores(cores)

    def get_pool_ps_cores(self):
        return self.env.get_pool_ps_cores()

    def clear_pool_ps_cores(self) -> None:
        self.env.clear_pool_ps_cores()

    def pool_ps_state(self, out=None):
        return self.env.pool_ps_state(out)

    def others_load(self):
        """(C, A, S) f32: the flows in flight on each server that OTHER balancers of the pool
        forwarded -- exactly the error of each balancer's own queue estimate (column 0).  Column 1
        of ground_truth() (n_hidden), or of pool_ps_state() (n_others) on a pool of
        processor-sharing servers."""
        gt = self._truth()
        return gt.view(self.num_pools, self.num_balancers, self.num_servers, gt.shape[-1])[..., 1].clone()

    def close(self) -> None:
        self.env.close()
