"""Ground-truth server state in numpy, written from the rule's table and not
from the kernel: a row of 8 f32 per (env, server) from a parsed state snapshot
(tests/statelayout.py), the worker counts, the rates and the availability the existing getters
report.  Every operation is an exact integer-to-float conversion or one f32 operation, so the
device's rows are these rows bit for bit.

    0 n_total    flows in the system (hidden ones and flows in service included)
    1 n_hidden   hidden cross-traffic flows among them (minus the lost_on word)
    2 busy       min(n, c)
    3 cpu        busy / c
    4 wait_s     n < c ? 0 : max(0, tc at queue position n - c), us * 1e-6
    5 backlog_s  n == 0 ? 0 : max(0, tc at queue position n - 1), us * 1e-6
    6 up         0 where the down flag is set
    7 capacity   c * mu
"""
import numpy as np

from tests import statelayout

COLS = 8
NAMES = ("n_total", "n_hidden", "busy", "cpu", "wait_s", "backlog_s", "up", "capacity")
F32 = np.float32


def queue_tc(d, B, S, Q):
    """queues[b][s]: the completion times of the queued flows, by position from the head."""
    hc = d["hc"].reshape(B, S)
    ring = statelayout.live_ring(d, B, S, Q).view(np.int32).reshape(B, S, Q, 2)
    out = []
    for b in range(B):
        row = []
        for s in range(S):
            h, n = int(hc[b, s] & 0x7FFF), int(hc[b, s] >> 16)
            row.append([int(ring[b, s, (h + i) % Q, 0]) for i in range(n)])
        out.append(row)
    return out


def ground_truth(d, B, S, Q, mu, workers=None, hidden=False, up=None):
    """(B, S, 8) f32.  d: the parsed state; mu (B, S) f32: the rate of one worker at each env's
    next step; workers (B, S) ints or None (one each); hidden: a cross-traffic handle (its lost_on
    words are minus the hidden flows); up (B, S) or None: the state's own down section, and every
    server up where it has none."""
    c = np.ones((B, S), np.int32) if workers is None else np.asarray(workers).reshape(B, S)
    c = c.astype(np.int32)
    mu = np.asarray(mu, F32).reshape(B, S)
    n = (d["hc"].reshape(B, S) >> 16).astype(np.int32)
    if up is None:
        up = d["down"].reshape(B, S) == 0 if "down" in d else np.ones((B, S), bool)
    up = np.asarray(up).reshape(B, S) != 0
    tcs = queue_tc(d, B, S, Q)
    wait = np.zeros((B, S), np.int32)
    backlog = np.zeros((B, S), np.int32)
    for b in range(B):
        for s in range(S):
            q, k = tcs[b][s], int(c[b, s])
            if len(q) >= k:
                wait[b, s] = max(0, q[len(q) - k])
            if q:
                backlog[b, s] = max(0, q[-1])
    busy = np.minimum(n, c)
    out = np.zeros((B, S, COLS), F32)
    out[..., 0] = n.astype(F32)
    if hidden:
        out[..., 1] = (-d["lost_on"].view(np.int32).reshape(B, S)).astype(F32)
    out[..., 2] = busy.astype(F32)
    out[..., 3] = busy.astype(F32) / c.astype(F32)
    out[..., 4] = wait.astype(F32) * F32(1e-6)
    out[..., 5] = backlog.astype(F32) * F32(1e-6)
    out[..., 6] = up.astype(F32)
    out[..., 7] = c.astype(F32) * mu
    return out


def reach(d, B, S, Q, workers=None, hidden=False):
    """What a state exercises, counted on the reference's own data."""
    c = np.ones((B, S), np.int64) if workers is None else np.asarray(workers).reshape(B, S)
    hc = d["hc"].reshape(B, S)
    n, head = (hc >> 16).astype(np.int64), (hc & 0x7FFF).astype(np.int64)
    r = {"multi_wait": int(((c > 1) & (n >= c) & (n - c > 0)).sum()),
         "wraps": int((head + n > Q).sum()), "full": int((n == Q).sum()),
         "empty": int((n == 0).sum()),
         "hidden": int((d["lost_on"].view(np.int32) < 0).sum()) if hidden else 0,
         "down": int((d["down"] != 0).sum()) if "down" in d else 0}
    return r


def parse_env(env, cross=False):
    """The parsed state of a VecLoadBalanceEnv (a cross-traffic handle keeps its lost_on section
    where a leak handle has it, an availability handle its down section where failures have it)."""
    c = env.cfg
    return statelayout.parse(env.handle.state_bytes(), c.num_envs, c.num_servers, c.queue_capacity,
                             bool(c.normalize_obs), c.fail_prob > 0 or env.server_availability,
                             leak=statelayout.has_leak(c) or cross,
                             dur_plane=statelayout.has_dur_plane(c),
                             split_P=statelayout.split_p(c))


def of_env(env, cross=False, workers=False, getter_rates=True):
    """The reference rows of a VecLoadBalanceEnv's state now -> ((B, S, 8) f32, the parsed state).
    getter_rates False: mu from the config (a handle whose rates were never set or read), else
    from env.rates, which reports the rates of each env's next step."""
    c = env.cfg
    B, S, Q = c.num_envs, c.num_servers, c.queue_capacity
    d = parse_env(env, cross)
    if getter_rates:
        mu = env.rates[1].cpu().numpy()
    else:
        mu = np.tile(np.array([c.server_rate[s] for s in range(S)], F32), (B, 1))
    w = env.get_server_workers().cpu().numpy() if workers else None
    up = env.servers_up().cpu().numpy() if env.server_availability else None
    return ground_truth(d, B, S, Q, mu, w, hidden=cross, up=up), d
