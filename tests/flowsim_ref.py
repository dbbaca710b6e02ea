"""An independent reference of the flow dynamics: a plain event simulator of ONE env.

Written from the text of DESIGN.md §3.2 (randomness), §3.3 (one step), §3.6 (TRACE rows) and §3.7
(reset), not from the oracle's sim_step or the kernels, and built differently on purpose:

- times are absolute int64 us since the reset; nothing is ever rebased;
- a server is a plain Python list of (tc, ta), oldest first; there is no ring and no head word;
- the arrival stream of an episode is computed ahead, in blocks, as absolute times (arrivals do
  not depend on the queues);
- the only step structure is that the weights in force change at k * dt: step k owns the
  arrivals with k dt <= ta < (k + 1) dt and the completions with k dt < tc <= (k + 1) dt.

Shared with the simulator under test, because they are pinned elsewhere: Philox4x32-10
(tests/policy_ref.py, against the Random123 vectors), the fixed logarithm polynomial (oracle_logf,
|err| < 1e-6 against math.log) and gen_alias (bit-exact against the reference's Python on 137
tables).  Nothing else of oracle/ or marllb_amd/csrc is imported.

Not modelled: the reservoirs and Algorithm R, the observation columns and the reward (pinned by
the goldens), lost FINs, server failures, next-step resets, NaN weights.
"""
import numpy as np

import oracle
from tests.policy_ref import philox4x32_10

POLICIES = ("sed", "sed2", "lsq", "lsq2", "alias")
_BLOCK = 256  # arrivals drawn ahead at a time
_F32 = np.float32
_2M24 = _F32(2.0 ** -24)


def _neg_log(u):
    """-ln u of f32 uniforms, by the fixed polynomial (f32 out)."""
    logf = oracle.load().oracle_logf
    return np.array([-logf(float(x)) for x in u], dtype=_F32)


def _uniform(r):
    """§3.2: u = ((r >> 8) + 1) * 2^-24 in (0, 1], exact in f32."""
    return ((r >> np.uint32(8)) + np.uint32(1)).astype(_F32) * _2M24


class StepResult:
    """What one step did: assigned (S,) flows per server, dropped, completed [(server, ta, tc)] in
    completion order (ties: lowest server)."""

    def __init__(self, assigned, dropped, completed):
        self.assigned, self.dropped, self.completed = assigned, dropped, completed

    def fct(self, s):
        """tc - ta of the flows server s completed, in its FIFO order."""
        return [tc - ta for (sv, ta, tc) in self.completed if sv == s]

    def tc(self, s):
        return [tc for (sv, ta, tc) in self.completed if sv == s]


class FlowSim:
    """One env.  seed: the 64-bit key; gid: the global env id; rate: arrivals / s; server_rates:
    mu_s; trace: a marllb_amd.trace.Trace (then `rate` is unused).  reset() starts the next
    episode and runs the warm-up; step(weights) runs one step at those weights."""

    def __init__(self, seed, gid, S, Q, policy, rate, server_rates, dt=0.25, warmup_steps=8,
                 trace=None):
        assert policy in POLICIES and len(server_rates) == S
        self.key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        self.gid, self.S, self.Q, self.policy = int(gid), int(S), int(Q), policy
        self.dt = int(round(float(_F32(dt)) * 1e6))
        self.warmup_steps = int(warmup_steps)
        # f32(1e6 / rate) of the f32 rates: the config holds floats
        self.mean_gap = _F32(1e6 / float(_F32(rate)))
        self.svc_scale = [_F32(1e6 / float(_F32(m))) for m in server_rates]
        self.trace = trace
        self.episode = 0
        self.alias_ties = 0

    # ---------------------------------------------------------------- arrivals (§3.2, §3.6)
    def _draw_block(self):
        """The next _BLOCK arrivals of the episode: absolute times, work, hash words."""
        k0 = len(self._ta)
        k = np.arange(k0, k0 + _BLOCK, dtype=np.uint64)
        ctr = np.stack([k, np.full_like(k, self.gid), np.full_like(k, self.episode),
                        np.full_like(k, 1 << 24)], axis=-1)
        d = philox4x32_10(ctr, np.array(self.key, dtype=np.uint64))
        if self.trace is not None:
            R = self.trace.rows
            row = (self.gid * 7919 + (self.episode - 1) * 1000003 + k.astype(object)) % R
            row = np.array(row, dtype=np.int64)
            gap = self.trace.gap_us[row].astype(np.int64)
            work = self.trace.work[row].astype(_F32)
        else:
            gap = (_neg_log(_uniform(d[:, 0])) * self.mean_gap).astype(np.int32).astype(np.int64)
            work = _neg_log(_uniform(d[:, 1]))
        last = self._ta[-1] if k0 else 0
        self._ta.extend((last + np.cumsum(gap)).tolist())
        self._work.extend(work)
        self._u2.extend(d[:, 2].tolist())

    def _arrival(self, k):
        while k >= len(self._ta):
            self._draw_block()
        return self._ta[k]

    # ---------------------------------------------------------------- reset (§3.7)
    def reset(self):
        """episode += 1, arrival index 0, time 0, empty queues, then the warm-up steps at weights
        1.0.  Returns the warm-up's StepResults."""
        self.episode += 1
        self._ta, self._work, self._u2 = [], [], []
        self.k = 0          # the index of the next arrival
        self.step_no = 0    # steps since the reset: the weights change at step_no * dt
        self.queues = [[] for _ in range(self.S)]
        ones = np.ones(self.S, _F32)
        return [self.step(ones) for _ in range(self.warmup_steps)]

    # ---------------------------------------------------------------- one step (§3.3)
    def _pop_due(self, t, done):
        """Completions with tc <= t, earliest first, ties to the lowest server."""
        while True:
            best = -1
            for s, q in enumerate(self.queues):
                if q and q[0][0] <= t and (best < 0 or q[0][0] < self.queues[best][0][0]):
                    best = s
            if best < 0:
                return
            tc, ta = self.queues[best].pop(0)
            done.append((best, ta, tc))

    def _score(self, s, w):
        n = len(self.queues[s])
        if self.policy in ("lsq", "lsq2"):
            return float(n)  # exact in f32
        return _F32(float(n + 1) / (float(w[s]) + 1e-9))

    def _choose(self, u2, w, alias_table):
        """The server of one arrival, or -1: dropped."""
        S, Q = self.S, self.Q
        free = [len(q) < Q for q in self.queues]
        if self.policy == "alias":
            act, odd, alias = alias_table
            n = len(act)
            if n == 0:
                return -1
            rn = _F32(u2 >> 8) * _2M24 * _F32(n)  # U in [0, 1): the word's top 24 bits
            bucket = min(int(rn), n - 1)
            self.alias_ties += int(rn - _F32(bucket) == odd[bucket])  # for the tests: a tie was met
            pick = int(alias[bucket]) if rn - _F32(bucket) > odd[bucket] else bucket
            return act[pick] if free[act[pick]] else -1  # no eligibility test: full -> drop
        if self.policy in ("sed2", "lsq2"):
            h1, h2 = ((u2 >> 16) * S) >> 16, ((u2 & 0xFFFF) * S) >> 16
            if free[h1] and free[h2]:
                return h2 if self._score(h2, w) < self._score(h1, w) else h1
            return h1 if free[h1] else (h2 if free[h2] else -1)
        h = (u2 * S) >> 32
        chosen, best = (h, self._score(h, w)) if free[h] else (-1, None)
        for s in range(S):
            if free[s]:
                sc = self._score(s, w)
                if chosen < 0 or sc < best:
                    chosen, best = s, sc
        return chosen

    def step(self, weights):
        w = np.asarray(weights, dtype=_F32)
        assert w.shape == (self.S,) and np.isfinite(w).all()
        end = (self.step_no + 1) * self.dt
        alias_table = None
        if self.policy == "alias":  # over the servers with w > 0, rebuilt every step
            act = [s for s in range(self.S) if w[s] > 0]
            odd, alias = oracle.gen_alias(w[act]) if act else (np.zeros(0), np.zeros(0, np.int32))
            alias_table = (act, odd.astype(_F32), alias)
        assigned, dropped, done = np.zeros(self.S, np.int64), 0, []
        while self._arrival(self.k) < end:
            ta = self._ta[self.k]
            self._pop_due(ta, done)  # a completion due no later than the arrival goes first
            s = self._choose(self._u2[self.k], w, alias_table)
            if s < 0:
                dropped += 1
            else:
                q = self.queues[s]
                start = max(ta, q[-1][0]) if q else ta
                svc = max(1, int(_F32(self._work[self.k]) * self.svc_scale[s]))
                q.append((start + svc, ta))
                assigned[s] += 1
            self.k += 1
        self._pop_due(end, done)
        self.step_no += 1
        return StepResult(assigned, dropped, done)

    # ---------------------------------------------------------------- after a step
    def in_flight(self):
        return [len(q) for q in self.queues]

    def next_arrival(self):
        """Absolute us of the arrival drawn but not yet assigned."""
        return self._arrival(self.k)
