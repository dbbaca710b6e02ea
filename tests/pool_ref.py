"""The reference of shared server pools: DESIGN.md §3.21 on top of tests.flowsim_ref.FlowSim.

Written from §3.21's text, not from the kernel.  A pool is A FlowSim members used for their
arrival streams alone (each exactly the stream the member would have as an env of its own: its
own gid, episode, arrival index and mean gap) and one set of S physical queues, plain lists of
(tc, ta, owner), oldest first, times absolute int64 us since the reset.  One event loop: the
completions due no later than the pool's next arrival go first (earliest first, ties to the
lowest server), then that arrival, the smallest next arrival time over the members, ties to the
lowest member.  A member's arrival is assigned by its own weights and its OWN flows in flight;
a server is eligible while its PHYSICAL queue is below Q.

step() reports per member what FlowSim reports per env; completed is [(server, ta, tc, owner)] in
completion order.
"""
import numpy as np

from tests.flowsim_ref import FlowSim, _F32

POLICIES = ("sed", "sed2", "lsq", "lsq2")


class PoolStepResult:
    def __init__(self, assigned, dropped, completed):
        self.assigned, self.dropped, self.completed = assigned, dropped, completed

    def fct(self, a, s):
        """tc - ta of member a's flows that server s completed, in its FIFO order."""
        return [tc - ta for (sv, ta, tc, own) in self.completed if sv == s and own == a]

    def tc(self, a, s):
        return [tc for (sv, ta, tc, own) in self.completed if sv == s and own == a]


class PoolSim:
    """One pool.  gid0: the first member's global env id (member a is gid0 + a); rates: (A,)
    arrivals / s, one per member; server_rates: mu_s of the physical servers."""

    def __init__(self, seed, gid0, A, S, Q, policy, rates, server_rates, dt=0.25, warmup_steps=8):
        assert policy in POLICIES and len(rates) == A and len(server_rates) == S
        self.A, self.S, self.Q, self.policy = int(A), int(S), int(Q), policy
        self.members = [FlowSim(seed, gid0 + a, S, Q, policy, rates[a], server_rates, dt=dt,
                                warmup_steps=0) for a in range(A)]
        self.dt = self.members[0].dt
        self.svc_scale = self.members[0].svc_scale
        self.warmup_steps = int(warmup_steps)
        self.ties = 0  # arrivals of two members at the same us (for the reach test)

    def set_rate(self, a, rate):
        """Member a's arrival rate from now on: the arrival already drawn keeps its time, every
        later gap is drawn at the new mean."""
        m = self.members[a]
        m._arrival(m.k)
        del m._ta[m.k + 1:], m._work[m.k + 1:], m._u2[m.k + 1:]
        m.mean_gap = _F32(1e6 / float(_F32(rate)))

    # ---------------------------------------------------------------- reset
    def reset(self):
        """Every member: episode += 1, arrival index 0; time 0, empty queues; then the shared
        warm-up at weights 1.0.  Returns the warm-up's results."""
        for m in self.members:
            m.episode += 1
            m._ta, m._work, m._u2 = [], [], []
            m.k = 0
        self.step_no = 0
        self.queues = [[] for _ in range(self.S)]
        ones = np.ones((self.A, self.S), _F32)
        return [self.step(ones) for _ in range(self.warmup_steps)]

    # ---------------------------------------------------------------- one step
    def own(self, a, s):
        return sum(1 for e in self.queues[s] if e[2] == a)

    def _pop_due(self, t, done):
        while True:
            best = -1
            for s, q in enumerate(self.queues):
                if q and q[0][0] <= t and (best < 0 or q[0][0] < self.queues[best][0][0]):
                    best = s
            if best < 0:
                return
            tc, ta, own = self.queues[best].pop(0)
            done.append((best, ta, tc, own))

    def _score(self, a, s, w):
        n = self.own(a, s)
        if self.policy in ("lsq", "lsq2"):
            return float(n)
        return _F32(float(n + 1) / (float(w[s]) + 1e-9))

    def _choose(self, a, u2, w):
        S = self.S
        free = [len(q) < self.Q for q in self.queues]  # the physical length
        if self.policy in ("sed2", "lsq2"):
            h1, h2 = ((u2 >> 16) * S) >> 16, ((u2 & 0xFFFF) * S) >> 16
            if free[h1] and free[h2]:
                return h2 if self._score(a, h2, w) < self._score(a, h1, w) else h1
            return h1 if free[h1] else (h2 if free[h2] else -1)
        h = (u2 * S) >> 32
        chosen, best = (h, self._score(a, h, w)) if free[h] else (-1, None)
        for s in range(S):
            if free[s]:
                sc = self._score(a, s, w)
                if chosen < 0 or sc < best:
                    chosen, best = s, sc
        return chosen

    def next_member(self):
        t = [m._arrival(m.k) for m in self.members]
        a = min(range(self.A), key=lambda i: (t[i], i))
        return a, t[a], sum(1 for x in t if x == t[a]) > 1

    def step(self, weights):
        w = np.asarray(weights, dtype=_F32)
        assert w.shape == (self.A, self.S) and np.isfinite(w).all()
        end = (self.step_no + 1) * self.dt
        assigned = np.zeros((self.A, self.S), np.int64)
        dropped = np.zeros(self.A, np.int64)
        done = []
        self.events = []  # (ta, member, server or -1, physical length there, own count there)
        while True:
            a, ta, tie = self.next_member()
            if ta >= end:
                break
            self.ties += int(tie)
            m = self.members[a]
            self._pop_due(ta, done)
            s = self._choose(a, m._u2[m.k], w[a])
            if s < 0:
                dropped[a] += 1
                self.events.append((ta, a, -1, [len(q) for q in self.queues],
                                    [self.own(a, x) for x in range(self.S)]))
            else:
                q = self.queues[s]
                start = max(ta, q[-1][0]) if q else ta
                svc = max(1, int(_F32(m._work[m.k]) * self.svc_scale[s]))
                q.append((start + svc, ta, a))
                assigned[a, s] += 1
            m.k += 1
        self._pop_due(end, done)
        self.step_no += 1
        return PoolStepResult(assigned, dropped, done)

    # ---------------------------------------------------------------- after a step
    def in_flight(self):
        """(A, S): each member's own flows in flight."""
        return [[self.own(a, s) for s in range(self.S)] for a in range(self.A)]

    def physical(self):
        return [len(q) for q in self.queues]
