"""The reference of shared server pools with processor-sharing servers: DESIGN.md §3.24.

Written from §3.24's text, not from the kernel, on top of tests.pool_ref.PoolSim's member streams
(each member a FlowSim used for its arrivals alone) with the server of tests.ps_cores_ref.PSCoresSim
restated over entries that carry their owner.  Times are absolute int64 us since the reset, nothing
is rebased; a physical server is the clock words V, acc, t_last, c cores and a plain list of
(tag, ta, owner) in non-decreasing tag order, a new entry after every equal tag:

  advance(s, t), d = t - t_last:  n = 0: acc = 0.  1 <= n <= c: V += d, acc = 0.
                                  n > c: acc += c d; V += acc // n; acc %= n.  Then t_last = t.
  next completion of s (n > 0):   n <= c: t_last + (tag_head - V)
                                  n > c:  x = (tag_head - V) n - acc; t_last + max(0, ceil(x / c))
  member a's arrival at ta on s (after the pops due by ta):  advance(s, ta); tag = V + svc; insert
  completion (s, tc):  advance(s, tc); V == tag_head, 0 <= acc < c (asserted); pop the head; the
                       sample tc - ta into the reservoir of (owner, s), the slot by Algorithm R with
                       the owner's reservoir-stream draw at the owner's count
  step end:  advance(s, end) for every server

The §3.23 invariants are asserted at every event: V == tag_head at a completion, the carry's
range, that the completion time is the smallest us at which V reaches the head's tag, and the
ledger (between two events W = sum(tag - V) - acc falls by exactly min(n, c) d, plus the carry an
advance with n <= c drops).

step() reports per member what PoolSim reports; completed is [(server, ta, tc, owner)] in
completion order (earliest first, ties to the lowest server; a server's own in queue order).
self.reach counts what a scenario met (tests/test_pool_ps.py asserts on it).
"""
import bisect

import numpy as np

from tests.pool_ref import PoolSim, PoolStepResult
from tests.ps_ref import K, stream_slot

_F32 = np.float32
INT32_MAX = 0x7FFFFFFF
REACH = ("ties", "head_before_other", "shift_gt8_mixed", "equal_tags_other_owner_same_us",
         "drop_full_own_zero", "carried_n_gt_c", "at_ta", "at_dt", "acc_left", "inserts")


class PoolPSSim(PoolSim):
    def __init__(self, *args, cores=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.cores = [1] * self.S if cores is None else [int(c) for c in cores]
        assert len(self.cores) == self.S and all(1 <= c <= 64 for c in self.cores)
        self.cores_changed = False
        self.reach = {k: 0 for k in REACH}
        self.key = self.members[0].key

    def set_cores(self, cores):
        """New counts from the next step (or reset) on: entries keep their remaining tags, the
        carry stays what it is."""
        cores = [int(c) for c in cores]
        assert len(cores) == self.S and all(1 <= c <= 64 for c in cores)
        if cores != self.cores:
            self.cores, self.cores_changed = cores, True

    # ---------------------------------------------------------------- reset
    def reset(self):
        A, S = self.A, self.S
        self.V, self.acc, self.t_last = [0] * S, [0] * S, [0] * S
        self.res = [[[None] * K for _ in range(S)] for _ in range(A)]  # (fct us, ts ms)
        self.res_count = [[0] * S for _ in range(A)]
        self.big = [[False] * S for _ in range(A)]
        self.last_done = [None] * S  # (tc, tag, owner) of the server's last completion
        self.assigned_log = []
        return super().reset()

    # ---------------------------------------------------------------- the server's rule
    def _ledger(self, s):
        return sum(e[0] - self.V[s] for e in self.queues[s]) - self.acc[s]

    def _advance(self, s, t):
        n, c = len(self.queues[s]), self.cores[s]
        d = t - self.t_last[s]
        assert d >= 0
        before, dropped = self._ledger(s), 0
        if n == 0:
            self.acc[s] = 0
        elif n <= c:
            dropped = self.acc[s]
            self.V[s] += d
            self.acc[s] = 0
        else:
            self.acc[s] += c * d
            self.V[s] += self.acc[s] // n
            self.acc[s] %= n
        self.t_last[s] = t
        if n > 0:
            assert self._ledger(s) == before - min(n, c) * d + dropped, ("ledger", s, t)
            assert dropped < c or self.cores_changed, ("dropped remainder", s, dropped, c)

    def _tc(self, s):
        q, c = self.queues[s], self.cores[s]
        n, left = len(q), q[0][0] - self.V[s]
        if n <= c:
            return self.t_last[s] + left
        x = left * n - self.acc[s]
        return self.t_last[s] + (0 if x <= 0 else -(-x // c))

    def _sample(self, a, s, ta, tc):
        cnt = self.res_count[a][s]
        m = self.members[a]
        slot = stream_slot(self.key, m.gid, m.episode, s, cnt)
        if slot >= 0:
            self.res[a][s][slot] = (tc - ta, tc // 1000)  # the pool's clock
            self.big[a][s] |= tc - ta >= (1 << 25) - 1
        self.res_count[a][s] = cnt + 1

    def _pop_due(self, t, done, at_arrival=True):
        r = self.reach
        while True:
            due = [(self._tc(s), s) for s, q in enumerate(self.queues) if q]
            due = [x for x in due if x[0] <= t]
            if not due:
                return
            tc, s = min(due)  # the earliest, ties to the lowest server
            r["at_ta" if at_arrival else "at_dt"] += tc == t
            n, c = len(self.queues[s]), self.cores[s]
            assert tc >= self.t_last[s]
            if n > c and tc > self.t_last[s]:  # the smallest such us: one earlier V is short
                assert self.V[s] + (self.acc[s] + c * (tc - 1 - self.t_last[s])) // n \
                    < self.queues[s][0][0], ("not the smallest t", s, tc)
            if n <= c and tc > self.t_last[s]:
                assert self.V[s] + (tc - 1 - self.t_last[s]) < self.queues[s][0][0]
            self._advance(s, tc)
            tag, ta, own = self.queues[s][0]
            assert self.V[s] == tag, (self.V[s], tag)
            assert 0 <= self.acc[s] < max(c, 1) and (c > 1 or self.acc[s] == 0), (self.acc[s], c)
            r["acc_left"] += self.acc[s] > 0
            prev = self.last_done[s]
            r["equal_tags_other_owner_same_us"] += (prev is not None and prev[0] == tc
                                                    and prev[1] == tag and prev[2] != own)
            self.last_done[s] = (tc, tag, own)
            self.queues[s].pop(0)
            done.append((s, ta, tc, own))
            self._sample(own, s, ta, tc)

    def _insert(self, s, ta, svc, a):
        """Member a's arrival at ta, needing svc us, onto server s (the pops due by ta are done)."""
        r = self.reach
        self._advance(s, ta)
        q = self.queues[s]
        tag = self.V[s] + svc
        tags = [e[0] for e in q]
        assert tags == sorted(tags)
        at = bisect.bisect_right(tags, tag)
        r["inserts"] += 1
        r["head_before_other"] += at == 0 and len(q) > 0 and q[0][2] != a
        r["shift_gt8_mixed"] += len(q) - at > 8 and len({e[2] for e in q[at:]}) > 1
        q.insert(at, (tag, ta, a))
        self.assigned_log.append((s, ta, svc, a))

    # ---------------------------------------------------------------- one step
    def step(self, weights):
        w = np.asarray(weights, dtype=_F32)
        assert w.shape == (self.A, self.S) and np.isfinite(w).all()
        end = (self.step_no + 1) * self.dt
        assigned = np.zeros((self.A, self.S), np.int64)
        dropped = np.zeros(self.A, np.int64)
        done = []
        self.events = []  # the drops: (ta, member, -1, physical lengths, own counts)
        self.assigned_log = []  # (server, ta, svc, member) of this step's assigned arrivals
        r = self.reach
        while True:
            a, ta, tie = self.next_member()
            if ta >= end:
                break
            self.ties += int(tie)
            r["ties"] += int(tie)
            m = self.members[a]
            self._pop_due(ta, done)
            s = self._choose(a, m._u2[m.k], w[a])
            if s < 0:
                dropped[a] += 1
                phys = [len(q) for q in self.queues]
                own = [self.own(a, x) for x in range(self.S)]
                self.events.append((ta, a, -1, phys, own))
                r["drop_full_own_zero"] += any(p >= self.Q and o == 0 for p, o in zip(phys, own))
            else:
                svc = max(1, int(_F32(m._work[m.k]) * self.svc_scale[s]))
                self._insert(s, ta, svc, a)
                assigned[a, s] += 1
            m.k += 1
        self._pop_due(end, done, at_arrival=False)
        for s in range(self.S):
            self._advance(s, end)
            r["carried_n_gt_c"] += len(self.queues[s]) > self.cores[s] and self.acc[s] != 0
        self.step_no += 1
        return PoolStepResult(assigned, dropped, done)

    # ---------------------------------------------------------------- after a step
    def remaining(self, s):
        """Server s's entries as the state holds them: (tag - V, ta, owner), in tag order."""
        return [(tag - self.V[s], ta, own) for tag, ta, own in self.queues[s]]

    def server_state(self, s):
        """(n, busy cores, unfinished work us, drain us) of physical server s (§3.23's view)."""
        rem = [e[0] for e in self.remaining(s)]
        n, c, acc = len(rem), self.cores[s], self.acc[s]
        work = sum(rem) - (acc if n > c else 0)
        V = t = 0
        for i, tag in enumerate(rem):
            m = n - i
            if m <= c:
                t, acc = t + (tag - V), 0
            else:
                x = (tag - V) * m - acc
                if x > 0:
                    d = -(-x // c)
                    t, acc = t + d, c * d - x
            V = tag
        return n, min(n, c), work, t

    def state_row(self, a, s):
        """lbsim_pool_ps_state's float32 row of member a: n, n - own, busy, work s, drain s."""
        n, busy, work, drain = self.server_state(s)
        sec = lambda us: _F32(min(us, INT32_MAX)) * _F32(1e-6)  # noqa: E731
        return [_F32(n), _F32(n - self.own(a, s)), _F32(busy), sec(work), sec(drain)]
