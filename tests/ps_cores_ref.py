"""The reference of processor-sharing servers with several cores: tests.ps_ref.PSSim with
DESIGN.md §3.23 added.

Written from §3.23's text, not from the kernel.  Times stay absolute int64 us, the servers plain
lists, as in PSSim.  Server s has c = cores[s] cores, 1 <= c <= 64; n is the number of its entries:

  advance(s, t), d = t - t_last:  n = 0: acc = 0.  1 <= n <= c: V += d, acc = 0.
                                  n > c: acc += c d; V += acc // n; acc %= n.  Then t_last = t.
  next completion of s (n > 0):   n <= c: t_last + (tag_head - V)
                                  n > c:  x = (tag_head - V) n - acc; t_last + (0 if x <= 0 else
                                          ceil(x / c))
  completion (s, tc):  advance(s, tc); V == tag_head and 0 <= acc < c (asserted); pop the head

Everything else -- arrivals, the sorted insert, the reservoir draw, the step end -- is PSSim's.

Every advance also checks the rule's own ledger: between two events of a server the quantity
W = sum(tag - V) - acc falls by exactly min(n, c) d, and where n <= c it rises by the carry the
advance drops (what a completion left when the server fell to n <= c: less than c core-us).

self.reach counts what a scenario met (tests/test_ps_cores.py asserts on it).

server_state(s) is the privileged view of §3.23: (n, min(n, c), work_us, drain_us).

ExactCoresPS is BruteForcePS's idea for c cores: every flow is served at rate min(n, c) / n, the
remaining work of each flow a fractions.Fraction.
"""
from fractions import Fraction

import numpy as np

from tests.ps_ref import PSSim

_F32 = np.float32
INT32_MAX = 0x7FFFFFFF


class PSCoresSim(PSSim):
    def __init__(self, *args, cores=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.cores = [1] * self.S if cores is None else [int(c) for c in cores]
        assert len(self.cores) == self.S and all(1 <= c <= 64 for c in self.cores)
        self.cores_changed = False
        for k in ("acc_left", "rem_dropped", "zero_delta", "found_n_eq_c", "carried_n_gt_c",
                  "full_drops_multicore", "all_own_core"):
            self.reach[k] = 0

    def set_cores(self, cores):
        """New counts from the next step (or reset) on: entries keep their remaining tags, the
        carry stays what it is."""
        cores = [int(c) for c in cores]
        assert len(cores) == self.S and all(1 <= c <= 64 for c in cores)
        if cores != self.cores:
            self.cores, self.cores_changed = cores, True

    # ---------------------------------------------------------------- the rule
    def _ledger(self, s):
        return sum(tag - self.V[s] for tag, _ in self.queues[s]) - self.acc[s]

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
            self.reach["rem_dropped"] += dropped > 0
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

    def _pop_due(self, t, done, at_arrival=True):
        r = self.reach
        while True:
            due = [(self._tc(s), s) for s, q in enumerate(self.queues) if q]
            due = [x for x in due if x[0] <= t]
            if not due:
                return
            tc, s = min(due)  # the earliest, ties to the lowest server
            r["same_us"] += sum(1 for x in due if x[0] == tc) > 1
            r["at_ta" if at_arrival else "at_dt"] += tc == t
            n, c = len(self.queues[s]), self.cores[s]
            assert tc >= self.t_last[s]
            if n > c and tc > self.t_last[s]:  # the smallest such t: one us earlier V is short
                was = (self.V[s], self.acc[s])
                assert self.V[s] + (self.acc[s] + c * (tc - 1 - self.t_last[s])) // n \
                    < self.queues[s][0][0], ("not the smallest t", s, tc, was)
            r["zero_delta"] += n > c and tc == self.t_last[s]
            self._advance(s, tc)
            tag, ta = self.queues[s][0]
            assert self.V[s] == tag, (self.V[s], tag)
            assert 0 <= self.acc[s] < max(c, 1) and (c > 1 or self.acc[s] == 0), (self.acc[s], c)
            r["acc_left"] += self.acc[s] > 0
            self.queues[s].pop(0)
            done.append((s, ta, tc))
            self.completion_log.append((s, ta, tc, 2 * self.bp_k[s] * self.bp_nmax[s],
                                        not self.queues[s]))
            if not self.queues[s]:
                self.bp_k[s] = self.bp_nmax[s] = 0
            self._sample(s, ta, tc)

    def _insert(self, s, ta, svc):
        n, c = len(self.queues[s]), self.cores[s]
        self.reach["found_n_eq_c"] += n == c
        self.reach["all_own_core"] += n < c
        super()._insert(s, ta, svc)

    def step(self, weights):
        full = self.reach["full_drops"]
        res = super().step(weights)
        if max(self.cores) > 1:
            self.reach["full_drops_multicore"] += self.reach["full_drops"] - full
        for s in range(self.S):
            self.reach["carried_n_gt_c"] += (len(self.queues[s]) > self.cores[s]
                                             and self.acc[s] != 0)
        return res

    # ---------------------------------------------------------------- after a step
    def server_state(self, s):
        """(n, busy cores, unfinished work us, drain us) of server s as it stands: the work is the
        sum of the remaining tags less the carry where n > c; the drain is the last completion
        time the rule gives from {V = 0, acc, t_last = 0} over the remaining tags, popping one by
        one with no further arrival."""
        rem = [r for r, _ in self.remaining(s)]
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

    def state_row(self, s):
        """server_state as lbsim_ps_server_state's float32 row: us to seconds as f32(us) * 1e-6f."""
        n, busy, work, drain = self.server_state(s)
        sec = lambda us: _F32(min(us, INT32_MAX)) * _F32(1e-6)  # noqa: E731
        return [_F32(n), _F32(busy), sec(work), sec(drain)]


class ExactCoresPS:
    """One exact processor-sharing server of c cores: arrive(ta, svc) in arrival order, then
    finish().  With n flows each is served at rate min(n, c) / n.  done: [(ta, tc)], tc a
    Fraction, in completion order (ties: the earlier arrival)."""

    def __init__(self, c):
        self.c = int(c)
        self.t = Fraction(0)
        self.flows = []  # [remaining, ta, seq]
        self.done = []
        self.seq = 0

    def _rate(self):
        n = len(self.flows)
        return Fraction(min(n, self.c), n)

    def _run_to(self, t):
        while self.flows:
            f = min(self.flows, key=lambda x: (x[0], x[2]))
            tc = self.t + f[0] / self._rate()
            if t is not None and tc > t:
                break
            for g in self.flows:
                g[0] -= f[0] if g is not f else 0
            self.flows.remove(f)
            self.done.append((f[1], tc))
            self.t = tc
        if t is not None:
            if self.flows:
                share = (t - self.t) * self._rate()
                for g in self.flows:
                    g[0] -= share
            self.t = Fraction(t)

    def arrive(self, ta, svc):
        self._run_to(Fraction(ta))
        self.flows.append([Fraction(svc), ta, self.seq])
        self.seq += 1

    def finish(self):
        self._run_to(None)
