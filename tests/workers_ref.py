"""The reference of multi-worker servers: tests.flowsim_ref.FlowSim with DESIGN.md §3.18 added.

Written from §3.18's text, not from the kernel.  A server's queue is a plain list of (tc, ta) kept
in non-decreasing tc order (a new entry after every equal or smaller tc); times stay absolute int64
us.  Two formulations of the start time, chosen by `explicit`:

(a) explicit=True: a list of c worker-free times per server; the flow goes to the earliest-free
    worker, ties to the lowest index, and starts at max(ta, that worker's free time);
(b) explicit=False: the sorted-queue rule -- with n flows queued, ta if n < c, else
    max(ta, tc of the entry at sorted position n - c).

They are the same process while c is constant since the reset (asserted by the tests); after
set_workers only (b) is defined.

step() returns a WorkerStepResult: StepResult plus, per server, the new reservoir records in the
sample order of §3.18 -- the carried-in flows that complete in the step in queue (tc) order, then
the flows that arrive and complete in the step in arrival order.  fct(s) / tc(s) follow that order.
self.reach counts what the scenario met (tests/test_server_workers.py asserts on it).

CrossWorkerSim layers hidden cross traffic (§3.17) on top, as tests/crosstraffic_ref.py does on
FlowSim, for the one combined test.
"""
import bisect

import numpy as np

from tests.flowsim_ref import FlowSim, StepResult, _F32

WINDOW = 8  # queue positions below it sit in the kernel's LDS window, the others in the ring


class WorkerStepResult(StepResult):
    def __init__(self, assigned, dropped, completed, records):
        super().__init__(assigned, dropped, completed)
        self.records = records  # per server [(ta, tc)] in sample order

    def fct(self, s):
        return [tc - ta for (ta, tc) in self.records[s]]

    def tc(self, s):
        return [tc for (ta, tc) in self.records[s]]


class WorkerSim(FlowSim):
    def __init__(self, *args, workers=None, explicit=False, **kwargs):
        super().__init__(*args, **kwargs)
        self.explicit = bool(explicit)
        self.workers = [1] * self.S
        self.free = None
        self.reach = {k: 0 for k in ("pushes", "out_of_order", "at_head", "max_shift",
                                     "cross_window", "ring_start", "carried_out_of_order",
                                     "multi_drop")}
        self.set_workers([1] * self.S if workers is None else workers)

    def set_workers(self, workers):
        w = [int(c) for c in workers]
        assert len(w) == self.S and all(1 <= c <= 64 for c in w)
        assert not (self.explicit and self.free is not None and w != self.workers), \
            "a change of c is defined by the sorted-queue rule only"
        self.workers = w

    def reset(self):
        self.free = [[0] * c for c in self.workers]  # every worker idle
        return super().reset()

    def fail(self, s):
        """Server s fails: its queue is emptied (the flows count as dropped) and its workers are
        idle.  Returns the number of flows lost."""
        n = len(self.queues[s])
        self.queues[s] = []
        self.free[s] = [0] * self.workers[s]
        return n

    def _start(self, s, ta):
        q, c = self.queues[s], self.workers[s]
        if self.explicit:
            f = self.free[s]
            w = min(range(c), key=lambda i: (f[i], i))
            return max(ta, f[w]), w
        n = len(q)
        if n - c >= WINDOW:
            self.reach["ring_start"] += 1
        return (ta if n < c else max(ta, q[n - c][0])), None

    # hooks of CrossWorkerSim (hidden cross traffic layered on): is the next arrival hidden and
    # where does it go, what a queue entry is, and whether one is hidden
    def _hidden(self):
        return False, -1

    def _entry(self, tc, ta, hid):
        return (tc, ta)

    def _is_hidden(self, e):
        return False

    def _push(self, s, tc, ta, hid=False):
        q, c = self.queues[s], self.workers[s]
        n = len(q)
        at = bisect.bisect_right([e[0] for e in q], tc)
        q.insert(at, self._entry(tc, ta, hid))
        r = self.reach
        r["pushes"] += 1
        r["out_of_order"] += at < n
        r["at_head"] += at == 0 and n > 0
        assert n - at <= c - 1, "the entry lands at most c - 1 positions from the tail"
        r["max_shift"] += c > 1 and n - at == c - 1
        r["cross_window"] += c > 1 and at < WINDOW <= n  # the entry at position 7 moves to 8

    def step(self, weights):
        import oracle
        w = np.asarray(weights, dtype=_F32)
        assert w.shape == (self.S,) and np.isfinite(w).all()
        end = (self.step_no + 1) * self.dt
        alias_table = None
        if self.policy == "alias":
            act = [s for s in range(self.S) if w[s] > 0]
            odd, alias = oracle.gen_alias(w[act]) if act else (np.zeros(0), np.zeros(0, np.int32))
            alias_table = (act, odd.astype(_F32), alias)
        # the carried-in flows that complete in this step, in queue order
        records = [[(e[1], e[0]) for e in q if e[0] <= end and not self._is_hidden(e)]
                   for q in self.queues]
        for rec in records:
            tas = [ta for ta, _ in rec]
            self.reach["carried_out_of_order"] += tas != sorted(tas)
        assigned, dropped, done = np.zeros(self.S, np.int64), 0, []
        while self._arrival(self.k) < end:
            ta = self._ta[self.k]
            self._pop_due(ta, done)
            hid, pick = self._hidden()
            if hid:  # (cross traffic) the action is ignored; a full server drops the flow
                s = pick if len(self.queues[pick]) < self.Q else -1
            else:
                s = self._choose(self._u2[self.k], w, alias_table)
            if s < 0:
                dropped += 1
                # (every policy but ALIAS drops only when every server is full)
                self.reach["multi_drop"] += (self.policy != "alias" and max(self.workers) > 1
                                             and all(len(q) == self.Q for q in self.queues))
            else:
                start, worker = self._start(s, ta)
                svc = max(1, int(_F32(self._work[self.k]) * self.svc_scale[s]))
                tc = start + svc
                if worker is not None:
                    self.free[s][worker] = tc
                self._push(s, tc, ta, hid)
                if tc <= end and not hid:  # arrives and completes in the step: its record now
                    records[s].append((ta, tc))
                assigned[s] += 0 if hid else 1
            self.k += 1
        self._pop_due(end, done)
        self.step_no += 1
        return WorkerStepResult(assigned, dropped, done, records)


class CrossWorkerSim(WorkerSim):
    """WorkerSim with hidden cross traffic layered on as
    tests/crosstraffic_ref.CrossSim does on FlowSim, for the one combined test: the decision and
    the pick are crosstraffic_ref's, a queue entry is (tc, ta, hidden) and keeps its flag through
    the sorted insert, scores, in_flight(), records and assignments count visible flows only."""

    def __init__(self, *args, share=0.0, weights=None, **kwargs):
        super().__init__(*args, **kwargs)
        from tests import crosstraffic_ref as cr
        self._cr = cr
        self.thr = cr.threshold(share)
        self.cum = cr.edges(weights, self.S)

    def _hidden(self):
        slt = self._cr.salt(self.key, self.gid, self.episode)
        return self._cr.decide(self.k, slt, self.thr, self.cum)

    def _entry(self, tc, ta, hid):
        return (tc, ta, bool(hid))

    def _is_hidden(self, e):
        return e[2]

    def _score(self, s, w):
        n = sum(1 for e in self.queues[s] if not e[2])  # the visible count
        if self.policy in ("lsq", "lsq2"):
            return float(n)
        return _F32(float(n + 1) / (float(w[s]) + 1e-9))

    def _pop_due(self, t, done):
        while True:
            best = -1
            for s, q in enumerate(self.queues):
                if q and q[0][0] <= t and (best < 0 or q[0][0] < self.queues[best][0][0]):
                    best = s
            if best < 0:
                return
            tc, ta, hid = self.queues[best].pop(0)
            if not hid:
                done.append((best, ta, tc))

    def in_flight(self):
        return [sum(1 for e in q if not e[2]) for q in self.queues]

    def hidden_in_flight(self):
        return [sum(1 for e in q if e[2]) for q in self.queues]
