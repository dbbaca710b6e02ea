"""The reference of processor-sharing servers: tests.flowsim_ref.FlowSim with DESIGN.md §3.22 added.

Written from §3.22's text, not from the kernel.  Times stay absolute int64 us; nothing is rebased.
A server is a virtual clock V, a carry acc, the time t_last of its last update and a plain list of
(tag, ta) kept in non-decreasing tag order, a new entry after every equal tag:

  advance(s, t):  n > 0: acc += t - t_last; V += acc // n; acc %= n.  n = 0: acc = 0.  t_last = t.
  next completion of s (n > 0):  t_last + (tag_head - V) * n - acc
  arrival at ta assigned to s (after the pops due by ta):  advance(s, ta); tag = V + svc; insert
  completion (s, tc):  advance(s, tc); V == tag_head and acc == 0 (asserted); pop the head
  step end:  advance(s, end) for every server

Every completion is offered to the server's reservoir by Algorithm R with the reservoir-stream
draw, restated here from §3.2 / §3.4 over tests.policy_ref.philox4x32_10: the block of index
count >> 1, its 64-bit half count & 1, j = floor(r64 (c + 1) / 2^64).

arrivals=(gap_table, work_table) draws the gaps and works from two quantile tables, restating the
host rule of marllb_amd.workload (bin(v) of the arrival's Philox words; the gap at least 1 us).

self.reach counts what a scenario met (tests/test_processor_sharing.py asserts on it).

BruteForcePS is a second formulation for one server fed with the arrivals (ta, svc) the reference
assigned to it: exact processor sharing with per-flow remaining work as fractions.Fraction of
served time, no virtual clock and no carry.
"""
import bisect
from fractions import Fraction

import numpy as np

from tests.flowsim_ref import _BLOCK, _F32, FlowSim, StepResult
from tests.policy_ref import philox4x32_10

K = 128
STREAM_RESERVOIR = 2


def table_bin(v):
    """marllb_amd.workload.table_bin's rule for one 32-bit word, restated."""
    v = int(v)
    if v < 32:
        return v
    e = v.bit_length() - 1
    return 32 * (e - 4) + ((v >> (e - 5)) & 31)


def stream_slot(key, gid, episode, server, count):
    """Algorithm R with the reservoir-stream draw: the slot of the sample that makes the count
    count + 1, or -1."""
    if count < K:
        return count
    ctr = np.array([[count >> 1, gid, episode, (STREAM_RESERVOIR << 24) | server]], np.uint64)
    d = [int(x) for x in philox4x32_10(ctr, np.array(key, dtype=np.uint64))[0]]
    r64 = (d[3] << 32 | d[2]) if count & 1 else (d[1] << 32 | d[0])
    j = (r64 * (count + 1)) >> 64
    return j if j < K else -1


class PSSim(FlowSim):
    def __init__(self, *args, arrivals=None, **kwargs):
        super().__init__(*args, **kwargs)
        assert self.policy != "alias" and self.trace is None
        self.tables = None
        if arrivals is not None:
            self.tables = tuple(np.asarray(t, _F32) for t in arrivals)
        self.reach = {k: 0 for k in ("inserts", "at_head", "shift_gt8", "equal_tags", "same_us",
                                     "at_ta", "at_dt", "full_drops", "acc_carried")}

    # ---------------------------------------------------------------- arrivals from tables
    def _draw_block(self):
        if self.tables is None:
            return super()._draw_block()
        k0 = len(self._ta)
        k = np.arange(k0, k0 + _BLOCK, dtype=np.uint64)
        ctr = np.stack([k, np.full_like(k, self.gid), np.full_like(k, self.episode),
                        np.full_like(k, 1 << 24)], axis=-1)
        d = philox4x32_10(ctr, np.array(self.key, dtype=np.uint64))
        gt, wt = self.tables
        t = self._ta[-1] if k0 else 0
        for i in range(_BLOCK):
            gap = max(1, int(_F32(gt[table_bin(d[i, 0])]) * self.mean_gap))
            t += gap
            self._ta.append(t)
            self._work.append(_F32(wt[table_bin(d[i, 1])]))
            self._u2.append(int(d[i, 2]))

    # ---------------------------------------------------------------- the servers
    def reset(self):
        S = self.S
        self.V, self.acc, self.t_last = [0] * S, [0] * S, [0] * S
        self.res = [[None] * K for _ in range(S)]  # (fct us, ts ms)
        self.res_count = [0] * S
        self.big = [False] * S
        self.written = [set() for _ in range(S)]
        self.bp_k, self.bp_nmax = [0] * S, [0] * S  # arrivals / deepest queue of the busy period
        self.completion_log, self.assigned_log = [], []
        return super().reset()

    def _advance(self, s, t):
        n = len(self.queues[s])
        assert t >= self.t_last[s]
        if n > 0:
            self.acc[s] += t - self.t_last[s]
            self.V[s] += self.acc[s] // n
            self.acc[s] %= n
        else:
            self.acc[s] = 0
        self.t_last[s] = t

    def _tc(self, s):
        q = self.queues[s]
        return self.t_last[s] + (q[0][0] - self.V[s]) * len(q) - self.acc[s]

    def _sample(self, s, ta, tc):
        c = self.res_count[s]
        slot = stream_slot(self.key, self.gid, self.episode, s, c)
        if slot >= 0:
            self.res[s][slot] = (tc - ta, tc // 1000)
            self.written[s].add(slot)
            self.big[s] |= tc - ta >= (1 << 25) - 1
        self.res_count[s] = c + 1

    def _pop_due(self, t, done, at_arrival=True):
        while True:
            due = [(self._tc(s), s) for s, q in enumerate(self.queues) if q]
            due = [x for x in due if x[0] <= t]
            if not due:
                return
            tc, s = min(due)  # the earliest, ties to the lowest server
            self.reach["same_us"] += sum(1 for x in due if x[0] == tc) > 1
            self.reach["at_ta" if at_arrival else "at_dt"] += tc == t
            self._advance(s, tc)
            tag, ta = self.queues[s][0]
            assert self.V[s] == tag and self.acc[s] == 0, (self.V[s], tag, self.acc[s])
            self.queues[s].pop(0)
            done.append((s, ta, tc))
            # for the tests: the coarse bound of its busy period so far, and whether it ends it
            self.completion_log.append((s, ta, tc, 2 * self.bp_k[s] * self.bp_nmax[s],
                                        not self.queues[s]))
            if not self.queues[s]:
                self.bp_k[s] = self.bp_nmax[s] = 0
            self._sample(s, ta, tc)

    def _insert(self, s, ta, svc):
        """The arrival at ta, needing svc us, onto server s (the pops due by ta are done)."""
        r = self.reach
        self._advance(s, ta)
        q = self.queues[s]
        # the unfinished work the arrival finds: sum(tag - V) - acc
        work = sum(tag - self.V[s] for tag, _ in q) - self.acc[s]
        tag = self.V[s] + svc
        tags = [e[0] for e in q]
        at = bisect.bisect_right(tags, tag)
        r["inserts"] += 1
        r["at_head"] += at == 0 and len(q) > 0
        r["shift_gt8"] += len(q) - at > 8
        r["equal_tags"] += tag in tags
        q.insert(at, (tag, ta))
        self.bp_k[s] += 1
        self.bp_nmax[s] = max(self.bp_nmax[s], len(q))
        self.assigned_log.append((s, ta, svc, work))

    def set_rates(self, rate=None, server_rates=None):
        """New rates from the next step on, as a mid-run lbsim_set_env_rates or a phase change of
        a rate schedule acts (§3.10, §3.12): the arrival already drawn keeps its time and work,
        every later gap is drawn again at the new mean gap, every later service time uses the new
        server rates.  Before reset(): the rates of the episode's first draw and warm-up."""
        if rate is not None:
            gap = _F32(1e6 / float(_F32(rate)))
            if gap != self.mean_gap:
                self.mean_gap = gap
                if getattr(self, "_ta", None):
                    self._arrival(self.k)  # the arrival already drawn
                    del self._ta[self.k + 1:], self._work[self.k + 1:], self._u2[self.k + 1:]
        if server_rates is not None:
            self.svc_scale = [_F32(1e6 / float(_F32(m))) for m in server_rates]

    def step(self, weights):
        w = np.asarray(weights, dtype=_F32)
        assert w.shape == (self.S,) and np.isfinite(w).all()
        end = (self.step_no + 1) * self.dt
        self.written = [set() for _ in range(self.S)]
        self.assigned_log = []  # (server, ta, svc, work found) of this step's assigned arrivals
        self.completion_log = []  # (server, ta, tc, coarse bound, ends its busy period)
        assigned, dropped, done = np.zeros(self.S, np.int64), 0, []
        r = self.reach
        while self._arrival(self.k) < end:
            ta = self._ta[self.k]
            self._pop_due(ta, done)
            s = self._choose(self._u2[self.k], w, None)
            if s < 0:
                dropped += 1
                r["full_drops"] += all(len(q) == self.Q for q in self.queues)
            else:
                svc = max(1, int(_F32(self._work[self.k]) * self.svc_scale[s]))
                self._insert(s, ta, svc)
                assigned[s] += 1
            self.k += 1
        self._pop_due(end, done, at_arrival=False)
        for s in range(self.S):
            self._advance(s, end)
            r["acc_carried"] += self.acc[s] != 0
        self.step_no += 1
        return StepResult(assigned, dropped, done)

    # ---------------------------------------------------------------- after a step
    def remaining(self, s):
        """Server s's entries as the state holds them: (tag - V, ta), in tag order."""
        return [(tag - self.V[s], ta) for tag, ta in self.queues[s]]


class BruteForcePS:
    """One exact processor-sharing server: arrive(ta, svc) in arrival order, then finish().
    done: [(ta, tc)] with tc a Fraction, in completion order (ties: the earlier arrival).
    work_at: the unfinished work just before each arrival, for the conservation check."""

    def __init__(self):
        self.t = Fraction(0)
        self.flows = []  # [remaining, ta, seq]
        self.done = []
        self.work_at = []
        self.arrivals = []  # (ta, svc), as fed
        self.seq = 0

    def _run_to(self, t):
        while self.flows:
            n = len(self.flows)
            f = min(self.flows, key=lambda x: (x[0], x[2]))
            tc = self.t + f[0] * n
            if t is not None and tc > t:
                break
            for g in self.flows:
                g[0] -= f[0] if g is not f else 0
            self.flows.remove(f)
            self.done.append((f[1], tc))
            self.t = tc
        if t is not None:
            if self.flows:
                share = (t - self.t) / len(self.flows)
                for g in self.flows:
                    g[0] -= share
            self.t = Fraction(t)

    def arrive(self, ta, svc):
        self._run_to(Fraction(ta))
        self.arrivals.append((ta, svc))
        self.work_at.append(sum(g[0] for g in self.flows))
        self.flows.append([Fraction(svc), ta, self.seq])
        self.seq += 1

    def finish(self):
        self._run_to(None)
