"""The reference of duration samples at every data ACK: tests.flowsim_ref.FlowSim with DESIGN.md
§3.25 added.

Written from §3.25's text, not from the kernel.  Times stay absolute int64 us; nothing is rebased.
Per server, a plain list of the flows that still have ACKs to come, oldest first, each with its
(ta, t0, tc): t0 = max(ta, tc of its predecessor on the server), tc = t0 + svc.  A flow emits
k = min(max_acks, max(1, svc // ack_us)) ACKs, ACK j = 1..k at t_j = t0 + (svc * j) // k, and step
n (the n-th since the reset, warm-up included) records the ACKs with n dt < t_j <= (n + 1) dt: a
loop over every j of every listed flow, no window arithmetic.  Each ACK offers the age t_j - ta,
stamped t_j // 1000 ms, to the duration reservoir of its server, in time order.

The duration reservoir runs Algorithm R with the reservoir-stream draw for every sample, restated
from tests.ps_ref.stream_slot with the stream word of §3.2: (2 << 24) | (1 << 17) | server.

self.reach counts what a scenario met (tests/test_ack_samples.py asserts on it).
"""
import numpy as np

import oracle
from tests.flowsim_ref import _F32, FlowSim, StepResult
from tests.policy_ref import philox4x32_10

K = 128
STREAM_RESERVOIR = 2
ACK_BIT = 1 << 17
BIG = (1 << 25) - 1


_BLOCKS = 64  # reservoir-stream blocks drawn at a time (one numpy call)
_CACHE = {}


def _block(key, gid, episode, server, idx):
    """Block idx of the duration reservoir's stream: Philox words (key; idx, gid, episode, the
    stream word), drawn _BLOCKS at a time and kept."""
    base = idx - idx % _BLOCKS
    ck = (key, gid, episode, server, base)
    if ck not in _CACHE:
        if len(_CACHE) > 4096:
            _CACHE.clear()
        i = np.arange(base, base + _BLOCKS, dtype=np.uint64)
        ctr = np.stack([i, np.full_like(i, gid), np.full_like(i, episode),
                        np.full_like(i, (STREAM_RESERVOIR << 24) | ACK_BIT | server)], axis=-1)
        _CACHE[ck] = philox4x32_10(ctr, np.array(key, dtype=np.uint64)).tolist()
    return _CACHE[ck][idx - base]


def ack_slot(key, gid, episode, server, count):
    """Algorithm R with the reservoir-stream draw under the duration reservoir's stream word: the
    slot of the sample that makes the count count + 1, or -1."""
    if count < K:
        return count
    d = _block(key, gid, episode, server, count >> 1)
    r64 = (d[3] << 32 | d[2]) if count & 1 else (d[1] << 32 | d[0])
    j = (r64 * (count + 1)) >> 64
    return j if j < K else -1


class Flow:
    __slots__ = ("s", "ta", "t0", "tc", "k", "acks", "steps")

    def __init__(self, s, ta, t0, tc, k):
        self.s, self.ta, self.t0, self.tc, self.k = s, ta, t0, tc, k
        self.acks = []   # (t_j, age, ts_ms) as recorded, in order
        self.steps = []  # the step each was recorded in


class AckSim(FlowSim):
    def __init__(self, *args, max_acks=8, ack_us=1000, **kwargs):
        super().__init__(*args, **kwargs)
        assert 1 <= max_acks <= 32 and 1 <= ack_us <= 1 << 30
        self.max_acks, self.ack_us = int(max_acks), int(ack_us)
        self.reach = {k: 0 for k in ("steps3", "silent_step", "at_dt", "cap_max", "cap_svc",
                                     "over128")}

    def reset(self):
        S = self.S
        self.open = [[] for _ in range(S)]      # flows with ACKs to come, oldest first
        self.flows = []                         # every flow assigned in this episode
        self.dur = [[None] * K for _ in range(S)]  # (age us, ts ms)
        self.dur_count = [0] * S
        self.big = [False] * S
        self.written = [{0} for _ in range(S)]  # emptied reservoirs: slot 0 marked
        self._warm = True
        out = super().reset()
        self._warm = False
        return out

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

    def _offer(self, s, age, ts):
        c = self.dur_count[s]
        slot = ack_slot(self.key, self.gid, self.episode, s, c)
        if slot >= 0:
            self.dur[s][slot] = (age, ts)
            self.written[s].add(slot)
            self.big[s] |= age >= BIG
        self.dur_count[s] = c + 1
        self.reach["over128"] += c + 1 == K + 1

    def step(self, weights):
        w = np.asarray(weights, dtype=_F32)
        assert w.shape == (self.S,) and np.isfinite(w).all()
        begin = self.step_no * self.dt
        end = begin + self.dt
        if not self._warm:
            self.written = [set() for _ in range(self.S)]
        alias_table = None
        if self.policy == "alias":
            act = [s for s in range(self.S) if w[s] > 0]
            odd, alias = oracle.gen_alias(w[act]) if act else (np.zeros(0), np.zeros(0, np.int32))
            alias_table = (act, odd.astype(_F32), alias)
        assigned, dropped, done = np.zeros(self.S, np.int64), 0, []
        while self._arrival(self.k) < end:
            ta = self._ta[self.k]
            self._pop_due(ta, done)
            s = self._choose(self._u2[self.k], w, alias_table)
            if s < 0:
                dropped += 1
            else:
                q = self.queues[s]
                t0 = max(ta, q[-1][0]) if q else ta
                svc = max(1, int(_F32(self._work[self.k]) * self.svc_scale[s]))
                q.append((t0 + svc, ta))
                raw = max(1, svc // self.ack_us)
                k = min(self.max_acks, raw)
                self.reach["cap_max"] += raw > self.max_acks
                self.reach["cap_svc"] += svc // self.ack_us == svc and svc < self.max_acks
                f = Flow(s, ta, t0, t0 + svc, k)
                self.open[s].append(f)
                self.flows.append(f)
                assigned[s] += 1
            self.k += 1
        self._pop_due(end, done)
        # the ACKs of (begin, end], per server in time order: one worker serves one flow at a time
        for s in range(self.S):
            in_service = any(f.t0 < end and f.tc > begin for f in self.open[s])
            n = 0
            for f in self.open[s]:
                svc = f.tc - f.t0
                for j in range(1, f.k + 1):
                    t = f.t0 + (svc * j) // f.k
                    if begin < t <= end:
                        f.acks.append((t, t - f.ta, t // 1000))
                        f.steps.append(self.step_no)
                        self._offer(s, t - f.ta, t // 1000)
                        self.reach["at_dt"] += t == end
                        n += 1
            self.reach["silent_step"] += in_service and n == 0
            for f in self.open[s]:
                if f.tc <= end:
                    self.reach["steps3"] += len(set(f.steps)) >= 3
            self.open[s] = [f for f in self.open[s] if f.tc > end]
        self.step_no += 1
        return StepResult(assigned, dropped, done)
