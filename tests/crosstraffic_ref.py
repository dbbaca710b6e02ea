"""The reference of hidden cross traffic: tests.flowsim_ref.FlowSim with DESIGN.md §3.17 added.

Written from §3.17's text, not from the kernel: the 24-bit threshold and cumulative edges, the
fmix32 hash of the arrival index, the pick, queue entries that carry a hidden flag, and scores and
in_flight() that count visible flows only.  Times stay absolute int64 us and queues plain lists, as
in FlowSim; a hidden entry is (tc, ta, True, step it was pushed in).

step() reports visible completions only (StepResult.completed); the hidden flows are counted
beside them: hidden_assigned (S,), hidden_dropped, hidden_completed [(server, tc, in_step)].
"""
import numpy as np

from tests.flowsim_ref import FlowSim, StepResult, _F32

ONE = 1 << 24
_M32 = 0xFFFFFFFF


def mix(h):
    """murmur3's fmix32."""
    h &= _M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & _M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & _M32
    h ^= h >> 16
    return h


def threshold(share):
    """thr = rint(f64(f32 share) * 2^24)."""
    return int(np.rint(np.float64(np.float32(share)) * np.float64(ONE)))


def edges(weights, S):
    """cum[s] = floor(2^24 c_s / c_{S-1}), c the sequential f64 prefix sum of the f32 weights;
    cum[S-1] = 2^24.  None: uniform."""
    w = np.ones(S, np.float32) if weights is None else np.asarray(weights, np.float32)
    assert w.shape == (S,) and np.isfinite(w).all() and (w >= 0).all()
    c = np.zeros(S, np.float64)
    acc = np.float64(0.0)
    for s in range(S):  # sequential on purpose
        acc = acc + np.float64(w[s])
        c[s] = acc
    assert c[-1] > 0
    cum = np.floor(c * np.float64(ONE) / c[-1]).astype(np.int64)
    cum[-1] = ONE
    return cum


def salt(key, gid, episode):
    k0, k1 = key
    return mix(mix(k0 ^ ((episode * 0x9E3779B9) & _M32)) ^ gid ^ ((k1 * 0x85EBCA6B) & _M32))


def decide(k, slt, thr, cum):
    """(hidden, server of the hidden flow) of arrival k."""
    h = mix(k ^ slt ^ 0x3C6EF372)
    x = mix(h ^ 0x6A09E667) >> 8
    return (h >> 8) < thr, int((np.asarray(cum) <= x).sum())


class CrossStepResult(StepResult):
    def __init__(self, assigned, dropped, completed, hidden_assigned, hidden_dropped,
                 hidden_completed):
        super().__init__(assigned, dropped, completed)
        self.hidden_assigned = hidden_assigned
        self.hidden_dropped = hidden_dropped      # (included in dropped)
        self.hidden_completed = hidden_completed  # [(server, tc, completed in its own step)]


class CrossSim(FlowSim):
    """FlowSim with a hidden share of its arrivals.  set_cross(share, weights) may be called at
    any time between steps: it applies to the arrivals assigned from then on."""

    def __init__(self, *args, share=0.0, weights=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.set_cross(share, weights)

    def set_cross(self, share, weights=None):
        assert 0.0 <= float(np.float32(share)) <= 1.0
        self.thr = threshold(share)
        self.cum = edges(weights, self.S)

    # a queue entry is (tc, ta, hidden, step pushed); the base class's helpers see what they need
    def _score(self, s, w):
        n = sum(1 for e in self.queues[s] if not e[2])  # the visible count
        if self.policy in ("lsq", "lsq2"):
            return float(n)
        return _F32(float(n + 1) / (float(w[s]) + 1e-9))

    def _pop_due(self, t, done, hidden_done=None):
        while True:
            best = -1
            for s, q in enumerate(self.queues):
                if q and q[0][0] <= t and (best < 0 or q[0][0] < self.queues[best][0][0]):
                    best = s
            if best < 0:
                return
            tc, ta, hid, pushed = self.queues[best].pop(0)
            if hid:
                hidden_done.append((best, tc, pushed == self.step_no))
            else:
                done.append((best, ta, tc))

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
        slt = salt(self.key, self.gid, self.episode)
        assigned, hidden = np.zeros(self.S, np.int64), np.zeros(self.S, np.int64)
        dropped = hdropped = 0
        done, hdone = [], []
        while self._arrival(self.k) < end:
            ta = self._ta[self.k]
            self._pop_due(ta, done, hdone)
            hid, pick = decide(self.k, slt, self.thr, self.cum)
            if hid:  # the action is ignored; a full server drops it
                s = pick if len(self.queues[pick]) < self.Q else -1
            else:
                s = self._choose(self._u2[self.k], w, alias_table)
            if s < 0:
                dropped += 1
                hdropped += int(hid)
            else:
                q = self.queues[s]
                start = max(ta, q[-1][0]) if q else ta
                svc = max(1, int(_F32(self._work[self.k]) * self.svc_scale[s]))
                q.append((start + svc, ta, hid, self.step_no))
                (hidden if hid else assigned)[s] += 1
            self.k += 1
        self._pop_due(end, done, hdone)
        self.step_no += 1
        return CrossStepResult(assigned, dropped, done, hidden, hdropped, hdone)

    def in_flight(self):
        """Visible flows queued per server."""
        return [sum(1 for e in q if not e[2]) for q in self.queues]

    def hidden_in_flight(self):
        return [sum(1 for e in q if e[2]) for q in self.queues]
