"""Action latency on the independent reference: tests/flowsim_ref.FlowSim with
the delay rule added from the section's text.

DelayRule goes in front of FlowSim or of a simulator derived from it whose step() picks every
server through _choose (tests/workers_ref.CrossWorkerSim: multi-worker servers and hidden cross
traffic).  It keeps the weight rows of the episode (hist[j] = W(j), the row of the action passed
to the step with ep_step = j), picks the row of every arrival by the rule -- W(k - m) from r us
into the step on, W(k - m - 1) before, ones for a negative index -- and has the ALIAS table of
either row.  Nothing else of a step reads weights, so the step itself is the base class's.  A
reset and its warm-up run at ones and start a new history.  Beside it the ring of the handle as
the text describes its storage: W(k) at row k % (M + 2), never cleared.

For the tests it also evaluates every arrival under the other row of its step and counts what the
scenario reaches (`reach`).
"""
import numpy as np

import oracle
from tests.flowsim_ref import FlowSim

_F32 = np.float32


class DelayRule:
    def __init__(self, *args, max_delay_steps=1, delay_us=0, **kw):
        super().__init__(*args, **kw)
        self.M = int(max_delay_steps)
        self.R = self.M + 2
        self.ring = np.zeros((self.R, self.S), _F32)
        self.hist = []
        self._rows = None  # inside a policy step: (r, start, j_new, j_old, rows, tables)
        self._warm = False
        self.set_delay(delay_us)
        self.reach = {**getattr(self, "reach", {}),  # (beside the base class's own counters)
                      "split_steps": 0, "flips": 0, "set_changes": 0, "arrivals": 0}
        self.first_offsets = []  # per policy step: the first arrival's offset in the step, or None
        self.rows_used = []      # per policy step: the row index j of every arrival it chose for

    def set_delay(self, delay_us):
        d = int(delay_us)
        assert 0 <= d <= self.M * self.dt, d
        self.delay_us = d

    # ------------------------------------------------------------ reset: ones, a new history
    def reset(self):
        self._warm = True
        try:
            out = super().reset()
        finally:
            self._warm = False
        self.hist = []
        return out

    def _table(self, w):
        if self.policy != "alias":
            return None
        act = [s for s in range(self.S) if w[s] > 0]
        odd, alias = oracle.gen_alias(w[act]) if act else (np.zeros(0), np.zeros(0, np.int32))
        return (act, odd.astype(_F32), alias)

    # ------------------------------------------------------------ the choice under the rule
    def _choose(self, u2, w, alias_table):
        if self._rows is None:  # a warm-up step: the weights it was given
            return super()._choose(u2, w, alias_table)
        r, start, j_new, j_old, rows, tables = self._rows
        off = self._ta[self.k] - start
        j = j_new if off >= r else j_old  # at the switch instant: the new row
        other = j_old if j == j_new else j_new
        ties = self.alias_ties
        alt = super()._choose(u2, rows[other], tables[other])
        self.alias_ties = ties  # (the other row's pick is only counted, not made)
        s = super()._choose(u2, rows[j], tables[j])
        self.reach["flips"] += int(alt != s)
        self.reach["arrivals"] += 1
        self.rows_used[-1].append(j)
        return s

    def step(self, weights):
        if self._warm:
            return super().step(weights)
        w_k = np.asarray(weights, dtype=_F32)
        assert w_k.shape == (self.S,) and np.isfinite(w_k).all()
        k = len(self.hist)  # ep_step as the launch reads it
        self.hist.append(w_k.copy())
        self.ring[k % self.R] = w_k
        m, r = divmod(self.delay_us, self.dt)
        j_new, j_old = k - m, k - m - 1
        ones = np.ones(self.S, _F32)
        rows = {j: (ones if j < 0 else self.hist[j]) for j in (j_new, j_old)}
        tables = {j: self._table(w) for j, w in rows.items()}
        start = self.step_no * self.dt
        k0 = self.k
        self.rows_used.append([])
        self._rows = (r, start, j_new, j_old, rows, tables)
        try:
            out = super().step(w_k)
        finally:
            self._rows = None
        self.first_offsets.append(self._ta[k0] - start if self.k > k0 else None)
        if 0 < r and len(set(self.rows_used[-1])) == 2:
            self.reach["split_steps"] += 1
            if set(np.flatnonzero(rows[j_new] > 0)) != set(np.flatnonzero(rows[j_old] > 0)):
                self.reach["set_changes"] += 1
        return out


class DelaySim(DelayRule, FlowSim):
    """One plain env under the rule."""
