"""tests/parity.py's state comparer on the CPU: two oracle handles stand in for the device and
its reference, so the comparer itself is shown to pass on equal states, to see a single changed
word, and to ignore exactly the ring slots that are not state."""
import numpy as np
import pytest

from tests import statelayout
from tests.parity import compare_state

B, S, Q, STEPS = 5, 3, 4, 3


def _oracle(oracle_mod, steps, b=None):
    """(config, handle) after a reset and `steps` steps; b: the one-env handle of env b."""
    from marllb_amd.env import make_config
    kw = dict(seed=17, queue_capacity=Q)
    cfg = make_config(B, S, **kw) if b is None else make_config(1, S, env_id_offset=b, **kw)
    ora = oracle_mod.OracleEnv(cfg)
    ora.reset()
    rng = np.random.default_rng(17)
    for _ in range(steps):
        a = rng.integers(0, 3, (B, S)).astype(np.int64)
        ora.step(a if b is None else a[b:b + 1])
    return cfg, ora


def _poked(buf, cfg, section, index):
    """The snapshot with word `index` of one section incremented."""
    off = 0
    for name, dt, n in statelayout.sections(B, S, Q, bool(cfg.normalize_obs)):
        if name == section:
            out = bytearray(buf)
            word = np.frombuffer(out, dt, 1, off + index * np.dtype(dt).itemsize)
            word += 1
            return bytes(out)
        off += np.dtype(dt).itemsize * n
    raise KeyError(section)


def test_compare_state_on_oracle_pairs(oracle_mod):
    cfg, a = _oracle(oracle_mod, STEPS)
    _, b = _oracle(oracle_mod, STEPS)
    ref = compare_state(a, b, cfg)  # in step
    np.testing.assert_array_equal(ref["hc"], statelayout.parse_cfg(b.state_bytes(), cfg)["hc"])
    snap = b.state_bytes()

    b.step(np.zeros((B, S), np.int64))  # one handle a step ahead
    with pytest.raises(AssertionError):
        compare_state(a, b, cfg)

    b.load_state(_poked(snap, cfg, "res_count", 7))  # one word of one section
    with pytest.raises(AssertionError, match="res_count"):
        compare_state(a, b, cfg)

    # a ring slot beyond the live count is not state
    hc = ref["hc"].reshape(B, S)
    head, count = hc & 0x7FFF, hc >> 16
    assert (count < Q).any() and (count > 0).any(), count
    e, s = np.argwhere(count < Q)[0]
    stale = (int(head[e, s]) + int(count[e, s])) % Q
    b.load_state(_poked(snap, cfg, "ring", ((e * S + s) * Q + stale) * 2))
    assert b.state_bytes() != snap  # the snapshots do differ, in that word
    compare_state(a, b, cfg)
    # ... and a live slot is
    e, s = np.argwhere(count > 0)[0]
    b.load_state(_poked(snap, cfg, "ring", ((e * S + s) * Q + int(head[e, s])) * 2))
    with pytest.raises(AssertionError):
        compare_state(a, b, cfg)
    a.close()
    b.close()


class _Stack:
    def __init__(self, envs):
        self.envs = envs

    def state_bytes(self):
        return [o.state_bytes() for o in self.envs]


def test_compare_state_stacks_one_env_snapshots(oracle_mod):
    cfg, whole = _oracle(oracle_mod, STEPS)
    ones = _Stack([_oracle(oracle_mod, STEPS, b)[1] for b in range(B)])
    ref = compare_state(whole, ones, cfg)
    assert ref["hc"].shape == (B * S,) and ref["_live_ring"].shape == (B, S, Q, 2)
    ones.envs[3].step(np.zeros((1, S), np.int64))  # env 3 of the stack a step ahead
    with pytest.raises(AssertionError):
        compare_state(whole, ones, cfg)
    whole.close()
    for o in ones.envs:
        o.close()
