"""The arrival-driven event loop of the server-per-lane dynamics (group_count_loop,
csrc/lbsim_dyn_group.h): one iteration per arrival, the queue counted by completion time instead of
popped.  Small envs against the CPU oracle, bit for bit (outputs of every step, the whole state, a
masked reset, more steps: parity.run_vs_reference), at the corners of the loop's bookkeeping: the
8-entry LDS window crossed in both directions, full rings with drops, Q below the window and a
lane without a server, Q above 32 with entries living across steps, steps without an arrival and
queues that empty and refill (the loop starts a flow at max(tail, ta) without testing for an empty
queue: an empty queue's tail is <= ta), repeated steps on the same registers (a reset's warm-up,
next-step resets), the two-choice, LSQ and trace instantiations.

Each case first asserts, from the oracle's own state at the step boundaries, that its inputs reach
the corner it is there for.  The cases run under the process's dispatch (mapping "auto": the
default kernels; "server": 8-lane groups at these batch sizes) and, in a child process with
LBSIM_DYN_GROUP_LANES=4, on the 4-lane groups of the headline 65536 x 4 kernel."""
import functools

import numpy as np
import pytest

from tests import parity, statelayout
from tests.parity import lib  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

STEPS = 12
SLOW = {"arrival_rate": 12.0, "server_rates": [1.2, 1.4, 1.6, 1.8], "step_interval": 10.0,
        "queue_capacity": 64}
SPARSE = {"arrival_rate": 6.0, "server_rates": [3.0, 4.0, 5.0, 6.0]}
CASES = {
    "a_window": dict(B=64, S=4, kw={}, corner="window"),
    "b_full": dict(B=36, S=4, kw={"load": 1.25}, corner="full"),
    "c_smallq": dict(B=48, S=3, kw={"queue_capacity": 6, "load": 1.3}, corner="full"),
    "d_longq": dict(B=32, S=4, kw=SLOW, corner="long"),
    "e_sparse": dict(B=64, S=4, kw=SPARSE, corner="sparse"),
    "f_warmup2": dict(B=64, S=4, kw={"warmup_steps": 2}, corner=None),
    "f_nextstep": dict(B=64, S=4, kw={"max_steps": 3, "next_step_reset": True}, corner=None),
    "g_sed2": dict(B=64, S=4, kw={"assign_policy": "sed2"}, corner=None),
    "g_lsq": dict(B=48, S=3, kw={"assign_policy": "lsq", "queue_capacity": 6, "load": 1.3},
                  corner="full"),
    "g_trace": dict(B=50, S=4, kw={"trace": "short", "step_interval": 0.5}, corner=None),
}
SEED = 7


def _kw(name):
    kw = dict(CASES[name]["kw"], seed=SEED)
    if kw.get("trace") == "short":
        from marllb_amd import trace
        kw["trace"] = trace.synthetic(37, 300.0, seed=7)
    return kw


@functools.lru_cache(maxsize=None)
def _oracle_boundaries(name):
    """The oracle alone on the case's action stream: per step boundary the queue lengths (B, S),
    and the envs' dropped and arr_idx words."""
    import oracle
    from marllb_amd.env import make_config
    oracle.load()
    c, kw = CASES[name], _kw(name)
    cfg = make_config(c["B"], c["S"], **kw)
    ora = oracle.OracleEnv(cfg, threads=4, trace=kw.get("trace"))
    ora.reset()
    rng = np.random.default_rng(SEED)
    cnt, dropped, arr_idx = [], [], []

    def snap():
        d = statelayout.parse_cfg(ora.state_bytes(), cfg)
        cnt.append((d["hc"] >> 16).reshape(c["B"], c["S"]).astype(np.int64))
        dropped.append(d["dropped"].copy())
        arr_idx.append(d["arr_idx"].copy())

    snap()
    for _ in range(STEPS):
        ora.step(parity.actions(rng, c["B"], c["S"], c["kw"]))
        snap()
    ora.close()
    return np.stack(cnt), np.stack(dropped), np.stack(arr_idx), int(cfg.queue_capacity)


def _assert_corner(name):
    """Conditions on the inputs (the oracle's state), not on the code under test."""
    corner = CASES[name]["corner"]
    cnt, dropped, arr_idx, Q = _oracle_boundaries(name)
    if corner == "window":  # some server above the 8-entry window, and below it at a later boundary
        above = cnt > 8
        later_below = np.flip(np.maximum.accumulate(np.flip(cnt < 8, 0), 0), 0)
        assert (above[:-1] & later_below[1:]).any()
    elif corner == "full":  # some server at Q, and arrivals dropped
        assert (cnt == Q).any() and dropped.max() > 0
    elif corner == "long":  # beyond 32 entries, across several boundaries
        assert Q > 32 and ((cnt > 32).sum(0) >= 3).any()
    elif corner == "sparse":
        # a step without an arrival (the loop body runs zero times), and a server that is empty
        # at one boundary and queued at a later one (a flow started on an empty queue)
        assert (arr_idx[1:] == arr_idx[:-1]).any()
        empty = cnt == 0
        later_queued = np.flip(np.maximum.accumulate(np.flip(cnt > 0, 0), 0), 0)
        assert (empty[:-1] & later_queued[1:]).any()


@pytest.mark.parametrize("mapping", ["auto", "server"])
@pytest.mark.parametrize("name", list(CASES))
def test_count_loop_vs_oracle(lib, oracle_mod, name, mapping):
    from marllb_amd.env import VecLoadBalanceEnv, make_config
    _assert_corner(name)
    c, kw = CASES[name], _kw(name)
    env = VecLoadBalanceEnv(c["B"], c["S"], device="cuda:0", autoreset=False, dyn_mapping=mapping,
                            **kw)
    ora = oracle_mod.OracleEnv(make_config(c["B"], c["S"], **kw), threads=4, trace=kw.get("trace"))

    def hook(e):  # in the child run: the 4-lane group kernel stepped the env
        parity.check_dispatch(lib, e, lambda kern, names: None,
                              forced_group="dynamics_group_kernel" if mapping == "server" else None)

    parity.run_vs_reference(env, ora, c["kw"], SEED, steps=STEPS, post_steps=4, hook=hook)
    ora.close()
    env.close()


def test_count_loop_four_lane_groups():
    """Every case on dynamics_group_kernel<4, ...>, the headline's form (the width is read once
    per process: a child run)."""
    parity.run_cases_in_child("test_dyn_count_loop.py", "test_count_loop_vs_oracle and server",
                              {"LBSIM_DYN_GROUP_LANES": "4"})
