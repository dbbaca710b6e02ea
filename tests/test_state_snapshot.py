"""On-device snapshots: lbsim_state_save / lbsim_state_load, VecLoadBalanceEnv.snapshot / restore.

The reference is always the unmodified oracle run in lock step with the GPU env.  At a save point
the oracle's own state_bytes() is kept; at a load point the expected state is built on the host
from the oracle's snapshots, section by section (tests/statelayout.py, rows reshaped (B, -1)): row b
from the saved snapshot's row src[b], or from the current snapshot where env b is kept.  The oracle
loads that composite and both sides go on; every comparison is bit for bit.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from tests import parity, statelayout
from tests.parity import ENV_LANE, GROUP, actions, compare_state, lib, step_both  # noqa: F401
from tests.test_env_rates import PerEnvOracles, make_rates

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

LOST_FIN = {"lost_fin_prob": 0.2, "flow_timeout": 0.5, "lost_fin_pending": 4,
            "n_flow_on_mode": "vpp"}
NEXT_STEP = {"autoreset": True, "autoreset_mode": "next_step"}


# ------------------------------------------------------------------ the reference construction

def layout(cfg, B=None):
    return statelayout.sections(cfg.num_envs if B is None else B, cfg.num_servers,
                                cfg.queue_capacity, bool(cfg.normalize_obs), cfg.fail_prob > 0,
                                statelayout.has_leak(cfg), statelayout.has_dur_plane(cfg),
                                statelayout.split_p(cfg))


def rows_of(cfg, snap, B=None):
    """A snapshot of B envs as one (B, bytes per env) uint8 array per section."""
    B = cfg.num_envs if B is None else B
    out, off = [], 0
    for _, dt, n in layout(cfg, B):
        nb = np.dtype(dt).itemsize * n
        out.append(np.frombuffer(snap[off:off + nb], np.uint8).reshape(B, -1))
        off += nb
    assert off == len(snap)
    return out


def composite(cfg, saved, cur, src):
    """The state after a load: env b has the saved snapshot's rows of env src[b] where
    0 <= src[b] < B, else its rows of the current snapshot."""
    B = cfg.num_envs
    parts = []
    for sv, cu in zip(rows_of(cfg, saved), rows_of(cfg, cur)):
        cu = cu.copy()
        for b in range(B):
            if 0 <= src[b] < B:
                cu[b] = sv[src[b]]
        parts.append(cu.tobytes())
    return b"".join(parts)


def one_env(cfg, snap, b):
    """Env b of a B-env snapshot as a one-env snapshot."""
    return b"".join(r[b].tobytes() for r in rows_of(cfg, snap))


def expected_obs(saved_obs, last_obs, src):
    B = len(src)
    out = last_obs.copy()
    for b in range(B):
        if 0 <= src[b] < B:
            out[b] = saved_obs[src[b]]
    return out


def masked(B):
    """Every third env restored, as an index list (-1: keep)."""
    return [b if b % 3 == 0 else -1 for b in range(B)]


class Snapshots:
    """A list of one-env snapshots as compare_state's reference side."""

    def __init__(self, snaps):
        self.snaps = snaps

    def state_bytes(self):
        return self.snaps


# ------------------------------------------------------------------ host (no GPU)

def _oracle(oracle_mod, B, S, kw, **over):
    from marllb_amd.env import make_config
    return oracle_mod.OracleEnv(make_config(B, S, **{**kw, **over}))


def test_identity_composite_continues_the_oracle(oracle_mod):
    """The construction is sound: an oracle loaded with the composite of its own snapshot (every
    env from itself) is that snapshot, and continues exactly as the oracle it came from."""
    B, S, kw = 5, 4, {"seed": 11}
    a, b = _oracle(oracle_mod, B, S, kw), _oracle(oracle_mod, B, S, kw)
    a.reset()
    rng = np.random.default_rng(0)
    for _ in range(4):
        a.step(actions(rng, B, S, kw))
    s = a.state_bytes()
    comp = composite(a.cfg, s, s, list(range(B)))
    assert comp == s
    assert composite(a.cfg, s, s, [-1] * B) == s
    b.load_state(comp)
    for _ in range(6):
        act = actions(rng, B, S, kw)
        for x, y in zip(a.step(act), b.step(act)):
            np.testing.assert_array_equal(x, y)
    assert a.state_bytes() == b.state_bytes()
    a.close()
    b.close()


@pytest.mark.parametrize("kw", [{}, LOST_FIN], ids=["default", "lost-fin"])
def test_permuted_composite_equals_one_env_oracles(oracle_mod, kw):
    """A fork by hand: a B-env oracle loaded with a permuted composite equals, env by env, the
    one-env oracles (env_id_offset = b) loaded with the one-env slices the permutation names."""
    B, S = 5, 4
    kw = {"seed": 12, **kw}
    ora = _oracle(oracle_mod, B, S, kw)
    ora.reset()
    rng = np.random.default_rng(1)
    for _ in range(4):
        ora.step(actions(rng, B, S, kw))
    saved = ora.state_bytes()
    for _ in range(3):
        ora.step(actions(rng, B, S, kw))
    cur = ora.state_bytes()
    src = [2, 0, -1, 4, 1]
    ora.load_state(composite(ora.cfg, saved, cur, src))
    ones = [_oracle(oracle_mod, 1, S, kw, env_id_offset=b) for b in range(B)]
    for b, o in enumerate(ones):
        o.load_state(one_env(ora.cfg, saved, src[b]) if src[b] >= 0 else one_env(ora.cfg, cur, b))
    for _ in range(4):
        act = actions(rng, B, S, kw)
        got = ora.step(act)
        want = [o.step(act[b:b + 1]) for b, o in enumerate(ones)]
        for i in range(4):
            np.testing.assert_array_equal(got[i], np.concatenate([w[i] for w in want]))
    compare_state(ora, Snapshots([o.state_bytes() for o in ones]), ora.cfg)
    # the permuted envs did not simply continue: env 0 now holds what env 2 had saved
    assert one_env(ora.cfg, saved, 2) != one_env(ora.cfg, saved, 0)
    for o in [ora, *ones]:
        o.close()


def test_signature_table_declares_the_exports():
    from marllb_amd import _lib
    declared = _lib.header_functions()
    for n in ("lbsim_state_save", "lbsim_state_load"):
        assert n in _lib._SIGNATURES and n in declared
        assert len(_lib._SIGNATURES[n][1]) == 5


def test_null_arguments_are_einval():
    """No GPU work: the argument checks come first."""
    from marllb_amd import _lib
    L = _lib.load()
    assert L.lbsim_state_save(None, None, 0, None, None) == _lib.EINVAL
    assert L.lbsim_state_load(None, None, 0, None, None) == _lib.EINVAL
    buf = ctypes.create_string_buffer(64)
    assert L.lbsim_state_save(None, buf, 64, None, None) == _lib.EINVAL
    assert L.lbsim_state_load(None, buf, 64, None, None) == _lib.EINVAL
    assert b"handle is NULL" in L.lbsim_last_error(None)
    assert L.lbsim_abi_version() == 10


def _probe_cases():
    """(B, buffer shift, bytes per env of each section) of the handles the GPU tests use."""
    from marllb_amd.env import make_config
    out = []
    for B in (1, 5, 16, 48, 130):
        for S, kw in ((3, {}), (4, {}), (4, {"normalize_obs": True, "fail_prob": 0.05}),
                      (4, LOST_FIN), (8, {"duration_mode": "service"}), (16, {}), (16, LOST_FIN),
                      (64, {"queue_capacity": 64})):
            cfg = make_config(B, S, seed=1, **kw)
            rows = [np.dtype(dt).itemsize * n // B for _, dt, n in layout(cfg)]
            out.append((B, 0, rows))
    # a buffer off the 16-byte grid: 4-byte units everywhere (16 x 4 default, 48 x 16 default)
    for B, shift in ((16, 4), (48, 8)):
        rows = next(r for b, _, r in out if b == B and len(r) == 18 and r[14] == (256 * 4 if B == 16
                                                                                 else 256 * 16))
        out.append((B, shift, rows))
    return out


def test_kernel_body_on_the_host(tmp_path):
    """csrc/lbsim_snapshot.h as host C++ (tests/snapshot_probe.cpp): the section table and the
    kernel's per-thread body, every thread of every block, give a full save, a masked save, an
    indexed load and an identity load that match a byte-wise reference and touch no guard byte."""
    from marllb_amd import build
    exe = str(tmp_path / "snapshot_probe")
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-O1", "-Wall", "-o", exe,
                    os.path.join(HERE, "snapshot_probe.cpp")], check=True)
    cases = _probe_cases()
    text = "".join(f"{B} {shift} " + " ".join(map(str, rows)) + "\n" for B, shift, rows in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    res = [json.loads(line) for line in r.stdout.splitlines()]
    assert len(res) == len(cases), r.stderr[-2000:]
    for (B, shift, rows), got in zip(cases, res):
        assert got["ok"], (B, shift, rows, got)
        assert got["sections"] == len(rows)
        assert got["long"] == sum(x >= 256 for x in rows)
        if shift:
            assert got["wide"] == 0
    assert r.returncode == 0
    # the headline shape's sections that can take 16-byte units do (B a multiple of 4)
    B, _, rows = next(c for c in cases if c[0] == 16 and len(c[2]) == 18 and c[2][14] == 1024)
    assert res[cases.index((B, 0, rows))]["wide"] == sum(x % 16 == 0 for x in rows)


# ------------------------------------------------------------------ GPU

def make_pair(oracle_mod, B, S, kw, env_kw=None):
    """A GPU env and the oracle of the same config, both reset and `pre` steps in."""
    from marllb_amd.env import VecLoadBalanceEnv
    env = VecLoadBalanceEnv(B, S, device="cuda:0", **{"autoreset": False, **(env_kw or {})}, **kw)
    ref = oracle_mod.OracleEnv(env.cfg, trace=kw.get("trace"))
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    return env, ref


def run_steps(env, ref, rng, kw, n, k0=0):
    B, S = env.num_envs, env.num_servers
    for k in range(n):
        step_both(env, ref, actions(rng, B, S, kw), k0 + k)


def _trace():
    from marllb_amd import trace
    return trace.synthetic(37, 300.0, seed=7)


# id: (B, S, config kwargs, VecLoadBalanceEnv kwargs)
BYTES_CASES = {
    "default": (16, 4, {}, None),
    "odd-5x3": (5, 3, {}, None),
    "normalize": (16, 4, {"normalize_obs": True}, None),
    "fail": (16, 4, {"fail_prob": 0.05}, None),
    "lost-fin-vpp": (16, 4, LOST_FIN, None),
    "service": (16, 4, {"duration_mode": "service"}, None),
    "s16-nextstep": (16, 16, {"max_steps": 3}, NEXT_STEP),
    "trace": (16, 4, {"trace": None}, None),
}


@gpu
@pytest.mark.parametrize("case", list(BYTES_CASES))
def test_full_save_is_get_state(lib, case):
    """After reset + 4 steps a buffer written by state_save of all envs, copied to the host, is
    handle.state_bytes(); loaded into a second handle it is that handle's state_bytes() too."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, kw, env_kw = BYTES_CASES[case]
    kw = {"seed": 40, **kw}
    if "trace" in kw:
        kw["trace"] = _trace()
    envs = [VecLoadBalanceEnv(B, S, device="cuda:0", **{"autoreset": False, **(env_kw or {})},
                              **kw) for _ in range(2)]
    env, twin = envs
    env.reset()
    rng = np.random.default_rng(2)
    for _ in range(4):
        env.step(torch.from_numpy(actions(rng, B, S, kw)))
    n = env.handle.state_size()
    buf = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda:0")
    env.handle.state_save(buf)
    want = env.handle.state_bytes()
    assert len(want) == n
    assert buf.cpu().numpy().tobytes() == want
    twin.handle.state_load(buf)
    assert twin.handle.state_bytes() == want
    for e in envs:
        e.close()


@gpu
def test_rewind_is_common_random_numbers(lib, oracle_mod):
    """Save; 5 steps on actions A; restore; A again gives the same outputs and final state;
    restore; other actions equal the oracle loaded from the saved snapshot and stepped on them."""
    B, S, kw = 16, 4, {"seed": 41}
    env, ref = make_pair(oracle_mod, B, S, kw)
    rng = np.random.default_rng(3)
    run_steps(env, ref, rng, kw, 4)
    snap, saved = env.snapshot(), ref.state_bytes()
    obs_saved = snap.obs.cpu().numpy().copy()
    A = [actions(rng, B, S, kw) for _ in range(5)]
    A2 = [actions(rng, B, S, kw) for _ in range(5)]
    assert any((x != y).any() for x, y in zip(A, A2))

    def one_pass():
        outs = []
        for a in A:
            o, r, d, info = env.step(torch.from_numpy(a), assign_counts=True)
            outs.append([t.cpu().numpy().copy() for t in (o, r, d, info["assign_counts"])])
        return outs, env.get_state()

    first, state1 = one_pass()
    np.testing.assert_array_equal(env.restore(snap).cpu().numpy(), obs_saved)
    second, state2 = one_pass()
    for k, (x, y) in enumerate(zip(first, second)):
        for u, v in zip(x, y):
            np.testing.assert_array_equal(u, v, err_msg=f"step {k}")
    assert state1 == state2
    env.restore(snap)
    ref.load_state(saved)
    for k, a in enumerate(A2):
        step_both(env, ref, a, 4 + k)
    compare_state(env.handle, ref, env.cfg)
    assert env.get_state() != state1  # other actions, another future
    env.close()
    ref.close()


# id: (dyn_mapping, B, S): the env-per-lane form, the default form, the server-per-lane groups
RESTORE_CASES = {"env-16x4": ("env", 16, 4), "auto-16x4": ("auto", 16, 4),
                 "group-16x16": ("server", 16, 16)}


@gpu
@pytest.mark.parametrize("case", list(RESTORE_CASES))
def test_masked_restore(lib, oracle_mod, case):
    """Save at step 4; at step 9 every third env goes back, the others keep going: the returned
    batch, 4 more steps and the whole state equal the composite reference."""
    mapping, B, S = RESTORE_CASES[case]
    kw = {"seed": 42, "dyn_mapping": mapping}
    env, ref = make_pair(oracle_mod, B, S, kw)
    rng = np.random.default_rng(4)
    run_steps(env, ref, rng, kw, 4)
    snap, saved = env.snapshot(), ref.state_bytes()
    obs_saved = snap.obs.cpu().numpy().copy()
    run_steps(env, ref, rng, kw, 5, 4)
    last = env._last_obs.cpu().numpy().copy()
    src = masked(B)
    mask = torch.tensor([s >= 0 for s in src])
    obs = env.restore(snap, mask=mask).cpu().numpy()
    np.testing.assert_array_equal(obs, expected_obs(obs_saved, last, src))
    assert (obs_saved[0] != last[0]).any()
    ref.load_state(composite(env.cfg, saved, ref.state_bytes(), src))
    compare_state(env.handle, ref, env.cfg)
    run_steps(env, ref, rng, kw, 4, 9)
    compare_state(env.handle, ref, env.cfg)

    def default(kern, names):
        if mapping == "env":
            assert kern == ENV_LANE, (kern, names)
        elif S > 8:
            assert kern == GROUP, (kern, names)
        else:
            assert kern != ENV_LANE, (kern, names)

    parity.check_dispatch(lib, env, default,
                          forced_group=None if mapping == "env" else "dynamics_group_kernel",
                          forced_wave=mapping != "env" and S <= 8)
    env.close()
    ref.close()


@gpu
@pytest.mark.parametrize("over", [{"LBSIM_DYN_GROUP_LANES": "4"}, {"LBSIM_DYN_WAVE": "1"}],
                         ids=["group-lanes-4", "wave"])
def test_masked_restore_under_forced_forms(over):
    """The masked-restore cases in a child process under the dynamics overrides (read once per
    process): 4-lane groups, one wave per env."""
    parity.run_cases_in_child("test_state_snapshot.py",
                              [f"test_masked_restore[{c}]" for c in RESTORE_CASES], over)


@gpu
@pytest.mark.parametrize("case", ["default", "odd-5x3", "lost-fin-vpp"])
def test_masked_save(lib, case):
    """A buffer prefilled with 0xA5, saved with a mask: the rows of the envs outside the mask are
    still 0xA5 in every section, the masked rows are state_bytes()'s."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, kw, _ = BYTES_CASES[case]
    env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=43, autoreset=False, **kw)
    env.reset()
    rng = np.random.default_rng(5)
    for _ in range(3):
        env.step(torch.from_numpy(actions(rng, B, S, kw)))
    mask = np.arange(B) % 3 == 1
    buf = torch.full((env.handle.state_size(),), 0xA5, dtype=torch.uint8, device="cuda:0")
    env.handle.state_save(buf, torch.from_numpy(mask.astype(np.uint8) * 7).to("cuda:0"))
    got = rows_of(env.cfg, buf.cpu().numpy().tobytes())
    want = rows_of(env.cfg, env.handle.state_bytes())
    for (name, _, _), g, w in zip(layout(env.cfg), got, want):
        np.testing.assert_array_equal(g[mask], w[mask], err_msg=name)
        assert (g[~mask] == 0xA5).all(), name
    env.close()


FORK_SRC = [3, 3, 2, 3, -1, 5, 16, 0, 0, 9, 12, 12, 1, 99, 14, 7]
FORK_CASES = {"default": (4, {}), "lost-fin-vpp": (4, LOST_FIN), "s16": (16, {})}


@gpu
@pytest.mark.parametrize("case", list(FORK_CASES))
@pytest.mark.parametrize("which", ["mixed", "broadcast"])
def test_fork(lib, oracle_mod, case, which):
    """restore(src=...): repeats, identity entries, -1 and entries >= B (both keep), and the
    broadcast src = 0; the outputs of 4 steps and the state equal the composite reference."""
    B = 16
    S, kw = FORK_CASES[case]
    kw = {"seed": 44, **kw}
    src = FORK_SRC if which == "mixed" else [0] * B
    env, ref = make_pair(oracle_mod, B, S, kw)
    rng = np.random.default_rng(6)
    run_steps(env, ref, rng, kw, 4)
    snap, saved = env.snapshot(), ref.state_bytes()
    obs_saved = snap.obs.cpu().numpy().copy()
    run_steps(env, ref, rng, kw, 3, 4)
    last = env._last_obs.cpu().numpy().copy()
    obs = env.restore(snap, src=torch.tensor(src)).cpu().numpy()
    np.testing.assert_array_equal(obs, expected_obs(obs_saved, last, src))
    ref.load_state(composite(env.cfg, saved, ref.state_bytes(), src))
    st = compare_state(env.handle, ref, env.cfg)
    if which == "broadcast":  # the copies share the one arrival already drawn
        assert (st["next_arr"] == st["next_arr"][0]).all()
        assert (st["next_work"] == st["next_work"][0]).all()
    run_steps(env, ref, rng, kw, 4, 7)
    st = compare_state(env.handle, ref, env.cfg)
    if which == "broadcast":  # ... and draw everything after it with their own ids
        final = env._last_obs.cpu().numpy().reshape(B, -1)
        assert len(np.unique(final, axis=0)) >= 2
        assert len(np.unique(st["next_arr"])) >= 2
    env.close()
    ref.close()


@gpu
def test_mask_wins_over_src(lib, oracle_mod):
    """restore(mask=, src=): the envs outside the mask keep their state whatever src says."""
    B, S, kw = 16, 4, {"seed": 45}
    env, ref = make_pair(oracle_mod, B, S, kw)
    rng = np.random.default_rng(7)
    run_steps(env, ref, rng, kw, 3)
    snap, saved = env.snapshot(), ref.state_bytes()
    run_steps(env, ref, rng, kw, 2, 3)
    mask = np.arange(B) % 2 == 0
    src = [s if m else -1 for s, m in zip(FORK_SRC, mask)]
    env.restore(snap, mask=torch.from_numpy(mask), src=np.array(FORK_SRC))
    ref.load_state(composite(env.cfg, saved, ref.state_bytes(), src))
    run_steps(env, ref, rng, kw, 3, 5)
    compare_state(env.handle, ref, env.cfg)
    env.close()
    ref.close()


@gpu
def test_shard_fork(lib, oracle_mod):
    """A handle with env_id_offset = 32: a fork equals an oracle with the same offset (the copies'
    draws are keyed by global ids 32 + b)."""
    B, S, kw = 16, 4, {"seed": 46, "env_id_offset": 32}
    env, ref = make_pair(oracle_mod, B, S, kw)
    assert ref.cfg.env_id_offset == 32
    rng = np.random.default_rng(8)
    run_steps(env, ref, rng, kw, 4)
    snap, saved = env.snapshot(), ref.state_bytes()
    run_steps(env, ref, rng, kw, 2, 4)
    env.restore(snap, src=torch.tensor(FORK_SRC, dtype=torch.int32, device="cuda:0"))
    ref.load_state(composite(env.cfg, saved, ref.state_bytes(), FORK_SRC))
    run_steps(env, ref, rng, kw, 4, 6)
    compare_state(env.handle, ref, env.cfg)
    env.close()
    ref.close()


@gpu
def test_graph_replays_restore_and_steps(lib, oracle_mod):
    """graph_mode: restore(snap), step, step captured into one graph.  Three replays give the same
    outputs, the oracle's two steps from the saved state; after snapshot(out=snap) at a later
    state a further replay follows the new state with no new capture."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, kw = 16, 4, {"seed": 47}
    env = VecLoadBalanceEnv(B, S, device="cuda:0", graph_mode=True, **kw)
    ref = oracle_mod.OracleEnv(env.cfg)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    rng = np.random.default_rng(9)
    run_steps(env, ref, rng, kw, 3)
    snap, saved = env.snapshot(), ref.state_bytes()
    acts = [actions(rng, B, S, kw) for _ in range(2)]
    a_dev = [torch.from_numpy(a).to("cuda:0") for a in acts]

    def body():
        env.restore(snap)
        o1, r1, _, _ = env.step(a_dev[0])
        o1, r1 = o1.clone(), r1.clone()  # the step's outputs are buffers the next step rewrites
        o2, r2, _, _ = env.step(a_dev[1])
        return o1, r1, o2, r2

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up, eager
        body()
    torch.cuda.current_stream().wait_stream(side)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        outs = body()

    def expect():
        w1, w2 = ref.step(acts[0]), ref.step(acts[1])
        return w1[0], w1[1], w2[0], w2[1]

    ref.load_state(saved)
    want = expect()
    for k in range(3):
        cg.replay()
        for g, w in zip(outs, want):
            np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg=f"replay {k}")
    compare_state(env.handle, ref, env.cfg)
    env.snapshot(out=snap)  # the state two steps on, into the same buffers
    want2 = expect()
    assert (want2[0] != want[0]).any()
    cg.replay()
    for g, w in zip(outs, want2):
        np.testing.assert_array_equal(g.cpu().numpy(), w, err_msg="replay after snapshot(out=)")
    compare_state(env.handle, ref, env.cfg)
    env.close()
    ref.close()


@gpu
def test_rates_and_flow_stats_stay_with_the_slot(lib, oracle_mod):
    """flow_stats=True with per-env rates: a fork changes neither the flow statistics nor the
    rates, and the loaded envs go on at their slots' rates -- equal to per-env oracles created
    with those rates and loaded with the snapshots the fork names."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, kw = 16, 4, {"seed": 48}
    r, mu = make_rates(B, S, 91)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=False, flow_stats=True, **kw)
    ora = PerEnvOracles(oracle_mod, B, S, kw, r, mu)
    env.set_rates(r, mu)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ora.reset())
    rng = np.random.default_rng(10)
    run_steps(env, ora, rng, kw, 4)
    snap, saved = env.snapshot(), ora.state_bytes()
    run_steps(env, ora, rng, kw, 3, 4)
    before = env.flow_stats(per_server=True, hist=True)
    assert int(before["count"].sum()) > 0
    env.restore(snap, src=torch.tensor(FORK_SRC))
    after = env.flow_stats(per_server=True, hist=True)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    np.testing.assert_array_equal(env.rates[0].cpu().numpy(), r)
    np.testing.assert_array_equal(env.rates[1].cpu().numpy(), mu)
    for b, s in enumerate(FORK_SRC):
        if 0 <= s < B:
            ora.envs[b].load_state(saved[s])
    run_steps(env, ora, rng, kw, 4, 7)
    compare_state(env.handle, ora, env.cfg)
    ora.close()
    env.close()


@gpu
def test_errors(lib):
    from marllb_amd.env import VecLoadBalanceEnv
    B, S = 16, 4
    env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=49, autoreset=False)
    fresh = VecLoadBalanceEnv(B, S, device="cuda:0", seed=49, autoreset=False)
    h, n = env.handle, env.handle.state_size()
    big = torch.zeros(n + 32, dtype=torch.uint8, device="cuda:0")
    for call in (h.state_save, h.state_load):
        with pytest.raises(lib.LbsimError, match=f"{n - 16} bytes, need {n}") as ei:
            call(big[:n - 16])
        assert ei.value.code == lib.ESHAPE
        with pytest.raises(ValueError, match="16-byte aligned"):
            call(big[1:1 + n])
        with pytest.raises(ValueError, match="16-byte aligned"):
            call(big[:n][1:])
    assert b"16-byte aligned" in lib.load().lbsim_last_error(h.h)
    with pytest.raises(ValueError, match="dev_buf is NULL"):
        lib.check(lib.load().lbsim_state_save(h.h, None, n, None, None), h.h)
    src = torch.arange(B, dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError, match="reset or loaded"):
        fresh.handle.state_load(big[:n], src)
    with pytest.raises(RuntimeError, match="reset"):
        fresh.snapshot()
    env.reset()
    with pytest.raises(ValueError, match="out="):
        env.snapshot(mask=torch.ones(B, dtype=torch.bool))
    snap = env.snapshot()
    with pytest.raises(ValueError, match="integer"):
        env.restore(snap, src=torch.zeros(B))
    with pytest.raises(ValueError, match="num_envs"):
        env.restore(snap, src=torch.zeros(B + 1, dtype=torch.int64))
    # a load of every env initialises a handle, as set_state does: it steps like the saved one
    fresh.restore(snap)
    a = torch.from_numpy(np.random.default_rng(0).integers(0, 3, (B, S)))
    x, y = env.step(a), fresh.step(a)
    assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    fresh.handle.state_load(snap.state, src)  # and now takes indices
    assert env.get_state() != snap.state.cpu().numpy().tobytes()
    assert lib.load().lbsim_abi_version() == 10
    env.close()
    fresh.close()


@gpu
def test_masked_snapshot_refreshes_rows(lib):
    """snapshot(mask=, out=): the masked envs' state and observation rows are refreshed, the
    others keep what the snapshot held."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S = 16, 4
    env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=50, autoreset=False)
    env.reset()
    a = torch.from_numpy(np.random.default_rng(1).integers(0, 3, (B, S)))
    env.step(a)
    snap = env.snapshot()
    old_state, old_obs = snap.state.cpu().numpy().tobytes(), snap.obs.cpu().numpy().copy()
    for _ in range(2):
        env.step(a)
    mask = np.arange(B) % 4 == 0
    assert env.snapshot(mask=torch.from_numpy(mask), out=snap) is snap
    src = [b if mask[b] else -1 for b in range(B)]
    assert snap.state.cpu().numpy().tobytes() == composite(env.cfg, env.get_state(), old_state, src)
    np.testing.assert_array_equal(snap.obs.cpu().numpy(),
                                  expected_obs(env._last_obs.cpu().numpy(), old_obs, src))
    env.close()


@gpu
def test_upstream_returns_follow_a_restore(lib):
    """feature_mode="upstream": the facade's own episode returns are part of the snapshot."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S = 5, 4
    env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=51, autoreset=False,
                            feature_mode="upstream", reservoir_mode="vpp")
    env.reset()
    a = torch.from_numpy(np.random.default_rng(2).integers(0, 3, (B, S)))
    env.step(a)
    snap = env.snapshot()

    def two():
        out = []
        for _ in range(2):
            o, r, _, info = env.step(a)
            out.append((o.clone(), r.clone(), info["episode_return"].clone()))
        return out

    first = two()
    obs = env.restore(snap)
    assert torch.equal(obs, snap.obs)
    for x, y in zip(first, two()):
        for u, v in zip(x, y):
            assert torch.equal(u, v)
    env.close()


@gpu
def test_drop_in_env_rewinds(lib):
    """LoadBalanceEnv: snapshot, three steps, restore, the same three actions give identical
    observations and rewards (and the facade's step count and return follow)."""
    from marllb_amd import DeviceSnapshot, LoadBalanceEnv
    env = LoadBalanceEnv(num_servers=4, seed=52, normalize_obs=True, max_steps=50)
    env.reset()
    rng = np.random.default_rng(3)
    o0 = None
    for _ in range(2):
        o0 = env.step(rng.integers(0, 3, 4))[0]
    snap = env.snapshot()
    assert isinstance(snap, DeviceSnapshot)
    acts = [rng.integers(0, 3, 4) for _ in range(3)]

    def three():
        return [env.step(a) for a in acts]

    first = three()
    assert env.current_step == 5
    np.testing.assert_array_equal(env.restore(snap), o0)
    assert env.current_step == 2
    for x, y in zip(first, three()):
        np.testing.assert_array_equal(x[0], y[0])
        assert x[1] == y[1] and x[2] == y[2]
        assert x[3]["step"] == y[3]["step"] and x[3]["episode_return"] == y[3]["episode_return"]
    # straight after a restore (no step in between) a snapshot holds the restored observation
    np.testing.assert_array_equal(env.restore(snap), o0)
    again = env.snapshot()
    np.testing.assert_array_equal(again.obs[0].cpu().numpy(), o0)
    assert again.state.cpu().numpy().tobytes() == snap.state.cpu().numpy().tobytes()
    env.close()
