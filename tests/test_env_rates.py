"""Per-env arrival and server rates (lbsim_set_env_rates, VecLoadBalanceEnv.set_rates).

The RNG is keyed by global env id, so one GPU handle of B heterogeneous envs must equal B one-env
oracle handles (env_id_offset = b), each created with that env's own rates: every comparison here
is bit for bit, observations, rewards, done flags, assignment counts and the device state.
"""
import numpy as np
import pytest

from tests import parity, statelayout
from tests.parity import ENV_LANE, GROUP, WAVE, actions, compare_state, lib, step_both  # noqa: F401

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu


def make_rates(B, S, seed):
    """Arrival log-uniform in [50, 2000] flows/s, per-env load arrival / sum(server) uniform in
    [0.3, 1.4], servers skewed up to 4 : 1; f32.  An env with a server below the config's minimum
    of 1 flow/s (S = 16: a slow, overloaded env's smallest share) is drawn again."""
    rng = np.random.default_rng(seed)

    def draw(n):
        r = np.exp(rng.uniform(np.log(50.0), np.log(2000.0), n))
        load = rng.uniform(0.3, 1.4, n)
        skew = rng.uniform(1.0, 4.0, (n, S))
        mu = (r / load)[:, None] * skew / skew.sum(axis=1, keepdims=True)
        return r.astype(np.float32), mu.astype(np.float32)

    r, mu = draw(B)
    while True:
        low = np.flatnonzero(mu.min(axis=1) < 1.0)
        if low.size == 0:
            return r, mu
        r[low], mu[low] = draw(low.size)


class PerEnvOracles:
    """B one-env oracle handles, env b with env_id_offset = offset + b and its own rates (r / mu
    None: the shared ones of kw), stepped with row b of the actions; results stacked."""

    def __init__(self, oracle_mod, B, S, kw, r, mu, offset=0):
        from marllb_amd.env import make_config
        self.B, self.S = B, S
        self.envs = []
        for b in range(B):
            rk = {}
            if r is not None:
                rk["arrival_rate"] = float(r[b])
            if mu is not None:
                rk["server_rates"] = mu[b].tolist()
            cfg = make_config(1, S, env_id_offset=offset + b, **{**kw, **rk})
            self.envs.append(oracle_mod.OracleEnv(cfg, trace=kw.get("trace")))

    def reset(self, mask=None, obs=None):
        if mask is None:
            return np.concatenate([o.reset() for o in self.envs])
        out = obs.copy()
        for b, o in enumerate(self.envs):
            if mask[b]:
                out[b:b + 1] = o.reset(mask=np.ones(1, np.uint8), obs=out[b:b + 1].copy())
        return out

    def step(self, a):
        res = [o.step(a[b:b + 1]) for b, o in enumerate(self.envs)]
        return tuple(np.concatenate([x[i] for x in res]) for i in range(4))

    def state_bytes(self):
        """One-env snapshots in env order (parity.compare_state stacks them)."""
        return [o.state_bytes() for o in self.envs]

    def with_rates(self, oracle_mod, kw, r, mu, offset=0):
        """New one-env oracles with other rates that continue from these oracles' states."""
        new = PerEnvOracles(oracle_mod, self.B, self.S, kw, r, mu, offset)
        for o, n in zip(self.envs, new.envs):
            n.load_state(o.state_bytes())
        return new

    def close(self):
        for o in self.envs:
            o.close()


def check_kernel(lib, env, mapping, kw, expect):
    """parity.check_dispatch with the case's expected kernel form as the default."""
    def default(kern, names):
        if expect == "env_lane":
            assert kern == ENV_LANE and names.get(0, "").startswith("dynamics_kernel<"), (kern, names)
        elif expect == "group":
            assert kern == GROUP and names.get(0, "").startswith("dynamics_group_"), (kern, names)
        elif expect == "fused":
            assert kern == GROUP and names.get(4, "").startswith("fused_step_kernel<"), (kern, names)
        elif expect == "step_wave":
            assert kern == WAVE and names.get(4, "").startswith("step_wave_kernel<"), (kern, names)
        elif expect == "wave_split":  # next-step auto-reset handles step in two launches
            assert kern == WAVE and names.get(0, "").startswith("dynamics_wave_kernel<"), (kern, names)
        else:
            raise AssertionError(expect)

    fits_wave = (mapping != "env" and env.cfg.num_servers <= 8 and kw.get("queue_capacity", 32) <= 32
                 and kw.get("assign_policy") != "alias" and not kw.get("fail_prob")
                 and not kw.get("lost_fin_prob"))
    group = None if mapping == "env" else "" if kw.get("step_kernel") == "fused" else "dynamics_group_kernel"
    parity.check_dispatch(lib, env, default, forced_group=group, forced_wave=fits_wave)


def run_vs_oracles(lib, oracle_mod, B, S, kw, mapping, expect, seed, r, mu, env_kw=None):
    """parity.run_vs_reference on a handle with the rates r / mu against per-env oracles, the
    kernel form checked after step 12.  Returns the stacked oracle state after step 12."""
    from marllb_amd.env import VecLoadBalanceEnv
    kw = dict(kw)
    if mapping == "server-fused":
        mapping, kw["step_kernel"] = "server", "fused"
    env = VecLoadBalanceEnv(B, S, device="cuda:0", dyn_mapping=mapping,
                            **{"autoreset": False, **(env_kw or {})}, **kw)
    okw = dict(kw)
    if env.next_step:
        okw["next_step_reset"] = True
    ora = PerEnvOracles(oracle_mod, B, S, okw, r, mu)
    env.set_rates(None if r is None else r, None if mu is None else torch.from_numpy(mu))
    mid = parity.run_vs_reference(env, ora, kw, seed,
                                  hook=lambda e: check_kernel(lib, e, mapping, kw, expect))
    ora.close()
    env.close()
    return mid


ALIAS = {"assign_policy": "alias", "action_type": "continuous"}
NEXT_STEP = {"autoreset": True, "autoreset_mode": "next_step"}
# id: (B, S, mapping, config kwargs, kernel form expected by default, VecLoadBalanceEnv kwargs)
CASES = {
    "wave-67x4": (67, 4, "auto", {}, "step_wave", None),
    "wave-67x3-warmup3": (67, 3, "auto", {"warmup_steps": 3}, "step_wave", None),
    "wave-35x8": (35, 8, "auto", {}, "step_wave", None),
    "wave-67x4-nextstep": (67, 4, "auto", {"max_steps": 5}, "wave_split", NEXT_STEP),
    "wave-67x4-q4": (67, 4, "auto", {"queue_capacity": 4}, "step_wave", None),
    "env-67x4-norm": (67, 4, "env", {"normalize_obs": True}, "env_lane", None),
    "env-67x3": (67, 3, "env", {}, "env_lane", None),
    "env-35x8": (35, 8, "env", {}, "env_lane", None),
    "env-19x16": (19, 16, "env", {}, "env_lane", None),
    "group-67x4-alias": (67, 4, "server", ALIAS, "group", None),
    "group-67x3-alias": (67, 3, "server", ALIAS, "group", None),
    "group-35x8-fail": (35, 8, "server", {"fail_prob": 0.05}, "group", None),
    "group-19x16": (19, 16, "server", {}, "group", None),
    "fused-67x4-alias": (67, 4, "server-fused", ALIAS, "fused", None),
    "fused-35x8-fail": (35, 8, "server-fused", {"fail_prob": 0.05}, "fused", None),
    "fused-19x16": (19, 16, "server-fused", {}, "fused", None),
}
RATE_SEED = 11


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_bit_exact_vs_per_env_oracles(lib, oracle_mod, case):
    """Every dynamics form with heterogeneous arrival and server rates against per-env oracles."""
    B, S, mapping, kw, expect, env_kw = CASES[case]
    idx = list(CASES).index(case)
    r, mu = make_rates(B, S, RATE_SEED + S)
    mid = run_vs_oracles(lib, oracle_mod, B, S, {"seed": 300 + idx, **kw}, mapping, expect, idx,
                         r, mu, env_kw)
    if kw.get("queue_capacity") == 4:
        # the small queues make the per-env load visible in the state: overloaded envs drop
        # flows, lightly loaded ones do not (read on the oracle side alone)
        assert (mid["dropped"] > 0).any() and (mid["dropped"] == 0).any(), mid["dropped"]


def _child(env_over):
    """This file's S <= 4 cases in a child process (the overrides are read once per process)."""
    ks = [f"test_bit_exact_vs_per_env_oracles[{c}]" for c, v in CASES.items() if v[1] <= 4]
    assert len(ks) >= 8
    parity.run_cases_in_child("test_env_rates.py", ks, env_over)


@gpu
def test_headline_four_lane_groups_bit_exact():
    """LBSIM_DYN_GROUP_LANES=4: the headline 65536 x 4 kernel (4-lane groups) on the S <= 4 cases."""
    _child({"LBSIM_DYN_GROUP_LANES": "4"})


@gpu
def test_wave_dynamics_bit_exact():
    """LBSIM_DYN_WAVE=1: the one-wave-per-env dynamics on every S <= 4 case it applies to."""
    _child({"LBSIM_DYN_WAVE": "1"})


@gpu
@pytest.mark.parametrize("which", ["lost_fin", "trace"])
def test_server_rates_only_on_restricted_handles(lib, oracle_mod, which):
    """Lost-FIN and TRACE handles take per-env server rates (with the shared arrival rate)."""
    from marllb_amd import trace
    B, S = 35, 4
    kw = ({"lost_fin_prob": 0.2, "flow_timeout": 0.5, "lost_fin_pending": 8} if which == "lost_fin"
          else {"trace": trace.synthetic(37, 300.0, seed=7)})
    shared = 400.0 if which == "lost_fin" else kw["trace"].rate  # the handle's arrival rate
    r, mu = make_rates(B, S, RATE_SEED)
    mu = (mu * (shared / r)[:, None]).astype(np.float32)  # the same per-env loads at that rate
    assert mu.min() >= 1.0
    expect = "group" if which == "lost_fin" else "step_wave"
    run_vs_oracles(lib, oracle_mod, B, S, {"seed": 41, **kw}, "auto", expect, 5, None, mu)


@gpu
def test_mid_run_change(lib, oracle_mod):
    """set_rates after 6 steps: the oracle side continues in B new one-env oracles created with
    the new rates that load the old oracles' states (the next arrival already drawn keeps its time
    and work; every later gap and service time uses the new rates)."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, kw = 67, 4, {"seed": 77}
    r0, mu0 = make_rates(B, S, 21)
    r1, mu1 = make_rates(B, S, 22)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=False, **kw)
    ora = PerEnvOracles(oracle_mod, B, S, kw, r0, mu0)
    env.set_rates(r0, mu0)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ora.reset())
    rng = np.random.default_rng(3)
    for k in range(6):
        step_both(env, ora, actions(rng, B, S, kw), k)
    env.set_rates(torch.from_numpy(r1).to("cuda:0"), mu1)
    new = ora.with_rates(oracle_mod, kw, r1, mu1)
    ora.close()
    for k in range(6, 12):
        step_both(env, new, actions(rng, B, S, kw), k)
    compare_state(env.handle, new, env.cfg)
    a, m = env.rates
    np.testing.assert_array_equal(a.cpu().numpy(), r1)
    np.testing.assert_array_equal(m.cpu().numpy(), mu1)
    new.close()
    env.close()


@gpu
def test_off_means_off(lib):
    """No rates, rates equal to the config's, and rates set then cleared give identical outputs
    and states; heterogeneous rates do not (the arrays are read)."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S = 67, 4
    r, mu = make_rates(B, S, 31)
    envs = [VecLoadBalanceEnv(B, S, device="cuda:0", seed=5, autoreset=False) for _ in range(4)]
    a_env, b_env, c_env, d_env = envs
    cfg = a_env.cfg
    b_env.set_rates(np.full(B, cfg.arrival_rate, np.float32),
                    np.tile(np.array(cfg.server_rate[:S], np.float32), (B, 1)))
    c_env.set_rates(r, mu)
    c_env.clear_rates()
    d_env.set_rates(r, mu)
    obs = [e.reset() for e in envs]
    assert torch.equal(obs[0], obs[1]) and torch.equal(obs[0], obs[2])
    rng = np.random.default_rng(4)
    differs = False
    for _ in range(8):
        a = torch.from_numpy(rng.integers(0, 3, (B, S)))
        out = [e.step(a, assign_counts=True) for e in envs]
        for o in out[1:3]:
            assert torch.equal(out[0][0], o[0]) and torch.equal(out[0][1], o[1])
            assert torch.equal(out[0][2], o[2])
            assert torch.equal(out[0][3]["assign_counts"], o[3]["assign_counts"])
        differs |= not torch.equal(out[0][3]["assign_counts"], out[3][3]["assign_counts"])
    assert a_env.get_state() == b_env.get_state() == c_env.get_state()
    assert differs
    for e in envs:
        e.close()


@gpu
@pytest.mark.parametrize("B,S", [(200, 4), (777, 16)])
def test_shard_invariance(lib, B, S):
    """Three uneven shards, each with env_id_offset = lo and its own rows of the rate arrays,
    together equal the full handle."""
    from marllb_amd.env import VecLoadBalanceEnv
    r, mu = make_rates(B, S, 50 + S)
    rng = np.random.default_rng(B)
    cuts = np.sort(rng.choice(np.arange(1, B), 2, replace=False))
    bounds = [0, *cuts.tolist(), B]
    full = VecLoadBalanceEnv(B, S, device="cuda:0", seed=9, autoreset=False)
    full.set_rates(r, mu)
    parts = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        e = VecLoadBalanceEnv(hi - lo, S, device="cuda:0", seed=9, autoreset=False, env_id_offset=lo)
        e.set_rates(r[lo:hi], mu[lo:hi])
        parts.append(e)
    assert torch.equal(full.reset(), torch.cat([e.reset() for e in parts]))
    for _ in range(5):
        a = torch.from_numpy(rng.integers(0, 3, (B, S)))
        fo, fr, fd, fi = full.step(a, assign_counts=True)
        po = [e.step(a[lo:hi], assign_counts=True) for e, lo, hi in zip(parts, bounds[:-1], bounds[1:])]
        assert torch.equal(fo, torch.cat([x[0] for x in po]))
        assert torch.equal(fr, torch.cat([x[1] for x in po]))
        assert torch.equal(fd, torch.cat([x[2] for x in po]))
        assert torch.equal(fi["assign_counts"], torch.cat([x[3]["assign_counts"] for x in po]))
    for e in [full, *parts]:
        e.close()


@gpu
def test_graph_replay_sees_rate_updates(lib):
    """A step captured after the first set_rates reads the handle's arrays on every replay, so a
    later set_rates takes effect without a new capture: equal to an eager twin doing the same."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S = 67, 4
    r0, mu0 = make_rates(B, S, 61)
    r1, mu1 = make_rates(B, S, 62)
    eager = VecLoadBalanceEnv(B, S, device="cuda:0", seed=8)
    graph = VecLoadBalanceEnv(B, S, device="cuda:0", seed=8, graph_mode=True)
    for e in (eager, graph):
        e.set_rates(r0, mu0)
        e.reset()
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(1)
    acts = [torch.randint(0, 3, (B, S), device="cuda:0", generator=gen) for _ in range(7)]
    a_static = acts[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up step (eager, graph_mode buffers)
        graph.step(a_static)
    torch.cuda.current_stream().wait_stream(side)
    eager.step(acts[0])
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):  # the capture records the step, it does not run it
        obs, rew, done, info = graph.step(a_static)
    for k in range(1, 7):
        if k == 4:  # after three replays: new rates, no new capture
            for e in (eager, graph):
                e.set_rates(r1, mu1)
        a_static.copy_(acts[k])
        cg.replay()
        eo, er, ed, _ = eager.step(acts[k])
        assert torch.equal(obs, eo), k
        assert torch.equal(rew, er) and torch.equal(done, ed), k
    assert graph.get_state() == eager.get_state()
    eager.close()
    graph.close()


@gpu
def test_errors(lib):
    from marllb_amd import trace
    from marllb_amd.env import VecLoadBalanceEnv
    B, S = 19, 4
    r, mu = make_rates(B, S, 71)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=3, autoreset=False)
    twin = VecLoadBalanceEnv(B, S, device="cuda:0", seed=3, autoreset=False)
    # a fresh handle reports the config's rates
    a, m = env.rates
    assert a.shape == (B,) and m.shape == (B, S)
    assert (a.cpu().numpy() == np.float32(env.cfg.arrival_rate)).all()
    np.testing.assert_array_equal(m.cpu().numpy(),
                                  np.tile(np.array(env.cfg.server_rate[:S], np.float32), (B, 1)))
    with pytest.raises(ValueError, match="arrival_rate"):
        env.set_rates(r[:-1], None)
    with pytest.raises(ValueError, match="server_rates"):
        env.set_rates(None, mu.T)
    with pytest.raises(ValueError, match="server_rates"):
        env.set_rates(r, mu.reshape(-1))
    for e in (env, twin):
        e.set_rates(r, mu)
        e.reset()
    for bad in (0.0, float("nan"), 1e9):
        rb, mb = r.copy(), mu.copy()
        rb[7] = bad
        with pytest.raises(ValueError, match="1 value"):
            env.set_rates(rb, None)
        mb[5, 2] = bad
        with pytest.raises(ValueError, match="2 value"):
            env.set_rates(rb, mb)  # nothing of a rejected call is taken, its valid half neither
        with pytest.raises(ValueError, match="1 value"):
            env.set_rates(None, mb)
    a, m = env.rates
    np.testing.assert_array_equal(a.cpu().numpy(), r)
    np.testing.assert_array_equal(m.cpu().numpy(), mu)
    act = torch.from_numpy(np.random.default_rng(0).integers(0, 3, (B, S)))
    for _ in range(3):
        x, y = env.step(act, assign_counts=True), twin.step(act, assign_counts=True)
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
        assert torch.equal(x[3]["assign_counts"], y[3]["assign_counts"])
    assert env.get_state() == twin.get_state()
    env.close()
    twin.close()
    lf = VecLoadBalanceEnv(B, S, device="cuda:0", lost_fin_prob=0.2, flow_timeout=0.5)
    tr = VecLoadBalanceEnv(B, S, device="cuda:0", trace=trace.synthetic(37, 300.0, seed=7))
    for e, why in ((lf, "lost-FIN"), (tr, "TRACE")):
        with pytest.raises(lib.LbsimError, match=why) as ei:
            e.set_rates(r, None)
        assert ei.value.code == lib.ENOTSUP
        with pytest.raises(lib.LbsimError, match=why):
            e.set_rates(r, mu)
        e.set_rates(None, mu)  # server rates alone are allowed
        np.testing.assert_array_equal(e.rates[1].cpu().numpy(), mu)
        e.close()


@gpu
def test_multi_agent_forwards_rates(lib):
    from marllb_amd import VecMultiAgentLoadBalanceEnv
    B, A, k = 8, 2, 2
    r, mu = make_rates(B, A * k, 81)
    env = VecMultiAgentLoadBalanceEnv(B, A, k, device="cuda:0", seed=1)
    env.set_rates(r, mu)
    np.testing.assert_array_equal(env.rates[0].cpu().numpy(), r)
    np.testing.assert_array_equal(env.vec.rates[1].cpu().numpy(), mu)
    env.clear_rates()
    assert (env.rates[0].cpu().numpy() == np.float32(env.vec.cfg.arrival_rate)).all()
    env.close()


@gpu
def test_lost_fin_overflow_accessor(lib):
    """Handle.lost_fin_overflow(): guesses dropped at a full pending ring (lost_fin_pending = 2
    overflows at once with most FINs lost and a long wrap-up delay); zeros without lost-FIN."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S = 16, 4
    env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=2, autoreset=False, lost_fin_prob=0.9,
                            flow_timeout=30.0, lost_fin_pending=2)
    env.reset()
    a = torch.zeros((B, S), dtype=torch.int64)
    for _ in range(4):
        env.step(a)
    over = env.handle.lost_fin_overflow()
    assert over.shape == (B,) and over.dtype == np.uint32 and (over > 0).any()
    st = statelayout.parse_cfg(env.get_state(), env.cfg)
    np.testing.assert_array_equal(over, st["lf_over"])
    env.close()
    plain = VecLoadBalanceEnv(B, S, device="cuda:0", seed=2)
    assert not plain.handle.lost_fin_overflow().any()
    plain.close()


# ------------------------------------------------------------------ host (no GPU)

def test_signature_table_declares_the_exports():
    from marllb_amd import _lib
    names = ("lbsim_set_env_rates", "lbsim_clear_env_rates", "lbsim_get_env_rates")
    declared = _lib.header_functions()
    for n in names:
        assert n in _lib._SIGNATURES and n in declared
    assert len(_lib._SIGNATURES["lbsim_set_env_rates"][1]) == 4
    assert len(_lib._SIGNATURES["lbsim_clear_env_rates"][1]) == 1
    assert len(_lib._SIGNATURES["lbsim_get_env_rates"][1]) == 4


def test_sample_rates_ranges_shapes_and_seed():
    from marllb_amd import sample_rates
    B, S = 500, 6
    g = torch.Generator()
    g.manual_seed(123)
    a, m = sample_rates(B, S, rate=(50.0, 2000.0), load=(0.3, 1.2), server_skew=(1.0, 4.0),
                        generator=g)
    assert a.shape == (B,) and m.shape == (B, S)
    assert a.dtype == torch.float32 and m.dtype == torch.float32
    assert a.min() >= 50.0 and a.max() <= 2000.0
    load = a.double() / m.double().sum(dim=1)
    assert load.min() >= 0.3 * (1 - 1e-6) and load.max() <= 1.2 * (1 + 1e-6)
    ratio = m.max(dim=1).values / m.min(dim=1).values
    assert ratio.max() <= 4.0 * (1 + 1e-6) and ratio.max() > 1.5
    assert a.log().std() > 0.5  # spread over the decades, not clustered
    g.manual_seed(123)
    a2, m2 = sample_rates(B, S, rate=(50.0, 2000.0), load=(0.3, 1.2), server_skew=(1.0, 4.0),
                          generator=g)
    assert torch.equal(a, a2) and torch.equal(m, m2)
    a3, _ = sample_rates(B, S, rate=(50.0, 2000.0), generator=g)
    assert not torch.equal(a, a3)
    with pytest.raises(ValueError, match="load"):
        sample_rates(4, 2, load=(0.0, 1.0))
