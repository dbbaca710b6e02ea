"""observe_pair_kernel with its episode words requested beside the decision words and the reward,
episode bookkeeping and output rows of all envs of a wave done at once (lane e = env e;
csrc/lbsim_kernels.h observe_pair_outputs): every step's obs / reward / done / episode_length /
episode_return and the whole state against the oracle, bit for bit, at the smallest shapes where
that code can go wrong.  Every case steps in two launches (step_kernel="split": these batches
would otherwise take the one-launch step_wave_kernel) and asserts the observe kernel by name.
"""
import numpy as np
import pytest

from tests import parity, statelayout
from tests.parity import lib, need_gpu  # noqa: F401  (fixtures: the library, the device guard)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _pair_kernel_ran(lib, env, facade=False):
    names = lib.launch_names(env.handle)
    want = "observe_pair_kernel<0, " + ("true" if facade else "false")
    assert names.get(1, "").startswith(want), names


def _step(env, ref, a, k, same_step=False, raw_ref=None):
    """Step k of env and oracle on the same actions: obs, reward, done, assign counts, episode
    length and return are equal.  same_step: the env's masked auto-reset launch follows the step,
    the oracle resets the done envs the same way.  raw_ref: an oracle of the same config without
    normalisation, whose rows are the step's raw_obs."""
    og, rg, dg, info = env.step(torch.from_numpy(a), assign_counts=True, raw_obs=raw_ref is not None)
    oo, ro, do, ao = ref.step(a)
    ln, rt = ref.episode_stats()
    if same_step and do.any():
        oo = ref.reset(mask=do, obs=oo)
    np.testing.assert_array_equal(info["assign_counts"].cpu().numpy(), ao, err_msg=f"assign step {k}")
    np.testing.assert_array_equal(og.cpu().numpy(), oo, err_msg=f"obs step {k}")
    np.testing.assert_array_equal(rg.cpu().numpy(), ro, err_msg=f"reward step {k}")
    np.testing.assert_array_equal(dg.cpu().numpy().astype(np.uint8), do, err_msg=f"done step {k}")
    np.testing.assert_array_equal(info["episode_length"].cpu().numpy(), ln, err_msg=f"ep_len step {k}")
    np.testing.assert_array_equal(info["episode_return"].cpu().numpy(), rt, err_msg=f"ep_ret step {k}")
    if raw_ref is not None:
        raw = raw_ref.step(a)[0]
        if same_step and do.any():
            raw = raw_ref.reset(mask=do, obs=raw)
        np.testing.assert_array_equal(info["raw_obs"].cpu().numpy(), raw, err_msg=f"raw_obs step {k}")
    return do


def _run(lib, oracle_mod, B, S, kw, steps=12, reset_at=6, same_step=False, raw=False,
         after_step=None, **env_kw):
    """Reset, `steps` steps with a masked reset of every other env before step reset_at (the envs
    of one wave are then at different episode steps), the whole state at the end."""
    from marllb_amd.env import VecLoadBalanceEnv, make_config
    kw = dict(kw)
    kw.setdefault("seed", 4000 + 16 * B + S)
    env_kw.setdefault("autoreset", False)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", step_kernel="split", **env_kw, **kw)
    ckw = dict(kw, next_step_reset=True) if env.next_step else kw
    ref = oracle_mod.OracleEnv(make_config(B, S, **ckw), threads=2)
    raw_ref = None
    if raw:
        raw_ref = oracle_mod.OracleEnv(make_config(B, S, **dict(ckw, normalize_obs=False)), threads=2)
        raw_ref.reset()
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    rng = np.random.default_rng(B * 31 + S)
    mask = (np.arange(B) % 2 == 0).astype(np.uint8)
    for k in range(steps):
        if k == reset_at:
            og = env.reset(mask=torch.from_numpy(mask)).cpu().numpy()
            np.testing.assert_array_equal(og, ref.reset(mask=mask, obs=og.copy()))
            if raw_ref is not None:
                raw_ref.reset(mask=mask)
        _step(env, ref, parity.actions(rng, B, S, kw), k, same_step, raw_ref)
        if after_step is not None:
            after_step(ref)
    _pair_kernel_ran(lib, env)
    parity.compare_state(env.handle, ref, env.cfg)
    env.close()
    ref.close()
    if raw_ref is not None:
        raw_ref.close()


@pytest.mark.parametrize("S,B", [(1, 1), (1, 7), (1, 9), (2, 5), (3, 3), (4, 1), (4, 3), (5, 2),
                                 (8, 2)])
def test_envs_per_wave_and_ragged_waves(lib, oracle_mod, S, B):
    """Envs per wave and ragged last waves: S = 1 with 1, 7 and 9 envs (8 envs per wave: one lane,
    seven lanes, a full wave and a wave of one), S = 2 with 5 (4 per wave, then 1), S = 3 with 3
    (2 envs = 6 rows per wave, two idle 8-lane groups, then 1 env), S = 4 with 1 and 3 (2 per
    wave), S = 5 and 8 with 2 (one env per wave; the reward takes the general metric code).  A
    masked reset of every other env after 6 of the 12 steps puts envs at different episode steps
    into one wave."""
    _run(lib, oracle_mod, B, S, {})


@pytest.mark.parametrize("S,B", [(1, 9), (2, 5), (4, 5)])
def test_next_step_reset_fresh_beside_running(lib, oracle_mod, S, B):
    """autoreset_mode="next_step" with max_steps = 3: the dynamics launch resets the envs that were
    done and leaves ep_step = -1, which the observe launch reads with its decision words: reward
    0, episode step 0, not done.  The masked reset before step 2 staggers the envs, so fresh envs
    sit beside running ones in one wave; 12 steps are four episodes."""
    _run(lib, oracle_mod, B, S, {"max_steps": 3}, reset_at=2, autoreset=True,
         autoreset_mode="next_step")


@pytest.mark.parametrize("S,B", [(1, 9), (4, 5)])
def test_same_step_reset_lengths_and_returns(lib, oracle_mod, S, B):
    """autoreset_mode="same_step" with max_steps = 3: done, the masked reset launch after the step,
    episode lengths and returns over four episodes, the envs of a wave staggered by the masked
    reset before step 2."""
    _run(lib, oracle_mod, B, S, {"max_steps": 3}, reset_at=2, same_step=True, autoreset=True)


def test_unchanged_and_mixed_waves(lib, oracle_mod):
    """Sparse arrivals (0.5 per env-step, the reservoirs filled by a long warm-up): whole waves
    whose 8 rows all kept their reservoirs (the cached features, column 0 from the hc word) next
    to waves with some rows changed and some not.  Both kinds are counted from the oracle's chg
    words after every step (88 unchanged and 168 mixed wave-steps of 256 on the oracle, every
    reservoir holding 12 to 32 samples: the mixed waves take the register path)."""
    from marllb_amd.env import make_config
    B, S = 32, 4
    kw = {"arrival_rate": 2.0, "server_rates": [1.0, 1.0, 1.5, 2.0], "warmup_steps": 160,
          "seed": 99}
    cfg = make_config(B, S, **kw)
    seen = np.zeros(3, np.int64)  # waves: unchanged / mixed / every row changed

    def count(ref):
        st = statelayout.parse_cfg(ref.state_bytes(), cfg)
        rows = np.unpackbits(st["chg"].view(np.uint8)).reshape(B * S, 128).any(1).reshape(-1, 8)
        seen[:] += [(~rows.any(1)).sum(), (rows.any(1) & ~rows.all(1)).sum(), rows.all(1).sum()]

    _run(lib, oracle_mod, B, S, kw, steps=16, reset_at=8, after_step=count)
    print("waves unchanged / mixed / all rows changed:", seen)
    assert seen[0] >= 10 and seen[1] >= 10, seen


def test_normalize_obs(lib, oracle_mod):
    """normalize_obs=True: the float64 running statistics per env (the per-env tail of the
    outputs), two envs per wave and a last wave of one."""
    _run(lib, oracle_mod, 5, 4, {"normalize_obs": True})


@pytest.mark.parametrize("S,B", [(2, 5), (4, 3)])
def test_raw_obs(lib, oracle_mod, S, B):
    """raw_obs=True beside normalised rows: the raw rows equal an un-normalised oracle's, the
    returned rows the normalised one's."""
    _run(lib, oracle_mod, B, S, {"normalize_obs": True}, raw=True)


@pytest.mark.parametrize("metric", ["variance", "gini"])
def test_reward_metric(lib, oracle_mod, metric):
    """A non-default reward metric at S = 4 (jain takes the straight-line code there, every other
    metric the general one), each lane with its own count of active servers."""
    _run(lib, oracle_mod, 5, 4, {"reward_metric": metric})


@pytest.mark.parametrize("A,k,B", [(2, 2, 5), (4, 2, 3)])
def test_multi_agent_facade(lib, oracle_mod, A, k, B):
    """The problem-05 facade instantiation (FAC): 2 agents x 2 servers (two envs per wave) and
    4 x 2 (one): the underlying rows, rewards, done and episode words against the oracle across
    same-step auto-resets (max_steps = 4), the agent observations against lbsim_agent_obs on the
    returned rows and the state against zeros ++ [step / max_steps, A]."""
    from marllb_amd import VecMultiAgentLoadBalanceEnv
    from marllb_amd.env import make_config
    S, T = A * k, 4
    kw = {"seed": 4100 + S, "action_type": "discrete", "max_steps": T}
    env = VecMultiAgentLoadBalanceEnv(B, A, k, device="cuda:0", step_kernel="split", **kw)
    ref = oracle_mod.OracleEnv(make_config(B, S, **kw), threads=2)
    env.reset()
    np.testing.assert_array_equal(env.vec._last_obs.cpu().numpy(), ref.reset())
    rng = np.random.default_rng(S)
    ep = np.zeros(B, np.int32)
    mask = (np.arange(B) % 2 == 0).astype(np.uint8)
    for t in range(10):
        if t == 2:
            env.reset(mask=torch.from_numpy(mask))
            og = env.vec._last_obs.cpu().numpy()
            np.testing.assert_array_equal(og, ref.reset(mask=mask, obs=og.copy()))
            ep[mask != 0] = 0
        a = parity.actions(rng, B, S, kw)
        ao, rew, done, info = env.step(torch.from_numpy(a))
        oo, ro, do, _ = ref.step(a)
        ln, rt = ref.episode_stats()
        if do.any():
            oo = ref.reset(mask=do, obs=oo)
        obs = env.vec._last_obs
        np.testing.assert_array_equal(obs.cpu().numpy(), oo, err_msg=f"obs step {t}")
        np.testing.assert_array_equal(rew[:, 0].cpu().numpy(), ro, err_msg=f"reward step {t}")
        np.testing.assert_array_equal(done.cpu().numpy().astype(np.uint8), do, err_msg=f"done step {t}")
        np.testing.assert_array_equal(info["episode_length"].cpu().numpy(), ln)
        np.testing.assert_array_equal(info["episode_return"].cpu().numpy(), rt)
        assert torch.equal(ao, env.agent_obs(obs)), t
        ep = np.where(do != 0, 0, ln).astype(np.int32)
        want = np.zeros((B, 4 * S + 10), np.float32)
        want[:, -2] = ep.astype(np.float32) / np.float32(T)
        want[:, -1] = float(A)
        np.testing.assert_array_equal(env.get_state().cpu().numpy(), want, err_msg=f"state step {t}")
    _pair_kernel_ran(lib, env.vec, facade=True)
    parity.compare_state(env.vec.handle, ref, env.vec.cfg)
    env.close()
    ref.close()
