"""Policy-in-the-loop rollouts on the GPU (marllb_amd/rollout.py; BASELINE configs[3], [4])."""
import pytest

torch = pytest.importorskip("torch")
from tests.parity import need_gpu  # noqa: E402, F401  (the autouse device guard)

pytestmark = pytest.mark.gpu


def test_sac_gru_rollout_deterministic_and_hidden_reset():
    from marllb_amd import VecLoadBalanceEnv
    from marllb_amd.policies import GRUPolicy
    from marllb_amd.rollout import SACGRURollout
    torch.manual_seed(0)
    pol = GRUPolicy(88, 8, 256, 128)
    runs = []
    for _ in range(2):
        env = VecLoadBalanceEnv(128, 8, device="cuda:0", seed=4, action_type="continuous",
                                max_steps=3, autoreset=True)
        ro = SACGRURollout(env, pol, seed=1)
        rs = [ro.step()[0].clone() for _ in range(3)]
        runs.append(rs)
        assert torch.all(ro.hidden == 0)  # every env finished at step 3: GRU state re-initialised
        env.close()
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_qmix_rollout_shapes():
    from marllb_amd.multi_agent import VecMultiAgentLoadBalanceEnv
    from marllb_amd.rollout import QMIXRollout
    torch.manual_seed(0)
    env = VecMultiAgentLoadBalanceEnv(64, 4, 4, device="cuda:0", seed=2, action_type="discrete")
    ro = QMIXRollout(env, seed=3)
    q_tot, rew, done, _ = ro.step()
    assert q_tot.shape == (64, 1) and torch.isfinite(q_tot).all()
    assert rew.shape == (64, 4) and done.shape == (64,)
    env.close()


def test_qmix_rollout_kernel_matches_gemm_form_greedy():
    """epsilon = 0: the one-kernel policy (lbsim_qmix_policy_step) and the GEMM form drive the
    multi-agent env through the same greedy actions, hence identical rewards, and Q_tot agrees."""
    from marllb_amd.multi_agent import VecMultiAgentLoadBalanceEnv
    from marllb_amd.rollout import QMIXRollout
    runs = []
    for fused_kernel in (True, False):
        torch.manual_seed(0)
        env = VecMultiAgentLoadBalanceEnv(256, 4, 4, device="cuda:0", seed=5,
                                          action_type="discrete", max_steps=2)
        ro = QMIXRollout(env, epsilon=0.0, seed=3)
        if not fused_kernel:  # force the GEMM + epilogue form on the same weights
            from marllb_amd.policies import FusedAgentQNets, FusedQMixer
            ro.kernel = None
            ro.fused = (FusedAgentQNets(ro.agents), FusedQMixer(ro.mixer))
            ro.hidden = torch.zeros(4, 256, ro.agents[0].gru_dim, device="cuda:0")
        else:
            assert ro.kernel is not None
        runs.append([tuple(t.clone() for t in ro.step()[:3]) for _ in range(4)])  # crosses a reset
        env.close()
    for (qk, rk, dk), (qg, rg, dg) in zip(*runs):
        assert torch.equal(rk, rg) and torch.equal(dk, dg)
        torch.testing.assert_close(qk, qg, rtol=1e-5, atol=1e-5)


def test_env_step_graph_capture_replays_bit_exact():
    """One VecLoadBalanceEnv.step (dynamics + observe launches + the every-step masked auto-reset
    of graph_mode) captured into a torch.cuda.CUDAGraph and replayed over two auto-reset boundaries
    equals eager stepping of an identical env, bit for bit."""
    from marllb_amd import VecLoadBalanceEnv
    B, S, T = 1024, 4, 4
    eager = VecLoadBalanceEnv(B, S, device="cuda:0", seed=8, max_steps=T)
    graph = VecLoadBalanceEnv(B, S, device="cuda:0", seed=8, max_steps=T, graph_mode=True)
    eager.reset()
    graph.reset()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    acts = [torch.randint(0, 3, (B, S), device="cuda:0", generator=g) for _ in range(3 * T)]
    a_static = acts[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up step (eager, graph_mode buffers)
        o, r, d, _ = graph.step(a_static)
    torch.cuda.current_stream().wait_stream(side)
    e = eager.step(acts[0])
    assert torch.equal(o, e[0]) and torch.equal(r, e[1]) and torch.equal(d, e[2])
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        obs, rew, done, info = graph.step(a_static)
    for k in range(1, 3 * T):
        a_static.copy_(acts[k])
        cg.replay()
        eo, er, ed, ei = eager.step(acts[k])
        assert torch.equal(obs, eo), k
        assert torch.equal(rew, er), k
        assert torch.equal(done, ed), k
        assert torch.equal(info["episode_return"], ei["episode_return"]), k
    eager.close()
    graph.close()


@pytest.mark.parametrize("B", [1024, 8256])
def test_env_step_graph_next_step_autoreset(oracle_mod, B):
    """autoreset_mode="next_step" (gymnasium NEXT_STEP): the captured step holds only the step's
    own launches (no masked-reset kernel: the reset of an env done last step runs inside them),
    and replays over three episode boundaries equal the oracle with next_step_reset, bit for bit
    (obs, reward, done, episode length / return); the step after done reports the reset obs,
    reward 0 and done False.  B = 1024: the one-launch wave step; 8256: group dynamics + observe."""
    import numpy as np
    from marllb_amd import VecLoadBalanceEnv
    from marllb_amd.env import make_config
    S, T = 4, 3
    graph = VecLoadBalanceEnv(B, S, device="cuda:0", seed=12, max_steps=T, graph_mode=True,
                              autoreset_mode="next_step")
    ora = oracle_mod.OracleEnv(make_config(B, S, seed=12, max_steps=T, next_step_reset=True),
                               threads=8)
    np.testing.assert_array_equal(graph.reset().cpu().numpy(), ora.reset())
    g = torch.Generator(device="cuda:0")
    g.manual_seed(3)
    acts = [torch.randint(0, 3, (B, S), device="cuda:0", generator=g) for _ in range(4 * (T + 1))]
    a_static = acts[0].clone()

    class Spy:  # counts the facade's reset calls (graph_mode same-step would make one per step)
        def __init__(self, lib):
            self._lib, self.resets = lib, 0

        def __getattr__(self, name):
            f = getattr(self._lib, name)
            if name != "lbsim_reset_ex":
                return f

            def counted(*a):
                self.resets += 1
                return f(*a)
            return counted
    spy = graph.handle.lib = Spy(graph.handle.lib)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up step (eager, graph_mode buffers)
        o, r, d, _ = graph.step(a_static)
    torch.cuda.current_stream().wait_stream(side)
    oo, ro, do, _ = ora.step(acts[0].cpu().numpy())
    assert np.array_equal(o.cpu().numpy(), oo) and np.array_equal(r.cpu().numpy(), ro)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        obs, rew, done, info = graph.step(a_static)
    assert spy.resets == 0  # the captured step holds no masked-reset launch
    for k in range(1, len(acts)):
        a_static.copy_(acts[k])
        cg.replay()
        oo, ro, do, _ = ora.step(acts[k].cpu().numpy())
        ln, rt = ora.episode_stats()
        np.testing.assert_array_equal(obs.cpu().numpy(), oo, err_msg=f"step {k}")
        np.testing.assert_array_equal(rew.cpu().numpy(), ro, err_msg=f"step {k}")
        np.testing.assert_array_equal(done.cpu().numpy().astype(np.uint8), do, err_msg=f"step {k}")
        np.testing.assert_array_equal(info["episode_length"].cpu().numpy(), ln)
        np.testing.assert_array_equal(info["episode_return"].cpu().numpy(), rt)
        if k % (T + 1) == T:  # the step after the episode end: the reset, reward 0
            assert not do.any() and (ro == 0).all() and (ln == 0).all()
    ora.close()
    graph.close()


def test_qmix_rollout_graph_capture_replays_bit_exact():
    """One QMIXRollout.step -- the fused QMIX policy kernel (Philox step counter on the device),
    the fused env step writing the agent observations and the state, the auto-reset -- captured
    and replayed equals the eager rollout (same weights and seeds) bit for bit, across episode
    ends (max_steps 3), epsilon-greedy draws included."""
    from marllb_amd.multi_agent import VecMultiAgentLoadBalanceEnv
    from marllb_amd.rollout import QMIXRollout
    B, T = 512, 3
    outs = []
    for graph_mode in (False, True):
        torch.manual_seed(0)
        env = VecMultiAgentLoadBalanceEnv(B, 4, 4, device="cuda:0", seed=12,
                                          action_type="discrete", max_steps=T,
                                          graph_mode=graph_mode)
        ro = QMIXRollout(env, epsilon=0.3, seed=7)
        seq = []
        if graph_mode:
            cg = ro.capture(warmup=2)  # two eager warm-up steps, then the captured one
            for _ in range(3 * T):
                cg.replay()
                q_tot, rew, done, _ = ro.last
                seq.append((q_tot.clone(), rew.clone(), done.clone(), ro.obs.clone()))
        else:
            for _ in range(2 + 3 * T):
                q_tot, rew, done, _ = ro.step()
                seq.append((q_tot.clone(), rew.clone(), done.clone(), ro.obs.clone()))
            seq = seq[2:]  # align with the graph run's two warm-up steps
        outs.append(seq)
        env.close()
    for k, (a, b) in enumerate(zip(*outs)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), k


@pytest.mark.parametrize("per_graph", [1, 3])
def test_sac_rollout_graph_capture_replays_bit_exact(per_graph):
    """SACGRURollout.step -- the one-launch SAC-GRU actor (Philox step counter on the device,
    hidden state updated in place, finished envs restarted from h = 0) and the env step -- captured
    (one or three steps per graph) and replayed equals the eager rollout bit for bit across
    episode ends (max_steps 3)."""
    from marllb_amd import VecLoadBalanceEnv
    from marllb_amd.rollout import SACGRURollout
    B, S, T = 512, 8, 3
    outs = []
    for graph_mode in (False, True):
        torch.manual_seed(0)
        env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=5, action_type="continuous",
                                max_steps=T, graph_mode=graph_mode)
        ro = SACGRURollout(env, seed=3)
        seq = []
        if graph_mode:
            cg = ro.capture(warmup=2, steps=per_graph)
            for _ in range(3 * T // per_graph):
                cg.replay()  # per_graph steps; the outputs are the last one's
                rew, done, _ = ro.last
                seq.append((rew.clone(), done.clone(), ro.obs.clone(), ro._h.clone()))
        else:
            for _ in range(2 + 3 * T):
                rew, done, _ = ro.step()
                seq.append((rew.clone(), done.clone(), ro.obs.clone(), ro._h.clone()))
            seq = seq[2:][per_graph - 1::per_graph]
        outs.append(seq)
        env.close()
    for k, (a, b) in enumerate(zip(*outs)):
        for x, y in zip(a, b):
            assert torch.equal(x, y), k
