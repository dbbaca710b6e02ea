"""Host references for the fused policy kernels (csrc/lbsim_fused.h, lbsim_nets.h) and the shape
cases tests/test_fused_policy_shapes.py runs them at.  No GPU here: float64 copies of the torch
modules on the CPU, a numpy Philox4x32-10 (the constants of csrc/lbsim_math.h) with the two draws
the kernels make from it, the comparison that also keeps the error record, and the cases' inputs,
built once per process on the CPU so the CPU fairness tests and the GPU tests see the same rows.

A case's inputs are made for BMAX = 129 rows; the smaller batches are its first rows, so one
float64 forward per case serves every batch size."""
import copy
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

from marllb_amd.policies import AgentQNet, GRUPolicy, QMixer

TOL = dict(rtol=1e-5, atol=1e-5)         # tests/test_fused_policy.py TOL
STOCH_TOL = dict(rtol=1e-4, atol=5e-5)   # the same file's stochastic-action comparison
TIE_GAP = 1e-4                           # greedy actions are compared where the top two Q differ by more
BATCHES = (1, 16, 129)
BMAX = 129
SAC_SEED = 0x123456789ABCDEF0
QMIX_SEED = 0x0FEDCBA987654321
STEPS = (0, 2 ** 31 + 5)
# Under SAC_SEED the draw of (row 89, action 0) at this step has its 24 high bits all zero: u1 is
# 2^-24 only because of the + 1 of u01_open0 (without it log(0) -- an infinite noise).  Found by
# scanning the steps from 0 with philox4x32_10 below; test_draws_use_the_whole_seed_and_step
# checks it.
U1_FLOOR_STEP, U1_FLOOR_AT = 5180, (89, 0)
SAC_STEPS = STEPS + (U1_FLOOR_STEP,)


# ------------------------------------------------------------------------------------ Philox
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_LO, _32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(ctr, key) -> np.ndarray:
    """Philox4x32-10 of counters (..., 4) under keys (..., 2) (broadcast), uint32 (..., 4)."""
    c = np.asarray(ctr).astype(np.uint64) & _LO
    k = np.asarray(key).astype(np.uint64) & _LO
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    x, y, z, w = (np.broadcast_to(c[..., i], shape) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape) for i in range(2))
    for _ in range(10):
        p0, p1 = _M0 * x, _M1 * z  # 32 x 32 -> 64 bits, no overflow
        x, y, z, w = (p1 >> _32) ^ y ^ k0, p1 & _LO, (p0 >> _32) ^ w ^ k1, p0 & _LO
        k0, k1 = (k0 + _W0) & _LO, (k1 + _W1) & _LO
    return np.stack([x, y, z, w], -1).astype(np.uint32)


def _draw(seed: int, step: int, B: int, A: int, stream: int) -> np.ndarray:
    """The kernels' counter (row, step, column, stream << 24) under key (seed lo, seed hi)."""
    ctr = np.zeros((B, A, 4), np.uint64)
    ctr[..., 0] = np.arange(B, dtype=np.uint64)[:, None]
    ctr[..., 1] = step & 0xFFFFFFFF
    ctr[..., 2] = np.arange(A, dtype=np.uint64)[None, :]
    ctr[..., 3] = stream << 24
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint64))


def sac_noise(seed: int, step: int, B: int, A: int) -> np.ndarray:
    """The SAC head's standard-normal draw for (row, action), float64 (B, A): Box-Muller of
    u1 in (0, 1] and u2 in [0, 1), the high 24 bits of the first two Philox words."""
    d = _draw(seed, step, B, A, 3)
    u1 = ((d[..., 0] >> 8).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = (d[..., 1] >> 8).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def qmix_draw(seed: int, step: int, B: int, A: int, n_actions: int, epsilon: float):
    """Epsilon-greedy's draw for (env, agent): explore (B, A) bool and the explored action (B, A)
    int64.  Both are exact: a 24-bit uniform against float32(epsilon), and a 32 x 32-bit product."""
    d = _draw(seed, step, B, A, 4)
    u = ((d[..., 0] >> 8).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    explore = u < np.float32(epsilon)
    action = (d[..., 1].astype(np.uint64) * np.uint64(n_actions)) >> _32
    return explore, action.astype(np.int64)


# ------------------------------------------------------------------------------------ modules
def randomize_biases(module: torch.nn.Module, seed: int) -> torch.nn.Module:
    """Every bias of module uniform in +-0.1 (the modules' initialisers zero most of them)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if "bias" in name:
                p.copy_((torch.rand(p.shape, generator=g, dtype=torch.float32) * 2 - 1) * 0.1)
    return module


def _as(module, dtype):
    return copy.deepcopy(module).cpu().to(dtype)


def _np(t) -> np.ndarray:
    return t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def sac_forward(pol: GRUPolicy, x, h, mask, dtype=torch.float64):
    """GRUPolicy.forward on the CPU in dtype on the float32 inputs, reset rows' hidden zeroed:
    mean, clamped log_std, hidden_new as float64 numpy."""
    m = _as(pol, dtype)
    h0 = h.cpu().to(dtype) * (~mask.cpu().bool()).unsqueeze(1).to(dtype)
    with torch.no_grad():
        mean, log_std, h1 = m(x.cpu().to(dtype), h0.unsqueeze(0).contiguous())
    return SimpleNamespace(mean=_np(mean), log_std=_np(log_std), hidden=_np(h1[0]))


def sac_action(pol: GRUPolicy, mean, log_std, eps=None, dtype=np.float64) -> np.ndarray:
    """tanh(mean + exp(log_std) eps) scale + bias (eps None: the deterministic action)."""
    mean, log_std = np.asarray(mean, dtype), np.asarray(log_std, dtype)
    x = mean if eps is None else mean + np.exp(log_std) * np.asarray(eps, dtype)
    return (np.tanh(x) * dtype(pol.action_scale) + dtype(pol.action_bias)).astype(np.float64)


def agents_forward(agents, obs, hid, mask, dtype=torch.float64):
    """Every AgentQNet on its column of obs (B, A, I) / hid (B, A, H): q (B, A, n), hidden (B, A, H)."""
    keep = (~mask.cpu().bool()).view(-1, 1).to(dtype)
    qs, hs = [], []
    with torch.no_grad():
        for a, net in enumerate(agents):
            q, h1 = _as(net, dtype)(obs[:, a].cpu().to(dtype),
                                    (hid[:, a].cpu().to(dtype) * keep).unsqueeze(0).contiguous())
            qs.append(_np(q))
            hs.append(_np(h1[0]))
    return SimpleNamespace(q=np.stack(qs, 1), hidden=np.stack(hs, 1))


def mixer_forward(mixer: QMixer, chosen, state, dtype=torch.float64) -> np.ndarray:
    """QMixer.forward on chosen (B, A) (any float array, cast to dtype) and state: (B, 1)."""
    with torch.no_grad():
        out = _as(mixer, dtype)(torch.as_tensor(np.asarray(chosen)).to(dtype),
                                state.cpu().to(dtype))
    return _np(out)


def greedy(q: np.ndarray):
    """argmax over the last axis (first maximum) and where it is well defined: the top two
    Q-values more than TIE_GAP apart (always, with a single action)."""
    g = q.argmax(-1)
    if q.shape[-1] == 1:
        return g, np.ones(g.shape, bool)
    top = np.sort(q, -1)
    return g, (top[..., -1] - top[..., -2]) > TIE_GAP


# ------------------------------------------------------------------------------------ comparison
def form() -> str:
    """The kernel form this process runs under (settings the library reads once per process)."""
    mt, kern = os.environ.get("LBSIM_FUSED_MT"), os.environ.get("LBSIM_QMIX_KERNEL")
    return "+".join(([f"mt{mt}"] if mt else []) + ([kern] if kern else [])) or "default"


def qmix_kernel(A: int) -> str:
    """The kernel launch_qmix_policy picks for A agents under form()."""
    kern = os.environ.get("LBSIM_QMIX_KERNEL")
    if kern == "tile" or os.environ.get("LBSIM_FUSED_MT") in ("2", "4"):
        return "qmix_policy_kernel"
    return "qmix_agent_pair_kernel" if A == 4 and kern != "wave" else "qmix_agent_wave_kernel"


def error_ratio(got, want, tol=TOL) -> float:
    """max |got - want| / (atol + rtol |want|): <= 1 is what assert_allclose accepts."""
    got, want = _np(got), _np(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    r = np.abs(got - want) / (tol["atol"] + tol["rtol"] * np.abs(want))
    return float("inf") if not np.all(np.isfinite(r)) else float(r.max())


def check(case: str, kernel: str, output: str, got, want, tol=TOL) -> float:
    """got within tol of want; with LBSIM_POLICY_ERR_LOG set, the ratio goes on record first."""
    ratio = error_ratio(got, want, tol)
    path = os.environ.get("LBSIM_POLICY_ERR_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "form": form(), "kernel": kernel, "output": output,
                                "err_over_tol": round(ratio, 4)}) + "\n")
    assert ratio <= 1.0, f"{case} [{form()}] {output}: max error {ratio:.3f} x tolerance"
    return ratio


class Fold:
    """One case's comparisons gathered over its batch sizes, steps and epsilons: check() compares
    each output once, over everything gathered, so the record has one line per (case, output)."""

    def __init__(self, case: str, kernel: str):
        self.case, self.kernel, self.items = case, kernel, {}

    def add(self, output: str, got, want, tol=TOL) -> None:
        got, want = _np(got), _np(want)
        assert got.shape == want.shape, (self.case, output, got.shape, want.shape)
        g, w, _ = self.items.setdefault(output, ([], [], tol))
        g.append(got.ravel())
        w.append(want.ravel())

    def check(self) -> None:
        for output, (g, w, tol) in self.items.items():
            check(self.case, self.kernel, output, np.concatenate(g), np.concatenate(w), tol)


# ------------------------------------------------------------------------------------ cases
# SAC: (state_dim, action_dim) and what differs from the nominal case (inputs N(0, 1), hidden
# N(0, 0.5), log_std clamped to +-0.05 so both sides of the clamp are hit).
SAC_CASES = {
    "11x1": dict(I=11, A=1),
    "22x2": dict(I=22, A=2),
    "44x4": dict(I=44, A=4),
    "16x3": dict(I=16, A=3, seed=163),  # (the name's own seed leaves 9 % on the upper clamp)
    "17x5": dict(I=17, A=5),
    "99x9": dict(I=99, A=9),
    "176x16": dict(I=176, A=16),
    "512x16": dict(I=512, A=16),
    "88x8_x10": dict(I=88, A=8, x_scale=10.0),
    "88x8_affine": dict(I=88, A=8, action_scale=4.95, action_bias=5.05, clamp=(-20.0, 2.0)),
}
NARROW_CLAMP = (-0.05, 0.05)

# QMIX: agents, servers per agent, obs, state, mixer E and he, n_actions.  obs and state are the
# widths the kernels see (MultiAgentEnv gives obs 4 k + 7 S, state 4 S + 10 for S = A k servers);
# the *_env rows are the three shapes whose MultiAgentEnv obs width differs from the listed one.
QMIX_CASES = {
    "4x1": dict(A=4, k=1, I=32, Ds=26, E=32, he=64, n=3),
    "4x2": dict(A=4, k=2, I=64, Ds=42, E=32, he=64, n=16),
    "4x3": dict(A=4, k=3, I=96, Ds=58, E=32, he=64, n=2),
    "4x8": dict(A=4, k=8, I=256, Ds=138, E=32, he=64, n=3),
    "1x4": dict(A=1, k=4, I=44, Ds=26, E=32, he=64, n=3),
    "2x4": dict(A=2, k=4, I=72, Ds=42, E=32, he=64, n=3),
    "3x2": dict(A=3, k=2, I=54, Ds=34, E=32, he=64, n=1),
    "5x1": dict(A=5, k=1, I=55, Ds=30, E=16, he=64, n=3),
    "8x2": dict(A=8, k=2, I=176, Ds=74, E=16, he=64, n=16),
    "4x4_he48": dict(A=4, k=4, I=128, Ds=74, E=16, he=48, n=3),
    # obs1 with padded columns: 100 is no multiple of 16 (the listed obs1 shapes, 32 and 96, are)
    "4x1_obs100": dict(A=4, k=1, I=100, Ds=26, E=32, he=64, n=3),
    # both input limits with the most agents the mixer takes: the wave kernel's largest LDS tile
    "10x1_max": dict(A=10, k=1, I=512, Ds=512, E=16, he=64, n=16),
    "3x2_env": dict(A=3, k=2, I=50, Ds=34, E=32, he=64, n=1),
    "5x1_env": dict(A=5, k=1, I=39, Ds=30, E=16, he=64, n=3),
    "8x2_env": dict(A=8, k=2, I=120, Ds=74, E=16, he=64, n=16),
}
TIE_CASE = "4x4_tie"
_TIE = dict(A=4, k=4, I=128, Ds=74, E=32, he=64, n=3)


def _seed_of(name: str) -> int:
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


@functools.lru_cache(maxsize=None)
def sac_case(name: str):
    """The case's module (float32, CPU, biases randomised), its BMAX input rows and the float64
    reference of them."""
    kw = SAC_CASES[name]
    lo, hi = kw.get("clamp", NARROW_CLAMP)
    seed = kw.get("seed", _seed_of(name))
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        pol = GRUPolicy(kw["I"], kw["A"], 256, 128, action_scale=kw.get("action_scale", 1.0),
                        action_bias=kw.get("action_bias", 0.0), log_std_min=lo, log_std_max=hi)
    randomize_biases(pol, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    x = torch.randn(BMAX, kw["I"], generator=g) * kw.get("x_scale", 1.0)
    h = torch.randn(BMAX, 128, generator=g) * 0.5
    mask = torch.zeros(BMAX, dtype=torch.bool)
    mask[::5] = True
    return SimpleNamespace(name=name, pol=pol, x=x, h=h, mask=mask, A=kw["A"],
                           ref=sac_forward(pol, x, h, mask))


@functools.lru_cache(maxsize=None)
def qmix_case(name: str):
    """The case's agents (own weights each) and mixer (float32, CPU, biases randomised), its BMAX
    input rows and the float64 Q-values and hidden states of them."""
    kw = _TIE if name == TIE_CASE else QMIX_CASES[name]
    seed = _seed_of(name)
    agents = []
    with torch.random.fork_rng():
        for a in range(kw["A"]):
            torch.manual_seed(seed + 10 * a)
            agents.append(randomize_biases(AgentQNet(kw["I"], kw["n"], 128, 64), seed + 10 * a + 1))
        torch.manual_seed(seed + 7)
        mixer = randomize_biases(QMixer(kw["A"], kw["Ds"], kw["E"], kw["he"]), seed + 8)
    if name == TIE_CASE:  # actions 1 and 2 tie exactly and beat action 0: greedy must say 1
        with torch.no_grad():
            for net in agents:
                net.fc3.weight[2] = net.fc3.weight[1]
                net.fc3.bias[2] = net.fc3.bias[1]
                net.fc3.bias[1:3] += 10.0
    g = torch.Generator().manual_seed(seed + 9)
    obs = torch.randn(BMAX, kw["A"], kw["I"], generator=g)
    hid = torch.randn(BMAX, kw["A"], 64, generator=g) * 0.5
    state = torch.randn(BMAX, kw["Ds"], generator=g)
    mask = torch.zeros(BMAX, dtype=torch.bool)
    mask[::7] = True
    return SimpleNamespace(name=name, agents=agents, mixer=mixer, obs=obs, hid=hid, state=state,
                           mask=mask, ref=agents_forward(agents, obs, hid, mask), **kw)


def qmix_expected_actions(c, B: int, epsilon: float, step: int):
    """The actions the reference decides for the case's first B rows: (action, decided) with
    decided False where greedy is a near tie (any action may come out there)."""
    g, clear = greedy(c.ref.q[:B])
    explore, ea = qmix_draw(QMIX_SEED, step, B, c.A, c.n, epsilon)
    return np.where(explore, ea, g), explore | clear
