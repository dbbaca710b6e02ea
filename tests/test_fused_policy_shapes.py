"""The fused policy kernels (csrc/lbsim_fused.h: sac_actor_kernel, qmix_policy_kernel,
qmix_agent_wave_kernel, qmix_agent_pair_kernel) and the GEMM form's epilogues (lbsim_nets.h) at the
shapes their launchers accept, against float64 evaluations on the host (tests/policy_ref.py):
float64 copies of the torch modules for the numbers, a numpy Philox for the noise and the
exploration.  Tolerance: the project's 1e-5 (abs + rel), 1e-4 / 5e-5 for stochastic actions;
explored actions and server actions exact, greedy actions exact where the reference's top two
Q-values are more than 1e-4 apart.

CPU part: the conditions that make those comparisons fair (the float32 module itself within a
quarter of the tolerance, both log_std clamps hit, few near ties, the explore share).  The GPU
cases are named *_shape_case: test_other_kernel_forms runs exactly those in child processes."""
import copy
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from marllb_amd import _lib  # noqa: E402
from marllb_amd.policies import FusedGRUPolicy, FusedQMIXPolicy, pack_linear  # noqa: E402
from tests import policy_ref as ref  # noqa: E402

DEV = "cuda:0"
SAC = list(ref.SAC_CASES)
QMIX = list(ref.QMIX_CASES)


# ------------------------------------------------------------------------------------ CPU: Philox
def test_numpy_philox_matches_the_oracle(oracle_mod):
    rng = np.random.default_rng(20)
    ctr = rng.integers(0, 2 ** 32, (300, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 2 ** 32, (300, 2), dtype=np.uint64).astype(np.uint32)
    ctr[:4] = [[0] * 4, [0xFFFFFFFF] * 4, [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [1, 0, 0, 0]]
    key[:4] = [[0, 0], [0xFFFFFFFF] * 2, [0xA4093822, 0x299F31D0], [0, 1]]
    got = ref.philox4x32_10(ctr, key)
    for i in range(len(ctr)):
        np.testing.assert_array_equal(got[i], oracle_mod.philox(ctr[i], key[i]), err_msg=str(i))
    # the Random123 known-answer vectors themselves
    np.testing.assert_array_equal(got[0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8])
    np.testing.assert_array_equal(got[1], [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD])
    np.testing.assert_array_equal(got[2], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1])


def test_draws_use_the_whole_seed_and_step():
    """sac_noise / qmix_draw against a scalar evaluation through the oracle's Philox: the counter
    (row, step, column, stream << 24), the key (seed lo, seed hi), u1 in (0, 1]."""
    import oracle
    seed, step = ref.SAC_SEED, 2 ** 31 + 5
    eps = ref.sac_noise(seed, step, 3, 2)
    ex, ea = ref.qmix_draw(seed, step, 3, 2, 5, 0.3)
    for b in range(3):
        for a in range(2):
            key = [seed & 0xFFFFFFFF, seed >> 32]
            d = oracle.philox([b, step, a, 3 << 24], key)
            u1, u2 = ((int(d[0]) >> 8) + 1) / 2 ** 24, (int(d[1]) >> 8) / 2 ** 24
            assert eps[b, a] == pytest.approx(np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2),
                                              rel=1e-12, abs=1e-12)
            d = oracle.philox([b, step, a, 4 << 24], key)
            assert bool(ex[b, a]) == (np.float32((int(d[0]) >> 8) / 2 ** 24) < np.float32(0.3))
            assert int(ea[b, a]) == (int(d[1]) * 5) >> 32
    assert not np.array_equal(eps, ref.sac_noise(seed & 0xFFFFFFFF, step, 3, 2))  # key1 matters
    assert not np.array_equal(eps, ref.sac_noise(seed, 5, 3, 2))                  # step bit 31 too
    assert np.all(np.isfinite(ref.sac_noise(seed, 0, 129, 16)))
    b, a = ref.U1_FLOOR_AT  # u1 = 2^-24 exactly: the smallest value, |eps| = sqrt(48 ln 2) |cos|
    assert int(ref._draw(seed, ref.U1_FLOOR_STEP, 129, 1, 3)[b, a, 0]) >> 8 == 0
    e = ref.sac_noise(seed, ref.U1_FLOOR_STEP, 129, 16)
    assert np.all(np.isfinite(e)) and 1.0 < abs(e[b, a]) < np.sqrt(48 * np.log(2))


# ------------------------------------------------------------------------------------ CPU: fairness
@pytest.mark.parametrize("name", SAC)
def test_sac_case_is_fair(name):
    """The float32 module on the CPU is within a quarter of the tolerance of the float64 one on
    every output the GPU test compares, and (narrow-clamp cases) the reference log_std sits on each
    side of the clamp for at least 10 % of its entries.  88x8_affine keeps the default [-20, 2]."""
    c = ref.sac_case(name)
    f32 = ref.sac_forward(c.pol, c.x, c.h, c.mask, torch.float32)
    r = c.ref
    assert ref.error_ratio(f32.hidden, r.hidden) <= 0.25
    assert ref.error_ratio(f32.log_std, r.log_std) <= 0.25
    assert ref.error_ratio(ref.sac_action(c.pol, f32.mean, f32.log_std, dtype=np.float32),
                           ref.sac_action(c.pol, r.mean, r.log_std)) <= 0.25
    for step in ref.SAC_STEPS:
        eps = ref.sac_noise(ref.SAC_SEED, step, ref.BMAX, c.A)
        assert ref.error_ratio(ref.sac_action(c.pol, f32.mean, f32.log_std, eps, np.float32),
                               ref.sac_action(c.pol, r.mean, r.log_std, eps),
                               ref.STOCH_TOL) <= 0.25
    if "clamp" not in ref.SAC_CASES[name]:
        lo, hi = ref.NARROW_CLAMP
        assert np.mean(r.log_std == lo) >= 0.10 and np.mean(r.log_std == hi) >= 0.10
    else:
        assert (c.pol.log_std_min, c.pol.log_std_max) == (-20.0, 2.0)


def test_sac_x10_case_saturates_gates():
    h = ref.sac_case("88x8_x10").ref.hidden
    assert np.mean(np.abs(h) > 0.999) > 0.02


@pytest.mark.parametrize("name", QMIX + [ref.TIE_CASE])
def test_qmix_case_is_fair(name):
    """float32 agents and mixer within a quarter of the tolerance of the float64 ones; at most
    1 % of the (env, agent) pairs are near ties; at epsilon 0.3 the reference explores on 20-40 %
    of them; every agent has weights of its own."""
    c = ref.qmix_case(name)
    f32 = ref.agents_forward(c.agents, c.obs, c.hid, c.mask, torch.float32)
    assert ref.error_ratio(f32.q, c.ref.q) <= 0.25
    assert ref.error_ratio(f32.hidden, c.ref.hidden) <= 0.25
    g, clear = ref.greedy(c.ref.q)
    if name != ref.TIE_CASE:
        assert np.mean(~clear) <= 0.01
    else:
        assert not clear.any() and np.all(c.ref.q[..., 1] == c.ref.q[..., 2])
        assert np.all(c.ref.q[..., 1] - c.ref.q[..., 0] > 1.0) and np.all(g == 1)
    for eps, step in zip((0.0, 0.3), ref.STEPS):
        act, _ = ref.qmix_expected_actions(c, ref.BMAX, eps, step)
        chosen = np.take_along_axis(c.ref.q, act[..., None], 2)[..., 0]
        assert ref.error_ratio(ref.mixer_forward(c.mixer, chosen.astype(np.float32), c.state,
                                                 torch.float32),
                               ref.mixer_forward(c.mixer, chosen.astype(np.float32), c.state)) <= 0.25
    explore, _ = ref.qmix_draw(ref.QMIX_SEED, ref.STEPS[1], ref.BMAX, c.A, c.n, 0.3)
    assert 0.20 <= explore.mean() <= 0.40
    assert not ref.qmix_draw(ref.QMIX_SEED, ref.STEPS[0], ref.BMAX, c.A, c.n, 0.0)[0].any()
    for a, b in zip(c.agents, c.agents[1:]):
        assert not torch.equal(a.fc1.weight, b.fc1.weight) and not torch.equal(a.fc3.bias, b.fc3.bias)


def test_case_tables_are_the_issue_s():
    """The shapes reach the paths they are there for (the launchers' arithmetic, on the host)."""
    r16 = lambda v: -(-v // 16) * 16  # noqa: E731
    assert [r16(ref.SAC_CASES[k]["I"]) // 16 for k in ("11x1", "22x2", "44x4", "16x3", "17x5")] \
        == [1, 2, 3, 1, 2]
    assert [(2 * ref.SAC_CASES[k]["A"] + 15) // 16 for k in ("44x4", "99x9", "176x16")] == [1, 2, 2]
    q = ref.QMIX_CASES
    for k in ("4x1", "4x3"):  # obs1: at most 128 padded columns, not whole 64-column blocks
        assert r16(q[k]["I"]) <= 128 and q[k]["I"] % 64 != 0
    assert q["4x2"]["I"] == 64 and q["4x4_he48"]["I"] == 128     # obs_async, nq = 1 and 2
    assert r16(q["4x8"]["I"]) > 128 and 16 * r16(q["4x8"]["Ds"]) > 3 * 512  # obs loop; stage_rows
    for k, c in q.items():
        assert c["A"] * c["E"] + c["E"] + 16 <= 3 * c["he"] and 3 * c["he"] + c["E"] <= 256
        if k in ("4x1_obs100", "10x1_max"):  # widths chosen for the kernels, not an env's
            continue
        assert c["Ds"] == 4 * c["A"] * c["k"] + 10
        if k not in ("3x2", "5x1", "8x2"):  # (their MultiAgentEnv widths are the *_env rows)
            assert c["I"] == 4 * c["k"] + 7 * c["A"] * c["k"]


def test_supported_agrees_with_the_launcher():
    """FusedQMIXPolicy.widths_supported says yes exactly where lbsim_qmix_policy_step's own checks
    do (B = 0: the checks run, nothing launches), across each limit and one step past it."""
    lib = _lib.load()

    def launcher(A, I, Ds, n, E, he, gru=64, hid=128):
        net = _lib.QmixPolicy(A, I, gru, hid, n, Ds, E, he, 1, 0.05)
        rc = lib.lbsim_qmix_policy_step(ctypes.byref(net), None, None, None, None, 0, 0, 0, None,
                                        None, None, None, None, None)
        assert rc in (_lib.OK, _lib.EINVAL, _lib.ENOTSUP)
        return rc == _lib.OK

    ok = FusedQMIXPolicy.widths_supported
    seen = set()
    for E in (0, 8, 16, 32, 48, 64):
        for he in (0, 8, 16, 48, 64, 80, 96):
            for A in (0, 1, 2, 3, 4, 5, 8, 10, 11, 16, 17):
                assert ok(A, 72, 42, 3, E, he) == launcher(A, 72, 42, 3, E, he), (A, E, he)
                seen.add(ok(A, 72, 42, 3, E, he))
    assert seen == {True, False}
    for v in (0, 1, 512, 513):
        assert ok(2, v, 42, 3, 32, 64) == launcher(2, v, 42, 3, 32, 64) == (1 <= v <= 512)
        assert ok(2, 72, v, 3, 32, 64) == launcher(2, 72, v, 3, 32, 64) == (1 <= v <= 512)
    for n in (0, 1, 16, 17):
        assert ok(2, 72, 42, n, 32, 64) == launcher(2, 72, 42, n, 32, 64) == (1 <= n <= 16)
    assert not ok(2, 72, 42, 3, 32, 64, 32, 128) and not launcher(2, 72, 42, 3, 32, 64, 32, 128)
    assert not ok(2, 72, 42, 3, 32, 64, 64, 96) and not launcher(2, 72, 42, 3, 32, 64, 64, 96)
    for kw in ref.QMIX_CASES.values():  # and every case of this file is one it accepts
        assert ok(kw["A"], kw["I"], kw["Ds"], kw["n"], kw["E"], kw["he"])
    # the issue's reading of it: A <= 4 at the default mixer widths, A <= 10 at E = 16
    assert [A for A in range(1, 17) if ok(A, 72, 42, 3, 32, 64)] == [1, 2, 3, 4]
    assert [A for A in range(1, 17) if ok(A, 72, 42, 3, 16, 64)] == list(range(1, 11))


# ------------------------------------------------------------------------------------ GPU helpers
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a HIP device")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _sac_fold(c, tag=""):
    return ref.Fold(f"sac/{c.name}{tag}", "sac_actor_kernel")


def _qmix_fold(c, tag=""):
    return ref.Fold(f"qmix/{c.name}{tag}", ref.qmix_kernel(c.A))


def _add_sac(fold, c, B, hidden, log_std, action, eps=None):
    """One launch's outputs over the case's first B rows (eps: the noise of a stochastic run)."""
    r = c.ref
    fold.add("hidden", hidden, r.hidden[:B])
    fold.add("log_std", log_std, r.log_std[:B])
    want = ref.sac_action(c.pol, r.mean[:B], r.log_std[:B], eps)
    if eps is None:
        fold.add("action_det", action, want)
    else:
        fold.add("action_stoch", action, want, ref.STOCH_TOL)


def _add_qmix(fold, c, B, epsilon, step, acts, sacts, q_tot, q, hidden, q_chosen=None):
    """Every output of one lbsim_qmix_policy_step over the case's first B rows: the integer ones
    compared here, exactly; the numeric ones gathered in fold."""
    case = f"{fold.case}/B{B}/eps{epsilon}"
    acts_np = acts.cpu().numpy()
    assert acts_np.min() >= 0 and acts_np.max() < c.n
    want, decided = ref.qmix_expected_actions(c, B, epsilon, step)
    np.testing.assert_array_equal(acts_np[decided], want[decided], err_msg=case)
    if sacts is not None:
        np.testing.assert_array_equal(sacts.cpu().numpy(), np.repeat(acts_np, c.k, axis=1),
                                      err_msg=case)
    fold.add("hidden", hidden, c.ref.hidden[:B])
    if q is not None:
        fold.add("q", q, c.ref.q[:B])
    chosen = np.take_along_axis(c.ref.q[:B], acts_np[..., None], 2)[..., 0]
    if q_chosen is not None:
        fold.add("q_chosen", q_chosen, chosen)
        if q is not None:
            assert torch.equal(q_chosen, q.gather(2, acts.unsqueeze(2)).squeeze(2))
    fold.add("q_tot", q_tot, ref.mixer_forward(c.mixer, chosen, c.state[:B]))


def _qmix_policy(c, epsilon):
    agents = [copy.deepcopy(a).to(DEV) for a in c.agents]
    mixer = copy.deepcopy(c.mixer).to(DEV)
    assert FusedQMIXPolicy.supported(agents, mixer, c.n)
    return FusedQMIXPolicy(agents, mixer, c.n, epsilon=epsilon, seed=ref.QMIX_SEED,
                           servers_per_agent=c.k)


# ------------------------------------------------------------------------------------ GPU: shapes
@pytest.mark.gpu
@pytest.mark.parametrize("name", SAC)
def test_sac_shape_case(name):
    """FusedGRUPolicy's one-launch form at B = 1, 16, 129: deterministic, then stochastic at
    steps 0 and 2^31 + 5 under a seed with both key halves set, and at the step whose draw for
    row 89 needs the + 1 of u01_open0; every fifth row reset."""
    _need_gpu()
    c = ref.sac_case(name)
    f = FusedGRUPolicy(copy.deepcopy(c.pol).to(DEV), seed=ref.SAC_SEED)
    assert f.kernel is not None
    fold = _sac_fold(c)
    for B in ref.BATCHES:
        x, h, mask = c.x[:B].to(DEV), c.h[:B].to(DEV), c.mask[:B].to(DEV)
        a, h1, ls = f(x, h, deterministic=True, reset_mask=mask)
        _add_sac(fold, c, B, h1, ls, a)
        assert torch.equal(h.cpu(), c.h[:B])  # not in place: the input is untouched
        for step in ref.SAC_STEPS:
            f.step_no = step
            a, h2, ls = f(x, h, reset_mask=mask)
            _add_sac(fold, c, B, h2, ls, a, ref.sac_noise(ref.SAC_SEED, step, B, c.A))
            assert torch.equal(h1, h2)
    fold.check()


@pytest.mark.gpu
@pytest.mark.parametrize("name", QMIX)
def test_qmix_shape_case(name):
    """FusedQMIXPolicy under the default kernel choice at B = 1, 16, 129: greedy at step 0 and
    epsilon 0.3 at step 2^31 + 5; every seventh row reset; Q-values asked for."""
    _need_gpu()
    c = ref.qmix_case(name)
    fold = _qmix_fold(c)
    for epsilon, step in zip((0.0, 0.3), ref.STEPS):
        pol = _qmix_policy(c, epsilon)
        for B in ref.BATCHES:
            pol.step_no = step
            hid = c.hid[:B].to(DEV).contiguous()
            acts, sacts, q_tot, q = pol(c.obs[:B].to(DEV), hid, c.state[:B].to(DEV),
                                        reset_mask=c.mask[:B].to(DEV), q_values=True)
            _add_qmix(fold, c, B, epsilon, step, acts, sacts, q_tot, q, hid)
    fold.check()


@pytest.mark.gpu
def test_qmix_exact_tie_shape_case():
    """Actions 1 and 2 have the same fc3 row and bias, 10 above action 0: the first maximum, as
    torch.argmax, is 1 for every (env, agent)."""
    _need_gpu()
    c = ref.qmix_case(ref.TIE_CASE)
    pol = _qmix_policy(c, 0.0)
    fold = _qmix_fold(c)
    for B in ref.BATCHES:
        pol.step_no = 0
        hid = c.hid[:B].to(DEV).contiguous()
        acts, sacts, q_tot, q = pol(c.obs[:B].to(DEV), hid, c.state[:B].to(DEV),
                                    reset_mask=c.mask[:B].to(DEV), q_values=True)
        assert torch.equal(q[..., 1], q[..., 2])
        assert bool((acts == 1).all()) and bool((sacts == 1).all())
        _add_qmix(fold, c, B, 0.0, 0, acts, sacts, q_tot, q, hid)
    fold.check()


# ------------------------------------------------------------------------------------ GPU: ABI, guards
PAD = 64  # sentinel rows before and after every buffer
_RAW = {torch.float32: torch.int32, torch.int32: torch.int32, torch.int64: torch.int64,
        torch.uint8: torch.uint8}
# float32: a NaN; a set mask byte; integers no action can be
_SENTINEL = {torch.int32: 0x7FC0BEEF, torch.int64: 0x7FF8DEADBEEF0123, torch.uint8: 1}


class Framed:
    """B rows inside a larger allocation, PAD sentinel rows on each side (NaN for floats, a set
    byte for the mask); rows = the B rows as a view, filled with value or left as sentinels."""

    def __init__(self, B, tail, dtype, value=None):
        raw = _RAW[dtype]
        self.B, self.sent = B, _SENTINEL[raw]
        self.big = torch.full((B + 2 * PAD, *tail), self.sent, dtype=raw, device=DEV)
        self.rows = self.big[PAD:PAD + B].view(dtype)
        if value is not None:
            self.rows.copy_(value.to(DEV))

    def intact(self):
        return bool((self.big[:PAD] == self.sent).all() and (self.big[PAD + self.B:] == self.sent).all())

    def written(self):
        return bool((self.big[PAD:PAD + self.B] != self.sent).all())


def _poison_k_padding(packed, n_rows, K, copies=1):
    """Ones where a packed [n_rows, K] weight (copies of it, stacked) holds its K padding, columns
    K .. 16 ceil(K / 16): the kernels zero those columns of the staged rows themselves, so the
    outputs may not depend on what the weights hold there."""
    kp = -(-K // 16) * 16
    ind = torch.zeros(n_rows, kp, device=packed.device)
    ind[:, K:] = 1.0
    pad = pack_linear(ind) > 0
    packed.view(copies, -1)[:, pad] = 1.0
    return int(pad.sum())


def _qmix_step(lib, net, c, B, step, obs, hid, mask, state, acts, sacts, q, q_chosen, q_tot):
    _lib.check(lib.lbsim_qmix_policy_step(
        ctypes.byref(net), _p(obs), _p(hid), _p(mask), _p(state), B, ref.QMIX_SEED,
        step & 0xFFFFFFFF, _p(acts), _p(sacts), _p(q), _p(q_chosen), _p(q_tot), _stream()))
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["4x4_he48", "2x4"])
def test_qmix_direct_abi_shape_case(name):
    """lbsim_qmix_policy_step with the QmixPolicy struct of a FusedQMIXPolicy: q_chosen_out is the
    Q-value of the action taken; server_actions_out and q_out are optional."""
    _need_gpu()
    c = ref.qmix_case(name)
    pol = _qmix_policy(c, 0.3)
    lib, B, step = _lib.load(), 129, ref.STEPS[1]
    obs, state = c.obs.to(DEV), c.state.to(DEV)
    mask = c.mask.to(DEV, torch.uint8)
    new = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=DEV)  # noqa: E731
    outs, fold = [], _qmix_fold(c, "/abi")
    for full in (False, True):
        hid = c.hid.to(DEV).contiguous()
        acts, q_chosen, q_tot = new(B, c.A, dt=torch.int64), new(B, c.A), new(B, 1)
        sacts = new(B, c.A * c.k, dt=torch.int32) if full else None
        q = new(B, c.A, c.n) if full else None
        _qmix_step(lib, pol.net, c, B, step, obs, hid, mask, state, acts, sacts, q, q_chosen, q_tot)
        _add_qmix(fold, c, B, 0.3, step, acts, sacts, q_tot, q, hid, q_chosen)
        outs.append((acts, q_chosen, q_tot, hid))
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    fold.check()


@pytest.mark.gpu
def test_sac_guards_shape_case():
    """lbsim_sac_actor_step on buffers framed by sentinel rows: no store outside rows [0, B), and
    no read of a neighbouring row reaches an output (the neighbours are NaN, the mask's set), at
    B = 1 and 129.  The packed w_ih holds ones in its K padding: the staged state rows are zero
    there."""
    _need_gpu()
    c = ref.sac_case("99x9")
    f = FusedGRUPolicy(copy.deepcopy(c.pol).to(DEV), seed=ref.SAC_SEED)
    assert f.kernel is not None
    assert _poison_k_padding(f._packed[0], 3 * 128, 99) == 3 * 128 * 13  # w_ih, columns 99..111
    fold = _sac_fold(c, "/framed")
    for B in (1, 129):
        state = Framed(B, (99,), torch.float32, c.x[:B])
        hidden = Framed(B, (128,), torch.float32, c.h[:B])
        mask = Framed(B, (), torch.uint8, c.mask[:B].to(torch.uint8))
        for det, step in ((1, 0), (0, ref.STEPS[1])):
            hidden.rows.copy_(c.h[:B].to(DEV))
            action, log_std = Framed(B, (c.A,), torch.float32), Framed(B, (c.A,), torch.float32)
            _lib.check(_lib.load().lbsim_sac_actor_step(
                ctypes.byref(f.kernel), _p(state.rows), _p(hidden.rows), _p(mask.rows), B, det,
                ref.SAC_SEED, step & 0xFFFFFFFF, _p(action.rows), _p(log_std.rows), _stream()))
            torch.cuda.synchronize()
            for buf in (state, hidden, mask, action, log_std):
                assert buf.intact()
            assert action.written() and log_std.written()
            assert torch.equal(state.rows.cpu(), c.x[:B])
            _add_sac(fold, c, B, hidden.rows, log_std.rows, action.rows,
                     None if det else ref.sac_noise(ref.SAC_SEED, step, B, c.A))
    fold.check()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["4x3", "4x1_obs100", "4x8", "5x1"])
def test_qmix_guards_shape_case(name):
    """The same for lbsim_qmix_policy_step: by default 4x3, 4x1_obs100 and 4x8 run the pair
    kernel (obs staged by obs1, by obs1 with padded columns, by the loop; state rows by the pre3
    path / stage_rows), 5x1 the wave kernel; under LBSIM_QMIX_KERNEL=tile (test_other_kernel_forms)
    all of them run qmix_policy_kernel."""
    _need_gpu()
    c = ref.qmix_case(name)
    pol = _qmix_policy(c, 0.3)
    # the agents' w_ih past the obs width, the mixer's first layers past the state width
    _poison_k_padding(pol._packed[0], 3 * 64, c.I, c.A)
    assert _poison_k_padding(pol._packed[10], 3 * c.he + c.E, c.Ds) > 0
    step, fold = ref.STEPS[1], _qmix_fold(c, "/framed")
    for B in (1, 129):
        obs = Framed(B, (c.A, c.I), torch.float32, c.obs[:B])
        hid = Framed(B, (c.A, 64), torch.float32, c.hid[:B])
        state = Framed(B, (c.Ds,), torch.float32, c.state[:B])
        mask = Framed(B, (), torch.uint8, c.mask[:B].to(torch.uint8))
        acts, sacts = Framed(B, (c.A,), torch.int64), Framed(B, (c.A * c.k,), torch.int32)
        q, q_chosen = Framed(B, (c.A, c.n), torch.float32), Framed(B, (c.A,), torch.float32)
        q_tot = Framed(B, (1,), torch.float32)
        _qmix_step(_lib.load(), pol.net, c, B, step, obs.rows, hid.rows, mask.rows, state.rows,
                   acts.rows, sacts.rows, q.rows, q_chosen.rows, q_tot.rows)
        for buf in (obs, hid, state, mask, acts, sacts, q, q_chosen, q_tot):
            assert buf.intact()
        for buf in (acts, sacts, q, q_chosen, q_tot):
            assert buf.written()
        assert torch.equal(obs.rows.cpu(), c.obs[:B]) and torch.equal(state.rows.cpu(), c.state[:B])
        _add_qmix(fold, c, B, 0.3, step, acts.rows, sacts.rows, q_tot.rows, q.rows, hid.rows,
                  q_chosen.rows)
    fold.check()


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"LBSIM_QMIX_KERNEL": "wave"},
                                 {"LBSIM_QMIX_KERNEL": "tile"},
                                 {"LBSIM_FUSED_MT": "1"},
                                 {"LBSIM_FUSED_MT": "2", "LBSIM_QMIX_KERNEL": "tile"},
                                 {"LBSIM_FUSED_MT": "4", "LBSIM_QMIX_KERNEL": "tile"}])
def test_other_kernel_forms(env):
    """Every *_shape_case of this file under the other kernel forms (read once per process, so in
    a child): one wave per agent at A = 4 too, the layer-split tile kernel, the 16 / 32 / 64-env
    tiles (at 512x16 the 64-env SAC tile backs off to 32)."""
    from tests.parity import run_cases_in_child
    run_cases_in_child("test_fused_policy_shapes.py", "shape_case", env, timeout=300)


# ------------------------------------------------------------------------------------ GPU: GEMM form
def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


@pytest.mark.gpu
@pytest.mark.parametrize("H", [7, 128])
@pytest.mark.parametrize("B", [1, 257])
def test_gru_gates_epilogue(B, H):
    _need_gpu()
    g = torch.Generator().manual_seed(100 * H + B)
    gi, gh = torch.randn(B, 3 * H, generator=g) * 2, torch.randn(B, 3 * H, generator=g) * 2
    h = torch.randn(B, H, generator=g) * 0.5
    out = Framed(B, (H,), torch.float32)
    d = [t.to(DEV) for t in (gi, gh, h)]
    _lib.check(_lib.load().lbsim_gru_gates(_p(d[0]), _p(d[1]), _p(d[2]), _p(out.rows), B, H,
                                           _stream()))
    torch.cuda.synchronize()
    a, c, hp = gi.double().numpy(), gh.double().numpy(), h.double().numpy()
    r, z = _sig(a[:, :H] + c[:, :H]), _sig(a[:, H:2 * H] + c[:, H:2 * H])
    n = np.tanh(a[:, 2 * H:] + r * c[:, 2 * H:])
    assert out.intact() and out.written()
    ref.check(f"gru_gates/B{B}/H{H}", "gru_gates_kernel", "hidden", out.rows, (1 - z) * n + z * hp)


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 16])
@pytest.mark.parametrize("B", [1, 257])
def test_sac_head_epilogue(B, A):
    _need_gpu()
    g = torch.Generator().manual_seed(100 * A + B)
    y = torch.randn(B, 2 * A, generator=g)
    pol = SimpleNamespace(action_scale=4.95, action_bias=5.05)
    yd, y64 = y.to(DEV), y.double().numpy()
    ls = np.clip(y64[:, A:], -0.5, 0.5)
    if B > 1:
        assert (ls == -0.5).mean() > 0.1 and (ls == 0.5).mean() > 0.1
    fold = ref.Fold(f"sac_head/B{B}/A{A}", "sac_head_kernel")
    for det, step in ((1, 0),) + tuple((0, s) for s in ref.SAC_STEPS):
        action, log_std = Framed(B, (A,), torch.float32), Framed(B, (A,), torch.float32)
        _lib.check(_lib.load().lbsim_sac_head(_p(yd), B, A, -0.5, 0.5, 4.95, 5.05, det,
                                              ref.SAC_SEED, step & 0xFFFFFFFF, _p(action.rows),
                                              _p(log_std.rows), _stream()))
        torch.cuda.synchronize()
        assert action.intact() and log_std.intact() and action.written() and log_std.written()
        fold.add("log_std", log_std.rows, ls)
        if det:
            fold.add("action_det", action.rows, ref.sac_action(pol, y64[:, :A], ls))
        else:
            eps = ref.sac_noise(ref.SAC_SEED, step, B, A)
            fold.add("action_stoch", action.rows, ref.sac_action(pol, y64[:, :A], ls, eps),
                     ref.STOCH_TOL)
    fold.check()


@pytest.mark.gpu
@pytest.mark.parametrize("A,E", [(1, 32), (16, 16)])
@pytest.mark.parametrize("B", [1, 257])
def test_qmix_tail_epilogue(B, A, E):
    """Row strides larger than the rows, as FusedQMixer passes slices of its concatenated GEMM."""
    _need_gpu()
    g = torch.Generator().manual_seed(100 * A + B)
    q = torch.randn(B, A, generator=g)
    z1 = torch.randn(B, A * E + 5, generator=g) * 0.5   # w1 = z1[:, 3:3 + A E]
    z2 = torch.randn(B, 2 * E + 9, generator=g) * 0.5   # b1 = z2[:, :E], w2 = z2[:, E + 2:2 E + 2]
    z3 = torch.randn(B, 3, generator=g)                 # b2 = z3[:, 1]
    d1, d2, d3 = z1.to(DEV), z2.to(DEV), z3.to(DEV)
    w1, b1, w2, b2 = d1[:, 3:3 + A * E], d2[:, :E], d2[:, E + 2:2 * E + 2], d3[:, 1:2]
    qd, out = q.to(DEV), Framed(B, (1,), torch.float32)
    _lib.check(_lib.load().lbsim_qmix_tail(_p(qd), _p(w1), w1.stride(0), _p(b1), b1.stride(0),
                                           _p(w2), w2.stride(0), _p(b2), b2.stride(0), B, A, E,
                                           _p(out.rows), _stream()))
    torch.cuda.synchronize()
    n = lambda t: t.cpu().double().numpy()  # noqa: E731
    hid = np.einsum("ba,bae->be", n(q), np.abs(n(w1)).reshape(B, A, E)) + n(b1)
    hid = np.where(hid > 0, hid, np.expm1(hid))
    want = (hid * np.abs(n(w2))).sum(1, keepdims=True) + n(b2)
    assert out.intact() and out.written()
    ref.check(f"qmix_tail/B{B}/A{A}/E{E}", "qmix_tail_kernel", "q_tot", out.rows, want)
