"""Exact flow-completion-time statistics (lbsim_flow_stats_*, VecLoadBalanceEnv(flow_stats=True)).

The reference is the unmodified oracle, read through its snapshot.  Algorithm R puts sample c into
slot c while c < 128, so while a server's count stays <= 128 its records [c_before, c_after) of a
step are exactly that step's completions, in order (lost-FIN handles: the duration reservoir,
whose samples are the real tc - ta).  A server that is down after a step completed nothing in it;
under next-step auto-reset an env whose previous step returned done contributes nothing for the
step that resets it; under same-step auto-reset the oracle's state is read before its masked
reset is applied.  Every comparison with the device is exact.
"""
import numpy as np
import pytest

from marllb_amd import flowstats
from tests import parity, statelayout
from tests.parity import GROUP, actions, lib, step_both  # noqa: F401  (lib: the fixture)
from tests.test_step_plan import run_probe

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
K = 128
Q_PPM = [500000, 900000, 990000, 1000000]
TWO_LAUNCH = 2  # kStepTwoLaunch


# ------------------------------------------------------------------ the two rules (no GPU)

def test_bins_are_monotone_contiguous_and_narrow():
    lower = flowstats.bin_lower_us()
    assert flowstats.NBINS == 192 and lower.shape == (193,) and lower[192] == 1 << 26
    k = np.arange(192)
    np.testing.assert_array_equal(flowstats.bin_of(lower[:192]), k)      # every bin is reachable
    np.testing.assert_array_equal(flowstats.bin_of(lower[1:] - 1), k)    # and ends where the next starts
    width = lower[1:] - lower[:192]
    assert (width[:8] == 1).all() and (8 * width[8:] <= lower[8:192]).all()
    rng = np.random.default_rng(0)
    v = np.unique(np.concatenate([np.arange(0, 5000), rng.integers(0, 1 << 27, 20000),
                                  (1 << np.arange(3, 28)) - 1, 1 << np.arange(3, 28)]))
    b = flowstats.bin_of(v)
    assert (np.diff(b) >= 0).all() and b.min() == 0 and b.max() == 191
    assert (flowstats.bin_of(np.array([1 << 26, (1 << 26) + 5, (1 << 31) - 1, 1 << 40])) == 191).all()
    inside = v < (1 << 26)
    assert (lower[b[inside]] <= v[inside]).all() and (v[inside] < lower[b[inside] + 1]).all()
    assert int(flowstats.bin_of(7)) == 7 and int(flowstats.bin_of(8)) == 8


def exact_quantile(sorted_vals, q_ppm):
    n = len(sorted_vals)
    r = max(1, (q_ppm * n + 999999) // 1000000)
    return int(sorted_vals[r - 1])


def check_bound(got, sorted_vals, q_ppm, what=""):
    """at or above the exact nearest-rank quantile, below 9/8 of it + 1; exact at q = 1"""
    want = exact_quantile(sorted_vals, q_ppm)
    assert want <= got and 8 * got < 9 * want + 8, (what, q_ppm, want, got)
    if q_ppm == 1000000:
        assert got == want, (what, want, got)


def test_quantile_rule_bounds_on_random_samples():
    rng = np.random.default_rng(1)
    for trial in range(60):
        n = int(rng.integers(1, 400))
        # (below 2^26 us: the last bin is open-ended, only q = 1 is bounded there)
        top = int(rng.choice([6, 40, 3000, 250000, 1 << 25, 1 << 26]))
        vals = np.sort(rng.integers(0, top, n))
        hist = np.bincount(flowstats.bin_of(vals), minlength=192)
        qs = [1, 1000, 500000, 900000, 990000, 999999, 1000000]
        got = flowstats.quantile_us(hist, vals[-1], qs)
        for q, g in zip(qs, got.tolist()):
            check_bound(g, vals, q, trial)
    empty = flowstats.quantile_us(np.zeros((3, 192), np.int64), np.zeros(3, np.int64), Q_PPM)
    assert empty.shape == (3, 4) and not empty.any()
    # below 8 us every bin is one value: exact at every quantile
    small = np.sort(rng.integers(0, 8, 50))
    got = flowstats.quantile_us(np.bincount(small, minlength=192), small[-1], [250000, 500000, 750000])
    assert got.tolist() == [exact_quantile(small, q) for q in (250000, 500000, 750000)]
    # past the clamp q = 1 is still exact: the last bin answers with the maximum
    big = np.sort(rng.integers(1 << 26, 1 << 30, 20))
    hb = np.bincount(flowstats.bin_of(big), minlength=192)
    assert hb[191] == 20 and flowstats.quantile_us(hb, big[-1], [1000000]).tolist() == [big[-1]]
    # out-of-range quantiles clamp to [1, 10^6]
    h = np.bincount(flowstats.bin_of(np.array([5, 100, 7000])), minlength=192)
    assert flowstats.quantile_us(h, 7000, [0, 2000000]).tolist() == [5, 7000]


# ------------------------------------------------------------------ ABI (no GPU)

NAMES = ("lbsim_flow_stats_enable", "lbsim_flow_stats_get", "lbsim_flow_stats_quantiles",
         "lbsim_flow_stats_clear")


def test_header_and_signature_table_declare_the_entry_points():
    from marllb_amd import _lib
    declared = _lib.header_functions()
    for n in NAMES:
        assert n in declared and n in _lib._SIGNATURES
    assert [len(_lib._SIGNATURES[n][1]) for n in NAMES] == [1, 6, 6, 3]
    assert "#define LBSIM_FLOW_STATS_BINS 192" in open(_lib.HEADER_PATH).read()


def test_abi_version_stays_and_null_handles_are_rejected():
    from marllb_amd import _lib
    lib = _lib.load()
    assert lib.lbsim_abi_version() == 10
    assert lib.lbsim_flow_stats_enable(None) == _lib.EINVAL
    assert lib.lbsim_flow_stats_get(None, None, None, None, None, None) == _lib.EINVAL
    assert lib.lbsim_flow_stats_quantiles(None, None, 1, 0, None, None) == _lib.EINVAL
    assert lib.lbsim_flow_stats_clear(None, None, None) == _lib.EINVAL


# ------------------------------------------------------------------ the plan (no GPU)

def _plan_row(B, S, simds=1024, **over):
    """plan_probe's first 20 input integers (tests/golden/step_plan.jsonl's header order); the
    21st, flow_stats, is appended by the test (absent: 0)."""
    f = dict(B=B, S=S, Q=32, policy=0, trace=0, fail=0, leak=0, split=0, res_vpp=0, dur_plane=0,
             next_reset=0, dyn_mapping=0, step_kernel=0, simds=simds, group_lanes_set=0,
             group_lanes=0, dyn_wave=-1, dyn_epw=0, ov_step_kernel=0, step_wave_occ=0)
    assert set(over) <= set(f)
    f.update(over)
    return list(f.values())


def test_statistics_handles_plan_the_full_group_kernel(tmp_path):
    rows = [_plan_row(67, 4),                        # would take the one-launch wave step
            _plan_row(67, 4, dyn_mapping=1),         # env-per-lane asked for
            _plan_row(4096, 8, dyn_mapping=1),
            _plan_row(67, 4, step_kernel=2),         # the fused step asked for
            _plan_row(65536, 4, step_kernel=2),
            _plan_row(65536, 4),                     # the headline shape
            _plan_row(65536, 4, next_reset=1),
            _plan_row(8192, 16, simds=416),
            _plan_row(19, 2, Q=32)]
    plain = run_probe(tmp_path, rows)
    off = run_probe(tmp_path, [r + [0] for r in rows])
    on = run_probe(tmp_path, [r + [1] for r in rows])
    assert off == plain  # the flag clear: the dispatch of today, field for field
    assert {p["form"] for p in plain} == {0, 1, 2} and {p["dyn"]["kernel"] for p in plain} == {0, 1, 2}
    for r, p, q in zip(rows, on, plain):
        assert p["form"] == TWO_LAUNCH and p["dynamics_kernel"] == GROUP, (r, p)
        for d in (p["dyn"], p["reset_dyn"]):
            assert d["kernel"] == GROUP and d["full"] == 1 and d["waves"] == 0, (r, d)
            assert d["width"] >= r[1] and d["width"] >= 2 and d["block"] == 64, (r, d)
            assert d["grid"] == -(-r[0] // d["epw"]), (r, d)
        assert p["nr"] == r[10]
        assert p["obs"] == q["obs"] and p["reset_obs"] == q["reset_obs"]  # the observe is unaffected
    # a handle that is full already plans the same with and without the flag
    full = [_plan_row(67, 4, res_vpp=1), _plan_row(65536, 4, res_vpp=1, step_kernel=2)]
    assert run_probe(tmp_path, [r + [1] for r in full]) == run_probe(tmp_path, full)


# ------------------------------------------------------------------ the oracle-side reference

class OracleFlows:
    """The oracle stepped beside the device, and the flow statistics its records imply."""

    def __init__(self, oracle_mod, B, S, kw, next_step=False, same_step=False, offset=0):
        from marllb_amd.env import make_config
        okw = dict(kw)
        if next_step:
            okw["next_step_reset"] = True
        self.cfg = make_config(B, S, env_id_offset=offset, **okw)
        self.ora = oracle_mod.OracleEnv(self.cfg, threads=4)
        self.B, self.S, self.next_step, self.same_step = B, S, next_step, same_step
        self.prev_done = np.zeros(B, bool)
        self.peak = 0  # the largest reservoir count seen: the reference needs <= 128
        self.clear()
        self.values = [[[] for _ in range(S)] for _ in range(B)]  # never cleared: see clear()

    def clear(self, mask=None):
        B, S = self.B, self.S
        if mask is None:
            self.count = np.zeros((B, S), np.uint32)
            self.sum_us = np.zeros((B, S), np.uint64)
            self.max_us = np.zeros((B, S), np.uint32)
            self.hist = np.zeros((B, S, flowstats.NBINS), np.uint32)
            self.values = [[[] for _ in range(S)] for _ in range(B)]
            return
        m = np.asarray(mask).astype(bool)
        self.count[m], self.sum_us[m], self.max_us[m], self.hist[m] = 0, 0, 0, 0
        for b in np.flatnonzero(m):
            self.values[b] = [[] for _ in range(S)]

    def _read(self):
        """(completion counts (B, S), records (B, S, K) us, queued (B, S), down (B, S) or None)"""
        cfg, B, S = self.cfg, self.B, self.S
        fail = cfg.fail_prob > 0
        sp = statelayout.split_p(cfg)
        d = statelayout.parse_cfg(self.ora.state_bytes(), cfg)
        count = d["res_count_dur"] if sp else d["res_count"]
        rec = d["res_dur"] if sp else d["res_fct"]  # lost-FIN: the real tc - ta
        down = d["down"].reshape(B, S) != 0 if fail else None
        return (count.reshape(B, S).astype(np.int64), rec.reshape(B, S, K),
                (d["hc"].reshape(B, S) >> 16).astype(np.int64), down)

    def reset(self):
        obs = self.ora.reset()
        self.c, _, self.q, _ = self._read()
        self.prev_done[:] = False
        return obs

    def step(self, a):
        oo, ro, do, ao = self.ora.step(a)
        c1, rec, q1, down = self._read()
        self.peak = max(self.peak, int(c1.max()))
        assert self.peak <= K, "the oracle's reservoirs wrapped: its records no longer list every flow"
        for b in range(self.B):
            if self.next_step and self.prev_done[b]:
                continue  # the step that resets the env: its warm-up is not counted
            for s in range(self.S):
                if down is not None and down[b, s]:
                    continue  # failed now or earlier: nothing completed, the queue was lost
                c0 = int(self.c[b, s])
                n = int(c1[b, s]) - c0
                # every flow is accounted for: assigned + queued before = completed + queued after
                assert n >= 0 and int(ao[b, s]) + int(self.q[b, s]) == n + int(q1[b, s]), (b, s)
                if n == 0:
                    continue
                v = rec[b, s, c0:c0 + n].astype(np.int64)
                self.count[b, s] += n
                self.sum_us[b, s] += np.uint64(v.sum())
                self.max_us[b, s] = max(int(self.max_us[b, s]), int(v.max()))
                np.add.at(self.hist[b, s], flowstats.bin_of(v), 1)
                self.values[b][s].extend(v.tolist())
        self.c, self.q = c1, q1
        if self.next_step:
            self.prev_done = do.astype(bool)
        if self.same_step and do.any():
            oo = self.ora.reset(mask=do, obs=oo)
            self.c, _, self.q, _ = self._read()
        return oo, ro, do, ao

    def close(self):
        self.ora.close()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def compare_stats(env, ref, what=""):
    """count, sum, maximum, histogram and the four quantiles (per server and per env) of the
    handle against the oracle-derived ones, exactly."""
    cnt, sm, mx, h = env.handle.flow_stats(hist=True)
    np.testing.assert_array_equal(u32(cnt), ref.count, err_msg=f"count {what}")
    np.testing.assert_array_equal(sm.cpu().numpy().view(np.uint64), ref.sum_us, err_msg=f"sum {what}")
    np.testing.assert_array_equal(u32(mx), ref.max_us, err_msg=f"max {what}")
    np.testing.assert_array_equal(u32(h), ref.hist, err_msg=f"hist {what}")
    qs = u32(env.handle.flow_quantiles(Q_PPM, per_server=True))
    qe = u32(env.handle.flow_quantiles(Q_PPM, per_server=False))
    np.testing.assert_array_equal(qs, flowstats.quantile_us(ref.hist, ref.max_us, Q_PPM),
                                  err_msg=f"server quantiles {what}")
    np.testing.assert_array_equal(
        qe, flowstats.quantile_us(ref.hist.astype(np.uint64).sum(1), ref.max_us.max(1), Q_PPM),
        err_msg=f"env quantiles {what}")
    return qs, qe


def check_against_values(ref, qs, qe):
    """the device quantiles against the sorted oracle values (the rule's guarantee)"""
    for b in range(ref.B):
        pooled = sorted(v for s in range(ref.S) for v in ref.values[b][s])
        for i, q in enumerate(Q_PPM):
            if pooled:
                check_bound(int(qe[b, i]), pooled, q, ("env", b))
            else:
                assert qe[b, i] == 0
            for s in range(ref.S):
                vals = sorted(ref.values[b][s])
                if vals:
                    check_bound(int(qs[b, s, i]), vals, q, ("server", b, s))
                else:
                    assert qs[b, s, i] == 0


def check_full_kernel(lib, env):
    """The full group kernel ran; in the child run, at the forced group width."""
    def default(kern, names):
        assert names.get(0, "").startswith("dynamics_group_full_kernel<"), names
        assert kern == GROUP

    parity.check_dispatch(lib, env, default, forced_group="dynamics_group_full_kernel")


ALIAS = {"assign_policy": "alias", "action_type": "continuous"}
NEXT = {"autoreset": True, "autoreset_mode": "next_step"}
SAME = {"autoreset": True, "autoreset_mode": "same_step"}
# id: (B, S, config kwargs, steps, VecLoadBalanceEnv kwargs)
CASES = {
    "67x4": (67, 4, {"arrival_rate": 100.0, "warmup_steps": 2}, 10, {}),
    "67x4-nowarmup": (67, 4, {"arrival_rate": 100.0, "warmup_steps": 0}, 12, {}),
    "67x3-inactive-lane": (67, 3, {"arrival_rate": 60.0, "warmup_steps": 3}, 10, {}),
    "35x8": (35, 8, {"arrival_rate": 160.0, "warmup_steps": 2}, 10, {}),
    "19x16": (19, 16, {"arrival_rate": 320.0, "warmup_steps": 2}, 10, {}),
    "35x8-fail": (35, 8, {"arrival_rate": 160.0, "warmup_steps": 2, "fail_prob": 0.05,
                          "recover_prob": 0.3}, 10, {}),
    "67x4-lostfin": (67, 4, {"arrival_rate": 100.0, "warmup_steps": 2, "lost_fin_prob": 0.2,
                             "flow_timeout": 0.4}, 10, {}),
    "19x16-lostfin-fail": (19, 16, {"arrival_rate": 320.0, "warmup_steps": 2, "lost_fin_prob": 0.1,
                                    "flow_timeout": 0.5, "fail_prob": 0.05, "recover_prob": 0.3},
                           10, {}),
    "67x4-q4-drops": (67, 4, {"arrival_rate": 100.0, "load": 1.3, "warmup_steps": 2,
                              "queue_capacity": 4}, 10, {}),
    "67x4-alias": (67, 4, {"arrival_rate": 100.0, "warmup_steps": 2, **ALIAS}, 10, {}),
    "67x4-envlane-asked": (67, 4, {"arrival_rate": 100.0, "warmup_steps": 2, "dyn_mapping": "env"},
                           10, {}),
    "67x4-nextstep": (67, 4, {"arrival_rate": 100.0, "warmup_steps": 2, "max_steps": 4}, 10, NEXT),
    "67x4-samestep": (67, 4, {"arrival_rate": 100.0, "warmup_steps": 2, "max_steps": 4}, 10, SAME),
    "19x2-long-flows": (19, 2, {"arrival_rate": 8.0, "warmup_steps": 0, "server_rates": [1.0, 1.0],
                                "queue_capacity": 32}, 160, {}),
}


def make_pair(oracle_mod, B, S, kw, env_kw, offset=0, **extra):
    from marllb_amd.env import VecLoadBalanceEnv
    ekw = {"autoreset": False, **env_kw, **extra}
    env = VecLoadBalanceEnv(B, S, device="cuda:0", flow_stats=True, env_id_offset=offset, **ekw, **kw)
    ref = OracleFlows(oracle_mod, B, S, kw, next_step=env.next_step,
                      same_step=bool(ekw["autoreset"]) and not env.next_step, offset=offset)
    return env, ref


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_statistics_equal_the_oracles_records(lib, oracle_mod, case):
    B, S, kw, steps, env_kw = CASES[case]
    idx = list(CASES).index(case)
    kw = {"seed": 500 + idx, **kw}
    env, ref = make_pair(oracle_mod, B, S, kw, env_kw)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    compare_stats(env, ref, "after reset")  # the warm-up counted nothing
    rng = np.random.default_rng(idx)
    dones = 0
    for k in range(steps):
        dones += int(step_both(env, ref, actions(rng, B, S, kw), k).sum())
        qs, qe = compare_stats(env, ref, f"step {k}")
    check_full_kernel(lib, env)
    check_against_values(ref, qs, qe)
    assert ref.count.sum() > 20 * B  # the case is not vacuous
    if env_kw:
        assert dones >= 2 * B  # episodes ended and restarted inside the run
    if "queue_capacity" in kw and kw["queue_capacity"] == 4:
        st = statelayout.parse_cfg(ref.ora.state_bytes(), ref.cfg)
        assert (st["dropped"] > 0).any()  # flows were dropped, and none of them counted
    if case == "19x2-long-flows":
        assert ref.max_us.max() > 30_000_000 and (ref.hist[:, :, 176:].sum() > 0)  # the top octaves
    if "fail_prob" in kw:
        assert ref._read()[3].any()  # some server is down at the end
    st = env.flow_stats()
    np.testing.assert_array_equal(st["count"].cpu().numpy(), ref.count.astype(np.int64).sum(1))
    np.testing.assert_array_equal(st["sum_us"].cpu().numpy(), ref.sum_us.sum(1).astype(np.int64))
    ref.close()
    env.close()


def _child(env_over):
    """This file's S <= 4 cases in a child process (the overrides are read once per process)."""
    ks = [f"test_statistics_equal_the_oracles_records[{c}]" for c, v in CASES.items() if v[1] <= 4]
    assert len(ks) >= 10
    parity.run_cases_in_child("test_flow_stats.py", ks, env_over)


@gpu
def test_forced_four_lane_groups():
    """LBSIM_DYN_GROUP_LANES=4: the headline shape's 4-lane full kernel on the S <= 4 cases."""
    _child({"LBSIM_DYN_GROUP_LANES": "4"})


@gpu
def test_clearing(lib, oracle_mod):
    """clear(mask): the masked envs restart from zero, the others go on; clear(): zeros."""
    B, S = 67, 4
    kw = {"seed": 41, "arrival_rate": 100.0, "warmup_steps": 2}
    env, ref = make_pair(oracle_mod, B, S, kw, {})
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    rng = np.random.default_rng(41)
    for k in range(5):
        step_both(env, ref, actions(rng, B, S, kw), k)
    mask = np.arange(B) % 3 == 0
    env.clear_flow_stats(torch.from_numpy(mask))
    ref.clear(mask)
    compare_stats(env, ref, "after the masked clear")
    assert not ref.count[mask].any() and ref.count[~mask].all()
    for k in range(5, 9):
        step_both(env, ref, actions(rng, B, S, kw), k)
    qs, qe = compare_stats(env, ref, "after 4 more steps")
    check_against_values(ref, qs, qe)
    env.clear_flow_stats(torch.from_numpy(mask.astype(np.uint8)).to("cuda:0"))  # uint8, on the device
    ref.clear(mask)
    compare_stats(env, ref, "after the second masked clear")
    env.clear_flow_stats()
    ref.clear()
    compare_stats(env, ref, "after the full clear")
    st = env.flow_stats(per_server=True, hist=True)
    assert not any(bool(t.any()) for t in st.values())
    assert not bool(env.fct_quantiles().any())
    ref.close()
    env.close()


@gpu
def test_captured_steps(lib, oracle_mod):
    """Three steps of a graph_mode env with next-step auto-reset and max_steps = 4 captured into
    one graph and replayed twice: the accumulators equal the oracle's over the same 6 steps."""
    B, S = 67, 4
    kw = {"seed": 43, "arrival_rate": 100.0, "warmup_steps": 2, "max_steps": 4}
    env, ref = make_pair(oracle_mod, B, S, kw, NEXT, graph_mode=True)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ref.reset())
    rng = np.random.default_rng(43)
    acts = [actions(rng, B, S, kw) for _ in range(7)]
    static = [torch.from_numpy(acts[0]).to("cuda:0") for _ in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up step (eager, graph_mode buffers)
        env.step(static[0])
    torch.cuda.current_stream().wait_stream(side)
    ref.step(acts[0])
    compare_stats(env, ref, "after the eager step")
    env.clear_flow_stats()
    ref.clear()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):  # the capture records the steps, it does not run them
        for a in static:
            obs, rew, done, _ = env.step(a)
    dones = 0
    for rep in range(2):
        for i in range(3):
            static[i].copy_(torch.from_numpy(acts[1 + 3 * rep + i]))
        cg.replay()
        for i in range(3):
            oo, ro, do, _ = ref.step(acts[1 + 3 * rep + i])
            dones += int(do.sum())
        np.testing.assert_array_equal(obs.cpu().numpy(), oo)  # the outputs of the graph's last step
        np.testing.assert_array_equal(done.cpu().numpy().astype(np.uint8), do)
    assert dones == B  # an episode ended inside the replays, its reset step counted nothing
    qs, qe = compare_stats(env, ref, "after two replays")
    check_against_values(ref, qs, qe)
    ref.close()
    env.close()


@gpu
def test_shards_hold_their_rows(lib):
    """Handles of 33 and 34 envs with env_id_offset 0 and 33 hold the rows of the 67-env handle."""
    from marllb_amd.env import VecLoadBalanceEnv
    B, S, cut = 67, 4, 33
    kw = dict(device="cuda:0", seed=47, autoreset=False, arrival_rate=100.0, warmup_steps=2,
              flow_stats=True)
    full = VecLoadBalanceEnv(B, S, **kw)
    parts = [VecLoadBalanceEnv(cut, S, env_id_offset=0, **kw),
             VecLoadBalanceEnv(B - cut, S, env_id_offset=cut, **kw)]
    assert torch.equal(full.reset(), torch.cat([e.reset() for e in parts]))
    rng = np.random.default_rng(47)
    for _ in range(6):
        a = torch.from_numpy(rng.integers(0, 3, (B, S)))
        fo = full.step(a)[0]
        assert torch.equal(fo, torch.cat([parts[0].step(a[:cut])[0], parts[1].step(a[cut:])[0]]))
    got = full.handle.flow_stats(hist=True)
    assert int(got[0].sum()) > 20 * B
    for i, t in enumerate(got):
        assert torch.equal(t, torch.cat([e.handle.flow_stats(hist=True)[i] for e in parts])), i
    for per_server in (False, True):
        assert torch.equal(full.fct_quantiles(per_server=per_server),
                           torch.cat([e.fct_quantiles(per_server=per_server) for e in parts]))
    for e in [full, *parts]:
        e.close()


@gpu
def test_misuse(lib):
    from marllb_amd.env import VecLoadBalanceEnv
    B, S = 19, 4
    plain = VecLoadBalanceEnv(B, S, device="cuda:0", seed=3, autoreset=False)
    twin = VecLoadBalanceEnv(B, S, device="cuda:0", seed=3, autoreset=False)
    assert torch.equal(plain.reset(), twin.reset())
    with pytest.raises(ValueError, match="first"):
        plain.handle.enable_flow_stats()  # after the first reset: refused, the handle as it was
    a = torch.from_numpy(np.random.default_rng(0).integers(0, 3, (B, S)))
    for _ in range(3):
        x, y = plain.step(a), twin.step(a)
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    assert lib.launch_names(plain.handle) == lib.launch_names(twin.handle)
    for call in (lambda: plain.handle.flow_stats(), lambda: plain.handle.flow_quantiles([500000]),
                 lambda: plain.handle.clear_flow_stats(), lambda: plain.flow_stats(),
                 lambda: plain.fct_quantiles(), lambda: plain.clear_flow_stats()):
        with pytest.raises(lib.LbsimError) as ei:
            call()
        assert ei.value.code == lib.ENOTSUP
    plain.close()
    twin.close()
    env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=3, autoreset=False, flow_stats=True)
    env.handle.enable_flow_stats()  # a second call is a no-op
    env.reset()
    env.handle.enable_flow_stats()
    env.step(a)
    with pytest.raises(ValueError, match="nq"):
        env.handle.flow_quantiles([])
    with pytest.raises(ValueError, match="nq"):
        env.handle.flow_quantiles([500000] * 17)
    assert env.handle.flow_quantiles([500000] * 16).shape == (B, 16)
    # out-of-range quantiles clamp: 0 -> 1 ppm (the minimum's bin), 2 * 10^6 -> the maximum
    q = u32(env.handle.flow_quantiles([0, 2000000, 1000000], per_server=True))
    cnt, _, mx, h = env.handle.flow_stats(hist=True)
    np.testing.assert_array_equal(q, flowstats.quantile_us(u32(h), u32(mx), [1, 1000000, 1000000]))
    np.testing.assert_array_equal(q[:, :, 1], u32(mx))
    st = env.flow_stats(per_server=True)
    assert st["count"].dtype == torch.int64 and st["mean_s"].dtype == torch.float64
    np.testing.assert_array_equal(st["count"].cpu().numpy(), u32(cnt))
    qs = env.fct_quantiles(q=(0.5, 1.0))
    assert qs.dtype == torch.float32 and qs.shape == (B, 2)
    np.testing.assert_allclose(qs[:, 1].cpu().numpy(), env.flow_stats()["max_s"].cpu().numpy(),
                               rtol=1e-6)
    env.close()


@gpu
def test_single_env_facade(lib):
    from marllb_amd import LoadBalanceEnv
    env = LoadBalanceEnv(num_servers=4, seed=5, flow_stats=True, arrival_rate=100.0)
    env.reset()
    for _ in range(4):
        env.step([0, 1, 2, 0])
    st = env.flow_stats(per_server=True, hist=True)
    assert isinstance(st["count"], list) and len(st["count"]) == 4 and sum(st["count"]) > 20
    assert len(st["hist"]) == 4 and [sum(r) for r in st["hist"]] == st["count"]
    tot = env.flow_stats()
    assert isinstance(tot["count"], int) and tot["count"] == sum(st["count"])
    assert tot["max_s"] == max(st["max_s"]) and 0 < tot["mean_s"] <= tot["max_s"]
    q = env.fct_quantiles((0.5, 1.0))
    assert isinstance(q, list) and len(q) == 2 and q[0] <= q[1]
    assert abs(q[1] - tot["max_s"]) <= 1e-6 * tot["max_s"]
    env.clear_flow_stats()
    assert env.flow_stats()["count"] == 0 and env.fct_quantiles() == [0.0, 0.0, 0.0]
    env.close()
    off = LoadBalanceEnv(num_servers=4, seed=5)
    off.reset()
    with pytest.raises(lib.LbsimError):
        off.flow_stats()
    off.close()
