"""Action latency: per-env control delay applied inside the step.

The reference is tests/delay_ref.DelaySim, tests/flowsim_ref.FlowSim with §3.19 added from its
text.  The scenario, cases, actions and weights are tests/test_flowsim_ref.py's (reset, 6 steps, a
masked reset of every third env, 6 steps).  Delays go by env and cycle through 0, dt/5, dt/2,
dt - 1 us, dt and dt + dt/3, with max_delay_steps = 2.

Not gpu: delay 0 against plain FlowSim (which test_flowsim_ref pins to the oracle), whole-step
delays against FlowSim driven with each env's shifted weight history, LSQ / LSQ2 against their
no-delay runs, what the scenario reaches, the switch instant, the helpers of csrc/lbsim_delay.h
compiled as host C++ under the address and undefined-behaviour sanitizers against a naive model,
the sampler and the ABI.  gpu: enabled handles against the reference exactly, weight ring
included; delay 0 against the unmodified oracle on every parity config; whole-step delays against
the oracle and against twin handles fed the shifted actions (cross traffic, server workers, an
outage); fractional delays with cross traffic, workers and an outage against the rule in front
of tests/workers_ref.CrossWorkerSim; and the interplay with resets, snapshots, forks, graphs,
shards and the facades.

The host tests of the reference compare DelaySim with FlowSim and do not run the library: they pin
the reference, which the gpu tests then hold the kernels to.  What fails without the feature are
the probe (no csrc/lbsim_delay.h), the sampler / ABI test and every gpu test.
"""
import copy
import os
import subprocess

import numpy as np
import pytest

from marllb_amd import build
from marllb_amd.env import make_config
from tests import delay_ref as dr
from tests import parity
from tests import test_flowsim_ref as fr
from tests import test_server_workers as sw
from tests import workers_ref as wr
from tests.flowsim_ref import FlowSim
from tests.parity import lib  # noqa: F401  (the fixture: fails a gpu test run without a device)

HERE = os.path.dirname(os.path.abspath(__file__))
K = 128
CASES = fr.CASES
STEPS, RESET_AT = fr.STEPS, fr.RESET_AT
M = 2  # max_delay_steps of the scenario
gpu = pytest.mark.gpu
LSQ = [c for c, v in CASES.items() if v[1].get("assign_policy") in ("lsq", "lsq2")]
WEIGHTED = [c for c in CASES if c not in LSQ]
ALIAS = [c for c in WEIGHTED if CASES[c][1].get("assign_policy") == "alias"]


# ------------------------------------------------------------------ the scenario's parameters

def dt_of(case):
    S, kw = fr.config_kwargs(case)
    return int(round(float(np.float32(make_config(1, S, **kw).step_interval)) * 1e6))


def delays_of(case, B, variant=0):
    """(B,) delays in us: env b takes entry (b + variant) % 6 of the cycle."""
    dt = dt_of(case)
    cyc = [0, dt // 5, dt // 2, dt - 1, dt, dt + dt // 3]
    return np.array([cyc[(b + variant) % 6] for b in range(B)], np.int64)


def seconds(us):
    """f32 seconds that convert back to exactly these microseconds (asserted)."""
    s = (np.asarray(us, np.float64) * 1e-6).astype(np.float32)
    np.testing.assert_array_equal(np.rint(s.astype(np.float64) * 1e6), np.asarray(us))
    return s


def make_sims(case, B, delays, max_delay_steps=M):
    S, kw = fr.config_kwargs(case)
    cfg = make_config(B, S, **kw)
    return [dr.DelaySim(kw["seed"], cfg.env_id_offset + b, S, cfg.queue_capacity,
                        kw.get("assign_policy", "sed"), cfg.arrival_rate,
                        [cfg.server_rate[s] for s in range(S)], dt=cfg.step_interval,
                        warmup_steps=cfg.warmup_steps, trace=kw.get("trace"),
                        max_delay_steps=max_delay_steps, delay_us=int(delays[b]))
            for b in range(B)]


_RUNS = {}
CHANGE_AT = 3  # variant "change": new delays before step 3 (and they stay)


def reference_run(case, B, delays=None, change=False):
    """The scenario on B DelaySim envs -> (cfg, kwargs, actions, events, sims).  An Event also
    carries the queues (ev.queues[b][s]: [(tc, ta)] absolute us) and the weight rings
    (ev.ring (B, M + 2, S) f32) after it.  Computed once per key."""
    key = (case, B, None if delays is None else tuple(int(d) for d in delays), change)
    if key in _RUNS:
        return _RUNS[key]
    S, kw = fr.config_kwargs(case)
    cfg = make_config(B, S, **kw)
    sims = make_sims(case, B, delays_of(case, B) if delays is None else delays)
    drops = np.zeros(B, np.int64)
    acts = fr.actions_of(case, B)
    events = []

    def snapshot(ev):
        ev.dropped = drops.copy()
        ev.in_flight = np.array([m.in_flight() for m in sims])
        ev.arr_idx = np.array([m.k for m in sims])
        ev.next_abs = np.array([m.next_arrival() for m in sims])
        ev.steps = np.array([m.step_no for m in sims])
        ev.queues = [[list(q) for q in m.queues] for m in sims]
        ev.ring = np.stack([m.ring for m in sims])
        events.append(ev)

    def reset(mask):
        ev = fr.Event(B, S)
        ev.mask = mask
        for b in np.flatnonzero(mask):
            drops[b] = 0
            for r in sims[b].reset():
                drops[b] += r.dropped
                for s in range(S):
                    ev.new[b][s][0].extend(r.fct(s))
                    ev.new[b][s][1].extend(r.tc(s))
        snapshot(ev)

    reset(np.ones(B, bool))
    for k in range(STEPS):
        if k == RESET_AT:
            reset(np.arange(B) % 3 == 0)
        if change and k == CHANGE_AT:
            for b, m in enumerate(sims):
                m.set_delay(delays_of(case, B, variant=2)[b])
        wts = fr.weights_of(acts[k], kw)
        ev = fr.Event(B, S)
        for b in range(B):
            r = sims[b].step(wts[b])
            ev.assigned[b] = r.assigned
            drops[b] += r.dropped
            ev.new[b] = [(r.fct(s), r.tc(s)) for s in range(S)]
        snapshot(ev)
    _RUNS[key] = (cfg, kw, acts, events, sims)
    return _RUNS[key]


def drive(case, B, backend, check, delays=None, change=False):
    """The scenario on `backend`: check(event, outputs) after every reset and step."""
    events = reference_run(case, B, delays, change)[3]
    acts = fr.actions_of(case, B)
    it = iter(events)
    check(next(it), backend.reset(None))
    for k in range(STEPS):
        if k == RESET_AT:
            check(next(it), backend.reset((np.arange(B) % 3 == 0).astype(np.uint8)))
        if change and k == CHANGE_AT:
            backend.env.set_action_delay(seconds(delays_of(case, B, variant=2)))
        check(next(it), backend.step(acts[k]))
    return events


def same_events(a, b):
    assert len(a) == len(b)
    for ea, eb in zip(a, b):
        np.testing.assert_array_equal(ea.assigned, eb.assigned)
        np.testing.assert_array_equal(ea.dropped, eb.dropped)
        np.testing.assert_array_equal(ea.arr_idx, eb.arr_idx)
        np.testing.assert_array_equal(ea.next_abs, eb.next_abs)
        assert ea.new == eb.new


# ------------------------------------------------------------------ not gpu: the reference

HOST_B = 12


def plain_args(case, B, b):
    S, kw = fr.config_kwargs(case)
    cfg = make_config(B, S, **kw)
    args = (kw["seed"], cfg.env_id_offset + b, S, cfg.queue_capacity,
            kw.get("assign_policy", "sed"), cfg.arrival_rate,
            [cfg.server_rate[s] for s in range(S)])
    return args, dict(dt=cfg.step_interval, warmup_steps=cfg.warmup_steps, trace=kw.get("trace"))


def same_result(ra, rb, plain, other):
    np.testing.assert_array_equal(ra.assigned, rb.assigned)
    assert ra.dropped == rb.dropped and ra.completed == rb.completed
    assert plain.queues == other.queues and plain.k == other.k
    assert plain.next_arrival() == other.next_arrival()


@pytest.mark.parametrize("j", [0, 1, 2])
@pytest.mark.parametrize("case", list(CASES))
def test_whole_step_delay_is_flowsim_on_the_shifted_history(case, j):
    """DelaySim at delay j dt is FlowSim, event for event, driven with the env's own weight
    history shifted by j steps: the history restarts at the env's masked reset and its first j
    rows are ones.  j = 0: DelaySim is FlowSim, and through test_flowsim_ref that is the oracle."""
    S, kw = fr.config_kwargs(case)
    B = 4
    acts = fr.actions_of(case, B)
    for b in range(B):
        args, opt = plain_args(case, B, b)
        plain = FlowSim(*args, **opt)
        late = dr.DelaySim(*args, max_delay_steps=M, delay_us=j * dt_of(case), **opt)
        for ra, rb in zip(plain.reset(), late.reset()):
            same_result(ra, rb, plain, late)
        hist = []
        for k in range(STEPS):
            if k == RESET_AT and b % 3 == 0:
                for ra, rb in zip(plain.reset(), late.reset()):
                    same_result(ra, rb, plain, late)
                hist = []
            wt = fr.weights_of(acts[k], kw)[b]
            hist.append(wt)
            shifted = hist[-1 - j] if len(hist) > j else np.ones(S, np.float32)
            same_result(plain.step(shifted), late.step(wt), plain, late)
        assert late.reach["split_steps"] == 0


@pytest.mark.parametrize("case", LSQ)
def test_lsq_ignores_the_delay(case):
    """LSQ and LSQ2 do not read weights: the delayed scenario is the plain one."""
    assert len(LSQ) == 3
    same_events(reference_run(case, HOST_B)[3], fr.reference_run(case, HOST_B)[3])


def reach_of(case, B):
    sims = reference_run(case, B)[4]
    return {k: sum(m.reach[k] for m in sims) for k in sims[0].reach}


def check_reaches(case, B):
    """The scenario is not vacuous (asserted on the reference alone)."""
    _, _, _, events, sims = reference_run(case, B)
    S = CASES[case][0]
    count = np.zeros((B, S), np.int64)
    peak = 0
    for ev in events:
        if ev.mask is not None:
            count[ev.mask] = 0
        count += np.array([[len(ev.new[b][s][0]) for s in range(S)] for b in range(B)])
        peak = max(peak, int(count.max()))
    assert peak <= K, "a reservoir wrapped: its records no longer list every flow"
    assert any(ev.mask is not None and not ev.mask.all() for ev in events)
    r = reach_of(case, B)
    assert r["arrivals"] > 20 * B
    # some env with 0 < r < dt had arrivals on both sides of its switch in one step
    assert r["split_steps"] > 0, case
    if case in WEIGHTED and S > 1:
        # an arrival that the other row of its step would have sent elsewhere.  (S = 1: there is
        # no other server -- the pick is server 0 or a drop under any weights -- so no delay can
        # make the two one-server cases reach this.)
        assert r["flips"] > 0, case
    if case in ALIAS and case != "s2-alias-tie":
        # a switch between rows with different sets of servers at w > 0.  (s2-alias-tie holds
        # every weight at (1, 3) and the rows before the episode are ones: always both servers.)
        assert r["set_changes"] > 0, case
    return peak, r


def test_scenario_reaches():
    for case in CASES:
        peak, r = check_reaches(case, HOST_B)
        print(f"REACH {case}: peak reservoir count {peak}, {r}")
    assert len(WEIGHTED) == 11 and len(ALIAS) == 3


def test_the_switch_instant():
    """An arrival exactly at the switch instant uses the new weights; one microsecond earlier it
    is the old ones'.  Env b's first arrival of step 1 comes ta1 us into the step: with the delay
    set to ta1 before that step every arrival of the step runs under W(1), which is the run
    without a delay; with ta1 + 1 the first arrival alone runs under W(0), as with any delay up to
    the second arrival's offset."""
    case, B = "s4-sed-levels", 6
    S, kw = fr.config_kwargs(case)
    dt = dt_of(case)
    acts = fr.actions_of(case, B)
    w0, w1 = fr.weights_of(acts[0], kw), fr.weights_of(acts[1], kw)
    seen = 0
    for b in range(B):
        args, opt = plain_args(case, B, b)

        def step1(delay):
            m = dr.DelaySim(*args, max_delay_steps=1, **opt)
            m.reset()
            m.step(w0[b])
            if delay is not None:
                m.set_delay(delay)
            return m, m.step(w1[b])

        base, rb = step1(None)
        offs = [t - dt * (base.step_no - 1) for t in base._ta[base.k - len(base.rows_used[1]):base.k]]
        if len(offs) < 2 or offs[0] == 0 or offs[1] <= offs[0] + 1:
            continue
        seen += 1
        ta1, ta2 = offs[0], offs[1]
        assert base.first_offsets[1] == ta1 and 0 < ta1 < dt
        at, ra = step1(ta1)
        assert at.rows_used[1] == [1] * len(offs)
        same_result(rb, ra, base, at)
        late, rl = step1(ta1 + 1)
        assert late.rows_used[1] == [0] + [1] * (len(offs) - 1)
        upto, ru = step1(ta2)
        assert upto.rows_used[1] == late.rows_used[1]
        same_result(rl, ru, late, upto)
    assert seen >= 3


def test_the_rule_in_front_of_workers_and_cross_traffic_is_delaysim():
    """DelayRule in front of tests/workers_ref.CrossWorkerSim (the reference of the device tests
    with cross traffic, workers and an outage) with one worker per server and no hidden share is
    DelaySim, event for event."""
    case, B = "s6-alias-continuous", 6
    S, kw = fr.config_kwargs(case)
    delays = delays_of(case, B)
    ones = np.ones((B, S), np.int32)
    both = composite(case, B, delays, ones, sw.rates_of(case, B, ones), np.zeros(B, np.float32),
                     np.ones((B, S), np.float32))
    plain = make_sims(case, B, delays)
    acts = fr.actions_of(case, B)
    for b in range(B):
        for ra, rb in zip(plain[b].reset(), both[b].reset()):
            assert ra.dropped == rb.dropped and ra.completed == rb.completed
        for k in range(6):
            wt = fr.weights_of(acts[k], kw)[b]
            ra, rb = plain[b].step(wt), both[b].step(wt)
            np.testing.assert_array_equal(ra.assigned, rb.assigned)
            assert ra.dropped == rb.dropped and ra.completed == rb.completed
            assert plain[b].rows_used[-1] == both[b].rows_used[-1]
            assert [[(e[0], e[1]) for e in q] for q in both[b].queues] == plain[b].queues
        np.testing.assert_array_equal(plain[b].ring, both[b].ring)
        assert plain[b].reach["split_steps"] == both[b].reach["split_steps"]


# ------------------------------------------------------------------ not gpu: the helpers

def test_helpers_against_a_naive_model(tmp_path):
    """tests/delay_probe.cpp: m, r, the rows read and written, the j < 0 rule and the distinctness
    of the R rows of csrc/lbsim_delay.h, for every M in 1..8, k in 0..40 and the delays round
    every multiple of dt, under the address and undefined-behaviour sanitizers; the converted
    delay_us against numpy's rint."""
    exe = str(tmp_path / "delay_probe")
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(HERE, "delay_probe.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0].startswith("OK ") and int(lines[0].split()[1]) > 100000
    conv = [line.split()[1:] for line in lines[1:]]
    assert len(conv) > 400 and all(line.startswith("C ") for line in lines[1:])
    accepted = refused = halves = 0
    for bits, m, dt, ok, us in conv:
        x = np.array([int(bits)], np.uint32).view(np.float32)[0]
        top = int(m) * int(dt)
        with np.errstate(invalid="ignore", over="ignore"):
            want = np.rint(np.float64(x) * 1e6)
        valid = bool(x >= 0) and want <= top
        assert bool(int(ok)) == valid, (x, ok)
        assert int(us) == (int(want) if valid else 0), (x, us, want)
        accepted += valid
        refused += not valid
        halves += valid and abs(np.float64(x) * 1e6 % 1.0 - 0.5) < 1e-3
    assert accepted > 300 and refused > 50 and halves > 10


def test_sampler_and_abi():
    import torch
    from marllb_amd import _lib, sample_action_delay
    d = sample_action_delay(500, seed=4)
    assert d.shape == (500,) and d.dtype == torch.float32
    assert float(d.min()) >= 0.0 and float(d.max()) <= 0.25 and float(d.max() - d.min()) > 0.2
    assert torch.equal(d, sample_action_delay(500, seed=4))
    assert not torch.equal(d, sample_action_delay(500, seed=5))
    n = sample_action_delay(500, 0.005, 0.2, seed=1)
    assert float(n.min()) >= 0.005 and float(n.max()) <= np.float32(0.2)
    c = sample_action_delay(500, 0.0, 1.0, seed=1, max_delay=0.5)  # clamped to the valid range
    assert float(c.max()) == 0.5 and int((c == 0.5).sum()) > 100
    us = np.rint(c.double().numpy() * 1e6)
    assert us.max() <= 500000
    for bad in (dict(low=-0.1), dict(low=0.3, high=0.2), dict(high=float("nan")),
                dict(high=float("inf")), dict(max_delay=-1.0)):
        with pytest.raises(ValueError):
            sample_action_delay(4, **bad)
    with pytest.raises(ValueError):
        sample_action_delay(0)
    header = open(os.path.join(os.path.dirname(HERE), "include", "lbsim.h")).read()
    for name, nargs in (("lbsim_action_delay_enable", 2), ("lbsim_set_action_delay", 4),
                        ("lbsim_get_action_delay", 3), ("lbsim_clear_action_delay", 2),
                        ("lbsim_action_delay_size", 2), ("lbsim_action_delay_save", 5),
                        ("lbsim_action_delay_load", 5)):
        assert f"int {name}(" in header
        assert len(_lib._SIGNATURES[name][1]) == nargs
        assert hasattr(_lib.load(), name)
    assert "#define LBSIM_ABI_VERSION 10 " in header
    assert _lib.load().lbsim_abi_version() == 10
    import inspect
    from marllb_amd.env import VecLoadBalanceEnv
    sig = inspect.signature(VecLoadBalanceEnv.__init__).parameters
    assert sig["action_delay"].default is False and sig["max_delay_steps"].default == 1


# ------------------------------------------------------------------ the device

GPU_B = fr.GPU_B


def backend(B, S, kw, delays=None, max_delay_steps=M, **extra):
    """An enabled env behind test_server_workers' DeviceBackend; delays in us (None: all 0)."""
    back = sw.DeviceBackend(B, S, kw, action_delay=True, max_delay_steps=max_delay_steps, **extra)
    if delays is not None:
        back.env.set_action_delay(seconds(delays))
        np.testing.assert_array_equal(
            back.env.handle.action_delay_us().cpu().numpy().view(np.uint32), delays)
    return back


def ring_of(env):
    import torch
    B, S = env.num_envs, env.num_servers
    assert env.handle.action_delay_size() == B * (env.max_delay_steps + 2) * S * 4
    buf = torch.full((B, env.max_delay_steps + 2, S), -7.0, dtype=torch.float32, device=env.device)
    env.handle.action_delay_save(buf)
    return buf.cpu().numpy()


def same_bits(a, b, msg):
    np.testing.assert_array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32),
                                  np.ascontiguousarray(b, np.float32).view(np.uint32), err_msg=msg)


class DelayCheck(sw.WorkersCheck):
    """test_server_workers' check of an Event (assign counts, dropped, arr_idx, clock, the next
    arrival, column 0, res_count, the records and their timestamps, columns 1-10 and the reward
    against oracle.features / oracle.rewards, the live ring entries, optionally the flow
    statistics), and the weight ring read through lbsim_action_delay_save."""

    def __call__(self, ev, out):
        super().__call__(ev, out)
        same_bits(ring_of(self.env), ev.ring, "weight ring")


def check_delay_kernel(lib, env):
    """The step ran dynamics_group_delay_kernel, of the forced width in a child run under
    LBSIM_DYN_GROUP_LANES."""
    names = lib.launch_names(env.handle)
    assert lib.load().lbsim_dynamics_kernel(env.handle.h) == parity.GROUP, names
    pre = "dynamics_group_delay_kernel<"
    lanes = os.environ.get("LBSIM_DYN_GROUP_LANES")
    if lanes and int(lanes) >= env.cfg.num_servers:
        pre += f"{lanes},"
    assert names.get(0, "").startswith(pre), names


MAPPED = [(c, m) for c in CASES for m in ("auto", "env", "server")
          if m != "env" or CASES[c][0] <= 16]


@gpu
@pytest.mark.parametrize("case,mapping", MAPPED)
def test_enabled_handles_equal_the_reference(lib, case, mapping):
    S, kw = fr.config_kwargs(case)
    back = backend(GPU_B, S, kw, delays_of(case, GPU_B), dyn_mapping=mapping)
    drive(case, GPU_B, back, DelayCheck(back.env))
    check_delay_kernel(lib, back.env)
    check_reaches(case, GPU_B)
    back.env.close()


@gpu
def test_forced_four_lane_groups():
    """LBSIM_DYN_GROUP_LANES=4: the headline shape's 4-lane full kernel on the S <= 4 cases."""
    ks = [f"test_enabled_handles_equal_the_reference[{c}-auto]" for c, v in CASES.items()
          if v[0] <= 4]
    assert len(ks) >= 6
    parity.run_cases_in_child("test_action_delay.py", ks, {"LBSIM_DYN_GROUP_LANES": "4"})


def _parity_configs():
    from tests.test_gpu_parity import CONFIGS
    return list(range(len(CONFIGS)))


@gpu
@pytest.mark.parametrize("idx", _parity_configs())
def test_delay_zero_equals_the_oracle(lib, oracle_mod, idx):
    """An enabled handle whose delays are all 0 (set explicitly, through the in-place rewrite):
    every output and every state section equal the unmodified oracle's, on the full kernel;
    lost-FIN configs included."""
    from marllb_amd.env import VecLoadBalanceEnv
    from tests.test_gpu_parity import CONFIGS, resolve_kw
    c = CONFIGS[idx]
    B, S, kw = c["B"], c["S"], resolve_kw(c["kw"])
    kw.setdefault("seed", 1000 + idx)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=False, action_delay=True, **kw)
    env.set_action_delay(0.0)
    ora = oracle_mod.OracleEnv(make_config(B, S, **kw), threads=4, trace=kw.get("trace"))
    parity.run_vs_reference(env, ora, dict(c["kw"]), idx, steps=8, post_steps=4,
                            hook=lambda e: check_delay_kernel(lib, e), levels=True)
    ora.close()
    env.close()


class Shifted:
    """The actions a handle without a delay has to be given to do what a handle with delay j dt
    does: each env's own history shifted by j steps, the value `ones` before it."""

    def __init__(self, B, j, ones):
        self.hist, self.j, self.ones = [[] for _ in range(B)], j, ones

    def reset(self, mask):
        for b in np.flatnonzero(mask):
            self.hist[b] = []

    def __call__(self, a):
        out = np.empty_like(a)
        for b, h in enumerate(self.hist):
            h.append(a[b])
            out[b] = h[-1 - self.j] if len(h) > self.j else self.ones
        return out


@gpu
@pytest.mark.parametrize("j", [1, 2])
@pytest.mark.parametrize("case", ["s4-sed-continuous", "s6-alias-continuous"])
def test_whole_step_delay_equals_the_oracle_on_shifted_actions(lib, oracle_mod, case, j):
    """Continuous actions express the weight 1.0: delay j dt against the unmodified oracle fed
    each env's actions j steps late, every output and, at the end, every state section."""
    import torch
    B = GPU_B
    S, kw = fr.config_kwargs(case)
    back = backend(B, S, kw, np.full(B, j * dt_of(case)))
    env = back.env
    ora = oracle_mod.OracleEnv(make_config(B, S, **kw), threads=4)
    np.testing.assert_array_equal(env.reset().cpu().numpy(), ora.reset())
    sh = Shifted(B, j, np.float32(1.0))
    acts = fr.actions_of(case, B)
    for k in range(STEPS):
        if k == RESET_AT:
            mask = (np.arange(B) % 3 == 0).astype(np.uint8)
            og = env.reset(mask=torch.from_numpy(mask)).cpu().numpy()
            np.testing.assert_array_equal(og, ora.reset(mask=mask, obs=og.copy()))
            sh.reset(mask)
        og, rg, dg, info = env.step(torch.from_numpy(acts[k]), assign_counts=True)
        oo, ro, do, ao = ora.step(sh(acts[k]))
        np.testing.assert_array_equal(info["assign_counts"].cpu().numpy(), ao, err_msg=f"assign {k}")
        np.testing.assert_array_equal(og.cpu().numpy(), oo, err_msg=f"obs {k}")
        np.testing.assert_array_equal(rg.cpu().numpy(), ro, err_msg=f"reward {k}")
    parity.compare_state(env.handle, ora, env.cfg)
    ora.close()
    env.close()


@gpu
@pytest.mark.parametrize("case", ["s4-sed-levels", "s8-sed2-rate500", "s6-alias-continuous",
                                  "s4-alias-zero-level"])
def test_mid_run_change(lib, case):
    """New delays before step 3, against the rule evaluated with the current value."""
    S, kw = fr.config_kwargs(case)
    back = backend(GPU_B, S, kw, delays_of(case, GPU_B))
    drive(case, GPU_B, back, DelayCheck(back.env), change=True)
    np.testing.assert_array_equal(
        back.env.handle.action_delay_us().cpu().numpy().view(np.uint32),
        delays_of(case, GPU_B, variant=2))
    back.env.close()


@gpu
def test_the_switch_instant_on_the_device(lib):
    """Each env's delay is the offset of its own first arrival of step 1 (even envs) or one
    microsecond more (odd envs), against the reference."""
    case, B = "s4-sed-levels", 24
    S, kw = fr.config_kwargs(case)
    dt = dt_of(case)
    sims = reference_run(case, B, np.zeros(B, np.int64))[4]
    first = np.array([m.first_offsets[1] if m.first_offsets[1] is not None else 0 for m in sims])
    delays = np.minimum(first + np.arange(B) % 2, dt)
    assert (first > 0).sum() > B // 2
    back = backend(B, S, kw, delays)
    drive(case, B, back, DelayCheck(back.env), delays=delays)
    back.env.close()


@gpu
@pytest.mark.parametrize("case", ["s4-q64-deep", "s6-alias-continuous"])
def test_flow_statistics(lib, case):
    S, kw = fr.config_kwargs(case)
    back = backend(GPU_B, S, kw, delays_of(case, GPU_B), flow_stats=True)
    chk = DelayCheck(back.env, stats=True)
    drive(case, GPU_B, back, chk)
    assert int(chk.fs[0].sum()) > 5 * GPU_B
    back.env.close()


def twins(case, B, j, setup, **extra):
    """A handle with delay j dt given the case's actions, and a handle without the feature given
    the shifted ones (continuous cases: 1.0 is expressible), both with `extra` and set up alike:
    equal outputs after every step and equal state bytes at the end."""
    import torch
    S, kw = fr.config_kwargs(case)
    late = backend(B, S, kw, np.full(B, j * dt_of(case)), **extra)
    plain = sw.DeviceBackend(B, S, kw, **extra)
    for e in (late.env, plain.env):
        setup(e, 0)
    for x, y in zip(late.reset(None), plain.reset(None)):
        assert (x is None and y is None) or np.array_equal(x, y)
    sh = Shifted(B, j, np.float32(1.0))
    acts = fr.actions_of(case, B)
    for k in range(8):
        for e in (late.env, plain.env):
            setup(e, k + 1)
        got, want = late.step(acts[k]), plain.step(sh(acts[k]))
        for x, y, what in zip(got, want, ("obs", "reward", "assign")):
            np.testing.assert_array_equal(x, y, err_msg=f"{what} step {k}")
    assert late.env.handle.state_bytes() == plain.env.handle.state_bytes()
    assert torch.equal(late.env.get_action_delay(),
                       torch.full((B,), np.float32(j * dt_of(case) * 1e-6), device="cuda:0"))
    return late, plain


@gpu
def test_hidden_cross_traffic(lib):
    """With cross traffic the hidden picks are unchanged and the visible picks follow the delayed
    row: a delay of one step equals the twin given every action one step late, hidden counts
    (lost_on, part of the state bytes) included."""
    from tests import test_cross_traffic as ct
    case, B = "s4-sed-continuous", 24
    share, w = ct.cross_params(case, B)

    def setup(env, k):
        if k == 0:
            env.set_cross_traffic(share, w)

    late, plain = twins(case, B, 1, setup, cross_traffic=True)
    _, hid = ct.hidden_queued(late.env)
    assert hid.sum() > 0
    late.env.close()
    plain.env.close()


@gpu
def test_server_workers_above_one(lib):
    case, B = "s6-alias-continuous", 24
    workers = sw.workers_of(case, B)

    def setup(env, k):
        if k == 0:
            env.set_server_workers(workers)

    late, plain = twins(case, B, 2, setup, server_workers=True)
    assert workers.max() > 1
    late.env.close()
    plain.env.close()


@gpu
def test_scripted_outage(lib):
    """Server 1 of every env down for steps 3 and 4."""
    case, B = "s4-sed-continuous", 24
    S = CASES[case][0]

    def setup(env, k):
        if k in (3, 5):
            up = np.ones((1, S), np.uint8)
            up[0, 1] = 0 if k == 3 else 1
            env.set_server_availability(up)

    late, plain = twins(case, B, 1, setup, server_availability=True)
    late.env.close()
    plain.env.close()


class DelayCrossWorkerSim(dr.DelayRule, wr.CrossWorkerSim):
    """§3.17 and §3.18 on the reference (tests/workers_ref.py) with the delay rule in front of the
    choice: a hidden arrival never reaches _choose."""


def composite(case, B, delays, workers, mus, share, w):
    S, kw = fr.config_kwargs(case)
    cfg = make_config(B, S, **kw)
    return [DelayCrossWorkerSim(kw["seed"], cfg.env_id_offset + b, S, cfg.queue_capacity,
                                kw.get("assign_policy", "sed"), cfg.arrival_rate,
                                [float(x) for x in mus[b]], dt=cfg.step_interval,
                                warmup_steps=cfg.warmup_steps, workers=workers[b], share=share[b],
                                weights=w[b], max_delay_steps=M, delay_us=int(delays[b]))
            for b in range(B)]


@gpu
@pytest.mark.parametrize("case", ["s4-q64-deep", "s6-alias-continuous"])
def test_mid_step_switch_with_cross_traffic_and_workers(lib, case):
    """Fractional delays with hidden cross traffic on multi-worker servers, against the reference
    with all three rules: the visible and hidden counts, drops and assignments after every step.
    The hidden picks do not read weights; the visible ones follow the delayed row, switching
    inside the step."""
    from tests import test_cross_traffic as ct
    B = 24
    S, kw = fr.config_kwargs(case)
    delays = delays_of(case, B)
    workers = sw.workers_of(case, B)
    mus = sw.rates_of(case, B, workers)
    share, w = ct.cross_params(case, B)
    back = backend(B, S, kw, delays, server_workers=True, cross_traffic=True)
    back.env.set_server_workers(workers)
    back.env.set_rates(None, mus)
    back.env.set_cross_traffic(share, w)
    sims = composite(case, B, delays, workers, mus, share, w)
    drops = np.array([sum(r.dropped for r in m.reset()) for m in sims])
    back.reset(None)
    acts = fr.actions_of(case, B)
    for k in range(8):
        wts = fr.weights_of(acts[k], kw)
        _, _, assign = back.step(acts[k])
        rs = [m.step(wts[b]) for b, m in enumerate(sims)]
        drops += np.array([r.dropped for r in rs])
        np.testing.assert_array_equal(assign, np.array([r.assigned for r in rs]))
        ct.assert_matches_sims(back.env, sims, drops)
        same_bits(ring_of(back.env), np.stack([m.ring for m in sims]), "weight ring")
    _, hid = ct.hidden_queued(back.env)
    assert hid.sum() > 0 and workers.max() > 1
    assert sum(m.reach["split_steps"] for m in sims) > B and sum(m.reach["flips"] for m in sims) > 0
    assert sum(m.reach["out_of_order"] for m in sims) > 0
    back.env.close()


@gpu
def test_mid_step_switch_across_a_scripted_outage(lib):
    """Fractional delays while server 1 of every env is scripted down for one step (the reference
    drops its queue and keeps it full of flows that never complete while it is down)."""
    case, B, J = "s4-sed-levels", 24, 1
    S, kw = fr.config_kwargs(case)
    delays = delays_of(case, B)
    ones = np.ones((B, S), np.int32)
    mus = sw.rates_of(case, B, ones)
    back = backend(B, S, kw, delays, server_availability=True)
    env, Q = back.env, back.env.cfg.queue_capacity
    sims = composite(case, B, delays, ones, mus, np.zeros(B, np.float32),
                     np.ones((B, S), np.float32))
    drops = np.array([sum(r.dropped for r in m.reset()) for m in sims])
    back.reset(None)
    acts = fr.actions_of(case, B)

    def both_step(k):
        nonlocal drops
        wts = fr.weights_of(acts[k], kw)
        _, _, assign = back.step(acts[k])
        rs = [m.step(wts[b]) for b, m in enumerate(sims)]
        drops = drops + np.array([r.dropped for r in rs])
        np.testing.assert_array_equal(assign, np.array([r.assigned for r in rs]))

    for k in range(3):
        both_step(k)
    sw.assert_matches_sims(env, sims, drops)
    up = np.ones((1, S), np.uint8)
    up[0, J] = 0
    env.set_server_availability(up)
    never = 1 << 60
    for b, m in enumerate(sims):
        drops[b] += m.fail(J)
        m.queues[J] = [(never, 0)] * Q
    both_step(3)
    for m in sims:
        assert len(m.queues[J]) == Q
        m.queues[J] = []
    d = sw.assert_matches_sims(env, sims, drops)
    assert (d["down"].reshape(B, S)[:, J] != 0).all()
    env.set_server_availability(np.ones((1, S), np.uint8))
    for k in range(4, 8):
        both_step(k)
    sw.assert_matches_sims(env, sims, drops)
    same_bits(ring_of(env), np.stack([m.ring for m in sims]), "weight ring")
    assert sum(m.reach["split_steps"] for m in sims) > B
    env.close()


def assert_matches(env, sims, drops):
    d = sw.assert_matches_sims(env, sims, drops)
    same_bits(ring_of(env), np.stack([m.ring for m in sims]), "weight ring")
    return d


@gpu
def test_next_step_auto_reset_across_an_episode_end(lib):
    """max_steps = 3 with next-step auto-reset: the step after an episode's end resets in place.
    It stores no row (the ring keeps the old episode's) and the new episode starts from ones."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    case, B = "s4-sed-levels", 24
    S, kw = fr.config_kwargs(case)
    delays = delays_of(case, B)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", autoreset=True, autoreset_mode="next_step",
                            action_delay=seconds(delays), max_delay_steps=M, max_steps=3, **kw)
    sims = make_sims(case, B, delays)
    drops = np.array([sum(r.dropped for r in m.reset()) for m in sims])
    env.reset()
    acts = fr.actions_of(case, B)
    for k in range(9):
        assert_matches(env, sims, drops)
        wts = fr.weights_of(acts[k], kw)
        _, _, done, info = env.step(torch.from_numpy(acts[k]), assign_counts=True)
        if k % 4 == 3:  # the step after the third: every env resets instead of stepping
            drops = np.array([sum(r.dropped for r in m.reset()) for m in sims])
            assert not info["assign_counts"].any()
        else:
            rs = [m.step(wts[b]) for b, m in enumerate(sims)]
            drops += np.array([r.dropped for r in rs])
            np.testing.assert_array_equal(info["assign_counts"].cpu().numpy(),
                                          np.array([r.assigned for r in rs]))
            assert bool(done.all()) == (k % 4 == 2)
    assert_matches(env, sims, drops)
    env.close()


@gpu
def test_snapshot_restore_and_fork(lib):
    """lbsim_state_size is unchanged and the ring travels beside the snapshot: save, run A,
    restore, run A reproduces the first run, ring included; a fork inherits its source's pending
    actions."""
    import torch
    case, B = "s4-sed-levels", 24
    S, kw = fr.config_kwargs(case)
    back = backend(B, S, kw, delays_of(case, B))
    env = back.env
    plain = sw.DeviceBackend(B, S, kw)
    assert plain.env.handle.state_size() == env.handle.state_size()
    plain.env.close()
    back.reset(None)
    acts = fr.actions_of(case, B)
    for k in range(4):
        back.step(acts[k])
    snap = env.snapshot()
    assert snap.delay.shape == (B, M + 2, S)
    before, ring_before = env.handle.state_bytes(), ring_of(env)
    first = [back.step(acts[k]) for k in range(4, 8)]
    after, ring_after = env.handle.state_bytes(), ring_of(env)
    assert not np.array_equal(ring_before, ring_after)
    env.restore(snap)
    assert env.handle.state_bytes() == before
    same_bits(ring_of(env), ring_before, "restored ring")
    again = [back.step(acts[k]) for k in range(4, 8)]
    for x, y in zip(first, again):
        for a, b in zip(x, y):
            np.testing.assert_array_equal(a, b)
    assert env.handle.state_bytes() == after
    same_bits(ring_of(env), ring_after, "ring after the second run")
    # a masked restore leaves the other envs' rows alone
    mask = torch.from_numpy(np.arange(B) % 2 == 0)
    env.restore(snap, mask=mask)
    ring = ring_of(env)
    same_bits(ring[0::2], ring_before[0::2], "masked restore: restored rows")
    same_bits(ring[1::2], ring_after[1::2], "masked restore: kept rows")
    # a fork: every env takes env src's state and pending actions, keeps its own delay, and
    # goes on under its own randomness after the one drawn arrival (§3.13): the reference is a
    # copy of the source's simulator at the snapshot, holding the arrivals up to the drawn one,
    # with the slot's global id and delay
    src = 4  # (delay dt: its pending row matters)
    delays = delays_of(case, B)
    sims = make_sims(case, B, delays)
    for m in sims:
        m.reset()
    wts = [fr.weights_of(a, kw) for a in acts]
    for k in range(4):
        sims[src].step(wts[k][src])
    env.restore(snap, src=torch.full((B,), src, dtype=torch.int32))
    same_bits(ring_of(env), np.repeat(ring_before[src:src + 1], B, 0), "forked ring")
    np.testing.assert_array_equal(env.handle.action_delay_us().cpu().numpy().view(np.uint32),
                                  delays)
    base = int(sw.workers_state(env)["dropped"][src])
    forks = []
    for b in range(B):
        f = copy.deepcopy(sims[src])
        f.gid = sims[b].gid
        del f._ta[f.k + 1:], f._work[f.k + 1:], f._u2[f.k + 1:]
        f.set_delay(delays[b])
        forks.append(f)
    drops = np.full(B, base, np.int64)
    for k in range(4, 8):
        _, _, assign = back.step(acts[k])
        rs = [f.step(wts[k][b]) for b, f in enumerate(forks)]
        drops += np.array([r.dropped for r in rs])
        np.testing.assert_array_equal(assign, np.array([r.assigned for r in rs]))
        assert_matches(env, forks, drops)
    d = sw.workers_state(env)
    assert len(set(d["arr_idx"].tolist())) > B // 2  # the slots went their own ways
    env.close()


@gpu
def test_replayed_graph_sees_an_in_place_rewrite(lib):
    """A step captured before set_action_delay rewrites the delays in place reads the new ones on
    replay, and the ring index follows ep_step on the device: equal to an eager twin."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    case, B = "s4-sed-levels", 24
    S, kw = fr.config_kwargs(case)
    d1, d2 = seconds(delays_of(case, B)), seconds(delays_of(case, B, variant=3))
    eager = VecLoadBalanceEnv(B, S, device="cuda:0", action_delay=d1, max_delay_steps=M, **kw)
    graph = VecLoadBalanceEnv(B, S, device="cuda:0", action_delay=d1, max_delay_steps=M,
                              graph_mode=True, **kw)
    for e in (eager, graph):
        e.reset()
    acts = [torch.from_numpy(a).to("cuda:0") for a in fr.actions_of(case, B)[:7]]
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
        if k == 4:  # after three replays: new delays, no new capture
            for e in (eager, graph):
                e.set_action_delay(d2)
        a_static.copy_(acts[k])
        cg.replay()
        eo, er, ed, _ = eager.step(acts[k])
        assert torch.equal(obs, eo), k
        assert torch.equal(rew, er) and torch.equal(done, ed), k
    assert graph.handle.state_bytes() == eager.handle.state_bytes()
    same_bits(ring_of(graph), ring_of(eager), "ring")
    eager.close()
    graph.close()


@gpu
def test_shards_at_uneven_sizes(lib):
    """Shards of 5, 12 and 7 envs with their own rows equal the 24-env handle's rows."""
    case, B = "s6-alias-continuous", 24
    S, kw = fr.config_kwargs(case)
    delays = delays_of(case, B)
    whole = backend(B, S, kw, delays)
    acts = fr.actions_of(case, B)
    whole.reset(None)
    outs = [whole.step(acts[k]) for k in range(5)]
    ring = ring_of(whole.env)
    lo = 0
    for n in (5, 12, 7):
        part = backend(n, S, {**kw, "env_id_offset": kw.get("env_id_offset", 0) + lo},
                       delays[lo:lo + n])
        part.reset(None)
        for k in range(5):
            for x, y in zip(part.step(acts[k][lo:lo + n]), outs[k]):
                np.testing.assert_array_equal(x, y[lo:lo + n])
        same_bits(ring_of(part.env), ring[lo:lo + n], "shard ring")
        part.env.close()
        lo += n
    whole.env.close()


@gpu
def test_facades_forward(lib):
    """LoadBalanceEnv and VecMultiAgentLoadBalanceEnv set, read back and clear the delay."""
    from marllb_amd.env import LoadBalanceEnv
    from marllb_amd.multi_agent import VecMultiAgentLoadBalanceEnv
    one = LoadBalanceEnv(num_servers=4, action_delay=0.02, seed=3)
    assert one.get_action_delay() == pytest.approx(0.02, abs=1e-7)
    one.reset()
    one.step(np.zeros(4, np.int64))
    one.set_action_delay(0.1)
    assert one.get_action_delay() == pytest.approx(0.1, abs=1e-7)
    with pytest.raises(ValueError):
        one.set_action_delay(0.3)  # above max_delay_steps * step_interval = 0.25
    assert one.get_action_delay() == pytest.approx(0.1, abs=1e-7)
    one.step(np.ones(4, np.int64))
    one.clear_action_delay()
    assert one.get_action_delay() == 0.0
    one.close()
    from marllb_amd.multi_agent import MultiAgentLoadBalanceEnv
    single = MultiAgentLoadBalanceEnv(num_agents=2, servers_per_agent=2, action_delay=0.05,
                                      max_delay_steps=2)
    assert single.get_action_delay() == pytest.approx(0.05, abs=1e-7)
    single.reset()
    single.step([np.float32(1.0), np.float32(2.0)])
    single.set_action_delay(0.4)
    assert single.get_action_delay() == pytest.approx(0.4, abs=1e-7)
    single.clear_action_delay()
    assert single.get_action_delay() == 0.0
    single.close()
    ma = VecMultiAgentLoadBalanceEnv(6, num_agents=2, servers_per_agent=2, action_delay=True,
                                     max_delay_steps=2)
    rows = np.arange(6, dtype=np.float32) * np.float32(0.1)
    ma.set_action_delay(rows)
    np.testing.assert_array_equal(np.rint(ma.get_action_delay().cpu().numpy().astype(np.float64)
                                          * 1e6), np.arange(6) * 100000)
    ma.reset()
    ma.set_action_delay(0.5)
    assert (ma.get_action_delay() == 0.5).all()
    ma.clear_action_delay()
    assert (ma.get_action_delay() == 0).all()
    ma.vec.close()


@gpu
def test_error_paths(lib):
    import torch
    from marllb_amd import _lib
    from marllb_amd.env import VecLoadBalanceEnv
    for bad in (0, 9, -1):  # M outside 1..8
        with pytest.raises(ValueError):
            VecLoadBalanceEnv(8, 4, device="cuda:0", action_delay=True, max_delay_steps=bad)
    late = VecLoadBalanceEnv(8, 4, device="cuda:0")
    with pytest.raises(ValueError):
        late.set_action_delay(0.1)  # not enabled: EINVAL
    with pytest.raises(ValueError):
        late.get_action_delay()
    with pytest.raises(ValueError):
        late.handle.action_delay_size()
    late.reset()
    with pytest.raises(ValueError):
        late.handle.enable_action_delay(1)  # after the first reset
    late.close()
    env = VecLoadBalanceEnv(8, 4, device="cuda:0", action_delay=True, max_delay_steps=2)
    assert (env.get_action_delay() == 0).all()
    env.set_action_delay(0.5)  # exactly M dt
    env.set_action_delay(np.linspace(0.0, 0.5, 8))
    before = env.handle.action_delay_us().cpu().numpy().copy()
    assert before.view(np.uint32).max() == 500000
    three = torch.zeros(3, dtype=torch.float32, device="cuda:0")
    with pytest.raises(_lib.LbsimError) as e:  # rows neither 1 nor B
        env.handle.set_action_delay(three, rows=3)
    assert e.value.code == _lib.ESHAPE
    with pytest.raises(ValueError):
        env.set_action_delay(np.zeros(3))
    rows = np.zeros(8)
    rows[6] = 0.500001
    for bad in (0.500001, -0.001, float("nan"), float("inf"), -float("inf"), rows,
                [0.1, 0.1, float("nan"), 0.1, 0.1, 0.1, 0.1, 0.1]):
        with pytest.raises(ValueError):
            env.set_action_delay(bad)
        np.testing.assert_array_equal(env.handle.action_delay_us().cpu().numpy(), before)
    size = env.handle.action_delay_size()
    assert size == 8 * 4 * 4 * 4
    for n in (size - 4, size + 4):  # a wrong buffer size on save and load
        buf = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        for call in (env.handle.action_delay_save, env.handle.action_delay_load):
            with pytest.raises(_lib.LbsimError) as e:
                call(buf)
            assert e.value.code == _lib.ESHAPE
    env.reset()
    env.step(torch.zeros((8, 4), dtype=torch.int64))
    env.close()
