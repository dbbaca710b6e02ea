"""Duration samples at every data ACK.

The reference is tests/acks_ref.AckSim, tests/flowsim_ref.FlowSim with §3.25 added from its text in
absolute int64 us.  The scenario is tests/test_flowsim_ref.py's (reset, 12 steps, a masked reset of
every third env after 6) on the cases below: S in {1, 2, 3, 4, 8, 16}, Q in {8, 32}, the five
policies, Poisson and TRACE, max_acks in {1, 8, 32} and ACK intervals of 1 us, 1000 us, 2^30 us and
a per-env mix.  "s2-fast" runs at a 500 us step with service times of some tens to hundreds of us,
so a service spans many steps; "s2-tiny" has service times of a few us, so k is capped by svc.

Not gpu: the reference's own properties (every flow's k ACKs, once, in order, on time), what the
scenarios reach, one ACK per flow against FlowSim, the helpers of csrc/lbsim_acks.h as host C++
under the sanitizers, check_ack_config, the plan.
gpu: enabled handles against the reference and against a plain twin exactly, after every reset and
step, then the interplay with the other domains and the error paths.
"""
import os
import subprocess

import numpy as np
import pytest

import oracle
from marllb_amd import _lib, build, trace
from marllb_amd.acks import ack_count, ack_times, check_ack_config
from marllb_amd.env import make_config
from tests import parity, statelayout
from tests import test_flowsim_ref as fr
from tests.acks_ref import AckSim
from tests.flowsim_ref import FlowSim
from tests.parity import lib  # noqa: F401  (the fixture: fails a gpu test run without a device)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K = 128
STEPS, RESET_AT = fr.STEPS, fr.RESET_AT
gpu = pytest.mark.gpu
ACK_KERNEL = 6  # LBSIM_DYN_KERNEL_ACK
CONT = {"action_type": "continuous"}
BIGI = 1 << 30
GPU_B, HOST_B = 67, 5

# id: (S, config kwargs, max_acks, ack_us: one value or "mixed")
CASES = {
    "s1-sed-q8-m1": (1, {"arrival_rate": 30.0, "server_rates": [20.0], "queue_capacity": 8,
                         "warmup_steps": 2}, 1, 1000),
    "s2-fast": (2, {"arrival_rate": 9000.0, "server_rates": [6000.0, 4000.0],
                    "queue_capacity": 8, "warmup_steps": 2, "step_interval": 0.0005}, 32, 1),
    "s2-tiny": (2, {"assign_policy": "lsq2", "arrival_rate": 40000.0,
                    "server_rates": [300000.0, 200000.0], "queue_capacity": 8, "warmup_steps": 2,
                    "step_interval": 0.0005}, 8, 1),
    "s3-lsq-q8-one-ack": (3, {"assign_policy": "lsq", "queue_capacity": 8, "arrival_rate": 60.0,
                              "load": 1.3, "warmup_steps": 2}, 8, BIGI),
    "s4-sed-q32": (4, {"discrete_weights": [0.5, 1.0, 8.0], "arrival_rate": 60.0,
                       "warmup_steps": 2}, 8, 1000),
    "s4-alias-q32-m32": (4, {"assign_policy": "alias", "discrete_weights": [0.0, 1.0, 3.0],
                             "arrival_rate": 60.0, "warmup_steps": 2}, 32, 1000),
    "s4-sed2-mixed": (4, {"assign_policy": "sed2", **CONT, "queue_capacity": 8,
                          "arrival_rate": 60.0, "warmup_steps": 2}, 32, "mixed"),
    "s8-trace": (8, {"_trace": True, "warmup_steps": 2, "step_interval": 0.1}, 8, 1000),
    "s16-lsq2-q8": (16, {"assign_policy": "lsq2", **CONT, "queue_capacity": 8,
                         "arrival_rate": 160.0, "warmup_steps": 2}, 1, 1),
}
FAST, TINY, MIXED = "s2-fast", "s2-tiny", "s4-sed2-mixed"
HOST_CASES = ("s1-sed-q8-m1", FAST, TINY, "s4-sed-q32", "s4-alias-q32-m32", MIXED, "s8-trace")


def config_kwargs(case):
    S, kw, m, us = CASES[case]
    kw = {"seed": 9100 + list(CASES).index(case), **kw}
    if kw.pop("_trace", False):
        kw["trace"] = trace.synthetic(37, 300.0, seed=7)
    return S, kw, m, us


def intervals_of(case, B):
    us = CASES[case][3]
    if us == "mixed":
        return np.array([(1, 250, 1000, 4000, BIGI)[b % 5] for b in range(B)], np.int32)
    return np.full(B, us, np.int32)


def actions_of(case, B, steps=STEPS):
    S, kw, _, _ = config_kwargs(case)
    rng = np.random.default_rng(100 + list(CASES).index(case))
    out = []
    for _ in range(steps):
        if kw.get("action_type") == "continuous":
            out.append(rng.uniform(-1.0, 11.0, (B, S)).astype(np.float32))
        else:
            n = len(kw.get("discrete_weights", [1.0, 1.5, 2.0]))
            out.append(rng.integers(-n, n, (B, S)).astype(np.int64))
    return out


def make_sims(case, B, policy=None, ack_us=None, max_acks=None, env_id_offset=None):
    S, kw, m, _ = config_kwargs(case)
    cfg = make_config(B, S, **kw)
    us = intervals_of(case, B) if ack_us is None else np.full(B, ack_us, np.int64)
    off = cfg.env_id_offset if env_id_offset is None else env_id_offset
    return [AckSim(kw["seed"], off + b, S, cfg.queue_capacity,
                   policy or kw.get("assign_policy", "sed"), cfg.arrival_rate,
                   [cfg.server_rate[s] for s in range(S)], dt=cfg.step_interval,
                   warmup_steps=cfg.warmup_steps, trace=kw.get("trace"),
                   max_acks=m if max_acks is None else max_acks, ack_us=int(us[b]))
            for b in range(B)]


class Snap:
    """What the reference says the duration reservoirs are after a reset or a step."""

    def __init__(self, sims, mask=None, assigned=None):
        B, S = len(sims), sims[0].S
        self.mask, self.assigned = mask, assigned
        self.count = np.array([m.dur_count for m in sims], np.int64)
        # {age us, ts ms} by slot; the slots at and beyond the count hold nothing: zeros
        self.rec = np.array([[[x or (0, 0) for x in m.dur[s]] for s in range(S)] for m in sims],
                            np.uint32)
        self.big = np.array([m.big for m in sims], bool)
        self.chg = np.zeros((B, S, 4), np.uint32)
        self.stepped = np.ones(B, bool) if mask is None else np.asarray(mask, bool)
        for b, m in enumerate(sims):
            for s in range(S):
                for slot in m.written[s]:
                    self.chg[b, s, slot >> 5] |= np.uint32(1 << (slot & 31))


_RUNS = {}


def reference_run(case, B, steps=STEPS, schedule=None, rates=None, **sim_kw):
    """The scenario on B AckSim envs -> (kwargs, actions, snapshots, sims), once per key.
    schedule = (arrival (B, P), server (B, P, S), H, wrap): a rate schedule, as
    tests/test_processor_sharing.py's; rates = (arrival (B,), server (B, S)): per-env rates."""
    key = (case, B, steps, schedule and schedule[2:], rates is not None, tuple(sorted(sim_kw.items())))
    if key in _RUNS:
        return _RUNS[key]
    S, kw, _, _ = config_kwargs(case)
    sims = make_sims(case, B, **sim_kw)
    acts = actions_of(case, B, steps)
    ep_step = np.zeros(B, np.int64)

    def phase(b, j):
        if schedule is not None:
            lam, mu = schedule[:2]
            sims[b].set_rates(float(lam[b, j]), [float(x) for x in mu[b, j]])

    def sched_phase(k):
        P, H, wrap = schedule[0].shape[1], schedule[2], schedule[3]
        return (k // H) % P if wrap else min(k // H, P - 1)

    if rates is not None:
        for b, m in enumerate(sims):
            m.set_rates(float(rates[0][b]), [float(x) for x in rates[1][b]])
    snaps = []

    def reset(mask):
        for b in np.flatnonzero(mask):
            phase(b, 0)
            sims[b].reset()
            ep_step[b] = 0
        snaps.append(Snap(sims, mask=mask))

    reset(np.ones(B, bool))
    for k in range(steps):
        if k == RESET_AT:
            reset(np.arange(B) % 3 == 0)
        wts = fr.weights_of(acts[k], kw)
        rs = []
        for b, m in enumerate(sims):
            if schedule is not None:
                phase(b, sched_phase(int(ep_step[b])))
            rs.append(m.step(wts[b]))
        ep_step += 1
        snaps.append(Snap(sims, assigned=np.array([r.assigned for r in rs])))
    _RUNS[key] = (kw, acts, snaps, sims)
    return _RUNS[key]


def reach_of(sims):
    return {k: sum(m.reach[k] for m in sims) for k in sims[0].reach}


# ------------------------------------------------------------------ not gpu: the reference

@pytest.mark.parametrize("policy", ["sed", "lsq2", "alias"])
@pytest.mark.parametrize("case", HOST_CASES)
def test_every_flow_has_its_acks_once_in_order_and_on_time(case, policy):
    """Every completed flow has had exactly k ACKs over all steps; its last sample equals its fct
    and carries its timestamp; its ages increase strictly; their mean is (t0 - ta) + svc (k + 1) /
    (2 k) to within k us; nothing is recorded before its time or twice."""
    sims = make_sims(case, HOST_B, policy=policy)
    S, kw, m, _ = config_kwargs(case)
    acts = actions_of(case, HOST_B)
    n_done = 0
    for b, sim in enumerate(sims):
        sim.reset()
        for k in range(8):
            sim.step(fr.weights_of(acts[k], kw)[b])
        end = sim.step_no * sim.dt
        for f in sim.flows:
            svc = f.tc - f.t0
            assert f.k == ack_count(svc, sim.ack_us, sim.max_acks) and 1 <= f.k <= min(m, svc)
            times = ack_times(f.t0, svc, sim.ack_us, sim.max_acks)
            due = [t for t in times if t <= end]
            assert [a[0] for a in f.acks] == due, "every ACK due so far, once, nothing early"
            for (t, age, ts), step in zip(f.acks, f.steps):
                assert step * sim.dt < t <= (step + 1) * sim.dt and age == t - f.ta
                assert ts == t // 1000
            ages = [a[1] for a in f.acks]
            assert all(x < y for x, y in zip(ages, ages[1:]))
            if f.tc <= end:
                n_done += 1
                assert len(f.acks) == f.k and f.acks[-1][:2] == (f.tc, f.tc - f.ta)
                want = (f.t0 - f.ta) + svc * (f.k + 1) / (2 * f.k)
                assert abs(sum(ages) / f.k - want) <= f.k
    assert n_done > 5 * HOST_B


def test_what_the_scenarios_reach():
    """A flow with ACKs in three or more steps, a step in which a server in service records none,
    an ACK at exactly dt, k capped by max_acks, k capped by svc, more than 128 duration samples on
    a server: each is met by the reference on the cases the device tests run."""
    fast = reach_of(reference_run(FAST, HOST_B)[3])
    assert fast["steps3"] > 0 and fast["at_dt"] > 0 and fast["cap_max"] > 0, fast
    assert fast["over128"] > 0, fast
    tiny = reach_of(reference_run(TINY, HOST_B)[3])
    assert tiny["cap_svc"] > 0, tiny
    one = reach_of(reference_run("s3-lsq-q8-one-ack", HOST_B)[3])
    assert one["silent_step"] > 0, one  # one ACK per flow: a long service is silent until its end
    assert reach_of(reference_run("s4-alias-q32-m32", HOST_B)[3])["over128"] > 0


@pytest.mark.parametrize("case", ["s1-sed-q8-m1", "s4-sed-q32", "s8-trace"])
def test_one_ack_per_flow_is_the_completion_sample(case):
    """At ack_us = 2^30 every flow has one ACK, at its completion: the duration reservoir's first
    128 records per server equal FlowSim's fct samples and timestamps, in completion order."""
    S, kw, _, _ = config_kwargs(case)
    cfg = make_config(1, S, **kw)
    args = (kw["seed"], cfg.env_id_offset, S, cfg.queue_capacity, kw.get("assign_policy", "sed"),
            cfg.arrival_rate, [cfg.server_rate[s] for s in range(S)])
    opt = dict(dt=cfg.step_interval, warmup_steps=cfg.warmup_steps, trace=kw.get("trace"))
    a, f = AckSim(*args, max_acks=32, ack_us=BIGI, **opt), FlowSim(*args, **opt)
    acts = actions_of(case, 1)
    done = [r for r in f.reset()]
    a.reset()
    for k in range(STEPS):
        w = fr.weights_of(acts[k], kw)[0]
        done.append(f.step(w))
        a.step(w)
    n = 0
    for s in range(S):
        want = [(tc - ta, tc // 1000) for r in done for (sv, ta, tc) in r.completed if sv == s]
        assert a.dur_count[s] == len(want)
        assert a.dur[s][:min(len(want), K)] == want[:K]
        n += len(want)
    assert n > 20


# ------------------------------------------------------------------ not gpu: the helpers

def test_helpers_against_a_brute_force_loop(tmp_path):
    """tests/acks_probe.cpp: k, t_j and the window function of csrc/lbsim_acks.h against loops
    over every j, on random inputs and the extremes (svc = 2^30, ack_us in {1, 2^30}, negative t0
    and a, b = dt), under the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "acks_probe")
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "acks_probe.cpp")],
                   check=True)
    for seed in (1, 2):
        r = subprocess.run([exe, str(seed)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        cases, empty, whole, part, cap_max, cap_svc, at_b = map(int, r.stdout.split())
        assert cases > 400000 and min(empty, whole, part, cap_max, cap_svc, at_b) > 1000


def test_python_rule_equals_the_reference_rule():
    """marllb_amd.acks.ack_count / ack_times: the docstring's rule on a few hand-made flows."""
    assert ack_count(7999, 1000, 8) == 7 and ack_count(8000, 1000, 8) == 8
    assert ack_count(50000, 1000, 8) == 8 and ack_count(3, 1, 8) == 3 and ack_count(1, BIGI, 32) == 1
    assert ack_times(100, 10, 1, 4) == [102, 105, 107, 110]
    assert ack_times(-5, 7, 1, 32) == [-4, -3, -2, -1, 0, 1, 2]
    assert ack_times(0, BIGI, BIGI, 32) == [BIGI]


# ------------------------------------------------------------------ not gpu: the rule and the plan

REFUSALS = [
    ({"lost_fin_prob": 0.1}, {}, "lost_fin_prob > 0"),
    ({"fail_prob": 0.01}, {}, "fail_prob > 0"),
    ({"duration_mode": "service"}, {}, "duration_mode SERVICE"),
    ({"reservoir_mode": "vpp"}, {}, "reservoir_mode VPP"),
    ({"n_flow_on_mode": "vpp"}, {}, "n_flow_on_mode VPP"),
    ({"next_step_reset": True}, {}, "next_step_reset"),
    ({}, {"server_availability": True}, "server availability"),
    ({}, {"cross_traffic": True}, "cross traffic"),
    ({}, {"server_workers": True}, "server workers"),
    ({}, {"action_delay": True}, "action delay"),
    ({}, {"balancers_per_pool": 2}, "server pools"),
    ({}, {"service_discipline": "ps"}, "processor sharing"),
    ({}, {"flow_stats": True}, "flow statistics"),
    ({}, {"workload_tables": True}, "workload tables"),
    ({}, {"trace_bank": True}, "a trace bank"),
    ({}, {"trace_schedule": True}, "a trace schedule"),
]


def test_check_ack_config_and_the_header():
    check_ack_config(make_config(8, 4))
    check_ack_config(make_config(8, 4, assign_policy="alias", normalize_obs=True), max_acks=32)
    for cfg_kw, opts, word in REFUSALS:
        with pytest.raises(_lib.LbsimError) as e:
            check_ack_config(make_config(8, 4, **cfg_kw), **opts)
        assert e.value.code == _lib.ENOTSUP
        assert f"ack samples with {word}: not supported" in str(e.value), word
    for bad in (0, 33, -1):
        with pytest.raises(_lib.LbsimError) as e:
            check_ack_config(make_config(8, 4), max_acks=bad)
        assert e.value.code == _lib.EINVAL
    header = open(os.path.join(ROOT, "include", "lbsim.h")).read()
    for name, nargs in (("lbsim_ack_samples_enable", 2), ("lbsim_ack_samples", 1),
                        ("lbsim_set_ack_interval", 3), ("lbsim_get_ack_interval", 2),
                        ("lbsim_clear_ack_interval", 1)):
        assert f"int {name}(" in header and len(_lib._SIGNATURES[name][1]) == nargs
    assert "LBSIM_DYN_KERNEL_ACK = 6" in header and "#define LBSIM_ABI_VERSION 10 " in header


def test_sample_ack_interval():
    from marllb_amd import sample_ack_interval
    v = sample_ack_interval(4096, 250, 4000, seed=3).numpy()
    assert v.dtype == np.int32 and v.min() >= 250 and v.max() <= 4000
    assert (v == sample_ack_interval(4096, 250, 4000, seed=3).numpy()).all()
    lg = np.log(v.astype(np.float64))  # log-uniform: the mean of the logs is the middle
    assert abs(lg.mean() - (np.log(250) + np.log(4000)) / 2) < 0.05
    assert (sample_ack_interval(5, 7, 7).numpy() == 7).all()
    for lo, hi in ((0, 5), (9, 3), (1, (1 << 30) + 1)):
        with pytest.raises(ValueError):
            sample_ack_interval(4, lo, hi)


PLAN_PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include "marllb_amd/csrc/lbsim_plan.h"
int main(int argc, char** argv) {
  lbk::PlanInput in{};
  in.B = std::atoi(argv[1]), in.S = std::atoi(argv[2]), in.Q = std::atoi(argv[3]);
  in.policy = std::atoi(argv[4]);
  in.dyn_mapping = std::atoi(argv[5]), in.step_kernel = std::atoi(argv[6]), in.simds = 1024;
  in.trace = std::atoi(argv[7]) != 0;
  in.ack_samples = std::atoi(argv[8]) != 0;
  const lbk::StepPlan p = lbk::make_plan(in, lbk::Overrides::from_env());
  std::printf("%d %d %d %d %u %u %d %d %d %d %d %d %d\n", p.form, p.dyn.kernel, p.dyn.width,
              (int)p.dyn.full, p.dyn.grid, p.dyn.block, p.reset_dyn.kernel, p.reset_dyn.width,
              (int)p.reset_dyn.full, p.obs.form, p.reset_obs.form, (int)p.nr, p.dyn.epw);
  return 0;
}
"""


def test_plan_of_an_ack_input(tmp_path):
    """make_plan (csrc/lbsim_plan.h, compiled alone): an ACK input gets the ACK kernel value on
    the full group form for the step and the reset, the two-launch step and the general observe
    (never a paired form), whatever the batch, the mapping or the step kernel asked for; and
    ack_samples = false plans as before."""
    src, exe = tmp_path / "ack_plan_probe.cpp", str(tmp_path / "ack_plan_probe")
    src.write_text(PLAN_PROBE)
    subprocess.run([build.hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", f"-I{ROOT}", "-o",
                    exe, str(src)], check=True)

    def plan(B, S, Q=32, policy=0, mapping=0, step_kernel=0, tr=0, ack=1, env=None):
        e = {k: v for k, v in os.environ.items() if not k.startswith("LBSIM_")}
        e.update(env or {})
        out = subprocess.run([exe] + [str(x) for x in (B, S, Q, policy, mapping, step_kernel, tr,
                                                       ack)],
                             capture_output=True, text=True, check=True, env=e).stdout.split()
        return dict(zip(("form", "kernel", "width", "full", "grid", "block", "rkernel", "rwidth",
                         "rfull", "obs", "robs", "nr", "epw"), map(int, out)))

    TWO_LAUNCH = 2  # kStepTwoLaunch
    PAIRED = (0, 1, 2)  # kObsPair, kObsPair16, kObsPairChunks
    for B in (67, 4096, 65536):
        for S, g in ((1, 2), (2, 2), (3, None), (4, None), (5, 8), (8, 8), (16, 16), (20, 32)):
            for mapping in (0, 1, 2):
                for sk in (0, 1, 2):  # LBSIM_STEP_AUTO / SPLIT / FUSED
                    p = plan(B, S, policy=S % 5, mapping=mapping, step_kernel=sk, tr=S == 8)
                    assert p["form"] == TWO_LAUNCH and p["nr"] == 0, (B, S, p)
                    assert p["kernel"] == p["rkernel"] == ACK_KERNEL
                    assert p["full"] == p["rfull"] == 1 and p["block"] == 64
                    if g is not None:  # (S = 3, 4: 8 lanes at a small batch, else 4)
                        assert p["width"] == p["rwidth"] == g
                    else:
                        assert p["width"] == p["rwidth"] == (8 if B <= 8192 else 4)
                    assert p["grid"] == -(-B // p["epw"]) and p["epw"] == 64 // p["width"]
                    assert p["obs"] not in PAIRED and p["robs"] not in PAIRED
    assert plan(67, 3, env={"LBSIM_DYN_GROUP_LANES": "4"})["width"] == 4
    assert plan(67, 3, env={"LBSIM_DYN_GROUP_LANES": "16"})["width"] == 16
    assert plan(67, 3, env={"LBSIM_DYN_WAVE": "1"})["kernel"] == ACK_KERNEL
    # ack_samples = false: the plans of before
    assert plan(2048, 4, ack=0)["kernel"] == parity.WAVE
    p = plan(65536, 4, ack=0)
    assert p["kernel"] == parity.GROUP and p["full"] == 0 and p["obs"] == 0  # kObsPair
    assert plan(65536, 4, mapping=1, ack=0)["kernel"] == parity.ENV_LANE


# ------------------------------------------------------------------ gpu: against the reference

class Dev:
    """An env and its way of running the scenario's events."""

    def __init__(self, B, S, kw, ack=None, **extra):
        import torch
        from marllb_amd.env import VecLoadBalanceEnv
        self.torch = torch
        extra.setdefault("autoreset", False)
        opts = {} if ack is None else {"ack_samples": True, "max_acks": ack[0],
                                       "ack_interval_us": ack[1]}
        self.env = VecLoadBalanceEnv(B, S, device="cuda:0", **opts, **extra, **kw)

    def reset(self, mask):
        obs = self.env.reset(mask=None if mask is None else
                             self.torch.from_numpy(np.asarray(mask, np.uint8)))
        return obs.cpu().numpy(), None, None

    def step(self, a):
        obs, rew, _, info = self.env.step(self.torch.from_numpy(a), assign_counts=True)
        return obs.cpu().numpy(), rew.cpu().numpy(), info["assign_counts"].cpu().numpy()


def parse_ack(buf, cfg, B=None):
    """An ACK handle's snapshot: a plain handle's sections, then res_dur as {us,
    ts} records and res_count_dur."""
    B = cfg.num_envs if B is None else B
    S, Q = cfg.num_servers, cfg.queue_capacity
    secs = statelayout.sections(B, S, Q, bool(cfg.normalize_obs))
    secs = secs + [("res_dur2", np.uint32, B * S * K * 2), ("res_count_dur", np.uint32, B * S)]
    d, off = {}, 0
    for name, dt, n in secs:
        nb = np.dtype(dt).itemsize * n
        d[name] = np.frombuffer(buf[off:off + nb], dtype=dt)
        off += nb
    assert off == len(buf), (off, len(buf))
    return d


def check_ack_kernel(env, lanes=None):
    names = _lib.launch_names(env.handle)
    assert _lib.load().lbsim_dynamics_kernel(env.handle.h) == ACK_KERNEL, names
    assert names.get(0, "").startswith("dynamics_group_ack_kernel<"), names
    assert _lib.launch_names(env.handle, 1).get(2, "").startswith("dynamics_group_ack_kernel<")
    forced = os.environ.get("LBSIM_DYN_GROUP_LANES")
    if forced and int(forced) >= env.cfg.num_servers:
        assert names[0].startswith(f"dynamics_group_ack_kernel<{forced},"), names
    assert env.handle.ack_samples() == env.max_acks


class AckCheck:
    """After a reset or a step: the ACK handle against the reference's duration reservoirs, against
    a plain twin's everything else, and its columns 6-10 and reward against the oracle's features
    of the reference's records.  All exact."""

    def __init__(self, env, plain, reward=True, normalized=False):
        self.env, self.plain, self.cfg = env, plain, env.cfg
        self.B, self.S = env.cfg.num_envs, env.cfg.num_servers
        self.reward, self.normalized = reward, normalized
        self.compared = {"records": 0, "over128": 0, "differs": 0}

    def __call__(self, ev, out, pout):
        B, S, Q = self.B, self.S, self.cfg.queue_capacity
        obs, rew, assign = out
        pobs, prew, passign = pout
        d = parse_ack(self.env.handle.state_bytes(), self.cfg)
        p = statelayout.parse_cfg(self.plain.handle.state_bytes(), self.plain.cfg)
        # ---- the duration reservoir against the reference
        np.testing.assert_array_equal(d["res_count_dur"].reshape(B, S), ev.count,
                                      err_msg="res_count_dur")
        held = (np.arange(K).reshape(1, 1, K) < np.minimum(ev.count, K)[..., None])[..., None]
        np.testing.assert_array_equal(np.where(held, d["res_dur2"].reshape(B, S, K, 2), 0), ev.rec,
                                      err_msg="duration records and timestamps, slot for slot")
        self.compared["records"] += int(np.minimum(ev.count, K).sum())
        self.compared["over128"] += int((ev.count > K).sum())
        val, ts = ev.rec[..., 0].copy(), ev.rec[..., 1].copy()
        hc = d["hc"].reshape(B, S)
        # (no sample of these scenarios reaches 2^25 - 1 us: neither reservoir sets the flag)
        np.testing.assert_array_equal(((hc >> 15) & 1).astype(bool), ev.big, err_msg="the big flag")
        # written slots: the fct reservoir's (the twin's) and the duration reservoir's
        np.testing.assert_array_equal(d["chg"].reshape(B, S, 4),
                                      p["chg"].reshape(B, S, 4) | ev.chg, err_msg="chg")
        # ---- everything else against the plain twin
        for name in ("next_arr", "next_work", "next_u2", "next_u3", "arr_idx", "episode", "clock",
                     "ep_step", "dropped", "hc", "last_tc", "res_count"):
            np.testing.assert_array_equal(d[name], p[name], err_msg=name)
        np.testing.assert_array_equal(statelayout.live_ring(d, B, S, Q),
                                      statelayout.live_ring(p, B, S, Q), err_msg="rings")
        rc = np.minimum(d["res_count"], K).reshape(B, S, 1)
        live = (np.arange(K).reshape(1, 1, K) < rc)[..., None]
        np.testing.assert_array_equal(np.where(live, d["res"].reshape(B, S, K, 2), 0),
                                      np.where(live, p["res"].reshape(B, S, K, 2), 0),
                                      err_msg="res records")
        if assign is not None:
            np.testing.assert_array_equal(assign, passign, err_msg="assign counts")
            np.testing.assert_array_equal(assign, ev.assigned, err_msg="assign counts (reference)")
        np.testing.assert_array_equal(obs[:, :, :6], pobs[:, :, :6], err_msg="columns 0-5")
        # ---- columns 6-10: the oracle's features of the reference's duration records
        if not self.normalized:
            f = oracle.features(val.view(np.int32).astype(np.float32) * np.float32(1e-6), ts,
                                np.minimum(ev.count, 0xFFFFFFFF).astype(np.uint32))
            np.testing.assert_array_equal(obs[:, :, 6:11], f.reshape(B, S, 5),
                                          err_msg="duration features")
            self.compared["differs"] += int((obs[:, :, 6:11] != obs[:, :, 1:6]).any())
            if rew is not None and self.reward:
                want = oracle.rewards(obs, self.cfg.reward_metric, self.cfg.reward_field)
                np.testing.assert_array_equal(rew, want, err_msg="reward")


def drive(case, B, dev, plain, check, steps=STEPS, **run_kw):
    """The scenario on the ACK handle and its plain twin: check after every reset and step."""
    _, acts, snaps, sims = reference_run(case, B, steps, **run_kw)
    it = iter(snaps)
    check(next(it), dev.reset(None), plain.reset(None))
    for k in range(steps):
        if k == RESET_AT:
            m = (np.arange(B) % 3 == 0).astype(np.uint8)
            check(next(it), dev.reset(m), plain.reset(m))
        check(next(it), dev.step(acts[k]), plain.step(acts[k]))
    return snaps, sims


def pair(case, B, **extra):
    S, kw, m, _ = config_kwargs(case)
    dev = Dev(B, S, kw, ack=(m, intervals_of(case, B)), **extra)
    return dev, Dev(B, S, kw, **extra)


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_enabled_handles_equal_the_reference(lib, case):
    """After every reset and step (the masked reset's envs restart their duration reservoirs from
    count 0): res_count_dur, every res_dur record and timestamp slot for slot, the chg mask and the
    big flag against AckSim; res, res_count, hc, the rings, last_tc, the counters, the assign
    counts and columns 0-5 against a plain handle of the same seed; columns 6-10 and the reward
    against the oracle on the reference's records."""
    dev, plain = pair(case, GPU_B)
    chk = AckCheck(dev.env, plain.env)
    snaps, sims = drive(case, GPU_B, dev, plain, chk)
    check_ack_kernel(dev.env)
    assert not plain.env.handle.ack_samples()
    assert (dev.env.get_ack_interval().cpu().numpy() == intervals_of(case, GPU_B)).all()
    assert chk.compared["records"] > 20 * GPU_B
    if CASES[case][2] > 1 and CASES[case][3] != BIGI:  # (one ACK per flow: its fct)
        assert chk.compared["differs"] > 0
    # the envs of the masked reset restarted from count 0: their counts fell
    before, after = snaps[RESET_AT].count, snaps[RESET_AT + 1].count
    assert (after[::3].sum(1) < before[::3].sum(1)).any()
    if case in (FAST, "s4-alias-q32-m32", MIXED):
        assert chk.compared["over128"] > 0
    r = reach_of(sims)
    if case == FAST:
        assert min(r[k] for k in ("steps3", "at_dt", "cap_max", "over128")) > 0, r
    if case == TINY:
        assert r["cap_svc"] > 0, r
    dev.env.close()
    plain.env.close()


@gpu
def test_forced_four_lane_groups():
    """LBSIM_DYN_GROUP_LANES=4: the 4-lane groups on a case of each S <= 4."""
    ks = [f"test_enabled_handles_equal_the_reference[{c}]"
          for c in ("s1-sed-q8-m1", FAST, "s3-lsq-q8-one-ack", "s4-sed-q32")]
    parity.run_cases_in_child("test_ack_samples.py", ks, {"LBSIM_DYN_GROUP_LANES": "4"})


@gpu
def test_per_env_rates_with_a_rate_schedule(lib):
    """Per-env rates, then a P = 3, H = 2 cyclic rate schedule of arrival and server rates."""
    B, P, H, case = 24, 3, 2, "s4-sed-q32"
    S, kw, m, _ = config_kwargs(case)
    rng = np.random.default_rng(6)
    lams = rng.uniform(40.0, 90.0, B).astype(np.float32)
    mus = rng.uniform(15.0, 40.0, (B, S)).astype(np.float32)
    dev, plain = pair(case, B)
    for e in (dev.env, plain.env):
        e.set_rates(lams, mus)
    drive(case, B, dev, plain, AckCheck(dev.env, plain.env), steps=8, rates=(lams, mus))
    for e in (dev.env, plain.env):
        e.close()
    lam = rng.uniform(40.0, 90.0, (B, P)).astype(np.float32)
    mu = rng.uniform(15.0, 40.0, (B, P, S)).astype(np.float32)
    dev, plain = pair(case, B)
    for e in (dev.env, plain.env):
        e.set_rate_schedule(lam, mu, steps_per_phase=H, wrap=True)
    chk = AckCheck(dev.env, plain.env)
    drive(case, B, dev, plain, chk, schedule=(lam, mu, H, True))
    check_ack_kernel(dev.env)
    assert chk.compared["over128"] > 0
    for e in (dev.env, plain.env):
        e.close()


@gpu
def test_normalize_obs(lib):
    """normalize_obs: the state against the reference, and the normalised columns 0-5 against the
    plain twin's (each column has its own running mean and deviation)."""
    case = "s4-sed-q32"
    S, kw, m, _ = config_kwargs(case)
    kw = {**kw, "normalize_obs": True}
    dev = Dev(24, S, kw, ack=(m, intervals_of(case, 24)))
    plain = Dev(24, S, kw)
    drive(case, 24, dev, plain, AckCheck(dev.env, plain.env, normalized=True), steps=8)
    obs = dev.step(actions_of(case, 24)[0])[0]
    assert np.isfinite(obs).all() and (obs[:, :, 6:11] != obs[:, :, 1:6]).any()
    dev.env.close()
    plain.env.close()


@gpu
def test_same_step_auto_reset(lib):
    """autoreset=True, same_step: an env that ends its episode resets in the same step, and its
    duration reservoirs are the new episode's (count from 0, the warm-up's ACKs in them)."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    B, case = 12, "s4-sed-q32"
    S, kw, m, _ = config_kwargs(case)
    env = VecLoadBalanceEnv(B, S, device="cuda:0", ack_samples=True, max_acks=m, max_steps=3, **kw)
    plain = VecLoadBalanceEnv(B, S, device="cuda:0", max_steps=3, **kw)
    chk = AckCheck(env, plain, reward=False)
    sims = make_sims(case, B)
    for sim in sims:
        sim.reset()
    chk(Snap(sims, mask=np.ones(B, bool)), (env.reset().cpu().numpy(), None, None),
        (plain.reset().cpu().numpy(), None, None))
    acts = actions_of(case, B)
    for k in range(7):
        a = torch.from_numpy(acts[k])
        obs, rew, done, info = env.step(a, assign_counts=True)
        pobs, prew, pdone, pinfo = plain.step(a, assign_counts=True)
        wts = fr.weights_of(acts[k], kw)
        rs = [sim.step(wts[b]) for b, sim in enumerate(sims)]
        ends = k % 3 == 2
        assert bool(done.all()) == ends and bool(done.any()) == ends
        assigned = np.array([r.assigned for r in rs])
        if ends:
            for sim in sims:
                sim.reset()
        chk(Snap(sims, assigned=assigned),
            (obs.cpu().numpy(), None, info["assign_counts"].cpu().numpy()),
            (pobs.cpu().numpy(), None, pinfo["assign_counts"].cpu().numpy()))
    assert chk.compared["records"] > 20 * B
    env.close()
    plain.close()


@gpu
def test_state_round_trip_and_a_plain_snapshot_rejected(lib):
    """lbsim_state_size grows by the two sections; get_state / set_state round-trips into a fresh
    ACK handle, which then steps as the first; a plain handle's snapshot is rejected by size, and
    so is an ACK snapshot by a plain handle.  lbsim_state_save / lbsim_state_load (snapshot /
    restore) carry the two sections per env, as on a lost-FIN handle."""
    case, B = "s4-sed-q32", 24
    S, kw, m, _ = config_kwargs(case)
    dev, plain = pair(case, B)
    n_ack, n_plain = len(dev.env.handle.state_bytes()), len(plain.env.handle.state_bytes())
    assert n_ack == n_plain + B * S * (K * 8 + 4)
    acts = actions_of(case, B)
    for d in (dev, plain):
        d.reset(None)
        for k in range(4):
            d.step(acts[k])
    state = dev.env.get_state()
    twin = Dev(B, S, kw, ack=(m, intervals_of(case, B)))
    twin.env.set_state(state)
    assert twin.env.handle.state_bytes() == state
    for x, y in zip(dev.step(acts[4]), twin.step(acts[4])):
        np.testing.assert_array_equal(x, y)
    assert twin.env.handle.state_bytes() == dev.env.handle.state_bytes()
    with pytest.raises((_lib.LbsimError, ValueError)):
        dev.env.set_state(plain.env.get_state())
    with pytest.raises((_lib.LbsimError, ValueError)):
        plain.env.set_state(state)
    # on-device snapshots: restore brings the duration reservoirs back byte for byte
    snap = dev.env.snapshot()
    before = dev.env.handle.state_bytes()
    dev.step(acts[5])
    assert dev.env.handle.state_bytes() != before
    dev.env.restore(snap)
    assert dev.env.handle.state_bytes() == before
    for e in (dev.env, plain.env, twin.env):
        e.close()


@gpu
def test_shards_at_uneven_sizes(lib):
    """Shards of 9 and 15 envs, each with its own rows of the intervals, equal the 24-env handle's
    rows: outputs, duration records and counts."""
    case, B = MIXED, 24
    S, kw, m, _ = config_kwargs(case)
    us = intervals_of(case, B)
    whole = Dev(B, S, kw, ack=(m, us))
    acts = actions_of(case, B)
    whole.reset(None)
    outs = [whole.step(acts[k]) for k in range(5)]
    dw = parse_ack(whole.env.handle.state_bytes(), whole.env.cfg)
    lo = 0
    for n in (9, 15):
        part = Dev(n, S, {**kw, "env_id_offset": lo}, ack=(m, us[lo:lo + n]))
        part.reset(None)
        for k in range(5):
            for x, y in zip(part.step(acts[k][lo:lo + n]), outs[k]):
                np.testing.assert_array_equal(x, y[lo:lo + n])
        dp = parse_ack(part.env.handle.state_bytes(), part.env.cfg)
        for name, w in (("res_count_dur", S), ("res_dur2", S * K * 2), ("hc", S), ("last_tc", S)):
            np.testing.assert_array_equal(dp[name].reshape(n, w),
                                          dw[name].reshape(B, w)[lo:lo + n], err_msg=name)
        part.env.close()
        lo += n
    whole.env.close()


@gpu
def test_replayed_graph(lib):
    """A captured step, replayed 3 times, equals an eager twin step for step; an interval set
    between replays reaches the replayed kernel."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    case, B = "s4-sed-q32", 24
    S, kw, m, _ = config_kwargs(case)
    opts = dict(device="cuda:0", ack_samples=True, max_acks=m, **kw)
    eager = VecLoadBalanceEnv(B, S, **opts)
    graph = VecLoadBalanceEnv(B, S, graph_mode=True, **opts)
    for e in (eager, graph):
        e.reset()
    acts = [torch.from_numpy(a).to("cuda:0") for a in actions_of(case, B)[:4]]
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
    for k in range(1, 4):
        if k == 3:
            for e in (eager, graph):
                e.set_ack_interval(250)
        a_static.copy_(acts[k])
        cg.replay()
        eo, er, ed, _ = eager.step(acts[k])
        assert torch.equal(obs, eo) and torch.equal(rew, er) and torch.equal(done, ed), k
    assert graph.handle.state_bytes() == eager.handle.state_bytes()
    eager.close()
    graph.close()


@gpu
def test_facades_and_the_interval_calls(lib):
    """LoadBalanceEnv and the multi-agent facades forward the kwargs and the interval calls; the
    interval calls check their range and shape, and an env without the option refuses them."""
    import torch
    from marllb_amd.env import LoadBalanceEnv, VecLoadBalanceEnv
    from marllb_amd.multi_agent import MultiAgentLoadBalanceEnv, VecMultiAgentLoadBalanceEnv
    one = LoadBalanceEnv(num_servers=4, ack_samples=True, max_acks=4, ack_interval_us=500, seed=3)
    assert one._vec.handle.ack_samples() == 4 and one.get_ack_interval() == 500
    one.reset()
    obs = one.step(np.zeros(4, np.int64))[0]
    assert (obs[:, 6:11] != obs[:, 1:6]).any()
    one.set_ack_interval(2000)
    assert one.get_ack_interval() == 2000
    one.clear_ack_interval()
    assert one.get_ack_interval() == 1000
    one.close()
    ma1 = MultiAgentLoadBalanceEnv(num_agents=2, servers_per_agent=2, ack_samples=True)
    ma1.set_ack_interval(300)
    assert ma1.get_ack_interval() == 300
    ma1.close()
    ma = VecMultiAgentLoadBalanceEnv(6, num_agents=2, servers_per_agent=2, ack_samples=True,
                                     max_acks=32)
    assert ma.vec.handle.ack_samples() == 32
    ma.set_ack_interval(np.arange(1, 7) * 100)
    assert ma.get_ack_interval().cpu().tolist() == [100, 200, 300, 400, 500, 600]
    ma.clear_ack_interval()
    ma.reset()
    ma.vec.close()
    env = VecLoadBalanceEnv(8, 4, device="cuda:0", ack_samples=True)
    assert env.handle.ack_samples() == 8 and (env.get_ack_interval() == 1000).all()
    env.handle.enable_ack_samples(8)  # the same value again: a no-op
    for bad in (0, -5, (1 << 30) + 1, 2.5, [100] * 3, float("nan")):
        with pytest.raises(ValueError):
            env.set_ack_interval(bad)
    assert (env.get_ack_interval() == 1000).all()  # the previous intervals stayed in force
    env.set_ack_interval(torch.full((8,), 1 << 30))
    assert (env.get_ack_interval() == 1 << 30).all()
    with pytest.raises(ValueError):
        env.handle.enable_ack_samples(4)  # another value: EINVAL
    env.reset()
    env.close()
    plain = VecLoadBalanceEnv(8, 4, device="cuda:0")
    for call in (lambda: plain.set_ack_interval(5), plain.get_ack_interval,
                 plain.clear_ack_interval):
        with pytest.raises(_lib.LbsimError) as e:
            call()
        assert e.value.code == _lib.ENOTSUP
    us = np.full(8, 5, np.int32)
    assert _lib.load().lbsim_set_ack_interval(plain.handle.h, us.ctypes.data, 8) == _lib.ENOTSUP
    plain.reset()
    with pytest.raises(ValueError):
        plain.handle.enable_ack_samples(8)  # after the reset: EINVAL
    with pytest.raises(_lib.LbsimError):
        VecLoadBalanceEnv(8, 4, device="cuda:0", ack_interval_us=500)
    with pytest.raises(_lib.LbsimError):
        VecLoadBalanceEnv(8, 4, device="cuda:0", ack_samples=True, max_acks=33)
    plain.close()


@gpu
def test_default_handles_launch_what_they_launched(lib):
    """A handle without the option launches the kernels it launched: the names of a default step
    and reset carry no ACK kernel, and the dynamics kernel value is a pre-existing one."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    for B, S, extra, kernel in ((67, 4, {}, parity.WAVE), (67, 4, {"flow_stats": True}, parity.GROUP),
                                (8192, 4, {}, parity.GROUP), (67, 16, {}, parity.GROUP)):
        env = VecLoadBalanceEnv(B, S, device="cuda:0", **extra)
        env.reset()
        env.step(torch.zeros((B, S), dtype=torch.int64))
        names = {**_lib.launch_names(env.handle), **_lib.launch_names(env.handle, 1)}
        assert names and not any("ack" in n for n in names.values()), names
        assert _lib.load().lbsim_dynamics_kernel(env.handle.h) == kernel
        env.close()


# ------------------------------------------------------------------ gpu: the refusals

@gpu
def test_every_refusal_leaves_the_handle_as_it_was(lib):
    """ENOTSUP, the message naming the option, in either order of the two calls where both are
    opt-ins; the handle and lbsim_dynamics_kernel stay as they were."""
    from marllb_amd.env import Handle, VecLoadBalanceEnv
    L = _lib.load()

    def handle(**kw):
        return Handle(make_config(8, 4, **kw), 0)

    def refused(h, fn, word):
        before = L.lbsim_dynamics_kernel(h.h), h.ack_samples(), len(h.state_bytes())
        with pytest.raises(_lib.LbsimError) as e:
            fn()
        assert e.value.code == _lib.ENOTSUP and word in str(e.value), (word, str(e.value))
        assert (L.lbsim_dynamics_kernel(h.h), h.ack_samples(), len(h.state_bytes())) == before

    # the config's options
    for cfg_kw, _, word in REFUSALS[:6]:
        h = handle(**cfg_kw)
        refused(h, lambda: h.enable_ack_samples(8), f"ack samples with {word}")
        h.close()
    # the opt-ins: the other one first, then ack samples first
    optins = [("server availability", lambda h: h.enable_server_avail()),
              ("cross traffic", lambda h: h.enable_cross_traffic()),
              ("server workers", lambda h: h.enable_server_workers()),
              ("action delay", lambda h: h.enable_action_delay(1)),
              ("server pools", lambda h: h.enable_server_pool(2)),
              ("server pools", lambda h: h.enable_server_pool_ps(2)),
              ("processor sharing", lambda h: h.enable_processor_sharing()),
              ("flow statistics", lambda h: h.enable_flow_stats())]
    for word, enable in optins:
        h = handle()
        enable(h)
        refused(h, lambda: h.enable_ack_samples(8), f"ack samples with {word}")
        h.close()
        h = handle()
        h.enable_ack_samples(8)
        assert L.lbsim_dynamics_kernel(h.h) == ACK_KERNEL
        refused(h, lambda: enable(h), word)
        h.close()
    # the constructor states the same rule before any handle exists
    with pytest.raises(_lib.LbsimError) as e:
        VecLoadBalanceEnv(8, 4, device="cuda:0", ack_samples=True, flow_stats=True)
    assert e.value.code == _lib.ENOTSUP and "flow statistics" in str(e.value)
    # workload tables, trace banks and trace schedules
    from marllb_amd import exponential_table
    env = VecLoadBalanceEnv(8, 4, device="cuda:0", ack_samples=True)
    tab = np.stack([exponential_table()])
    refused(env.handle, lambda: env.set_workload_tables(tab, 0, 0), "workload tables")
    env.close()
    tr = trace.synthetic(37, 300.0, seed=7)
    env = VecLoadBalanceEnv(8, 4, device="cuda:0", ack_samples=True, trace=tr)
    refused(env.handle, lambda: env.set_trace_bank([tr, tr]), "a trace bank")
    refused(env.handle, lambda: env.set_trace_schedule(np.zeros(8, np.int32)), "a trace schedule")
    env.reset()
    env.close()
    # lbsim_ground_truth stays available
    env = VecLoadBalanceEnv(8, 4, device="cuda:0", ack_samples=True)
    env.reset()
    assert tuple(env.ground_truth().shape)[:2] == (8, 4)
    env.close()


# ------------------------------------------------------------------ gpu: the columns' meaning

@gpu
def test_duration_columns_differ_from_fct_and_rank_the_overloaded_server_last(lib):
    """512 x 4 at weights [2, 1, 1, 1] against all 1.0, as test_default_reward_sees_the_policy
    (the default config, 40 steps): the duration columns now differ from the fct columns -- at
    the default 1000 us interval every flow of 2 ms of service or more, 78 % of them at a mean of
    8 ms, offers ages below its fct, so more than half of the entries must differ -- and they
    still rank the overloaded server last: server 0 has the largest flow_duration_avg_decay, and
    the skewed weights lower the mean reward.  The reward on column 10 differs from the plain
    handle's and equals the metric of the new columns."""
    import torch
    from marllb_amd.env import VecLoadBalanceEnv
    B, S = 512, 4
    out = {}
    for name, row, ack in (("fair", [0, 0, 0, 0], True), ("skew", [2, 0, 0, 0], True),
                           ("plain", [2, 0, 0, 0], False)):
        env = VecLoadBalanceEnv(B, S, device="cuda:0", seed=7, autoreset=False, ack_samples=ack)
        env.reset()
        a = torch.tensor(row, dtype=torch.int64).repeat(B, 1)
        acc, col = [], []
        for k in range(40):
            obs, rew, _, _ = env.step(a)
            if k >= 20:
                acc.append(rew.double().mean().item())
                col.append(obs[:, :, 10].double().mean(0).cpu().numpy())
        out[name] = (obs.cpu().numpy(), rew.cpu().numpy(), float(np.mean(acc)), np.mean(col, 0))
        cfg = env.cfg
        env.close()
    obs, rew, mean_skew, col = out["skew"]
    print("differing entries", (obs[:, :, 6:11] != obs[:, :, 1:6]).mean(), "rewards fair / skew /"
          " plain skew", out["fair"][2], mean_skew, out["plain"][2], "column 10", col)
    assert (obs[:, :, 6:11] != obs[:, :, 1:6]).mean() > 0.5
    np.testing.assert_array_equal(obs[:, :, :6], out["plain"][0][:, :, :6])
    assert (rew != out["plain"][1]).mean() > 0.5
    np.testing.assert_array_equal(rew, oracle.rewards(obs, cfg.reward_metric, cfg.reward_field))
    assert col.argmax() == 0, col
    assert out["fair"][2] > mean_skew, (out["fair"][2], mean_skew)
