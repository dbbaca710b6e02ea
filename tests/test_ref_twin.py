"""The reference's own C reservoir twin (simulation-mode/problem-01-reservoir-sampling/src/
reservoir.h, compiled where it lies by oracle/ref_build.py into oracle/_ref/, CPU) against our
oracle -- test infrastructure checking test infrastructure.

* Algorithm R (reservoir.h:118-143): the twin's reservoir after every add equals a replay of the
  oracle's rule (count < K -> slot count, else slot j = draw mod (count + 1), kept if j < K) fed
  with the twin's own xorshift128+ draws (reservoir.h:80-106), predicted here.  The oracle
  applies the same rule to a Philox draw, so only the draw differs.
* Statistics (reservoir.h:179-268) vs the oracle's, which follows the Python reference
  (reservoir.py:105-196, pinned by tests/golden): mean, mean_decay and p90_decay agree within
  float32 summation-order tolerance; p90 differs by design -- the C twin takes the nearest index
  sorted[(int)(0.9f n)], the Python reference and the oracle numpy's linear interpolation -- so the
  twin's p90 is checked against that index of the sorted values.

The twin's answers on these inputs are recorded in tests/golden/ref_twin.npz (gen_ref_twin.py), so
the checks run wherever the suite runs; where the build compiled the twin it is also run again and
must answer what is recorded.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_ref_twin as rec  # noqa: E402  (drives the twin; shared with the recorder)

K = rec.K
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def gold(golden_dir):
    """tests/golden/ref_twin.npz: the twin's answers on this module's inputs (gen_ref_twin.py)."""
    return np.load(os.path.join(golden_dir, "ref_twin.npz"))


@pytest.fixture(scope="module")
def twin():
    """The twin itself where the build compiled it (the reference tree was present), else None:
    the tests then check the recorded answers alone."""
    return rec.load_twin() if os.path.exists(rec.LIB) else None


def twin_answers(twin, recorded, run):
    """The twin's answers for one case: recorded ones, and where the twin is built also what it
    answers now, which must be what is recorded."""
    if twin is not None:
        live = run(twin)
        for a, b in zip(live, recorded):
            np.testing.assert_array_equal(a, b)
    return recorded


def xorshift_state(seed):  # reservoir.h:55-74 reservoir_init
    if seed == 0:
        return [0x123456789ABCDEF0, 0xFEDCBA9876543210]
    return [seed & M64, (seed ^ M64) & M64]


def xorshift128plus(st):  # reservoir.h:80-89
    x, y = st[0], st[1]
    st[0] = y
    x = (x ^ (x << 23)) & M64
    st[1] = x ^ y ^ (x >> 17) ^ (y >> 26)
    return (st[1] + y) & M64


def algorithm_r_slot(count, draw):
    """The oracle's rule (oracle/lbsim_oracle.c reservoir_add, reservoir.py:64-85) given a draw
    in [0, count] for a full reservoir; -1 = not stored."""
    if count < K:
        return count
    return draw if draw < K else -1


@pytest.mark.parametrize("seed", [0, 1, 20260109])
def test_algorithm_r_rule_matches_the_c_twin(twin, gold, seed):
    vals = gold[f"algr_vals_{seed}"]
    t_accepted, t_count, t_final = twin_answers(
        twin, [gold[f"algr_accepted_{seed}"], gold[f"algr_count_{seed}"],
               gold[f"algr_final_{seed}"]], lambda lib: rec.run_algr(lib, seed, vals))
    assert len(vals) == 3000
    st = xorshift_state(seed)
    mine = np.zeros(K, np.float32)
    stored = 0
    for i, v in enumerate(vals):
        draw = xorshift128plus(st) % (i + 1) if i >= K else 0  # random_range(count + 1)
        slot = algorithm_r_slot(i, draw)
        assert bool(t_accepted[i]) == (slot >= 0), f"add {i}"
        if slot >= 0:
            mine[slot] = v
            stored += 1
        assert t_count[i] == i + 1
    np.testing.assert_array_equal(t_final, mine)
    assert K < stored < len(vals)


def test_algorithm_r_inclusion_probability_twin_and_oracle(twin, gold, oracle_mod):
    """Each of N items ends in the reservoir with probability K/N under both RNGs (the twin's
    xorshift128+ and the oracle's Philox Algorithm R draw, oracle_algr_slot)."""
    N, trials = rec.INCL_N, rec.INCL_TRIALS
    assert (N, trials) == (512, 300)
    lib = oracle_mod.load()
    key = np.array([20260109, 0], np.uint32)
    (hits_t,) = twin_answers(twin, [gold["incl_hits"]], lambda t: [rec.run_inclusion(t)])
    assert hits_t.shape == (N,) and hits_t.sum() == trials * K
    hits_o = np.zeros(N)
    for t in range(trials):
        res = np.arange(K)
        for c in range(K, N):
            s = lib.oracle_algr_slot(c, t, 1, 0, oracle_mod.ptr(key))
            if s >= 0:
                res[s] = c
        hits_o[res] += 1
    p = K / N
    sd = np.sqrt(trials * p * (1 - p))
    for hits in (hits_t, hits_o):
        z = (hits - trials * p) / sd
        assert abs(z.mean()) < 0.2 and z.std() < 1.3, (z.mean(), z.std())


def test_statistics_c_twin_vs_oracle(twin, gold, oracle_mod):
    now_ms = rec.STAT_NOW_MS
    assert int(gold["stat_cases"]) == 18
    for case in range(18):
        v, age_ms = gold[f"stat_v_{case}"], gold[f"stat_age_{case}"]
        n = len(v)
        ts_ms = (now_ms - age_ms).astype(np.uint32)
        (c_out,) = twin_answers(twin, [gold[f"stat_out_{case}"]],
                                lambda lib: [rec.run_stats(lib, v, age_ms)])
        vv = np.zeros(K, np.float32)
        vv[:n] = v
        tt = np.zeros(K, np.uint32)
        tt[:n] = ts_ms
        o = oracle_mod.features(vv, tt, np.array([n], np.uint32))[0]
        mean, p90, std, md, p90d = c_out
        np.testing.assert_allclose(mean, o[0], rtol=2e-6)           # sequential vs pairwise f32
        np.testing.assert_allclose(std, o[2], rtol=2e-3, atol=1e-6)  # one-pass vs two-pass
        np.testing.assert_allclose(md, o[3], rtol=2e-5)              # f32 vs f64 weighted mean
        srt = np.sort(v)
        assert p90 == srt[min(int(np.float32(0.9) * np.float32(n)), n - 1)]  # nearest index
        if n > 1 and srt[0] != srt[-1]:
            lo = int(np.floor(np.float32(n - 1) * np.float32(0.9)))
            assert srt[lo] <= o[1] <= srt[min(lo + 1, n - 1)]  # the oracle interpolates
        # p90_decay: same crossing unless a cumulative weight sits at the 90% cut within float32
        # rounding of it (the C twin sums float32 sequentially, the oracle in exact fixed point)
        w = np.exp(np.log(np.float32(0.9)) * (age_ms / 1000.0))
        order = np.argsort(v, kind="stable")
        cs = np.cumsum(w[order])
        if np.min(np.abs(cs - 0.9 * cs[-1])) > 1e-4 * cs[-1]:
            assert p90d == o[4]
