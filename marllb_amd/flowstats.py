"""The two rules of the exact flow statistics on the host, in numpy.

The device accumulates, per (env, server), a log-binned histogram of the true flow completion
times in integer microseconds (lbsim_flow_stats_enable) and reads quantiles off it
(lbsim_flow_stats_quantiles).  This module states the same bin rule and the same quantile rule
with integers only, for callers that post-process histograms (merging shards, pooling envs) and
as the restatement the tests hold the kernels to.
"""
from __future__ import annotations

import numpy as np

NBINS = 192  # LBSIM_FLOW_STATS_BINS
CLAMP_US = (1 << 26) - 1  # values at or above 2^26 us (67 s) land in the last, open-ended bin
PPM = 1_000_000


def bin_of(us) -> np.ndarray:
    """Bin of a completion time in us (array or scalar): v = min(us, 2^26 - 1); v itself below 8,
    else with e = floor(log2 v): 8 (e - 2) + ((v >> (e - 3)) & 7)."""
    v = np.minimum(np.asarray(us, dtype=np.int64), CLAMP_US)
    if (v < 0).any():
        raise ValueError("completion times are non-negative")
    w = np.maximum(v, 8)
    e = np.zeros(w.shape, np.int64)  # floor(log2 w), by integer shifts
    for sh in (16, 8, 4, 2, 1):
        m = (w >> (e + sh)) > 0
        e = e + np.where(m, sh, 0)
    return np.where(v < 8, v, 8 * (e - 2) + ((w >> (e - 3)) & 7))


def bin_lower_us() -> np.ndarray:
    """(NBINS + 1,) int64: the lower edge of every bin, and 2^26 (where the clamp sits) as the
    entry after the last.  Bins 0..7 are 1 us wide; bin k >= 8 starts at (8 + k % 8) << (k // 8 - 1)
    and is at most 1/8 of that wide."""
    k = np.arange(NBINS + 1, dtype=np.int64)
    return np.where(k < 8, k, (8 + k % 8) << np.maximum(k // 8 - 1, 0))


def quantile_us(hist, max_us, q_ppm) -> np.ndarray:
    """Quantiles of histogram rows: hist (..., NBINS), max_us (...), q_ppm (nq,) integers in parts
    per million (clamped to [1, 10^6]) -> (..., nq) int64 us.  Per row with n samples: rank
    r = max(1, ceil(q_ppm n / 10^6)), k the first bin whose cumulative count reaches r, result
    min(lower(k + 1) - 1, max_us); max_us for k = 191; 0 for n = 0.  The result is at or above the
    exact nearest-rank quantile and less than 1/8 above it (exact at q = 1 and below 8 us).
    An env's row is the sum of its servers' histograms with the maximum of their max_us."""
    h = np.asarray(hist).astype(np.uint64)
    if h.shape[-1] != NBINS:
        raise ValueError(f"hist needs {NBINS} bins on its last axis")
    mx = np.asarray(max_us).astype(np.int64)
    q = np.clip(np.atleast_1d(np.asarray(q_ppm)).astype(np.int64), 1, PPM)
    cum = np.cumsum(h, axis=-1, dtype=np.uint64)
    n = cum[..., -1]
    lower = bin_lower_us()
    out = np.zeros(h.shape[:-1] + (len(q),), np.int64)
    for i, qi in enumerate(q.tolist()):
        r = np.maximum((np.uint64(qi) * n + np.uint64(PPM - 1)) // np.uint64(PPM), np.uint64(1))
        k = (cum < r[..., None]).sum(axis=-1)  # the first bin at or past the rank
        k = np.minimum(k, NBINS - 1)
        hi = np.where(k == NBINS - 1, mx, lower[k + 1] - 1)
        out[..., i] = np.where(n == 0, 0, np.minimum(hi, mx))
    return out
