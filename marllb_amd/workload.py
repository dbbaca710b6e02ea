"""Workload tables: arrival-gap and flow-size distributions as on-device quantile tables
(VecLoadBalanceEnv.set_workload_tables, lbsim_set_workload_tables).

A table is TABLE_BINS f32 quantile levels of a mean-1 distribution, indexed by the raw 32-bit
Philox word v an arrival already draws; small v is the tail, the orientation -ln u has:

    bin(v) = v                                   for v < 32
           = 32 (e - 4) + ((v >> (e - 5)) & 31)  with e = floor(log2 v), otherwise

Bins 0..31 hold one word each, bin k >= 32 holds 2^(k // 32 - 1): a staircase of 32 levels per
octave of tail probability, down to 2^-32.  The device looks a level up and nothing else (no
interpolation), so this module states the whole rule: csrc/lbsim_table.h is the same function.

numpy only, float64 inside, f32 tables out.
"""
import math

import numpy as np

TABLE_BINS = 896  # LBSIM_TABLE_BINS


def table_bin(v):
    """The bin of Philox word(s) v (an int or an array of uint32 values) -- csrc/lbsim_table.h."""
    a = np.asarray(v, dtype=np.uint64)
    if np.any(a >> np.uint64(32)):
        raise ValueError("table_bin: words are 32-bit")
    # floor(log2 v) without floating point: the position of the highest set bit
    e = np.zeros(a.shape, np.int64)
    for s in (16, 8, 4, 2, 1):
        e = np.where((a >> (e + s).astype(np.uint64)) > 0, e + s, e)
    shift = np.maximum(e - 5, 0).astype(np.uint64)
    k = 32 * (e - 4) + ((a >> shift) & np.uint64(31)).astype(np.int64)
    out = np.where(a < 32, a.astype(np.int64), k)
    return int(out) if np.ndim(v) == 0 else out


def bin_edges() -> np.ndarray:
    """(TABLE_BINS + 1,) uint64: the first word of each bin; the last entry is 2^32."""
    k = np.arange(TABLE_BINS + 1, dtype=np.uint64)
    octave = np.maximum(k // np.uint64(32), np.uint64(1)) - np.uint64(1)
    body = (np.uint64(32) + (k & np.uint64(31))) << octave
    return np.where(k < 32, k, body)


def bin_mass() -> np.ndarray:
    """(TABLE_BINS,) uint64: the Philox words of each bin (probability * 2^32); sums to 2^32."""
    e = bin_edges()
    return e[1:] - e[:-1]


def table_mean(t) -> float:
    """The mass-weighted mean of a table: the mean of the distribution the device draws."""
    t = np.asarray(t, np.float64)
    return float(np.sum(t * bin_mass().astype(np.float64)) / 2.0 ** 32)


def table_cv2(t) -> float:
    """The squared coefficient of variation of the distribution the device draws."""
    t = np.asarray(t, np.float64)
    m = table_mean(t)
    m2 = float(np.sum(t * t * bin_mass().astype(np.float64)) / 2.0 ** 32)
    return m2 / (m * m) - 1.0


_QUAD = 64  # midpoint rule points per bin (bins of fewer words: one point per word)


def quantile_table(ppf) -> np.ndarray:
    """The f32 table of a distribution given by its quantile function ppf (vectorised, on
    [0, 1]): entry k is the mean of ppf(1 - v / 2^32) over the words v of bin k, by midpoint
    quadrature in f64 (word v stands for the probability interval (v, v + 1) / 2^32: its
    midpoint), and the whole table is then scaled so that its mass-weighted mean is 1 -- a
    server rate mu and an arrival rate lambda keep their meaning."""
    edges = bin_edges().astype(np.float64)
    t = np.empty(TABLE_BINS, np.float64)
    for k in range(TABLE_BINS):
        lo, hi = edges[k], edges[k + 1]
        n = int(min(_QUAD, hi - lo))
        x = lo + (np.arange(n, dtype=np.float64) + 0.5) * ((hi - lo) / n)
        t[k] = float(np.mean(np.asarray(ppf(1.0 - x / 2.0 ** 32), np.float64)))
    if not np.all(np.isfinite(t)) or np.any(t < 0.0):
        raise ValueError("quantile_table: ppf must be finite and >= 0 on (0, 1)")
    m = float(np.sum(t * bin_mass().astype(np.float64)) / 2.0 ** 32)
    if not m > 0.0:
        raise ValueError("quantile_table: the distribution's mean must be > 0")
    return (t / m).astype(np.float32)


def exponential_table() -> np.ndarray:
    """Exp(1): the law of the closed form, as a staircase."""
    return quantile_table(lambda q: -np.log1p(-q))


def bounded_pareto_table(alpha: float = 1.5, bound: float = 1000.0) -> np.ndarray:
    """Bounded Pareto of shape alpha on [x_min, bound * x_min], scaled to mean 1: the law of
    trace.synthetic(work="pareto")."""
    if not (alpha > 0.0 and bound > 1.0):
        raise ValueError(f"pareto: need alpha > 0 and bound > 1 (got {alpha}, {bound})")
    a, c = float(alpha), 1.0 - float(bound) ** -float(alpha)
    return quantile_table(lambda q: (1.0 - q * c) ** (-1.0 / a))


def _norm_ppf(q):
    """The standard normal quantile (Acklam's rational approximation, then one Halley step
    against math.erfc: ~1e-15 relative)."""
    q = np.asarray(q, np.float64)
    a = [-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02,
         1.383577518672690e+02, -3.066479806614716e+01, 2.506628277459239e+00]
    b = [-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02,
         6.680131188771972e+01, -1.328068155288572e+01]
    c = [-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00,
         -2.549732539343734e+00, 4.374664141464968e+00, 2.938163982698783e+00]
    d = [7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00,
         3.754408661907416e+00]
    x = np.empty_like(q)
    lo, hi = q < 0.02425, q > 1.0 - 0.02425
    mid = ~(lo | hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.sqrt(-2.0 * np.log(np.where(lo, q, 1.0)))
        x = np.where(lo, (((((c[0] * r + c[1]) * r + c[2]) * r + c[3]) * r + c[4]) * r + c[5]) /
                     ((((d[0] * r + d[1]) * r + d[2]) * r + d[3]) * r + 1.0), x)
        r = np.sqrt(-2.0 * np.log(np.where(hi, 1.0 - q, 1.0)))
        x = np.where(hi, -(((((c[0] * r + c[1]) * r + c[2]) * r + c[3]) * r + c[4]) * r + c[5]) /
                     ((((d[0] * r + d[1]) * r + d[2]) * r + d[3]) * r + 1.0), x)
        s = np.where(mid, q - 0.5, 0.0)
        r = s * s
        num = (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * s
        x = np.where(mid, num / (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1.0), x)
    erfc = np.vectorize(math.erfc, otypes=[np.float64])
    e = 0.5 * erfc(-x / math.sqrt(2.0)) - q
    u = e * math.sqrt(2.0 * math.pi) * np.exp(x * x / 2.0)
    return x - u / (1.0 + x * u / 2.0)


def lognormal_table(sigma: float = 1.0) -> np.ndarray:
    """Lognormal with log-standard-deviation sigma, scaled to mean 1."""
    if not sigma > 0.0:
        raise ValueError(f"lognormal: need sigma > 0 (got {sigma})")
    return quantile_table(lambda q: np.exp(float(sigma) * _norm_ppf(q)))


def hyperexp_table(cv2: float = 8.0) -> np.ndarray:
    """Two-phase hyperexponential with balanced means and squared coefficient of variation
    cv2 >= 1 (cv2 = 1: Exp(1)): bursty gaps, or a mix of mice and elephants."""
    if not cv2 >= 1.0:
        raise ValueError(f"hyperexp: need cv2 >= 1 (got {cv2})")
    p1 = 0.5 * (1.0 + math.sqrt((cv2 - 1.0) / (cv2 + 1.0)))
    p2 = 1.0 - p1
    r1, r2 = 2.0 * p1, 2.0 * p2  # rates: each phase carries half the mean

    def ppf(q):
        # the survival function p1 exp(-r1 x) + p2 exp(-r2 x) = 1 - q, solved by bisection on x
        s = 1.0 - np.asarray(q, np.float64)
        lo = np.zeros_like(s)
        hi = np.full_like(s, 64.0 / min(r1, r2))
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            big = p1 * np.exp(-r1 * mid) + p2 * np.exp(-r2 * mid) > s
            lo = np.where(big, mid, lo)
            hi = np.where(big, hi, mid)
        return 0.5 * (lo + hi)
    return quantile_table(ppf)


def weibull_table(shape: float = 0.5) -> np.ndarray:
    """Weibull of the given shape (< 1: heavy-tailed, 1: Exp(1), > 1: lighter), scaled to mean 1."""
    if not shape > 0.0:
        raise ValueError(f"weibull: need shape > 0 (got {shape})")
    return quantile_table(lambda q: (-np.log1p(-q)) ** (1.0 / float(shape)))


def constant_table() -> np.ndarray:
    """Every draw is 1: deterministic gaps (a D/./1 queue) or equal-sized flows."""
    return np.ones(TABLE_BINS, np.float32)


def empirical_table(samples) -> np.ndarray:
    """The empirical distribution of `samples` (>= 0, for example trace.builtin().work): its
    quantile function is the order statistic x_(ceil(q n)), scaled to mean 1."""
    x = np.sort(np.asarray(samples, np.float64).ravel())
    if x.size == 0 or not np.all(np.isfinite(x)) or x[0] < 0.0:
        raise ValueError("empirical_table: samples must be finite, >= 0 and not empty")
    n = x.size

    def ppf(q):
        i = np.ceil(np.asarray(q, np.float64) * n).astype(np.int64) - 1
        return x[np.clip(i, 0, n - 1)]
    return quantile_table(ppf)


def sample_table_ids(B: int, choices, generator=None) -> np.ndarray:
    """(B,) int32 table ids drawn uniformly from `choices` (a sequence of ids of the bank): the
    per-env gap_id or work_id of VecLoadBalanceEnv.set_workload_tables.  generator: a
    numpy.random.Generator or a seed."""
    c = np.asarray(choices, np.int64).ravel()
    if c.size == 0 or np.any(c < 0):
        raise ValueError("sample_table_ids: choices must be ids >= 0, at least one")
    rng = generator
    if not isinstance(rng, np.random.Generator):
        rng = np.random.default_rng(generator)
    return c[rng.integers(0, c.size, size=int(B))].astype(np.int32)
