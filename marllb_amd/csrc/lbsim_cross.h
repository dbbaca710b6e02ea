// lbsim_cross.h — hidden cross traffic: flows on the servers that the agent's
// balancer did not forward and cannot see.  The rule -- the 24-bit share threshold, the 24-bit
// cumulative weight edges, the per-arrival hash and the hidden flow's server -- as plain
// __host__ __device__ functions (tests/cross_probe.cpp compiles them as host C++ with no HIP
// header), and, under hipcc, the kernel that converts and validates a caller's shares and weights.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LBX_HD __host__ __device__ inline
#else
#define LBX_HD inline
#endif

namespace lbk {

constexpr uint32_t kCrossOne = 1u << 24;  // share 1: every arrival hidden
// t_arrival of a hidden flow's queue entry: its flag (a real relative arrival time is within
// 2^30 us of the step start; the rebase leaves the flag alone)
constexpr int32_t kHiddenTa = INT32_MIN;

// The arrays of a cross-traffic handle: thr[B] and cum[B*S] (nullptr: the handle has none).  An
// argument of dynamics_group_full_kernel beside FlowStats, not a part of DevState (§3.11).
struct CrossTraffic {
  uint32_t* thr;
  uint32_t* cum;
};

// murmur3's fmix32 (lf_mix of lbsim_kernels.h)
LBX_HD uint32_t cross_mix(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// share in [0, 1] (NaN: no)
LBX_HD bool cross_share_ok(float share) { return share >= 0.0f && share <= 1.0f; }
// thr = rint(share * 2^24): an arrival is hidden iff the top 24 bits of its hash are below it
LBX_HD uint32_t cross_thr(float share) { return (uint32_t)rint((double)share * 16777216.0); }

// The edges of S weights w[0], w[stride], ...: cum[s] = floor(2^24 c_s / c_{S-1}) with c the
// sequential f64 prefix sum of the f32 weights (the scaling by 2^24 is exact: one division, rounded
// once), cum[S-1] = 2^24.  False (cum unspecified) unless every weight is finite and >= 0 and
// their sum > 0.
LBX_HD bool cross_edges(const float* w, int64_t stride, int S, uint32_t* cum) {
  double total = 0.0;
  bool ok = true;
  for (int s = 0; s < S; ++s) {
    const float x = w[s * stride];
    ok = ok && x >= 0.0f && x <= 3.4028234663852886e38f;  // finite, >= 0 (NaN: no)
    total += (double)x;
  }
  if (!ok || !(total > 0.0)) return false;
  double c = 0.0;
  for (int s = 0; s < S; ++s) {
    c += (double)w[s * stride];
    cum[s] = (uint32_t)floor(c * 16777216.0 / total);
  }
  cum[S - 1] = kCrossOne;
  return true;
}
// Uniform weights: c_s = s + 1.
LBX_HD void cross_edges_uniform(int S, uint32_t* cum) {
  for (int s = 0; s < S; ++s) cum[s] = (uint32_t)floor((double)(s + 1) * 16777216.0 / (double)S);
  cum[S - 1] = kCrossOne;
}

// The episode's salt (the lost-FIN hash's), the hash of its arrival k, the decision and the word
// that picks the hidden flow's server: a pure function of (seed, global env id, episode, arrival
// index), not of the arrival's Philox words.
LBX_HD uint32_t cross_salt(uint32_t key0, uint32_t key1, uint32_t gid, uint32_t episode) {
  return cross_mix(cross_mix(key0 ^ (episode * 0x9E3779B9u)) ^ gid ^ (key1 * 0x85EBCA6Bu));
}
LBX_HD uint32_t cross_hash(uint32_t k, uint32_t salt) { return cross_mix(k ^ salt ^ 0x3C6EF372u); }
LBX_HD bool cross_hidden(uint32_t h, uint32_t thr) { return (h >> 8) < thr; }
LBX_HD uint32_t cross_pick_word(uint32_t h) { return cross_mix(h ^ 0x6A09E667u) >> 8; }
// The server: the number of edges at or below the word (< S, as cum[S-1] = 2^24 is above every
// 24-bit word).  The kernel counts them with one ballot, lane s holding cum[s].
LBX_HD int cross_pick(const uint32_t* cum, int S, uint32_t x) {
  int n = 0;
  for (int s = 0; s < S; ++s) n += cum[s] <= x ? 1 : 0;
  return n;
}

#if defined(__HIPCC__) && defined(LBSIM_CROSS_KERNELS)
// (lbsim_api.hip alone defines LBSIM_CROSS_KERNELS: a __global__ belongs to one object)
// lbsim_set_cross_traffic: row b of share[rows] / weight[rows, S] (strides 0: the one row for
// every env; weight nullptr: uniform) into thr_out[b] and cum_out[b, :], one thread per env.  Offenders
// (a share outside [0, 1] or NaN; a row of weights with a negative or non-finite entry or no
// positive sum) are counted into *bad, as rate_table_kernel counts its.
__global__ void __launch_bounds__(256)
    cross_convert_kernel(const float* share, int64_t share_stride, const float* weight,
                         int64_t weight_stride, int B, int S, uint32_t* thr_out, uint32_t* cum_out,
                         uint32_t* bad) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t off = 0u;
  if (b < (int64_t)B) {
    const float sh = share != nullptr ? share[b * share_stride] : 0.0f;  // (enable: share 0)
    off += cross_share_ok(sh) ? 0u : 1u;
    thr_out[b] = cross_share_ok(sh) ? cross_thr(sh) : 0u;
    uint32_t* const cum = cum_out + b * S;
    if (weight == nullptr) cross_edges_uniform(S, cum);
    else off += cross_edges(weight + b * weight_stride, 1, S, cum) ? 0u : 1u;
  }
  for (int d = 32; d > 0; d >>= 1) off += __shfl_xor(off, d, 64);
  if ((threadIdx.x & 63) == 0 && off != 0u) atomicAdd(bad, off);
}
#endif

}  // namespace lbk
