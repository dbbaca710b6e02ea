// lbsim_delay.h — action latency: the weights derived from an action come into
// force delay_us after the start of the step they were passed to.  The rule -- the whole steps m
// and the remainder r of a delay, which weight rows a launch reads and writes, and what a row
// before the episode's first step holds -- as plain __host__ __device__ functions
// (tests/delay_probe.cpp compiles them as host C++ with no HIP header), and, under hipcc, the
// kernels that convert and validate a caller's delays and gather the ring's rows for a snapshot.
//
// W(j) is the f32 weight row of the action passed to the step with ep_step = j of the current
// episode, W(j < 0) = 1.0 on every server (the warm-up's weights).  With k = ep_step as the
// dynamics launch reads it, an arrival at ta (us from the step's start) is assigned under
// W(k - m) if ta >= r and under W(k - m - 1) if ta < r.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LBD_HD __host__ __device__ inline
#else
#define LBD_HD inline
#endif

namespace lbk {

constexpr int32_t kMaxDelaySteps = 8;

// The arrays of an action-delay handle (null pointers: the handle has none).  An argument of
// dynamics_group_full_kernel beside FlowStats, CrossTraffic and ServerWorkers, not a part of
// DevState (§3.11).  wring[B, R, S] f32: row j % R of env b holds W(j); delay_us[B].
struct ActionDelay {
  float* wring;
  const uint32_t* delay_us;
  int32_t R;  // rows per env: max_delay_steps + 2
};

LBD_HD bool delay_steps_ok(int32_t M) { return M >= 1 && M <= kMaxDelaySteps; }
LBD_HD int32_t delay_rows(int32_t M) { return M + 2; }
// The largest valid delay: M whole steps.
LBD_HD uint32_t delay_max_us(int32_t M, int32_t dt) { return (uint32_t)M * (uint32_t)dt; }
LBD_HD bool delay_us_ok(uint32_t d, int32_t M, int32_t dt) { return d <= delay_max_us(M, dt); }

// Seconds -> us: rint of the f64 product (round half to even, the default mode); false for a NaN,
// a negative value or one above M * dt (out: 0).
LBD_HD bool delay_convert(float delay_s, int32_t M, int32_t dt, uint32_t& out) {
  out = 0u;
  const double us = __builtin_rint((double)delay_s * 1e6);
  if (!(delay_s >= 0.0f) || us > (double)delay_max_us(M, dt)) return false;  // (NaN: the first)
  out = (uint32_t)us;
  return true;
}

LBD_HD int32_t delay_whole(uint32_t d, int32_t dt) { return (int32_t)(d / (uint32_t)dt); }  // m
LBD_HD int32_t delay_rem(uint32_t d, int32_t dt) { return (int32_t)(d % (uint32_t)dt); }    // r

// The step whose row is in force from ta = r on (new) and the one before it (old: ta < r), for a
// launch that reads ep_step = k.  Negative: the row of ones.
LBD_HD int32_t delay_step_new(int32_t k, int32_t m) { return k - m; }
LBD_HD int32_t delay_step_old(int32_t k, int32_t m) { return k - m - 1; }
LBD_HD bool delay_is_ones(int32_t j) { return j < 0; }
// The ring row of step j >= 0.  The launch of step k writes row k % R and reads steps k - m and
// k - m - 1, m <= M = R - 2: R consecutive steps k - M - 1 .. k have distinct rows, so the write
// never lands on a row the same launch reads.
LBD_HD int32_t delay_row(int32_t j, int32_t R) { return j % R; }

#if defined(__HIPCC__) && defined(LBSIM_DELAY_KERNELS)
// (lbsim_api.hip alone defines LBSIM_DELAY_KERNELS: a __global__ belongs to one object)
// lbsim_set_action_delay: out[b] from src[rows] seconds (rows 1: the one value for every env; src
// nullptr: every delay 0), one thread per env.  Offenders are counted into *bad, as
// workers_convert_kernel counts its, and stored as 0.
__global__ void __launch_bounds__(256)
    delay_convert_kernel(const float* src, int rows, int32_t B, int32_t M, int32_t dt,
                         uint32_t* out, uint32_t* bad) {
  const int32_t b = (int32_t)(blockIdx.x * 256u + threadIdx.x);
  uint32_t off = 0u;
  if (b < B) {
    uint32_t d = 0u;
    if (src != nullptr) off = delay_convert(src[rows == 1 ? 0 : b], M, dt, d) ? 0u : 1u;
    out[b] = d;
  }
  for (int d = 32; d > 0; d >>= 1) off += __shfl_xor(off, d, 64);
  if ((threadIdx.x & 63) == 0 && off != 0u) atomicAdd(bad, off);
}

// lbsim_action_delay_save / _load (the ring beside a §3.13 snapshot): word i of env b's row of
// `row` words.  save (dir 0): ring row b -> buffer row b where mask[b] != 0 (mask nullptr: every
// env); load (dir 1): buffer row src_env[b] -> ring row b where 0 <= src_env[b] < B (src_env
// nullptr: row b).  One thread per word, plain loads and stores; a load reads the buffer only and
// a save the ring only, so nothing is read that the launch writes.
__global__ void __launch_bounds__(256)
    delay_gather_kernel(float* ring, float* buf, const uint8_t* mask, const int32_t* src_env,
                        int dir, int32_t B, int32_t row) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * row) return;
  const int32_t b = (int32_t)(i / row);
  const int32_t w = (int32_t)(i - (int64_t)b * row);
  if (dir == 0) {
    if (mask != nullptr && mask[b] == 0) return;
    buf[i] = ring[i];
  } else {
    const int32_t s = src_env != nullptr ? src_env[b] : b;
    if (s < 0 || s >= B) return;
    ring[i] = buf[(int64_t)s * row + w];
  }
}
#endif

}  // namespace lbk
