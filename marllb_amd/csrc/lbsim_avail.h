// lbsim_avail.h — scripted server availability (lbsim_set_server_avail).
//
// One kernel, avail_apply_kernel, runs in front of the first launch of every step of a handle
// with lbsim_server_avail_enable: one thread per (env, server) compares the bit the table wants
// at the env's phase with DevState::down and applies the difference to the state as it is.
//
//   up -> down   §3.9's failure, word for word the oracle's branch: the queued flows count as
//                dropped, hc = head (count 0, no big flag), last_tc = none, res_count = 0,
//                lost_on = 0 where the handle has it, a split handle's res_count_dur and pend_hc
//                0, reservoir_mode VPP's bins (and the duration plane) zeroed, down = 1 -- and
//                the server's ten cached features 0: the dynamics launch that follows clears
//                chg at its start, so the observe behind it reuses fcache for this server.
//   down -> up   down = 0 and nothing else.
//
// The dynamics kernels are untouched: they honour down behind their null test, and draw no random
// failure because such a handle has fail_thr = 0.  The same kernel pointed at outputs answers
// lbsim_get_server_avail (apply = 0: nothing of the state is written).
//
// Plain vector stores; dropped[b] takes one integer atomic add per failing server with queued
// flows (order-independent, so results stay bit-reproducible).  Nothing is read by one thread
// that another thread of the launch writes, except dropped[b] through that atomic.
//
// avail_server is the whole per-(env, server) body as a host-and-device function over a struct of
// section pointers: tests/avail_probe.cpp runs it thread by thread on the host, with guard bytes
// around every array.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LBSIM_AVAIL_HD __host__ __device__
#else
#define LBSIM_AVAIL_HD
#endif

namespace lbk {

constexpr int kAvailK = 128;                     // reservoir slots per server (K)
constexpr int kAvailFeat = 10;                   // cached features per server (fcache)
constexpr uint32_t kAvailHcHead = (1u << 15) - 1u;  // hc: ring head below the big flag (kHcHead)
constexpr int32_t kAvailLastNone = -(1 << 30);   // last_tc of a server that popped nothing
constexpr int kAvailMaxPhases = 4096;

// The sections the transition touches, and the handle's shape.
struct AvailState {
  const int32_t* ep_step;   // [B]
  uint32_t* hc;             // [B*S]
  int32_t* last_tc;         // [B*S]
  uint32_t* res_count;      // [B*S]
  uint32_t* res;            // [B*S*K] records of two words
  float* fcache;            // [B*S*10]
  uint32_t* down;           // [B*S]
  uint32_t* lost_on;        // [B*S] or nullptr
  uint32_t* res_dur;        // [B*S*K] words (split: records of two words) or nullptr
  uint32_t* res_count_dur;  // [B*S], split handles only
  uint32_t* pend_hc;        // [B*S], split handles only
  int32_t B, S;
  int32_t split, res_vpp;
  int32_t max_steps, next_reset;
};

// The table in force: up[B, P, S] bytes, nonzero = up (nullptr: every server up), each phase held
// for H steps, cyclic or clamped.
struct AvailTable {
  const uint8_t* up;
  int32_t P, H, wrap;
};

// lbsim_get_server_avail's outputs, each optional.
struct AvailOut {
  uint8_t* want;    // [B, S]: 1 where the next step launch wants the server up
  uint8_t* up_now;  // [B, S]: 1 where the server is up now
  int32_t* phase;   // [B]
};

// The phase at episode step k (k / H, cyclic or clamped): lbsim_set_rate_schedule's rule, that
// marllb_amd.randomize.schedule_phase states on the host.  P >= 1, H >= 1.
LBSIM_AVAIL_HD inline uint32_t avail_phase(int32_t k, uint32_t P, uint32_t H, bool wrap) {
  const uint32_t j = (uint32_t)(k > 0 ? k : 0) / H;
  return wrap ? j % P : (j < P ? j : P - 1u);
}

// Thread i of the launch, i < B * S: server i - b * S of env b = i / S.  Returns the flows the
// server lost (to be added to dropped[b] by the caller; 0 unless apply and the server fails).
// An env whose next step launch resets it instead (next-step auto-reset, ep_step >= max_steps) is
// left alone: the reset brings every server up, and its next step runs at phase 0.
LBSIM_AVAIL_HD inline uint32_t avail_server(const AvailState& a, const AvailTable& t,
                                            const AvailOut& o, int apply, int64_t i) {
  const int64_t b = i / a.S;
  const int32_t s = (int32_t)(i - b * a.S);
  const int32_t k = a.ep_step[b];
  const bool resets = a.next_reset != 0 && k >= a.max_steps;
  uint32_t phase = 0u;
  if (t.P > 1 && !resets) phase = avail_phase(k, (uint32_t)t.P, (uint32_t)t.H, t.wrap != 0);
  bool want_up = true;
  if (t.up != nullptr && !resets)
    want_up = t.up[((size_t)b * (size_t)t.P + phase) * (size_t)a.S + (size_t)s] != 0;
  const bool is_down = a.down[i] != 0u;
  if (o.want != nullptr) o.want[i] = want_up ? 1 : 0;
  if (o.up_now != nullptr) o.up_now[i] = is_down ? 0 : 1;
  if (o.phase != nullptr && s == 0) o.phase[b] = (int32_t)phase;
  if (!apply || resets || want_up != is_down) return 0u;
  if (want_up) {  // down -> up
    a.down[i] = 0u;
    return 0u;
  }
  // up -> down
  const uint32_t hc = a.hc[i];
  a.hc[i] = hc & kAvailHcHead;
  a.last_tc[i] = kAvailLastNone;
  a.res_count[i] = 0u;
  if (a.lost_on != nullptr) a.lost_on[i] = 0u;
  if (a.split) {
    a.res_count_dur[i] = 0u;
    a.pend_hc[i] = 0u;
  }
  if (a.res_vpp) {
    uint32_t* r = a.res + (size_t)i * (kAvailK * 2);
    for (int w = 0; w < kAvailK * 2; ++w) r[w] = 0u;
    if (a.res_dur != nullptr) {
      const int n = a.split ? kAvailK * 2 : kAvailK;
      uint32_t* d = a.res_dur + (size_t)i * (size_t)n;
      for (int w = 0; w < n; ++w) d[w] = 0u;
    }
  }
  float* f = a.fcache + (size_t)i * kAvailFeat;
  for (int w = 0; w < kAvailFeat; ++w) f[w] = 0.0f;
  a.down[i] = 1u;
  return hc >> 16;
}

#if defined(__HIPCC__)
__global__ void __launch_bounds__(256)
    avail_apply_kernel(AvailState a, AvailTable t, AvailOut o, int apply, uint32_t* dropped) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)a.B * a.S) return;
  const uint32_t lost = avail_server(a, t, o, apply, i);
  if (lost != 0u) atomicAdd(dropped + i / a.S, lost);
}

// A caller's table to the handle's: out[b, phase, s] = in[b * row_stride + phase * S + s] != 0
// (row stride 0: one shared table), n = B * P * S bytes.
__global__ void __launch_bounds__(256)
    avail_table_kernel(const uint8_t* in, int64_t row_stride, int64_t per_env, int64_t n,
                       uint8_t* out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t b = i / per_env;
  out[i] = in[b * row_stride + (i - b * per_env)] != 0 ? 1 : 0;
}
#endif

}  // namespace lbk
