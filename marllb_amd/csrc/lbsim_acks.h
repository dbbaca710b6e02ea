// lbsim_acks.h — duration samples at every data ACK: where the ACKs of a flow
// fall, as plain __host__ __device__ functions (tests/acks_probe.cpp compiles them as host C++
// with no HIP header), as lbsim_ps.h does.
//
// All quantities are integer us relative to the step start.  A flow that starts service at t0 and
// needs svc >= 1 us completes at tc = t0 + svc and emits k = min(max_acks, max(1, svc / ack_us))
// ACKs, ACK j = 1..k at t_j = t0 + (svc j) / k: k <= svc, so the times increase strictly, and
// t_k = tc.  Products are taken in 64 bits (svc <= 2^30, k <= 32).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LBACK_HD __host__ __device__ inline
#else
#define LBACK_HD inline
#endif

namespace lbk {

constexpr int32_t kAckMaxAcks = 32;            // max_acks in [1, 32]
constexpr int32_t kAckMaxInterval = 1 << 30;   // ack_us in [1, 2^30]
constexpr int32_t kAckDefaultMax = 8;
constexpr int32_t kAckDefaultInterval = 1000;

// The ACK dynamics kernel's argument: the envs' ACK intervals [B] in us (a null pointer: the
// handle has no ACK samples) and the handle's max_acks.
struct AckSamples {
  const int32_t* us;
  int32_t max_acks;
};

LBACK_HD bool ack_max_ok(int32_t max_acks) { return max_acks >= 1 && max_acks <= kAckMaxAcks; }
LBACK_HD bool ack_interval_ok(int32_t us) { return us >= 1 && us <= kAckMaxInterval; }

// k: the ACKs of a flow of svc us of service.
LBACK_HD int32_t ack_count(int32_t svc, int32_t ack_us, int32_t max_acks) {
  int32_t k = svc / ack_us;
  k = k < 1 ? 1 : k;
  return k < max_acks ? k : max_acks;
}

// t_j, j in [1, k].
LBACK_HD int32_t ack_time(int32_t t0, int32_t svc, int32_t k, int32_t j) {
  return (int32_t)((int64_t)t0 + ((int64_t)svc * (int64_t)j) / (int64_t)k);
}

// The ACKs with t_j <= t: how many of the k (0 .. k).  t_j <= t is (svc j) / k <= t - t0, which is
// svc j < k (t - t0 + 1): j <= ceil(k (t - t0 + 1) / svc) - 1.
LBACK_HD int32_t ack_done_by(int32_t t0, int32_t svc, int32_t k, int32_t t) {
  const int64_t d = (int64_t)t - (int64_t)t0 + 1;
  if (d <= 0) return 0;
  const int64_t n = ((int64_t)k * d + (int64_t)svc - 1) / (int64_t)svc - 1;
  return n >= (int64_t)k ? k : (int32_t)n;
}

// The ACKs of a flow in (a, b], a <= b: j in [jlo, jhi], none when jlo > jhi.  No loop over the
// k ACKs: a window that holds none costs two divisions.
LBACK_HD void ack_window(int32_t t0, int32_t svc, int32_t k, int32_t a, int32_t b, int32_t& jlo,
                         int32_t& jhi) {
  jlo = ack_done_by(t0, svc, k, a) + 1;
  jhi = ack_done_by(t0, svc, k, b);
}

}  // namespace lbk
