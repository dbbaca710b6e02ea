// lbsim_workers.h — multi-worker servers: a server with c identical workers
// behind one FCFS queue.  The rule -- the valid range, where a queue position lives (the LDS
// window or the HBM ring), the start time of an arrival and the sorted insert of its entry -- as
// plain __host__ __device__ functions over a queue accessor (tests/workers_probe.cpp compiles them
// as host C++ with no HIP header, on a plain array standing for window plus ring), and, under
// hipcc, the kernel that converts and validates a caller's counts.
//
// A queue accessor A gives the entries by their position from the head, 0 = the earliest
// completion:  A::get(pos) -> an entry whose .x is t_complete and .y t_arrival,  A::set(pos, e).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LBW_HD __host__ __device__ inline
#else
#define LBW_HD inline
#endif

namespace lbk {

constexpr int32_t kMaxWorkers = 64;

// The array of a server-workers handle: c[B*S] (nullptr: the handle has none).  An argument of
// dynamics_group_full_kernel beside FlowStats and CrossTraffic, not a part of DevState (§3.11).
struct ServerWorkers {
  const int32_t* c;
};

LBW_HD bool workers_ok(int32_t c) { return c >= 1 && c <= kMaxWorkers; }

// Queue position pos (from the head) of a server whose window of WL slots (a power of two) starts
// at slot lh and whose ring of Q entries starts at head: positions below WL are window slots, the
// others ring entries.
LBW_HD bool workers_in_window(int pos, int WL) { return pos < WL; }
LBW_HD int workers_win_slot(int lh, int pos, int WL) { return (lh + pos) & (WL - 1); }
LBW_HD int workers_ring_index(int head, int pos, int Q) {  // head < Q, pos < Q
  const int r = head + pos;
  return r >= Q ? r - Q : r;
}

// Start of an arrival at ta on a server of c workers holding n queued flows (sorted by t_complete,
// the pops due by ta done): a free worker if n < c, else when the entry at position n - c
// completes -- the c queued flows with the latest completions hold the workers.
template <class A>
LBW_HD int32_t workers_start(const A& q, int n, int c, int32_t ta) {
  if (n < c) return ta;
  const int32_t t = q.get(n - c).x;
  return t > ta ? t : ta;
}

// The sorted insert of entry e into the n queued ones: after every entry with an equal or smaller
// t_complete, entries with a larger one moved one position up, from the tail.  e.x exceeds the
// start, which is at least the t_complete at position n - c, so at most c - 1 entries move.
// Returns the position e took.
template <class A, class E>
LBW_HD int workers_insert(const A& q, int n, const E& e) {
  int at = n;
  while (at > 0) {
    const E prev = q.get(at - 1);
    if (prev.x <= e.x) break;
    q.set(at, prev);
    --at;
  }
  q.set(at, e);
  return at;
}

#if defined(__HIPCC__) && defined(LBSIM_WORKERS_KERNELS)
// (lbsim_api.hip alone defines LBSIM_WORKERS_KERNELS: a __global__ belongs to one object)
// lbsim_set_server_workers: element i of out[B*S] from src[rows, S] (rows 1: the one row for
// every env; src nullptr: every count 1), one thread per element.  Offenders (a count outside
// [1, kMaxWorkers]) are counted into *bad, as rate_table_kernel counts its, and stored as 1.
__global__ void __launch_bounds__(256)
    workers_convert_kernel(const int32_t* src, int rows, int64_t n, int S, int32_t* out,
                           uint32_t* bad) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t off = 0u;
  if (i < n) {
    const int32_t c = src == nullptr ? 1 : src[rows == 1 ? i % S : i];
    off = workers_ok(c) ? 0u : 1u;
    out[i] = workers_ok(c) ? c : 1;
  }
  for (int d = 32; d > 0; d >>= 1) off += __shfl_xor(off, d, 64);
  if ((threadIdx.x & 63) == 0 && off != 0u) atomicAdd(bad, off);
}
#endif

}  // namespace lbk
