// lbsim_ps.h — processor-sharing servers: one worker per server, shared
// equally by the n flows queued on it.  The rule -- the virtual clock's advance, the next
// completion of a server and the sorted insert of an arrival's entry -- as plain
// __host__ __device__ functions over a queue accessor (tests/ps_probe.cpp compiles them as host
// C++ with no HIP header, on a plain array standing for the ring), as lbsim_workers.h does.
//
// All quantities are integer us.  A server keeps a virtual clock V (the service every queued
// flow has received since the step began), a carry acc in [0, n) of us not yet turned into
// virtual time, the time t_last of its last update, and its n entries {tag, ta} in
// non-decreasing tag order: a flow that arrives needing svc us of service gets tag = V + svc and
// completes when V reaches its tag.
//
// A queue accessor A gives the entries by their position from the head, 0 = the smallest tag:
//   A::get(pos) -> an entry whose .x is the tag and .y t_arrival,  A::set(pos, e).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LBPS_HD __host__ __device__ inline
#else
#define LBPS_HD inline
#endif

namespace lbk {

// A server's clock words.
struct PsClock {
  int32_t V, acc, t_last;
};

// advance(s, t): the t - t_last us since the last update are shared by the n queued flows, the
// remainder of the division carried in acc; an empty server carries nothing.
LBPS_HD void ps_advance(PsClock& c, int n, int32_t t) {
  if (n > 0) {
    const uint32_t a = (uint32_t)(c.acc + (t - c.t_last));  // < n + dt
    const uint32_t q = a / (uint32_t)n;
    c.V += (int32_t)q;
    c.acc = (int32_t)(a - q * (uint32_t)n);
  } else {
    c.acc = 0;
  }
  c.t_last = t;
}

// The next completion of a server with n > 0 entries, the head's tag tag_head: the smallest t at
// which ps_advance brings V to tag_head (there acc is 0).  In 64 bits, then saturated: a time
// beyond the int32 range is later than every step end it is compared with.
LBPS_HD int32_t ps_next_completion(const PsClock& c, int n, int32_t tag_head) {
  const int64_t t = (int64_t)c.t_last + (int64_t)(tag_head - c.V) * (int64_t)n - (int64_t)c.acc;
  return t > (int64_t)0x7FFFFFFF ? (int32_t)0x7FFFFFFF : (int32_t)t;
}

// The completion at tc = ps_next_completion: what ps_advance(c, n, tc) gives, without the division.
LBPS_HD void ps_complete(PsClock& c, int32_t tc, int32_t tag_head) {
  c.V = tag_head;
  c.acc = 0;
  c.t_last = tc;
}

// The sorted insert of entry e into the n queued ones: after every entry with an equal or smaller
// tag, entries with a larger one moved one position up, from the tail.  Returns the position e
// took (0: the new head).
template <class A, class E>
LBPS_HD int ps_insert(const A& q, int n, const E& e) {
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

// Step end, after ps_advance(c, n, dt): stored tags become tag - V, the remaining service, and
// arrival times relative to the next step's start; then V = 0, t_last = 0, acc kept.
template <class A>
LBPS_HD void ps_rebase(const A& q, int n, PsClock& c, int32_t dt) {
  for (int i = 0; i < n; ++i) {
    auto e = q.get(i);
    e.x -= c.V;
    e.y -= dt;
    q.set(i, e);
  }
  c.V = 0;
  c.t_last = 0;
}

// The ring index of queue position pos: head < Q, pos < Q.
LBPS_HD int ps_ring_index(int head, int pos, int Q) {
  const int r = head + pos;
  return r >= Q ? r - Q : r;
}

}  // namespace lbk
