// lbsim_ps.h — processor-sharing servers: one worker per server, shared
// equally by the n flows queued on it; with per-server core counts (§3.23), c cores shared by the
// flows beyond c.  The rule -- the virtual clock's advance, the next
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

// ---- servers with c cores: with n <= c flows every flow has a core to itself,
// above c the c cores are shared, each flow served at rate c / n.  The same clock words; the carry
// counts core-us: in [0, n) between events, in [0, c) just after a completion.  c = 1 is the rule
// above, bit for bit (each overload hands c == 1 to the function above).
//
// Widths.  c * (t - t_last) can reach 64 dt, beyond 32 bits for a step of a minute, so the advance
// never forms it: with t - t_last = qd n + rd it adds c qd to V and divides acc + c rd, which is
// below (c + 1) n <= 65 Q, a second time.  Every word of the advance is a 32-bit one.  The next
// completion forms (tag_head - V) n - acc in 64 bits, as the function above does, and divides in 32
// wherever the value fits (it does for every config §3.15 accepts: svc Q <= 2^30).

// advance(s, t) of a server with c cores.
LBPS_HD void ps_advance(PsClock& k, int n, int c, int32_t t) {
  if (c == 1) return ps_advance(k, n, t);
  if (n > c) {
    const uint32_t d = (uint32_t)(t - k.t_last), un = (uint32_t)n;
    const uint32_t qd = d / un, rd = d - qd * un;
    const uint32_t a = (uint32_t)k.acc + (uint32_t)c * rd;  // < n + c n
    const uint32_t q = a / un;
    k.V += (int32_t)((uint32_t)c * qd + q);  // <= t - t_last: c < n
    k.acc = (int32_t)(a - q * un);
  } else {
    if (n > 0) k.V += t - k.t_last;
    k.acc = 0;
  }
  k.t_last = t;
}

// The next completion of a server with c cores and n > 0 entries: the smallest tc >= t_last at
// which the advance brings V to tag_head, saturated as above, and the carry rem that advance leaves
// there: 0 with n <= c, else c (tc - t_last) + acc - (tag_head - V) n, in [0, c).
struct PsDue {
  int32_t tc, rem;
};
LBPS_HD PsDue ps_next_completion(const PsClock& k, int n, int c, int32_t tag_head) {
  if (c == 1) return PsDue{ps_next_completion(k, n, tag_head), 0};
  int64_t t = (int64_t)k.t_last;
  int32_t rem = 0;
  if (n <= c) {
    t += (int64_t)(tag_head - k.V);
  } else {
    const int64_t x = (int64_t)(tag_head - k.V) * (int64_t)n - (int64_t)k.acc;
    if (x <= 0) {  // an equal tag behind a completion at t_last: the carry stays
      rem = k.acc;
    } else {
      uint64_t q;
      uint32_t r;
      if (x <= (int64_t)0xFFFFFFFF) {
        const uint32_t q32 = (uint32_t)x / (uint32_t)c;
        r = (uint32_t)x - q32 * (uint32_t)c;
        q = q32;
      } else {
        q = (uint64_t)x / (uint64_t)c;
        r = (uint32_t)((uint64_t)x - q * (uint64_t)c);
      }
      if (r != 0u) {
        q += 1u;
        rem = c - (int32_t)r;
      }
      t += (int64_t)q;
    }
  }
  return PsDue{t > (int64_t)0x7FFFFFFF ? (int32_t)0x7FFFFFFF : (int32_t)t, rem};
}

// The completion at due = ps_next_completion(k, n, c, tag_head), not saturated: what
// ps_advance(k, n, c, due.tc) gives, without the divisions.
LBPS_HD void ps_complete(PsClock& k, const PsDue& due, int32_t tag_head) {
  k.V = tag_head;
  k.acc = due.rem;
  k.t_last = due.tc;
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

// A server's privileged view between two launches (lbsim_ps_server_state; V = 0, t_last = 0, the
// entries hold the remaining tags): work_us = the unfinished work sum(tag) - (n > c ? acc : 0) in
// us of one core, drain_us = the time until the server is empty with no further arrival, the last
// completion time the rule itself gives popping the entries one by one.  Both saturate at 2^31 - 1.
template <class A>
LBPS_HD void ps_server_state(const A& q, int n, int c, int32_t acc, int32_t& work_us,
                             int32_t& drain_us) {
  PsClock k{0, acc, 0};
  int64_t work = n > c ? -(int64_t)acc : 0;
  for (int i = 0; i < n; ++i) {
    const int32_t tag = q.get(i).x;
    work += (int64_t)tag;
    ps_complete(k, ps_next_completion(k, n - i, c, tag), tag);
  }
  work_us = work > (int64_t)0x7FFFFFFF ? (int32_t)0x7FFFFFFF : (int32_t)work;
  drain_us = k.t_last;
}

// The ring index of queue position pos: head < Q, pos < Q.
LBPS_HD int ps_ring_index(int head, int pos, int Q) {
  const int r = head + pos;
  return r >= Q ? r - Q : r;
}

}  // namespace lbk
