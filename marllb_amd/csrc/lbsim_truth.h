// lbsim_truth.h — ground-truth server state: what the simulator knows about a
// server between two launches and the observation does not show -- every flow in the system, the
// hidden ones, the busy workers, the wait an arrival would face, the time to drain, whether the
// server is up, its capacity.  The rule as plain __host__ __device__ functions over a queue
// accessor, as lbsim_workers.h states its own (tests/truth_probe.cpp compiles them as host C++
// with no HIP header, on a plain array standing for the ring); ground_truth_kernel
// (lbsim_api.hip) evaluates it with one lane per (env, server).
//
// Between launches the whole queue lives in the HBM ring, sorted by t_complete (FIFO order on a
// handle without server workers is that order too), times relative to the start of the next step:
// "now" is 0.  A queue accessor A gives the entries by their position from the head:
// A::get(pos) -> an entry whose .x is t_complete.
#pragma once
#include <cstdint>

#include "lbsim_workers.h"

namespace lbk {

constexpr int kTruthCols = 8;  // LBSIM_TRUTH_COLS
// the columns of a row
constexpr int kTruthTotal = 0;     // flows in the system, hidden ones and flows in service included
constexpr int kTruthHidden = 1;    // of them, hidden cross-traffic flows
constexpr int kTruthBusy = 2;      // busy workers, min(n, c)
constexpr int kTruthCpu = 3;       // busy / c
constexpr int kTruthWait = 4;      // seconds until a worker is free for a flow arriving now
constexpr int kTruthBacklog = 5;   // seconds until the server drains with no further arrival
constexpr int kTruthUp = 6;        // 0 while the server is down, else 1
constexpr int kTruthCapacity = 7;  // c * mu, flows/s at the rate of the env's next step

// DevState::hc = ring head | the sticky big flag (bit 15) | count << 16
LBW_HD int truth_head(uint32_t hc) { return (int)(hc & 0x7FFFu); }
LBW_HD int truth_count(uint32_t hc) { return (int)(hc >> 16); }

// us_to_seconds: the conversion of every time the simulator reports
LBW_HD float truth_seconds(int32_t us) { return (float)us * 1e-6f; }

// The queue positions the rule reads: the entry whose completion frees a worker for an arrival
// (n - c; -1: a worker is free) and the last entry, the largest completion time (n - 1; -1: the
// queue is empty).  With c = 1 they are the same position.
LBW_HD int truth_wait_pos(int n, int c) { return n < c ? -1 : n - c; }
LBW_HD int truth_backlog_pos(int n) { return n - 1; }

// The wait of a flow arriving now, in us: workers_start at ta = 0.
template <class A>
LBW_HD int32_t truth_wait_us(const A& q, int n, int c) {
  return workers_start(q, n, c, 0);
}

// The time until the last queued flow completes, in us.
template <class A>
LBW_HD int32_t truth_backlog_us(const A& q, int n) {
  if (n == 0) return 0;
  const int32_t t = q.get(truth_backlog_pos(n)).x;
  return t > 0 ? t : 0;
}

// One row.  hc: the server's ring word; c: its worker count (1 on a handle without server
// workers); lost: the lost_on word of a cross-traffic handle (minus the hidden flows queued), 0 on
// any other handle; down: the server's down flag (false on a handle without one); mu: the rate of
// one worker in flows/s.  Every operation is an exact conversion or one correctly rounded f32
// operation.  At most two entries are read, one when c = 1, none from an empty queue.
template <class A>
LBW_HD void truth_row(const A& q, uint32_t hc, int32_t c, int32_t lost, bool down, float mu,
                      float (&out)[kTruthCols]) {
  const int n = truth_count(hc);
  const int busy = n < c ? n : c;
  int32_t wait = 0, backlog = 0;
  if (n > 0) {
    backlog = q.get(truth_backlog_pos(n)).x;
    const int pw = truth_wait_pos(n, c);
    wait = pw < 0 ? 0 : (pw == truth_backlog_pos(n) ? backlog : q.get(pw).x);
    backlog = backlog > 0 ? backlog : 0;
    wait = wait > 0 ? wait : 0;
  }
  out[kTruthTotal] = (float)n;
  out[kTruthHidden] = (float)(-lost);
  out[kTruthBusy] = (float)busy;
  out[kTruthCpu] = (float)busy / (float)c;
  out[kTruthWait] = truth_seconds(wait);
  out[kTruthBacklog] = truth_seconds(backlog);
  out[kTruthUp] = down ? 0.0f : 1.0f;
  out[kTruthCapacity] = (float)c * mu;
}

}  // namespace lbk
