// workers_probe — the multi-worker rule of marllb_amd/csrc/lbsim_workers.h as host C++, for
// tests/test_server_workers.py (built there with -fsanitize=address,undefined and run as a
// program).  `workers_probe <seed>` drives, for every c in 1..64 and Q in {3, 8, 9, 32, 64}, a
// random run of arrivals and pops on one server whose queue is laid out as the kernel's: a window
// of 8 slots that starts at slot lh (queue positions 0..7) and a ring of Q entries that starts at
// head (positions 8..), the slot a pop frees taking position 8's entry.  After every operation the
// queue read back through the accessor must equal a naive model: explicit per-worker free times
// (earliest-free worker, ties to the lowest index) for the start, and a stable sort by t_complete
// for the order.  Prints one line per (c, Q):
//   <c> <Q> <pushes> <out-of-order inserts> <largest shift> <ring reads for the start>
// and exits 1 at the first mismatch.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../marllb_amd/csrc/lbsim_workers.h"

namespace {

constexpr int WL = 8;

struct Entry {
  int32_t x, y;  // t_complete, t_arrival
};

struct Rng {  // xorshift64*
  uint64_t s;
  uint32_t next() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
  }
  int below(int n) { return (int)(next() % (uint32_t)n); }
};

// window plus ring as plain arrays, read and written by queue position
struct PlainQueue {
  Entry* win;   // [WL]
  Entry* ring;  // [Q]
  int lh, head, Q;
  int* sets;    // entries written
  int* ring_gets;
  Entry get(int pos) const {
    if (lbk::workers_in_window(pos, WL)) return win[lbk::workers_win_slot(lh, pos, WL)];
    ++*ring_gets;
    return ring[lbk::workers_ring_index(head, pos, Q)];
  }
  void set(int pos, const Entry& e) const {
    ++*sets;
    if (lbk::workers_in_window(pos, WL)) win[lbk::workers_win_slot(lh, pos, WL)] = e;
    else ring[lbk::workers_ring_index(head, pos, Q)] = e;
  }
};

int fail(const char* what, int c, int Q, int step) {
  std::printf("MISMATCH %s: c %d Q %d step %d\n", what, c, Q, step);
  return 1;
}

int run(int c, int Q, uint64_t seed) {
  Rng rng{seed * 0x9E3779B97F4A7C15ull + (uint64_t)(c * 131 + Q) + 1u};
  std::vector<Entry> win((size_t)WL), ring((size_t)Q);
  int lh = rng.below(WL), head = rng.below(Q), cnt = 0;
  std::vector<Entry> model;           // the queue, sorted by x, stable
  std::vector<int32_t> free_at((size_t)c, 0);
  int32_t now = 0;
  int pushes = 0, ooo = 0, max_shift = 0, ring_starts = 0;
  // mean service c x the mean gap x load: queues of every depth up to Q
  const int gap = 1000, svc_mean = (int)(gap * c * (0.7 + 0.1 * (double)rng.below(7)));
  for (int step = 0; step < 4000; ++step) {
    now += 1 + rng.below(2 * gap);
    // the pops due by the arrival
    while (cnt > 0 && win[(size_t)lh].x <= now) {
      if (model.empty() || model[0].x != win[(size_t)lh].x || model[0].y != win[(size_t)lh].y)
        return fail("pop", c, Q, step);
      model.erase(model.begin());
      if (cnt > WL) win[(size_t)lh] = ring[(size_t)lbk::workers_ring_index(head, WL, Q)];
      lh = (lh + 1) & (WL - 1);
      head = head + 1 == Q ? 0 : head + 1;
      --cnt;
    }
    if (cnt == Q) continue;  // full: dropped
    int sets = 0, ring_gets = 0;
    const PlainQueue q{win.data(), ring.data(), lh, head, Q, &sets, &ring_gets};
    const int32_t start = lbk::workers_start(q, cnt, c, now);
    ring_starts += ring_gets;
    // the model's start: the earliest-free worker, ties to the lowest index
    int w = 0;
    for (int i = 1; i < c; ++i) w = free_at[(size_t)i] < free_at[(size_t)w] ? i : w;
    const int32_t want = std::max(now, free_at[(size_t)w]);
    if (start != want) return fail("start", c, Q, step);
    const int32_t svc = 1 + (rng.below(4) == 0 ? rng.below(8 * svc_mean) : rng.below(svc_mean));
    const Entry e{start + svc, now};
    free_at[(size_t)w] = e.x;
    const int at = lbk::workers_insert(q, cnt, e);
    model.push_back(e);
    std::stable_sort(model.begin(), model.end(),
                     [](const Entry& a, const Entry& b) { return a.x < b.x; });
    ++cnt;
    ++pushes;
    const int shift = cnt - 1 - at;
    if (shift != sets - 1) return fail("moves", c, Q, step);
    if (shift > c - 1) return fail("shift above c - 1", c, Q, step);
    ooo += shift > 0;
    max_shift = std::max(max_shift, shift);
    if ((int)model.size() != cnt) return fail("count", c, Q, step);
    int unused_sets = 0, unused_gets = 0;
    const PlainQueue rd{win.data(), ring.data(), lh, head, Q, &unused_sets, &unused_gets};
    for (int i = 0; i < cnt; ++i) {
      const Entry g = rd.get(i);
      if (g.x != model[(size_t)i].x || g.y != model[(size_t)i].y)
        return fail("order", c, Q, step);
    }
    if (model[(size_t)at].x != e.x || model[(size_t)at].y != e.y)
      return fail("position", c, Q, step);
  }
  std::printf("%d %d %d %d %d %d\n", c, Q, pushes, ooo, max_shift, ring_starts);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1u;
  for (int c = 1; c <= 64; ++c) {
    if (!lbk::workers_ok(c)) return 1;
    for (int Q : {3, 8, 9, 32, 64})
      if (run(c, Q, seed) != 0) return 1;
  }
  if (lbk::workers_ok(0) || lbk::workers_ok(65) || lbk::workers_ok(-1)) return 1;
  return 0;
}
