// truth_probe — the ground-truth rule of marllb_amd/csrc/lbsim_truth.h as host C++, for
// tests/test_ground_truth.py (built there with -fsanitize=address,undefined and run as a
// program).  `truth_probe <seed>` evaluates truth_row, for every c in 1..64, Q in {3, 8, 9, 32,
// 64}, every n in 0..Q and every head position, on a ring of exactly Q heap entries (a read past
// it is the sanitizer's to report) whose n live entries are sorted by t_complete, some of them due
// (<= 0), and whose other slots hold a poison value no result may show.  Each row must equal, bit
// for bit, a brute-force computation on the queue copied out by modulo: the workers are held by
// the c flows with the latest completions, an arrival waits for the earliest of them, the server
// drains at the latest completion of all.  The ring reads are counted: none from an empty queue,
// one when both positions coincide, never more than two.  Prints one line per (c, Q):
//   <c> <Q> <rows> <rows whose queue wraps the ring> <rows with two reads> <rows with n >= c > 1>
// and exits 1 at the first mismatch.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../marllb_amd/csrc/lbsim_truth.h"

namespace {

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

constexpr int32_t kPoison = 0x7F0F0F0F;

struct RingQueue {
  const Entry* ring;  // [Q]
  int head, Q;
  int* gets;
  Entry get(int pos) const {
    ++*gets;
    return ring[lbk::workers_ring_index(head, pos, Q)];
  }
};

int fail(const char* what, int c, int Q, int n, int head) {
  std::printf("MISMATCH %s: c %d Q %d n %d head %d\n", what, c, Q, n, head);
  return 1;
}

int run(int c, int Q, uint64_t seed) {
  Rng rng{seed * 0x9E3779B97F4A7C15ull + (uint64_t)(c * 131 + Q) + 1u};
  int rows = 0, wrapped = 0, two = 0, multi = 0;
  for (int n = 0; n <= Q; ++n) {
    for (int head = 0; head < Q; ++head) {
      std::vector<Entry> ring((size_t)Q, Entry{kPoison, kPoison});
      // sorted completion times; the first ones may be due already (a pop happens only inside a
      // launch), equal times included
      std::vector<int32_t> tc((size_t)n);
      int32_t t = -rng.below(3) * rng.below(5000);
      for (int i = 0; i < n; ++i) {
        t += rng.below(4) == 0 ? 0 : rng.below(400000);
        tc[(size_t)i] = t;
      }
      for (int i = 0; i < n; ++i) ring[(size_t)((head + i) % Q)] = Entry{tc[(size_t)i], -i};
      const bool down = n == 0 && rng.below(2) == 0;
      const int32_t lost = -rng.below(n + 1);
      const float mu = 1.0f + (float)rng.below(1 << 20) / 7.0f;
      // the ring word: head, the sticky flag at random, the count
      const uint32_t hc = (uint32_t)head | (rng.below(2) ? 0x8000u : 0u) | (uint32_t)n << 16;
      if (lbk::truth_head(hc) != head || lbk::truth_count(hc) != n) return fail("hc", c, Q, n, head);
      int gets = 0;
      const RingQueue q{ring.data(), head, Q, &gets};
      float got[lbk::kTruthCols];
      lbk::truth_row(q, hc, c, lost, down, mu, got);
      // brute force
      const int busy = std::min(n, c);
      int32_t wait = 0, backlog = 0;
      if (n >= c) {  // the c latest completions hold the workers: the earliest of them
        wait = *std::min_element(tc.end() - c, tc.end());
        wait = std::max(wait, 0);
      }
      if (n > 0) backlog = std::max(*std::max_element(tc.begin(), tc.end()), 0);
      const float want[lbk::kTruthCols] = {
          (float)n, (float)(-lost), (float)busy, (float)busy / (float)c, (float)wait * 1e-6f,
          (float)backlog * 1e-6f, down ? 0.0f : 1.0f, (float)c * mu};
      if (std::memcmp(got, want, sizeof(want)) != 0) return fail("row", c, Q, n, head);
      for (float v : got)
        if (!(v >= 0.0f)) return fail("negative", c, Q, n, head);
      int gets2 = 0;
      const RingQueue q2{ring.data(), head, Q, &gets2};
      if (lbk::truth_wait_us(q2, n, c) != wait || lbk::truth_backlog_us(q2, n) != backlog)
        return fail("parts", c, Q, n, head);
      const int reads = n == 0 ? 0 : (n < c || n - c == n - 1 ? 1 : 2);
      if (gets != reads) return fail("reads", c, Q, n, head);
      ++rows;
      wrapped += head + n > Q;
      two += reads == 2;
      multi += c > 1 && n >= c;
    }
  }
  std::printf("%d %d %d %d %d %d\n", c, Q, rows, wrapped, two, multi);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1u;
  for (int c = 1; c <= 64; ++c)
    for (int Q : {3, 8, 9, 32, 64})
      if (run(c, Q, seed) != 0) return 1;
  if (lbk::truth_seconds(1500000) != 1500000.0f * 1e-6f) return 1;
  return 0;
}
