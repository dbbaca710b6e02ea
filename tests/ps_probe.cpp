// ps_probe — the processor-sharing rule of marllb_amd/csrc/lbsim_ps.h as host C++, for
// tests/test_processor_sharing.py (built there with -fsanitize=address,undefined and run as a
// program).  `ps_probe <seed>` drives, for every Q in {3, 8, 9, 32, 64}, a random run of arrivals,
// completions and step ends on one server whose entries sit in a ring of Q slots that starts at
// head, as the kernel's do.  After every operation the queue read back through the accessor must
// equal a naive model -- the entries stable-sorted by tag -- and the clock a naive model of the
// rule in 64-bit arithmetic; at every completion V == the head's tag and acc == 0, and the
// completion time is the smallest t at which the naive advance reaches the tag (t - 1 does not).
// Prints one line per Q:
//   <Q> <inserts> <at head of a non-empty queue> <in the middle> <at the tail> <largest shift>
//   <inserts into a queue of Q - 1> <equal tags> <completions> <rebases with acc != 0>
// and exits 1 at the first mismatch.  `ps_probe <seed> trace` also prints every operation, times
// relative to the current step's start, for the test to replay through the Python rule
// (tests/ps_ref.PSSim): "Q <Q>" at the start of a run, "C <tc> <ta>" a completion, "A <ta> <svc>
// <position>" an insert, "D <ta>" an arrival dropped at a full queue, "E <acc> <n> {<remaining>
// <ta>}..." a step end after the rebase, and the summary line after "S".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../marllb_amd/csrc/lbsim_ps.h"

namespace {

struct Entry {
  int32_t x, y;  // tag, t_arrival
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

struct PlainRing {
  Entry* ring;  // [Q]
  int head, Q;
  int* sets;
  Entry get(int pos) const { return ring[lbk::ps_ring_index(head, pos, Q)]; }
  void set(int pos, const Entry& e) const {
    ++*sets;
    ring[lbk::ps_ring_index(head, pos, Q)] = e;
  }
};

struct NaiveClock {  // the rule of DESIGN.md §3.22 in 64 bits
  int64_t V = 0, acc = 0, t_last = 0;
  void advance(int n, int64_t t) {
    if (n > 0) {
      acc += t - t_last;
      V += acc / n;
      acc %= n;
    } else {
      acc = 0;
    }
    t_last = t;
  }
};

bool g_trace = false;

int fail(const char* what, int Q, int step) {
  std::printf("MISMATCH %s: Q %d step %d\n", what, Q, step);
  return 1;
}

int run(int Q, uint64_t seed) {
  Rng rng{seed * 0x9E3779B97F4A7C15ull + (uint64_t)Q + 1u};
  std::vector<Entry> ring((size_t)Q);
  int head = rng.below(Q), n = 0;
  std::vector<Entry> model;  // sorted by tag, stable
  lbk::PsClock ck{0, 0, 0};
  NaiveClock nv;
  const int32_t dt = 50000;
  if (g_trace) std::printf("Q %d\n", Q);
  int32_t now = 0;
  int inserts = 0, at_head = 0, middle = 0, at_tail = 0, max_shift = 0, nearly_full = 0, equal = 0,
      completions = 0, carried = 0;
  // the mean service over the mean gap swings around 1: queues of every depth up to Q
  const int gap = 1000;
  for (int step = 0; step < 6000; ++step) {
    const int load = 6 + rng.below(9);  // tenths
    int32_t ta = now + 1 + rng.below(2 * gap);
    int sets = 0;
    // the step ends that come before the arrival, each with the completions due by it
    for (;;) {
      const int32_t th = ta < dt ? ta : dt;
      while (n > 0) {
        const PlainRing q{ring.data(), head, Q, &sets};
        const Entry h = q.get(0);
        const int32_t tc = lbk::ps_next_completion(ck, n, h.x);
        if (tc > th) break;
        // the naive clock reaches the tag at tc and not at tc - 1
        NaiveClock a = nv, b = nv;
        a.advance(n, tc);
        if (tc - 1 >= nv.t_last) {
          b.advance(n, tc - 1);
          if (b.V >= h.x) return fail("completion not the smallest t", Q, step);
        }
        if (a.V != h.x || a.acc != 0) return fail("naive clock at the completion", Q, step);
        lbk::PsClock g = ck;
        lbk::ps_advance(g, n, tc);
        lbk::ps_complete(ck, tc, h.x);
        if (g.V != ck.V || g.acc != ck.acc || g.t_last != ck.t_last)
          return fail("ps_complete is not ps_advance", Q, step);
        nv = a;
        if (model.empty() || model[0].x != h.x || model[0].y != h.y) return fail("pop", Q, step);
        model.erase(model.begin());
        head = head + 1 == Q ? 0 : head + 1;
        --n;
        ++completions;
        if (g_trace) std::printf("C %d %d\n", tc, h.y);
      }
      if (ta < dt) break;
      // the step's end: every clock to dt, then the rebase
      const PlainRing q{ring.data(), head, Q, &sets};
      lbk::ps_advance(ck, n, dt);
      nv.advance(n, dt);
      if (ck.V != nv.V || ck.acc != nv.acc) return fail("advance to the step end", Q, step);
      carried += ck.acc != 0;
      for (Entry& e : model) {
        e.x -= (int32_t)nv.V;
        e.y -= dt;
      }
      lbk::ps_rebase(q, n, ck, dt);
      nv.V = 0;
      nv.t_last = 0;
      if (ck.V != 0 || ck.t_last != 0 || ck.acc != nv.acc) return fail("rebase", Q, step);
      if (g_trace) {
        std::printf("E %d %d", ck.acc, n);
        for (int i = 0; i < n; ++i) std::printf(" %d %d", q.get(i).x, q.get(i).y);
        std::printf("\n");
      }
      ta -= dt;
    }
    now = ta;
    if (n == Q) {  // full: dropped
      if (g_trace) std::printf("D %d\n", ta);
      continue;
    }
    const PlainRing q{ring.data(), head, Q, &sets};
    lbk::ps_advance(ck, n, ta);
    nv.advance(n, ta);
    if (ck.V != nv.V || ck.acc != nv.acc || ck.t_last != nv.t_last) return fail("advance", Q, step);
    // a quarter of the flows are long, some repeat the head's or the tail's tag exactly
    int32_t svc = 1 + (rng.below(4) == 0 ? rng.below(8 * gap * load / 10) : rng.below(gap * load / 10));
    const int pick = rng.below(8);
    if (n > 0 && pick == 0 && model[0].x > ck.V) svc = model[0].x - ck.V;
    if (n > 0 && pick == 1 && model.back().x > ck.V) svc = model.back().x - ck.V;
    if (n > 0 && pick == 2) svc = 1;  // ahead of everything queued (or equal to the head)
    const Entry e{ck.V + svc, ta};
    bool eq = false;
    for (const Entry& m : model) eq |= m.x == e.x;
    sets = 0;
    const int at = lbk::ps_insert(q, n, e);
    if (g_trace) std::printf("A %d %d %d\n", ta, svc, at);
    model.push_back(e);
    std::stable_sort(model.begin(), model.end(),
                     [](const Entry& a, const Entry& b) { return a.x < b.x; });
    ++n;
    ++inserts;
    const int shift = n - 1 - at;
    if (shift != sets - 1) return fail("moves", Q, step);
    at_head += at == 0 && n > 1;
    at_tail += at == n - 1 && n > 1;
    middle += at > 0 && at < n - 1;
    nearly_full += n == Q;
    equal += eq;
    max_shift = std::max(max_shift, shift);
    if ((int)model.size() != n) return fail("count", Q, step);
    for (int i = 0; i < n; ++i) {
      const Entry g = q.get(i);
      if (g.x != model[(size_t)i].x || g.y != model[(size_t)i].y) return fail("order", Q, step);
    }
    if (model[(size_t)at].x != e.x || model[(size_t)at].y != e.y) return fail("position", Q, step);
  }
  std::printf("%s%d %d %d %d %d %d %d %d %d %d\n", g_trace ? "S " : "", Q, inserts, at_head, middle, at_tail, max_shift,
              nearly_full, equal, completions, carried);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1u;
  g_trace = argc > 2;
  for (int Q : {3, 8, 9, 32, 64})
    if (run(Q, seed) != 0) return 1;
  // the next completion saturates instead of wrapping: (2^30 / 64) x 64 us past t_last = 2^30
  const lbk::PsClock far{0, 0, 1 << 30};
  if (lbk::ps_next_completion(far, 64, 1 << 24) != 0x7FFFFFFF) return 1;
  return 0;
}
