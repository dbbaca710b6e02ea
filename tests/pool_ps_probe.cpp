// pool_ps_probe — the ring accessor of a PS pool's server, entries {tag, ta, owner} (DESIGN.md
// §3.24), over the rule of marllb_amd/csrc/lbsim_ps.h as host C++, for tests/test_pool_ps.py
// (built there with -fsanitize=address,undefined and run as a program).  The accessor restates
// dynamics_pool_ps_kernel's: the {tag, ta} pairs in one heap array of exactly Q slots, the owner
// bytes in another, both by ring index from the physical head, an owner read clamped below A.
// `pool_ps_probe <seed>` drives, for every Q in {3, 8, 9, 32, 64}, c in {1, 2, 3, 64} and A in
// {1, 3, 8}, a random run of arrivals of random owners, completions and step ends on one server.
// After every operation the queue must equal a naive array model: a stable sort by tag of
// {tag, ta, owner}, so that every moved entry kept its owner, the per-owner counts the model's; the
// clock must equal the rule in 64-bit arithmetic; with c >= Q every flow's tc - ta is its svc.
// Prints one line per (Q, c, A):
//   <Q> <c> <A> <inserts> <completions> <inserts at the head before another owner's entry>
//   <moves of more than 8 entries of mixed owners> <equal tags of different owners>
// and exits 1 at the first mismatch.  `pool_ps_probe <seed> trace` also prints every operation,
// times relative to the current step's start, for the test to replay through the Python rule
// (tests/pool_ps_ref.PoolPSSim): "Q <Q> <c> <A>" at the start of a run, "C <tc> <ta> <owner>" a
// completion, "A <ta> <svc> <position> <owner>" an insert, "D <ta> <owner>" an arrival dropped at
// a full queue, "E <acc> <n> <work> <drain> {<remaining> <ta> <owner>}..." a step end after the
// rebase, and the summary line after "S".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../marllb_amd/csrc/lbsim_ps.h"

namespace {

struct Pair {
  int32_t x, y;
};
struct Entry {  // what the accessor hands lbsim_ps.h: .x the tag, .y t_arrival, .o the owner
  int32_t x, y, o;
};
struct Flow {
  int32_t x, y, o, svc;
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

struct OwnerRing {
  Pair* ring;     // [Q]
  uint8_t* own;   // [Q]
  int head, Q, A;
  Entry get(int pos) const {
    const int i = lbk::ps_ring_index(head, pos, Q);
    const int o = (int)own[i];
    return Entry{ring[i].x, ring[i].y, o < A ? o : 0};
  }
  void set(int pos, const Entry& e) const {
    const int i = lbk::ps_ring_index(head, pos, Q);
    ring[i] = Pair{e.x, e.y};
    own[i] = (uint8_t)e.o;
  }
};

struct NaiveClock {  // the rule of DESIGN.md §3.23 in 64 bits
  int64_t V = 0, acc = 0, t_last = 0;
  void advance(int n, int c, int64_t t) {
    const int64_t d = t - t_last;
    if (n == 0) {
      acc = 0;
    } else if (n <= c) {
      V += d;
      acc = 0;
    } else {
      acc += (int64_t)c * d;
      V += acc / n;
      acc %= n;
    }
    t_last = t;
  }
};

bool g_trace = false;

int fail(const char* what, int Q, int c, int A, int step) {
  std::printf("MISMATCH %s: Q %d c %d A %d step %d\n", what, Q, c, A, step);
  return 1;
}

bool same(const lbk::PsClock& k, const NaiveClock& nv) {
  return k.V == nv.V && k.acc == nv.acc && k.t_last == nv.t_last;
}

int run(int Q, int c, int A, uint64_t seed, int steps) {
  Rng rng{seed * 0x9E3779B97F4A7C15ull + (uint64_t)((Q * 131 + c) * 17 + A)};
  // heap arrays of exactly Q entries: one slot past either end is the sanitizer's
  std::unique_ptr<Pair[]> ring(new Pair[(size_t)Q]);
  std::unique_ptr<uint8_t[]> own(new uint8_t[(size_t)Q]);
  for (int i = 0; i < Q; ++i) ring[(size_t)i] = Pair{0, 0}, own[(size_t)i] = 0xFF;
  int head = rng.below(Q), n = 0;
  std::vector<Flow> model;  // sorted by tag, stable
  std::vector<int> nown((size_t)A, 0);
  lbk::PsClock ck{0, 0, 0};
  NaiveClock nv;
  const int32_t dt = 50000;
  if (g_trace) std::printf("Q %d %d %d\n", Q, c, A);
  int32_t now = 0;
  int inserts = 0, completions = 0, head_other = 0, moved_mixed = 0, equal_other = 0;
  const int gap = 1000;
  const int width = c < Q ? c : Q;
  for (int step = 0; step < steps; ++step) {
    const bool low = ((step / 300) & 1) != 0;
    const int load = low ? 1 + rng.below(3) : 6 + rng.below(9);
    int32_t ta = now + 1 + rng.below(2 * gap);
    for (;;) {
      const int32_t th = ta < dt ? ta : dt;
      while (n > 0) {
        const OwnerRing q{ring.get(), own.get(), head, Q, A};
        const Entry h = q.get(0);
        const lbk::PsDue due = lbk::ps_next_completion(ck, n, c, h.x);
        if (due.tc > th) break;
        if (due.tc < ck.t_last) return fail("completion before t_last", Q, c, A, step);
        NaiveClock a = nv;
        a.advance(n, c, due.tc);
        if (a.V != h.x || a.acc != due.rem || a.acc < 0 || a.acc >= c)
          return fail("the clock at the completion", Q, c, A, step);
        lbk::ps_complete(ck, due, h.x);
        nv = a;
        if (model.empty() || model[0].x != h.x || model[0].y != h.y || model[0].o != h.o)
          return fail("pop", Q, c, A, step);
        if (c >= Q && due.tc - h.y != model[0].svc) return fail("c >= Q: fct is not svc", Q, c, A, step);
        model.erase(model.begin());
        nown[(size_t)h.o] -= 1;
        if (nown[(size_t)h.o] < 0) return fail("own count below 0", Q, c, A, step);
        head = head + 1 == Q ? 0 : head + 1;
        --n;
        ++completions;
        if (g_trace) std::printf("C %d %d %d\n", due.tc, h.y, h.o);
      }
      if (ta < dt) break;
      const OwnerRing q{ring.get(), own.get(), head, Q, A};
      lbk::ps_advance(ck, n, c, dt);
      nv.advance(n, c, dt);
      if (!same(ck, nv)) return fail("advance to the step end", Q, c, A, step);
      for (Flow& e : model) {
        e.x -= (int32_t)nv.V;
        e.y -= dt;
      }
      lbk::ps_rebase(q, n, ck, dt);
      nv.V = 0;
      nv.t_last = 0;
      if (!same(ck, nv)) return fail("rebase", Q, c, A, step);
      for (int i = 0; i < n; ++i) {  // the rebase moved no owner
        const Entry g = q.get(i);
        const Flow& m = model[(size_t)i];
        if (g.x != m.x || g.y != m.y || g.o != m.o) return fail("rebase order", Q, c, A, step);
      }
      int32_t work = -1, drain = -1;
      lbk::ps_server_state(q, n, c, ck.acc, work, drain);
      if (g_trace) {
        std::printf("E %d %d %d %d", ck.acc, n, work, drain);
        for (int i = 0; i < n; ++i) std::printf(" %d %d %d", q.get(i).x, q.get(i).y, q.get(i).o);
        std::printf("\n");
      }
      ta -= dt;
    }
    now = ta;
    const int owner = rng.below(A);
    if (n == Q) {  // full: dropped, counted for the owner
      if (g_trace) std::printf("D %d %d\n", ta, owner);
      continue;
    }
    const OwnerRing q{ring.get(), own.get(), head, Q, A};
    lbk::ps_advance(ck, n, c, ta);
    nv.advance(n, c, ta);
    if (!same(ck, nv)) return fail("advance", Q, c, A, step);
    const int mean = gap * load / 10 * width;
    int32_t svc = 1 + (rng.below(4) == 0 ? rng.below(4 * mean) : rng.below(mean));
    const int pick = rng.below(8);
    if (n > 0 && pick == 0 && model[0].x > ck.V) svc = model[0].x - ck.V;
    if (n > 0 && pick == 1 && !low && model.back().x > ck.V) svc = model.back().x - ck.V;
    if (n > 0 && pick == 2) svc = 1;  // ahead of everything queued (or equal to the head)
    const Entry e{ck.V + svc, ta, owner};
    const int at = lbk::ps_insert(q, n, e);
    if (g_trace) std::printf("A %d %d %d %d\n", ta, svc, at, owner);
    head_other += at == 0 && n > 0 && model[0].o != owner;
    if (n - at > 8) {
      bool mixed = false;
      for (int i = at + 1; i < n; ++i) mixed |= model[(size_t)i].o != model[(size_t)at].o;
      moved_mixed += mixed;
    }
    for (const Flow& m : model) equal_other += m.x == e.x && m.o != owner;
    model.push_back(Flow{e.x, e.y, owner, svc});
    std::stable_sort(model.begin(), model.end(),
                     [](const Flow& a, const Flow& b) { return a.x < b.x; });
    nown[(size_t)owner] += 1;
    ++n;
    ++inserts;
    if ((int)model.size() != n) return fail("count", Q, c, A, step);
    std::vector<int> cnt((size_t)A, 0);
    for (int i = 0; i < n; ++i) {
      const Entry g = q.get(i);
      const Flow& m = model[(size_t)i];
      if (g.x != m.x || g.y != m.y || g.o != m.o) return fail("order", Q, c, A, step);
      cnt[(size_t)g.o] += 1;
    }
    if (cnt != nown) return fail("own counts", Q, c, A, step);
    if (model[(size_t)at].x != e.x || model[(size_t)at].y != e.y || model[(size_t)at].o != owner)
      return fail("position", Q, c, A, step);
  }
  std::printf("%s%d %d %d %d %d %d %d %d\n", g_trace ? "S " : "", Q, c, A, inserts, completions,
              head_other, moved_mixed, equal_other);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1u;
  g_trace = argc > 2;
  for (int Q : {3, 8, 9, 32, 64})
    for (int c : {1, 2, 3, 64})
      for (int A : {1, 3, 8})
        if (run(Q, c, A, seed, g_trace ? 400 : 1200) != 0) return 1;
  // an owner byte that no member has (loaded bytes): read as member 0, never past the LDS rows
  Pair one[1] = {{5, 1}};
  uint8_t ob[1] = {200};
  const OwnerRing q{one, ob, 0, 1, 3};
  if (q.get(0).o != 0) return 1;
  return 0;
}
