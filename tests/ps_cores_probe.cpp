// ps_cores_probe — the c-core processor-sharing rule of marllb_amd/csrc/lbsim_ps.h (DESIGN.md
// §3.23) as host C++, for tests/test_ps_cores.py (built there with -fsanitize=address,undefined
// and run as a program).  `ps_cores_probe <seed>` drives, for every c in 1..64 and every Q in
// {3, 8, 9, 32, 64}, a random run of arrivals, completions and step ends on one server whose
// entries sit in a ring of Q slots that starts at head, as the kernel's do.  After every operation
// the clock must equal a naive model of the rule in 64-bit arithmetic and the queue a stable sort
// by tag; at every completion the naive advance reaches the head's tag exactly at tc and not at
// tc - 1, leaves acc in [0, c), and the shortcut ps_complete(due) equals ps_advance(tc); with
// c = 1 every result equals the one-core functions'; with c >= Q every flow's tc - ta is its svc;
// at every step end ps_server_state equals the naive work and the naive clock run forward until
// the server is empty.  Prints one line per (c, Q):
//   <c> <Q> <inserts> <completions> <completions leaving acc > 0> <remainders dropped at n <= c>
//   <completions at t_last with n > c> <arrivals finding n == c> <step ends with n > c, acc != 0>
// and exits 1 at the first mismatch.  `ps_cores_probe <seed> trace` runs c in {1, 2, 3, 5, 8, 64}
// only and also prints every operation, times relative to the current step's start, for the test
// to replay through the Python rule (tests/ps_cores_ref.PSCoresSim): "Q <Q> <c>" at the start of
// a run, "C <tc> <ta>" a completion, "A <ta> <svc> <position>" an insert, "D <ta>" an arrival
// dropped at a full queue, "E <acc> <n> <work> <drain> {<remaining> <ta>}..." a step end after
// the rebase, and the summary line after "S".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../marllb_amd/csrc/lbsim_ps.h"

namespace {

struct Entry {
  int32_t x, y;  // tag, t_arrival
};

struct Flow {
  int32_t x, y, svc;
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
  Entry get(int pos) const { return ring[lbk::ps_ring_index(head, pos, Q)]; }
  void set(int pos, const Entry& e) const { ring[lbk::ps_ring_index(head, pos, Q)] = e; }
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

int fail(const char* what, int c, int Q, int step) {
  std::printf("MISMATCH %s: c %d Q %d step %d\n", what, c, Q, step);
  return 1;
}

bool same(const lbk::PsClock& k, const NaiveClock& nv) {
  return k.V == nv.V && k.acc == nv.acc && k.t_last == nv.t_last;
}

int run(int c, int Q, uint64_t seed, int steps) {
  Rng rng{seed * 0x9E3779B97F4A7C15ull + (uint64_t)(Q * 131 + c)};
  std::vector<Entry> ring((size_t)Q);
  int head = rng.below(Q), n = 0;
  std::vector<Flow> model;  // sorted by tag, stable
  lbk::PsClock ck{0, 0, 0};
  NaiveClock nv;
  const int32_t dt = 50000;
  if (g_trace) std::printf("Q %d %d\n", Q, c);
  int32_t now = 0;
  int inserts = 0, completions = 0, acc_left = 0, rem_dropped = 0, zero_delta = 0, n_eq_c = 0,
      carried = 0;
  const int gap = 1000;
  const int width = c < Q ? c : Q;  // the flows served side by side: the load follows it
  for (int step = 0; step < steps; ++step) {
    // tenths: stretches of overload (the cores are shared, the queue fills) between stretches
    // that let the server fall back to n <= c
    const bool low = ((step / 300) & 1) != 0;
    const int load = low ? 1 + rng.below(3) : 6 + rng.below(9);
    int32_t ta = now + 1 + rng.below(2 * gap);
    for (;;) {
      const int32_t th = ta < dt ? ta : dt;
      while (n > 0) {
        const PlainRing q{ring.data(), head, Q};
        const Entry h = q.get(0);
        const lbk::PsDue due = lbk::ps_next_completion(ck, n, c, h.x);
        if (c == 1 && (due.tc != lbk::ps_next_completion(ck, n, h.x) || due.rem != 0))
          return fail("c = 1 is not the one-core next completion", c, Q, step);
        if (due.tc > th) break;
        if (due.tc < ck.t_last) return fail("completion before t_last", c, Q, step);
        NaiveClock a = nv, b = nv;
        a.advance(n, c, due.tc);
        if (due.tc - 1 >= nv.t_last) {
          b.advance(n, c, due.tc - 1);
          if (b.V >= h.x) return fail("completion not the smallest t", c, Q, step);
        }
        if (a.V != h.x) return fail("naive clock misses the tag at the completion", c, Q, step);
        if (a.acc < 0 || a.acc >= c || a.acc != due.rem)
          return fail("the carry left at the completion", c, Q, step);
        lbk::PsClock g = ck;
        lbk::ps_advance(g, n, c, due.tc);
        rem_dropped += n <= c && ck.acc > 0;
        zero_delta += n > c && due.tc == ck.t_last;
        lbk::ps_complete(ck, due, h.x);
        if (g.V != ck.V || g.acc != ck.acc || g.t_last != ck.t_last)
          return fail("ps_complete is not ps_advance", c, Q, step);
        nv = a;
        acc_left += ck.acc > 0;
        if (model.empty() || model[0].x != h.x || model[0].y != h.y) return fail("pop", c, Q, step);
        if (c >= Q && due.tc - h.y != model[0].svc)
          return fail("c >= Q: fct is not svc", c, Q, step);
        model.erase(model.begin());
        head = head + 1 == Q ? 0 : head + 1;
        --n;
        ++completions;
        if (g_trace) std::printf("C %d %d\n", due.tc, h.y);
      }
      if (ta < dt) break;
      // the step's end: the clock to dt, then the rebase, then the privileged view
      const PlainRing q{ring.data(), head, Q};
      rem_dropped += n > 0 && n <= c && ck.acc > 0;
      lbk::ps_advance(ck, n, c, dt);
      nv.advance(n, c, dt);
      if (!same(ck, nv)) return fail("advance to the step end", c, Q, step);
      carried += n > c && ck.acc != 0;
      for (Flow& e : model) {
        e.x -= (int32_t)nv.V;
        e.y -= dt;
      }
      lbk::ps_rebase(q, n, ck, dt);
      nv.V = 0;
      nv.t_last = 0;
      if (!same(ck, nv)) return fail("rebase", c, Q, step);
      int32_t work = -1, drain = -1;
      lbk::ps_server_state(q, n, c, ck.acc, work, drain);
      {
        int64_t w = n > c ? -nv.acc : 0;
        for (const Flow& e : model) w += e.x;
        NaiveClock f = nv;
        int64_t last = 0;
        for (int i = 0; i < n; ++i) {  // forward with no arrival: each head at its smallest t
          const int m = n - i;
          int64_t t = f.t_last;
          for (;;) {  // (gallop, then the exact us)
            NaiveClock p = f;
            p.advance(m, c, t);
            if (p.V >= model[(size_t)i].x) break;
            const int64_t left = model[(size_t)i].x - p.V;
            t += left > 2 ? left / 2 : 1;  // V gains at most 1 per us
          }
          f.advance(m, c, t);
          if (f.V != model[(size_t)i].x) return fail("naive drain overshoots", c, Q, step);
          last = t;
        }
        if (work != w || drain != last) return fail("ps_server_state", c, Q, step);
      }
      if (g_trace) {
        std::printf("E %d %d %d %d", ck.acc, n, work, drain);
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
    const PlainRing q{ring.data(), head, Q};
    n_eq_c += n == c;
    rem_dropped += n > 0 && n <= c && ck.acc > 0;
    if (c == 1) {
      lbk::PsClock one = ck;
      lbk::ps_advance(one, n, ta);
      lbk::ps_advance(ck, n, c, ta);
      if (one.V != ck.V || one.acc != ck.acc || one.t_last != ck.t_last)
        return fail("c = 1 is not the one-core advance", c, Q, step);
    } else {
      lbk::ps_advance(ck, n, c, ta);
    }
    nv.advance(n, c, ta);
    if (!same(ck, nv)) return fail("advance", c, Q, step);
    // a quarter of the flows are long, some repeat the head's or the tail's tag exactly
    const int mean = gap * load / 10 * width;
    int32_t svc = 1 + (rng.below(4) == 0 ? rng.below(4 * mean) : rng.below(mean));
    const int pick = rng.below(8);
    if (n > 0 && pick == 0 && model[0].x > ck.V) svc = model[0].x - ck.V;
    // (a copy of the longest flow is load of its own: not while the server is to drain)
    if (n > 0 && pick == 1 && !low && model.back().x > ck.V) svc = model.back().x - ck.V;
    if (n > 0 && pick == 2) svc = 1;  // ahead of everything queued (or equal to the head)
    const Entry e{ck.V + svc, ta};
    const int at = lbk::ps_insert(q, n, e);
    if (g_trace) std::printf("A %d %d %d\n", ta, svc, at);
    model.push_back(Flow{e.x, e.y, svc});
    std::stable_sort(model.begin(), model.end(),
                     [](const Flow& a, const Flow& b) { return a.x < b.x; });
    ++n;
    ++inserts;
    if ((int)model.size() != n) return fail("count", c, Q, step);
    for (int i = 0; i < n; ++i) {
      const Entry g = q.get(i);
      if (g.x != model[(size_t)i].x || g.y != model[(size_t)i].y) return fail("order", c, Q, step);
    }
    if (model[(size_t)at].x != e.x || model[(size_t)at].y != e.y) return fail("position", c, Q, step);
  }
  std::printf("%s%d %d %d %d %d %d %d %d %d\n", g_trace ? "S " : "", c, Q, inserts, completions,
              acc_left, rem_dropped, zero_delta, n_eq_c, carried);
  return 0;
}

// The completion of a server {V, acc, t_last} with n entries on c cores at the head's tag, against
// the naive clock: reaches the tag at tc, not at tc - 1, the carry as returned.
bool one_completion(lbk::PsClock k, int n, int c, int32_t tag) {
  const lbk::PsDue due = lbk::ps_next_completion(k, n, c, tag);
  NaiveClock a, b;
  a.V = b.V = k.V, a.acc = b.acc = k.acc, a.t_last = b.t_last = k.t_last;
  a.advance(n, c, due.tc);
  b.advance(n, c, (int64_t)due.tc - 1);
  lbk::PsClock g = k;
  lbk::ps_advance(g, n, c, due.tc);
  return a.V == tag && a.acc == due.rem && b.V < tag && g.V == tag && g.acc == due.rem;
}

}  // namespace

int main(int argc, char** argv) {
  const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1u;
  g_trace = argc > 2;
  for (int c = 1; c <= 64; ++c) {
    if (g_trace && c != 1 && c != 2 && c != 3 && c != 5 && c != 8 && c != 64) continue;
    for (int Q : {3, 8, 9, 32, 64})
      if (run(c, Q, seed, g_trace ? 600 : 1200) != 0) return 1;
  }
  // the next completion saturates instead of wrapping: 2^32 / 2 us past t_last = 2^30
  const lbk::PsClock far{0, 0, 1 << 30};
  if (lbk::ps_next_completion(far, 64, 2, 1 << 26).tc != 0x7FFFFFFF) return 1;
  if (lbk::ps_next_completion(far, 2, 2, 0x7FFFFFF0).tc != 0x7FFFFFFF) return 1;
  // (tag_head - V) n beyond 32 bits, the completion within range: the 64-bit division
  for (int c : {5, 33, 63})
    for (int32_t acc : {0, 1, 40})
      if (!one_completion(lbk::PsClock{5, acc, 1000}, 64, c, (1 << 27) + 5 + c)) return 1;
  // a step of 100 s on 64 cores: c (t - t_last) is beyond 32 bits, the advance is not
  for (int n : {65, 100, 4096}) {
    lbk::PsClock k{7, n - 1, 3};
    NaiveClock nv;
    nv.V = 7, nv.acc = n - 1, nv.t_last = 3;
    lbk::ps_advance(k, n, 64, 100000000);
    nv.advance(n, 64, 100000000);
    if (!same(k, nv)) return 1;
  }
  return 0;
}
