// acks_probe.cpp -- csrc/lbsim_acks.h as host C++ (no HIP header) against a brute-force loop:
// k, t_j and "the ACKs of a flow in (a, b]".  tests/test_ack_samples.py builds it with
// -fsanitize=address,undefined and runs it as its own process: acks_probe <seed>.
// Prints one line: cases, windows_empty, windows_all, windows_part, capped_max, capped_svc,
// ack_at_b; exits 1 at the first mismatch.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../marllb_amd/csrc/lbsim_acks.h"

using namespace lbk;

namespace {

long long n_cases = 0, n_empty = 0, n_all = 0, n_part = 0, n_cap_max = 0, n_cap_svc = 0, n_at_b = 0;

int fail(const char* what, long long t0, long long svc, long long ack, long long m, long long a,
         long long b, long long got, long long want) {
  std::printf("MISMATCH %s: t0=%lld svc=%lld ack_us=%lld max_acks=%lld a=%lld b=%lld got=%lld "
              "want=%lld\n", what, t0, svc, ack, m, a, b, got, want);
  return 1;
}

// One case: every quantity in 64-bit (or wider) arithmetic and plain loops.
int check(int32_t t0, int32_t svc, int32_t ack_us, int32_t max_acks, int32_t a, int32_t b) {
  ++n_cases;
  long long kw = (long long)svc / ack_us;
  if (kw < 1) kw = 1;
  if (kw > max_acks) { kw = max_acks; ++n_cap_max; }
  if ((long long)svc / ack_us == svc && svc < max_acks) ++n_cap_svc;
  const int32_t k = ack_count(svc, ack_us, max_acks);
  if (k != kw) return fail("k", t0, svc, ack_us, max_acks, a, b, k, kw);
  if (k > svc) return fail("k <= svc", t0, svc, ack_us, max_acks, a, b, k, svc);
  long long prev = t0, lo = 0, hi = -1, done_a = 0, done_b = 0;
  for (int j = 1; j <= k; ++j) {
    const long long t = (long long)t0 + (long long)(((__int128)svc * j) / k);
    const int32_t got = ack_time(t0, svc, k, j);
    if (got != t) return fail("t_j", t0, svc, ack_us, max_acks, a, b, got, t);
    if (t <= prev) return fail("increasing", t0, svc, ack_us, max_acks, a, b, t, prev);
    prev = t;
    if (t <= a) ++done_a;
    if (t <= b) ++done_b;
    if (t > a && t <= b) {
      if (lo == 0) lo = j;
      hi = j;
      if (t == b) ++n_at_b;
    }
  }
  if (prev != (long long)t0 + svc) return fail("t_k = tc", t0, svc, ack_us, max_acks, a, b, prev, t0 + (long long)svc);
  if (ack_done_by(t0, svc, k, a) != done_a)
    return fail("done_by(a)", t0, svc, ack_us, max_acks, a, b, ack_done_by(t0, svc, k, a), done_a);
  if (ack_done_by(t0, svc, k, b) != done_b)
    return fail("done_by(b)", t0, svc, ack_us, max_acks, a, b, ack_done_by(t0, svc, k, b), done_b);
  int32_t jlo, jhi;
  ack_window(t0, svc, k, a, b, jlo, jhi);
  if (lo == 0) {  // none
    ++n_empty;
    if (jlo <= jhi) return fail("empty window", t0, svc, ack_us, max_acks, a, b, jlo, jhi);
  } else {
    if (hi - lo + 1 == k) ++n_all; else ++n_part;
    if (jlo != lo) return fail("jlo", t0, svc, ack_us, max_acks, a, b, jlo, lo);
    if (jhi != hi) return fail("jhi", t0, svc, ack_us, max_acks, a, b, jhi, hi);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const unsigned seed = argc > 1 ? (unsigned)std::atoi(argv[1]) : 1u;
  std::mt19937_64 rng(seed);
  auto uni = [&](long long lo, long long hi) {
    return (long long)(lo + (long long)(rng() % (unsigned long long)(hi - lo + 1)));
  };
  // the extremes: svc = 2^30, ack_us in {1, 2^30}, negative t0 and a, b = dt
  const int32_t big = 1 << 30;
  const int32_t dts[] = {500, 250000, 100000000};
  for (int32_t dt : dts)
    for (int32_t svc : {1, 2, 31, 32, 33, 1000, 7999, 8000, 8001, big - 1, big})
      for (int32_t ack : {1, 2, 1000, big - 1, big})
        for (int32_t m : {1, 2, 8, 31, 32})
          for (long long t0 : {(long long)-big, -(long long)svc + 1, -(long long)svc / 2, -1LL,
                               0LL, 1LL, (long long)dt - 1, (long long)dt, (long long)dt + 5})
            for (long long a : {(long long)-big, -(long long)dt, -1LL, 0LL}) {
              if (t0 + svc > 0x7FFFFFFFLL || t0 < -(long long)big) continue;
              if (check((int32_t)t0, svc, ack, m, (int32_t)a, dt)) return 1;
            }
  // random cases: short and long services against short and long windows
  for (int i = 0; i < 400000; ++i) {
    const int32_t svc = (int32_t)(i % 3 == 0 ? uni(1, 40) : i % 3 == 1 ? uni(1, 300000) : uni(1, big));
    const int32_t ack = (int32_t)(i % 4 == 0 ? 1 : i % 4 == 1 ? uni(1, 50) : i % 4 == 2 ? uni(1, 5000) : uni(1, big));
    const int32_t m = (int32_t)uni(1, 32);
    const int32_t t0 = (int32_t)uni(-(long long)svc - 100, 300000);
    long long a = uni(-400000, 300000), b = a + (i % 5 == 0 ? uni(0, 3) : uni(0, 400000));
    if (i % 7 == 0) {  // a window end exactly on an ACK
      const int32_t k = ack_count(svc, ack, m);
      b = ack_time(t0, svc, k, (int32_t)uni(1, k));
      a = b - uni(0, 1000);
    }
    if (check(t0, svc, ack, m, (int32_t)a, (int32_t)b)) return 1;
  }
  std::printf("%lld %lld %lld %lld %lld %lld %lld\n", n_cases, n_empty, n_all, n_part, n_cap_max,
              n_cap_svc, n_at_b);
  return 0;
}
