// delay_probe.cpp — csrc/lbsim_delay.h as host C++ against a naive model (tests/test_action_delay.py
// builds it with the address and undefined-behaviour sanitizers and runs it).
//
// For every M in 1..8, dt in {250000, 50000, 7}, every k in 0..40 and the delays 0, 1, dt - 1, dt,
// dt + 1, ..., M dt: m and r against repeated subtraction, the two steps read and the j < 0 rule
// against the text, the rows against a counted walk round the ring, the row written against every
// row read on a ring array with guard words, and the R rows k, k - 1, ..., k - M - 1 pairwise
// distinct.  Prints "OK <checks>", then one line "C <f32 bits> <M> <dt> <ok> <us>" per converted
// value for the caller to compare with numpy's rint.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../marllb_amd/csrc/lbsim_delay.h"

using namespace lbk;

static long checks = 0;
#define CHECK(c)                                                        \
  do {                                                                  \
    ++checks;                                                           \
    if (!(c)) {                                                         \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);           \
      return 1;                                                         \
    }                                                                   \
  } while (0)

static int naive_row(int j, int R) {  // j >= 0: j steps round a ring of R rows from row 0
  int row = 0;
  for (int i = 0; i < j; ++i) row = row + 1 == R ? 0 : row + 1;
  return row;
}

int main() {
  const int dts[] = {250000, 50000, 7};
  for (int M = 1; M <= kMaxDelaySteps; ++M) {
    CHECK(delay_steps_ok(M));
    const int R = delay_rows(M);
    CHECK(R == M + 2);
    for (int dt : dts) {
      CHECK(delay_max_us(M, dt) == (uint32_t)(M * dt));
      std::vector<uint32_t> delays;
      for (int j = 0; j <= M; ++j)
        for (int e = -1; e <= 1; ++e) {
          const long d = (long)j * dt + e;
          if (d >= 0 && d <= (long)M * dt) delays.push_back((uint32_t)d);
        }
      CHECK(!delay_us_ok((uint32_t)(M * dt) + 1u, M, dt));
      for (uint32_t d : delays) {
        CHECK(delay_us_ok(d, M, dt));
        int m = 0;
        long rest = d;
        while (rest >= dt) rest -= dt, ++m;
        CHECK(delay_whole(d, dt) == m && delay_rem(d, dt) == (int)rest);
        CHECK(m <= M && (m < M || rest == 0));
        for (int k = 0; k <= 40; ++k) {
          const int jn = delay_step_new(k, m), jo = delay_step_old(k, m);
          CHECK(jn == k - m && jo == jn - 1);
          CHECK(delay_is_ones(jn) == (jn < 0) && delay_is_ones(jo) == (jo < 0));
          // the ring of one env with a guard word on either side: the launch marks the rows it
          // reads, then writes its own
          std::vector<int> ring((size_t)R + 2, 0);
          int* const rows = ring.data() + 1;
          for (int j : {jn, jo}) {
            if (delay_is_ones(j) || j == k) continue;  // ones / the launch's own action
            const int row = delay_row(j, R);
            CHECK(row >= 0 && row < R && row == naive_row(j, R));
            rows[row] = 1;
          }
          const int wrow = delay_row(k, R);
          CHECK(wrow >= 0 && wrow < R && wrow == naive_row(k, R));
          CHECK(rows[wrow] == 0);  // never a row this launch reads
          CHECK(ring.front() == 0 && ring.back() == 0);
          std::vector<int> seen((size_t)R, 0);  // k, k - 1, ..., k - M - 1: R distinct rows
          for (int j = k; j >= k - M - 1 && j >= 0; --j) {
            CHECK(seen[(size_t)delay_row(j, R)] == 0);
            seen[(size_t)delay_row(j, R)] = 1;
          }
        }
      }
    }
  }
  CHECK(!delay_steps_ok(0) && !delay_steps_ok(9) && !delay_steps_ok(-1));
  std::printf("OK %ld\n", checks);

  // conversions: multiples of a step that is no whole number of us, exact half microseconds, the
  // bounds, and what must be refused
  const int M = 2, dt = 250000;
  std::vector<float> v;
  for (int i = 0; i < 400; ++i) v.push_back((float)i * 0.0015037f);  // up to 0.6 s: past M dt
  for (int i = 0; i < 64; ++i) v.push_back(((float)i + 0.5f) * 1e-6f);
  for (float x : {0.0f, -0.0f, 0.5f, 0.50000006f, 0.5000005f, 0.500001f, 0.49999997f, 1e-7f,
                  4.9e-7f, 5.1e-7f, -1e-9f, -1.0f, 1e9f, std::numeric_limits<float>::infinity(),
                  std::numeric_limits<float>::quiet_NaN()})
    v.push_back(x);
  for (float x : v) {
    uint32_t bits, us = 77u;
    std::memcpy(&bits, &x, 4);
    const bool ok = delay_convert(x, M, dt, us);
    std::printf("C %u %d %d %d %u\n", bits, M, dt, ok ? 1 : 0, us);
  }
  return 0;
}
