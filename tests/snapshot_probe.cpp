// snapshot_probe.cpp — csrc/lbsim_snapshot.h on the host: the table the API builds for a handle's
// sections and the kernel's per-thread body, run thread by thread against a byte-wise reference.
// Plain host C++ (tests/test_state_snapshot.py compiles and runs it; no GPU).
//
// stdin: one case per line, "B buf_shift row_bytes...": B envs, the snapshot buffer placed
// buf_shift bytes past a 16-byte boundary (0 in the library, which rejects anything else; 4 / 8
// here force the 4-byte units onto every section), then each section's bytes per env.
// Per case: a full save, a masked save over a prefilled buffer, and a load with source indices
// (repeats, identity, negative and >= B entries).  Every array sits between guard bytes; a wrong
// byte or a touched guard fails the case.  stdout: one JSON object per case.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../marllb_amd/csrc/lbsim_snapshot.h"

using namespace lbk;

namespace {

constexpr size_t kGuard = 256;
constexpr unsigned char kCanary = 0x5C;

// `bytes` usable bytes, 16-byte aligned plus `shift`, between two guards.
struct Guarded {
  std::vector<unsigned char> raw;
  size_t lead = 0, bytes = 0;
  Guarded(size_t n, size_t shift) : raw(n + 2 * kGuard + 16, kCanary), bytes(n) {
    const uintptr_t base = (uintptr_t)raw.data() + kGuard;
    lead = kGuard + (16 - base % 16) % 16 + shift;
  }
  unsigned char* data() { return raw.data() + lead; }
  bool intact() const {
    for (size_t i = 0; i < raw.size(); ++i)
      if ((i < lead || i >= lead + bytes) && raw[i] != kCanary) return false;
    return true;
  }
};

uint32_t g_rng = 12345u;
uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 17;
  g_rng ^= g_rng << 5;
  return g_rng;
}

void run(const SnapTable& t, uint64_t blocks, char* buf, const uint8_t* mask, const int32_t* src,
         int dir, int64_t B) {
  for (uint64_t blk = 0; blk < blocks; ++blk)
    for (uint32_t tid = 0; tid < kSnapBlock; ++tid) snap_thread(t, buf, mask, src, dir, B, blk, tid);
}

bool run_case(int64_t B, size_t shift, const std::vector<size_t>& rows, std::string& why,
              SnapTable& t, uint64_t& blocks) {
  const int n = (int)rows.size();
  size_t total = 0;
  std::vector<size_t> off(n);
  for (int i = 0; i < n; ++i) {
    off[i] = total;
    total += rows[i] * (size_t)B;
  }
  std::vector<Guarded> live, dest;
  for (int i = 0; i < n; ++i) {
    live.emplace_back(rows[i] * (size_t)B, 0);
    dest.emplace_back(rows[i] * (size_t)B, 0);
    for (size_t j = 0; j < live[i].bytes; ++j) {
      live[i].data()[j] = (unsigned char)rnd();
      dest[i].data()[j] = (unsigned char)rnd();
    }
  }
  Guarded buf(total, shift);
  std::vector<SnapInput> in(n), in_dest(n);
  for (int i = 0; i < n; ++i) {
    in[i] = SnapInput{live[i].data(), live[i].bytes};
    in_dest[i] = SnapInput{dest[i].data(), dest[i].bytes};
  }
  blocks = snap_table_build(t, in.data(), n, B, buf.data());
  if (t.n != n) return why = "table lost a section", false;
  for (int k = 0; k < t.n; ++k) {
    const SnapSection& s = t.sec[k];
    if ((k < t.n_long) != (s.row >= kSnapRowMin)) return why = "long / short order", false;
    if (s.width != 4 && s.width != 16) return why = "width", false;
    if (s.row % s.width || (uintptr_t)s.live % s.width || ((uintptr_t)buf.data() + s.off) % s.width)
      return why = "a unit is not aligned", false;
    if (shift % 16 == 0 && s.row % 16 == 0 && s.off % 16 == 0 && s.width != 16)
      return why = "an aligned section got 4-byte units", false;
  }
  char* b = reinterpret_cast<char*>(buf.data());

  // 1. a full save is the sections back to back
  memset(buf.data(), 0xA5, total);
  run(t, blocks, b, nullptr, nullptr, kSnapSave, B);
  for (int i = 0; i < n; ++i)
    if (memcmp(buf.data() + off[i], live[i].data(), live[i].bytes)) return why = "full save", false;

  // 2. a masked save leaves the other envs' bytes
  std::vector<uint8_t> mask(B);
  for (int64_t e = 0; e < B; ++e) mask[e] = (uint8_t)(rnd() % 3 == 0 ? rnd() | 1u : 0u);
  memset(buf.data(), 0xA5, total);
  run(t, blocks, b, mask.data(), nullptr, kSnapSave, B);
  for (int i = 0; i < n; ++i)
    for (int64_t e = 0; e < B; ++e)
      for (size_t j = 0; j < rows[i]; ++j) {
        const unsigned char want = mask[e] ? live[i].data()[e * rows[i] + j] : 0xA5;
        if (buf.data()[off[i] + e * rows[i] + j] != want) return why = "masked save", false;
      }

  // 3. a load with source indices into other arrays
  run(t, blocks, b, nullptr, nullptr, kSnapSave, B);
  std::vector<int32_t> src(B);
  for (int64_t e = 0; e < B; ++e) {
    const uint32_t r = rnd() % 8;
    src[e] = r == 0 ? -1 - (int32_t)(rnd() % 5) : r == 1 ? (int32_t)(B + rnd() % 5)
             : r == 2 ? (int32_t)e : (int32_t)(rnd() % B);
  }
  std::vector<std::vector<unsigned char>> want(n);
  for (int i = 0; i < n; ++i) {
    want[i].assign(dest[i].data(), dest[i].data() + dest[i].bytes);
    for (int64_t e = 0; e < B; ++e)
      if (src[e] >= 0 && src[e] < B)
        memcpy(&want[i][e * rows[i]], live[i].data() + (size_t)src[e] * rows[i], rows[i]);
  }
  SnapTable td;
  const uint64_t blocks_d = snap_table_build(td, in_dest.data(), n, B, buf.data());
  run(td, blocks_d, b, nullptr, src.data(), kSnapLoad, B);
  for (int i = 0; i < n; ++i)
    if (memcmp(want[i].data(), dest[i].data(), dest[i].bytes)) return why = "indexed load", false;

  // 4. a load without indices is the identity
  run(td, blocks_d, b, nullptr, nullptr, kSnapLoad, B);
  for (int i = 0; i < n; ++i)
    if (memcmp(live[i].data(), dest[i].data(), dest[i].bytes)) return why = "identity load", false;

  if (!buf.intact()) return why = "guard of the buffer", false;
  for (int i = 0; i < n; ++i)
    if (!live[i].intact() || !dest[i].intact()) return why = "guard of a state array", false;
  return true;
}

}  // namespace

int main() {
  std::string line;
  char tmp[4096];
  int rc = 0;
  while (fgets(tmp, sizeof(tmp), stdin)) {
    std::istringstream is(tmp);
    long long B;
    size_t shift, r;
    if (!(is >> B >> shift)) continue;
    std::vector<size_t> rows;
    while (is >> r) rows.push_back(r);
    std::string why;
    SnapTable t{};
    uint64_t blocks = 0;
    const bool ok = run_case(B, shift, rows, why, t, blocks);
    int wide = 0;
    for (int k = 0; k < t.n; ++k) wide += t.sec[k].width == 16;
    printf("{\"ok\": %s, \"why\": \"%s\", \"sections\": %d, \"long\": %d, \"wide\": %d, "
           "\"blocks\": %llu}\n", ok ? "true" : "false", why.c_str(), t.n, t.n_long, wide,
           (unsigned long long)blocks);
    if (!ok) rc = 1;
  }
  return rc;
}
