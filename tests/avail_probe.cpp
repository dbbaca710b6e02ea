// csrc/lbsim_avail.h as host C++: avail_apply_kernel's per-(env, server) body run for every
// thread of a launch, on sections placed between guard bytes (tests/test_server_avail.py builds
// this with -fsanitize=address,undefined and compares what it writes with the numpy rule).
//
//   avail_probe IN OUT
//
// IN: 16 int32 header words {B, S, split, res_vpp, has_lost_on, dur_words, P, H, wrap,
// next_reset, max_steps, has_table, 0...}, then the arrays back to back, in this order (an absent
// one has no bytes): ep_step[B], dropped[B], hc, last_tc, res_count [B*S], res [B*S*256],
// fcache [B*S*10], down [B*S], lost_on [B*S], res_dur [B*S*128*dur_words], res_count_dur,
// pend_hc [B*S] (4-byte words all), table [B*P*S] bytes.
// OUT: want [B*S] bytes, up_now [B*S] bytes, phase [B] int32 as a launch with apply = 0 reports
// them (which must leave every section as it was), then the arrays above (without the table)
// after a launch with apply = 1.  Exit status 0 when no guard byte changed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../marllb_amd/csrc/lbsim_avail.h"

namespace {

constexpr size_t kGuard = 64;
constexpr unsigned char kFill = 0xA5;

struct Guarded {
  std::vector<unsigned char> mem;
  size_t bytes = 0;
  void load(FILE* f, size_t n) {
    bytes = n;
    mem.assign(n + 2 * kGuard, kFill);
    if (n != 0 && fread(mem.data() + kGuard, 1, n, f) != n) {
      fprintf(stderr, "short input\n");
      exit(2);
    }
  }
  void blank(size_t n) {
    bytes = n;
    mem.assign(n + 2 * kGuard, kFill);
    memset(mem.data() + kGuard, 0, n);
  }
  template <typename T>
  T* ptr() { return bytes != 0 ? reinterpret_cast<T*>(mem.data() + kGuard) : nullptr; }
  bool intact() const {
    for (size_t i = 0; i < kGuard; ++i)
      if (mem[i] != kFill || mem[kGuard + bytes + i] != kFill) return false;
    return true;
  }
  void save(FILE* f) const {
    if (bytes != 0) fwrite(mem.data() + kGuard, 1, bytes, f);
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = fopen(argv[1], "rb");
  if (in == nullptr) return 2;
  int32_t hd[16];
  if (fread(hd, 4, 16, in) != 16) return 2;
  const size_t B = (size_t)hd[0], S = (size_t)hd[1], BS = B * S;
  const int split = hd[2], res_vpp = hd[3], has_lost = hd[4], dur_words = hd[5];
  const int P = hd[6], H = hd[7], wrap = hd[8], next_reset = hd[9], max_steps = hd[10];
  const int has_table = hd[11];
  const size_t sizes[12] = {B * 4,
                            B * 4,
                            BS * 4,
                            BS * 4,
                            BS * 4,
                            BS * (size_t)lbk::kAvailK * 8,
                            BS * (size_t)lbk::kAvailFeat * 4,
                            BS * 4,
                            has_lost ? BS * 4 : 0,
                            BS * (size_t)lbk::kAvailK * 4 * (size_t)dur_words,
                            split ? BS * 4 : 0,
                            split ? BS * 4 : 0};
  Guarded sec[12], table, want, up_now, phase;
  for (int k = 0; k < 12; ++k) sec[k].load(in, sizes[k]);
  table.load(in, has_table ? B * (size_t)P * S : 0);
  fclose(in);
  want.blank(BS);
  up_now.blank(BS);
  phase.blank(B * 4);

  lbk::AvailState a{};
  a.ep_step = sec[0].ptr<int32_t>();
  uint32_t* const dropped = sec[1].ptr<uint32_t>();
  a.hc = sec[2].ptr<uint32_t>();
  a.last_tc = sec[3].ptr<int32_t>();
  a.res_count = sec[4].ptr<uint32_t>();
  a.res = sec[5].ptr<uint32_t>();
  a.fcache = sec[6].ptr<float>();
  a.down = sec[7].ptr<uint32_t>();
  a.lost_on = sec[8].ptr<uint32_t>();
  a.res_dur = sec[9].ptr<uint32_t>();
  a.res_count_dur = sec[10].ptr<uint32_t>();
  a.pend_hc = sec[11].ptr<uint32_t>();
  a.B = (int32_t)B, a.S = (int32_t)S;
  a.split = split, a.res_vpp = res_vpp;
  a.max_steps = max_steps, a.next_reset = next_reset;
  const lbk::AvailTable t{table.ptr<uint8_t>(), has_table ? P : 0, H, wrap};

  // apply = 0: the outputs, and not a byte of the state
  std::vector<unsigned char> before[12];
  for (int k = 0; k < 12; ++k) before[k] = sec[k].mem;
  const lbk::AvailOut o{want.ptr<uint8_t>(), up_now.ptr<uint8_t>(), phase.ptr<int32_t>()};
  bool ok = true;
  for (size_t i = 0; i < BS; ++i) ok &= lbk::avail_server(a, t, o, 0, (int64_t)i) == 0u;
  for (int k = 0; k < 12; ++k) ok &= before[k] == sec[k].mem;
  // apply = 1, the kernel's launch: every thread once, the lost flows added to the env's word
  for (size_t i = 0; i < BS; ++i)
    dropped[i / S] += lbk::avail_server(a, t, lbk::AvailOut{}, 1, (int64_t)i);
  for (int k = 0; k < 12; ++k) ok &= sec[k].intact();
  ok &= table.intact() && want.intact() && up_now.intact() && phase.intact();

  FILE* out = fopen(argv[2], "wb");
  if (out == nullptr) return 2;
  want.save(out);
  up_now.save(out);
  phase.save(out);
  for (int k = 0; k < 12; ++k) sec[k].save(out);
  fclose(out);
  if (!ok) fprintf(stderr, "a guard byte changed, or a launch with apply = 0 wrote the state\n");
  return ok ? 0 : 1;
}
