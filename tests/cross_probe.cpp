// cross_probe — the cross-traffic rule of marllb_amd/csrc/lbsim_cross.h as host C++, for
// tests/test_cross_traffic.py (built there with -fsanitize=address,undefined and run as a
// program).  One command per line of stdin, one line of stdout each; floats travel as their bits:
//   thr <share bits>                      -> <ok> <thr>
//   edges <S> <weight bits> x S           -> <ok> <cum> x S
//   uniform <S>                           -> <cum> x S
//   sweep <S> <cum> x S                   -> cross_pick of EVERY 24-bit word, as its runs:
//                                            <pick at 0> then <x> <pick at x> per change
//   hash <key0> <key1> <gid> <episode> <k> <thr>   -> <salt> <h> <hidden> <word>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../marllb_amd/csrc/lbsim_cross.h"

static float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "thr") {
      uint32_t b;
      in >> b;
      const float sh = from_bits(b);
      const bool ok = lbk::cross_share_ok(sh);
      std::printf("%d %u\n", ok ? 1 : 0, ok ? lbk::cross_thr(sh) : 0u);
    } else if (cmd == "edges" || cmd == "uniform" || cmd == "sweep") {
      int S = 0;
      in >> S;
      if (S < 1 || S > 64) return 2;
      std::vector<float> w((size_t)S);
      std::vector<uint32_t> cum((size_t)S, 0u);
      if (cmd == "edges") {
        for (int s = 0; s < S; ++s) {
          uint32_t b;
          in >> b;
          w[(size_t)s] = from_bits(b);
        }
        const bool ok = lbk::cross_edges(w.data(), 1, S, cum.data());
        std::printf("%d", ok ? 1 : 0);
        for (int s = 0; s < S; ++s) std::printf(" %u", ok ? cum[(size_t)s] : 0u);
        std::printf("\n");
      } else if (cmd == "uniform") {
        lbk::cross_edges_uniform(S, cum.data());
        for (int s = 0; s < S; ++s) std::printf("%s%u", s ? " " : "", cum[(size_t)s]);
        std::printf("\n");
      } else {
        for (int s = 0; s < S; ++s) in >> cum[(size_t)s];
        int last = lbk::cross_pick(cum.data(), S, 0u);
        std::printf("%d", last);
        for (uint32_t x = 1; x < lbk::kCrossOne; ++x) {
          const int p = lbk::cross_pick(cum.data(), S, x);
          if (p != last) std::printf(" %u %d", x, p);
          last = p;
        }
        std::printf("\n");
      }
    } else if (cmd == "hash") {
      uint32_t k0, k1, gid, ep, k, thr;
      in >> k0 >> k1 >> gid >> ep >> k >> thr;
      const uint32_t salt = lbk::cross_salt(k0, k1, gid, ep);
      const uint32_t h = lbk::cross_hash(k, salt);
      std::printf("%u %u %d %u\n", salt, h, lbk::cross_hidden(h, thr) ? 1 : 0,
                  lbk::cross_pick_word(h));
    } else if (!cmd.empty()) {
      return 2;
    }
  }
  return 0;
}
