// pool_probe -- the shared-server-pool rule of marllb_amd/csrc/lbsim_pool.h as host C++, for
// tests/test_server_pools.py (built there with -fsanitize=address,undefined and run as a
// program).  One command per input line, one output line each:
//   check B off A            -> pool_enable_check
//   lanes S A forced         -> pool_group_lanes
//   next A t0 .. t(A-1)      -> pool_next_member
//   svc workbits scalebits   -> pool_service of the two f32 bit patterns
//   fifo Q head n (ta svc owner) x n
//        one physical FIFO on a ring of exactly Q heap entries whose head starts at `head` (a read
//        or write past the ring is the sanitizer's to report): before each arrival the heads due
//        by ta leave, the arrival joins if the queue is below Q and is dropped otherwise, and at
//        the end the queue drains.  Prints "c tc ta owner" per completion and "d ta owner" per
//        drop in order, then "w <ring word before the drain>".
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../marllb_amd/csrc/lbsim_pool.h"

namespace {

struct Entry {
  int32_t x, y;
};

struct HeapRing {
  std::vector<Entry>* e;
  std::vector<uint8_t>* o;
  Entry entry(int i) const { return e->at((size_t)i); }
  int owner(int i) const { return (int)o->at((size_t)i); }
  void put(int i, int32_t tc, int32_t ta, int own) const {
    e->at((size_t)i) = Entry{tc, ta};
    o->at((size_t)i) = (uint8_t)own;
  }
};

float from_bits(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "check") {
      long long B, off, A;
      in >> B >> off >> A;
      std::printf("%d\n", lbk::pool_enable_check(B, off, A));
    } else if (cmd == "lanes") {
      int S, A, f;
      in >> S >> A >> f;
      std::printf("%d\n", lbk::pool_group_lanes(S, A, f));
    } else if (cmd == "next") {
      int A;
      in >> A;
      std::vector<int32_t> t((size_t)A);
      for (auto& v : t) in >> v;
      std::printf("%d\n", lbk::pool_next_member(t.data(), A));
    } else if (cmd == "svc") {
      uint32_t w, s;
      in >> w >> s;
      std::printf("%d\n", lbk::pool_service(from_bits(w), from_bits(s)));
    } else if (cmd == "fifo") {
      int Q, head, n;
      in >> Q >> head >> n;
      std::vector<Entry> ring((size_t)Q, Entry{0x7F0F0F0F, 0x7F0F0F0F});
      std::vector<uint8_t> own((size_t)Q, 0xEE);
      const HeapRing r{&ring, &own};
      lbk::PoolFifo f = lbk::pool_fifo_load((uint32_t)head, r, Q);
      auto pop = [&]() {
        const int32_t tc = f.head_tc, ta = r.entry(f.head).y;
        const int o = lbk::pool_pop(f, r, Q);
        std::printf("c %d %d %d ", tc, ta, o);
      };
      for (int i = 0; i < n; ++i) {
        int32_t ta, svc;
        int o;
        in >> ta >> svc >> o;
        while (lbk::pool_due(f, ta)) pop();
        if (lbk::pool_eligible(f, Q)) lbk::pool_push(f, r, Q, ta, svc, o);
        else std::printf("d %d %d ", ta, o);
      }
      const uint32_t word = lbk::pool_hc_word(f);
      // the word read back through the ring gives the same fifo
      const lbk::PoolFifo g = lbk::pool_fifo_load(word, r, Q);
      if (g.head != f.head || g.cnt != f.cnt ||
          (f.cnt > 0 && (g.head_tc != f.head_tc || g.head_owner != f.head_owner || g.tail != f.tail)))
        return 1;
      while (f.cnt > 0) pop();
      std::printf("w %u\n", word);
    } else if (!cmd.empty()) {
      return 2;
    }
  }
  return 0;
}
