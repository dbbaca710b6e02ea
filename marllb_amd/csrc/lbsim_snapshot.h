// lbsim_snapshot.h — on-device snapshots (lbsim_state_save / lbsim_state_load).
//
// One kernel, state_gather_kernel, moves per-env rows between the handle's state arrays and a
// caller-owned device buffer laid out as lbsim_get_state lays out its host buffer (DESIGN.md §4:
// the sections back to back, each B contiguous rows).  Save and load are the same code with the
// roles of buffer and state swapped:
//
//   save   row b of every section -> the buffer's row b, for the envs with mask[b] != 0
//   load   the buffer's row src[b] of every section -> row b, where 0 <= src[b] < B
//
// The sections come by value in a SnapTable (at most 27 of them), so one launch serves them all.
// The host sorts them into two kinds:
//
//   long rows   (>= kSnapRowMin bytes: the rings, the reservoir records, the pending rings, at
//               larger S also fcache / chg / the normalisation sums) carry nearly all the bytes.
//               One wave per env walks its long rows, 64 lanes x 16 B contiguous per instruction,
//               four such pieces loaded before the first is stored.  The env, its source and the
//               skip test are wave-uniform.
//   short rows  (the per-env words, hc / last_tc / res_count, at small S chg and fcache): one
//               lane per unit, a block covering 256 / (units per row) whole envs, so consecutive
//               lanes touch consecutive addresses.
//
// A unit is 16 bytes where the section's offset in the buffer, its array and its row size are all
// multiples of 16 (offsets are multiples of 4 B only, so an odd B leaves sections unaligned), else
// 4 bytes.  Plain loads and stores, no LDS, no atomics; nothing is read that the launch writes.
//
// snap_thread is the whole per-thread body as a host-and-device function: tests/snapshot_probe.cpp
// runs it thread by thread on the host against a byte-wise reference, with guard bytes around
// every array.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LBSIM_SNAP_HD __host__ __device__
#else
#define LBSIM_SNAP_HD
#endif

namespace lbk {

constexpr int kSnapMaxSections = 28;   // sections(h) has at most 27
constexpr uint32_t kSnapRowMin = 256;  // bytes: rows from this size on go to whole waves
constexpr uint32_t kSnapBlock = 256;   // threads per block (4 waves)
constexpr int kSnapSave = 0, kSnapLoad = 1;

#if defined(__HIPCC__)
using SnapV4 = uint4;
#else
struct alignas(16) SnapV4 {
  uint32_t x, y, z, w;
};
#endif

struct SnapSection {
  char* live;               // the handle's array: B rows
  uint64_t off;             // the section's byte offset in the snapshot buffer
  uint64_t block0;          // short rows: the section's first block among the short-row blocks
  uint32_t row;             // bytes per env, a multiple of `width`
  uint32_t width;           // bytes per unit: 16 or 4
  uint32_t envs_per_block;  // short rows: 256 / (row / width)
  uint32_t pad_;
};

struct SnapTable {
  SnapSection sec[kSnapMaxSections];  // [0, n_long): long rows; [n_long, n): short rows
  int32_t n, n_long;
  uint64_t long_blocks;   // ceil(B / 4) when n_long > 0: one wave per env
  uint64_t short_blocks;  // sum over the short sections of ceil(B / envs_per_block)
};

// A section as the handle lists it: its array and the bytes of all B rows.
struct SnapInput {
  void* ptr;
  size_t bytes;
};

// The table of a handle's n sections (snapshot order, n <= kSnapMaxSections) against the buffer
// `buf`; returns the blocks the launch has to cover.  The unit width is chosen here, per section,
// from the alignment of the array, of the section's place in the buffer and of the row size.
inline uint64_t snap_table_build(SnapTable& t, const SnapInput* in, int n, int64_t B,
                                 const void* buf) {
  t = SnapTable{};
  for (int pass = 0; pass < 2; ++pass) {  // long rows first
    uint64_t off = 0;
    for (int i = 0; i < n; off += in[i].bytes, ++i) {
      const uint32_t row = (uint32_t)(in[i].bytes / (size_t)B);
      if ((row >= kSnapRowMin) != (pass == 0)) continue;
      const bool wide = row % 16u == 0 && (uintptr_t)in[i].ptr % 16u == 0 &&
                        ((uintptr_t)buf + off) % 16u == 0;
      SnapSection& s = t.sec[t.n++];
      s.live = static_cast<char*>(in[i].ptr);
      s.off = off;
      s.row = row;
      s.width = wide ? 16u : 4u;
    }
    if (pass == 0) t.n_long = t.n;
  }
  t.long_blocks = t.n_long > 0 ? (uint64_t)((B + 3) / 4) : 0;
  uint64_t blk = 0;
  for (int k = t.n_long; k < t.n; ++k) {
    SnapSection& s = t.sec[k];
    s.envs_per_block = kSnapBlock / (s.row / s.width);
    s.block0 = blk;
    blk += ((uint64_t)B + s.envs_per_block - 1) / s.envs_per_block;
  }
  t.short_blocks = blk;
  return t.long_blocks + t.short_blocks;
}

// The source row of env b, or false where env b is skipped: a save skips the envs outside the
// mask, a load those whose source index is outside [0, B).
LBSIM_SNAP_HD inline bool snap_source(int dir, int64_t b, int64_t B, const uint8_t* mask,
                                      const int32_t* src_env, int64_t& s) {
  if (dir == kSnapSave) {
    s = b;
    return mask == nullptr || mask[b] != 0;
  }
  s = src_env != nullptr ? (int64_t)src_env[b] : b;
  return s >= 0 && s < B;
}

// One wave's copy of a row of n units of T: lane l takes units l, l + 64, ...; four pieces
// (4 x 64 units) are loaded before the first is stored.
template <typename T>
LBSIM_SNAP_HD inline void snap_row(char* to, const char* from, uint32_t n, uint32_t lane) {
  const T* f = reinterpret_cast<const T*>(from);
  T* d = reinterpret_cast<T*>(to);
  for (uint32_t u = lane; u < n; u += 256u) {
    // named values, not an array: an indexed array of four is staged through LDS by the compiler
    const bool p1 = u + 64u < n, p2 = u + 128u < n, p3 = u + 192u < n;
    T r0 = f[u], r1 = T(), r2 = T(), r3 = T();
    if (p1) r1 = f[u + 64u];
    if (p2) r2 = f[u + 128u];
    if (p3) r3 = f[u + 192u];
    d[u] = r0;
    if (p1) d[u + 64u] = r1;
    if (p2) d[u + 128u] = r2;
    if (p3) d[u + 192u] = r3;
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#define LBSIM_SNAP_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#else
#define LBSIM_SNAP_UNIFORM(x) (x)
#endif

// Thread `tid` of block `blk` of the launch (blk < t.long_blocks + t.short_blocks).
LBSIM_SNAP_HD inline void snap_thread(const SnapTable& t, char* buf, const uint8_t* mask,
                                      const int32_t* src_env, int dir, int64_t B, uint64_t blk,
                                      uint32_t tid) {
  if (blk < t.long_blocks) {  // one wave per env, over its long rows
    const uint32_t wave = (uint32_t)LBSIM_SNAP_UNIFORM((int32_t)(tid >> 6));
    const int64_t b = (int64_t)(blk * 4u + wave);
    if (b >= B) return;
    int64_t s;
    if (!snap_source(dir, b, B, mask, src_env, s)) return;
    // the source fits 31 bits (s < B): one scalar register, so every row base below is scalar
    s = (int64_t)LBSIM_SNAP_UNIFORM((int32_t)s);
    const uint32_t lane = tid & 63u;
    for (int k = 0; k < t.n_long; ++k) {
      const SnapSection& sec = t.sec[k];
      char* in_buf = buf + sec.off + (uint64_t)s * sec.row;
      char* in_state = sec.live + (uint64_t)b * sec.row;
      char* to = dir == kSnapSave ? in_buf : in_state;
      const char* from = dir == kSnapSave ? in_state : in_buf;
      if (sec.width == 16u) snap_row<SnapV4>(to, from, sec.row / 16u, lane);
      else snap_row<uint32_t>(to, from, sec.row / 4u, lane);
    }
    return;
  }
  const uint64_t sblk = blk - t.long_blocks;  // short rows: the section this block belongs to
  int k = t.n_long;
  for (int i = t.n_long + 1; i < t.n; ++i)
    if (sblk >= t.sec[i].block0) k = i;
  const SnapSection& sec = t.sec[k];
  const uint32_t units = sec.row / sec.width;  // 1 .. 63
  if (tid >= sec.envs_per_block * units) return;
  const uint32_t e = tid / units, j = tid - e * units;
  const int64_t b = (int64_t)((sblk - sec.block0) * sec.envs_per_block + e);
  if (b >= B) return;
  int64_t s;
  if (!snap_source(dir, b, B, mask, src_env, s)) return;
  char* in_buf = buf + sec.off + (uint64_t)s * sec.row + (uint64_t)j * sec.width;
  char* in_state = sec.live + (uint64_t)b * sec.row + (uint64_t)j * sec.width;
  char* to = dir == kSnapSave ? in_buf : in_state;
  const char* from = dir == kSnapSave ? in_state : in_buf;
  if (sec.width == 16u) *reinterpret_cast<SnapV4*>(to) = *reinterpret_cast<const SnapV4*>(from);
  else *reinterpret_cast<uint32_t*>(to) = *reinterpret_cast<const uint32_t*>(from);
}

#if defined(__HIPCC__)
// Blocks beyond the grid are taken in a stride, so the grid stays below the launch limit however
// many envs the handle has.
__global__ void __launch_bounds__(kSnapBlock)
    state_gather_kernel(SnapTable t, char* buf, const uint8_t* mask, const int32_t* src_env,
                        int dir, int64_t B) {
  const uint64_t total = t.long_blocks + t.short_blocks;
  for (uint64_t blk = blockIdx.x; blk < total; blk += gridDim.x)
    snap_thread(t, buf, mask, src_env, dir, B, blk, threadIdx.x);
}
#endif

}  // namespace lbk
