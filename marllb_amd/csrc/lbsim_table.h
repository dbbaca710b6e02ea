// lbsim_table.h — the bin rule of the workload tables (lbsim_set_workload_tables; DESIGN.md
// §3.15).
//
// A table is kTableBins f32 quantile levels indexed by a raw 32-bit Philox word v; small v is the
// tail, the orientation -ln u has.  Words below 32 have a bin each; from 32 on every octave of v
// has 32 bins (the shape of flow_bin with 5 mantissa bits): a pure lookup, integer only, so the
// device and the host (marllb_amd/workload.py, tests/workload_probe.cpp) state the same rule.
// Plain host C++ without the HIP compiler.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LBSIM_TABLE_HD __host__ __device__ __forceinline__
#else
#define LBSIM_TABLE_HD inline
#endif

namespace lbk {

constexpr int kTableBins = 896;  // LBSIM_TABLE_BINS: 32 + 32 * (31 - 4)

LBSIM_TABLE_HD int table_bin(uint32_t v) {
  if (v < 32u) return (int)v;
  const int e = 31 - __builtin_clz(v);
  return 32 * (e - 4) + (int)((v >> (e - 5)) & 31u);
}
// first word of bin k (k = kTableBins: 2^32)
LBSIM_TABLE_HD uint64_t table_bin_lower(int k) {
  return k < 32 ? (uint64_t)k : (uint64_t)(32u + ((uint32_t)k & 31u)) << (k / 32 - 1);
}

}  // namespace lbk
