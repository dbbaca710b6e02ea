// workload_probe.cpp — csrc/lbsim_table.h on the host: table_bin, the bin rule of the workload
// tables, compiled as plain host C++ (tests/test_workload_tables.py compiles and runs it; no GPU).
//
// stdin: one 32-bit word per line (decimal).  stdout: kTableBins, then table_bin of each word, one
// per line.  A word whose bin's first word (table_bin_lower) lies above it, or whose next bin
// starts at or below it, fails the run.
#include <cinttypes>
#include <cstdint>
#include <cstdio>

#include "../marllb_amd/csrc/lbsim_table.h"

int main() {
  printf("%d\n", lbk::kTableBins);
  unsigned long long v;
  int rc = 0;
  while (scanf("%llu", &v) == 1) {
    if (v >> 32) return 2;
    const int k = lbk::table_bin((uint32_t)v);
    if (k < 0 || k >= lbk::kTableBins || lbk::table_bin_lower(k) > v ||
        lbk::table_bin_lower(k + 1) <= v)
      rc = 1;
    printf("%d\n", k);
  }
  return rc;
}
