// amg_select_args.h — the verdict on the arguments of amg_select_reads (amg_select.hip), and on the one thing about them
// that only the device can tell: whether the `allowed` table reaches the longest read.  Plain C++ without a HIP header:
// select_check.cpp runs it under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

enum { SEL_VALID = 0, SEL_JUNK = 1 };  // == AMG_SELECT_* (include/amg.h)

// 0: the call may go on; else a message in msg (when there is room for one).  have_allowed: allowed != NULL.
static inline int sel_check_args(int32_t mode, bool have_allowed, int64_t n_allowed, char* msg, size_t cap) {
  if (msg && cap) msg[0] = 0;
  if (mode != SEL_VALID && mode != SEL_JUNK) {
    if (msg && cap) snprintf(msg, cap, "mode %d is neither AMG_SELECT_VALID nor AMG_SELECT_JUNK", (int)mode);
    return 1;
  }
  if (mode == SEL_JUNK && (!have_allowed || n_allowed <= 0)) {
    if (msg && cap) snprintf(msg, cap, "AMG_SELECT_JUNK needs the allowed table (n_allowed > 0)");
    return 1;
  }
  return 0;
}

// allowed[w] is read for every listed read's window count w: the table must hold the longest read's entry.
// max_windows: the most windows a read of the set has (0: no read is listed, any table will do).
static inline int sel_check_table(int32_t mode, int64_t max_windows, int64_t n_allowed, char* msg, size_t cap) {
  if (msg && cap) msg[0] = 0;
  if (mode != SEL_JUNK || max_windows <= 0 || max_windows < n_allowed) return 0;
  if (msg && cap)
    snprintf(msg, cap, "a read has %lld windows, the allowed table ends at %lld (n_allowed must exceed the longest read's windows)",
             (long long)max_windows, (long long)n_allowed - 1);
  return 1;
}
