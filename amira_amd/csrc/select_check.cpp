// select_check.cpp — the host logic of amg_select_reads (amg_select_args.h: the verdict on the arguments, and on the
// allowed table against the longest read) as plain host C++ under AddressSanitizer + UBSan:
// `make -C amira_amd/csrc select_check`, by hand on a CPU.  No part of `all`.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "amg_select_args.h"

#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      fprintf(stderr, "select_check: line %d: %s does not hold\n", __LINE__, #cond);   \
      exit(1);                                                                          \
    }                                                                                   \
  } while (0)

int main() {
  char msg[192];
  // ---- mode range
  for (int mode = -3; mode <= 4; ++mode) {
    const int v = sel_check_args(mode, true, 10, msg, sizeof msg);
    CHECK((v == 0) == (mode == SEL_VALID || mode == SEL_JUNK));
    CHECK((v == 0) == (msg[0] == 0) && strlen(msg) < sizeof msg);
  }
  CHECK(sel_check_args(INT32_MAX, true, 1, msg, sizeof msg) != 0);
  CHECK(sel_check_args(INT32_MIN, true, 1, msg, sizeof msg) != 0);
  // ---- the table: VALID takes none (and ignores one), JUNK needs one with an entry
  CHECK(sel_check_args(SEL_VALID, false, 0, msg, sizeof msg) == 0);
  CHECK(sel_check_args(SEL_VALID, false, -5, msg, sizeof msg) == 0);
  CHECK(sel_check_args(SEL_VALID, true, 7, msg, sizeof msg) == 0);
  CHECK(sel_check_args(SEL_JUNK, false, 7, msg, sizeof msg) != 0 && msg[0] != 0);
  CHECK(sel_check_args(SEL_JUNK, true, 0, msg, sizeof msg) != 0 && msg[0] != 0);
  CHECK(sel_check_args(SEL_JUNK, true, -1, msg, sizeof msg) != 0);
  CHECK(sel_check_args(SEL_JUNK, true, INT64_MIN, msg, sizeof msg) != 0);
  CHECK(sel_check_args(SEL_JUNK, true, 1, msg, sizeof msg) == 0);
  CHECK(sel_check_args(SEL_JUNK, true, INT64_MAX, msg, sizeof msg) == 0);
  // ---- no room for a message is no fault, a small room is not overrun
  CHECK(sel_check_args(9, true, 1, nullptr, 0) != 0);
  CHECK(sel_check_args(9, true, 1, msg, 0) != 0);
  {
    char* tiny = static_cast<char*>(malloc(8));  // on the heap: a write beyond it is seen
    CHECK(sel_check_args(9, true, 1, tiny, 8) != 0 && strlen(tiny) < 8);
    CHECK(sel_check_args(SEL_JUNK, false, 0, tiny, 8) != 0 && strlen(tiny) < 8);
    CHECK(sel_check_table(SEL_JUNK, 100, 100, tiny, 8) != 0 && strlen(tiny) < 8);
    CHECK(sel_check_table(SEL_JUNK, 100, 101, tiny, 8) == 0 && tiny[0] == 0);
    free(tiny);
  }
  // ---- the longest read against n_allowed: allowed[w] is read for w = the read's windows, so n_allowed > w
  const int64_t windows[] = {1, 2, 63, 64, 65, 88, 1ll << 31, INT64_MAX - 1};
  for (int64_t w : windows) {
    CHECK(sel_check_table(SEL_JUNK, w, w + 1, msg, sizeof msg) == 0 && msg[0] == 0);
    CHECK(sel_check_table(SEL_JUNK, w, w, msg, sizeof msg) != 0 && msg[0] != 0 && strlen(msg) < sizeof msg);
    CHECK(sel_check_table(SEL_JUNK, w, 1, msg, sizeof msg) == (w >= 1 ? 1 : 0));
    CHECK(sel_check_table(SEL_VALID, w, 0, msg, sizeof msg) == 0);  // VALID reads no table
  }
  CHECK(sel_check_table(SEL_JUNK, INT64_MAX, INT64_MAX, msg, sizeof msg) != 0);
  // no read is listed (no read, or none with a window): any table will do
  CHECK(sel_check_table(SEL_JUNK, 0, 1, msg, sizeof msg) == 0);
  CHECK(sel_check_table(SEL_JUNK, 0, INT64_MAX, msg, sizeof msg) == 0);
  CHECK(sel_check_table(SEL_JUNK, 5, 6, nullptr, 0) == 0 && sel_check_table(SEL_JUNK, 6, 6, nullptr, 0) != 0);
  printf("select_check: all cases passed\n");
  return 0;
}
