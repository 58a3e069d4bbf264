// handoff_check.cpp — the refusals that guard scratch hand-offs (finish_kill on KillMarks, fp_list_sort on an FpKeyList)
// on values that do not match the ctx, as a plain host program against libamg.so: `make -C amira_amd/csrc handoff_check`,
// by hand on a CPU.  No part of `all`.  Every call below must return before it touches a device: the ctx is a bare
// struct on the stack, its buffers are host bytes that nothing dereferences.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "amg_internal.h"

#define CHECK(cond)                                                                     \
  do {                                                                                  \
    if (!(cond)) {                                                                      \
      fprintf(stderr, "handoff_check: line %d: %s does not hold\n", __LINE__, #cond);  \
      exit(1);                                                                          \
    }                                                                                   \
  } while (0)

int main() {
  static unsigned char cur[64], old[64];
  amg_ctx c;
  c.n_nodes = 40;
  c.s0.p = cur;
  c.s0.cap = sizeof cur;
  int64_t removed = -1;
  // marks of an allocation the buffer no longer has, of another node count, and none at all
  CHECK(finish_kill(&c, KillMarks{old, 40}, &removed, nullptr) == AMG_E_STATE);
  CHECK(strstr(amg_last_error(), "kill marks") != nullptr);
  CHECK(finish_kill(&c, KillMarks{cur, 39}, &removed, nullptr) == AMG_E_STATE);
  CHECK(finish_kill(&c, KillMarks{cur, 41}, &removed, nullptr) == AMG_E_STATE);
  CHECK(finish_kill(&c, KillMarks(), &removed, nullptr) == AMG_E_STATE);
  c.s0.p = nullptr;  // (a ctx that never reserved any)
  CHECK(finish_kill(&c, KillMarks(), &removed, nullptr) == AMG_E_STATE);
  CHECK(removed == -1);  // nothing was answered

  // a key list whose arrays are not the ctx's current ones: each of the four pointers counts
  static unsigned long long f[8], fs[8];
  static unsigned int s[8], ss[8];
  c.s1.p = f, c.s2.p = fs, c.s3.p = s, c.s4.p = ss;
  const FpKeyList good{f, s, fs, ss, 0};
  for (int i = 0; i < 4; ++i) {
    FpKeyList l = good;
    if (i == 0) l.first = fs;
    if (i == 1) l.slot = ss;
    if (i == 2) l.first_sorted = f;
    if (i == 3) l.slot_sorted = s;
    CHECK(fp_list_sort(&c, l, 8) == AMG_E_STATE);
    CHECK(strstr(amg_last_error(), "key list") != nullptr);
  }
  CHECK(fp_list_sort(&c, FpKeyList(), 8) == AMG_E_STATE);
  printf("handoff_check: all cases passed\n");
  return 0;
}
