// dist_walk_check.cpp — the host logic of the read walks across ranks (amg_dist_walk_hdr.h: the argument hash, the verdict
// on the gathered headers, the size of the data exchange) on canned headers, as plain host C++ under AddressSanitizer +
// UBSan: `make -C amira_amd/csrc dist_walk_check`, by hand on a CPU.  No part of `all`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "amg_dist_walk_hdr.h"

#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      fprintf(stderr, "dist_walk_check: line %d: %s does not hold\n", __LINE__, #cond);   \
      exit(1);                                                                             \
    }                                                                                      \
  } while (0)

// `world` blocks of exactly `stride` words on the heap, so that a read beyond a block or the last one is seen
static std::vector<int64_t> blocks_of(int world, int stride, int which, int64_t k, int64_t n, int64_t nodes, int64_t comps,
                                      uint64_t hash) {
  std::vector<int64_t> b((size_t)world * stride, 7777);
  for (int r = 0; r < world; ++r) {
    int64_t* h = b.data() + (size_t)r * stride;
    h[DW_H_WHICH] = which;
    h[DW_H_STATUS] = 0;
    h[DW_H_K] = k;
    h[DW_H_N] = n;
    h[DW_H_NODES] = nodes;
    h[DW_H_COMPS] = comps;
    h[DW_H_HASH] = (int64_t)hash;
    h[DW_H_TWO_V] = 1000;
  }
  return b;
}

int main() {
  char msg[256];
  // ---- the hash: the flags count as 0 / 1, every length and every position counts
  {
    std::vector<uint8_t> f(131, 0), g(131, 0);
    f[0] = 1, g[0] = 200;  // non-zero is non-zero
    f[130] = g[130] = 1;
    const int32_t mg[3] = {3, 5, 1 << 30};
    CHECK(dw_hash_args(f.data(), 131, mg, 3) == dw_hash_args(g.data(), 131, mg, 3));
    g[64] = 1;
    CHECK(dw_hash_args(f.data(), 131, mg, 3) != dw_hash_args(g.data(), 131, mg, 3));
    CHECK(dw_hash_args(f.data(), 131, mg, 3) != dw_hash_args(f.data(), 130, mg, 3));
    CHECK(dw_hash_args(f.data(), 131, mg, 3) != dw_hash_args(f.data(), 131, mg, 2));
    CHECK(dw_hash_args(nullptr, 131, mg, 3) != dw_hash_args(f.data(), 131, mg, 3));
    CHECK(dw_hash_args(f.data(), 131, nullptr, 0) != dw_hash_args(f.data(), 131, mg, 0));
    const int32_t mg2[3] = {3, 5, -1};
    CHECK(dw_hash_args(nullptr, 0, mg, 3) != dw_hash_args(nullptr, 0, mg2, 3));
    for (int n = 0; n <= 130; ++n) (void)dw_hash_args(f.data(), n, nullptr, 0);  // every tail length of the flag words
    std::vector<uint8_t> none;
    (void)dw_hash_args(none.data(), 0, nullptr, 0);
  }
  // ---- first message and data sizes
  CHECK(dw_first_words(DW_DEPTH) == 24 && dw_first_words(DW_AMR_TRIM) == 8 && dw_first_words(DW_COMPONENT_READS) == 8);
  for (int world = 1; world <= 9; ++world)
    for (int which = DW_DEPTH; which <= DW_COMPONENT_READS; ++which) {
      const int stride = dw_first_words(which);
      for (int self = 0; self < world; ++self) {
        std::vector<int64_t> b = blocks_of(world, stride, which, 5, which == DW_DEPTH ? 7 : which == DW_AMR_TRIM ? 0 : 1, 65, 3, 42);
        CHECK(dw_judge(b.data(), world, stride, self, msg, sizeof msg) == 0 && msg[0] == 0);
        // any field of any other rank differing: every rank says no
        for (int r = 0; r < world; ++r)
          for (int f = 0; f < DW_HDR_WORDS; ++f) {
            std::vector<int64_t> c = b;
            c[(size_t)r * stride + f] += f == DW_H_STATUS ? -3 : 1;
            if (world == 1 && f != DW_H_STATUS && f != DW_H_WHICH) continue;  // (one rank agrees with itself)
            const int v = dw_judge(c.data(), world, stride, self, msg, sizeof msg);
            if (world == 1 && f == DW_H_WHICH && which < DW_COMPONENT_READS) continue;  // (another valid walk)
            CHECK(v != 0 && msg[0] != 0 && strlen(msg) < sizeof msg);
          }
      }
    }
  // ---- sizes of the data exchange from an agreed header
  {
    const int64_t nodes[] = {0, 1, 63, 64, 65, 100, 128, (1ll << 29)};
    const int64_t words[] = {0, 1, 1, 1, 2, 2, 2, (1ll << 23)};
    for (int i = 0; i < 8; ++i) {
      std::vector<int64_t> b = blocks_of(1, DW_HDR_WORDS, DW_AMR_TRIM, 3, 0, nodes[i], 0, 1);
      CHECK(dw_judge(b.data(), 1, DW_HDR_WORDS, 0, msg, sizeof msg) == 0);
      CHECK(dw_data_words(b.data()) == words[i]);
      b[DW_H_WHICH] = DW_COMPONENT_READS;
      b[DW_H_COMPS] = nodes[i] / 2;
      CHECK(dw_data_words(b.data()) == 2 * (nodes[i] / 2));
      b[DW_H_WHICH] = DW_DEPTH;
      CHECK(dw_data_words(b.data()) == 0);
    }
  }
  // ---- headers no walk makes, and bad calls
  {
    std::vector<int64_t> b = blocks_of(2, DW_HDR_WORDS, DW_AMR_TRIM, 3, 0, -1, 0, 1);
    CHECK(dw_judge(b.data(), 2, DW_HDR_WORDS, 0, msg, sizeof msg) != 0);
    b = blocks_of(2, DW_HDR_WORDS, DW_COMPONENT_READS, 3, 1, 10, 11, 1);  // more components than nodes
    CHECK(dw_judge(b.data(), 2, DW_HDR_WORDS, 1, msg, sizeof msg) != 0);
    b = blocks_of(2, DW_HDR_WORDS, 9, 3, 1, 10, 1, 1);
    CHECK(dw_judge(b.data(), 2, DW_HDR_WORDS, 1, msg, sizeof msg) != 0);
    b = blocks_of(2, DW_HDR_WORDS, DW_AMR_TRIM, 3, 0, 1ll << 31, 0, 1);
    CHECK(dw_judge(b.data(), 2, DW_HDR_WORDS, 0, msg, sizeof msg) != 0);
    b = blocks_of(2, DW_HDR_WORDS, DW_AMR_TRIM, 3, 0, 10, 0, 1);
    CHECK(dw_judge(b.data(), 2, DW_HDR_WORDS, 2, msg, sizeof msg) != 0);   // self outside the world
    CHECK(dw_judge(b.data(), 2, DW_HDR_WORDS - 1, 0, msg, sizeof msg) != 0);
    CHECK(dw_judge(nullptr, 2, DW_HDR_WORDS, 0, msg, sizeof msg) != 0);
    CHECK(dw_judge(b.data(), 2, DW_HDR_WORDS, 0, nullptr, 0) == 0);         // no room for a message is no fault
    b[DW_HDR_WORDS + DW_H_K] = 5;
    char tiny[8];
    CHECK(dw_judge(b.data(), 2, DW_HDR_WORDS, 0, tiny, sizeof tiny) != 0 && strlen(tiny) < sizeof tiny);
  }
  printf("dist_walk_check: all cases passed\n");
  return 0;
}
