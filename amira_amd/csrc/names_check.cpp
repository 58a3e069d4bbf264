// names_check.cpp — amg_names.h on the host with a main of its own, under AddressSanitizer + UBSan (make names_check, by
// hand on a CPU, no part of `all`): SHA-256 on a published vector, save_long's forms and lengths at their boundaries,
// and whole names of rows over the boundary vocabulary against digests that pickle + hashlib gave (protocols 4 and 5).
#include <cstdio>
#include <cstring>
#include <vector>

#include "amg_names.h"

static int failures = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      ++failures;                            \
      std::printf("FAIL %s:%d ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);              \
      std::printf("\n");                     \
    }                                        \
  } while (0)

struct Big {
  uint8_t b[32];  // big-endian
};
static Big pow2(int n) {
  Big x;
  std::memset(x.b, 0, 32);
  x.b[31 - n / 8] = (uint8_t)(1u << (n % 8));
  return x;
}
static Big add(Big x, int d) {  // d = +1 or -1
  for (int i = 31; i >= 0; --i) {
    const int v = x.b[i] + d;
    x.b[i] = (uint8_t)v;
    if (v >= 0 && v <= 255) break;
  }
  return x;
}
static Big all_ones(int bytes) {
  Big x;
  std::memset(x.b, 0, 32);
  std::memset(x.b + 32 - bytes, 0xff, (size_t)bytes);
  return x;
}

// the 25 magnitudes of tests/names_oracle.py, ascending
static std::vector<Big> boundary_table() {
  std::vector<Big> t;
  Big zero;
  std::memset(zero.b, 0, 32);
  t.push_back(zero);
  t.push_back(pow2(0));
  t.push_back(all_ones(1));
  t.push_back(pow2(8));
  t.push_back(all_ones(2));
  t.push_back(pow2(16));
  t.push_back(add(pow2(31), -1));
  t.push_back(pow2(31));
  t.push_back(add(pow2(31), 1));
  for (int m : {5, 8, 31, 32}) {
    t.push_back(add(pow2(8 * m - 1), -1));
    t.push_back(pow2(8 * m - 1));
    t.push_back(add(pow2(8 * m - 1), 1));
    t.push_back(all_ones(m));
  }
  return t;
}

struct Vector {
  int pp, k;
  int row[17];
  const char* hex;
  long long py_hash;
};
static const Vector kVectors[] = {
    {4, 1, {0}, "06a588f27eee819c492088b8dcca11044a8d52b5ae1d0d6cf31d004c4577674e", 1926319283984878788ll},
    {4, 1, {25}, "aa78b97ad81e995f6cd4b0da37d05bebbb888475dc8bc83a9d1e8c282c295f86", 523458833376715ll},
    {4, 1, {49}, "fefbb3b372acafb04d3af7ce9e971f6e281e93d0316f49daf42c3674979480cd", 1965310527654992824ll},
    {4, 1, {23}, "ca317724c7ebcc1bee8e589c2be18864d5c3d726ee88e6d30222ac997d40dfe3", 1640953397542810672ll},
    {4, 2, {24, 25}, "752056af3e232400c610afea1414d73b2d57b69afebf0acd77431230af274c92", 493742336214137511ll},
    {4, 2, {3, 47}, "9efc2c6b4b2dd8ce9b3600639507edef5ef8b449128cd82cf2c86a0452e2aac1", 1181908790874115878ll},
    {4, 3, {0, 24, 49}, "d03f507c4c9e50e1f8d8b57111d27ab520946ff3fd64a120b2f405e0c8c91d57", 893360200062248090ll},
    {4, 4, {1, 2, 3, 47}, "04360f500b8fc00b4b663c07429a2a92bc11d46a16cf6539b20a846233a03a69", 1749307171497451455ll},
    {4, 5, {10, 20, 30, 40, 45}, "b5d215b67cb85b89a22c175c2450b6f6a1cee8a344ba22608c50dc281cc5cd53", 718716961621261473ll},
    {4, 17, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16},
     "fe0e7692fb730d1bcd98dde800904cc49ae8e6322a54558677c6640393653806", 1311169316664990940ll},
    {5, 1, {0}, "3d08cff3c1642e35788888bd4d01e6a3f5faedede3e1318860d412141ea32bc3", 319078657815662533ll},
    {5, 1, {25}, "dccc43e093347a5f97ed1b8898803afa4c5b3298f89e361330ef82da4a703306", 547111413670571823ll},
    {5, 1, {49}, "9c5501c3ce329a6178366fbb1a7b32bd6eeaff4f472261f8d23fc6dee224da27", 87599998874248703ll},
    {5, 1, {23}, "75239bfda19934b37f456be2439bb7daaa5afdc82c7da0b222be1736f1d351e1", 1020339422276074605ll},
    {5, 2, {24, 25}, "99c5e909d40eeb669e5d159ed5ed113d36f8b0d5fd47921b3150bff7c1de396c", 877570830298902636ll},
    {5, 2, {3, 47}, "257efced9c2fdc13cdb064e1a701831cfabb15f739f6b38029fa057e82bdf7e1", 713196956558329108ll},
    {5, 3, {0, 24, 49}, "d294e1fc77f650a528a29bf4cc7dad35c449cece4f409200c07ec6e95b1bb88a", 1529028693528997243ll},
    {5, 4, {1, 2, 3, 47}, "20ee8f13efcedd9d49ef78a6d5c098f4ceb664de698efc1b9bed2cf415a385e6", 764667990619512985ll},
    {5, 5, {10, 20, 30, 40, 45}, "5ac57e78dcc1366cfc2e05df0544fe105417e84d79caeeda4e5f30ae34e5a2de", 404440598375398762ll},
    {5, 17, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16},
     "71da7d8c101e6fb70f3a88487a390d61685999efb007c525405b6d66766be13f", 487909533617543167ll},
};

static void hex_of(const uint32_t h[8], char out[65]) {
  for (int i = 0; i < 8; ++i) std::snprintf(out + 8 * i, 9, "%08x", h[i]);
}

int main() {
  {  // SHA-256("abc"), FIPS 180-2 appendix B.1
    uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    uint32_t w[16] = {0x61626380u};
    w[15] = 24;
    amg_sha256_block(h, w);
    char hex[65];
    hex_of(h, hex);
    CHECK(!std::strcmp(hex, "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"), "sha256(abc) = %s", hex);
  }
  const std::vector<Big> table = boundary_table();
  CHECK(table.size() == 25, "%zu magnitudes", table.size());
  {  // save_long's form and payload length: value index, sign, form, n
    const struct {
      int at, sign, form, n;
    } want[] = {{0, 1, 0, 1},   {0, -1, 0, 1},  {1, 1, 0, 1},   {1, -1, 2, 4},  {2, 1, 0, 1},    {3, 1, 1, 2},
                {4, 1, 1, 2},   {5, 1, 2, 4},   {6, 1, 2, 4},   {7, 1, 3, 5},   {7, -1, 2, 4},   {8, -1, 3, 5},
                {9, 1, 3, 5},   {10, 1, 3, 6},  {10, -1, 3, 5}, {11, -1, 3, 6}, {12, 1, 3, 6},   {12, -1, 3, 6},
                {21, 1, 3, 32}, {22, 1, 3, 33}, {22, -1, 3, 32}, {23, -1, 3, 33}, {24, 1, 3, 33}, {24, -1, 3, 33}};
    for (const auto& c : want) {
      AmgLong x;
      amg_long_load(table[(size_t)c.at].b, c.sign, &x);
      CHECK(x.form == c.form && x.n == c.n, "value %d sign %d: form %d n %d, want %d %d", c.at, c.sign, x.form, x.n, c.form, c.n);
    }
    AmgLong x;
    amg_long_load(table[10].b, -1, &x);  // -2^39: 00 00 00 00 80, the trailing ff dropped
    CHECK(x.m[0] == 0u && (x.m[1] & 0xffu) == 0x80u, "-2^39 = %08x %08x", x.m[1], x.m[0]);
  }
  uint32_t ring[AMG_NAMES_RING];
  for (const Vector& v : kVectors) {
    int32_t row[17];
    for (int j = 0; j < v.k; ++j) row[j] = v.row[j];
    TokenRow src;
    src.genes = table[0].b, src.V = (int32_t)table.size(), src.tokens = row;
    uint32_t h[8];
    amg_name_of_row(src, v.k, v.pp, ring, h);
    char hex[65];
    hex_of(h, hex);
    CHECK(!std::strcmp(hex, v.hex), "protocol %d k %d first token %d: %s", v.pp, v.k, v.row[0], hex);
    CHECK(amg_py_hash256(h) == v.py_hash, "protocol %d k %d: hash %lld", v.pp, v.k, (long long)amg_py_hash256(h));
  }
  {  // the smaller of two digests as big-endian integers
    const uint32_t a[8] = {1, 0, 0, 0, 0, 0, 0, 9}, b[8] = {1, 0, 0, 0, 0, 0, 1, 0};
    CHECK(amg_digest_less(a, b) && !amg_digest_less(b, a) && !amg_digest_less(a, a), "digest order");
  }
  // a row of 256 entries of the longest form: nothing is written outside the ring (ASan watches the array)
  {
    std::vector<int32_t> row(AMG_NAMES_MAX_K, 2 * (int32_t)table.size() - 1);
    TokenRow src;
    src.genes = table[0].b, src.V = (int32_t)table.size(), src.tokens = row.data();
    uint32_t h[8];
    amg_name_of_row(src, AMG_NAMES_MAX_K, 4, ring, h);
    CHECK(amg_name_body_bytes(src, AMG_NAMES_MAX_K) == 1 + 256 * 35 + 3, "body of 256 longest entries");
  }
  std::printf(failures ? "names_check: %d FAILED\n" : "names_check: ok\n", failures);
  return failures ? 1 : 0;
}
