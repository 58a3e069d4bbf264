// amg_names.h — THE rule for the 256-bit names of nodes and edges, stated once for the kernel (amg_names.hip), its host
// twin (amg_names_host) and the host checker (names_check.cpp).  No HIP header: plain C++ that hipcc also compiles for
// the device.
//
// A name is SHA-256 of pickle.dumps(tuple of k signed 256-bit ints) (construct_gene_mer.py:94-97, construct_edge.py:
// 104-124).  An entry of the tuple is a 32-byte big-endian digest of some table with a sign: a gene's hash for a node,
// a node's name for an edge.  The message:
//     80 pp | 95 <u64 LE len(body)> | body          pp = pickle protocol 4 or 5
//     body = [28 if k > 3] | enc(x_1) .. enc(x_k) | (85 / 86 / 87 for k = 1 / 2 / 3, 74 for k > 3) | 94 | 2e
// enc(x) is CPython's save_long: 4b b (0 <= x < 256), 4d u16 (x < 65536), 4a i32 (-2^31 <= x < 2^31), else 8a n and n
// bytes little-endian two's complement, n = (bit_length(|x|) >> 3) + 1, less one for x < 0 when the last byte is ff and
// the one before it has its top bit set.  A tuple that holds the same int twice is not memoised.
//
// How a lane makes a name: NameStream writes the message piece by piece (the frame header, one entry, the tuple's end
// with SHA's 80, SHA's padding with the bit length) as big-endian dwords into a ring of 32 dwords of its own, and
// compresses 16 of them whenever 16 are complete.  A piece is at most 17 dwords and is only written while fewer than 16
// are pending, so the ring never overflows; the loop "fill, then compress if 16 are pending" is the same for every lane
// of a wave whatever the lengths of its entries, which keeps the compression wave-uniform.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AMG_HD __host__ __device__ inline
#else
#define AMG_HD inline
#endif

#define AMG_NAMES_MAX_K 256
#define AMG_NAMES_RING 32  // dwords of a lane's ring: two SHA blocks

AMG_HD uint32_t amg_rotr(uint32_t x, int n) { return __builtin_rotateright32(x, (uint32_t)n); }
AMG_HD uint32_t amg_bswap(uint32_t x) { return __builtin_bswap32(x); }

// one SHA-256 compression of the 16 big-endian message words w[0 .. 16) into h[0 .. 8).  The rounds are unrolled over a
// 16-word schedule: every index below is a compile-time constant once unrolled, so the schedule stays in registers.
AMG_HD void amg_sha256_block(uint32_t h[8], const uint32_t* wsrc) {
  constexpr uint32_t K[64] = {
      0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
      0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
      0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
      0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
      0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
      0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
      0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
      0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = wsrc[i];
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    if (t >= 16) {
      const uint32_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
      const uint32_t s0 = amg_rotr(w15, 7) ^ amg_rotr(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = amg_rotr(w2, 17) ^ amg_rotr(w2, 19) ^ (w2 >> 10);
      w[t & 15] += s0 + w[(t + 9) & 15] + s1;
    }
    const uint32_t S1 = amg_rotr(e, 6) ^ amg_rotr(e, 11) ^ amg_rotr(e, 25);
    const uint32_t ch = (e & f) ^ (~e & g);
    const uint32_t t1 = hh + S1 + ch + K[t] + w[t & 15];
    const uint32_t S0 = amg_rotr(a, 2) ^ amg_rotr(a, 13) ^ amg_rotr(a, 22);
    const uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
    const uint32_t t2 = S0 + mj;
    hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
  }
  h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
}

// a signed entry as enc() needs it: the magnitude as nine little-endian dwords in two's complement (m[8] is the sign
// extension: byte 32 of a LONG1 of 33 bytes), its bit length, and what save_long makes of it
struct AmgLong {
  uint32_t m[9];
  int form;  // 0: 4b b, 1: 4d u16, 2: 4a i32, 3: 8a n bytes
  int n;     // payload bytes behind the opcode (form 3: behind 8a n)
};
// bytes of enc(x): opcode, (form 3: the length byte,) payload
AMG_HD int amg_long_bytes(const AmgLong& x) { return x.n + (x.form == 3 ? 2 : 1); }

// digest: 32 bytes big-endian at a 4-byte boundary; sign: > 0 or < 0 (a magnitude of zero has no sign)
AMG_HD void amg_long_load(const uint8_t* digest, int sign, AmgLong* x) {
  const uint8_t* d = static_cast<const uint8_t*>(__builtin_assume_aligned(digest, 4));
  uint32_t mag[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    uint32_t w;
    __builtin_memcpy(&w, d + 4 * (7 - i), 4);
    mag[i] = amg_bswap(w);
  }
  int bits = 0;  // bit_length(|x|)
  bool pow2 = false;  // |x| is a power of two
  {
    int words = 0;  // non-zero words
    uint32_t top = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (mag[i]) {
        ++words;
        top = mag[i];
        bits = 32 * i + (32 - __builtin_clz(mag[i]));
      }
    pow2 = words == 1 && (top & (top - 1)) == 0;
  }
  const bool neg = sign < 0 && bits > 0;
  if (neg) {  // ~byte + carry, the carry running from the least significant end: the order LONG1 emits
    uint32_t carry = 1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t v = ~mag[i] + carry;
      carry = (carry && v == 0) ? 1u : 0u;
      mag[i] = v;
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) x->m[i] = mag[i];
  x->m[8] = neg ? 0xffffffffu : 0u;
  if (!neg && bits <= 8)
    x->form = 0, x->n = 1;
  else if (!neg && bits <= 16)
    x->form = 1, x->n = 2;
  else if (bits <= 31 || (neg && bits == 32 && pow2))
    x->form = 2, x->n = 4;  // -2^31 <= x < 2^31
  else {
    x->form = 3;
    x->n = (bits >> 3) + 1;
    // x < 0, n > 1, last byte ff and the top bit of the one before it set: only |x| = 2^(8m - 1) does that
    if (neg && (bits & 7) == 0 && pow2) x->n -= 1;
  }
}

// Python's hash() of the name (a non-negative int): the digest mod 2^61 - 1, by folding 61-bit limbs (2^61 = 1 mod M)
AMG_HD int64_t amg_py_hash256(const uint32_t h[8]) {
  const uint64_t M = (1ull << 61) - 1;
  const uint64_t q3 = ((uint64_t)h[0] << 32) | h[1], q2 = ((uint64_t)h[2] << 32) | h[3];
  const uint64_t q1 = ((uint64_t)h[4] << 32) | h[5], q0 = ((uint64_t)h[6] << 32) | h[7];
  uint64_t s = (q0 & M) + (((q0 >> 61) | (q1 << 3)) & M) + (((q1 >> 58) | (q2 << 6)) & M) +
               (((q2 >> 55) | (q3 << 9)) & M) + (q3 >> 52);
  s = (s & M) + (s >> 61);
  if (s >= M) s -= M;
  return (int64_t)s;
}

// true when the digest a is below b, both as big-endian unsigned integers (word 0 is the most significant)
AMG_HD bool amg_digest_less(const uint32_t a[8], const uint32_t b[8]) {
  bool less = false, decided = false;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (!decided && a[i] != b[i]) less = a[i] < b[i], decided = true;
  }
  return less;
}

// The message of one name, written through a ring of AMG_NAMES_RING dwords and compressed block by block.
// Src: entry(j, &digest, &sign) gives entry j of the row.
struct NameStream {
  enum Stage { HEADER = 0, ENTRY = 1, TAIL = 2, PAD = 3, END = 4 };
  uint32_t h[8];
  uint32_t* ring;     // the lane's own AMG_NAMES_RING dwords
  uint64_t acc;       // bytes not yet a whole dword, in its low 8 * acc_n bits
  uint32_t acc_n;     // 0 .. 3
  uint32_t wr, rd;    // dwords written / compressed so far (ring positions are these & (AMG_NAMES_RING - 1))
  uint32_t stage, j;  // the next piece; j: the next entry
  uint32_t k, pp;
  uint64_t msg_bytes;

  // `count` bytes, the first in the most significant of the low 8 * count bits of v; count in [1, 4]
  AMG_HD void put(uint32_t v, uint32_t count) {
    acc = (acc << (8 * count)) | v;
    acc_n += count;
    if (acc_n >= 4) {
      acc_n -= 4;
      ring[wr & (AMG_NAMES_RING - 1)] = (uint32_t)(acc >> (8 * acc_n));
      ++wr;
    }
  }
  AMG_HD void put_dword(uint32_t v) {
    ring[wr & (AMG_NAMES_RING - 1)] = v;
    ++wr;
  }

  // body_bytes: len(body), which the frame header states before the first entry (amg_name_body_bytes)
  AMG_HD void begin(uint32_t* ring_, uint32_t k_, uint32_t pp_, uint64_t body_bytes, bool active) {
    h[0] = 0x6a09e667u, h[1] = 0xbb67ae85u, h[2] = 0x3c6ef372u, h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu, h[5] = 0x9b05688cu, h[6] = 0x1f83d9abu, h[7] = 0x5be0cd19u;
    ring = ring_, acc = 0, acc_n = 0, wr = rd = 0, j = 0, k = k_, pp = pp_;
    msg_bytes = 11 + body_bytes;
    stage = active ? HEADER : END;
  }
  AMG_HD bool done() const { return stage == END && wr == rd; }

  template <class Src>
  AMG_HD void piece(const Src& src) {
    if (stage == HEADER) {
      const uint64_t body = msg_bytes - 11;
      put(0x8000u | pp, 2);
      put(0x95u, 1);
      put(amg_bswap((uint32_t)body), 4);  // u64 little-endian: low dword first, each byte-reversed into stream order
      put(amg_bswap((uint32_t)(body >> 32)), 4);
      if (k > 3) put(0x28u, 1);
      stage = ENTRY;
    } else if (stage == ENTRY) {
      const uint8_t* digest;
      int sign;
      src.entry((int)j, &digest, &sign);
      AmgLong x;
      amg_long_load(digest, sign, &x);
      if (x.form == 0)
        put(0x4b00u | (x.m[0] & 0xffu), 2);
      else if (x.form == 1)
        put(0x4d0000u | ((x.m[0] & 0xffu) << 8) | ((x.m[0] >> 8) & 0xffu), 3);
      else if (x.form == 2) {
        put(0x4au, 1);
        put(amg_bswap(x.m[0]), 4);
      } else {
        put(0x8a00u | (uint32_t)x.n, 2);
        const int n = x.n;
#pragma unroll
        for (int i = 0; i < 8; ++i)
          if (n >= 4 * i + 4) put(amg_bswap(x.m[i]), 4);
        // what is left of the last dword: 0 .. 3 bytes (n = 33: the sign byte of m[8])
        const int rest = n & 3;
        uint32_t last = 0;
#pragma unroll
        for (int i = 0; i < 9; ++i)
          if ((n >> 2) == i) last = x.m[i];
        if (rest) put(amg_bswap(last) >> (8 * (4 - rest)), (uint32_t)rest);
      }
      if (++j == k) stage = TAIL;
    } else if (stage == TAIL) {
      put(k == 1 ? 0x85u : k == 2 ? 0x86u : k == 3 ? 0x87u : 0x74u, 1);
      put(0x942e80u, 3);  // MEMOIZE, STOP, and SHA's first padding byte
      if (acc_n) put(0u, 4 - acc_n);  // zero bytes up to the dword boundary
      stage = PAD;
    } else if (stage == PAD) {
      while ((wr & 15) != 14) put_dword(0u);
      const uint64_t bits = msg_bytes * 8;
      put_dword((uint32_t)(bits >> 32));
      put_dword((uint32_t)bits);
      stage = END;
    }
  }
  // pieces while fewer than 16 dwords are pending
  template <class Src>
  AMG_HD void fill(const Src& src) {
    while (wr - rd < 16 && stage != END) piece(src);
  }
  AMG_HD void compress_if_full() {
    if (wr - rd >= 16) {
      amg_sha256_block(h, ring + (rd & (AMG_NAMES_RING - 1)));
      rd += 16;
    }
  }
};

// len(body) of a row: the entries are looked at once for their lengths, before the first byte is written
template <class Src>
AMG_HD uint64_t amg_name_body_bytes(const Src& src, int k) {
  uint64_t n = (k > 3 ? 1 : 0) + 3;  // MARK, the tuple opcode, MEMOIZE, STOP
  for (int j = 0; j < k; ++j) {
    const uint8_t* digest;
    int sign;
    src.entry(j, &digest, &sign);
    AmgLong x;
    amg_long_load(digest, sign, &x);
    n += (uint64_t)amg_long_bytes(x);
  }
  return n;
}

// ---- the two kinds of rows
// a row of k tokens over the gene table G[n_genes][32]: token t >= V is +G[t - V], below it -G[V - 1 - t]
struct TokenRow {
  const uint8_t* genes;
  const int32_t* tokens;
  int32_t V;
  AMG_HD void entry(int j, const uint8_t** digest, int* sign) const {
    const int32_t t = tokens[j];
    *digest = genes + 32 * (int64_t)(t >= V ? t - V : V - 1 - t);
    *sign = t >= V ? 1 : -1;
  }
};
// (s, t) or (-s, -t) of an edge: two names with their directions, times `flip`
struct PairRow {
  const uint8_t* two_names;  // [2][32]: source, target
  int sdir, tdir, flip;
  AMG_HD void entry(int j, const uint8_t** digest, int* sign) const {
    *digest = two_names + 32 * j;
    *sign = (j ? tdir : sdir) * flip;
  }
};

// one name start to end in one lane's own loop (the host twin, the checker; the kernel runs the same three calls with a
// wave-wide loop condition)
template <class Src>
AMG_HD void amg_name_of_row(const Src& src, int k, int pp, uint32_t* ring, uint32_t out[8]) {
  NameStream s;
  s.begin(ring, (uint32_t)k, (uint32_t)pp, amg_name_body_bytes(src, k), true);
  while (!s.done()) {
    s.fill(src);
    s.compress_if_full();
  }
  for (int i = 0; i < 8; ++i) out[i] = s.h[i];
}
