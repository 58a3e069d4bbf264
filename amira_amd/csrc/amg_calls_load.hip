// amg_calls_load.hip — native front-end, host code only.
//
// The hot path's input is the gene-call JSON that Amira itself dumps and reloads
// (gene_calls_with_gene_filtering.json / corrected_gene_calls.json: {"read": ["+geneA", ...]},
// reference __main__.py:464-496, result_utils.py:1260-1264) plus the matching gene-position
// JSON ({"read": [[start, end], ...]}).  Turning that into CSR tokens in Python costs ~10 s
// per 60 M genes; this does it natively:
//   * a small strict JSON reader for exactly these two shapes (strings with escapes, integers);
//   * gene parsing as construct_gene.py:49-65 (strand = first char, ' ' -> '_' in the name);
//   * the reference's gene hash: sha256(pickle.dumps(name)) with pickle protocol 4 framing
//     (80 04 95 <len8> 8c <n> <utf8> 94 2e, or 58 <len4> for names of 256+ bytes),
//     construct_gene.py:5-10 — computed once per DISTINCT name;
//   * ranks by ascending hash -> tokens (amira_amd/tokens.py: V + rank / V - 1 - rank).
// Checked bit for bit against the Python path in tests/test_calls_cpu.py (no GPU needed).
#include <algorithm>
#include <memory>

#include <sys/mman.h>

#include "amg_calls.h"

namespace amgc {
// ------------------------------------------------------------------ SHA-256 (FIPS 180-4)
static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
static void sha256_block(uint32_t h[8], const uint8_t* p) {
  static const uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
      0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
      0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
      0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
      0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
      0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
      0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  uint32_t w[64];
  for (int i = 0; i < 16; ++i)
    w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
  for (int i = 16; i < 64; ++i) {
    uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3);
    uint32_t s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
    w[i] = w[i - 16] + s0 + w[i - 7] + s1;
  }
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
  for (int i = 0; i < 64; ++i) {
    uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25), ch = (e & f) ^ (~e & g);
    uint32_t t1 = hh + S1 + ch + K[i] + w[i];
    uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22), mj = (a & b) ^ (a & c) ^ (b & c);
    uint32_t t2 = S0 + mj;
    hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}
void sha256(const uint8_t* p, size_t n, uint8_t out[32]) {
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  size_t at = 0;
  for (; at + 64 <= n; at += 64) sha256_block(h, p + at);
  // the rest, the 0x80 byte, zeros and the length in bits at the end of a block: one block, or two when the rest is long
  uint8_t tail[128] = {};
  const size_t rest = n - at, padded = rest < 56 ? 64 : 128;
  if (rest) memcpy(tail, p + at, rest);
  tail[rest] = 0x80;
  for (int i = 0; i < 8; ++i) tail[padded - 1 - i] = (uint8_t)((uint64_t)n * 8 >> (8 * i));
  for (size_t b = 0; b < padded; b += 64) sha256_block(h, tail + b);
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 4; ++j) out[4 * i + j] = (uint8_t)(h[i] >> (24 - 8 * j));
}

void gene_hash(const std::string& name, uint8_t out[32]) {
  const bool small = name.size() < 256;
  std::string msg("\x80\x04\x95", 3);  // PROTO 4, FRAME: the bytes that follow, in 8 bytes
  const uint64_t frame = (small ? 2 : 5) + name.size() + 2;
  for (int i = 0; i < 8; ++i) msg.push_back((char)(frame >> (8 * i)));
  msg.push_back(small ? (char)0x8c : 'X');  // SHORT_BINUNICODE with its length in 1 byte, BINUNICODE in 4
  for (int i = 0; i < (small ? 1 : 4); ++i) msg.push_back((char)((uint32_t)name.size() >> (8 * i)));
  msg += name;
  msg.push_back((char)0x94);  // MEMOIZE
  msg.push_back('.');         // STOP
  sha256(reinterpret_cast<const uint8_t*>(msg.data()), msg.size(), out);
}

// ------------------------------------------------------------------ the JSON reader's strings with escapes
static void utf8(std::string& s, uint32_t cp) {
  if (cp < 0x80) s.push_back((char)cp);
  else if (cp < 0x800) { s.push_back((char)(0xC0 | cp >> 6)); s.push_back((char)(0x80 | (cp & 0x3F))); }
  else if (cp < 0x10000) {
    s.push_back((char)(0xE0 | cp >> 12)); s.push_back((char)(0x80 | ((cp >> 6) & 0x3F)));
    s.push_back((char)(0x80 | (cp & 0x3F)));
  } else {
    s.push_back((char)(0xF0 | cp >> 18)); s.push_back((char)(0x80 | ((cp >> 12) & 0x3F)));
    s.push_back((char)(0x80 | ((cp >> 6) & 0x3F))); s.push_back((char)(0x80 | (cp & 0x3F)));
  }
}
static bool hex4(const char*& p, const char* end, uint32_t* v) {
  if (end - p < 4) return false;
  uint32_t x = 0;
  for (int i = 0; i < 4; ++i) {
    char c = p[i];
    x <<= 4;
    if (c >= '0' && c <= '9') x |= c - '0';
    else if (c >= 'a' && c <= 'f') x |= c - 'a' + 10;
    else if (c >= 'A' && c <= 'F') x |= c - 'A' + 10;
    else return false;
  }
  p += 4;
  *v = x;
  return true;
}
bool Reader::str(std::string& out) {
  ws();
  if (p >= end || *p != '"') { err = "expected string"; return false; }
  ++p;
  out.clear();
  while (p < end && *p != '"') {
    if (*p != '\\') { out.push_back(*p++); continue; }
    if (++p >= end) break;
    char c = *p++;
    switch (c) {
      case 'n': out.push_back('\n'); break;
      case 't': out.push_back('\t'); break;
      case 'r': out.push_back('\r'); break;
      case 'b': out.push_back('\b'); break;
      case 'f': out.push_back('\f'); break;
      case 'u': {
        uint32_t cp;
        if (!hex4(p, end, &cp)) { err = "bad \\u escape"; return false; }
        if (cp >= 0xD800 && cp < 0xDC00 && end - p >= 6 && p[0] == '\\' && p[1] == 'u') {
          const char* save = p;
          p += 2;
          uint32_t lo;
          if (hex4(p, end, &lo) && lo >= 0xDC00 && lo < 0xE000) cp = 0x10000 + ((cp - 0xD800) << 10) + (lo - 0xDC00);
          else p = save;
        }
        utf8(out, cp);
        break;
      }
      default: out.push_back(c);  // \" \\ \/
    }
  }
  if (p >= end) { err = "unterminated string"; return false; }
  ++p;
  return true;
}

// ------------------------------------------------------------------ the name table's slots
void Interner::rehash(size_t new_size) {
  slots.assign(new_size, -1);
  mask = new_size - 1;
  for (size_t id = 0; id < off.size(); ++id) {
    size_t s = hash(at(id), len[id]) & mask;
    while (slots[s] >= 0) s = (s + 1) & mask;
    slots[s] = (int32_t)id;
  }
}
void Interner::reserve(size_t n_items, size_t n_bytes) {
  size_t want = slots.size();
  while (want < n_items * 2 + 2) want *= 4;
  if (want != slots.size()) rehash(want);
  arena.reserve(n_bytes);
  off.reserve(n_items);
  len.reserve(n_items);
}
}  // namespace amgc

namespace {
using namespace amgc;

// ------------------------------------------------------------------ one driver for the two parsers
// why a piece did not parse, and where in the file
struct PartError {
  std::string error;  // empty: the piece parsed
  long long error_at = 0;
  bool fail(Reader& r, const char* what, const char* file_begin) {
    error = std::string(what) + (r.err.empty() ? "" : (": " + r.err));
    error_at = (long long)(r.p - file_begin);
    return false;
  }
};

// the file in memory; [*begin, *end) = what lies between its outer braces, an object of read -> `what`
int object_body(FileView& file, const char* path, const char* what, const char** begin, const char** end) {
  std::string err;
  if (!file.open(path, err)) return amg_fail(AMG_E_ARG, "%s", err.c_str());
  const char* fb = file.data;
  Reader outer{fb, fb + file.size, ""};
  if (!outer.lit('{')) return amg_fail(AMG_E_ARG, "%s: expected an object of read -> %s (offset %lld)", path, what, (long long)(outer.p - fb));
  const char* e = fb + file.size;
  while (e > outer.p && is_json_blank(e[-1])) --e;
  if (e <= outer.p || e[-1] != '}') return amg_fail(AMG_E_ARG, "%s: expected '}' (offset %lld)", path, (long long)(e - fb));
  *begin = outer.p;
  *end = e - 1;
  return AMG_OK;
}

// Cut the body of a {"key": [...], "key": [...]} object into `want` pieces at entry boundaries, found by their bytes as
// json.dumps writes them: `], "` — the bracket that closes one entry's list, the comma, the quote that opens the next
// key.  Inside a JSON string a quote is always escaped, so these four bytes can only MISLEAD when a string ends with
// `], ` right before its closing quote; every piece is then parsed on its own terms and must consume exactly its bytes —
// a cut in the wrong place fails that parse and the caller falls back to the single-threaded path.  A file written
// with other separators simply yields one piece.  Pieces: [begin, end) with begin at a key's opening quote.
std::vector<std::pair<const char*, const char*>> split_entries(const char* b, const char* e, int want) {
  std::vector<std::pair<const char*, const char*>> out;
  const char* at = b;
  const size_t total = (size_t)(e - b);
  for (int i = 1; i < want && at < e; ++i) {
    const char* nominal = b + total / want * i;
    if (nominal <= at) continue;
    const char* q = nominal;
    const char* cut = nullptr;
    while (q + 4 <= e) {
      q = static_cast<const char*>(memchr(q, ']', (size_t)(e - q - 3)));
      if (!q) break;
      if (q[1] == ',' && q[2] == ' ' && q[3] == '"') { cut = q; break; }
      ++q;
    }
    if (!cut) break;
    out.emplace_back(at, cut + 1);
    at = cut + 3;
  }
  out.emplace_back(at, e);
  return out;
}

// The pieces of [b, e), one thread each: reset(n) makes ready for an attempt with n pieces, parse_piece(i, reader,
// error) parses piece i.  A piece that does not parse on its own terms sends everything down the single-threaded path
// (whose error message, if the file is really malformed, names the true offset).  Returns that error, or an empty one.
template <class Parse, class Reset>
PartError parse_in_pieces(const char* b, const char* e, Parse parse_piece, Reset reset) {
  for (int attempt = 0;; ++attempt) {
    const auto pieces = split_entries(b, e, attempt == 0 ? worker_count((size_t)(e - b)) : 1);
    std::vector<PartError> errors(pieces.size());
    reset(pieces.size());
    run_parts(pieces.size(), [&](size_t i) {
      Reader r{pieces[i].first, pieces[i].second, ""};
      parse_piece(i, r, errors[i]);
    });
    const auto bad = std::find_if(errors.begin(), errors.end(), [](const PartError& x) { return !x.error.empty(); });
    if (bad == errors.end()) return PartError();
    if (pieces.size() == 1) return *bad;
  }
}

// ------------------------------------------------------------------ gene calls
// what one thread makes of its piece of the file (on cache lines of its own: every gene moves the ends of gid and strand)
struct alignas(64) CallsPart {
  Interner ids;                 // read ids of the piece, in file order
  std::vector<int64_t> n_genes; // per read
  Interner genes;               // gene names, local first-seen ids
  std::vector<int32_t> gid;     // per gene occurrence: LOCAL name id
  std::vector<int8_t> strand;
  bool blanks = false;          // a gene name held a blank (stored with '_' in its place, construct_gene.py:54-56)
};

// the reference's complaint about the gene string [b, e), strand character first (construct_gene.py:49-65), or null
const char* check_gene(const char* b, const char* e, bool all_blank) {
  if (all_blank) return "Gene information is missing";
  if (*b != '+' && *b != '-') return "Strand information missing for a gene";
  if (e - b < 2) return "Gene name information missing for a gene";
  return nullptr;
}

// one gene string -> its strand and its LOCAL name id, appended to the part
bool parse_gene(Reader& r, CallsPart& part, PartError& pe, const char* file_begin, std::string& owned, std::string& fixed) {
  // one pass over the gene string: closing quote, escapes, blanks and the hash of the name
  // (construct_gene.py:49-65: strand = first char, name = rest with ' ' -> '_')
  r.ws();
  if (r.p >= r.end || *r.p != '"') { r.err = "expected string"; return pe.fail(r, "gene", file_begin); }
  const char* gb = r.p + 1;
  const char* q = gb;
  uint64_t hsh = Fnv1a::start();
  bool blank = true, has_space = false, plain = true;
  if (q < r.end && *q != '"' && *q != '\\') { blank = blank && *q == ' '; ++q; }  // strand char: not hashed
  while (q < r.end && *q != '"') {
    const char ch = *q;
    if (ch == '\\') { plain = false; break; }
    if (ch == ' ') has_space = true; else blank = false;
    hsh = Fnv1a::step(hsh, (unsigned char)(ch == ' ' ? '_' : ch));
    ++q;
  }
  const char* ge;
  int32_t id;
  if (plain && q < r.end) {
    ge = q;
    r.p = q + 1;
    if (const char* what = check_gene(gb, ge, blank)) return pe.fail(r, what, file_begin);
    hsh = Fnv1a::finish(hsh);
    if (!has_space) {
      id = part.genes.intern_h(gb + 1, (size_t)(ge - gb - 1), hsh);
    } else {
      fixed.assign(gb + 1, ge);
      std::replace(fixed.begin(), fixed.end(), ' ', '_');
      id = part.genes.intern_h(fixed.data(), fixed.size(), hsh);
    }
  } else {  // escapes (or a truncated file): the general string reader
    if (!r.str(owned)) return pe.fail(r, "gene", file_begin);
    gb = owned.data();
    ge = gb + owned.size();
    has_space = owned.find(' ') != std::string::npos;
    if (const char* what = check_gene(gb, ge, owned.find_first_not_of(' ') == std::string::npos)) return pe.fail(r, what, file_begin);
    fixed.assign(gb + 1, ge);
    std::replace(fixed.begin(), fixed.end(), ' ', '_');
    id = part.genes.intern(fixed.data(), fixed.size());
  }
  if (has_space) part.blanks = true;
  part.gid.push_back(id);
  part.strand.push_back(*gb == '+' ? 1 : -1);
  return true;
}

// entries `"read": ["+gene", ...]` separated by commas, up to the end of the reader's range (which must be reached)
bool parse_call_entries(Reader& r, CallsPart& part, PartError& pe, const char* file_begin) {
  std::string key, owned, fixed;
  r.ws();
  if (r.p >= r.end) return true;
  do {
    const char *kb, *ke;
    if (!r.str_view(&kb, &ke, &key)) return pe.fail(r, "read id", file_begin);
    {
      // json.load keeps the LAST value of a duplicated key at the FIRST key's position;
      // gene-call files never repeat a read id, so this is rejected rather than emulated
      const size_t before = part.ids.size();
      const int32_t rid = part.ids.intern(kb, (size_t)(ke - kb));
      if ((size_t)rid != before) return pe.fail(r, "duplicate read id", file_begin);
    }
    if (!r.lit(':') || !r.lit('[')) return pe.fail(r, "expected ': ['", file_begin);
    const size_t first_gene = part.gid.size();
    if (!r.lit(']')) {
      do {
        if (!parse_gene(r, part, pe, file_begin, owned, fixed)) return false;
      } while (r.lit(','));
      if (!r.lit(']')) return pe.fail(r, "expected ']'", file_begin);
    }
    part.n_genes.push_back((int64_t)(part.gid.size() - first_gene));
  } while (r.lit(','));
  r.ws();
  if (r.p != r.end) return pe.fail(r, "expected ',' or the end of the object", file_begin);
  return true;
}

// ---- the five steps of amg_calls_load_json
PartError parse_pieces(const char* b, const char* e, const char* file_begin, std::vector<CallsPart>& parts) {
  auto parse = [&](size_t i, Reader& r, PartError& pe) {
    parts[i].gid.reserve((size_t)(r.end - r.p) / 8);
    parts[i].strand.reserve((size_t)(r.end - r.p) / 8);
    parse_call_entries(r, parts[i], pe, file_begin);
  };
  return parse_in_pieces(b, e, parse, [&](size_t n) { parts.clear(); parts.resize(n); });
}

void reserve_read_ids(const std::vector<CallsPart>& parts, amg_calls* c) {
  size_t n_ids = 0, id_bytes = 0;
  for (auto& p : parts) {
    n_ids += p.ids.size();
    id_bytes += p.ids.arena.size();
  }
  c->read_ids.reserve(n_ids, id_bytes);
  c->read_off.reserve(n_ids + 1);
}

// read ids in file order (one table for the whole file: a read id must not repeat), read offsets; false: *repeated
bool merge_read_ids(const std::vector<CallsPart>& parts, amg_calls* c, std::string* repeated) {
  for (auto& p : parts) {
    c->blanks = c->blanks || p.blanks;
    for (size_t i = 0; i < p.ids.size(); ++i) {
      const size_t before = c->read_ids.size();
      const int32_t rid = c->read_ids.intern(p.ids.at(i), p.ids.len[i]);
      if ((size_t)rid != before) { *repeated = p.ids.name(i); return false; }
      c->read_off.push_back(c->read_off.back() + p.n_genes[i]);
    }
  }
  return true;
}

// gene names of all pieces -> one table
struct GeneTable {
  Interner genes;
  std::vector<std::vector<int32_t>> to_global;  // per piece: local name id -> id in `genes`
};
void merge_gene_tables(const std::vector<CallsPart>& parts, GeneTable& t) {
  t.to_global.resize(parts.size());
  for (size_t k = 0; k < parts.size(); ++k) {
    auto& p = parts[k];
    t.to_global[k].resize(p.genes.size());
    for (size_t i = 0; i < p.genes.size(); ++i) t.to_global[k][i] = t.genes.intern(p.genes.at(i), p.genes.len[i]);
  }
}

// hash every distinct name once, rank by hash: fills c->names and c->hashes, returns id in `genes` -> rank
std::vector<int32_t> rank_by_hash(const Interner& genes, amg_calls* c) {
  const size_t V = genes.size();
  std::vector<std::string> names_seen(V);
  for (size_t i = 0; i < V; ++i) names_seen[i] = genes.name(i);
  std::vector<uint8_t> h(V * 32);
  const size_t workers = (size_t)std::max(1, std::min(worker_count(V * 4096), (int)((V + 255) / 256)));
  run_parts(workers, [&](size_t w) {
    for (size_t i = w; i < V; i += workers) gene_hash(names_seen[i], &h[i * 32]);
  });
  std::vector<int32_t> order(V);
  for (size_t i = 0; i < V; ++i) order[i] = (int32_t)i;
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
    int cmp = memcmp(&h[(size_t)a * 32], &h[(size_t)b * 32], 32);  // big-endian digest == integer order
    return cmp != 0 ? cmp < 0 : a < b;
  });
  std::vector<int32_t> rank(V);
  c->names.resize(V);
  c->hashes.resize(V * 32);
  for (size_t rnk = 0; rnk < V; ++rnk) {
    rank[order[rnk]] = (int32_t)rnk;
    c->names[rnk] = names_seen[order[rnk]];
    memcpy(&c->hashes[rnk * 32], &h[(size_t)order[rnk] * 32], 32);
  }
  return rank;
}

// tokens, every piece into its own stretch
void emit_tokens(const std::vector<CallsPart>& parts, const GeneTable& t, const std::vector<int32_t>& rank, amg_calls* c) {
  const int32_t Vp = (int32_t)(rank.empty() ? 1 : rank.size());
  std::vector<size_t> base(parts.size() + 1, 0);
  for (size_t k = 0; k < parts.size(); ++k) base[k + 1] = base[k] + parts[k].gid.size();
  c->tokens.resize(base.back());
  run_parts(parts.size(), [&](size_t k) {
    const auto& p = parts[k];
    int32_t* dst = c->tokens.data() + base[k];
    const int32_t* g2 = t.to_global[k].data();
    for (size_t i = 0; i < p.gid.size(); ++i) {
      const int32_t r = rank[g2[p.gid[i]]];
      dst[i] = p.strand[i] > 0 ? Vp + r : Vp - 1 - r;
    }
  });
}
}  // namespace

extern "C" int amg_calls_load_json(const char* path, amg_calls** out) {
  if (!path || !out) return amg_fail(AMG_E_ARG, "null argument");
  *out = nullptr;
  FileView file;
  const char *body_b, *body_e;
  if (int rc = object_body(file, path, "gene list", &body_b, &body_e)) return rc;
  const PhaseClock phase;
  std::vector<CallsPart> parts;
  const PartError bad = parse_pieces(body_b, body_e, file.data, parts);
  if (!bad.error.empty()) return amg_fail(AMG_E_ARG, "%s: %s (offset %lld)", path, bad.error.c_str(), bad.error_at);
  phase.note("parse %.3fs cpu %.3fs wall, %zu piece(s)\n", phase.cpu(), phase.wall(), parts.size());
  std::unique_ptr<amg_calls> c(new amg_calls());
  reserve_read_ids(parts, c.get());
  phase.note("  ids reserved %.3fs wall\n", phase.wall());
  std::string repeated;
  if (!merge_read_ids(parts, c.get(), &repeated)) return amg_fail(AMG_E_ARG, "%s: duplicate read id %s", path, repeated.c_str());
  phase.note("  ids merged %.3fs wall\n", phase.wall());
  GeneTable table;
  merge_gene_tables(parts, table);
  const std::vector<int32_t> rank = rank_by_hash(table.genes, c.get());
  phase.note("  genes ranked %.3fs wall\n", phase.wall());
  emit_tokens(parts, table, rank, c.get());
  phase.note("total %.3fs cpu %.3fs wall\n", phase.cpu(), phase.wall());
  *out = c.release();
  return AMG_OK;
}

extern "C" int amg_calls_free(amg_calls* c) {
  delete c;
  return AMG_OK;
}

extern "C" int amg_calls_counts(amg_calls* c, int64_t* n_reads, int64_t* n_tokens, int64_t* n_genes,
                                int64_t* names_bytes, int64_t* ids_bytes) {
  if (!c) return amg_fail(AMG_E_ARG, "null calls");
  if (n_reads) *n_reads = (int64_t)c->read_ids.size();
  if (n_tokens) *n_tokens = (int64_t)c->tokens.size();
  if (n_genes) *n_genes = (int64_t)c->names.size();
  int64_t nb = 0, ib = 0;
  for (auto& s : c->names) nb += (int64_t)s.size() + 1;
  for (size_t i = 0; i < c->read_ids.size(); ++i) ib += (int64_t)c->read_ids.len[i] + 1;
  if (names_bytes) *names_bytes = nb;
  if (ids_bytes) *ids_bytes = ib;
  return AMG_OK;
}

extern "C" int amg_calls_has_blanks(amg_calls* c, int32_t* out) {
  if (!c || !out) return amg_fail(AMG_E_ARG, "null argument");
  *out = c->blanks ? 1 : 0;
  return AMG_OK;
}

extern "C" int amg_calls_get(amg_calls* c, int32_t* tokens, int64_t* read_offsets, char* gene_names,
                             char* read_ids, uint8_t* gene_hashes) {
  if (!c) return amg_fail(AMG_E_ARG, "null calls");
  if (tokens && !c->tokens.empty()) memcpy(tokens, c->tokens.data(), c->tokens.size() * sizeof(int32_t));
  if (read_offsets) memcpy(read_offsets, c->read_off.data(), c->read_off.size() * sizeof(int64_t));
  if (gene_names) for (auto& s : c->names) { memcpy(gene_names, s.c_str(), s.size() + 1); gene_names += s.size() + 1; }
  if (read_ids)
    for (size_t i = 0; i < c->read_ids.size(); ++i) {
      const size_t n = c->read_ids.len[i];
      memcpy(read_ids, c->read_ids.at(i), n);
      read_ids[n] = 0;
      read_ids += n + 1;
    }
  if (gene_hashes && !c->hashes.empty()) memcpy(gene_hashes, c->hashes.data(), c->hashes.size());
  return AMG_OK;
}

// process_pandora_json (pre_processing.py:44-63) keeps the genes of interest that occur in the reads, collected in a
// Python set in the order the reads first show them.  Here: for every wanted gene rank the index of the first token
// that carries it (either strand), -1 when none does — the stream cut into stretches, one thread each.
extern "C" int amg_calls_first_use(const int32_t* tokens, int64_t n_tokens, int32_t two_v, const int32_t* wanted_ranks,
                                   int64_t n_wanted, int64_t* first_index) {
  if ((n_tokens > 0 && !tokens) || (n_wanted > 0 && (!wanted_ranks || !first_index)) || two_v <= 0 || (two_v & 1))
    return amg_fail(AMG_E_ARG, "amg_calls_first_use: bad argument");
  const int32_t V = two_v / 2;
  std::vector<int32_t> slot((size_t)V, -1);  // gene rank -> index into wanted_ranks
  for (int64_t i = 0; i < n_wanted; ++i) {
    first_index[i] = -1;
    if (wanted_ranks[i] < 0 || wanted_ranks[i] >= V) return amg_fail(AMG_E_ARG, "amg_calls_first_use: rank outside [0, V)");
    if (slot[(size_t)wanted_ranks[i]] < 0) slot[(size_t)wanted_ranks[i]] = (int32_t)i;
  }
  if (n_wanted == 0 || n_tokens == 0) return AMG_OK;
  const size_t workers = (size_t)worker_count((size_t)n_tokens * sizeof(int32_t));
  std::vector<std::vector<int64_t>> part(workers, std::vector<int64_t>((size_t)n_wanted, -1));
  std::vector<int> bad(workers, 0);
  run_parts(workers, [&](size_t w) {
    const int64_t a = n_tokens * (int64_t)w / (int64_t)workers, b = n_tokens * (int64_t)(w + 1) / (int64_t)workers;
    int64_t* mine = part[w].data();
    const int32_t* sl = slot.data();
    for (int64_t t = a; t < b; ++t) {
      const int32_t tok = tokens[t];
      if ((uint32_t)tok >= (uint32_t)two_v) { bad[w] = 1; return; }
      const int32_t s = sl[tok >= V ? tok - V : V - 1 - tok];
      if (s >= 0 && mine[s] < 0) mine[s] = t;
    }
  });
  for (int b : bad)
    if (b) return amg_fail(AMG_E_ARG, "amg_calls_first_use: a token lies outside [0, two_v)");
  for (size_t w = 0; w < workers; ++w)
    for (int64_t i = 0; i < n_wanted; ++i)
      if (first_index[i] < 0 && part[w][(size_t)i] >= 0) first_index[i] = part[w][(size_t)i];
  for (int64_t i = 0; i < n_wanted; ++i)  // a rank listed twice answers both times
    if (first_index[i] < 0 && slot[(size_t)wanted_ranks[i]] != (int32_t)i) first_index[i] = first_index[slot[(size_t)wanted_ranks[i]]];
  return AMG_OK;
}

// ------------------------------------------------------------------ gene positions
// gene positions {"read": [[s, e], ...]} laid out in the read order of `c`; reads missing from
// the file, or with a different number of entries than genes, are an error
namespace {
bool parse_position_entries(Reader& r, const amg_calls* c, int64_t* gene_start, int64_t* gene_end, char* seen,
                            PartError& pe, const char* file_begin) {
  std::string key;
  r.ws();
  if (r.p >= r.end) return true;
  do {
    const char *kb, *ke;
    if (!r.str_view(&kb, &ke, &key)) return pe.fail(r, "read id", file_begin);
    const int32_t rid = c->read_ids.find(kb, (size_t)(ke - kb));  // -1: a read that has no gene calls
    if (!r.lit(':') || !r.lit('[')) return pe.fail(r, "expected ': ['", file_begin);
    int64_t at = rid < 0 ? -1 : c->read_off[rid];
    int64_t lim = rid < 0 ? -1 : c->read_off[rid + 1];
    if (!r.lit(']')) {
      do {
        long long s, e;
        if (!r.lit('[') || !r.integer(&s) || !r.lit(',') || !r.integer(&e) || !r.lit(']'))
          return pe.fail(r, "expected [start, end]", file_begin);
        if (at >= 0) {
          if (at >= lim) return pe.fail(r, "more positions than genes for a read", file_begin);
          gene_start[at] = s;
          gene_end[at] = e;
          ++at;
        }
      } while (r.lit(','));
      if (!r.lit(']')) return pe.fail(r, "expected ']'", file_begin);
    }
    if (rid >= 0) {
      if (at != lim) return pe.fail(r, "fewer positions than genes for a read", file_begin);
      seen[rid] = 1;
    }
  } while (r.lit(','));
  r.ws();
  if (r.p != r.end) return pe.fail(r, "expected ',' or the end of the object", file_begin);
  return true;
}
}  // namespace

extern "C" int amg_calls_load_positions_json(amg_calls* c, const char* path, int64_t* gene_start,
                                             int64_t* gene_end) {
  if (!c || !path || !gene_start || !gene_end) return amg_fail(AMG_E_ARG, "null argument");
  FileView file;
  const char *body_b, *body_e;
  if (int rc = object_body(file, path, "positions", &body_b, &body_e)) return rc;
  std::vector<char> seen(c->read_ids.size(), 0);
  {  // the caller's arrays are fresh memory too: huge pages for their page-aligned middle, where the kernel offers them
    const size_t n_tok = (size_t)c->read_off.back() * sizeof(int64_t);
    for (int64_t* a : {gene_start, gene_end}) {
      const uintptr_t lo = ((uintptr_t)a + kTwoMb - 1) & ~(uintptr_t)(kTwoMb - 1), hi = ((uintptr_t)a + n_tok) & ~(uintptr_t)(kTwoMb - 1);
      if (hi > lo) madvise(reinterpret_cast<void*>(lo), hi - lo, MADV_HUGEPAGE);
    }
  }
  const PartError bad = parse_in_pieces(
      body_b, body_e,
      [&](size_t, Reader& r, PartError& pe) { parse_position_entries(r, c, gene_start, gene_end, seen.data(), pe, file.data); },
      [&](size_t) { std::fill(seen.begin(), seen.end(), 0); });
  if (!bad.error.empty()) return amg_fail(AMG_E_ARG, "%s: %s (offset %lld)", path, bad.error.c_str(), bad.error_at);
  for (size_t i = 0; i < seen.size(); ++i)
    if (!seen[i] && c->read_off[i + 1] > c->read_off[i]) return amg_fail(AMG_E_ARG, "%s: no positions for read %s", path, c->read_ids.name(i).c_str());
  return AMG_OK;
}
