// amg_calls_write.hip — native write-back, host code only: corrected CSR and gene positions
// -> the two JSON files of result_utils.py:1260-1264, byte for byte as json.dumps writes them.
#include <algorithm>
#include <cstdio>

#include "amg_calls.h"

namespace {
using namespace amgc;

// the bytes of a JSON string for s[0..n): quotes, backslashes and control characters as json.dumps(ensure_ascii=False)
// writes them; at most 6 n + 2 bytes
char* json_string_raw(char* q, const char* s, size_t n) {
  *q++ = '"';
  for (size_t i = 0; i < n; ++i) {
    const unsigned char ch = (unsigned char)s[i];
    if (ch == '"' || ch == '\\') { *q++ = '\\'; *q++ = (char)ch; }
    else if (ch < 0x20) { q += snprintf(q, 8, "\\u%04x", ch); }
    else *q++ = (char)ch;
  }
  *q++ = '"';
  return q;
}

const char kDigits2[201] =
    "00010203040506070809101112131415161718192021222324252627282930313233343536373839404142434445464748495051525354555657585960616263646566676869707172737475767778798081828384858687888990919293949596979899";
inline char* put_i64(char* q, long long v) {
  unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
  if (v < 0) *q++ = '-';
  char buf[24];
  int n = 0;
  while (u >= 100) {
    const unsigned r = (unsigned)(u % 100);
    u /= 100;
    buf[n++] = kDigits2[2 * r + 1];
    buf[n++] = kDigits2[2 * r];
  }
  if (u >= 10) {
    buf[n++] = kDigits2[2 * u + 1];
    buf[n++] = kDigits2[2 * u];
  } else {
    buf[n++] = (char)('0' + u);
  }
  while (n) *q++ = buf[--n];
  return q;
}

// {"read": [item, ...], ...} with one item per token (json.dumps separators ', ' and ': ', ensure_ascii=False).  The
// text of a stretch of reads is made by one thread each, the stretches are written in order.  bound(ta, tb): at least
// the bytes of the items of tokens [ta, tb) with their separators; put_item(q, t): token t's item through the cursor.
template <class Bound, class PutItem>
int write_rows(const char* path, const char* label, const PhaseClock& phase, const int64_t* read_offsets, int64_t n_reads,
               const char* read_ids, size_t bytes_per_token, Bound bound, PutItem put_item) {
  std::vector<const char*> rid((size_t)n_reads + 1);
  const char* p = read_ids;
  for (int64_t r = 0; r < n_reads; ++r) { rid[r] = p; p += strlen(p) + 1; }
  rid[n_reads] = p;
  PiecewiseFile f(path);
  if (f.fd < 0) return amg_fail(AMG_E_ARG, "cannot write %s", path);
  const int64_t T = n_reads > 0 ? read_offsets[n_reads] : 0;
  const size_t workers = (size_t)std::max<int64_t>(1, std::min<int64_t>(worker_count((size_t)T * bytes_per_token + 1), n_reads));
  std::vector<RawText> text(workers);
  std::vector<char> fine(workers, 1);
  // batches of stretches, so that the text in memory stays bounded for very large files
  const int64_t per_batch = std::max<int64_t>((int64_t)workers * 65536, 1);
  f.put('{');
  double t_text = 0, t_put = 0;
  for (int64_t lo = 0; lo < n_reads && f.ok; lo += per_batch) {
    const int64_t hi = std::min(n_reads, lo + per_batch);
    const double t0 = phase.wall();
    run_parts(workers, [&](size_t w) {
      RawText& o = text[w];
      const int64_t a = lo + (hi - lo) * (int64_t)w / (int64_t)workers, b = lo + (hi - lo) * (int64_t)(w + 1) / (int64_t)workers;
      // the items' bound, a bound for the read ids (escapes), the framing of a read
      const size_t need = bound(read_offsets[a], read_offsets[b]) + (size_t)(rid[b] - rid[a]) * 6 + (size_t)(b - a) * 8 + 16;
      if (!o.room(need)) { fine[w] = 0; return; }
      char* q = o.b;
      for (int64_t r = a; r < b; ++r) {
        if (r) { *q++ = ','; *q++ = ' '; }
        q = json_string_raw(q, rid[r], (size_t)(rid[r + 1] - rid[r] - 1));
        *q++ = ':'; *q++ = ' '; *q++ = '[';
        for (int64_t t = read_offsets[r]; t < read_offsets[r + 1]; ++t) {
          if (t > read_offsets[r]) { *q++ = ','; *q++ = ' '; }
          q = put_item(q, t);
        }
        *q++ = ']';
      }
      o.n = (size_t)(q - o.b);
    });
    for (char g : fine) if (!g) return amg_fail(AMG_E_NOMEM, "no memory for the text of %s", path);
    const double t1 = phase.wall();
    put_raw(f, text);
    t_text += t1 - t0;
    t_put += phase.wall() - t1;
  }
  f.put('}');
  if (!f.finish()) return amg_fail(AMG_E_ARG, "short write to %s", path);
  phase.note("write %s: text %.3fs, file %.3fs, total %.3fs wall, %zu workers\n", label, t_text, t_put, phase.wall(), workers);
  return AMG_OK;
}

// where the spelling of a token starts in the calls writer's table: "+name" at 2 g, "-name" at 2 g + 1 for gene rank g
inline size_t spelled_index(int32_t tok, int64_t V) {
  const int64_t g = tok >= V ? tok - V : V - 1 - tok;
  return (size_t)2 * (size_t)g + (tok >= V ? 0 : 1);
}
}  // namespace

// write-back: corrected CSR -> {"read": ["+gene", ...]} — result_utils.py:1260-1264.  Every gene's two spellings
// ("+name" and "-name" as JSON strings) are made once; a read's text is a run of copies.
extern "C" int amg_calls_write_json(const char* path, const int32_t* tokens, const int64_t* read_offsets,
                                    int64_t n_reads, const char* gene_names, int64_t n_genes,
                                    const char* read_ids) {
  if (!path || !read_offsets || !gene_names || !read_ids) return amg_fail(AMG_E_ARG, "null argument");
  const PhaseClock phase;
  // spelled[2 g] / spelled[2 g + 1]: the JSON strings of "+name" / "-name" of gene rank g, in one arena
  std::vector<uint32_t> sp_off((size_t)2 * n_genes + 1, 0);
  std::string arena;
  {
    const char* p = gene_names;
    std::string tmp;
    for (int64_t i = 0; i < n_genes; ++i) {
      const size_t nl = strlen(p);
      for (int sgn = 0; sgn < 2; ++sgn) {
        tmp.assign(1, sgn == 0 ? '+' : '-');
        tmp.append(p, nl);
        const size_t at = arena.size();
        arena.resize(at + 6 * tmp.size() + 2);
        char* e = json_string_raw(&arena[at], tmp.data(), tmp.size());
        arena.resize((size_t)(e - arena.data()));
        sp_off[2 * i + sgn + 1] = (uint32_t)arena.size();
      }
      p += nl + 1;
    }
  }
  const int64_t V = n_genes ? n_genes : 1;
  return write_rows(
      path, "calls", phase, read_offsets, n_reads, read_ids, 10,
      [&](int64_t ta, int64_t tb) {  // exact size of the genes' spellings
        size_t need = 0;
        for (int64_t t = ta; t < tb; ++t) {
          const size_t i = spelled_index(tokens[t], V);
          need += sp_off[i + 1] - sp_off[i] + 2;
        }
        return need;
      },
      [&](char* q, int64_t t) {
        const size_t i = spelled_index(tokens[t], V);
        const uint32_t len = sp_off[i + 1] - sp_off[i];
        memcpy(q, arena.data() + sp_off[i], len);
        return q + len;
      });
}

// positions write-back: {"read": [[start, end], ...]} as json.dumps(gene_position_dict) writes it
// (result_utils.py:1260-1264, second file)
template <class Int>
static int write_positions_json(const char* path, const Int* gene_start, const Int* gene_end,
                                const int64_t* read_offsets, int64_t n_reads, const char* read_ids) {
  if (!path || !read_offsets || !read_ids || ((!gene_start || !gene_end) && n_reads > 0 && read_offsets[n_reads] > 0))
    return amg_fail(AMG_E_ARG, "null argument");
  const PhaseClock phase;
  return write_rows(
      path, "positions", phase, read_offsets, n_reads, read_ids, 16,
      [&](int64_t ta, int64_t tb) {  // a bound from the longest number of the stretch
        unsigned long long most = 0;
        bool neg = false;
        for (int64_t t = ta; t < tb; ++t) {
          const long long s0 = gene_start[t], e0 = gene_end[t];
          neg = neg || s0 < 0 || e0 < 0;
          const unsigned long long us = s0 < 0 ? 0ull - (unsigned long long)s0 : (unsigned long long)s0;
          const unsigned long long ue = e0 < 0 ? 0ull - (unsigned long long)e0 : (unsigned long long)e0;
          most = us > most ? us : most;
          most = ue > most ? ue : most;
        }
        int digits = 1;
        while (most >= 10) { most /= 10; ++digits; }
        return (size_t)(tb - ta) * (size_t)(2 * (digits + (neg ? 1 : 0)) + 6);
      },
      [&](char* q, int64_t t) {
        *q++ = '[';
        q = put_i64(q, (long long)gene_start[t]);
        *q++ = ','; *q++ = ' ';
        q = put_i64(q, (long long)gene_end[t]);
        *q++ = ']';
        return q;
      });
}

extern "C" int amg_calls_write_positions_json(const char* path, const int64_t* gene_start, const int64_t* gene_end,
                                              const int64_t* read_offsets, int64_t n_reads, const char* read_ids) {
  return write_positions_json<int64_t>(path, gene_start, gene_end, read_offsets, n_reads, read_ids);
}
extern "C" int amg_calls_write_positions_json32(const char* path, const int32_t* gene_start, const int32_t* gene_end,
                                                const int64_t* read_offsets, int64_t n_reads, const char* read_ids) {
  return write_positions_json<int32_t>(path, gene_start, gene_end, read_offsets, n_reads, read_ids);
}
