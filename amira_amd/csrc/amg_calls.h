// amg_calls.h — what the units of the native front-end / write-back share (amg_calls_io, _load, _write; SURVEY section 8
// row f2).  Host code only, no HIP header: the units compile as plain C++ too (calls_check.cpp, under the host sanitizers).
#pragma once
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <unistd.h>

#include "amg_host.h"

namespace amgc __attribute__((visibility("hidden"))) {
const size_t kTwoMb = (size_t)2 << 20;

inline bool is_json_blank(char c) { return c == ' ' || c == '\n' || c == '\t' || c == '\r'; }

// ------------------------------------------------------------------ amg_calls_io.hip: buffers, threads, files
// a 2 MB-aligned block of at least `want` bytes from the cache of big buffers; *got = its size, which big_free wants back
void* big_alloc(size_t want, size_t* got);
void big_free(void* p, size_t size);

// threads for `bytes` of work: AMG_CALLS_THREADS, else the cores (32 at most) with at least 4 MB each
int worker_count(size_t bytes);

template <class F>
void run_parts(size_t n, F f) {
  if (n <= 1) {
    if (n == 1) f(0);
    return;
  }
  std::vector<std::thread> th;
  th.reserve(n);
  for (size_t i = 0; i < n; ++i) th.emplace_back([&f, i] { f(i); });
  for (auto& t : th) t.join();
}

// time since its construction; note() prints to stderr when AMG_CALLS_TIMING is set, and only then
struct PhaseClock {
  const bool on = getenv("AMG_CALLS_TIMING") != nullptr;
  const clock_t c_start = clock();
  const std::chrono::steady_clock::time_point w_start = std::chrono::steady_clock::now();
  double wall() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - w_start).count(); }
  double cpu() const { return (double)(clock() - c_start) / CLOCKS_PER_SEC; }
  template <class... A>
  void note(const char* fmt, A... a) const { if (on) fprintf(stderr, fmt, a...); }
};

// the file in memory, read by several threads at once (each its own stretch, pread): a gigabyte of gene calls is in
// memory in a fraction of a second, and — unlike a file mapping, whose first touch of every page is a fault served
// one at a time in sandboxed kernels — the parsers then run on ordinary memory
struct FileView {
  const char* data = nullptr;
  size_t size = 0;
  // (not a vector: no zero fill of a gigabyte that is about to be overwritten; a block of the big-buffer cache)
  char* owned = nullptr;
  size_t owned_bytes = 0;
  FileView() = default;
  FileView(const FileView&) = delete;
  FileView& operator=(const FileView&) = delete;
  ~FileView() { big_free(owned, owned_bytes); }
  bool open(const char* path, std::string& err);
};

// output file written in pieces by many threads: the texts of a batch go to their offsets with pwrite, side by side
// (one thread's write() into the page cache moves 1.5 - 2 GB/s: it was two thirds of a writer's time)
struct PiecewiseFile {
  int fd = -1;
  off_t pos = 0;
  bool ok = true;
  // (no O_TRUNC: a file that is being replaced keeps its pages in the page cache and the new text is copied over them
  // — freeing a gigabyte of cached pages and faulting them in again cost as much as the write; finish() cuts the file
  // to its new length)
  explicit PiecewiseFile(const char* path) { fd = open(path, O_WRONLY | O_CREAT, 0666); }
  ~PiecewiseFile() { if (fd >= 0) close(fd); }
  static bool put_at(int fd, const char* p, size_t n, off_t at) {
    while (n) {
      const ssize_t w = pwrite(fd, p, n, at);
      if (w <= 0) return false;
      p += w;
      n -= (size_t)w;
      at += w;
    }
    return true;
  }
  void put(char ch) {
    ok = ok && put_at(fd, &ch, 1, pos);
    ++pos;
  }
  bool finish() {
    ok = ok && fd >= 0 && ftruncate(fd, pos) == 0;
    const bool closed = fd >= 0 && close(fd) == 0;
    fd = -1;
    return ok && closed;
  }
};

// A worker's text: ONE block sized by an upper bound, filled through a bare cursor (appending to a string checked its
// capacity once per character: the texts were two thirds of a writer's time), a block of the big-buffer cache.
struct RawText {
  char* b = nullptr;
  size_t got = 0, n = 0;
  RawText() = default;
  RawText(const RawText&) = delete;
  RawText& operator=(const RawText&) = delete;
  ~RawText() { big_free(b, got); }
  bool room(size_t want) {
    n = 0;
    if (want <= got) return true;
    big_free(b, got);
    b = static_cast<char*>(big_alloc(want, &got));
    if (!b) got = 0;
    return b != nullptr;
  }
};

// the texts one behind the other at the file's position, one thread each
bool put_raw(PiecewiseFile& f, const std::vector<RawText>& text);

// ------------------------------------------------------------------ amg_calls_load.hip: reader, name tables, hashes
// FNV-1a with a last fold, the name hash of Interner: whoever hashes while scanning (the gene fast path) takes the same
// three steps, or one name gets two ids
struct Fnv1a {
  static uint64_t start() { return 1469598103934665603ull; }
  static uint64_t step(uint64_t h, unsigned char byte) { return (h ^ byte) * 1099511628211ull; }
  static uint64_t finish(uint64_t h) { return h ^ (h >> 29); }
};

// name bytes -> first-seen id, open addressing over (offset, length) into one arena
struct Interner {
  std::vector<char> arena;
  std::vector<uint32_t> off, len;
  std::vector<int32_t> slots;
  size_t mask = 0;
  Interner() { rehash(1 << 16); }
  static uint64_t hash(const char* b, size_t n) {
    uint64_t h = Fnv1a::start();
    for (size_t i = 0; i < n; ++i) h = Fnv1a::step(h, (unsigned char)b[i]);
    return Fnv1a::finish(h);
  }
  void reserve(size_t n_items, size_t n_bytes);  // room for n_items names of n_bytes in all without growing
  int32_t intern(const char* b, size_t n) { return intern_h(b, n, hash(b, n)); }
  int32_t intern_h(const char* b, size_t n, uint64_t h) {  // h: hash(b, n), trusted
    const size_t s = probe(b, n, h);
    if (slots[s] >= 0) return slots[s];
    const int32_t id = (int32_t)off.size();
    off.push_back((uint32_t)arena.size());
    len.push_back((uint32_t)n);
    arena.insert(arena.end(), b, b + n);
    slots[s] = id;
    if (off.size() * 2 > slots.size()) rehash(slots.size() * 4);
    return id;
  }
  int32_t find(const char* b, size_t n) const { return slots[probe(b, n, hash(b, n))]; }  // -1: not there
  size_t size() const { return off.size(); }
  const char* at(size_t id) const { return &arena[off[id]]; }
  std::string name(size_t id) const { return std::string(at(id), len[id]); }

 private:
  // the slot that holds the name, or the free one (slots[s] < 0) where it would go
  size_t probe(const char* b, size_t n, uint64_t h) const {
    size_t s = h & mask;
    for (; slots[s] >= 0; s = (s + 1) & mask) {
      const int32_t id = slots[s];
      if (len[id] == n && memcmp(&arena[off[id]], b, n) == 0) break;
    }
    return s;
  }
  void rehash(size_t new_size);
};

// minimal strict JSON reader for the two shapes of the front end (strings with escapes, integers)
struct Reader {
  const char* p;
  const char* end;
  std::string err;
  void ws() { while (p < end && is_json_blank(*p)) ++p; }
  bool lit(char c) {
    ws();
    if (p < end && *p == c) { ++p; return true; }
    return false;
  }
  bool str(std::string& out);
  // fast path: the string as a view into the file when it has no escapes (then *owned is
  // empty and [*b, *e) is the content); otherwise falls back to str() into *owned
  bool str_view(const char** b, const char** e, std::string* owned) {
    ws();
    if (p >= end || *p != '"') { err = "expected string"; return false; }
    const char* q = p + 1;
    while (q < end && *q != '"' && *q != '\\') ++q;
    if (q < end && *q == '"') {
      *b = p + 1;
      *e = q;
      p = q + 1;
      owned->clear();
      return true;
    }
    if (!str(*owned)) return false;
    *b = owned->data();
    *e = owned->data() + owned->size();
    return true;
  }
  bool integer(long long* v) {
    ws();
    const char* s = p;
    if (p < end && (*p == '-' || *p == '+')) ++p;
    if (p >= end || *p < '0' || *p > '9') { err = "expected integer"; return false; }
    long long x = 0;
    while (p < end && *p >= '0' && *p <= '9') x = x * 10 + (*p++ - '0');
    if (p < end && (*p == '.' || *p == 'e' || *p == 'E')) {  // tolerate 12.0
      while (p < end && (*p == '.' || *p == 'e' || *p == 'E' || *p == '+' || *p == '-' || (*p >= '0' && *p <= '9'))) ++p;
    }
    *v = (*s == '-') ? -x : x;
    return true;
  }
};

void sha256(const uint8_t* p, size_t n, uint8_t out[32]);  // FIPS 180-4

// sha256(pickle.dumps(name)) for pickle.DEFAULT_PROTOCOL = 4 (CPython 3.8 - 3.13)
void gene_hash(const std::string& name, uint8_t out[32]);
}  // namespace amgc

struct amg_calls {
  amgc::Interner read_ids;  // read ids in file order (id = index), one arena instead of a string per read
  std::vector<int64_t> read_off{0};
  std::vector<int32_t> tokens;
  std::vector<std::string> names;  // rank order
  std::vector<uint8_t> hashes;     // 32 bytes per name, rank order
  bool blanks = false;             // some gene name of the file held a blank
};
