// amg_calls_io.hip — buffers, threads and files of the native front-end / write-back, host
// code only: the cache of big buffers, the file read in pieces, the file written in pieces.
#include <algorithm>
#include <mutex>

#include <sys/mman.h>
#include <sys/stat.h>

#include "amg_calls.h"

// ------------------------------------------------------------------ big host buffers, kept between calls
// A load or a write of a cfg-3-sized file fills one to two gigabytes of fresh heap (the file's bytes, the writers'
// texts); freed, glibc hands blocks of that size straight back to the kernel and the next call faults every page in
// again (every piece of a JSON -> sweep -> JSON round ran ~40 % slower inside the round than alone).  The 2 MB-aligned
// blocks of FileView and of the writers' texts go to a small cache instead and serve the next call that asks for about
// as much; amg_calls_trim() gives everything back to the system.
namespace {
using amgc::kTwoMb;
struct BigCache {
  static const int kSlots = 80;  // (two writers' 32 texts each + the file views)
  static const size_t kMaxBytes = (size_t)8 << 30;
  std::mutex mu;
  void* ptr[kSlots] = {};
  size_t bytes[kSlots] = {};
  size_t held = 0;
  // the smallest cached block of at least `want` bytes that is not more than twice as large; *got = its size
  void* take(size_t want, size_t* got) {
    std::lock_guard<std::mutex> g(mu);
    int best = -1;
    for (int i = 0; i < kSlots; ++i)
      if (ptr[i] && bytes[i] >= want && bytes[i] <= 2 * want + 4 * kTwoMb && (best < 0 || bytes[i] < bytes[best])) best = i;
    if (best < 0) return nullptr;
    void* p = ptr[best];
    *got = bytes[best];
    held -= bytes[best];
    ptr[best] = nullptr;
    bytes[best] = 0;
    return p;
  }
  bool give(void* p, size_t n) {  // false: no room, the caller frees the block
    std::lock_guard<std::mutex> g(mu);
    if (getenv("AMG_CALLS_NO_CACHE") || held + n > kMaxBytes) return false;
    for (int i = 0; i < kSlots; ++i)
      if (!ptr[i]) {
        ptr[i] = p;
        bytes[i] = n;
        held += n;
        return true;
      }
    return false;
  }
  size_t trim() {
    std::lock_guard<std::mutex> g(mu);
    const size_t was = held;
    for (int i = 0; i < kSlots; ++i) {
      if (ptr[i]) free(ptr[i]);
      ptr[i] = nullptr;
      bytes[i] = 0;
    }
    held = 0;
    return was;
  }
};
BigCache g_big;
}  // namespace

namespace amgc {
// advised as huge pages (a gigabyte of fresh heap is 250 k page faults otherwise, served under one lock while 32
// threads fill it)
void* big_alloc(size_t want, size_t* got) {
  const size_t whole = (want + kTwoMb - 1) & ~(kTwoMb - 1);
  if (void* p = g_big.take(whole, got)) return p;
  void* p = nullptr;
  if (posix_memalign(&p, kTwoMb, whole) != 0 || !p) return nullptr;
  madvise(p, whole, MADV_HUGEPAGE);  // (advice: ignored where transparent huge pages are off)
  *got = whole;
  return p;
}
void big_free(void* p, size_t size) {
  if (p && !g_big.give(p, size)) free(p);
}

int worker_count(size_t bytes) {
  if (const char* e = getenv("AMG_CALLS_THREADS")) return std::max(1, atoi(e));
  unsigned hw = std::thread::hardware_concurrency();
  int n = (int)std::min<unsigned>(hw ? hw : 1, 32);
  const int by_size = (int)(bytes >> 22) + 1;  // at least 4 MB of text per thread
  return std::max(1, std::min(n, by_size));
}

bool FileView::open(const char* path, std::string& err) {
  int fd = ::open(path, O_RDONLY);
  if (fd < 0) { err = std::string("cannot open ") + path; return false; }
  struct stat st;
  if (fstat(fd, &st) != 0) { ::close(fd); err = std::string("cannot stat ") + path; return false; }
  size = (size_t)st.st_size;
  owned = static_cast<char*>(big_alloc(size + 1, &owned_bytes));
  if (!owned) { ::close(fd); err = "out of memory"; return false; }
  data = owned;
  const int workers = size ? worker_count(size) : 0;
  std::vector<int> bad((size_t)std::max(workers, 1), 0);
  run_parts((size_t)workers, [&](size_t w) {
    size_t at = size / (size_t)workers * w;
    const size_t end = w + 1 == (size_t)workers ? size : size / (size_t)workers * (w + 1);
    while (at < end) {
      const ssize_t n = pread(fd, owned + at, end - at, (off_t)at);
      if (n <= 0) { bad[w] = 1; return; }
      at += (size_t)n;
    }
  });
  ::close(fd);
  for (int b : bad)
    if (b) { err = std::string("short read of ") + path; return false; }
  return true;
}

bool put_raw(PiecewiseFile& f, const std::vector<RawText>& text) {
  std::vector<off_t> at(text.size() + 1, f.pos);
  for (size_t w = 0; w < text.size(); ++w) at[w + 1] = at[w] + (off_t)text[w].n;
  std::vector<char> good(text.size(), 1);
  const int fd = f.fd;
  run_parts(text.size(), [&](size_t w) { good[w] = text[w].n == 0 || PiecewiseFile::put_at(fd, text[w].b, text[w].n, at[w]); });
  for (char g : good) f.ok = f.ok && g;
  f.pos = at[text.size()];
  return f.ok;
}
}  // namespace amgc

extern "C" int amg_calls_trim(int64_t* released_bytes) {
  const size_t was = g_big.trim();
  if (released_bytes) *released_bytes = (int64_t)was;
  return AMG_OK;
}
