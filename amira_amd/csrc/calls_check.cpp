// calls_check.cpp — the gene-call front end (amg_calls_io / _load / _write) on its own, as plain host C++ under the host
// sanitizers: `make calls_check` builds it with AddressSanitizer + UBSan and with ThreadSanitizer, see tools/README.md.
// It writes small inputs into a temporary directory, runs every entry point on them with 1 to 16 threads and exits
// non-zero at the first mismatch.  What the values mean against Python is tests/test_calls_cpu.py's business; this
// program is about pieces, bounds and threads.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <filesystem>
#include <fstream>
#include <sstream>

#include "amg_calls.h"

thread_local std::string g_amg_err;
int amg_fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_amg_err = buf;
  return code;
}

#define CHECK(cond)                                                                                             \
  do {                                                                                                          \
    if (!(cond)) {                                                                                              \
      fprintf(stderr, "calls_check: line %d: %s does not hold (last error: %s)\n", __LINE__, #cond, g_amg_err.c_str()); \
      exit(1);                                                                                                  \
    }                                                                                                           \
  } while (0)

namespace {
typedef std::vector<std::pair<long long, long long>> Positions;
struct Entry {
  std::string id;
  std::vector<std::string> genes;  // "+name" / "-name"
  Positions pos;
};
typedef std::vector<Entry> Data;

std::string g_dir;
std::string in_dir(const char* name) { return g_dir + "/" + name; }
void threads(int n) { setenv("AMG_CALLS_THREADS", std::to_string(n).c_str(), 1); }
const int kThreads[] = {1, 2, 5, 16};

// ---- json.dumps as far as these files need it (ascii: two-byte UTF-8 as \uXXXX, what ensure_ascii=True writes)
std::string dumps(const std::string& s, bool ascii = false) {
  std::string o = "\"";
  for (size_t i = 0; i < s.size(); ++i) {
    const unsigned char ch = (unsigned char)s[i];
    if (ch == '"' || ch == '\\') { o += '\\'; o += (char)ch; }
    else if (ascii && (ch & 0xE0) == 0xC0 && i + 1 < s.size()) {
      char u[8];
      snprintf(u, sizeof(u), "\\u%04x", (unsigned)((ch & 0x1F) << 6 | ((unsigned char)s[++i] & 0x3F)));
      o += u;
    } else o += (char)ch;
  }
  return o + "\"";
}
// the calls file; escape_every: every so many-th gene string is written with \u escapes (0: none)
std::string calls_text(const Data& d, int escape_every = 0) {
  std::string o = "{";
  int n = 0;
  for (size_t r = 0; r < d.size(); ++r) {
    o += (r ? ", " : "") + dumps(d[r].id) + ": [";
    for (size_t g = 0; g < d[r].genes.size(); ++g) o += (g ? ", " : "") + dumps(d[r].genes[g], escape_every && ++n % escape_every == 0);
    o += "]";
  }
  return o + "}";
}
std::string positions_text(const Data& d) {
  std::string o = "{";
  for (size_t r = 0; r < d.size(); ++r) {
    o += (r ? ", " : "") + dumps(d[r].id) + ": [";
    for (size_t g = 0; g < d[r].pos.size(); ++g)
      o += (g ? ", [" : "[") + std::to_string(d[r].pos[g].first) + ", " + std::to_string(d[r].pos[g].second) + "]";
    o += "]";
  }
  return o + "}";
}
std::string put_file(const char* name, const std::string& text) {
  const std::string path = in_dir(name);
  std::ofstream(path, std::ios::binary) << text;
  return path;
}
std::string get_file(const std::string& path) {
  std::ostringstream s;
  s << std::ifstream(path, std::ios::binary).rdbuf();
  return s.str();
}

// 700 reads of 0 / 1 / 3 / 8 / 30 genes; names with a blank, UTF-8, a quote, a backslash and one of 300 bytes
Data make_data() {
  std::vector<std::string> names;
  for (int i = 0; i < 40; ++i) names.push_back("g" + std::to_string(i));
  for (const char* s : {"two words", "caf\xc3\xa9", "q\"uote", "back\\slash", "two caf\xc3\xa9s"}) names.push_back(s);  // (the last: a blank on both paths)
  names.push_back(std::string(300, 'x'));
  const int sizes[] = {0, 1, 3, 8, 30};
  uint64_t rng = 7;
  auto next = [&](unsigned n) { rng = rng * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(rng >> 33) % n; };
  Data d(700);
  for (int i = 0; i < 700; ++i) {
    char id[16];
    snprintf(id, sizeof(id), "read_%04d", i);
    d[i].id = id;
    const int n = i == 0 ? 0 : sizes[next(5)];
    for (int j = 0; j < n; ++j) {
      d[i].genes.push_back((next(2) ? "+" : "-") + names[next((unsigned)names.size())]);
      d[i].pos.push_back({j * 100, j * 100 + 1 + (int)next(90)});
    }
  }
  return d;
}

// ---- what a load hands back
struct Loaded {
  std::vector<int32_t> tokens;
  std::vector<int64_t> off, gs, ge;
  std::vector<std::string> names, ids;
  std::vector<uint8_t> hashes;
  bool operator==(const Loaded& o) const {
    return tokens == o.tokens && off == o.off && gs == o.gs && ge == o.ge && names == o.names && ids == o.ids && hashes == o.hashes;
  }
};
std::vector<std::string> split_nul(const std::vector<char>& buf, size_t n) {
  std::vector<std::string> out;
  const char* p = buf.data();
  for (size_t i = 0; i < n; ++i) { out.emplace_back(p); p += out.back().size() + 1; }
  return out;
}
std::string join_nul(const std::vector<std::string>& v) {
  std::string o;
  for (auto& s : v) o.append(s.c_str(), s.size() + 1);
  return o;
}
// AMG_OK and *out filled, or the loader's error code (positions == nullptr: calls only)
int load(const std::string& calls, const char* positions, Loaded* out) {
  amg_calls* c = nullptr;
  int rc = amg_calls_load_json(calls.c_str(), &c);
  if (rc != AMG_OK) { CHECK(c == nullptr); return rc; }
  int64_t n_reads, n_tokens, n_genes, names_bytes, ids_bytes;
  CHECK(amg_calls_counts(c, &n_reads, &n_tokens, &n_genes, &names_bytes, &ids_bytes) == AMG_OK);
  Loaded l;
  l.tokens.resize((size_t)n_tokens);
  l.off.resize((size_t)n_reads + 1);
  l.hashes.resize((size_t)n_genes * 32);
  std::vector<char> names((size_t)names_bytes + 1), ids((size_t)ids_bytes + 1);
  CHECK(amg_calls_get(c, l.tokens.data(), l.off.data(), names.data(), ids.data(), l.hashes.data()) == AMG_OK);
  l.names = split_nul(names, (size_t)n_genes);
  l.ids = split_nul(ids, (size_t)n_reads);
  if (positions) {
    l.gs.assign((size_t)n_tokens + 1, -7);  // (+ 1: never a null pointer, and a guard behind the last position)
    l.ge.assign((size_t)n_tokens + 1, -7);
    rc = amg_calls_load_positions_json(c, positions, l.gs.data(), l.ge.data());
    CHECK(l.gs.back() == -7 && l.ge.back() == -7);
    l.gs.pop_back();
    l.ge.pop_back();
  }
  CHECK(amg_calls_free(c) == AMG_OK);
  if (rc == AMG_OK) *out = l;
  return rc;
}
bool failed_with(int rc, const char* what) { return rc == AMG_E_ARG && g_amg_err.find(what) != std::string::npos; }

std::string spelled(const Loaded& l, int32_t tok) {
  const int32_t V = (int32_t)l.names.size();
  return tok >= V ? "+" + l.names[(size_t)(tok - V)] : "-" + l.names[(size_t)(V - 1 - tok)];
}
std::string underscored(std::string gene) {
  std::replace(gene.begin() + 1, gene.end(), ' ', '_');
  return gene;
}
// the load is what the data says: ids in file order, every token spells its gene, names in hash order, positions
void check_against(const Loaded& l, const Data& d) {
  CHECK(l.ids.size() == d.size() && l.off.size() == d.size() + 1 && l.off[0] == 0);
  for (size_t r = 0; r < d.size(); ++r) {
    CHECK(l.ids[r] == d[r].id && l.off[r + 1] - l.off[r] == (int64_t)d[r].genes.size());
    for (size_t g = 0; g < d[r].genes.size(); ++g) {
      const size_t t = (size_t)l.off[r] + g;
      CHECK(spelled(l, l.tokens[t]) == underscored(d[r].genes[g]));
      CHECK(l.gs[t] == d[r].pos[g].first && l.ge[t] == d[r].pos[g].second);
    }
  }
  for (size_t i = 0; i < l.names.size(); ++i) {
    uint8_t h[32];
    amgc::gene_hash(l.names[i], h);
    CHECK(memcmp(h, &l.hashes[i * 32], 32) == 0);
    CHECK(i == 0 || memcmp(&l.hashes[(i - 1) * 32], h, 32) < 0);
  }
}

// ---- loader and positions in pieces, round trip through the calls writer
void check_loader_in_pieces(const Data& plain) {
  Data tricky = plain;
  tricky.push_back({"odd], ", {"+g1", "-g2"}, {{1, 2}, {3, 4}}});  // the cut pattern inside a key: the single-piece fallback
  for (const Data* d : {&plain, (const Data*)&tricky}) {
    const std::string cj = put_file("c.json", calls_text(*d, 3)), pj = put_file("p.json", positions_text(*d));
    Data want = *d;
    for (auto& e : want)
      for (auto& g : e.genes) g = underscored(g);
    Loaded one;
    for (int n : kThreads) {
      threads(n);
      Loaded l;
      CHECK(load(cj, pj.c_str(), &l) == AMG_OK);
      if (n == 1) { one = l; check_against(one, *d); }
      CHECK(l == one);
      const std::string back = in_dir("back.json");
      CHECK(amg_calls_write_json(back.c_str(), l.tokens.data(), l.off.data(), (int64_t)l.ids.size(), join_nul(l.names).c_str(),
                                 (int64_t)l.names.size(), join_nul(l.ids).c_str()) == AMG_OK);
      CHECK(get_file(back) == calls_text(want));
      Loaded again;
      CHECK(load(back, pj.c_str(), &again) == AMG_OK && again == one);
    }
  }
}

void check_position_errors(const Data& plain) {
  const std::string cj = put_file("c.json", calls_text(plain));
  size_t with_genes = 300;
  while (plain[with_genes].genes.empty()) ++with_genes;
  for (int n : {1, 5}) {
    threads(n);
    Loaded l;
    Data d = plain;
    d[with_genes].pos.push_back({1, 2});
    CHECK(failed_with(load(cj, put_file("p.json", positions_text(d)).c_str(), &l), "more positions than genes for a read"));
    d = plain;
    d[with_genes].pos.pop_back();
    CHECK(failed_with(load(cj, put_file("p.json", positions_text(d)).c_str(), &l), "fewer positions than genes for a read"));
    d = plain;
    d.erase(d.begin() + (long)with_genes);
    CHECK(failed_with(load(cj, put_file("p.json", positions_text(d)).c_str(), &l), ("no positions for read " + plain[with_genes].id).c_str()));
    CHECK(failed_with(load(cj, put_file("p.json", "[]").c_str(), &l), "expected an object of read -> positions (offset 0)"));
  }
}

// ---- positions through both writers
template <class Int>
std::string written_positions(const std::vector<long long>& s, const std::vector<long long>& e, const std::vector<int64_t>& off,
                              const std::string& ids, int (*write)(const char*, const Int*, const Int*, const int64_t*, int64_t, const char*)) {
  const std::vector<Int> s2(s.begin(), s.end()), e2(e.begin(), e.end());
  const std::string path = in_dir("wp.json");
  CHECK(write(path.c_str(), s2.data(), e2.data(), off.data(), (int64_t)off.size() - 1, ids.c_str()) == AMG_OK);
  return get_file(path);
}
void check_position_writers() {
  // numbers of 1, 2, 9, 10 digits and negative ones for both widths; 18 and 19 digits for the 64-bit writer alone
  const std::vector<long long> narrow = {0, 1, 2, 9, 10, 99, 100, 999999999, 1000000000, 2147483647, -1, -10, -99, -2147483647 - 1};
  std::vector<long long> wide = narrow;
  for (long long v : {999999999999999999ll, 1000000000000000000ll, -1000000000000000000ll, 9223372036854775807ll}) wide.push_back(v);
  for (const auto* vals : {&narrow, (const std::vector<long long>*)&wide}) {
    Data d;
    size_t at = 0;
    for (int r = 0; r < 40; ++r) {  // reads of 0 .. 6 positions; "a\"b" needs an escape in its key
      d.push_back({r == 3 ? "a\"b" : "r" + std::to_string(r), {}, {}});
      for (int g = 0; g < r % 7; ++g, ++at) d.back().pos.push_back({(*vals)[at % vals->size()], (*vals)[(at * 5 + 3) % vals->size()]});
    }
    std::vector<long long> s, e;
    std::vector<int64_t> off{0};
    std::vector<std::string> ids;
    for (auto& x : d) {
      for (auto& p : x.pos) { s.push_back(p.first); e.push_back(p.second); }
      off.push_back((int64_t)s.size());
      ids.push_back(x.id);
    }
    for (int n : kThreads) {
      threads(n);
      CHECK(written_positions<int64_t>(s, e, off, join_nul(ids), amg_calls_write_positions_json) == positions_text(d));
      if (vals == &narrow) CHECK(written_positions<int32_t>(s, e, off, join_nul(ids), amg_calls_write_positions_json32) == positions_text(d));
    }
  }
}

void check_writers_replace(const Data& plain) {
  const Data few(plain.begin() + 300, plain.begin() + 305);
  const std::string cj = put_file("c.json", calls_text(few)), pj = put_file("p.json", positions_text(few));
  for (int n : {1, 7}) {
    threads(n);
    Loaded l;
    CHECK(load(cj, pj.c_str(), &l) == AMG_OK);
    const std::string out_c = put_file("out_c.json", std::string(200000, 'x')), out_p = put_file("out_p.json", std::string(200000, 'x'));
    const std::string names = join_nul(l.names), ids = join_nul(l.ids);
    CHECK(amg_calls_write_json(out_c.c_str(), l.tokens.data(), l.off.data(), 5, names.c_str(), (int64_t)l.names.size(), ids.c_str()) == AMG_OK);
    CHECK(amg_calls_write_positions_json(out_p.c_str(), l.gs.data(), l.ge.data(), l.off.data(), 5, ids.c_str()) == AMG_OK);
    Data want = few;
    for (auto& e : want)
      for (auto& g : e.genes) g = underscored(g);
    CHECK(get_file(out_c) == calls_text(want) && get_file(out_p) == positions_text(few));
    const std::string nowhere = in_dir("no_such_dir/x.json");
    CHECK(failed_with(amg_calls_write_json(nowhere.c_str(), l.tokens.data(), l.off.data(), 5, names.c_str(), (int64_t)l.names.size(), ids.c_str()), "cannot write"));
    CHECK(failed_with(amg_calls_write_positions_json(nowhere.c_str(), l.gs.data(), l.ge.data(), l.off.data(), 5, ids.c_str()), "cannot write"));
    CHECK(amg_calls_write_json(out_c.c_str(), nullptr, l.off.data(), 0, names.c_str(), (int64_t)l.names.size(), ids.c_str()) == AMG_OK);
    CHECK(get_file(out_c) == "{}");
  }
}

// ---- malformed files: the message of a parse in four pieces is the message of a parse in one
void check_errors(const Data& plain) {
  const std::string text = calls_text(plain);
  Loaded l;
  auto same_error = [&](const std::string& bad_text, const char* what) {
    const std::string path = put_file("bad.json", bad_text);
    threads(1);
    CHECK(failed_with(load(path, nullptr, &l), what));
    const std::string single = g_amg_err;
    CHECK(single.find("(offset ") != std::string::npos);
    threads(4);
    CHECK(failed_with(load(path, nullptr, &l), what) && g_amg_err == single);
  };
  const size_t cut = text.find("], \"", text.size() * 3 / 8) + 3;  // a key's opening quote inside the second of four pieces
  const std::pair<const char*, const char*> bad_genes[] = {
      {"\"gene_without_strand\"", "Strand information missing for a gene"}, {"\"+\"", "Gene name information missing for a gene"},
      {"\" \"", "Gene information is missing"}, {"\"\"", "Gene information is missing"},
      // ... and through the reader of strings with escapes
      {"\"g\\\\ne\"", "Strand information missing for a gene"}, {"\"\\u002b\"", "Gene name information missing for a gene"},
      {"\"\\u0020 \"", "Gene information is missing"}, {"\"+g\\u12\"", "gene: bad \\u escape"}};
  for (auto& b : bad_genes) same_error(text.substr(0, cut) + "\"bad\": [\"+g1\", " + b.first + "], " + text.substr(cut), b.second);
  same_error(text.substr(0, cut) + "\"twice\": [], \"twice\": [], " + text.substr(cut), "duplicate read id");  // inside one piece ...
  same_error(text.substr(0, text.size() / 2), "expected '}'");                                       // truncated
  same_error(text.substr(0, text.size() / 2) + "}", "");                                            // ... inside a piece
  same_error(text.substr(1), "expected an object of read -> gene list (offset 0)");
  // ... across two pieces: the pieces parse, the merge of their tables reports the read
  const std::string dup = put_file("dup.json", text.substr(0, text.size() - 1) + ", \"read_0003\": [\"+g1\"]}");
  threads(1);
  CHECK(failed_with(load(dup, nullptr, &l), "duplicate read id (offset "));
  threads(4);
  CHECK(failed_with(load(dup, nullptr, &l), "duplicate read id read_0003"));
  CHECK(failed_with(load(in_dir("missing.json"), nullptr, &l), "cannot open"));
  amg_calls* c = nullptr;
  CHECK(amg_calls_load_json(nullptr, &c) == AMG_E_ARG && amg_calls_load_json(dup.c_str(), nullptr) == AMG_E_ARG);
  // an empty object and an empty file
  CHECK(load(put_file("e.json", " {} \n"), nullptr, &l) == AMG_OK && l.ids.empty() && l.tokens.empty() && l.off.size() == 1);
  CHECK(failed_with(load(put_file("e.json", ""), nullptr, &l), "expected an object"));
}

void check_first_use() {
  const int32_t V = 50;
  std::vector<int32_t> tokens;
  uint64_t rng = 3;
  for (int i = 0; i < 5000; ++i) {
    rng = rng * 6364136223846793005ull + 1442695040888963407ull;
    const int32_t g = (int32_t)((rng >> 33) % 48), plus = (int32_t)((rng >> 20) & 1);  // ranks 48 and 49 never occur
    tokens.push_back(plus ? V + g : V - 1 - g);
  }
  const std::vector<int32_t> wanted = {0, 7, 49, 7, 20, 47, 6};  // one rank twice, one that never occurs
  std::vector<int64_t> want(wanted.size(), -1);
  for (size_t i = 0; i < wanted.size(); ++i)
    for (size_t t = 0; t < tokens.size() && want[i] < 0; ++t)
      if ((tokens[t] >= V ? tokens[t] - V : V - 1 - tokens[t]) == wanted[i]) want[i] = (int64_t)t;
  CHECK(want[2] == -1 && want[1] == want[3] && want[1] >= 0);
  for (int n : kThreads) {
    threads(n);
    std::vector<int64_t> got(wanted.size(), -5);
    CHECK(amg_calls_first_use(tokens.data(), (int64_t)tokens.size(), 2 * V, wanted.data(), (int64_t)wanted.size(), got.data()) == AMG_OK);
    CHECK(got == want);
    CHECK(amg_calls_first_use(nullptr, 0, 2 * V, wanted.data(), (int64_t)wanted.size(), got.data()) == AMG_OK);
    CHECK(got == std::vector<int64_t>(wanted.size(), -1));
    CHECK(amg_calls_first_use(tokens.data(), (int64_t)tokens.size(), 2 * V, nullptr, 0, nullptr) == AMG_OK);
    std::vector<int32_t> outside = tokens;
    outside[4000] = 2 * V;
    CHECK(failed_with(amg_calls_first_use(outside.data(), (int64_t)outside.size(), 2 * V, wanted.data(), (int64_t)wanted.size(), got.data()), "outside [0, two_v)"));
    outside[4000] = -1;
    CHECK(failed_with(amg_calls_first_use(outside.data(), (int64_t)outside.size(), 2 * V, wanted.data(), (int64_t)wanted.size(), got.data()), "outside [0, two_v)"));
  }
  const int32_t bad_rank = V;
  int64_t first;
  CHECK(failed_with(amg_calls_first_use(tokens.data(), (int64_t)tokens.size(), 2 * V, &bad_rank, 1, &first), "rank outside [0, V)"));
}

void check_block_cache(const Data& plain) {
  const std::string cj = put_file("c.json", calls_text(plain)), pj = put_file("p.json", positions_text(plain));
  threads(5);
  Loaded first, l;
  CHECK(load(cj, pj.c_str(), &first) == AMG_OK);
  for (int no_cache = 0; no_cache < 2; ++no_cache) {
    if (no_cache) setenv("AMG_CALLS_NO_CACHE", "1", 1);
    int64_t released = -1;
    CHECK(amg_calls_trim(nullptr) == AMG_OK);
    CHECK(load(cj, pj.c_str(), &l) == AMG_OK && l == first);
    CHECK(amg_calls_trim(&released) == AMG_OK && (no_cache ? released == 0 : released > 0));
    CHECK(amg_calls_trim(&released) == AMG_OK && released == 0);
    CHECK(load(cj, pj.c_str(), &l) == AMG_OK && l == first);
    CHECK(load(cj, pj.c_str(), &l) == AMG_OK && l == first);  // (served from the kept blocks, where they are kept)
  }
  unsetenv("AMG_CALLS_NO_CACHE");
}

void check_sha256() {
  const std::pair<std::string, const char*> vectors[] = {
      {"", "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855"},
      {"abc", "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"},
      {"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1"},
      {std::string(64, 'a'), "ffe054fe7ae0cb6dc65c3af9b61d5209f439851db43d0ba5997337df154668eb"}};  // padding opens a second block
  for (auto& v : vectors) {
    uint8_t out[32];
    amgc::sha256(reinterpret_cast<const uint8_t*>(v.first.data()), v.first.size(), out);
    std::string hex;
    for (uint8_t b : out) { char x[4]; snprintf(x, sizeof(x), "%02x", b); hex += x; }
    CHECK(hex == v.second);
  }
}
}  // namespace

int main() {
  const char* tmp = getenv("TMPDIR");
  std::string pattern = std::string(tmp && *tmp ? tmp : "/tmp") + "/calls_check.XXXXXX";
  CHECK(mkdtemp(&pattern[0]) != nullptr);
  g_dir = pattern;
  const Data plain = make_data();
  check_sha256();
  check_loader_in_pieces(plain);
  check_position_errors(plain);
  check_position_writers();
  check_writers_replace(plain);
  check_errors(plain);
  check_first_use();
  check_block_cache(plain);
  amg_calls_trim(nullptr);
  std::filesystem::remove_all(g_dir);
  printf("calls_check: all cases passed\n");
  return 0;
}
