// amg_names.hip — the 256-bit names of nodes and edges made on the device (include/amg.h: amg_names_create / _destroy,
// amg_node_names, amg_edge_names, amg_names_probe) and the host twin amg_names_host.  The rule itself — the pickle
// bytes, SHA-256, Python's hash of the result — is amg_names.h, shared by both.
//
//   k_names        a lane per name of a row of k tokens over the gene table: node rows by id, the two endpoint rows of
//                  an edge, or the rows of the probe.  Each lane streams its message through a ring of 32 dwords of its
//                  own in LDS (NameStream); the loop "fill, compress when 16 dwords are pending" runs until no lane of
//                  the wave has anything left, a lane that has finished does nothing in it.
//   k_edge_names   a lane per edge: the names of (s, t) and (-s, -t) over the two endpoint names k_names left in
//                  scratch, the smaller of the two.
// Output goes through a bounded device buffer (NAMES_CHUNK names by default) that is copied out chunk by chunk; all
// scratch belongs to the call and is released when it returns.
#include "amg_internal.h"
#include "amg_names.h"

struct amg_names {
  int device = 0;
  DevBuf genes;  // uint8[n_genes][32], rank order, big-endian
  int64_t n_genes = 0;
  int32_t pp = 4;
};

#define NAMES_CHUNK (1ll << 22)
#define NAMES_TPB 256
#define NAMES_STRIDE (AMG_NAMES_RING + 1)  // odd: the lanes of a ds_read / ds_write fall on distinct banks

enum NamesMode { NM_ROWS = 0, NM_NODES = 1, NM_ENDPOINTS = 2 };
struct NamesArgs {
  const uint8_t* genes;
  int32_t V, k, pp, mode;
  long long n;               // names of this launch
  const int* tokens;         // NM_ROWS: [n][k]; otherwise the graph's node_tokens
  const int* ids;            // node ids (NM_NODES) / edge ids (NM_ENDPOINTS) of this chunk, or null: base, base + 1, ..
  long long base;
  const unsigned char* alive;  // NM_NODES: node_alive, NM_ENDPOINTS: edge_alive; a dead one gets zeros
  const int *e_src, *e_tgt;    // NM_ENDPOINTS: name 2 i is the source of edge i of the chunk, 2 i + 1 its target
  uint4* out;                  // [n][2]: the digest, big-endian bytes
  long long* py;               // [n] or null
};

__device__ __forceinline__ void names_store(uint4* out, long long i, const uint32_t h[8]) {
  out[2 * i] = make_uint4(amg_bswap(h[0]), amg_bswap(h[1]), amg_bswap(h[2]), amg_bswap(h[3]));
  out[2 * i + 1] = make_uint4(amg_bswap(h[4]), amg_bswap(h[5]), amg_bswap(h[6]), amg_bswap(h[7]));
}

__global__ __launch_bounds__(NAMES_TPB) void k_names(NamesArgs a) {
  __shared__ uint32_t rings[NAMES_TPB * NAMES_STRIDE];
  const long long i = (long long)blockIdx.x * NAMES_TPB + threadIdx.x;
  bool active = i < a.n;
  long long row = 0;
  if (active) {
    if (a.mode == NM_ROWS)
      row = i;
    else if (a.mode == NM_NODES) {
      row = a.ids ? a.ids[i] : a.base + i;
      active = a.alive[row] != 0;
    } else {
      const long long e = a.ids ? a.ids[i >> 1] : a.base + (i >> 1);
      active = a.alive[e] != 0;
      row = (i & 1) ? a.e_tgt[e] : a.e_src[e];
    }
  }
  TokenRow src;
  src.genes = a.genes, src.V = a.V, src.tokens = a.tokens + row * a.k;
  NameStream s;
  s.begin(rings + threadIdx.x * NAMES_STRIDE, (uint32_t)a.k, (uint32_t)a.pp,
          active ? amg_name_body_bytes(src, a.k) : 0, active);
  while (__any(!s.done())) {  // wave-uniform: as many rounds as the wave's longest message has blocks
    s.fill(src);
    s.compress_if_full();
  }
  if (i >= a.n) return;
  if (!active)
#pragma unroll
    for (int w = 0; w < 8; ++w) s.h[w] = 0;
  names_store(a.out, i, s.h);
  if (a.py) a.py[i] = active ? amg_py_hash256(s.h) : 0;
}

struct EdgeNamesArgs {
  long long n;
  const uint8_t* ends;  // [n][2][32] from k_names(NM_ENDPOINTS)
  const int* ids;
  long long base;
  const unsigned char* alive;
  const signed char *sdir, *tdir;
  int32_t pp;
  uint4* out;
  long long* py;
};

__global__ __launch_bounds__(NAMES_TPB) void k_edge_names(EdgeNamesArgs a) {
  __shared__ uint32_t rings[NAMES_TPB * NAMES_STRIDE];
  const long long i = (long long)blockIdx.x * NAMES_TPB + threadIdx.x;
  bool active = i < a.n;
  PairRow src;
  src.two_names = a.ends + 64 * (active ? i : 0), src.sdir = src.tdir = 1, src.flip = 1;
  if (active) {
    const long long e = a.ids ? a.ids[i] : a.base + i;
    active = a.alive[e] != 0;
    src.sdir = a.sdir[e], src.tdir = a.tdir[e];
  }
  uint32_t best[8];
#pragma unroll
  for (int w = 0; w < 8; ++w) best[w] = 0;
  for (int pass = 0; pass < 2; ++pass) {  // (s, t), then (-s, -t)
    src.flip = pass ? -1 : 1;
    NameStream s;
    s.begin(rings + threadIdx.x * NAMES_STRIDE, 2u, (uint32_t)a.pp, active ? amg_name_body_bytes(src, 2) : 0, active);
    while (__any(!s.done())) {
      s.fill(src);
      s.compress_if_full();
    }
    if (active && (pass == 0 || amg_digest_less(s.h, best)))
#pragma unroll
      for (int w = 0; w < 8; ++w) best[w] = s.h[w];
  }
  if (i >= a.n) return;
  names_store(a.out, i, best);
  if (a.py) a.py[i] = active ? amg_py_hash256(best) : 0;
}

// ------------------------------------------------------------------ the handle
extern "C" int amg_names_create(int32_t device, const uint8_t* gene_digests, int64_t n_genes, int32_t pickle_protocol,
                                amg_names** out) {
  if (!out) return amg_fail(AMG_E_ARG, "amg_names_create: null out");
  *out = nullptr;
  if (!gene_digests || n_genes < 1 || n_genes > (1ll << 30))
    return amg_fail(AMG_E_ARG, "amg_names_create: %lld genes", (long long)n_genes);
  if (pickle_protocol != 4 && pickle_protocol != 5)
    return amg_fail(AMG_E_ARG, "amg_names_create: pickle protocol %d (4 and 5 are restated)", (int)pickle_protocol);
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) return amg_fail(AMG_E_HIP, "no HIP device");
  HIPCHK(hipSetDevice(device));
  amg_names* g = new amg_names();
  g->device = device, g->n_genes = n_genes, g->pp = pickle_protocol;
  int rc = g->genes.ensure((size_t)n_genes * 32);
  if (rc == AMG_OK && hipMemcpy(g->genes.p, gene_digests, (size_t)n_genes * 32, hipMemcpyHostToDevice) != hipSuccess)
    rc = amg_fail(AMG_E_HIP, "amg_names_create: the gene table did not reach the device");
  if (rc != AMG_OK) {
    g->genes.release();
    delete g;
    return rc;
  }
  *out = g;
  return AMG_OK;
}

extern "C" int amg_names_destroy(amg_names* g) {
  if (!g) return AMG_OK;
  (void)hipSetDevice(g->device);
  g->genes.release();
  delete g;
  return AMG_OK;
}

// ------------------------------------------------------------------ the launcher
// the call's own device arrays
struct NamesScratch {
  DevBuf ids, rows, out, py, ends;
  ~NamesScratch() {
    for (DevBuf* b : {&ids, &rows, &out, &py, &ends}) b->release();
  }
};
// A names call times its kernels as a stage of the ctx (amg_last_timings) only where it cannot hide another call's
// stages: when the ctx holds none, or those of an earlier names call.
static bool names_timed(amg_ctx* c) {
  if (!c->timing) return false;
  if (!c->stages.empty() && strncmp(c->stages[0].name, "names", 5) != 0) return false;
  stages_reset(c);
  return true;
}

enum NamesWhat { NAMES_OF_ROWS, NAMES_OF_NODES, NAMES_OF_EDGES };
// n names in chunks of `chunk`: ids (host, or null for 0 .. n - 1) or, for NAMES_OF_ROWS, rows[n][k] (host)
static int names_run(amg_ctx* c, const amg_names* g, NamesWhat what, const int32_t* ids, const int32_t* rows, int32_t k,
                     int64_t n, int64_t chunk, uint8_t* digests, int64_t* py_hash) {
  if (n == 0) return AMG_OK;
  if (chunk <= 0) chunk = NAMES_CHUNK;
  if (chunk > n) chunk = n;
  hipStream_t st = c->stream;
  NamesScratch S;
  AMGCHK(S.out.ensure((size_t)chunk * 32));
  if (py_hash) AMGCHK(S.py.ensure((size_t)chunk * 8));
  if (ids) AMGCHK(S.ids.ensure((size_t)chunk * 4));
  if (what == NAMES_OF_ROWS) AMGCHK(S.rows.ensure((size_t)chunk * k * 4));
  if (what == NAMES_OF_EDGES) AMGCHK(S.ends.ensure((size_t)chunk * 64));
  const bool timed = names_timed(c);
  for (int64_t at = 0; at < n; at += chunk) {
    const int64_t m = n - at < chunk ? n - at : chunk;
    if (ids) HIPCHK(hipMemcpyAsync(S.ids.p, ids + at, (size_t)m * 4, hipMemcpyHostToDevice, st));
    if (what == NAMES_OF_ROWS)
      HIPCHK(hipMemcpyAsync(S.rows.p, rows + at * k, (size_t)m * k * 4, hipMemcpyHostToDevice, st));
    if (timed) stage_begin(c, what == NAMES_OF_EDGES ? "names_edges" : "names_nodes");
    NamesArgs a;
    memset(&a, 0, sizeof(a));
    a.genes = g->genes.as<uint8_t>(), a.V = (int32_t)g->n_genes, a.pp = g->pp;
    a.ids = ids ? S.ids.as<int>() : nullptr, a.base = at;
    if (what == NAMES_OF_ROWS) {
      a.mode = NM_ROWS, a.k = k, a.n = m, a.tokens = S.rows.as<int>();
      a.out = S.out.as<uint4>(), a.py = py_hash ? S.py.as<long long>() : nullptr;
    } else if (what == NAMES_OF_NODES) {
      a.mode = NM_NODES, a.k = c->k, a.n = m, a.tokens = c->node_tokens.as<int>();
      a.alive = c->node_alive.as<unsigned char>();
      a.out = S.out.as<uint4>(), a.py = py_hash ? S.py.as<long long>() : nullptr;
    } else {
      a.mode = NM_ENDPOINTS, a.k = c->k, a.n = 2 * m, a.tokens = c->node_tokens.as<int>();
      a.alive = c->edge_alive.as<unsigned char>();
      a.e_src = c->edge_src.as<int>(), a.e_tgt = c->edge_tgt.as<int>();
      a.out = S.ends.as<uint4>(), a.py = nullptr;
    }
    hipLaunchKernelGGL(k_names, dim3(nblk(a.n, NAMES_TPB)), dim3(NAMES_TPB), 0, st, a);
    if (what == NAMES_OF_EDGES) {
      EdgeNamesArgs e;
      memset(&e, 0, sizeof(e));
      e.n = m, e.ends = S.ends.as<uint8_t>(), e.ids = a.ids, e.base = at, e.pp = g->pp;
      e.alive = c->edge_alive.as<unsigned char>();
      e.sdir = c->edge_sdir.as<signed char>(), e.tdir = c->edge_tdir.as<signed char>();
      e.out = S.out.as<uint4>(), e.py = py_hash ? S.py.as<long long>() : nullptr;
      hipLaunchKernelGGL(k_edge_names, dim3(nblk(m, NAMES_TPB)), dim3(NAMES_TPB), 0, st, e);
    }
    if (timed) stage_end(c);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(digests + at * 32, S.out.p, (size_t)m * 32, hipMemcpyDeviceToHost, st));
    if (py_hash) HIPCHK(hipMemcpyAsync(py_hash + at, S.py.p, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // the next chunk reuses the buffers
  }
  return AMG_OK;
}

static int names_args_ok(const char* who, amg_ctx* c, const amg_names* g, int64_t n, const uint8_t* digests) {
  if (!g) return amg_fail(AMG_E_ARG, "%s: null names handle", who);
  if (g->device != c->device) return amg_fail(AMG_E_ARG, "%s: the handle is on device %d, the ctx on %d", who, g->device, c->device);
  if (n < 0 || (n > 0 && !digests)) return amg_fail(AMG_E_ARG, "%s: bad arguments", who);
  return AMG_OK;
}
static int names_of_graph(const char* who, amg_ctx* c, const amg_names* g, NamesWhat what, const int32_t* ids, int64_t n,
                          uint8_t* digests, int64_t* py_hash) {
  NEED_BUILT(c);
  AMGCHK(names_args_ok(who, c, g, n, digests));
  if (2 * g->n_genes != (int64_t)c->two_v)
    return amg_fail(AMG_E_ARG, "%s: the handle names %lld genes, the ctx's reads have two_v = %d", who,
                    (long long)g->n_genes, (int)c->two_v);
  const int64_t limit = what == NAMES_OF_NODES ? c->n_nodes : c->n_edges;
  if (n == 0) return AMG_OK;
  if (ids) {
    for (int64_t i = 0; i < n; ++i)
      if (ids[i] < 0 || ids[i] >= limit)
        return amg_fail(AMG_E_ARG, "%s: id %d at %lld lies outside [0, %lld)", who, (int)ids[i], (long long)i, (long long)limit);
  } else if (n != limit)
    return amg_fail(AMG_E_ARG, "%s: without ids n must be %lld, not %lld", who, (long long)limit, (long long)n);
  return names_run(c, g, what, ids, nullptr, c->k, n, 0, digests, py_hash);
}

extern "C" int amg_node_names(amg_ctx* c, const amg_names* g, const int32_t* node_ids, int64_t n, uint8_t* digests,
                              int64_t* py_hash) {
  return names_of_graph("amg_node_names", c, g, NAMES_OF_NODES, node_ids, n, digests, py_hash);
}

extern "C" int amg_edge_names(amg_ctx* c, const amg_names* g, const int32_t* edge_ids, int64_t n, uint8_t* digests,
                              int64_t* py_hash) {
  return names_of_graph("amg_edge_names", c, g, NAMES_OF_EDGES, edge_ids, n, digests, py_hash);
}

static int names_rows_ok(const char* who, int64_t n_genes, const int32_t* rows, int64_t n, int32_t k) {
  if (k < 1 || k > AMG_NAMES_MAX_K) return amg_fail(AMG_E_ARG, "%s: k = %d lies outside [1, %d]", who, (int)k, AMG_NAMES_MAX_K);
  if (n < 0 || n > (1ll << 40) / k || (n > 0 && !rows)) return amg_fail(AMG_E_ARG, "%s: bad arguments", who);
  for (int64_t i = 0; i < n * k; ++i)
    if (rows[i] < 0 || rows[i] >= 2 * n_genes)
      return amg_fail(AMG_E_ARG, "%s: token %d at %lld lies outside [0, %lld)", who, (int)rows[i], (long long)i,
                      (long long)(2 * n_genes));
  return AMG_OK;
}

extern "C" int amg_names_probe(amg_ctx* c, const amg_names* g, const int32_t* rows, int64_t n, int32_t k,
                               int64_t chunk_names, uint8_t* digests, int64_t* py_hash) {
  if (!c) return amg_fail(AMG_E_ARG, "null ctx");
  AMGCHK(names_args_ok("amg_names_probe", c, g, n, digests));
  AMGCHK(names_rows_ok("amg_names_probe", g->n_genes, rows, n, k));
  HIPCHK(hipSetDevice(c->device));
  return names_run(c, g, NAMES_OF_ROWS, nullptr, rows, k, n, chunk_names, digests, py_hash);
}

// ------------------------------------------------------------------ the host twin: no device call
extern "C" int amg_names_host(const uint8_t* gene_digests, int64_t n_genes, int32_t pickle_protocol, const int32_t* rows,
                              int64_t n, int32_t k, uint8_t* digests, int64_t* py_hash) {
  if (!gene_digests || n_genes < 1 || n_genes > (1ll << 30))
    return amg_fail(AMG_E_ARG, "amg_names_host: %lld genes", (long long)n_genes);
  if (pickle_protocol != 4 && pickle_protocol != 5)
    return amg_fail(AMG_E_ARG, "amg_names_host: pickle protocol %d (4 and 5 are restated)", (int)pickle_protocol);
  if (n > 0 && !digests) return amg_fail(AMG_E_ARG, "amg_names_host: no room for the digests");
  AMGCHK(names_rows_ok("amg_names_host", n_genes, rows, n, k));
  std::vector<uint8_t> table;  // a copy at a 4-byte boundary, whatever the caller's pointer is
  if (reinterpret_cast<uintptr_t>(gene_digests) & 3) {
    table.assign(gene_digests, gene_digests + (size_t)n_genes * 32);
    gene_digests = table.data();
  }
  uint32_t ring[AMG_NAMES_RING];
  for (int64_t i = 0; i < n; ++i) {
    TokenRow src;
    src.genes = gene_digests, src.V = (int32_t)n_genes, src.tokens = rows + i * k;
    uint32_t h[8];
    amg_name_of_row(src, k, pickle_protocol, ring, h);
    for (int w = 0; w < 8; ++w) {
      const uint32_t be = amg_bswap(h[w]);
      memcpy(digests + i * 32 + 4 * w, &be, 4);
    }
    if (py_hash) py_hash[i] = amg_py_hash256(h);
  }
  return AMG_OK;
}
