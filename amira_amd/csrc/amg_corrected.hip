// amg_corrected.hip — the corrected read set at the boundary: handing it to the host (64- and 32-bit positions),
// 32-bit positions coming in, and making it the current read set of this or another context.
#include "amg_correct.h"

// positions of the corrected set, gathered from the pools (only when the host asks for them)
__global__ __launch_bounds__(256) void k_gather_positions(CorrArgs a, const long long* __restrict__ c_off,
                                                          const long long* __restrict__ c_posoff, long long c_reads,
                                                          long long* __restrict__ o_gs, long long* __restrict__ o_ge) {
  const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= c_reads) return;
  const int lane = threadIdx.x & 63;
  const long long a0 = c_off[q], n = c_off[q + 1] - a0;
  const long long *gs, *ge;
  pos_base(a, c_posoff[q], gs, ge);
  for (long long i = lane; i < n; i += 64) {
    o_gs[a0 + i] = gs[i];
    o_ge[a0 + i] = ge[i];
  }
}

// arguments of the gather kernels: they read the position pools and nothing else
static CorrArgs pool_args(amg_ctx* c) {
  CorrArgs a;
  memset(&a, 0, sizeof(a));
  fill_pos_args(c, a);
  return a;
}

// one array of the corrected set to the host (a null destination: the caller does not want it)
static int to_host(amg_ctx* c, void* dst, const DevBuf& src, size_t bytes) {
  if (!dst || !bytes) return AMG_OK;
  HIPCHK(hipMemcpyAsync(dst, src.p, bytes, hipMemcpyDeviceToHost, c->stream));
  return AMG_OK;
}

extern "C" int amg_get_corrected(amg_ctx* c, int32_t* tokens, int64_t* read_offsets, int32_t* orig_read,
                                 uint8_t* changed, int64_t* gene_start, int64_t* gene_end) {
  if (!c) return amg_fail(AMG_E_ARG, "null ctx");
  if (!c->have_corrected) return amg_fail(AMG_E_STATE, "amg_correct_reads or amg_select_reads first");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  AMGCHK(to_host(c, tokens, c->c_tokens_buf, (size_t)c->c_tokens * sizeof(int32_t)));
  AMGCHK(to_host(c, read_offsets, c->c_read_off, (size_t)(c->c_reads + 1) * sizeof(int64_t)));
  AMGCHK(to_host(c, orig_read, c->c_orig, (size_t)c->c_reads * sizeof(int32_t)));
  AMGCHK(to_host(c, changed, c->c_changed, (size_t)c->c_reads));
  if (c->have_pos && (gene_start || gene_end) && c->c_tokens > 0) {
    AMGCHK(c->c_gstart.ensure((size_t)(c->c_tokens + 64) * sizeof(long long)));
    AMGCHK(c->c_gend.ensure((size_t)(c->c_tokens + 64) * sizeof(long long)));
    const CorrArgs a = pool_args(c);
    hipLaunchKernelGGL(k_gather_positions, dim3(nblk(c->c_reads, 4)), dim3(256), 0, st, a,
                       c->c_read_off.as<long long>(), c->c_pos_off.as<long long>(), (long long)c->c_reads,
                       c->c_gstart.as<long long>(), c->c_gend.as<long long>());
    AMGCHK(to_host(c, gene_start, c->c_gstart, (size_t)c->c_tokens * sizeof(int64_t)));
    AMGCHK(to_host(c, gene_end, c->c_gend, (size_t)c->c_tokens * sizeof(int64_t)));
  }
  HIPCHK(hipStreamSynchronize(st));
  return AMG_OK;
}

// ---- 32-bit positions at the boundary.  Read coordinates fit 32 bits; the position arrays are four fifths of what a
// cleaning sweep moves over PCIe (16 of 20 bytes per gene).  amg_set_positions32 takes them as int32 (widened on the
// device into the engine's own arrays); amg_get_corrected32 hands back, for every corrected read, WHERE its positions
// are — a slice of the caller's own arrays for a read that was left alone or only trimmed, new values (int32, laid end
// to end) only for the reads whose positions the carry-over produced.
__global__ void k_widen_pos(const int* __restrict__ s32, const int* __restrict__ e32, long long n,
                            long long* __restrict__ s64, long long* __restrict__ e64) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    s64[i] = (long long)s32[i];
    e64[i] = (long long)e32[i];
  }
}

extern "C" int amg_set_positions32(amg_ctx* c, const int32_t* gene_start, const int32_t* gene_end,
                                   const int64_t* read_len, int on_device) {
  if (!c) return amg_fail(AMG_E_ARG, "null ctx");
  if (c->two_v <= 0) return amg_fail(AMG_E_STATE, "amg_set_reads first");
  if (!gene_start || !gene_end) return amg_fail(AMG_E_ARG, "null positions");
  if (on_device != 0 && on_device != 1) return amg_fail(AMG_E_ARG, "amg_set_positions32: on_device is 0 or 1 (the arrays are widened, never borrowed)");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const long long T = c->n_tokens;
  const int* d_s = gene_start;
  const int* d_e = gene_end;
  if (!on_device) {  // staged in the buffers the read-back of a correction uses (free until then)
    AMGCHK(c->c_gstart.ensure((size_t)(T + 64) * sizeof(long long)));
    AMGCHK(c->c_gend.ensure((size_t)(T + 64) * sizeof(long long)));
    if (T > 0) {
      HIPCHK(hipMemcpyAsync(c->c_gstart.p, gene_start, (size_t)T * sizeof(int), hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(c->c_gend.p, gene_end, (size_t)T * sizeof(int), hipMemcpyHostToDevice, st));
    }
    d_s = c->c_gstart.as<int>();
    d_e = c->c_gend.as<int>();
  }
  c->gene_start.unborrow();
  c->gene_end.unborrow();
  AMGCHK(c->gene_start.ensure((size_t)(T + 64) * sizeof(long long)));
  AMGCHK(c->gene_end.ensure((size_t)(T + 64) * sizeof(long long)));
  if (T > 0)
    hipLaunchKernelGGL(k_widen_pos, dim3(nblk(T, 1024) < 4096u ? nblk(T, 1024) : 4096u), dim3(256), 0, st, d_s, d_e, T,
                       c->gene_start.as<long long>(), c->gene_end.as<long long>());
  ctx_positions_replaced(c, T, false);
  if (read_len) {
    c->read_len.unborrow();
    AMGCHK(c->read_len.ensure((size_t)c->n_reads * sizeof(int64_t) + 64));
    if (c->n_reads > 0)
      HIPCHK(hipMemcpyAsync(c->read_len.p, read_len, (size_t)c->n_reads * sizeof(int64_t),
                            on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    ctx_read_lengths_set(c);
  }
  HIPCHK(hipStreamSynchronize(st));
  return AMG_OK;
}

// per corrected read: number of positions the carry-over produced for it (0: its positions are a slice of the caller's)
// (own: indices below it are the CALLER's arrays — 0 once amg_adopt_corrected has compacted the pools into arrays of
// the engine's own, after which every read's positions travel)
__global__ void k_new_pos_len(const long long* __restrict__ c_off, const long long* __restrict__ c_posoff, long long own,
                              long long c_reads, long long* __restrict__ len) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < c_reads) len[q] = c_posoff[q] >= own ? c_off[q + 1] - c_off[q] : 0;
}

__global__ __launch_bounds__(256) void k_gather_new_positions32(CorrArgs a, const long long* __restrict__ c_off,
                                                                const long long* __restrict__ c_posoff, long long c_reads,
                                                                const long long* __restrict__ new_off,
                                                                long long* __restrict__ pos_src, int* __restrict__ o_gs,
                                                                int* __restrict__ o_ge, unsigned long long* too_wide,
                                                                long long own) {
  const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= c_reads) return;
  const int lane = threadIdx.x & 63;
  const long long off = c_posoff[q];
  if (off < own) {
    if (lane == 0) pos_src[q] = off;
    return;
  }
  const long long n = c_off[q + 1] - c_off[q], at = new_off[q];
  if (lane == 0) pos_src[q] = -1 - at;
  const long long *gs, *ge;
  pos_base(a, off, gs, ge);
  bool wide = false;
  for (long long i = lane; i < n; i += 64) {
    const long long s = gs[i], e = ge[i];
    wide = wide || s != (long long)(int)s || e != (long long)(int)e;
    o_gs[at + i] = (int)s;
    o_ge[at + i] = (int)e;
  }
  if (wide) *too_wide = 1ull;
}

extern "C" int amg_get_corrected32(amg_ctx* c, int32_t* tokens, int64_t* read_offsets, int32_t* orig_read,
                                   uint8_t* changed, int64_t* pos_src, int32_t* new_start, int32_t* new_end,
                                   int64_t* n_new) {
  if (!c) return amg_fail(AMG_E_ARG, "null ctx");
  if (!c->have_corrected) return amg_fail(AMG_E_STATE, "amg_correct_reads or amg_select_reads first");
  if (!pos_src || !n_new) return amg_fail(AMG_E_ARG, "amg_get_corrected32: pos_src and n_new are required");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const long long R = c->c_reads;
  *n_new = 0;
  AMGCHK(to_host(c, tokens, c->c_tokens_buf, (size_t)c->c_tokens * sizeof(int32_t)));
  AMGCHK(to_host(c, read_offsets, c->c_read_off, (size_t)(R + 1) * sizeof(int64_t)));
  AMGCHK(to_host(c, orig_read, c->c_orig, (size_t)R * sizeof(int32_t)));
  AMGCHK(to_host(c, changed, c->c_changed, (size_t)R));
  if (!c->have_pos || R == 0) {
    HIPCHK(hipStreamSynchronize(st));
    return c->have_pos ? AMG_OK : amg_fail(AMG_E_STATE, "amg_get_corrected32: no positions were set");
  }
  // lengths -> offsets of the new positions (s1: lengths + their prefix, s2: pos_src), then one gather
  AMGCHK(c->s1.ensure((size_t)(2 * R + 4) * sizeof(long long)));
  AMGCHK(c->s2.ensure((size_t)(R + 2) * sizeof(long long)));
  AMGCHK(c->c_gstart.ensure((size_t)(c->c_tokens + 64) * sizeof(long long)));
  AMGCHK(c->c_gend.ensure((size_t)(c->c_tokens + 64) * sizeof(long long)));
  long long* len = c->s1.as<long long>();
  long long* off = len + (R + 2);
  const CorrArgs a = pool_args(c);
  unsigned long long* flag = c->status.as<unsigned long long>() + ST_MISC;
  HIPCHK(hipMemsetAsync(flag, 0, sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(len + R, 0, sizeof(long long), st));
  const long long own = c->pos0_own ? 0 : a.n0;
  hipLaunchKernelGGL(k_new_pos_len, dim3(nblk(R, 256)), dim3(256), 0, st, c->c_read_off.as<long long>(),
                     c->c_pos_off.as<long long>(), own, R, len);
  AMGCHK(prim_exscan_i64(c, len, off, (size_t)R + 1));
  hipLaunchKernelGGL(k_gather_new_positions32, dim3(nblk(R, 4)), dim3(256), 0, st, a, c->c_read_off.as<long long>(),
                     c->c_pos_off.as<long long>(), R, off, c->s2.as<long long>(), c->c_gstart.as<int>(),
                     c->c_gend.as<int>(), flag, own);
  unsigned long long h[2] = {0, 0};
  {
    FetchList l;
    l.add(off + R);
    l.add(flag);
    AMGCHK(fetch(c, l, h));
  }
  if (h[1]) return amg_fail(AMG_E_ARG, "amg_get_corrected32: a position does not fit 32 bits (amg_get_corrected returns 64-bit positions)");
  *n_new = (int64_t)h[0];
  AMGCHK(to_host(c, pos_src, c->s2, (size_t)R * sizeof(int64_t)));
  AMGCHK(to_host(c, new_start, c->c_gstart, (size_t)h[0] * sizeof(int32_t)));
  AMGCHK(to_host(c, new_end, c->c_gend, (size_t)h[0] * sizeof(int32_t)));
  HIPCHK(hipStreamSynchronize(st));
  return AMG_OK;
}

// every corrected read's positions laid end to end as 32-bit values (gathered on the device: half the bytes of
// amg_get_corrected's position arrays over PCIe, and those arrays are four fifths of what a correction hands back)
__global__ __launch_bounds__(256) void k_gather_positions32(CorrArgs a, const long long* __restrict__ c_off,
                                                            const long long* __restrict__ c_posoff, long long c_reads,
                                                            int* __restrict__ o_gs, int* __restrict__ o_ge,
                                                            unsigned long long* too_wide) {
  const long long q = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= c_reads) return;
  const int lane = threadIdx.x & 63;
  const long long a0 = c_off[q], n = c_off[q + 1] - a0;
  const long long *gs, *ge;
  pos_base(a, c_posoff[q], gs, ge);
  bool wide = false;
  for (long long i = lane; i < n; i += 64) {
    const long long s = gs[i], e = ge[i];
    wide = wide || s != (long long)(int)s || e != (long long)(int)e;
    o_gs[a0 + i] = (int)s;
    o_ge[a0 + i] = (int)e;
  }
  if (wide) *too_wide = 1ull;
}

extern "C" int amg_get_corrected_positions32(amg_ctx* c, int32_t* gene_start, int32_t* gene_end) {
  if (!c || !gene_start || !gene_end) return amg_fail(AMG_E_ARG, "null argument");
  if (!c->have_corrected) return amg_fail(AMG_E_STATE, "amg_correct_reads or amg_select_reads first");
  if (!c->have_pos) return amg_fail(AMG_E_STATE, "no gene positions were set");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const long long R = c->c_reads, T = c->c_tokens;
  if (T == 0) return AMG_OK;
  AMGCHK(c->c_gstart.ensure((size_t)(T + 64) * sizeof(long long)));
  AMGCHK(c->c_gend.ensure((size_t)(T + 64) * sizeof(long long)));
  unsigned long long* flag = c->status.as<unsigned long long>() + ST_MISC;
  HIPCHK(hipMemsetAsync(flag, 0, sizeof(unsigned long long), st));
  const CorrArgs a = pool_args(c);
  hipLaunchKernelGGL(k_gather_positions32, dim3(nblk(R, 4)), dim3(256), 0, st, a, c->c_read_off.as<long long>(),
                     c->c_pos_off.as<long long>(), R, c->c_gstart.as<int>(), c->c_gend.as<int>(), flag);
  unsigned long long wide = 0;
  {
    FetchList l;
    l.add(flag);
    AMGCHK(fetch(c, l, &wide));
  }
  if (wide) return amg_fail(AMG_E_ARG, "amg_get_corrected_positions32: a position does not fit 32 bits (amg_get_corrected returns 64-bit positions)");
  HIPCHK(hipMemcpyAsync(gene_start, c->c_gstart.p, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(gene_end, c->c_gend.p, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return AMG_OK;
}

extern "C" int amg_adopt_corrected(amg_ctx* c) {
  if (!c) return amg_fail(AMG_E_ARG, "null ctx");
  if (!c->have_corrected) return amg_fail(AMG_E_STATE, "amg_correct_reads or amg_select_reads first");
  // borrowed genes / offsets / lengths go back to their owner: the corrected set lives in our own
  // allocations.  The position arrays stay where they are (borrowed or not): corrected reads point
  // into them and into the pool of produced positions.
  // The pool of produced positions only grows while corrections follow each other without a new
  // amg_set_positions.  Once it holds more than twice the live genes the corrected set's positions are gathered
  // into flat arrays of our own, which become the new "caller's arrays" (borrowed ones go back to their owner
  // here, earlier than the contract promises), and the pool starts empty again.
  bool compacted = false;
  if (c->have_pos && c->c_tokens > 0) {
    long long slack = 1ll << 20;
    if (const char* e = getenv("AMG_POS_COMPACT_MIN")) slack = atoll(e);  // test hook
    if (c->c_pos1_used > 2 * c->c_tokens + slack) {
      HIPCHK(hipSetDevice(c->device));
      AMGCHK(c->c_gstart.ensure((size_t)(c->c_tokens + 64) * sizeof(long long)));
      AMGCHK(c->c_gend.ensure((size_t)(c->c_tokens + 64) * sizeof(long long)));
      const CorrArgs a = pool_args(c);
      hipLaunchKernelGGL(k_gather_positions, dim3(nblk(c->c_reads, 4)), dim3(256), 0, c->stream, a,
                         c->c_read_off.as<long long>(), c->c_pos_off.as<long long>(), (long long)c->c_reads,
                         c->c_gstart.as<long long>(), c->c_gend.as<long long>());
      HIPCHK(hipStreamSynchronize(c->stream));  // the borrowed arrays are read for the last time
      c->gene_start.unborrow();
      c->gene_end.unborrow();
      std::swap(c->gene_start, c->c_gstart);
      std::swap(c->gene_end, c->c_gend);
      compacted = true;  // (pool 0 is no longer what the caller handed over)
    }
  }
  for (DevBuf* b : {&c->tokens, &c->read_off, &c->read_len}) b->unborrow();
  std::swap(c->tokens, c->c_tokens_buf);
  std::swap(c->read_off, c->c_read_off);
  std::swap(c->rd_src, c->c_src);
  if (c->have_pos && !compacted) std::swap(c->pos_off, c->c_pos_off);
  if (c->have_read_len) std::swap(c->read_len, c->c_read_len);
  ctx_corrected_adopted(c, compacted);
  return AMG_OK;
}

// The corrected set of `src` becomes the read set of `dst`, device to device: what the reference does between
// correct_reads and the next GeneMerGraph(...) (graph_utils.py:147-150, :165) without the reads leaving the GPU.
// Positions are gathered into flat arrays of dst's own (pool 0, identity offsets); src keeps its corrected set.
extern "C" int amg_set_reads_from_corrected(amg_ctx* dst, amg_ctx* src) {
  if (!dst || !src) return amg_fail(AMG_E_ARG, "null ctx");
  if (!src->have_corrected) return amg_fail(AMG_E_STATE, "amg_correct_reads or amg_select_reads on the source ctx first");
  if (dst == src) return amg_adopt_corrected(src);
  if (dst->device != src->device) return amg_fail(AMG_E_ARG, "amg_set_reads_from_corrected: one device");
  HIPCHK(hipSetDevice(dst->device));
  HIPCHK(hipStreamSynchronize(src->stream));
  hipStream_t st = dst->stream;
  const long long R = src->c_reads, T = src->c_tokens;
  AMGCHK(dst->tokens.ensure((size_t)T * sizeof(int32_t) + 64));
  AMGCHK(dst->read_off.ensure((size_t)(R + 1) * sizeof(int64_t) + 64));
  if (T > 0) HIPCHK(hipMemcpyAsync(dst->tokens.p, src->c_tokens_buf.p, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(dst->read_off.p, src->c_read_off.p, (size_t)(R + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
  ctx_reads_replaced(dst, R, T, src->two_v);  // (dst has no graph of its own any more)
  if (src->have_pos) {
    AMGCHK(dst->gene_start.ensure((size_t)(T + 64) * sizeof(long long)));
    AMGCHK(dst->gene_end.ensure((size_t)(T + 64) * sizeof(long long)));
    if (R > 0 && T > 0) {
      const CorrArgs a = pool_args(src);
      hipLaunchKernelGGL(k_gather_positions, dim3(nblk(R, 4)), dim3(256), 0, st, a, src->c_read_off.as<long long>(),
                         src->c_pos_off.as<long long>(), R, dst->gene_start.as<long long>(),
                         dst->gene_end.as<long long>());
    }
    ctx_positions_replaced(dst, T, true);  // gathered here: not arrays any caller holds
  }
  if (src->have_read_len) {
    AMGCHK(dst->read_len.ensure((size_t)(R + 1) * sizeof(long long) + 64));
    if (R > 0)
      HIPCHK(hipMemcpyAsync(dst->read_len.p, src->c_read_len.p, (size_t)R * sizeof(long long), hipMemcpyDeviceToDevice, st));
    ctx_read_lengths_set(dst);
  }
  HIPCHK(hipStreamSynchronize(st));
  // (amg_adopt_corrected: the same bound — for a build at the gene-mer size it was made for)
  dst->hint_bound = src->c_node_bound;
  dst->hint_bound_k = src->c_node_bound_k;
  return AMG_OK;
}
