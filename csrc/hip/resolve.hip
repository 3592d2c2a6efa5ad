// After the filter passes: the step gate, the resolve with its compaction of the outputs (K16)
// and the metadata column (K18). (kernel_common.h: the families, the launch ABI.)
#include "kernel_common.h"

#include "../common/gate.h"
#include "../common/metafmt.h"
// doc_text.h: nothing here calls it. It defines a static __constant__ table (g_wb_pair_tab), and a
// table defined in a header is emitted into every unit that includes it, read or not; the include
// keeps this unit's code object what it was while every unit included all of docproc.h. Follow-up:
// declare the table where it is read, then drop this include (180 bytes of .rodata go with it).
#include "../common/doc_text.h"

namespace {

// Step gate (csrc/common/gate.h): one thread per document. A live document that a step of the
// just-finished pass filters (or that a kernel flagged for the CPU path) gets `code`: later
// passes skip it. Codes are written once, so dead[doc] = the first pass the document skipped.
__global__ __launch_bounds__(256) void k_gate(const DevGate* __restrict__ gate, GateRecs recs, int32_t ndocs,
                                              const uint32_t* __restrict__ flags, uint8_t* dead, uint8_t code) {
  const int doc = blockIdx.x * blockDim.x + threadIdx.x;
  if (doc >= ndocs || dead[doc]) return;
  bool fail = flags[doc] != 0;
  const int ns = gate->n_steps;
  for (int s = 0; s < ns && !fail; ++s) {
    const DevGateStep& g = gate->steps[s];
    if (g.kind == GK_NONE) continue;
    const int64_t* r = recs.p[g.slot] + (int64_t)g.prefix * ndocs + (int64_t)doc * g.width;
    fail = gate_fails(g, r);
  }
  if (fail) dead[doc] = code;
}

}  // namespace

extern "C" {

int tb_gate(hipStream_t stream, const void* gate, const int64_t* const* recs, int32_t nrecs, int32_t ndocs,
            const uint32_t* flags, uint8_t* dead, int32_t code) {
  if (ndocs <= 0) return 0;
  if (nrecs < 0 || nrecs > kMaxGateSteps || code <= 0 || code > 255) return (int)hipErrorInvalidValue;
  GateRecs r{};
  for (int i = 0; i < nrecs; ++i) r.p[i] = recs[i];
  hipLaunchKernelGGL(k_gate, dim3((ndocs + 255) / 256), dim3(256), 0, stream, (const DevGate*)gate, r, ndocs, flags,
                     dead, (uint8_t)code);
  return (int)hipGetLastError();
}

size_t tb_sizeof_gate() { return sizeof(DevGate); }

}  // extern "C"

namespace {

// K16 resolve (csrc/common/gate.h resolve_doc): one thread per document. Writes the first failing
// step, the status, and the compaction inputs of the outputs: per document 4 int64 lanes
// {kept bytes, excluded bytes, kept count, excluded count} of its final content version, which four
// strided scans turn into output positions and byte offsets for k_compact.
struct VersionTab {
  const uint8_t* b[kMaxVersions];
  const int64_t* off[kMaxVersions];
};

__global__ __launch_bounds__(256) void k_resolve(const DevResolve* __restrict__ rp, GateRecs recs, int32_t ndocs,
                                                 const uint32_t* __restrict__ flags, VersionTab vt,
                                                 int32_t* __restrict__ fail, uint8_t* __restrict__ status,
                                                 uint8_t* __restrict__ fver, int64_t* __restrict__ lanes) {
  const int doc = blockIdx.x * blockDim.x + threadIdx.x;
  if (doc >= ndocs) return;
  int32_t f, v;
  uint8_t st;
  resolve_doc(*rp, recs.p, ndocs, doc, flags[doc], f, st, v);
  fail[doc] = f;
  status[doc] = st;
  fver[doc] = (uint8_t)v;
  const int64_t len = vt.off[v][doc + 1] - vt.off[v][doc];
  int64_t* l = lanes + 4 * (int64_t)doc;
  l[0] = st == kResolveKept ? len : 0;
  l[1] = st == kResolveFiltered ? len : 0;
  l[2] = st == kResolveKept ? 1 : 0;
  l[3] = st == kResolveFiltered ? 1 : 0;
}

// K16 compaction: one 256-thread workgroup per document copies its final content into the output
// buffer — kept documents first, then excluded ones, each group in document order (the order the
// host path produces) — and writes its output row and start offset. sc = the four inclusive scans
// [kept bytes | excluded bytes | kept count | excluded count], n entries each. The copy works in
// destination-aligned dwords: each thread loads the two source dwords that cover its destination
// dword and funnel-shifts them together (v_alignbyte), so interior bytes move 4 at a time whatever
// the relative alignment; only the partial first and last destination dwords go byte by byte.
// Source reads may run up to 3 bytes past a document (the batch and version buffers are padded).
constexpr int kCompactThreads = 256;  // LANES threads per document: 64 (four per workgroup) or 256

template <int kCompactLanes>
__global__ __launch_bounds__(kCompactThreads) void k_compact(const uint8_t* __restrict__ status,
                                                             const uint8_t* __restrict__ fver, VersionTab vt,
                                                             int32_t ndocs, const int64_t* __restrict__ sc,
                                                             uint8_t* __restrict__ out, int64_t cap,
                                                             int64_t* __restrict__ out_off, int32_t* __restrict__ rows,
                                                             int32_t* __restrict__ err) {
  const int doc = (int)blockIdx.x * (kCompactThreads / kCompactLanes) + (int)(threadIdx.x / kCompactLanes);
  const int t = (int)(threadIdx.x % kCompactLanes);
  if (doc >= ndocs) return;
  const int64_t n = ndocs;
  const int64_t nk = sc[3 * n - 1], nx = sc[4 * n - 1], kb = sc[n - 1], xb = sc[2 * n - 1];
  if (doc == 0 && t == 0) out_off[nk + nx] = kb + xb;
  const uint8_t st = status[doc];
  if (st != kResolveKept && st != kResolveFiltered) return;
  const int v = fver[doc];
  const int64_t s0 = vt.off[v][doc], len = vt.off[v][doc + 1] - s0;
  int64_t pos, boff;
  if (st == kResolveKept) {
    pos = sc[2 * n + doc] - 1;
    boff = sc[doc] - len;
  } else {
    pos = nk + sc[3 * n + doc] - 1;
    boff = kb + sc[n + doc] - len;
  }
  if (boff < 0 || len < 0 || boff + len > cap) {  // never with the C4 growth bound; checked anyway
    if (t == 0) *err = 1;
    return;
  }
  if (t == 0) {
    out_off[pos] = boff;
    rows[pos] = doc;
  }
  if (len == 0) return;
  const uint8_t* src = vt.b[v] + s0;
  uint8_t* dst = out + boff;
  // destination dwords fully inside [boff, boff + len): [a0, a1) in dword units of `out`
  const int64_t a0 = (boff + 3) >> 2, a1 = (boff + len) >> 2;
  if (a1 <= a0) {  // short: no whole destination dword
    for (int64_t i = t; i < len; i += kCompactLanes) dst[i] = src[i];
    return;
  }
  const int64_t head = a0 * 4 - boff, tail = boff + len - a1 * 4;  // bytes before / after
  if (t < head) dst[t] = src[t];
  if (t < tail) dst[len - tail + t] = src[len - tail + t];
  // destination dword w (absolute) takes source bytes from sp = src + (4w - boff)
  const uintptr_t sbase = (uintptr_t)src + (uintptr_t)head;  // source of the first whole dword
  const uint32_t sh = (uint32_t)(sbase & 3u);
  const uint32_t* s32 = (const uint32_t*)(sbase - sh);
  uint32_t* d32 = (uint32_t*)out + a0;
  const int64_t nw = a1 - a0;
  for (int64_t k = t; k < nw; k += kCompactLanes) {
    const uint32_t lo = s32[k];
    const uint32_t hi = sh ? s32[k + 1] : 0u;
    // little endian: bytes sh.. of lo, then the low bytes of hi
    d32[k] = sh ? __builtin_amdgcn_alignbyte(hi, lo, sh) : lo;
  }
}

}  // namespace

extern "C" {

struct TbResolveOut {  // outputs and scratch of tb_resolve
  int32_t* fail;
  uint8_t *status, *fver;
  int64_t *lanes, *sc;
  uint8_t* out;
  int64_t cap;  // bytes of out
  int64_t* out_off;
  int32_t *rows, *err;
};
size_t tb_sizeof_resolve_out() { return sizeof(TbResolveOut); }
size_t tb_sizeof_resolve() { return sizeof(DevResolve); }

// K16: resolve + four scans + compaction, all on `stream`. vb/vo: content versions 0..nver-1;
// lanes: 4*ndocs int64 scratch, sc: 4*ndocs int64 scan output; out must hold the final contents
// (cap bytes: the caller bounds it by version 0 plus the C4 growth; a document that would pass
// the end sets *err and is not written), out_off ndocs+1, rows ndocs.
int tb_resolve(hipStream_t stream, const void* rp, const int64_t* const* recs, int32_t nrecs, int32_t ndocs,
               const uint32_t* flags, const uint8_t* const* vb, const int64_t* const* vo, int32_t nver,
               const TbResolveOut* o) {
  int32_t *fail = o->fail, *rows = o->rows, *err = o->err;
  uint8_t *status = o->status, *fver = o->fver, *out = o->out;
  int64_t *lanes = o->lanes, *sc = o->sc, *out_off = o->out_off;
  const int64_t cap = o->cap;
  if (ndocs <= 0) return 0;
  if (nrecs < 0 || nrecs > kMaxGateSteps || nver < 1 || nver > kMaxVersions) return (int)hipErrorInvalidValue;
  GateRecs r{};
  for (int i = 0; i < nrecs; ++i) r.p[i] = recs[i];
  VersionTab vt{};
  for (int i = 0; i < nver; ++i) {
    vt.b[i] = vb[i];
    vt.off[i] = vo[i];
  }
  hipLaunchKernelGGL(k_resolve, dim3((ndocs + 255) / 256), dim3(256), 0, stream, (const DevResolve*)rp, r, ndocs,
                     flags, vt, fail, status, fver, lanes);
  for (int j = 0; j < 4; ++j) {
    const int rc = tb_scan_strided_i64(stream, lanes + j, 4, ndocs, sc + (int64_t)j * ndocs);
    if (rc) return rc;
  }
  // one wave per document (short documents, the common case), a whole workgroup per document once
  // they average over 8 KB (the output holds every document, so cap / ndocs is about their length)
  if (cap / (ndocs > 0 ? ndocs : 1) > 8192)
    hipLaunchKernelGGL(k_compact<256>, dim3(ndocs), dim3(kCompactThreads), 0, stream, status, fver, vt, ndocs, sc, out, cap, out_off, rows,
                     err);
  else
    hipLaunchKernelGGL(k_compact<64>, dim3((ndocs + 3) / 4), dim3(kCompactThreads), 0, stream, status, fver, vt, ndocs, sc, out, cap, out_off, rows,
                     err);
  return (int)hipGetLastError();
}

}  // extern "C"

namespace {

// K18: the metadata column of the compacted outputs (csrc/common/metafmt.h). Output row pos
// (kept rows first, then excluded, the order of k_compact's `rows`) is formatted from the records
// of document rows[pos]; nk / nx are the last entries of the kept / excluded count scans.
struct MetaTokens {
  const int32_t* p[kMaxMetaTokens];  // k_bpe_count results by kept output
};

// One lane per output row: byte length (0 past the last row) and validity. An unformattable row
// sets its bit of the error word (the host then assembles the batch itself).
__global__ __launch_bounds__(256) void k_meta_size(const DevResolve* __restrict__ rp, const DevMetaPlan* __restrict__ mp,
                                                   GateRecs recs, int32_t ndocs, const int32_t* __restrict__ fail,
                                                   const int32_t* __restrict__ rows, const int64_t* __restrict__ sc,
                                                   MetaTokens tk, int64_t* __restrict__ lens,
                                                   uint8_t* __restrict__ valid, int32_t* __restrict__ err) {
  const int pos = blockIdx.x * blockDim.x + threadIdx.x;
  if (pos >= ndocs) return;
  const int64_t n = ndocs;
  const int64_t nk = sc[3 * n - 1], n_rows = nk + sc[4 * n - 1];
  uint32_t len = 0;
  if (pos < n_rows) {
    const int32_t doc = rows[pos];
    if ((uint32_t)doc >= (uint32_t)ndocs) {  // k_compact ran out of room and left the row unwritten
      atomicOr(err, kMetaErrUnformattable);
    } else {
      int32_t tok[kMaxMetaTokens];
      for (int t = 0; t < kMaxMetaTokens; ++t) tok[t] = (t < mp->n_tokens && pos < nk) ? tk.p[t][pos] : -1;
      MetaCountSink k;
      if (!meta_row(*rp, *mp, recs.p, n, doc, pos < nk ? -1 : fail[doc], tok, k)) atomicOr(err, kMetaErrUnformattable);
      len = k.n;
    }
  }
  lens[pos] = len;
  valid[pos] = len > 0;
}

// One lane per output row, one wave per workgroup. A lane formats its row into its own LDS slice
// (65 dwords apart, so the lanes' byte stores fall into different banks), copying literals from an
// LDS copy of the plan's pool; the rows of a wave are consecutive in the column, so the wave then
// copies its byte range to HBM one aligned dword per lane and step (bytes at the ragged ends and
// next to a long row one by one), finding the first byte's row by bisection of the wave's 65 row
// starts. A row longer than a slice is written straight to the column by its lane and skipped by
// the copy. The barriers, the starts and the copy loop sit outside the divergent formatting: every
// lane takes part, and a lane without a row has length 0. moff: the column's offsets [ndocs + 1]
// (the scan of k_meta_size's lengths).
constexpr int kMetaSlice = 260;
constexpr int kMetaWave = 64;
constexpr int kMetaPoolLds = 4096;  // a larger pool is read from the plan in HBM

__global__ __launch_bounds__(kMetaWave) void k_meta_write(const DevResolve* __restrict__ rp,
                                                          const DevMetaPlan* __restrict__ mp, GateRecs recs,
                                                          int32_t ndocs, const int32_t* __restrict__ fail,
                                                          const int32_t* __restrict__ rows,
                                                          const int64_t* __restrict__ sc, MetaTokens tk,
                                                          const int64_t* __restrict__ moff, uint8_t* __restrict__ out,
                                                          int64_t cap, int32_t* __restrict__ err) {
  __shared__ uint32_t s_stage[kMetaWave * kMetaSlice / 4];
  __shared__ uint32_t s_pool[kMetaPoolLds / 4];
  __shared__ uint32_t s_start[kMetaWave + 1];
  const int lane = threadIdx.x;
  const int64_t n = ndocs;
  const int64_t pos0 = (int64_t)blockIdx.x * kMetaWave, pos = pos0 + lane;
  const int64_t total = moff[n];
  if (total > cap || total < 0) {  // uniform over the grid: nothing is written
    if (pos == 0) atomicOr(err, kMetaErrOverflow);
    return;
  }
  const int64_t nk = sc[3 * n - 1];
  const int64_t base = moff[pos0];
  const int64_t o0 = moff[pos < n ? pos : n], o1 = moff[pos + 1 < n ? pos + 1 : n];
  const uint32_t len = (uint32_t)(o1 - o0);
  s_start[lane] = (uint32_t)(o0 - base);
  if (lane == kMetaWave - 1) s_start[kMetaWave] = (uint32_t)(o1 - base);
  {
    const uint32_t* gp = (const uint32_t*)mp->pool;  // (the pool sits at a multiple of 4 in the plan)
    const int pool_words = (mp->pool_used + 3) >> 2;
    for (int i = lane; i < pool_words && i < kMetaPoolLds / 4; i += kMetaWave) s_pool[i] = gp[i];
  }
  const char* pool = mp->pool_used <= kMetaPoolLds ? (const char*)s_pool : mp->pool;
  __syncthreads();
  char* stage = (char*)s_stage + lane * kMetaSlice;
  const int32_t doc = pos < n ? rows[pos] : -1;
  if (len > 0 && (uint32_t)doc < (uint32_t)ndocs) {
    int32_t tok[kMaxMetaTokens];
    for (int t = 0; t < kMaxMetaTokens; ++t) tok[t] = (t < mp->n_tokens && pos < nk) ? tk.p[t][pos] : -1;
    MetaWriteSink k(len <= (uint32_t)kMetaSlice ? stage : (char*)out + o0);
    (void)meta_row(*rp, *mp, recs.p, n, doc, pos < nk ? -1 : fail[doc], tok, k, pool);
  }
  __syncthreads();
  // unit u = the aligned dword of `out` that holds the wave's bytes [4u - mis, 4u - mis + 4)
  const uint32_t w_bytes = s_start[kMetaWave];
  uint8_t* gout = out + base;
  const uint32_t mis = (uint32_t)((uintptr_t)gout & 3u);
  const uint32_t n_units = (w_bytes + mis + 3) >> 2;
  const uint8_t* stage8 = (const uint8_t*)s_stage;
  for (uint32_t u = lane; u < n_units; u += kMetaWave) {
    const int32_t j0 = (int32_t)(4 * u) - (int32_t)mis;
    const uint32_t ja = j0 < 0 ? 0u : (uint32_t)j0;
    const uint32_t jb = (uint32_t)(j0 + 4) < w_bytes ? (uint32_t)(j0 + 4) : w_bytes;
    int r = 0, hi = kMetaWave - 1;  // the last row with start <= ja (rows of length 0 share a start)
    while (r < hi) {
      const int mid = (r + hi + 1) >> 1;
      if (s_start[mid] <= ja) r = mid;
      else hi = mid - 1;
    }
    uint32_t word = 0, have = 0;
    for (uint32_t j = ja; j < jb; ++j) {
      while (s_start[r + 1] <= j) ++r;  // j < w_bytes = s_start[64]: r stays <= 63
      if (s_start[r + 1] - s_start[r] <= (uint32_t)kMetaSlice) {
        const uint32_t sh = (uint32_t)((int32_t)j - j0);
        word |= (uint32_t)stage8[r * kMetaSlice + (j - s_start[r])] << (8 * sh);
        have |= 1u << sh;
      }
    }
    if (have == 0xFu) {
      *(uint32_t*)(gout + j0) = word;
    } else {
      for (uint32_t b = 0; b < 4; ++b)
        if (have >> b & 1) gout[j0 + (int32_t)b] = (uint8_t)(word >> (8 * b));
    }
  }
}

}  // namespace

extern "C" {

// K18 after tb_resolve (and the token counts) on `stream`: k_meta_size, the scan of the lengths
// into off[1 .. ndocs] (off[0] = 0), k_meta_write. fail / rows / sc: tb_resolve's outputs; toks:
// ntoks k_bpe_count result arrays (= the plan's n_tokens). lens: ndocs int64 scratch, off:
// ndocs + 1, valid: ndocs, out: cap bytes (the plan's row_cap * ndocs); err: kMetaErr* bits.
struct TbMetaOut {
  int64_t *lens, *off;
  uint8_t *valid, *out;
  int64_t cap;
  int32_t* err;
};
size_t tb_sizeof_meta_out() { return sizeof(TbMetaOut); }
size_t tb_sizeof_meta_plan() { return sizeof(DevMetaPlan); }

int tb_meta_format(hipStream_t stream, const void* rp, const void* mp, const int64_t* const* recs, int32_t nrecs,
                   int32_t ndocs, const int32_t* fail, const int32_t* rows, const int64_t* sc,
                   const int32_t* const* toks, int32_t ntoks, const TbMetaOut* o) {
  if (ndocs <= 0) return 0;
  if (nrecs < 0 || nrecs > kMaxGateSteps || ntoks < 0 || ntoks > kMaxMetaTokens || !o->lens || !o->off || !o->valid ||
      !o->out || !o->err || o->cap < 0)
    return (int)hipErrorInvalidValue;
  GateRecs r{};
  for (int i = 0; i < nrecs; ++i) r.p[i] = recs[i];
  MetaTokens tk{};
  for (int i = 0; i < ntoks; ++i) tk.p[i] = toks[i];
  hipLaunchKernelGGL(k_meta_size, dim3((ndocs + 255) / 256), dim3(256), 0, stream, (const DevResolve*)rp,
                     (const DevMetaPlan*)mp, r, ndocs, fail, rows, sc, tk, o->lens, o->valid, o->err);
  (void)hipMemsetAsync(o->off, 0, sizeof(int64_t), stream);
  const int rc = tb_scan_strided_i64(stream, o->lens, 1, ndocs, o->off + 1);
  if (rc) return rc;
  hipLaunchKernelGGL(k_meta_write, dim3((ndocs + kMetaWave - 1) / kMetaWave), dim3(kMetaWave), 0, stream,
                     (const DevResolve*)rp, (const DevMetaPlan*)mp, r, ndocs, fail, rows, sc, tk,
                     (const int64_t*)o->off, o->out, o->cap, o->err);
  return (int)hipGetLastError();
}

}  // extern "C"
