// C4 kernels: pass A (line filtering, citation removal, the rewritten text into scratch), pass B
// (compaction into the next content version) and the bad-words matcher.
// (kernel_common.h: the families, the launch ABI.)
#include "kernel_common.h"

#include "../common/badwords.h"
#include "../common/c4_pass_a.h"

namespace {

// C4 pass A leaves src[0] relative to the document's scratch slice (the convention the host
// emulation shares); pass B copies straight out of the arena, so the leader makes it absolute.
template <class P>
__device__ __forceinline__ void c4_src_absolute(DocCtx<P>& x, int64_t* src, int64_t slice_begin) {
  if (x.par.leader() && src[0] >= 0) src[0] += slice_begin;
}

// TB_C4_WPE: register budget of the C4 pass A wave kernel (0: none). 8 waves/SIMD = 64 VGPRs,
// one fewer than it takes unconstrained: 2.86 -> 2.42 ms/step (profiles/r8_c4w8/).
// 7 waves/SIMD (70 VGPRs, no spill): with the dictionary-script inputs the 8-wave build spills 9
// VGPRs, and that build rewrote a few documents wrongly on the GPU (test_badwords_device, C4 in
// front; the 6- and 7-wave builds and the host emulation of the same source are exact) -- unexplained,
// so the kernel stays spill-free
#ifndef TB_C4_WPE
#define TB_C4_WPE 7
#endif
#if TB_C4_WPE > 0
#define TB_C4_ATTR __attribute__((amdgpu_waves_per_eu(TB_C4_WPE, 8)))
#else
#define TB_C4_ATTR
#endif
__global__ __launch_bounds__(64) TB_C4_ATTR void k_c4_pass_a(
    const DevC4* __restrict__ c4, const uint8_t* __restrict__ bytes, const int64_t* __restrict__ off,
    const int32_t* __restrict__ perm, int32_t ndocs, char* scratch, const int64_t* __restrict__ scratch_off,
    const uint64_t* __restrict__ pw, uint32_t pw_n, DevTables tabs, int64_t* rec, int64_t* src, uint32_t* flags,
    uint32_t lds_bytes, uint64_t* prof, const uint8_t* __restrict__ dead, const uint32_t* __restrict__ line_stats,
    uint32_t* c4_words, DictLines dict_lines) {
  const int doc = perm ? perm[blockIdx.x] : (int)blockIdx.x;
  if (doc >= ndocs || (dead && dead[doc])) return;  // skipped: record zeros, rewritten length 0
  DocCtx<WavePar> x = make_ctx(tabs, pw, pw_n, scratch, scratch_off, doc, (int)blockIdx.x, flags, lds_bytes, prof);
  lds_ascii_props(x);
  const uint8_t* b = bytes + off[doc];
  const uint32_t n = (uint32_t)(off[doc + 1] - off[doc]);
  c4_pass_a(x, *c4, b, n, rec + (int64_t)doc * 7, src + (int64_t)doc * 2,
            line_stats ? line_stats + line_stats_base(off[doc], doc) : nullptr, c4_words ? c4_words + doc : nullptr,
            dict_lines.at((uint32_t)doc));
  c4_src_absolute(x, src + (int64_t)doc * 2, scratch_off[blockIdx.x]);
}

__global__ __launch_bounds__(kBlockThreads) void k_c4_pass_a_blk(
    const DevC4* __restrict__ c4, const uint8_t* __restrict__ bytes, const int64_t* __restrict__ off,
    const int32_t* __restrict__ perm, int32_t ndocs, char* scratch, const int64_t* __restrict__ scratch_off,
    const uint64_t* __restrict__ pw, uint32_t pw_n, DevTables tabs, int64_t* rec, int64_t* src, uint32_t* flags,
    uint32_t lds_bytes, uint64_t* prof, const uint8_t* __restrict__ dead, const uint32_t* __restrict__ line_stats,
    uint32_t* c4_words, DictLines dict_lines) {
  const int doc = perm[blockIdx.x];
  if (doc >= ndocs || (dead && dead[doc])) return;
  DocCtx<BlockPar<kBlockThreads>> x =
      make_ctx<BlockPar<kBlockThreads>>(tabs, pw, pw_n, scratch, scratch_off, doc, (int)blockIdx.x, flags, lds_bytes, prof);
  x.par.xs = g_block_xs;
  lds_ascii_props(x);
  const uint8_t* b = bytes + off[doc];
  const uint32_t n = (uint32_t)(off[doc + 1] - off[doc]);
  c4_pass_a(x, *c4, b, n, rec + (int64_t)doc * 7, src + (int64_t)doc * 2,
            line_stats ? line_stats + line_stats_base(off[doc], doc) : nullptr, c4_words ? c4_words + doc : nullptr,
            dict_lines.at((uint32_t)doc));
  c4_src_absolute(x, src + (int64_t)doc * 2, scratch_off[blockIdx.x]);
}

}  // namespace

extern "C" {

size_t tb_sizeof_c4() { return sizeof(DevC4); }

int tb_c4_pass_a(hipStream_t stream, const void* c4, const TbDocs* d, const TbWork* w, const TbTables* tb,
                 int64_t* src, const uint32_t* line_stats, uint32_t* c4_words, const DictLines* dict) {
  const uint32_t lds_bytes = w->lds_bytes;
  if (d->ndocs <= 0) return 0;
  const int32_t nblocks = d->n_launch <= 0 ? d->ndocs : d->n_launch;
  if (lds_bytes > kMaxLdsPerDoc) return (int)hipErrorInvalidValue;
  if (lds_bytes > 65536)
    (void)hipFuncSetAttribute((const void*)k_c4_pass_a, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  hipLaunchKernelGGL(k_c4_pass_a, dim3(nblocks), dim3(64), lds_bytes, stream, (const DevC4*)c4, d->bytes, d->off,
                     d->perm, d->ndocs, w->scratch, w->scratch_off, tb->pw, tb->pw_n, tb->ucd, w->rec, src, w->flags,
                     lds_bytes, w->prof, d->dead, line_stats, c4_words, dict ? *dict : DictLines{});
  return (int)hipGetLastError();
}

int tb_c4_pass_a_blk(hipStream_t stream, const void* c4, const TbDocs* d, const TbWork* w, const TbTables* tb,
                     int64_t* src, const uint32_t* line_stats, uint32_t* c4_words, const DictLines* dict) {
  const int32_t nblocks = d->n_launch;
  const uint32_t lds_bytes = w->lds_bytes;
  if (nblocks <= 0) return 0;
  if (!d->perm || lds_bytes > kMaxLdsPerBlk) return (int)hipErrorInvalidValue;
  if (lds_bytes > 65536)
    (void)hipFuncSetAttribute((const void*)k_c4_pass_a_blk, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes);
  hipLaunchKernelGGL(k_c4_pass_a_blk, dim3(nblocks), dim3(kBlockThreads), lds_bytes, stream, (const DevC4*)c4,
                     d->bytes, d->off, d->perm, d->ndocs, w->scratch, w->scratch_off, tb->pw, tb->pw_n, tb->ucd, w->rec,
                     src, w->flags, lds_bytes, w->prof, d->dead, line_stats, c4_words, dict ? *dict : DictLines{});
  return (int)hipGetLastError();
}

}  // extern "C"

namespace {

__global__ __launch_bounds__(256) void k_c4_pass_b(const uint8_t* __restrict__ bytes, const int64_t* __restrict__ off,
                                                   int32_t ndocs, const char* __restrict__ scratch,
                                                   const int64_t* __restrict__ scratch_off,
                                                   const int64_t* __restrict__ src, const int64_t* __restrict__ new_off,
                                                   uint8_t* __restrict__ out) {
  const int doc = blockIdx.x;
  if (doc >= ndocs) return;
  const int64_t len = new_off[doc + 1] - new_off[doc];
  const int64_t s = src[2 * doc];
  (void)scratch_off;  // src holds absolute arena offsets (c4_src_absolute)
  const uint8_t* from = s < 0 ? bytes + off[doc] : (const uint8_t*)scratch + s;
  uint8_t* to = out + new_off[doc];
  for (int64_t i = threadIdx.x; i < len; i += blockDim.x) to[i] = from[i];
}

}  // namespace

extern "C" {

int tb_c4_pass_b(hipStream_t stream, const uint8_t* bytes, const int64_t* off, int32_t ndocs, const char* scratch,
                 const int64_t* scratch_off, const int64_t* src, const int64_t* new_off, uint8_t* out) {
  if (ndocs <= 0) return 0;
  hipLaunchKernelGGL(k_c4_pass_b, dim3(ndocs), dim3(256), 0, stream, bytes, off, ndocs, scratch, scratch_off, src,
                     new_off, out);
  return (int)hipGetLastError();
}

}  // extern "C"

namespace {

// C4 bad words (reference c4_filters.rs:431-441,463-551): does any list entry occur, case-folded,
// with \W (or text edge) on both sides (no boundary requirement for CJK lists)? One wave per
// document, four documents per workgroup; every code point position (UTF-8 lead byte) of a
// 64-byte chunk starts a walk of the hashed trie table (csrc/common/badwords.h) in parallel; the
// wave stops at the first chunk that contains a match. In the batch pipeline it reads the content
// version its step sees and skips the documents a pass before the step filtered
// (0 < dead <= dead_max); matched: -1 skipped / no list, 0 no match, 1 match.
constexpr int kBwWaves = 4;
// Work items: without a segment list, wave w takes document w and the start positions
// [0, seg_bytes) and writes its verdict; with one (seg_doc / seg_idx, launched afterwards on the
// same stream), wave w takes positions [seg_idx * seg_bytes, +seg_bytes) of document seg_doc[w] —
// the long documents' remaining segments, so no single wave walks a whole long document — skips
// documents already decided, and only ever writes a match.
__global__ __launch_bounds__(64 * kBwWaves) void k_badwords_match(
    const uint8_t* __restrict__ bytes, const int64_t* __restrict__ off, int32_t nitems,
    const int32_t* __restrict__ root, const uint8_t* __restrict__ cjk, int32_t root0, int32_t cjk0,
    const uint8_t* __restrict__ dead, uint32_t dead_max, BwTable tab, DevTables tabs, BwFold fold,
    int8_t* __restrict__ matched, const int32_t* __restrict__ seg_doc, const int32_t* __restrict__ seg_idx,
    uint32_t seg_bytes) {
  __shared__ uint8_t asc[128];
  const UcdView ucd{tabs.s1, tabs.s2, tabs.l1, tabs.l2};
  if (threadIdx.x < 128) asc[threadIdx.x] = bw_ascii_entry(ucd, fold, threadIdx.x);
  __syncthreads();
  const int item = (int)blockIdx.x * kBwWaves + (int)(threadIdx.x >> 6);
  if (item >= nitems) return;
  const int doc = seg_doc ? seg_doc[item] : item;
  const uint32_t lane = threadIdx.x & 63;
  const int32_t r0 = root ? root[doc] : root0;
  const uint32_t dd = dead ? dead[doc] : 0u;
  if (seg_doc) {
    if (matched[doc] != 0) return;  // decided (match, or skipped) by the first pass
  } else if (r0 < 0 || (dd != 0 && dd <= dead_max)) {
    if (lane == 0) matched[doc] = -1;
    return;
  }
  const uint8_t* b = bytes + off[doc];
  const uint32_t n = (uint32_t)(off[doc + 1] - off[doc]);
  const bool any_edge = (cjk ? cjk[doc] : (uint8_t)cjk0) != 0;
  const uint32_t p0 = seg_doc ? (uint32_t)seg_idx[item] * seg_bytes : 0u;
  const uint32_t p1 = p0 + seg_bytes < n ? p0 + seg_bytes : n;
  bool found = false;
  // 256 positions per iteration, 4 consecutive bytes per lane: the left-boundary test of a
  // position reads the previous byte from the lane's own bytes or its neighbour; only positions
  // that start a word walk the trie (the walk itself may run past the segment end)
  for (uint32_t base = p0; base < p1 && !found; base += 256) {
    const uint32_t s0 = base + 4 * lane;
    uint8_t c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = s0 + k < p1 ? b[s0 + k] : (uint8_t)0;
    const uint8_t before = s0 > 0 && s0 < p1 ? b[s0 - 1] : (uint8_t)' ';
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t s = s0 + k;
      if (s >= p1 || !utf8_is_lead(c[k])) continue;
      const uint8_t pb = k ? c[k - 1] : before;
      bool left = any_edge || s == 0 || (pb < 0x80 ? (asc[pb] & 0x80u) == 0 : bw_left_ok(b, n, s, ucd, asc));
      if (left && bw_walk_from(b, n, s, r0, any_edge, tab, ucd, fold, asc)) { found = true; break; }
    }
    found = __ballot(found) != 0;
  }
  if (lane == 0 && (found || !seg_doc)) matched[doc] = found ? 1 : 0;
}

}  // namespace

extern "C" {

struct TbBadWords {  // inputs of one C4BadWords step (tb_badwords_match)
  const int32_t* root;
  const uint8_t* cjk;
  const uint32_t* table;
  const uint16_t* f1;
  const int32_t *f2, *seg_doc, *seg_idx;
  int32_t root0, cjk0;
  uint32_t dead_max, table_mask, seg_bytes;
};
size_t tb_sizeof_badwords() { return sizeof(TbBadWords); }

// n_launch items: the documents [0, n_launch), or with seg_doc / seg_idx that many segments.
int tb_badwords_match(hipStream_t stream, const TbDocs* d, const TbTables* tb, const TbBadWords* b, int8_t* matched) {
  const int32_t nitems = d->n_launch;
  if (nitems <= 0) return 0;
  if (!b->table || ((b->table_mask + 1) & b->table_mask) != 0 || b->seg_bytes < 256 || (b->seg_bytes & 255) ||
      (!b->seg_doc != !b->seg_idx))
    return (int)hipErrorInvalidValue;
  const BwTable bt{b->table, b->table_mask};
  const BwFold fold{b->f1, b->f2};
  hipLaunchKernelGGL(k_badwords_match, dim3((nitems + kBwWaves - 1) / kBwWaves), dim3(64 * kBwWaves), 0, stream,
                     d->bytes, d->off, nitems, b->root, b->cjk, b->root0, b->cjk0, d->dead, b->dead_max, bt, tb->ucd,
                     fold, matched, b->seg_doc, b->seg_idx, b->seg_bytes);
  return (int)hipGetLastError();
}

}  // extern "C"
