// Stage analysis kernels (decode + UAX#29 words + lines + hashes -> Gopher / FineWeb records): one
// wave per document, one workgroup per long document, and the split long documents' n-gram and
// duplicated-line tasks. Also the ABI version and the sizes of the shared launch structs.
// (kernel_common.h: the families, the launch ABI.)
#include <algorithm>

#include "kernel_common.h"

#include "../common/stage_analyze.h"

namespace {

// The stage kernel is register-bound (occupancy = waves/SIMD the VGPR budget allows). With the
// n-gram orders and their word arrays moved to the k_gr_ngrams kernels it is built for 8 waves/SIMD (64 VGPRs,
// the spills it adds sit outside the per-chunk loops) with a 5 KB LDS slice per wave: 4.55 vs
// 5.05 ms per launch at 6 waves / 6.5 KB, 7 waves no gain (profiles/r8_wpe/; 6 beat 4 and 5 before,
// profiles/r7_ngram/ab_occupancy.txt; before the move 4 waves won, round 2).
#define TB_STAGE_KERNEL(NAME, ATTR, EXPORT)                                                           \
  __global__ __launch_bounds__(64) ATTR void NAME(                                                   \
      const DevPlan* __restrict__ plan, const DevStage* __restrict__ stage, const uint8_t* __restrict__ bytes, \
      const int64_t* __restrict__ off, const int32_t* __restrict__ perm, int32_t ndocs, char* scratch,        \
      const int64_t* __restrict__ scratch_off, const uint64_t* __restrict__ pw, uint32_t pw_n, DevTables tabs, \
      int64_t* rec, uint32_t* flags, uint32_t lds_bytes, uint64_t* prof,                               \
      const uint8_t* __restrict__ dead, uint32_t* line_stats, GrExport* gr_export, DictIn dict) {      \
    const int doc = perm ? perm[blockIdx.x] : (int)blockIdx.x;                                        \
    if (doc >= ndocs || (dead && dead[doc])) return;                                                  \
    DocCtx<WavePar> x = make_ctx(tabs, pw, pw_n, scratch, scratch_off, doc, (int)blockIdx.x, flags, lds_bytes, prof);   \
    const uint32_t n = (uint32_t)(off[doc + 1] - off[doc]);                                           \
    lds_ascii_props(x);                                                                               \
    const uint8_t* b = lds_text(x, bytes + off[doc], n);                                              \
    StageOut out{rec, (uint32_t)ndocs, (uint32_t)doc};                                                \
    if (line_stats) out.line_stats = line_stats + line_stats_base(off[doc], doc);                     \
    if (gr_export) { out.gr_export = gr_export + blockIdx.x; out.b_global = bytes + off[doc]; }       \
    out.dict = dict;                                                                                  \
    /* (language id: its own kernel) */                                                               \
    analyze_stage<WavePar, false, false, EXPORT>(x, *stage, *plan, LidTables{}, b, n, out);           \
  }

#ifndef TB_STAGE_WPE
#define TB_STAGE_WPE 8
#endif
TB_STAGE_KERNEL(k_stage_analyze_wave, __attribute__((amdgpu_waves_per_eu(TB_STAGE_WPE, 8))), false)
// launches with an export (split mode: tb_stage_analyze with gr_export): the n-gram kernels take
// the words, so the in-stage n-gram code and the prefix hash are compiled out of this build
TB_STAGE_KERNEL(k_stage_analyze_wave_ex, __attribute__((amdgpu_waves_per_eu(TB_STAGE_WPE, 8))), true)

// Register budget of the long-document stage kernel: 6 waves per SIMD (<= 80 VGPRs), so with the
// default 48 KB LDS slice three 512-thread workgroups (three documents) share a CU instead of one
// (174 VGPRs unconstrained). The kernel is latency-bound; config 5 (4096 x 50 KB documents,
// profiles/r2_c5/blk_variants.txt): 70.9K docs/s unconstrained/64 KB, 110.0K at 4 waves/64 KB,
// 113.7K at 6 waves/48 KB. TB_BLK_WPE=k builds another budget (0: none) for A/B runs.
// Re-measured with the round-5 kernels (profiles/r8_blk4): 4 waves (128 VGPRs, 93 spilled
// instead of 229) at 64 KB gives 139.9K vs 150.4K at 6 waves -- the spills stay cheaper than
// the lost occupancy.
#ifndef TB_BLK_WPE
#define TB_BLK_WPE 6
#endif
#if TB_BLK_WPE > 0
#define TB_BLK_ATTR __attribute__((amdgpu_waves_per_eu(TB_BLK_WPE, 8)))
#else
#define TB_BLK_ATTR
#endif

template <int NT, bool kPre = false>
__device__ __forceinline__ void stage_blk_body(
    const DevPlan* __restrict__ plan, const DevStage* __restrict__ stage, const uint8_t* __restrict__ bytes,
    const int64_t* __restrict__ off, const int32_t* __restrict__ perm, int32_t ndocs, char* scratch,
    const int64_t* __restrict__ scratch_off, const uint64_t* __restrict__ pw, uint32_t pw_n, DevTables tabs,
    int64_t* rec, uint32_t* flags, uint32_t lds_bytes, uint64_t* prof, const uint8_t* __restrict__ dead,
    GrExport* gr_export, int32_t n_split, uint32_t split_bytes, uint32_t* line_stats, const PreDoc* pre,
    int32_t n_pre, DictIn dict) {
  const int doc = perm[blockIdx.x];
  if (doc >= ndocs || (dead && dead[doc])) return;
  DocCtx<BlockPar<NT>> x =
      make_ctx<BlockPar<NT>>(tabs, pw, pw_n, scratch, scratch_off, doc, (int)blockIdx.x, flags, lds_bytes, prof);
  static_assert(16 * (NT / 64) + 64 <= (int)sizeof(g_block_xs), "BlockPar<NT>'s exchange area fits g_block_xs");
  x.par.xs = g_block_xs;
  lds_ascii_props(x);
  const uint8_t* b = bytes + off[doc];
  const uint32_t n = (uint32_t)(off[doc + 1] - off[doc]);
  StageOut out{rec, (uint32_t)ndocs, (uint32_t)doc};
  out.dict = dict;
  if (line_stats) out.line_stats = line_stats + line_stats_base(off[doc], doc);
  if constexpr (kPre) {
    if (pre[blockIdx.x].n != n) return;  // (never: the host builds the descriptors from these lengths)
    out.pre = pre + blockIdx.x;
  }
  // split documents (the first n_split launch positions, longer than split_bytes) export their
  // word arrays; k_gr_dup_split finishes their duplicated n-gram orders
  if (gr_export && (int)blockIdx.x < n_split && n > split_bytes) out.gr_export = gr_export + blockIdx.x;
  analyze_stage<BlockPar<NT>, false, kPre>(x, *stage, *plan, LidTables{}, b, n, out);
}

#define TB_STAGE_BLK_KERNEL(NAME, NT, PRE, ATTR)                                                       \
  __global__ __launch_bounds__(NT) ATTR void NAME(                                                   \
      const DevPlan* __restrict__ plan, const DevStage* __restrict__ stage, const uint8_t* __restrict__ bytes, \
      const int64_t* __restrict__ off, const int32_t* __restrict__ perm, int32_t ndocs, char* scratch,         \
      const int64_t* __restrict__ scratch_off, const uint64_t* __restrict__ pw, uint32_t pw_n, DevTables tabs,  \
      int64_t* rec, uint32_t* flags, uint32_t lds_bytes, uint64_t* prof, const uint8_t* __restrict__ dead,   \
      GrExport* gr_export, int32_t n_split, uint32_t split_bytes, uint32_t* line_stats,                \
      const PreDoc* pre, int32_t n_pre, DictIn dict) {                                                 \
    stage_blk_body<NT, PRE>(plan, stage, bytes, off, perm, ndocs, scratch, scratch_off, pw, pw_n, tabs, rec, flags, \
                       lds_bytes, prof, dead, gr_export, n_split, split_bytes, line_stats, pre, n_pre, dict); \
  }
TB_STAGE_BLK_KERNEL(k_stage_analyze_blk, kBlockThreads, false, TB_BLK_ATTR)
// documents with a pre-pass (tb_stage_analyze_blk with `pre`): every launch position has one
TB_STAGE_BLK_KERNEL(k_stage_analyze_blk_pre, kBlockThreads, true, TB_BLK_ATTR)

// Mid-sized workgroup documents (tb_stage_analyze_blk_mid; the caller picks them by length): the
// same body with kBlockMidThreads threads and a register budget of its own. At 4-32 KB the kernel
// is bound by the latency of one document's chain of passes, not by its spills or its thread
// count: with three documents per CU (48 KB slices) 256 threads take as long per document as 512
// (spill-free at 3 waves/SIMD, 168 VGPRs: 2.82 against 2.75 ms per step for both stages). What
// pays is more documents per CU, which four waves per document allow: five 31 KB slices at
// 5 waves/SIMD (96 VGPRs, 134 spilled) 2.47 ms; four at 4 waves 2.52, six at 6 waves 2.60, eight
// at 8 waves 3.16 (profiles/blk_mid/). TB_BLK_MID_WPE=k builds another budget (0: none) for A/B
// runs; the LDS slice is the caller's (pipeline/device.py MID_LDS_BYTES).
#ifndef TB_BLK_MID_WPE
#define TB_BLK_MID_WPE 5
#endif
#if TB_BLK_MID_WPE > 0
#define TB_BLK_MID_ATTR __attribute__((amdgpu_waves_per_eu(TB_BLK_MID_WPE, 8)))
#else
#define TB_BLK_MID_ATTR
#endif
constexpr int kBlockMidThreads = 256;
TB_STAGE_BLK_KERNEL(k_stage_analyze_blk_mid, kBlockMidThreads, false, TB_BLK_MID_ATTR)

}  // namespace

extern "C" {

int tb_abi_version() { return 27; }
size_t tb_sizeof_tables() { return sizeof(TbTables); }
size_t tb_sizeof_docs() { return sizeof(TbDocs); }
size_t tb_sizeof_work() { return sizeof(TbWork); }
size_t tb_sizeof_dict_in() { return sizeof(DictIn); }
size_t tb_sizeof_dict_lines() { return sizeof(DictLines); }
size_t tb_sizeof_plan() { return sizeof(DevPlan); }
size_t tb_sizeof_stage() { return sizeof(DevStage); }
int tb_block_threads() { return kBlockThreads; }
int tb_phase_slots() { return kPhaseSlots; }
int tb_stage_waves() { return TB_STAGE_WPE; }  // waves per SIMD the wave stage kernel is built for

// Wave kernels: grid = launch positions perm[0 .. n_launch) (n_launch <= 0: all ndocs).
int tb_stage_analyze(hipStream_t stream, const void* plan, const void* stage, const TbDocs* d, const TbWork* w,
                     const TbTables* tb, uint32_t* line_stats, void* gr_export, const DictIn* dict) {
  const uint32_t lds_bytes = w->lds_bytes;
  if (d->ndocs <= 0) return 0;
  const int32_t nblocks = d->n_launch <= 0 ? d->ndocs : d->n_launch;
  if (lds_bytes > kMaxLdsPerDoc) return (int)hipErrorInvalidValue;
  auto kern = gr_export ? k_stage_analyze_wave_ex : k_stage_analyze_wave;
  if (lds_bytes > 65536)
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64), lds_bytes, stream, (const DevPlan*)plan,
                     (const DevStage*)stage, d->bytes, d->off, d->perm, d->ndocs, w->scratch, w->scratch_off, tb->pw,
                     tb->pw_n, tb->ucd, w->rec, w->flags, lds_bytes, w->prof, d->dead, line_stats, (GrExport*)gr_export,
                     dict ? *dict : DictIn{});
  return (int)hipGetLastError();
}

// Long-document variants: `perm` must point at the long prefix of the length-sorted
// permutation, `n_launch` documents, one workgroup each. `pre`: the pre-pass descriptors of
// every launched document (k_stage_analyze_blk_pre), or null.
int tb_stage_analyze_blk(hipStream_t stream, const void* plan, const void* stage, const TbDocs* d, const TbWork* w,
                         const TbTables* tb, void* gr_export, int32_t n_split, uint32_t split_bytes,
                         uint32_t* line_stats, const void* pre, const DictIn* dict) {
  const int32_t nblocks = d->n_launch;
  const uint32_t lds_bytes = w->lds_bytes;
  if (nblocks <= 0) return 0;
  if (!d->perm || lds_bytes > kMaxLdsPerBlk || n_split < 0 || n_split > nblocks) return (int)hipErrorInvalidValue;
  auto kern = pre ? k_stage_analyze_blk_pre : k_stage_analyze_blk;
  if (lds_bytes > 65536)
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  hipLaunchKernelGGL(kern, dim3(nblocks), dim3(kBlockThreads), lds_bytes, stream, (const DevPlan*)plan,
                     (const DevStage*)stage, d->bytes, d->off, d->perm, d->ndocs, w->scratch, w->scratch_off, tb->pw,
                     tb->pw_n, tb->ucd, w->rec, w->flags, lds_bytes, w->prof, d->dead, (GrExport*)gr_export, n_split,
                     split_bytes, line_stats, (const PreDoc*)pre, pre ? nblocks : 0, dict ? *dict : DictIn{});
  return (int)hipGetLastError();
}

// The same launch with kBlockMidThreads threads per document (k_stage_analyze_blk_mid), for the
// shorter workgroup documents. It has no pre-pass build; split documents may take it like the
// other one.
int tb_stage_analyze_blk_mid(hipStream_t stream, const void* plan, const void* stage, const TbDocs* d,
                             const TbWork* w, const TbTables* tb, void* gr_export, int32_t n_split,
                             uint32_t split_bytes, uint32_t* line_stats, const DictIn* dict) {
  const int32_t nblocks = d->n_launch;
  const uint32_t lds_bytes = w->lds_bytes;
  if (nblocks <= 0) return 0;
  if (!d->perm || lds_bytes > kMaxLdsPerBlk || n_split < 0 || n_split > nblocks) return (int)hipErrorInvalidValue;
  if (lds_bytes > 65536)
    (void)hipFuncSetAttribute((const void*)k_stage_analyze_blk_mid, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes);
  hipLaunchKernelGGL(k_stage_analyze_blk_mid, dim3(nblocks), dim3(kBlockMidThreads), lds_bytes, stream,
                     (const DevPlan*)plan, (const DevStage*)stage, d->bytes, d->off, d->perm, d->ndocs, w->scratch,
                     w->scratch_off, tb->pw, tb->pw_n, tb->ucd, w->rec, w->flags, lds_bytes, w->prof, d->dead,
                     (GrExport*)gr_export, n_split, split_bytes, line_stats, (const PreDoc*)nullptr, 0,
                     dict ? *dict : DictIn{});
  return (int)hipGetLastError();
}

}  // extern "C"

namespace {

// SURVEY 5.7 intra-document split: one workgroup per (split document, task): n_tasks = the
// GopherRepetition step's duplicated n-gram orders, its top orders, then duplicated lines and
// duplicated paragraphs. Block k handles launch
// position k / n_tasks (perm order, the stage kernel's export slot) and task k % n_tasks; each
// task works in its own 1/n_tasks share of the document's unused scratch slice.
// Persistent (SURVEY 5.7 work queue): the grid is what the CUs hold at once; every workgroup
// takes the next (document, task) from an atomic cursor until the queue is empty, in launch order
// (documents longest first, their tasks together), so the heaviest tasks start first and a
// workgroup that finishes early takes more. Every workgroup exits once the cursor passes the end.
__global__ __launch_bounds__(kBlockThreads) TB_BLK_ATTR void k_gr_dup_split(
    const DevStage* __restrict__ stage, int32_t gr_step, const int32_t* __restrict__ perm, int32_t n_split,
    int32_t n_tasks, int32_t ndocs, const GrExport* __restrict__ ex, const uint64_t* __restrict__ pw, uint32_t pw_n,
    DevTables tabs, int64_t* rec, uint32_t* flags, uint32_t lds_bytes, uint32_t* cursor) {
  __shared__ int s_task;
  const int total = n_split * n_tasks;
  const DevStep& ds = stage->steps[gr_step];
  while (true) {
    if (threadIdx.x == 0) s_task = (int)atomicAdd(cursor, 1u);
    __syncthreads();
    const int task = s_task;
    __syncthreads();  // (s_task is rewritten by the next iteration's claim)
    if (task >= total) break;
    const int k = task / n_tasks, t = task % n_tasks;
    const int doc = perm[k];
    if (doc >= ndocs) continue;
    const GrExport e = ex[k];
    if (!e.valid) continue;  // not exported: skipped, returned early (flagged for the CPU path) or short
    DocCtx<BlockPar<kBlockThreads>> x;
    x.prof = nullptr;
    x.lds = lds_bytes ? (char*)g_lds_arena : nullptr;
    x.lcap = lds_bytes;
    x.lused = 0;
    x.ucd = UcdView{tabs.s1, tabs.s2, tabs.l1, tabs.l2};
    x.pw = pw;
    x.pw_n = pw_n;
    x.ipw = pw ? pw + pw_n + 1 : nullptr;
    const uint64_t region = (e.free_cap / (uint64_t)n_tasks) & ~255ull;
    x.scr = e.free_base + (uint64_t)t * region;
    x.cap = region;
    x.used = 0;
    x.flag = flags + doc;
    x.par.xs = g_block_xs;
    int64_t* r = rec + (int64_t)ds.rec_prefix * ndocs + (int64_t)doc * ds.width;
    if (t < ds.n_dup) gr_dup_one_order(x, ds, t, e, r);
    else if (t < ds.n_dup + ds.n_top) gr_top_one_order(x, ds, t - ds.n_dup, e, r);
    else if (t < ds.n_dup + ds.n_top + 2) gr_lines_split(x, t - ds.n_dup - ds.n_top, e, r);
    if (x.overflow) x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW);
    __syncthreads();  // the task's LDS is the next task's
  }
}

}  // namespace

extern "C" {

// gr_export: n_split descriptors written by tb_stage_analyze_blk (zeroed by the caller first);
// gr_step: index of the GopherRepetition step in the stage, n_tasks its duplicated + top n-gram
// orders.
int tb_gr_dup_split(hipStream_t stream, const void* stage, int32_t gr_step, const TbDocs* d, int32_t n_tasks,
                    const void* gr_export, const TbWork* w, const TbTables* tb, uint32_t* cursor) {
  const int32_t n_split = d->n_launch;
  const uint32_t lds_bytes = w->lds_bytes;
  if (n_split <= 0 || n_tasks <= 0) return 0;
  if (!d->perm || !gr_export || gr_step < 0 || gr_step >= kMaxStageSteps || n_tasks > 2 * kMaxNgramEntries + 2 ||
      lds_bytes > kMaxLdsPerBlk)
    return (int)hipErrorInvalidValue;
  if (!cursor) return (int)hipErrorInvalidValue;
  if (lds_bytes > 65536)
    (void)hipFuncSetAttribute((const void*)k_gr_dup_split, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  // the persistent grid: resident workgroups per CU (registers, LDS) x CUs, at most one per task
  const int cus = device_cus();
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_gr_dup_split, kBlockThreads, lds_bytes) !=
          hipSuccess || per_cu <= 0)
    per_cu = 1;
  const int64_t total = (int64_t)n_split * n_tasks;
  // persistent: one resident wave of workgroups pulls tasks from the cursor (one workgroup per
  // task, ordered by the hardware dispatcher instead, measured slower: profiles/r8_c5/)
  const int grid = (int)std::min<int64_t>(total, (int64_t)cus * per_cu);
  (void)hipMemsetAsync(cursor, 0, sizeof(uint32_t), stream);
  hipLaunchKernelGGL(k_gr_dup_split, dim3((uint32_t)grid), dim3(kBlockThreads), lds_bytes, stream,
                     (const DevStage*)stage, gr_step, d->perm, n_split, n_tasks, d->ndocs, (const GrExport*)gr_export,
                     tb->pw, tb->pw_n, tb->ucd, w->rec, w->flags, lds_bytes, cursor);
  return (int)hipGetLastError();
}

}  // extern "C"
