// What the HIP kernel translation units of csrc/hip/ share. gfx950 (MI355X), C ABI, every launch
// on a caller-provided stream (the native HIP runtime layer's, csrc/hip/runtime.hip).
//
// Document kernels run one wavefront per document (block = 64 lanes = one wave64): the lanes
// cooperate through DPP shuffles and ballots (csrc/common/par.h WavePar), per-document working
// arrays live in a per-document slice of an HBM scratch arena (L2-resident while the wave
// works on it). Grid = number of documents, visited through a length-sorted permutation so the
// longest documents start first (tail-latency balance under the power-law length distribution).
// Long documents take one workgroup of kBlockThreads each instead (BlockPar).
//
// One translation unit per kernel family, each with its kernels, its TB_*_WPE register budgets
// and its extern "C" launchers right below the kernels they launch:
//
//  stage.hip     : tb_stage_analyze[_blk[_mid]]: decode + UAX#29 words + lines + hashes -> Gopher/FineWeb
//                  records; tb_gr_dup_split: the n-gram orders and duplicated lines of split
//                  long documents
//  gr_ngrams.hip : tb_gr_split_wave: the GopherRepetition n-gram fields of the one-wave documents:
//                  word ids, byte prefixes and concatenation hashes are built on chip from the word
//                  spans the stage kernel exports (k_gr_ngrams*, one workgroup per document)
//  langid.hip    : tb_langid_mfma: fastText int8 embedding bag + bf16 MFMA head (16 docs per tile)
//                  -> language records
//  c4.hip        : tb_c4_pass_a[_blk]: C4 line filtering, citation removal, rewritten text into
//                  scratch; tb_c4_pass_b: compaction of the rewritten texts into the next content
//                  version; tb_badwords_match
//  prepass.hip   : tb_pre_decode / tb_pre_wcanon: code points, word marks and word arrays of very
//                  long documents, spread over many workgroups; tb_pow_table
//  resolve.hip   : tb_gate, tb_resolve (+ compaction), tb_meta_format (the metadata column)
//
// Launch ABI: the argument groups every document kernel shares travel as `const T*` to plain
// structs -- TbTables (Unicode tables, hash powers: per batch), TbDocs (content version, launch
// positions, counts, dead marks: per launch), TbWork (scratch, records, flags, LDS slice: per
// launch), DictIn / DictLines (devplan.h) -- and the launchers unpack them into the kernels'
// argument lists. ops/kernels.py holds the one ctypes mirror of each.
//
// Only what more than one family uses lives here (of the document algorithms the context alone,
// doc_ctx.h: each unit includes the family headers of csrc/common/ it calls, docproc.h has their
// map); the kernels of every unit sit in that unit's anonymous namespace, and so do the
// device-side declarations below.
#pragma once
#include <hip/hip_runtime.h>

#include "../common/doc_ctx.h"

using namespace tb;

namespace {

constexpr uint32_t kMaxLdsPerDoc = 160 * 1024;
// Workgroup kernels also hold static LDS (g_block_xs) on top of the dynamic slice: a 160 KB
// slice fails at launch (HSA_STATUS_ERROR_INVALID_ALLOCATION, measured), so they take <= 128 KB.
constexpr uint32_t kMaxLdsPerBlk = 128 * 1024;

struct DevTables {
  const uint16_t* s1;
  const uint32_t* s2;
  const uint16_t* l1;
  const int32_t* l2;
};

// Dynamic LDS: each workgroup (= one wave = one document) gets `lds_bytes` of fast arena; the
// document's working arrays are carved from it first and spill to its HBM scratch slice.
extern __shared__ __attribute__((aligned(16))) char g_lds_arena[];

template <class P = WavePar>
__device__ __forceinline__ DocCtx<P> make_ctx(const DevTables& t, const uint64_t* pw, uint32_t pw_n,
                                             char* scratch, const int64_t* scratch_off, int doc, int k,
                                             uint32_t* flags, uint32_t lds_bytes, uint64_t* prof) {
  DocCtx<P> x;
  x.prof = prof ? prof + (size_t)doc * kPhaseSlots : nullptr;
  x.lds = lds_bytes ? (char*)g_lds_arena : nullptr;
  x.lcap = lds_bytes;
  x.lused = 0;
  x.ucd = UcdView{t.s1, t.s2, t.l1, t.l2};
  x.pw = pw;
  x.pw_n = pw_n;
  x.ipw = pw ? pw + pw_n + 1 : nullptr;
  // scratch slices are laid out in dispatch order (k = position in the launched permutation), so
  // the waves resident at the same time work in one contiguous window of the arena
  x.scr = scratch + scratch_off[k];
  x.cap = (uint64_t)(scratch_off[k + 1] - scratch_off[k]);
  x.used = 0;
  x.flag = flags + doc;
  return x;
}

// Per-wave LDS copies that turn the hottest global reads into LDS reads: the compact UCD properties
// of U+0000..U+00FF (every decode looks up ASCII and Latin-1 letters there instead of the two-level
// global table) and, for wave-path documents, the text
// itself (read by every pass: lead bytes, decoding, hashing, byte verification). The text copy
// moves whole dwords (the batch buffers are padded, so the up to 3 bytes read past a document's
// end stay inside the allocation).
template <class P>
__device__ __forceinline__ void lds_ascii_props(DocCtx<P>& x) {
  uint16_t* asc = x.template try_lds<uint16_t>(256);
  if (!asc) return;
  x.par.for_n(256, [&](uint32_t c) { asc[c] = compact_prop(x.ucd.props(c)); });
  x.par.sync();
  x.asc = asc;
}

template <class P>
__device__ __forceinline__ const uint8_t* lds_text(DocCtx<P>& x, const uint8_t* b, uint32_t n) {
  const uintptr_t a0 = (uintptr_t)b & ~(uintptr_t)3;
  const uint32_t head = (uint32_t)((uintptr_t)b - a0);
  const uint32_t nd = (head + n + 3) >> 2;
  uint32_t* d = x.template try_lds<uint32_t>(nd + 1);
  if (!d) return b;
  const uint32_t* src = (const uint32_t*)a0;
  x.par.for_n(nd, [&](uint32_t k) { d[k] = src[k]; });
  x.par.sync();
  return (const uint8_t*)d + head;
}

// Long documents: one workgroup of kBlockThreads (8 waves by default) per document (BlockPar), launched
// over the long prefix of the length-sorted permutation.
#ifndef TB_BLOCK_THREADS
#define TB_BLOCK_THREADS 512
#endif
constexpr int kBlockThreads = TB_BLOCK_THREADS;
// BlockPar's exchange area (x.par.xs): static LDS of the workgroup kernels that name it, and of no
// other kernel (sized for kBlockThreads; a kernel with fewer threads uses its first part)
__shared__ __attribute__((aligned(16))) char g_block_xs[16 * (kBlockThreads / 64) + 64];

}  // namespace

// CUs of the current device (queried once; thread-safe static initialisation). inline: the
// library keeps one cached value however many units ask; hidden: not part of its exported symbols.
__attribute__((visibility("hidden"))) inline int device_cus() {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) !=
        hipSuccess || n <= 0)
      n = 256;
    return n;
  }();
  return cus;
}

extern "C" {

int tb_scan_strided_i64(hipStream_t stream, const int64_t* src, int64_t stride, int64_t n, int64_t* out);  // runtime.hip

// Launch arguments travel in a few plain structs (mirrored field by field as ctypes.Structure in
// ops/kernels.py, sizes checked through tb_sizeof_*); each launcher unpacks the fields it needs
// into its kernel's argument list. DictIn / DictLines (devplan.h) are passed the same way.
struct TbTables {      // read-only tables of a batch
  DevTables ucd;       // Unicode property tables (s1, s2, l1, l2)
  const uint64_t* pw;  // B^0 .. B^pw_n, then B^-0 .. B^-pw_n (hashes)
  uint32_t pw_n;
};
struct TbDocs {          // the documents of one launch
  const uint8_t* bytes;  // a content version: text and offsets [ndocs + 1]
  const int64_t* off;
  const int32_t* perm;      // launch positions perm[0 .. n_launch)
  const uint8_t* dead;      // the batch's dead marks, or null
  int32_t n_launch, ndocs;  // ndocs: documents in the batch (the record stride)
};
struct TbWork {  // what a document kernel writes
  char* scratch;
  const int64_t* scratch_off;  // slices by launch position
  int64_t* rec;
  uint32_t* flags;
  uint64_t* prof;      // phase counters, or null
  uint32_t lds_bytes;  // dynamic LDS slice per workgroup
};

size_t tb_sizeof_tables();  // (defined in stage.hip)
size_t tb_sizeof_docs();
size_t tb_sizeof_work();

}  // extern "C"
