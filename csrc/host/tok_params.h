// The token counters' parameter blocks (csrc/common/bpe.h DevBpe, csrc/common/wordpiece.h DevWp,
// csrc/common/unigram.h DevUni): the one list of conditions a tokenizer spec must meet
// (bpe_spec_error / wp_spec_error / uni_spec_error) and the one place that writes the blocks' fields
// (bpe_fill_params / wp_fill_params / uni_fill_params), for both executions: with host addresses
// the block drives the host emulation (tok_module.cpp bpe_count / wp_count / uni_count,
// tools/*_selftest.cpp), with HBM addresses the kernels (tok_module.cpp bpe_params / wp_params /
// uni_params, uploaded by ops/kernels.py). No pybind here: the selftests include this file by relative path.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>

#include "../common/bpe_case.h"
#include "../common/bpe_sp.h"
#include "../common/unigram.h"
#include "../common/bpe_classes.inc"
#include "../common/bpe_case_classes.inc"
#include "../common/nfc_qc.inc"
#include "../common/wp_classes.inc"
#include "../common/wp_fold.inc"

namespace tb {

template <class T>
struct TokSpan {
  const T* p = nullptr;
  size_t n = 0;
};

// ---- the host-side view of a spec (models/tokenizer.py BpeSpec / WordPieceSpec) ----
struct BpeSpecView {
  TokSpan<uint32_t> byte_id;
  TokSpan<uint64_t> keys, vals;
  TokSpan<uint8_t> added;
  TokSpan<int32_t> added_off;
  TokSpan<uint64_t> vslots;
  TokSpan<uint8_t> vpool;
  TokSpan<uint32_t> sp_ascii;
  TokSpan<uint64_t> sp_cp;
  uint32_t mask = 0;
  int32_t post_add = 0;
  int32_t kind = kBpeGpt2;
  bool ignore_merges = false;
  uint32_t vmask = 0;
  int32_t vlongest = 0;
  bool nfc = false;
  uint32_t sp_mask = 0, sp_id = 0;
  int32_t sp_flags = 0;
};

struct WpSpecView {
  TokSpan<uint64_t> slots;  // WpSlot pairs
  TokSpan<uint8_t> pool, added;
  TokSpan<int32_t> added_off;
  uint32_t mask = 0, flags = 0, cls_shift = 0, self_bit = 0;
  int32_t max_chars = 0, longest = 0, post_add = 0;
  int32_t fold = 0;  // wp_fold.inc: 0 none, 1 lowercase, 2 strip_accents, 3 both
};

struct UniSpecView {
  TokSpan<uint64_t> slots;  // UniSlot triples
  TokSpan<uint8_t> pool, added, cls2, sp;
  TokSpan<uint16_t> cls1;
  TokSpan<int32_t> added_off;
  uint32_t mask = 0, flags = 0;
  int32_t longest_cp = 0, longest = 0, post_add = 0;
  double unk_score = 0;
  // the normalizer's replacements; all empty: a spec without a map
  TokSpan<uint16_t> map1, map2;
  TokSpan<uint32_t> map_rec;
  TokSpan<uint8_t> map_pool;
  bool mapped() const { return map1.n || map2.n || map_rec.n || map_pool.n; }
};

// ---- where the arrays a block points to are: in host memory, or in HBM ----
struct BpePtrs {
  const uint32_t* byte_id = nullptr;
  const uint64_t *keys = nullptr, *vals = nullptr;
  const uint8_t* added = nullptr;
  const int32_t* aoff = nullptr;  // the spec's added_off (the kinds that keep it in memory)
  const uint64_t* vslots = nullptr;
  const uint8_t* vpool = nullptr;
  const uint32_t* sp_ascii = nullptr;
  const uint64_t* sp_cp = nullptr;
  const uint16_t* cls1 = nullptr;  // bpe_classes.inc
  const uint32_t* cls2 = nullptr;
  const uint16_t* ccls1 = nullptr;  // bpe_case_classes.inc
  const uint32_t* ccls2 = nullptr;
  const uint8_t *nfc1 = nullptr, *nfc2 = nullptr;  // nfc_qc.inc
};

struct WpPtrs {
  const uint64_t* slots = nullptr;
  const uint8_t *pool = nullptr, *added = nullptr;
  const uint16_t* cls1 = nullptr;  // wp_classes.inc
  const uint8_t* cls2 = nullptr;
  const uint16_t* fold1 = nullptr;  // wp_fold.inc: stage 1 of all three modes, [3][TB_WP_FOLD_NSTAGE1]
  const uint16_t* fold2 = nullptr;
  const uint8_t* foldp = nullptr;
};

struct UniPtrs {
  const uint64_t* slots = nullptr;
  const uint8_t *pool = nullptr, *added = nullptr, *cls2 = nullptr;
  const uint16_t* cls1 = nullptr;
  const int32_t* aoff = nullptr;
  const uint16_t *map1 = nullptr, *map2 = nullptr;  // a spec with a map
  const uint32_t* map_rec = nullptr;
  const uint8_t* map_pool = nullptr;
};

// the static tables in host memory
inline BpePtrs bpe_host_tables() {
  BpePtrs p;
  p.cls1 = TB_BPE_CLS_STAGE1;
  p.cls2 = TB_BPE_CLS_STAGE2;
  p.ccls1 = TB_BPE_CASE_STAGE1;
  p.ccls2 = TB_BPE_CASE_STAGE2;
  p.nfc1 = TB_NFC_QC_STAGE1;
  p.nfc2 = TB_NFC_QC_STAGE2;
  return p;
}

// ... and a spec's own arrays where the view has them: what the host emulation counts with
inline BpePtrs bpe_host_ptrs(const BpeSpecView& v) {
  BpePtrs p = bpe_host_tables();
  p.byte_id = v.byte_id.p;
  p.keys = v.keys.p;
  p.vals = v.vals.p;
  p.added = v.added.p;
  p.aoff = v.added_off.p;
  p.vslots = v.vslots.p;
  p.vpool = v.vpool.p;
  p.sp_ascii = v.sp_ascii.p;
  p.sp_cp = v.sp_cp.p;
  return p;
}

inline WpPtrs wp_host_ptrs(const WpSpecView& v) {
  WpPtrs p;
  p.slots = v.slots.p;
  p.pool = v.pool.p;
  p.added = v.added.p;
  p.cls1 = TB_WP_CLS_STAGE1;
  p.cls2 = TB_WP_CLS_STAGE2;
  p.fold1 = TB_WP_FOLD_STAGE1;
  p.fold2 = TB_WP_FOLD_STAGE2;
  p.foldp = TB_WP_FOLD_POOL;
  return p;
}

inline UniPtrs uni_host_ptrs(const UniSpecView& v) {
  UniPtrs p;
  p.slots = v.slots.p;
  p.pool = v.pool.p;
  p.added = v.added.p;
  p.cls1 = v.cls1.p;
  p.cls2 = v.cls2.p;
  p.aoff = v.added_off.p;
  p.map1 = v.map1.p;
  p.map2 = v.map2.p;
  p.map_rec = v.map_rec.p;
  p.map_pool = v.map_pool.p;
  return p;
}

// ---- the conditions: nullptr, or what is wrong with the spec ----
inline const char* tok_added_error(const TokSpan<uint8_t>& added, const TokSpan<int32_t>& off, size_t max_added,
                                   size_t max_bytes) {
  if (off.n > max_added + 1) return "too many added tokens";
  if (off.n == 0) return nullptr;
  if (off.p[0] != 0) return "added_off does not start at 0";
  if (!std::is_sorted(off.p, off.p + off.n)) return "added_off is not sorted";
  if ((size_t)off.p[off.n - 1] > added.n) return "added_off ends past the added tokens' bytes";
  if ((size_t)off.p[off.n - 1] > max_bytes) return "the added tokens have too many bytes";
  return nullptr;
}

inline const char* bpe_spec_error(const BpeSpecView& v) {
  const bool sp = v.kind == kBpeSp, mem = bpe_kind_mem_added(v.kind);
  if (!mem && v.kind != kBpeGpt2) return "bpe: unknown kind";
  if (v.byte_id.n != 256) return "bpe: byte_id needs 256 entries";
  if (v.keys.n != (size_t)v.mask + 1) return "bpe: keys needs mask + 1 entries";
  if (v.vals.n != v.keys.n) return "bpe: vals needs as many entries as keys";
  if (const char* e = tok_added_error(v.added, v.added_off, mem ? kBpeSplitMaxAdded : kBpeMaxAdded,
                                      mem ? kBpeSplitMaxAddedBytes : v.added.n))
    return e;
  if (v.ignore_merges && (!mem || sp)) return "bpe: ignore_merges needs a split-regex kind";
  if (v.nfc && (!mem || sp)) return "bpe: the NFC gate needs a split-regex kind";
  if (v.ignore_merges) {
    if (v.vslots.n != 2 * ((size_t)v.vmask + 1) || v.vlongest < 1) return "bpe: vocabulary table shape";
    for (size_t i = 0; i <= v.vmask; ++i) {  // every listed entry lies in the pool
      const uint64_t e = v.vslots.p[2 * i + 1];
      if (e != kWpEmpty && (e >> 32) + (uint32_t)e > (uint64_t)v.vpool.n) return "bpe: a vocabulary entry lies past vpool";
    }
  }
  if (sp) {
    if (v.sp_ascii.n != 128) return "bpe: sp_ascii needs 128 entries";
    if (v.sp_cp.n != (size_t)v.sp_mask + 1) return "bpe: sp_cp needs sp_mask + 1 entries";
    if (!bpe_sp_flags_valid(v.sp_flags)) return "bpe: sp_flags";
    // a free slot ends every probe
    if (std::find(v.sp_cp.p, v.sp_cp.p + v.sp_cp.n, kBpeSpEmpty) == v.sp_cp.p + v.sp_cp.n)
      return "bpe: sp_cp has no free slot";
  }
  return nullptr;
}

inline const char* wp_spec_error(const WpSpecView& v) {
  static_assert(sizeof(WpSlot) == 16, "WpSlot is two uint64");
  if (v.slots.n != 2 * ((size_t)v.mask + 1) || v.longest < 1) return "wordpiece: vocabulary table shape";
  if (const char* e = tok_added_error(v.added, v.added_off, kBpeMaxAdded, v.added.n)) return e;
  if (v.cls_shift != 0 && v.cls_shift != 2) return "wordpiece: cls_shift is 0 or 2";
  if (v.max_chars < 0) return "wordpiece: max_chars";
  if (v.fold < 0 || v.fold > 3) return "wordpiece: fold is 0 to 3";
  return nullptr;
}

constexpr size_t kUniClsStage1 = 0x110000 >> 7;  // entries of UniSpecView::cls1

inline const char* uni_spec_error(const UniSpecView& v) {
  static_assert(sizeof(UniSlot) == 24, "UniSlot is three uint64");
  const size_t cap = (size_t)v.mask + 1;
  if ((cap & v.mask) != 0 || v.slots.n != 3 * cap) return "unigram: vocabulary table shape";
  if (v.longest_cp < 1 || v.longest_cp > kUniMaxPieceCp || v.longest < 1 || v.longest > kUniMaxPieceBytes)
    return "unigram: the longest piece exceeds the ring";
  size_t free_slots = 0;
  for (size_t i = 0; i < cap; ++i) {  // every listed piece lies in the pool and fits the longest
    const uint64_t e = v.slots.p[3 * i + 1];
    if (e == kWpEmpty) {
      ++free_slots;
      continue;
    }
    const uint64_t nb = (uint32_t)e & 0x7FFFFFFFu;
    if (nb < 1 || nb > (uint64_t)v.longest || (e >> 32) + nb > (uint64_t)v.pool.n) return "unigram: a piece lies past the pool";
  }
  if (free_slots == 0) return "unigram: the vocabulary table has no free slot";
  if (v.cls1.n != kUniClsStage1) return "unigram: cls1 needs one entry per 128 code points";
  for (size_t i = 0; i < v.cls1.n; ++i)
    if (((size_t)v.cls1.p[i] + 1) * 32 > v.cls2.n) return "unigram: a class block lies past cls2";
  if (const char* e = tok_added_error(v.added, v.added_off, kBpeSplitMaxAdded, kBpeSplitMaxAddedBytes)) return e;
  if (v.sp.n < 1 || v.sp.n > 4) return "unigram: the replacement character has 1 to 4 bytes";
  if (v.flags & ~kUniByteFallback) return "unigram: flags";
  if (!std::isfinite(v.unk_score)) return "unigram: unk_score";
  if (!v.mapped()) return nullptr;
  if (v.map1.n != kUniClsStage1) return "unigram: map1 needs one entry per 128 code points";
  if (v.map_rec.n == 0 || v.map_pool.n == 0) return "unigram: a map needs records and a pool";
  for (size_t i = 0; i < v.map1.n; ++i)
    if (((size_t)v.map1.p[i] + 1) * 128 > v.map2.n) return "unigram: a map block lies past map2";
  for (size_t i = 0; i < v.map2.n; ++i)
    if (v.map2.p[i] != kUniMapNone && v.map2.p[i] >= v.map_rec.n) return "unigram: map2 names a record past map_rec";
  for (size_t i = 0; i < v.map_rec.n; ++i) {
    const size_t nb = v.map_rec.p[i] & kUniRecLen;
    if (nb > (size_t)kUniMaxMapBytes) return "unigram: a replacement exceeds the cap";
    if ((size_t)(v.map_rec.p[i] >> 8) + nb > v.map_pool.n) return "unigram: a replacement lies past map_pool";
  }
  for (uint32_t c = 0; c < 0x110000; ++c) {  // the counter looks every map code point's record up
    const int k = (v.cls2.p[(size_t)v.cls1.p[c >> 7] * 32 + ((c & 127) >> 2)] >> (2 * (c & 3))) & 3;
    const uint16_t r = v.map2.p[(size_t)v.map1.p[c >> 7] * 128 + (c & 127)];
    if (k == UNI_MAP && (r == kUniMapNone || (v.map_rec.p[r] & kUniRecJoin))) return "unigram: a map code point has no record";
    if (k != UNI_MAP && r != kUniMapNone && !(k == UNI_SPACE && (v.map_rec.p[r] & kUniRecJoin)))
      return "unigram: a record of a code point that is not of the map class";
  }
  return nullptr;
}

// ---- the blocks: the only code that writes their fields ----
inline DevBpe bpe_fill_params(const BpeSpecView& v, const BpePtrs& p) {
  if (const char* e = bpe_spec_error(v)) throw std::invalid_argument(e);
  DevBpe T{};
  T.byte_id = p.byte_id;
  T.keys = p.keys;
  T.vals = p.vals;
  T.cls1 = p.cls1;
  T.cls2 = p.cls2;
  T.added = p.added;
  T.mask = v.mask;
  T.n_added = v.added_off.n ? (int32_t)v.added_off.n - 1 : 0;
  T.post_add = v.post_add;
  T.kind = v.kind;
  if (bpe_kind_mem_added(v.kind)) {  // offsets in memory behind the first-byte mask
    T.aoff = p.aoff;
    bpe_added_mask(v.added.p, v.added_off.p, T.n_added, T.amask);
  } else {
    std::copy(v.added_off.p, v.added_off.p + v.added_off.n, T.added_off);
  }
  T.vslots = p.vslots;
  T.vpool = p.vpool;
  T.vmask = v.vmask;
  T.vlongest = v.vlongest;
  T.ignore_merges = v.ignore_merges;
  T.ccls1 = p.ccls1;
  T.ccls2 = p.ccls2;
  T.nfc1 = p.nfc1;
  T.nfc2 = p.nfc2;
  T.nfc = v.nfc;
  T.sp_ascii = p.sp_ascii;
  T.sp_cp = p.sp_cp;
  T.sp_mask = v.sp_mask;
  T.sp_id = v.sp_id;
  T.sp_flags = v.sp_flags;
  if (!bpe_params_ok(T)) throw std::invalid_argument("bpe: a table the tokenizer's kind reads has no address");
  return T;
}

inline DevWp wp_fill_params(const WpSpecView& v, const WpPtrs& p) {
  if (const char* e = wp_spec_error(v)) throw std::invalid_argument(e);
  DevWp T{};
  T.slots = reinterpret_cast<const WpSlot*>(p.slots);
  T.pool = p.pool;
  T.cls1 = p.cls1;
  T.cls2 = p.cls2;
  T.added = p.added;
  if (v.fold) {  // the stage 1 of the tokenizer's mode; the launcher then runs k_wp_count_fold
    if (p.fold1 == nullptr) throw std::invalid_argument("wordpiece: the fold tables have no address");
    T.fold1 = p.fold1 + (size_t)(v.fold - 1) * TB_WP_FOLD_NSTAGE1;
    T.fold2 = p.fold2;
    T.foldp = p.foldp;
  }
  uint64_t asc[4];
  wp_ascii_classes(TB_WP_CLS_STAGE1, TB_WP_CLS_STAGE2, v.cls_shift, asc);
  T.asc0 = asc[0]; T.asc1 = asc[1]; T.asc2 = asc[2]; T.asc3 = asc[3];
  T.mask = v.mask;
  T.flags = v.flags;
  T.cls_shift = v.cls_shift;
  T.self_bit = v.self_bit;
  T.max_chars = v.max_chars;
  T.longest = v.longest;
  T.post_add = v.post_add;
  T.n_added = v.added_off.n ? (int32_t)v.added_off.n - 1 : 0;
  std::copy(v.added_off.p, v.added_off.p + v.added_off.n, T.added_off);
  if (!wp_params_ok(T)) throw std::invalid_argument("wordpiece: a table the tokenizer's mode reads has no address");
  return T;
}

inline DevUni uni_fill_params(const UniSpecView& v, const UniPtrs& p) {
  if (const char* e = uni_spec_error(v)) throw std::invalid_argument(e);
  DevUni T{};
  T.slots = reinterpret_cast<const UniSlot*>(p.slots);
  T.pool = p.pool;
  T.cls1 = p.cls1;
  T.cls2 = p.cls2;
  T.added = p.added;
  T.aoff = p.aoff;
  uint64_t asc[4] = {0, 0, 0, 0};  // the ASCII classes, from the view's table (host memory)
  for (uint32_t c = 0; c < 128; ++c)
    asc[c >> 5] |= (uint64_t)((v.cls2.p[(size_t)v.cls1.p[0] * 32 + (c >> 2)] >> (2 * (c & 3))) & 3) << (2 * (c & 31));
  T.asc0 = asc[0]; T.asc1 = asc[1]; T.asc2 = asc[2]; T.asc3 = asc[3];
  T.n_added = v.added_off.n ? (int32_t)v.added_off.n - 1 : 0;
  bpe_added_mask(v.added.p, v.added_off.p, T.n_added, T.amask);
  T.unk_score = v.unk_score;
  T.mask = v.mask;
  T.flags = v.flags;
  for (size_t j = 0; j < v.sp.n; ++j) T.sp_bytes |= (uint32_t)v.sp.p[j] << (8 * j);
  T.sp_len = (int32_t)v.sp.n;
  T.longest_cp = v.longest_cp;
  T.longest = v.longest;
  T.post_add = v.post_add;
  if (v.mapped()) {
    T.map1 = p.map1;
    T.map2 = p.map2;
    T.mrec = p.map_rec;
    T.mpool = p.map_pool;
    if (!uni_has_map(T) || T.map2 == nullptr || T.mrec == nullptr || T.mpool == nullptr)
      throw std::invalid_argument("unigram: a table of the map has no address");
  }
  if (!uni_params_ok(T)) throw std::invalid_argument("unigram: a table the counter reads has no address");
  return T;
}

// ---- the merge table ----
// DevBpe::keys / vals over the merges (a[i], b[i]) -> (rank[i], nid[i]): open addressing over
// mask + 1 >= 2 n slots; a pair listed twice keeps its last rank (HashMap collect). False when a
// pair is the reserved key kBpeEmpty.
inline bool bpe_fill_pairs(const uint32_t* a, const uint32_t* b, const uint32_t* rank, const uint32_t* nid, size_t n,
                           uint64_t* keys, uint64_t* vals, uint64_t mask) {
  std::fill(keys, keys + mask + 1, kBpeEmpty);
  std::fill(vals, vals + mask + 1, ~0ull);
  for (size_t i = 0; i < n; ++i) {
    const uint64_t key = ((uint64_t)a[i] << 32) | b[i];
    if (key == kBpeEmpty) return false;
    uint64_t h = bpe_hash(key) & mask;
    while (keys[h] != kBpeEmpty && keys[h] != key) h = (h + 1) & mask;
    keys[h] = key;
    vals[h] = ((uint64_t)rank[i] << 32) | nid[i];
  }
  return true;
}

// slots of an open-addressed table of n entries at load <= 1/2 (a power of two, 16 at least)
inline size_t tok_table_cap(size_t n) {
  size_t cap = 16;
  while (cap < 2 * n) cap <<= 1;
  return cap;
}

}  // namespace tb
