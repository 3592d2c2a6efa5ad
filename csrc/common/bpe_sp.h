// Character-level BPE token counting for the SentencePiece-converted tokenizers (Llama-2, Mistral
// v0.1-0.3, TinyLlama, Phi-3, Gemma): the policy BpeSp of the counting loops of bpe.h.
// Shared by the HIP kernels (csrc/hip/bpe.hip k_bpe_sp_count / k_bpe_sp_long) and the host
// emulation (csrc/host/tok_module.cpp bpe_count), which CPU tests pin to the `tokenizers` library.
//
// These files have no ByteLevel alphabet. The space is written U+2581, the model's symbols are code
// points, and a code point that is no vocabulary entry becomes one <0xNN> token per UTF-8 byte
// (byte_fallback). Two layouts:
//   L  normalizer Replace(" ", U+2581), with or without Prepend(U+2581) in front of it, and no
//      pre-tokenizer: the library merges the whole document as one word;
//   M  no normalizer, pre-tokenizer Metaspace(U+2581, prepend_scheme, split).
// The device does not normalise: it reads the raw text and treats U+0020 and U+2581 alike ("sp").
//
// Chunks. With Metaspace(split=true) a pre-token starts at every sp (and at offset 0). Without a
// split (L, and M with split=false) the document is one word, but the spec is only built when no
// merge (x, y) has x ending in a code point other than U+2581 and y starting with U+2581: then no
// merge ever joins across a position where sp follows a code point that is not sp, and the merges
// of the whole text are the merges of each chunk sp* [^sp]* on its own. So the pre-tokens of the
// counting loops are: kBpeSpSplit set, sp? [^sp]*; else sp* [^sp]*. Either start is decided by one
// code point and its predecessor, so a lane finds its first start locally (as BpeGpt2 does).
//
// Prepend. Layout L's Prepend puts one U+2581 in front of every text that is not empty; Metaspace
// (always / first) does so unless the text starts with sp. The chunk at offset 0 then begins with
// a symbol that has no byte (lead): it counts towards the limits of the merge arrays (kBpeMaxWord,
// kBpeMaxLong), which are one byte lower for that chunk.
//
// Symbols. A code point that is a vocabulary entry is one symbol: ASCII through a direct array,
// the others through a small open-addressed table; sp is the id of U+2581. Every other code point
// is one symbol per byte, the ids of <0xNN>. Symbols never outnumber bytes + lead.
#pragma once
#include "bpe_split.h"

namespace tb {

constexpr uint32_t kBpeSpNone = 0xFFFFFFFFu;   // sp_ascii: the code point is no vocabulary entry
constexpr uint64_t kBpeSpEmpty = ~0ull;        // sp_cp: free slot
constexpr uint32_t kBpeSpSpace = 0x2581;
// (BpeSpFlags and bpe_sp_flags_valid: bpe.h, next to the block they are a field of)

TB_HD bool bpe_sp_is_space(int32_t c) { return c == ' ' || c == (int32_t)kBpeSpSpace; }

// vocabulary id of the code point c, kBpeSpNone when it is no entry (its bytes fall back)
TB_HD uint32_t bpe_sp_symbol(const DevBpe& T, uint32_t c) {
  if (c < 128) return c == ' ' ? T.sp_id : T.sp_ascii[c];
  if (c == kBpeSpSpace) return T.sp_id;
  uint32_t h = (uint32_t)bpe_hash(c) & T.sp_mask;
  for (;;) {
    const uint64_t e = T.sp_cp[h];
    if (e == kBpeSpEmpty) return kBpeSpNone;
    if ((uint32_t)(e >> 32) == c) return (uint32_t)e;
    h = (h + 1) & T.sp_mask;
  }
}

// symbols without bytes in front of the chunk that starts at s: the prepended U+2581
TB_HD int bpe_sp_lead(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s) {
  if (s != 0 || n <= 0) return 0;
  const int mode = T.sp_flags & kBpeSpPrependMask;
  if (mode == kBpeSpPrependAlways) return 1;
  if (mode != kBpeSpPrependUnlessSpace) return 0;
  return (b[0] == ' ' || (n >= 3 && b[0] == 0xE2 && b[1] == 0x96 && b[2] == 0x81)) ? 0 : 1;
}

// End of the chunk that starts at s (s < n): sp? or sp* by the layout, then the code points up to
// the next sp; -1 on invalid UTF-8.
TB_HD int64_t bpe_sp_next_token(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s) {
  int64_t e = s;
  bool head = true;  // still in the chunk's leading sp
  while (e < n) {
    int l;
    const int32_t c = bpe_decode(b, e, n, &l);
    if (c < 0) return -1;
    if (bpe_sp_is_space(c)) {
      if (!head) break;
      if (T.sp_flags & kBpeSpSplit) head = false;
    } else {
      head = false;
    }
    e += l;
  }
  return e;
}

// first chunk start at or after byte s0 (0 < s0; n if none), -1 on invalid UTF-8
TB_HD int64_t bpe_sp_first_start(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s0) {
  int64_t i = s0;
  while (i < n && (b[i] & 0xC0) == 0x80) ++i;
  if (i >= n) return n;
  const int64_t p = bpe_prev_start(b, i);
  int l;
  int32_t c = bpe_decode(b, p, n, &l);
  if (c < 0 || p + l != i) return -1;
  bool after_sp = bpe_sp_is_space(c);
  while (i < n) {
    c = bpe_decode(b, i, n, &l);
    if (c < 0) return -1;
    const bool sp = bpe_sp_is_space(c);
    if (sp && (!after_sp || (T.sp_flags & kBpeSpSplit))) return i;
    after_sp = sp;
    i += l;
  }
  return n;
}

// The chunk's initial symbols (its L bytes are valid UTF-8, lead = bpe_sp_lead of its start):
// put(i, id, len) for symbol number i, which stands for len bytes (0: the prepended U+2581);
// returns their number, at most L + lead.
template <class PutF>
TB_HD int bpe_sp_symbols(const DevBpe& T, const uint8_t* w, int L, int lead, PutF&& put) {
  int m = 0;
  if (lead) put(m++, T.sp_id, 0);
  for (int i = 0; i < L;) {
    int l = 1;
    const int32_t c = bpe_decode(w, i, L, &l);
    const uint32_t id = c < 0 ? kBpeSpNone : bpe_sp_symbol(T, (uint32_t)c);
    if (id != kBpeSpNone) {
      put(m++, id, l);
    } else {
      for (int j = 0; j < l; ++j) put(m++, T.byte_id[w[i + j]], 1);
    }
    i += l;
  }
  return m;
}

struct BpeSp {
  static constexpr bool kSyncSplit = false;
  static constexpr bool kByteSymbols = false;
  static TB_HD int64_t first_start(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s0) {
    return bpe_sp_first_start(T, b, n, s0);
  }
  static TB_HD int64_t range_end(const DevBpe&, const uint8_t*, int64_t, int64_t s1) { return s1; }
  static TB_HD int64_t next_token(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s) {
    return bpe_sp_next_token(T, b, n, s);
  }
  static TB_HD bool whole(const DevBpe&, const uint8_t*, int64_t) { return false; }
  static TB_HD bool has_added(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s0, int64_t s1) {
    return bpe_split_has_added(T, b, n, s0, s1);
  }
  static TB_HD int lead(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s) { return bpe_sp_lead(T, b, n, s); }
  static TB_HD int symbols(const DevBpe& T, const uint8_t* w, int L, int lead, BpeArr c) {
    return bpe_sp_symbols(T, w, L, lead, [&](int i, uint32_t id, int) { c[i] = id; });
  }
};

#ifndef __HIP_DEVICE_COMPILE__
// DevBpe::sp_cp over the code points cps (>= 128) with their ids: open addressing, load <= 1/2
inline void bpe_sp_fill(const uint32_t* cps, const uint32_t* ids, size_t n, uint64_t* slots, uint32_t mask) {
  for (size_t i = 0; i <= mask; ++i) slots[i] = kBpeSpEmpty;
  for (size_t i = 0; i < n; ++i) {
    uint32_t h = (uint32_t)bpe_hash(cps[i]) & mask;
    while (slots[h] != kBpeSpEmpty && (uint32_t)(slots[h] >> 32) != cps[i]) h = (h + 1) & mask;
    slots[h] = ((uint64_t)cps[i] << 32) | ids[i];
  }
}
#endif

}  // namespace tb
