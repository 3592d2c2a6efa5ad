// Byte-level BPE token counting for tokenizers whose pre-tokenizer is
// Sequence[Split(Regex(P), Isolated), ByteLevel(use_regex=false)] (Llama-3, the cl100k_base
// conversions, Qwen2; behind Qwen2's NFC normalizer the NFC gate of bpe.h decides per document): the
// policy BpeSplit of the counting loops of bpe.h.
// Shared by the HIP kernels (csrc/hip/bpe.hip k_bpe_split_count / k_bpe_split_long) and the host
// emulation (csrc/host/tok_module.cpp bpe_count), which CPU tests pin to the `tokenizers` library.
//
// Pattern A: (?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}|
//            ?[^\s\p{L}\p{N}]+[\r\n]*|\s*[\r\n]+|\s+(?!\S)|\s+
// Pattern B: the same with \p{N} for \p{N}{1,3}.
// Every code point is matched by some alternative, so the pieces Isolated leaves are exactly the
// matches, leftmost-first from each token start s (c0 the code point at s, c1 the next):
//   * an apostrophe followed by s/t/m/d or re/ve/ll in either case, or by U+017F (which folds to
//     s), is a contraction;
//   * a letter starts a letter run; so does any c0 other than \r, \n, a letter or a number when c1
//     is a letter ("!abc", "\tabc", " abc");
//   * a number starts a run of up to three numbers (A) or is a token of its own (B); numbers take
//     no leading space;
//   * an "other" code point (not whitespace, letter or number), or U+0020 followed by one, starts
//     the run of others, which swallows the \r and \n after it;
//   * a whitespace run [s, e) that holds a \r or \n ends after its last one; else it is one token
//     when it ends the text or is a single code point, and stops before its last code point
//     otherwise (the lookahead of \s+(?!\S)).
// Classes are those of bpe_classes.inc (both regexes run in the library's one engine).
//
// Lane split. Token starts are not local here (a number run is cut in threes from where it began,
// a run of others decides by its first code point whether "!abc" is one token), but two kinds of
// position start a token whatever precedes them:
//   K1  a code point that is no letter directly after a letter (letters are consumed only by a
//       contraction or a letter run, and either ends with its last letter);
//   K2  a code point that is no whitespace directly after \r or \n (both alternatives that consume
//       newlines end after the last one of their run).
// A range [s0, s1) counts the tokens that start in [sync(s0), sync(s1)), sync(x) the first such
// position at or after x (0 for x = 0, n if there is none): a range without a sync point counts
// nothing and the one before it runs through.
//
// ignore_merges. A pre-token whose bytes are a vocabulary entry is one token: the vocabulary's raw
// bytes sit in an open-addressed table of WpSlot pairs over a pool (wordpiece.h: polynomial hash,
// every key match compared byte for byte).
//
// Added tokens. Up to kBpeSplitMaxAdded of them, contents and offsets in memory; a 256-bit mask of
// their first bytes stands in front of the comparison, so a text byte that starts none costs one
// test. Their text anywhere sends the document to the host, as in bpe.h.
#pragma once
#include "wordpiece.h"

namespace tb {

// bytes of the contraction at the apostrophe b[s], 0 if none
TB_HD int bpe_split_contraction(const uint8_t* b, int64_t n, int64_t s) {
  if (s + 1 >= n) return 0;
  const uint32_t x = b[s + 1] | 0x20u;  // (a byte >= 0x80 stays one)
  if (x == 's' || x == 't' || x == 'm' || x == 'd') return 2;
  if (s + 2 >= n) return 0;
  const uint32_t y = b[s + 2];
  if (b[s + 1] == 0xC5 && y == 0xBF) return 3;  // U+017F LATIN SMALL LETTER LONG S
  const uint32_t yl = y | 0x20u;
  return ((x == 'r' && yl == 'e') || (x == 'v' && yl == 'e') || (x == 'l' && yl == 'l')) ? 3 : 0;
}

// End of the pre-token that starts at the token start s (s < n); -1 on invalid UTF-8.
TB_HD int64_t bpe_split_next_token(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s) {
  int l0;
  const int32_t c0 = bpe_decode(b, s, n, &l0);
  if (c0 < 0) return -1;
  if (c0 == '\'') {
    const int L = bpe_split_contraction(b, n, s);
    if (L) return s + L;
  }
  const int k0 = bpe_cls(T, (uint32_t)c0);
  if (k0 == BPE_L) return bpe_run_end(T, b, s + l0, n, BPE_L);
  if (k0 == BPE_N) {
    int64_t e = s + l0;
    for (int q = 1; q < (T.kind == kBpeSplitA ? 3 : 1) && e < n; ++q) {
      int l;
      const int32_t c = bpe_decode(b, e, n, &l);
      if (c < 0) return -1;
      if (bpe_cls(T, (uint32_t)c) != BPE_N) break;
      e += l;
    }
    return e;
  }
  int l1 = 0, k1 = -1;
  if (s + l0 < n) {
    const int32_t c1 = bpe_decode(b, s + l0, n, &l1);
    if (c1 < 0) return -1;
    k1 = bpe_cls(T, (uint32_t)c1);
  }
  if (k1 == BPE_L && c0 != '\r' && c0 != '\n') return bpe_run_end(T, b, s + l0 + l1, n, BPE_L);
  if (k0 == BPE_O || (c0 == ' ' && k1 == BPE_O)) {
    int64_t e = bpe_run_end(T, b, s + l0 + (k0 == BPE_O ? 0 : l1), n, BPE_O);
    if (e < 0) return -1;
    while (e < n && (b[e] == '\r' || b[e] == '\n')) ++e;
    return e;
  }
  // a whitespace run
  int64_t last = s, e = s + l0, nl = (c0 == '\r' || c0 == '\n') ? e : -1;
  int cnt = 1;
  while (e < n) {
    int l;
    const int32_t c = bpe_decode(b, e, n, &l);
    if (c < 0) return -1;
    if (bpe_cls(T, (uint32_t)c) != BPE_W) break;
    last = e;
    e += l;
    ++cnt;
    if (c == '\r' || c == '\n') nl = e;
  }
  if (nl >= 0) return nl;                  // \s*[\r\n]+
  return (e < n && cnt >= 2) ? last : e;  // \s+(?!\S), \s+
}

// sync(x): the first position of kind K1 or K2 at or after byte x (0 < x); n if none, -1 on
// invalid UTF-8
TB_HD int64_t bpe_split_sync(const DevBpe& T, const uint8_t* b, int64_t n, int64_t x) {
  int64_t i = x;
  while (i < n && (b[i] & 0xC0) == 0x80) ++i;
  if (i >= n) return n;
  const int64_t p = bpe_prev_start(b, i);
  int l;
  int32_t c = bpe_decode(b, p, n, &l);
  if (c < 0 || p + l != i) return -1;
  bool after_letter = bpe_cls(T, (uint32_t)c) == BPE_L, after_nl = c == '\r' || c == '\n';
  while (i < n) {
    c = bpe_decode(b, i, n, &l);
    if (c < 0) return -1;
    const int k = bpe_cls(T, (uint32_t)c);
    if ((after_letter && k != BPE_L) || (after_nl && k != BPE_W)) return i;
    after_letter = k == BPE_L;
    after_nl = c == '\r' || c == '\n';
    i += l;
  }
  return n;
}

// ignore_merges: are the L bytes at w a vocabulary entry?
TB_HD bool bpe_split_whole(const DevBpe& T, const uint8_t* w, int64_t L) {
  if (!T.ignore_merges || L < 2 || L > T.vlongest) return false;
  uint64_t h = 0;
  for (int64_t j = 0; j < L; ++j) h = wp_push(h, w[j]);
  const uint64_t key = wp_key(h, (uint32_t)L, 0);
  uint32_t s = (uint32_t)key & T.vmask;
  for (;;) {
    const uint64_t k = T.vslots[2 * (size_t)s], v = T.vslots[2 * (size_t)s + 1];
    if (v == kWpEmpty) return false;
    if (k == key && (uint32_t)v == (uint32_t)L) {
      const uint8_t* e = T.vpool + (v >> 32);
      int64_t j = 0;
      while (j < L && e[j] == w[j]) ++j;
      if (j == L) return true;
    }
    s = (s + 1) & T.vmask;
  }
}

// does the text of an added token start at a byte in [s0, s1)?
TB_HD bool bpe_split_has_added(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s0, int64_t s1) {
  for (int64_t i = s0; i < s1; ++i) {
    const uint32_t x = b[i];
    if (!((T.amask[x >> 6] >> (x & 63)) & 1)) continue;
    for (int a = 0; a < T.n_added; ++a) {
      const int32_t o = T.aoff[a];
      const int64_t tl = T.aoff[a + 1] - o;
      if (tl <= 0 || i + tl > n || T.added[o] != x) continue;
      int64_t j = 1;
      while (j < tl && b[i + j] == T.added[o + j]) ++j;
      if (j == tl) return true;
    }
  }
  return false;
}

struct BpeSplit : BpeByteLevel {
  static constexpr bool kSyncSplit = true;
  static TB_HD int64_t first_start(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s0) {
    return bpe_split_sync(T, b, n, s0);
  }
  static TB_HD int64_t range_end(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s1) {
    return s1 >= n ? n : bpe_split_sync(T, b, n, s1);
  }
  static TB_HD int64_t next_token(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s) {
    return bpe_split_next_token(T, b, n, s);
  }
  static TB_HD bool whole(const DevBpe& T, const uint8_t* w, int64_t L) { return bpe_split_whole(T, w, L); }
  static TB_HD bool has_added(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s0, int64_t s1) {
    return bpe_split_has_added(T, b, n, s0, s1);
  }
};

#ifndef __HIP_DEVICE_COMPILE__
// the first-byte mask DevBpe::amask of the added tokens (off: n_added + 1 offsets into added)
inline void bpe_added_mask(const uint8_t* added, const int32_t* off, int n_added, uint64_t out[4]) {
  for (int w = 0; w < 4; ++w) out[w] = 0;
  for (int a = 0; a < n_added; ++a)
    if (off[a + 1] > off[a]) out[added[off[a]] >> 6] |= 1ull << (added[off[a]] & 63);
}
#endif

}  // namespace tb
