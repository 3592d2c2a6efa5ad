// Byte-level BPE token counting for the case-aware split patterns: the policy BpeCase of the
// counting loops of bpe.h, beside BpeSplit (bpe_split.h), with the same layout
// Sequence[Split(Regex(P), Isolated), ByteLevel(use_regex=false)], ignore_merges and added tokens.
// Shared by the HIP kernels (csrc/hip/bpe.hip k_bpe_case_count / k_bpe_case_long) and the host
// emulation (csrc/host/tok_module.cpp bpe_count), which CPU tests pin to the `tokenizers` library.
//
// Pattern C (o200k_base), with Up = [\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}], Lo = [\p{Ll}\p{Lm}\p{Lo}\p{M}]
// and S = (?i:'s|'t|'re|'ve|'m|'ll|'d):
//   1  [^\r\n\p{L}\p{N}]?Up*Lo+S?      2  [^\r\n\p{L}\p{N}]?Up+Lo*S?      3  \p{N}{1,3}
//   4   ?[^\s\p{L}\p{N}]+[\r\n/]*      5  \s*[\r\n]+      6  \s+(?!\S)      7  \s+
// Pattern D (Tekken): the same without S and with \p{N} for \p{N}{1,3}.
//
// Classes (bpe_case_classes.inc, 4 bits per code point, read off the library's Split): U (Lu, Lt:
// in Up only), l (Ll: in Lo only), B (Lm, Lo: in both), M (marks: in both, but no \p{L}, so an M is
// also a candidate for the optional leading code point and for the run of alternative 4), N, W, O.
//
// The regex backtracks; what it settles on from a token start s (c0 the code point at s):
//   * Letters from p (bpe_case_letters): let R be the maximal run of U/B/M from p. If an l follows
//     R, alternative 1 takes R and the maximal run of l/B/M after it. Else Lo+ has nothing to take,
//     and Up* gives code points back until one of them can serve: alternative 1 ends after the last
//     B or M of R ("AあB" -> "Aあ", "B"). Else (R is all U) alternative 2 takes R, if it is not
//     empty. In pattern C a contraction right after the match joins it ("DON'T", "it's").
//   * c0 of class U, l, B or M: letters from s. (An M tries the leading code point first, but
//     letters from s give the same end: R only grows by the M itself, which is also where
//     alternative 1 without the leading code point ends when nothing else can serve; that comes
//     before alternative 2 with it: "́ABC" -> "́", "ABC".)
//   * c0 of class O or W other than \r and \n: the leading code point, if letters from the next
//     code point match ("!ABC", " abc", "/b").
//   * c0 of class N: a run of up to three N (C) or a single one (D).
//   * c0 of class O, or U+0020 before an O or M: the maximal run of O/M, then every \r, \n and '/'
//     that follows ("!\n/\n").
//   * else a whitespace run [s, e): with a \r or \n it ends after its last one; else it is one
//     token when it ends the text or is a single code point, and stops before its last code point
//     otherwise.
//
// Lane split, as in bpe_split.h: a range counts the tokens that start in [sync(s0), sync(s1)), and
// two kinds of position start a token whatever precedes them:
//   K1' a code point that is none of U, l, B, M and no apostrophe, directly after a code point X of
//       class U, l or B. X is a \p{L}, which only alternatives 1 and 2 consume, and never as their
//       leading code point; so X lies in the letter part or in the contraction of its token. The
//       letter part cannot pass X (the next code point is in neither set), a contraction ends the
//       token, and none starts after X (no apostrophe): the token ends with X. (X may have been
//       given back by an earlier token's Up*; then it starts or continues a later one, to which
//       the same applies.)
//   K2' a code point that is neither whitespace nor '/', directly after \r or \n. Those are
//       consumed only by the tail [\r\n/]* of alternative 4 and by alternative 5 (the leading
//       code point excludes them, and a whitespace run that holds one is taken by alternative 5);
//       the tail is greedy and stops before a code point outside it, and alternative 5 ends after
//       the last \r or \n of its whitespace run, which is the one before this code point.
// A case boundary is no sync point: whether "DEF" starts a token in "AbcDEFgh" depends on where the
// run began.
#pragma once
#include "bpe_split.h"

namespace tb {

enum BpeCaseCls : int { BPC_O = 0, BPC_U = 1, BPC_LOW = 2, BPC_B = 3, BPC_M = 4, BPC_N = 5, BPC_W = 6 };

TB_HD int bpe_case_cls(const DevBpe& T, uint32_t c) {
  if (c < 128) {
    if (c >= 'A' && c <= 'Z') return BPC_U;
    if (c >= 'a' && c <= 'z') return BPC_LOW;
    if (c >= '0' && c <= '9') return BPC_N;
    if (c == ' ' || (c >= 9 && c <= 13)) return BPC_W;
    return BPC_O;
  }
  const uint32_t w = T.ccls2[(uint32_t)T.ccls1[c >> 7] * 16 + ((c & 127) >> 3)];
  return (int)((w >> (4 * (c & 7))) & 15);
}

TB_HD bool bpe_case_in_sets(int k) { return k >= BPC_U && k <= BPC_M; }

// End of the match of alternative 1, else 2 (without the leading code point) from the code point
// start p; 0 if neither matches, -1 on invalid UTF-8.
TB_HD int64_t bpe_case_letters(const DevBpe& T, const uint8_t* b, int64_t n, int64_t p) {
  int64_t i = p, last_bm = -1;
  int l, k = -1;
  while (i < n) {  // R: the run of U/B/M
    const int32_t c = bpe_decode(b, i, n, &l);
    if (c < 0) return -1;
    k = bpe_case_cls(T, (uint32_t)c);
    if (k != BPC_U && k != BPC_B && k != BPC_M) break;
    i += l;
    if (k != BPC_U) last_bm = i;
    k = -1;
  }
  int64_t e;
  if (k == BPC_LOW) {
    while (i < n) {
      const int32_t c = bpe_decode(b, i, n, &l);
      if (c < 0) return -1;
      k = bpe_case_cls(T, (uint32_t)c);
      if (k != BPC_LOW && k != BPC_B && k != BPC_M) break;
      i += l;
    }
    e = i;
  } else if (last_bm >= 0) {
    e = last_bm;
  } else if (i > p) {
    e = i;
  } else {
    return 0;
  }
  if (T.kind == kBpeCaseC && e < n && b[e] == '\'') e += bpe_split_contraction(b, n, e);
  return e;
}

// End of the pre-token that starts at the token start s (s < n); -1 on invalid UTF-8.
TB_HD int64_t bpe_case_next_token(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s) {
  int l0;
  const int32_t c0 = bpe_decode(b, s, n, &l0);
  if (c0 < 0) return -1;
  const int k0 = bpe_case_cls(T, (uint32_t)c0);
  if (bpe_case_in_sets(k0)) return bpe_case_letters(T, b, n, s);
  if (k0 == BPC_N) {
    int64_t e = s + l0;
    for (int q = 1; q < (T.kind == kBpeCaseC ? 3 : 1) && e < n; ++q) {
      int l;
      const int32_t c = bpe_decode(b, e, n, &l);
      if (c < 0) return -1;
      if (bpe_case_cls(T, (uint32_t)c) != BPC_N) break;
      e += l;
    }
    return e;
  }
  int l1 = 0, k1 = -1;
  if (s + l0 < n) {
    const int32_t c1 = bpe_decode(b, s + l0, n, &l1);
    if (c1 < 0) return -1;
    k1 = bpe_case_cls(T, (uint32_t)c1);
  }
  if (bpe_case_in_sets(k1) && c0 != '\r' && c0 != '\n') return bpe_case_letters(T, b, n, s + l0);
  if (k0 == BPC_O || (c0 == ' ' && k1 == BPC_O)) {
    int64_t e = s + l0;
    while (e < n) {
      int l;
      const int32_t c = bpe_decode(b, e, n, &l);
      if (c < 0) return -1;
      const int k = bpe_case_cls(T, (uint32_t)c);
      if (k != BPC_O && k != BPC_M) break;
      e += l;
    }
    while (e < n && (b[e] == '\r' || b[e] == '\n' || b[e] == '/')) ++e;
    return e;
  }
  // a whitespace run
  int64_t last = s, e = s + l0, nl = (c0 == '\r' || c0 == '\n') ? e : -1;
  int cnt = 1;
  while (e < n) {
    int l;
    const int32_t c = bpe_decode(b, e, n, &l);
    if (c < 0) return -1;
    if (bpe_case_cls(T, (uint32_t)c) != BPC_W) break;
    last = e;
    e += l;
    ++cnt;
    if (c == '\r' || c == '\n') nl = e;
  }
  if (nl >= 0) return nl;                  // \s*[\r\n]+
  return (e < n && cnt >= 2) ? last : e;  // \s+(?!\S), \s+
}

// sync(x): the first position of kind K1' or K2' at or after byte x (0 < x); n if none, -1 on
// invalid UTF-8
TB_HD int64_t bpe_case_sync(const DevBpe& T, const uint8_t* b, int64_t n, int64_t x) {
  int64_t i = x;
  while (i < n && (b[i] & 0xC0) == 0x80) ++i;
  if (i >= n) return n;
  const int64_t p = bpe_prev_start(b, i);
  int l;
  int32_t c = bpe_decode(b, p, n, &l);
  if (c < 0 || p + l != i) return -1;
  int k = bpe_case_cls(T, (uint32_t)c);
  bool after_letter = k == BPC_U || k == BPC_LOW || k == BPC_B, after_nl = c == '\r' || c == '\n';
  while (i < n) {
    c = bpe_decode(b, i, n, &l);
    if (c < 0) return -1;
    k = bpe_case_cls(T, (uint32_t)c);
    if ((after_letter && !bpe_case_in_sets(k) && c != '\'') || (after_nl && k != BPC_W && c != '/')) return i;
    after_letter = k == BPC_U || k == BPC_LOW || k == BPC_B;
    after_nl = c == '\r' || c == '\n';
    i += l;
  }
  return n;
}

struct BpeCase : BpeByteLevel {
  static constexpr bool kSyncSplit = true;
  static TB_HD int64_t first_start(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s0) {
    return bpe_case_sync(T, b, n, s0);
  }
  static TB_HD int64_t range_end(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s1) {
    return s1 >= n ? n : bpe_case_sync(T, b, n, s1);
  }
  static TB_HD int64_t next_token(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s) {
    return bpe_case_next_token(T, b, n, s);
  }
  static TB_HD bool whole(const DevBpe& T, const uint8_t* w, int64_t L) { return bpe_split_whole(T, w, L); }
  static TB_HD bool has_added(const DevBpe& T, const uint8_t* b, int64_t n, int64_t s0, int64_t s1) {
    return bpe_split_has_added(T, b, n, s0, s1);
  }
};

}  // namespace tb
