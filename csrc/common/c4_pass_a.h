// C4QualityFilter, pass A: decisions + rewritten text in scratch (reference c4_filters.rs:147-295).
// rec: LOREM, CURLY, TOO_LONG, NO_PUNCT, TOO_FEW, SENTENCES, NEW_LEN
// src: (byte offset of the new text in the doc's scratch, or -1 = unchanged original; length)
#pragma once
#include "devplan.h"
#include "doc_text.h"
#include "uax29.h"

namespace tb {

// Case-insensitive substring test as Rust `to_lowercase().contains(pat)` for an ASCII lowercase
// pattern: ASCII letters fold, U+212A KELVIN SIGN lowercases to 'k'; no other code point
// lowercases to a sequence that can match an ASCII-letter/space pattern.
TB_HD bool ci_contains(const uint8_t* b, uint32_t n, const char* pat, int plen) {
  for (uint32_t s = 0; s < n; ++s) {
    uint32_t i = s;
    int j = 0;
    for (; j < plen; ++j) {
      if (i >= n) break;
      const char pc = pat[j];
      uint8_t c = b[i];
      if (c >= 'A' && c <= 'Z') c = (uint8_t)(c + 32);
      if (c == (uint8_t)pc) { ++i; continue; }
      if (pc == 'k' && i + 2 < n && b[i] == 0xE2 && b[i + 1] == 0x84 && b[i + 2] == 0xAA) { i += 3; continue; }
      break;
    }
    if (j == plen) return true;
  }
  return false;
}

// Sentence count of split_into_sentences() over code points [s, e) (already trimmed text),
// saturated: sentences are counted chunk by chunk and counting stops after the chunk
// that reaches `limit`, so the result is exact below `limit` and >= limit otherwise (C4's
// min_num_sentences test and its reason string only use counts below the limit). A chunk's
// breaks are compacted, every segment with a non-whitespace code point counts once; the part
// before the chunk's first break continues the previous chunk's last segment (`seen`: that
// segment already counted).
template <class P>
TB_HD uint32_t count_sentences_upto(DocCtx<P>& x, const Cps& c, uint32_t s, uint32_t e, uint32_t limit) {
  const uint32_t m = e - s;
  if (m == 0 || limit == 0) return 0;
  constexpr uint32_t kChunk = 256;
  const auto mark = x.mark();
  uint32_t* starts = x.template alloc_hot<uint32_t>(kChunk + 1);
  uint32_t* segf = x.template alloc_hot<uint32_t>(kChunk + 1);
  if (x.overflow) return 0;
  const PropArr prop = c.props() + s;
  CpsAcc acc{prop};
  uint32_t cnt = 0;
  bool seen = false;
  for (uint32_t base = 0; base < m && cnt < limit; base += kChunk) {
    const uint32_t len = m - base < kChunk ? m - base : kChunk;
    const uint32_t NS = x.par.template compact<int>(
        len, [&](uint32_t i, int&) { const uint32_t g = base + i; return g == 0 || sb_break(acc, (int)m, (int)g); },
        [&](uint32_t i, uint32_t k, int&) { starts[k] = i; });
    x.par.sync();
    const uint32_t first = NS ? starts[0] : len;
    const bool lead_any = x.par.template sum<uint32_t>(first, [&](uint32_t i) {
      return is_ws(prop[base + i]) ? 0u : 1u;
    }) != 0;
    const uint32_t segs = x.par.template sum<uint32_t>(NS, [&](uint32_t k) {
      const uint32_t a = starts[k], bnd = k + 1 < NS ? starts[k + 1] : len;
      uint32_t f = 0;
      for (uint32_t j = a; j < bnd; ++j) if (!is_ws(prop[base + j])) { f = 1; break; }
      segf[k] = f;
      return f;
    });
    x.par.sync();
    if (!seen && lead_any) ++cnt;
    cnt += segs;
    seen = NS ? segf[NS - 1] != 0 : (seen || lead_any);
    x.par.sync();
  }
  x.reset(mark);
  return cnt;
}

TB_HD bool end_punct(uint32_t c) {
  return c == '.' || c == '!' || c == '?' || c == '"' || c == '\'' || c == 0x201D;
}

// Case-insensitive prefix test with the same folding as ci_contains (ASCII letters, and
// U+212A KELVIN SIGN as 'k'): does `pat` start at b[0] within n bytes?
TB_HD bool ci_starts_with(const uint8_t* b, uint32_t n, const char* pat, int plen) {
  uint32_t i = 0;
  for (int j = 0; j < plen; ++j) {
    if (i >= n) return false;
    const char pc = pat[j];
    uint8_t c = b[i];
    if (c >= 'A' && c <= 'Z') c = (uint8_t)(c + 32);
    if (c == (uint8_t)pc) { ++i; continue; }
    if (pc == 'k' && i + 2 < n && b[i] == 0xE2 && b[i + 1] == 0x84 && b[i + 2] == 0xAA) { i += 3; continue; }
    return false;
  }
  return true;
}

// Bits of the per-line pattern flags (c4_pass_a)
enum : uint32_t { C4F_JS = 1, C4F_POLICY = 2 };

// C4 pass A's first pass over the bytes (c4_byte_scan): the whole-document filters, a possible
// citation, and whether a javascript / policy phrase starts anywhere (C4F_JS / C4F_POLICY).
enum : uint32_t { C4S_LOREM = 4, C4S_CURLY = 8, C4S_CITE = 16 };

// The 16 bytes of the text b[0, n) from byte s, ASCII-lowercased, little endian in lo and hi
// (zero past the end): the five aligned dwords that hold them, loaded together and shifted into
// place.
TB_HD void lower16_at(const uint8_t* b, uint32_t n, uint32_t s, uint64_t& lo, uint64_t& hi) {
  const uint32_t sh = (uint32_t)((uintptr_t)(b + s) & 3u);
  const int64_t q = (int64_t)s - sh;
  uint32_t d[5];
#pragma unroll
  for (uint32_t k = 0; k < 5; ++k) d[k] = text_dword(b, n, q + 4 * k);
  const uint64_t w0 = (uint64_t)d[0] | ((uint64_t)d[1] << 32), w1 = (uint64_t)d[2] | ((uint64_t)d[3] << 32);
  uint64_t v0 = w0, v1 = w1;
  if (sh) {
    v0 = (w0 >> (8 * sh)) | (w1 << (64 - 8 * sh));
    v1 = (w1 >> (8 * sh)) | ((uint64_t)d[4] << (64 - 8 * sh));
  }
  lo = swar_lower8(v0);
  hi = swar_lower8(v1);
}

// Does the phrase pat (len bytes, 9 <= len <= 16; plo / phi: its bytes packed) start at byte s,
// case-folded as ci_starts_with folds? lo / hi are lower16_at(b, n, s). kpos: the index of the
// phrase's 'k' (-1: none). A Kelvin sign there is three bytes long and moves the rest of the
// phrase, so only a window whose first difference is 0xE2 at kpos goes to the byte-wise test.
TB_HD bool c4_phrase_eq(const uint8_t* b, uint32_t n, uint32_t s, uint64_t lo, uint64_t hi, uint64_t plo,
                        uint64_t phi, int len, int kpos, const char* pat) {
  const uint64_t xl = lo ^ plo;
  const uint64_t xh = (hi ^ phi) & (~0ull >> (64 - 8 * (len - 8)));
  if ((xl | xh) == 0) return true;
  if (kpos < 0) return false;
  const int j = xl ? (__builtin_ctzll(xl) >> 3) : 8 + (__builtin_ctzll(xh) >> 3);
  if (j != kpos) return false;
  const uint32_t c = (uint32_t)((kpos < 8 ? lo >> (8 * kpos) : hi >> (8 * (kpos - 8))) & 0xFFu);
  return c == 0xE2 && ci_starts_with(b + s, n - s, pat, len);
}
#define TB_C4_PHRASE_EQ(pat, kpos) \
  c4_phrase_eq(b, n, s, lo, hi, pack_le(pat, sizeof(pat) - 1), pack_le(pat, sizeof(pat) - 1, 8), \
               (int)sizeof(pat) - 1, kpos, pat)

// The pattern bits (C4F_JS | C4F_POLICY) of the phrases starting at byte s (case-folded). lw holds
// the lowercased bytes from s, at least five of them (scan_bytes16). Every phrase starts with
// ASCII letters and spaces other than 'k' (the only pattern letter with a multi-byte match, the
// Kelvin sign) up to its fifth byte, "cookie policy" up to its third: a phrase can only match
// where lw starts with its prefix, and a text almost never holds one of these prefixes without
// the phrase. Only such a position loads its 16 bytes and compares them to the packed phrase.
TB_HD uint32_t c4_phrases_at(const DevC4& c4, const uint8_t* b, uint32_t n, uint32_t s, uint64_t lw) {
  const uint64_t p5 = lw & 0xFFFFFFFFFFull;
  const uint32_t c3 = (uint32_t)(lw >> 24) & 0xFFu;
  int t;
  if (p5 == pack5("terms")) t = 1;
  else if (p5 == pack5("use c")) t = 6;
  else if (p5 == pack5("use o")) t = 5;
  else if (p5 == pack5("uses ")) t = 4;
  else if (p5 == pack5("priva")) t = 2;
  else if (p5 == pack5("javas")) t = 0;
  else if (((uint32_t)lw & 0xFFFFFFu) == pack3("coo") && (c3 == 'k' || c3 == 0xE2)) t = 3;
  else return 0;
  if (t == 0 ? !c4.filter_javascript : !c4.filter_policy) return 0;
  uint64_t lo, hi;
  lower16_at(b, n, s, lo, hi);
  bool hit;
  switch (t) {
    case 0: hit = TB_C4_PHRASE_EQ("javascript", -1); break;
    case 1: hit = TB_C4_PHRASE_EQ("terms of use", -1); break;
    case 2: hit = TB_C4_PHRASE_EQ("privacy policy", -1); break;
    case 3: hit = TB_C4_PHRASE_EQ("cookie policy", 3); break;
    case 4: hit = TB_C4_PHRASE_EQ("uses cookies", 8); break;
    case 5: hit = TB_C4_PHRASE_EQ("use of cookies", 10); break;
    default: hit = TB_C4_PHRASE_EQ("use cookies", 7); break;
  }
  return hit ? (t == 0 ? C4F_JS : C4F_POLICY) : 0u;
}

// Does "lorem ipsum" start at byte s (case-folded)? lw as for c4_phrases_at.
TB_HD bool c4_lorem_at(const uint8_t* b, uint32_t n, uint32_t s, uint64_t lw) {
  if ((lw & 0xFFFFFFFFFFull) != pack5("lorem")) return false;
  uint64_t lo, hi;
  lower16_at(b, n, s, lo, hi);
  return TB_C4_PHRASE_EQ("lorem ipsum", -1);
}
#undef TB_C4_PHRASE_EQ

// Every byte position s of b[0, n) visited as f(s, c0, c1, lw): its byte, the next one (0 past the
// end) and lw, the bytes from s to the end of its 8-byte window ASCII-lowercased (little endian,
// five to eight of them, zero past the text and above them). Items are four aligned
// dwords whose five loads (one of look-ahead) are issued together, and the lowercase windows
// come from SWAR shifts: one memory round trip per 16 bytes, no per-byte loads.
template <class P, class F>
TB_HD void scan_bytes16(DocCtx<P>& x, const uint8_t* b, uint32_t n, F&& f) {
  const uintptr_t a0 = (uintptr_t)b & ~(uintptr_t)3;
  const uint32_t head = (uint32_t)((uintptr_t)b - a0);
  const uint32_t nd = (head + n + 3) >> 2;
  const uint32_t* w = (const uint32_t*)a0;
  auto dw = [&](uint32_t k) -> uint32_t {  // dword k of the aligned stream, bytes outside the text zero
    return k < nd ? text_dword(b, n, (int64_t)4 * k - head) : 0u;
  };
  x.par.for_n((nd + 3) >> 2, [&](uint32_t g) {
    uint32_t d[5];
#pragma unroll
    for (uint32_t i = 0; i < 5; ++i) d[i] = dw(4 * g + i);
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t k = 4 * g + i;
      const uint64_t v = (uint64_t)d[i] | ((uint64_t)d[i + 1] << 32);
      const uint64_t lo = swar_lower8(v);
      for (uint32_t r = 0; r < 4; ++r) {
        const int64_t sp = (int64_t)4 * k + r - head;
        if (sp < 0 || sp >= (int64_t)n) continue;
        f((uint32_t)sp, (uint32_t)(v >> (8 * r)) & 0xFFu, (uint32_t)(v >> (8 * r + 8)) & 0xFFu,
          lo >> (8 * r));
      }
    }
  });
}

// Could a javascript / policy phrase start here (its case-folded 3-byte prefix)? The cheap first
// test of every position; c4_phrases_at goes on with the longer prefix.
TB_HD bool c4_phrase_prefix(uint64_t lw) {
  const uint32_t l3 = (uint32_t)lw & 0xFFFFFFu;
  return l3 == pack3("jav") || l3 == pack3("ter") || l3 == pack3("pri") || l3 == pack3("coo") || l3 == pack3("use");
}

// One pass over the bytes: lorem ipsum and curly brackets (lowercase().contains("lorem ipsum") ==
// the pattern starts, case-folded, at some 'l'), a possible citation ('[' followed by a digit:
// a non-ASCII byte after the '[' counts too, so the test is conservative) and the phrase bits;
// only a position whose 5-byte prefix matches runs the exact comparison (c4_phrase_eq).
template <class P>
TB_HD uint32_t c4_byte_scan(DocCtx<P>& x, const DevC4& c4, const uint8_t* b, uint32_t n) {
  uint32_t acc = 0;
  const bool phrases = c4.filter_javascript || c4.filter_policy;
  scan_bytes16(x, b, n, [&](uint32_t s, uint32_t c0, uint32_t c1, uint64_t lw) {
    if (c4.filter_curly_bracket && (c0 == '{' || c0 == '}')) acc |= C4S_CURLY;
    if (c0 == '[' && ((c1 >= '0' && c1 <= '9') || c1 >= 0x80)) acc |= C4S_CITE;
    if (c4.filter_lorem_ipsum && c4_lorem_at(b, n, s, lw)) acc |= C4S_LOREM;
    if (phrases && c4_phrase_prefix(lw)) acc |= c4_phrases_at(c4, b, n, s, lw);
  });
  return x.par.reduce_or(acc);
}

// C4 pass A, common end: the joined kept lines Jb[0, Jtot) are trimmed and their sentences counted
// (saturated at min_num_sentences), then the record and the rewritten text's source are written.
template <class P>
TB_HD void c4_finish(DocCtx<P>& x, const DevC4& c4, uint32_t n, uint8_t* Jb, uint32_t Jtot, int64_t s_long,
                     int64_t s_punct, int64_t s_few, int64_t* r, int64_t* src) {
  Cps jc = decode(x, Jb, Jtot);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  const uint32_t JC = jc.n;
  const PropArr jprop = jc.props();
  uint32_t tcs, tce;
  trim_span(x, jprop, JC, tcs, tce);
  uint32_t nsent = 0, bstart = 0, blen = 0;
  if (tcs < tce) {
    const uint32_t lim = c4.min_num_sentences > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)c4.min_num_sentences;
    nsent = count_sentences_upto(x, jc, tcs, tce, lim);
    bstart = jc.o(tcs);
    blen = jc.o(tce) - jc.o(tcs);
  }
  x.stamp(PH_C4_SENT);
  const int64_t jrel = (int64_t)((const char*)Jb - x.scr) + bstart;
  // The rewrite can only grow a document by one '\n' per sentence not followed by whitespace
  // (split_paragraph=false). Bounding the growth to kC4MaxGrowth bytes lets the host size the
  // next version's buffer (and its D2H copy) up front without a sync; the rare document that
  // would exceed it is recomputed on the CPU path.
  if (blen > n + kC4MaxGrowth) {
    x.set_flag(DOC_NEEDS_CPU);
    x.par.single([&]() { src[0] = 0; src[1] = 0; });
    return;
  }
  x.par.single([&]() {
    r[0] = 0; r[1] = 0; r[2] = s_long; r[3] = s_punct; r[4] = s_few; r[5] = nsent; r[6] = blen;
    src[0] = jrel;
    src[1] = blen;
  });
}

// The code point that ends the non-empty byte span [s, e) of b[0, n).
TB_HD uint32_t last_cp(const uint8_t* b, uint32_t s, uint32_t e, uint32_t n) {
  uint32_t p = e - 1;
  while (p > s && !utf8_is_lead(b[p])) --p;
  int len;
  return utf8_decode(b, p, n, &len);
}

// C4 pass A for a document with no citation to remove: every processed line is its trimmed
// original line, so the processed text Pb, the per-code-point line ids and the kept-byte prefix
// of the general path are not built. The lines come as trimmed byte spans [lbs[k], lbe[k])
// (lbs[NLn] = 0xFFFFFFFF) with their word counts and longest words; the phrase search, terminal
// punctuation and the join read the original bytes of each line's span. Same records and
// rewritten text as the general path.
template <class P>
TB_HD void c4_plain_tail(DocCtx<P>& x, const DevC4& c4, const uint8_t* b, uint32_t n, uint32_t NLn,
                         const uint32_t* lbs, const uint32_t* lbe, const uint32_t* nw, const uint32_t* mx,
                         uint32_t phrase_bits, int64_t* r, int64_t* src, uint32_t* wout = nullptr) {
  uint32_t* pf = x.template alloc_hot<uint32_t>(NLn + 1);   // pattern flags per line
  uint8_t* code = x.template alloc_hot<uint8_t>(NLn + 1);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  auto line_of_byte = [&](uint32_t bs) {  // last line with byte start <= bs
    uint32_t lo = 0, hi = NLn;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (lbs[mid] <= bs) lo = mid; else hi = mid;
    }
    return lo;
  };
  const bool phrases = NLn > 0 && (phrase_bits & (C4F_JS | C4F_POLICY));
  if (phrases) {
    x.par.for_n(NLn, [&](uint32_t k) { pf[k] = 0; });
    x.par.sync();
    // only when the byte scan saw a phrase somewhere (rare). A phrase (letters and spaces, starting
    // with a letter) that matches at a byte lies inside one line's trimmed span: it cannot cross
    // the line feed or run into trailing whitespace.
    scan_bytes16(x, b, n, [&](uint32_t s, uint32_t, uint32_t, uint64_t lw) {
      if (!c4_phrase_prefix(lw)) return;
      const uint32_t bits = c4_phrases_at(c4, b, n, s, lw);
      if (bits) P::or32(&pf[line_of_byte(s)], bits);
    });
    x.par.sync();
  }
  x.par.for_n(NLn, [&](uint32_t k) {
    const uint32_t s0 = lbs[k], e0 = lbe[k], ln = e0 - s0;
    const uint32_t fl = phrases ? pf[k] : 0u;
    uint8_t cd = 0;
    if (c4.max_word_length > 0 && (int64_t)mx[k] > c4.max_word_length) {
      cd = 1;
    } else if (c4.filter_no_terminal_punct) {
      const bool term = ln > 0 && end_punct(last_cp(b, s0, e0, n));
      const bool ell = ln >= 3 && b[e0 - 1] == '.' && b[e0 - 2] == '.' && b[e0 - 3] == '.';
      if (!term || ell) cd = 2;
    }
    if (cd == 0 && c4.min_words_per_line > 0 && (int64_t)nw[k] < c4.min_words_per_line) cd = 3;
    if (cd == 0 && c4.filter_javascript && (fl & C4F_JS)) cd = 4;
    if (cd == 0 && c4.filter_policy && (fl & C4F_POLICY)) cd = 5;
    code[k] = cd;
  });
  x.par.sync();
  const uint64_t s12 = x.par.template sum<uint64_t>(NLn, [&](uint32_t k) {
    return (uint64_t)(code[k] == 1) | ((uint64_t)(code[k] == 2) << 32);
  });
  const int64_t s_long = (int64_t)(s12 & 0xFFFFFFFFull), s_punct = (int64_t)(s12 >> 32);
  const int64_t s_few = x.par.template sum<int64_t>(NLn, [&](uint32_t k) { return (int64_t)(code[k] == 3); });
  if (wout) {
    // words of the rewrite (the kept lines joined by '\n', trimmed): words never cross a line
    // feed, so they are the kept lines' words (StageOut::dict_words of the next version)
    const uint32_t wk = x.par.template sum<uint32_t>(NLn, [&](uint32_t k) { return code[k] == 0 ? nw[k] : 0u; });
    x.par.single([&]() { *wout = wk; });
  }
  x.stamp(PH_C4_CODES);
  // ---- joined kept lines (HBM: read back by pass B), copied byte by byte ----
  uint32_t* joff = x.template alloc_hot<uint32_t>(NLn + 1);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  uint32_t Jtot = x.par.template scan<uint32_t>(
      NLn, 0u, [](uint32_t a, uint32_t b2) { return a + b2; },
      [&](uint32_t k) { return code[k] == 0 ? lbe[k] - lbs[k] + 1 : 0u; },
      [&](uint32_t k, uint32_t e) { joff[k] = e; });
  if (Jtot > 0) Jtot -= 1;
  uint8_t* Jb = x.template alloc_global<uint8_t>(Jtot + 1);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  x.par.sync();
  if (NLn > 0) {
    x.par.for_n(n, [&](uint32_t i) {
      const uint32_t k = line_of_byte(i);
      if (code[k] != 0 || i < lbs[k] || i >= lbe[k]) return;
      Jb[joff[k] + (i - lbs[k])] = b[i];
    });
    x.par.for_n(NLn, [&](uint32_t k) {
      const uint32_t ln = lbe[k] - lbs[k];
      if (code[k] == 0 && joff[k] + ln < Jtot) Jb[joff[k] + ln] = '\n';
    });
  }
  x.par.sync();
  x.stamp(PH_C4_JOIN);
  c4_finish(x, c4, n, Jb, Jtot, s_long, s_punct, s_few, r, src);
}

// The plain path from this pass's own decode and lines [la, lb) (code points): words come from
// one segmentation of the whole text — the words of a trimmed line are exactly the document's
// words inside its span (UAX#29 always breaks around a line feed, WB3a/b, and trimming only
// drops whitespace, which no word contains) — assigned to lines by their first code point.
template <class P>
TB_HD void c4_pass_a_plain(DocCtx<P>& x, const DevC4& c4, const uint8_t* b, uint32_t n, const Cps& c,
                           const uint32_t* la, const uint32_t* lb, uint32_t NLn, int64_t* r, int64_t* src,
                           uint32_t phrase_bits) {
  const OffArr off = c.offs();
  uint32_t* lbs = x.template alloc_hot<uint32_t>(NLn + 1);
  uint32_t* lbe = x.template alloc_hot<uint32_t>(NLn + 1);
  uint32_t* nw = x.template alloc_hot<uint32_t>(NLn + 1);
  uint32_t* mx = x.template alloc_hot<uint32_t>(NLn + 1);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  x.par.for_n(NLn, [&](uint32_t k) { lbs[k] = off[la[k]]; lbe[k] = off[lb[k]]; nw[k] = 0; mx[k] = 0; });
  x.par.single([&]() { lbs[NLn] = 0xFFFFFFFFu; });
  x.par.sync();
  x.stamp(PH_C4_CITE);
  if (NLn > 0) {
    auto line_of_cp = [&](uint32_t cs) {  // last line with la <= cs
      uint32_t lo = 0, hi = NLn;
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (la[mid] <= cs) lo = mid; else hi = mid;
      }
      return lo;
    };
    const auto mw = x.mark();
    Words wd = words(x, c);
    if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
    x.par.for_n(wd.n, [&](uint32_t q) {
      const uint32_t k = line_of_cp(wd.cs[q]);
      P::add32(&nw[k], 1u);
      P::max32(&mx[k], wd.ce[q] - wd.cs[q]);
    });
    x.par.sync();
    x.reset(mw);
  }
  x.stamp(PH_C4_WORDS);
  c4_plain_tail(x, c4, b, n, NLn, lbs, lbe, nw, mx, phrase_bits, r, src);
}

// The plain path from the stage's line export (LineStat region, header = line count): no decode,
// lines or words here.
template <class P>
TB_HD void c4_pass_a_export(DocCtx<P>& x, const DevC4& c4, const uint8_t* b, uint32_t n, const uint32_t* region,
                            uint32_t NLn, int64_t* r, int64_t* src, uint32_t phrase_bits, uint32_t* wout = nullptr) {
  const LineStat* ls = (const LineStat*)(region + 4);
  uint32_t* lbs = x.template alloc_hot<uint32_t>(NLn + 1);
  uint32_t* lbe = x.template alloc_hot<uint32_t>(NLn + 1);
  uint32_t* nw = x.template alloc_hot<uint32_t>(NLn + 1);
  uint32_t* mx = x.template alloc_hot<uint32_t>(NLn + 1);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  x.par.for_n(NLn, [&](uint32_t k) {
    const LineStat e = ls[k];
    lbs[k] = e.bs; lbe[k] = e.be; nw[k] = e.nw; mx[k] = e.mx;
  });
  x.par.single([&]() { lbs[NLn] = 0xFFFFFFFFu; });
  x.par.sync();
  x.stamp(PH_C4_WORDS);
  c4_plain_tail(x, c4, b, n, NLn, lbs, lbe, nw, mx, phrase_bits, r, src, wout);
}

// The byte past a citation starting at b[i] == '[' inside [i, e) (a trimmed line), 0 when none
// starts there, 0xFFFFFFFF when the match depends on a non-ASCII byte (a Unicode digit or space).
TB_HD uint32_t c4_cite_end_bytes(const UcdView& ucd, const uint8_t* b, uint32_t i, uint32_t e) {
  uint32_t p = i + 1;
  if (p >= e) return 0;
  if (b[p] >= 0x80) return 0xFFFFFFFFu;
  if (b[p] < '0' || b[p] > '9') return 0;
  while (p < e && b[p] >= '0' && b[p] <= '9') ++p;
  while (true) {
    if (p < e && b[p] >= 0x80) return 0xFFFFFFFFu;  // a non-ASCII digit could continue \d+
    if (!(p < e && b[p] == ',')) break;
    uint32_t q = p + 1;
    while (q < e && b[q] < 0x80 && (ucd.props(b[q]) & P_WS)) ++q;
    if (q < e && b[q] >= 0x80) return 0xFFFFFFFFu;  // Unicode whitespace or digit
    if (!(q < e && b[q] >= '0' && b[q] <= '9')) break;
    while (q < e && b[q] >= '0' && b[q] <= '9') ++q;
    p = q;
  }
  return (p < e && b[p] == ']') ? p + 1 : 0;
}

// C4 pass A for a document with a possible citation, from the stage's line export: the
// citations (reference CITATION_REGEX, c4_filters.rs:33, applied to each trimmed line) are found on
// the bytes of the exported trimmed line spans, the processed lines Pb are built byte-parallel
// (a removed-byte bitmap and its prefix popcounts give every kept byte's place), and only the lines
// that lost a citation are segmented again; no decode, no Rust lines, no per-code-point line ids.
// Returns false without writing anything when a candidate needs Unicode classes (a non-ASCII byte
// where \d or \s could continue the match): the general path runs then.
template <class P>
TB_HD bool c4_pass_a_cite_export(DocCtx<P>& x, const DevC4& c4, const uint8_t* b, uint32_t n, const uint32_t* region,
                                 uint32_t NLn, int64_t* r, int64_t* src) {
  const LineStat* ls = (const LineStat*)(region + 4);
  const auto mark0 = x.mark();
  const uint32_t nwd = (n + 31) / 32 + 1;
  uint32_t* lbs = x.template alloc_hot<uint32_t>(NLn + 1);
  uint32_t* lbe = x.template alloc_hot<uint32_t>(NLn + 1);
  uint32_t* nw = x.template alloc_hot<uint32_t>(NLn + 1);
  uint32_t* mx = x.template alloc_hot<uint32_t>(NLn + 1);
  uint32_t* plen = x.template alloc_hot<uint32_t>(NLn + 1);
  uint32_t* poff = x.template alloc_hot<uint32_t>(NLn + 1);
  uint8_t* code = x.template alloc_hot<uint8_t>(NLn + 1);    // 1: the line lost a citation (then the codes)
  uint32_t* pf = x.template alloc_hot<uint32_t>(NLn + 1);    // pattern flags per line
  uint32_t* rmb = x.template alloc_hot<uint32_t>(nwd);       // removed bytes
  uint32_t* wr = x.template alloc_hot<uint32_t>(nwd + 1);    // exclusive popcount prefix of rmb
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return true; }
  x.par.for_n(NLn, [&](uint32_t k) {
    const LineStat e = ls[k];
    lbs[k] = e.bs; lbe[k] = e.be; nw[k] = e.nw; mx[k] = e.mx; code[k] = 0; pf[k] = 0;
  });
  x.par.for_n(nwd, [&](uint32_t w) { rmb[w] = 0; });
  x.par.single([&]() { lbs[NLn] = 0xFFFFFFFFu; });
  x.par.sync();
  auto line_of_byte = [&](uint32_t bs) {  // last line with byte start <= bs
    uint32_t lo = 0, hi = NLn;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (lbs[mid] <= bs) lo = mid; else hi = mid;
    }
    return lo;
  };
  uint32_t bad = 0;
  x.par.for_n(n, [&](uint32_t i) {
    if (b[i] != '[') return;
    const uint32_t k = line_of_byte(i), e = lbe[k];
    if (i < lbs[k] || i >= e) return;
    const uint32_t ce = c4_cite_end_bytes(x.ucd, b, i, e);
    if (ce == 0xFFFFFFFFu) { bad = 1; return; }
    if (ce == 0) return;
    for (uint32_t q = i; q < ce; ++q) P::or32(&rmb[q >> 5], 1u << (q & 31));
    code[k] = 1;
  });
  x.par.sync();
  if (x.par.reduce_or(bad)) {
    x.reset(mark0);
    return false;
  }
  x.par.template scan<uint32_t>(
      nwd, 0u, [](uint32_t a, uint32_t c2) { return a + c2; }, [&](uint32_t w) { return (uint32_t)__builtin_popcount(rmb[w]); },
      [&](uint32_t w, uint32_t e) { wr[w] = e; });
  x.par.sync();
  auto rank = [&](uint32_t i) {  // removed bytes before byte i
    return wr[i >> 5] + (uint32_t)__builtin_popcount(rmb[i >> 5] & ((1u << (i & 31)) - 1u));
  };
  auto removed = [&](uint32_t i) { return (rmb[i >> 5] >> (i & 31)) & 1u; };
  x.par.for_n(NLn, [&](uint32_t k) { plen[k] = (lbe[k] - lbs[k]) - (rank(lbe[k]) - rank(lbs[k])); });
  x.par.sync();
  const uint32_t Ptot = x.par.template scan<uint32_t>(
      NLn, 0u, [](uint32_t a, uint32_t c2) { return a + c2; }, [&](uint32_t k) { return plen[k] + 1u; },
      [&](uint32_t k, uint32_t e) { poff[k] = e; });
  uint8_t* Pb = x.template alloc<uint8_t>(Ptot + 1);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return true; }
  x.par.sync();
  x.par.for_n(n, [&](uint32_t i) {
    const uint32_t k = line_of_byte(i);
    if (i < lbs[k] || i >= lbe[k] || removed(i)) return;
    Pb[poff[k] + (i - lbs[k]) - (rank(i) - rank(lbs[k]))] = b[i];
  });
  x.par.for_n(NLn, [&](uint32_t k) { Pb[poff[k] + plen[k]] = '\n'; });
  x.par.single([&]() { poff[NLn] = Ptot; });
  x.par.sync();
  x.stamp(PH_C4_CITE);
  auto line_of_p = [&](uint32_t bs) {  // last line with poff <= bs
    uint32_t lo = 0, hi = NLn;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (poff[mid] <= bs) lo = mid; else hi = mid;
    }
    return lo;
  };
  // words of the lines that lost a citation (joined with '\n', so no word spans two lines)
  {
    uint32_t* coff = x.template alloc_hot<uint32_t>(NLn + 1);
    if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return true; }
    const uint32_t Ctot = x.par.template scan<uint32_t>(
        NLn, 0u, [](uint32_t a, uint32_t c2) { return a + c2; },
        [&](uint32_t k) { return code[k] ? plen[k] + 1 : 0u; }, [&](uint32_t k, uint32_t e) { coff[k] = e; });
    x.par.for_n(NLn, [&](uint32_t k) { if (code[k]) { nw[k] = 0; mx[k] = 0; } });
    x.par.sync();
    if (Ctot > 0) {
      const auto mc = x.mark();
      uint8_t* Pc = x.template alloc<uint8_t>(Ctot + 1);
      if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return true; }
      x.par.for_n(Ptot, [&](uint32_t i) {
        const uint32_t k = line_of_p(i);
        if (code[k] && i - poff[k] <= plen[k]) Pc[coff[k] + (i - poff[k])] = Pb[i];  // (its '\n' too)
      });
      x.par.sync();
      uint32_t dict = 0;
      Cps cc = decode(x, Pc, Ctot, false, &dict);
      if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return true; }
      if (dict) {  // dictionary-script text in a cited line: its words need ICU
        x.set_flag(DOC_NEEDS_CPU);
        return true;
      }
      Words cw = words(x, cc);
      if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return true; }
      x.par.for_n(cw.n, [&](uint32_t q) {
        const uint32_t bs = cw.bs[q];
        uint32_t lo = 0, hi = NLn;  // last line with coff <= bs: the cited line holding the word
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) >> 1;
          if (coff[mid] <= bs) lo = mid; else hi = mid;
        }
        P::add32(&nw[lo], 1u);
        P::max32(&mx[lo], cw.ce[q] - cw.cs[q]);
      });
      x.par.sync();
      x.reset(mc);
    }
  }
  x.stamp(PH_C4_WORDS);
  if (c4.filter_javascript || c4.filter_policy) {
    scan_bytes16(x, Pb, Ptot, [&](uint32_t s, uint32_t, uint32_t, uint64_t lw) {
      if (!c4_phrase_prefix(lw)) return;
      const uint32_t bits = c4_phrases_at(c4, Pb, Ptot, s, lw);
      if (bits) P::or32(&pf[line_of_p(s)], bits);
    });
  }
  x.par.sync();
  x.par.for_n(NLn, [&](uint32_t k) {
    const uint8_t* lp = Pb + poff[k];
    const uint32_t ln = plen[k];
    uint8_t cd = 0;
    if (c4.max_word_length > 0 && (int64_t)mx[k] > c4.max_word_length) {
      cd = 1;
    } else if (c4.filter_no_terminal_punct) {
      bool term = false;
      if (ln > 0) {
        uint32_t st = ln - 1;
        while (st > 0 && (lp[st] & 0xC0) == 0x80) --st;
        int len;
        term = end_punct(utf8_decode(lp, st, ln, &len));
      }
      const bool ell = ln >= 3 && lp[ln - 1] == '.' && lp[ln - 2] == '.' && lp[ln - 3] == '.';
      if (!term || ell) cd = 2;
    }
    if (cd == 0 && c4.min_words_per_line > 0 && (int64_t)nw[k] < c4.min_words_per_line) cd = 3;
    if (cd == 0 && c4.filter_javascript && (pf[k] & C4F_JS)) cd = 4;
    if (cd == 0 && c4.filter_policy && (pf[k] & C4F_POLICY)) cd = 5;
    code[k] = cd;
  });
  x.par.sync();
  const uint64_t s12 = x.par.template sum<uint64_t>(NLn, [&](uint32_t k) {
    return (uint64_t)(code[k] == 1) | ((uint64_t)(code[k] == 2) << 32);
  });
  const int64_t s_long = (int64_t)(s12 & 0xFFFFFFFFull), s_punct = (int64_t)(s12 >> 32);
  const int64_t s_few = x.par.template sum<int64_t>(NLn, [&](uint32_t k) { return (int64_t)(code[k] == 3); });
  x.stamp(PH_C4_CODES);
  // ---- joined kept lines (HBM: read back by pass B), copied from Pb ----
  uint32_t* joff = x.template alloc_hot<uint32_t>(NLn + 1);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return true; }
  uint32_t Jtot = x.par.template scan<uint32_t>(
      NLn, 0u, [](uint32_t a, uint32_t b2) { return a + b2; },
      [&](uint32_t k) { return code[k] == 0 ? plen[k] + 1 : 0u; }, [&](uint32_t k, uint32_t e) { joff[k] = e; });
  if (Jtot > 0) Jtot -= 1;
  uint8_t* Jb = x.template alloc_global<uint8_t>(Jtot + 1);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return true; }
  x.par.sync();
  x.par.for_n(Ptot, [&](uint32_t i) {
    const uint32_t k = line_of_p(i);
    const uint32_t j = i - poff[k];
    if (code[k] != 0 || j >= plen[k]) return;
    Jb[joff[k] + j] = Pb[i];
  });
  x.par.for_n(NLn, [&](uint32_t k) {
    if (code[k] == 0 && joff[k] + plen[k] < Jtot) Jb[joff[k] + plen[k]] = '\n';
  });
  x.par.sync();
  x.stamp(PH_C4_JOIN);
  c4_finish(x, c4, n, Jb, Jtot, s_long, s_punct, s_few, r, src);
  return true;
}

// `wout` (optional): the rewrite's word count when it comes from the stage's line export (the
// only path a dictionary-script document takes here; kNoWords stays otherwise)
// `hls` (optional): a dictionary-script document's per-line word statistics from the host (ICU,
// text.h dict_c4_lines: [NL, nw_0, mx_0, ...]) in place of segmenting its processed lines here.
template <class P>
TB_HD void c4_pass_a(DocCtx<P>& x, const DevC4& c4, const uint8_t* b, uint32_t n, int64_t* r, int64_t* src,
                     const uint32_t* line_stats = nullptr, uint32_t* wout = nullptr, const uint32_t* hls = nullptr) {
  x.stamp(PH_START);
  const uint32_t scan = c4_byte_scan(x, c4, b, n);
  const bool lorem = scan & C4S_LOREM, curly = scan & C4S_CURLY;
  if (lorem || curly) {
    x.par.single([&]() {
      r[0] = lorem; r[1] = curly; r[2] = r[3] = r[4] = r[5] = 0; r[6] = n;
      src[0] = -1; src[1] = n;
    });
    return;
  }
  x.stamp(PH_C4_LOREM);
  // A citation needs a '[' followed by a digit: without one (the common case) every processed
  // line is its trimmed original line and the plain path runs on the original bytes.
  const bool maybe_cite = c4.remove_citations != 0 && (scan & C4S_CITE);
  if (line_stats && c4.split_paragraph) {
    const uint32_t NL = line_stats[0];  // the stage kernel of this content version wrote it
    if (NL != kLineStatsNone) {
      if (!maybe_cite) {
        c4_pass_a_export(x, c4, b, n, line_stats, NL, r, src, scan, wout);
        return;
      }
      // (documents with host line statistics, i.e. dictionary-script lines, take the general
      // path, which has the ICU statistics of every processed line; workgroup documents too:
      // k_c4_pass_a_blk 1.09 -> 0.57 ms/step, profiles/r10_ab_citeblk)
      if (!hls && NL > 0 && c4_pass_a_cite_export(x, c4, b, n, line_stats, NL, r, src)) return;
    }
  }
  uint32_t dict = 0;
  Cps c = decode(x, b, n, false, &dict);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  x.stamp(PH_C4_DECODE);
  const uint32_t C = c.n;
  const PropArr prop = c.props();
  const OffArr off = c.offs();
  if (!dict) hls = nullptr;
  if (dict && (!hls || !c4.split_paragraph)) {
    x.set_flag(DOC_NEEDS_CPU);
    return;
  }
  // ---- line spans [la, lb) in code points, trimmed ----
  uint32_t* la = x.template alloc<uint32_t>(C + 1);
  uint32_t* lb = x.template alloc<uint32_t>(C + 1);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  uint32_t NLn = 0;
  if (c4.split_paragraph) {
    Lines L = rust_lines(x, c);
    if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
    NLn = L.n;
    x.par.for_n(NLn, [&](uint32_t k) {
      uint32_t s = L.ls[k], e = L.le[k];
      while (s < e && is_ws(prop[s])) ++s;
      while (e > s && is_ws(prop[e - 1])) --e;
      la[k] = s;
      lb[k] = e;
    });
  } else {
    uint32_t tcs, tce;
    trim_span(x, prop, C, tcs, tce);
    if (tcs < tce) {
      const uint32_t m = tce - tcs;
      uint32_t* st = x.template alloc<uint32_t>(m + 1);
      if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
      CpsAcc acc{prop + tcs};
      const uint32_t NS = x.par.template compact<int>(
          m, [&](uint32_t i, int&) { return i == 0 || sb_break(acc, (int)m, (int)i); },
          [&](uint32_t i, uint32_t k, int&) { st[k] = i; });
      x.par.sync();
      struct SS { uint32_t s, e; };
      NLn = x.par.template compact<SS>(
          NS,
          [&](uint32_t k, SS& ss) {
            uint32_t s = tcs + st[k], e = tcs + (k + 1 < NS ? st[k + 1] : m);
            while (s < e && is_ws(prop[s])) ++s;
            while (e > s && is_ws(prop[e - 1])) --e;
            ss.s = s;
            ss.e = e;
            return s < e;
          },
          [&](uint32_t, uint32_t q, SS& ss) { la[q] = ss.s; lb[q] = ss.e; });
    }
  }
  x.par.sync();
  x.stamp(PH_C4_LINES);
  if (hls && hls[0] != NLn) {  // (never: the host splits the same Rust lines)
    x.set_flag(DOC_NEEDS_CPU);
    return;
  }
  if (!maybe_cite && !hls) {
    c4_pass_a_plain(x, c4, b, n, c, la, lb, NLn, r, src, scan);
    return;
  }
  // ---- citation removal -> processed lines Pb (every step parallel over code points) ----
  // lid[j]: the line whose trimmed span holds code point j (kNoLine otherwise), by a max-scan
  // of line-start markers (lines are ordered and disjoint).
  constexpr uint32_t kNoLine = 0xFFFFFFFFu;
  uint32_t* lid = x.template alloc<uint32_t>(C + 1);
  uint32_t* Pw = x.template alloc<uint32_t>(C + 1);   // exclusive prefix of kept bytes
  uint8_t* rm = x.template alloc<uint8_t>(C + 1);     // inside a removed citation
  uint32_t* plen = x.template alloc_hot<uint32_t>(NLn + 1);
  uint32_t* poff = x.template alloc_hot<uint32_t>(NLn + 1);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  x.par.for_n(C, [&](uint32_t j) { lid[j] = 0; rm[j] = 0; });
  x.par.sync();
  x.par.for_n(NLn, [&](uint32_t k) { if (la[k] < lb[k]) lid[la[k]] = k + 1; });
  x.par.sync();
  x.par.template scan<uint32_t>(
      C, 0u, [](uint32_t a, uint32_t b2) { return a > b2 ? a : b2; }, [&](uint32_t j) { return lid[j]; },
      [&](uint32_t j, uint32_t e) {
        const uint32_t cur = e > lid[j] ? e : lid[j];  // inclusive max
        lid[j] = (cur > 0 && j < lb[cur - 1]) ? cur - 1 : kNoLine;
      });
  x.par.sync();
  auto cite_end = [&](uint32_t j, uint32_t e) -> uint32_t {  // cp index past a citation at j, or 0
    if (c.lead(j) != '[') return 0;
    uint32_t p = j + 1;
    if (p >= e || !(prop[p] & P_DIGIT)) return 0;
    while (p < e && (prop[p] & P_DIGIT)) ++p;
    while (p < e && c.lead(p) == ',') {
      uint32_t q = p + 1;
      while (q < e && (prop[q] & P_WS)) ++q;
      if (q < e && (prop[q] & P_DIGIT)) {
        while (q < e && (prop[q] & P_DIGIT)) ++q;
        p = q;
      } else {
        break;
      }
    }
    return (p < e && c.lead(p) == ']') ? p + 1 : 0;
  };
  const bool rmc = c4.remove_citations != 0;
  if (rmc) {
    // a citation holds only digits, commas, whitespace and ']': no '[' inside one, so every
    // '[' can be tested independently (same result as the left-to-right scan)
    x.par.for_n(C, [&](uint32_t j) {
      if (c.lead(j) != '[' || lid[j] == kNoLine) return;
      const uint32_t ce = cite_end(j, lb[lid[j]]);
      for (uint32_t q = j; q < ce; ++q) rm[q] = 1;
    });
    x.par.sync();
  }
  auto kept_bytes = [&](uint32_t j) -> uint32_t {
    return (lid[j] != kNoLine && !rm[j]) ? off[j + 1] - off[j] : 0u;
  };
  const uint32_t Ktot = x.par.template scan<uint32_t>(
      C, 0u, [](uint32_t a, uint32_t b2) { return a + b2; }, kept_bytes, [&](uint32_t j, uint32_t e) { Pw[j] = e; });
  x.par.single([&]() { Pw[C] = Ktot; });
  x.par.sync();
  x.par.for_n(NLn, [&](uint32_t k) {
    plen[k] = Pw[lb[k]] - Pw[la[k]];
    poff[k] = Pw[la[k]] + k;  // kept bytes of the earlier lines + one '\n' per earlier line
  });
  const uint32_t Ptot = Ktot + NLn;
  uint8_t* Pb = x.template alloc<uint8_t>(Ptot + 1);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  x.par.sync();
  x.par.for_n(C, [&](uint32_t j) {
    const uint32_t nb = kept_bytes(j);
    if (!nb) return;
    uint8_t* d = Pb + Pw[j] + lid[j];
    for (uint32_t q = 0; q < nb; ++q) d[q] = b[off[j] + q];
  });
  x.par.for_n(NLn, [&](uint32_t k) { Pb[poff[k] + plen[k]] = '\n'; });
  x.par.single([&]() { poff[NLn] = Ptot; });
  // Pb is read next (decode tests its bytes without a barrier of its own): in the workgroup kernel
  // a wave would otherwise segment bytes another wave has not written yet - whatever the scratch
  // slice held before - and lose or split the words of a line
  x.par.sync();
  x.stamp(PH_C4_CITE);
  // ---- words of the processed lines ----
  uint32_t* nw = nullptr;
  uint32_t* mx = nullptr;
  uint32_t* pf = nullptr;  // pattern flags per line
  uint8_t* code = nullptr;
  auto line_arrays = [&]() {
    nw = x.template alloc_hot<uint32_t>(NLn + 1);
    mx = x.template alloc_hot<uint32_t>(NLn + 1);
    pf = x.template alloc_hot<uint32_t>(NLn + 1);
    code = x.template alloc_hot<uint8_t>(NLn + 1);
    if (x.overflow) return false;
    x.par.for_n(NLn, [&](uint32_t k) { nw[k] = 0; mx[k] = 0; pf[k] = 0; code[k] = 0; });
    x.par.sync();
    return true;
  };
  auto line_of_byte = [&](uint32_t bs) {  // last line with poff <= bs
    uint32_t lo = 0, hi = NLn;
    while (hi - lo > 1) {
      uint32_t mid = (lo + hi) >> 1;
      if (poff[mid] <= bs) lo = mid; else hi = mid;
    }
    return lo;
  };
  // (one-wave documents only: in the workgroup kernel the per-byte line lookups of the cited-line
  // copy cost more than segmenting the whole processed text, measured)
  const bool from_export = P::kWaves == 1 && line_stats && c4.split_paragraph && NLn > 0 && line_stats[0] == NLn;
  if (hls) {
    if (!line_arrays()) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
    x.par.for_n(NLn, [&](uint32_t k) { nw[k] = hls[1 + 2 * k]; mx[k] = hls[2 + 2 * k]; });
    x.par.sync();
  } else if (from_export) {
    if (!line_arrays()) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
    // Lines that lost no citation are their trimmed original lines: their counts come from the
    // stage's line export. Only the processed text of the lines that lost one (code[k] = 1 marks
    // them here) is segmented, joined with '\n' so that no word spans two lines.
    const LineStat* ls = (const LineStat*)(line_stats + 4);
    x.par.for_n(C, [&](uint32_t j) { if (rm[j] && lid[j] != kNoLine) code[lid[j]] = 1; });
    x.par.sync();
    uint32_t* coff = x.template alloc_hot<uint32_t>(NLn + 1);
    if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
    const uint32_t Ctot = x.par.template scan<uint32_t>(
        NLn, 0u, [](uint32_t a, uint32_t b2) { return a + b2; },
        [&](uint32_t k) { return code[k] ? plen[k] + 1 : 0u; }, [&](uint32_t k, uint32_t e) { coff[k] = e; });
    x.par.for_n(NLn, [&](uint32_t k) {
      if (!code[k]) { nw[k] = ls[k].nw; mx[k] = ls[k].mx; }
    });
    x.par.sync();
    if (Ctot > 0) {
      const auto mc = x.mark();
      uint8_t* Pc = x.template alloc<uint8_t>(Ctot + 1);
      if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
      x.par.for_n(Ptot, [&](uint32_t i) {
        const uint32_t k = line_of_byte(i);
        if (code[k] && i - poff[k] <= plen[k]) Pc[coff[k] + (i - poff[k])] = Pb[i];  // (its '\n' too)
      });
      x.par.sync();
      Cps cc = decode(x, Pc, Ctot);
      Words cw = words(x, cc);
      if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
      x.par.for_n(cw.n, [&](uint32_t q) {
        const uint32_t bs = cw.bs[q];
        uint32_t lo = 0, hi = NLn;  // last line with coff <= bs: the cited line holding the word
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) >> 1;
          if (coff[mid] <= bs) lo = mid; else hi = mid;
        }
        P::add32(&nw[lo], 1u);
        P::max32(&mx[lo], cw.ce[q] - cw.cs[q]);
      });
      x.par.sync();
      x.reset(mc);
    }
  } else {
    Cps pc = decode(x, Pb, Ptot);
    Words pwd = words(x, pc);
    if (!line_arrays() || x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
    x.par.for_n(pwd.n, [&](uint32_t q) {
      const uint32_t lo = line_of_byte(pwd.bs[q]);
      P::add32(&nw[lo], 1u);
      P::max32(&mx[lo], pwd.ce[q] - pwd.cs[q]);
    });
  }
  x.stamp(PH_C4_WORDS);
  // javascript / policy phrases: to_lowercase().contains() per line == a case-folded match
  // starting at some byte of the line; every byte position is tested in parallel.
  if (c4.filter_javascript || c4.filter_policy) {
    // The phrases hold letters and spaces only, so a match never runs over the '\n' that ends
    // its line: match against the rest of Pb first, look the line up only on a match.
    scan_bytes16(x, Pb, Ptot, [&](uint32_t s, uint32_t, uint32_t, uint64_t lw) {
      if (!c4_phrase_prefix(lw)) return;
      const uint32_t bits = c4_phrases_at(c4, Pb, Ptot, s, lw);
      if (bits) P::or32(&pf[line_of_byte(s)], bits);
    });
  }
  x.par.sync();
  x.par.for_n(NLn, [&](uint32_t k) {
    const uint8_t* lp = Pb + poff[k];
    const uint32_t ln = plen[k];
    uint8_t cd = 0;
    if (c4.max_word_length > 0 && (int64_t)mx[k] > c4.max_word_length) {
      cd = 1;
    } else if (c4.filter_no_terminal_punct) {
      bool term = false;
      if (ln > 0) {
        uint32_t st = ln - 1;
        while (st > 0 && (lp[st] & 0xC0) == 0x80) --st;
        int len;
        term = end_punct(utf8_decode(lp, st, ln, &len));
      }
      const bool ell = ln >= 3 && lp[ln - 1] == '.' && lp[ln - 2] == '.' && lp[ln - 3] == '.';
      if (!term || ell) cd = 2;
    }
    if (cd == 0 && c4.min_words_per_line > 0 && (int64_t)nw[k] < c4.min_words_per_line) cd = 3;
    if (cd == 0 && c4.filter_javascript && (pf[k] & C4F_JS)) cd = 4;
    if (cd == 0 && c4.filter_policy && (pf[k] & C4F_POLICY)) cd = 5;
    code[k] = cd;
  });
  x.par.sync();
  const int64_t s_long = x.par.template sum<int64_t>(NLn, [&](uint32_t k) { return (int64_t)(code[k] == 1); });
  const int64_t s_punct = x.par.template sum<int64_t>(NLn, [&](uint32_t k) { return (int64_t)(code[k] == 2); });
  const int64_t s_few = x.par.template sum<int64_t>(NLn, [&](uint32_t k) { return (int64_t)(code[k] == 3); });
  if (wout && hls) {  // words of the rewrite: the kept lines' (see c4_plain_tail)
    const uint32_t wk = x.par.template sum<uint32_t>(NLn, [&](uint32_t k) { return code[k] == 0 ? nw[k] : 0u; });
    x.par.single([&]() { *wout = wk; });
  }
  x.stamp(PH_C4_CODES);
  // ---- joined kept lines (HBM: read back by pass B), scattered per code point ----
  uint32_t* joff = x.template alloc_hot<uint32_t>(NLn + 1);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  uint32_t Jtot = x.par.template scan<uint32_t>(
      NLn, 0u, [](uint32_t a, uint32_t b2) { return a + b2; },
      [&](uint32_t k) { return code[k] == 0 ? plen[k] + 1 : 0u; }, [&](uint32_t k, uint32_t e) { joff[k] = e; });
  if (Jtot > 0) Jtot -= 1;
  uint8_t* Jb = x.template alloc_global<uint8_t>(Jtot + 1);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  x.par.sync();
  x.par.for_n(C, [&](uint32_t j) {
    const uint32_t nb = kept_bytes(j);
    if (!nb || code[lid[j]] != 0) return;
    const uint32_t k = lid[j];
    uint8_t* d = Jb + joff[k] + (Pw[j] - Pw[la[k]]);
    for (uint32_t q = 0; q < nb; ++q) d[q] = b[off[j] + q];
  });
  x.par.for_n(NLn, [&](uint32_t k) {
    if (code[k] == 0 && joff[k] + plen[k] < Jtot) Jb[joff[k] + plen[k]] = '\n';
  });
  x.par.sync();
  x.stamp(PH_C4_JOIN);
  c4_finish(x, c4, n, Jb, Jtot, s_long, s_punct, s_few, r, src);
}

}  // namespace tb
