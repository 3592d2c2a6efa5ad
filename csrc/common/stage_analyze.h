// Stage analysis for one content version: writes the records of every step of the stage.
#pragma once
#include "devplan.h"
#include "doc_dedup.h"
#include "doc_langid.h"
#include "doc_text.h"
#include "gopher_rep.h"

namespace tb {

// Lowercase (Rust str::to_lowercase on the word) hashed on the fly; optionally compared to `ref`.
template <class F>
TB_HD void lower_bytes(const UcdView& ucd, const Cps& cv, uint32_t s, uint32_t e, F&& push) {
  uint8_t buf[4];
  const PropArr prop = cv.props();
  for (uint32_t k = s; k < e; ++k) {
    uint32_t c = cv.cp(k);
    uint32_t lc;
    if (c == 0x3A3) {
      bool before = false, after = false;
      for (uint32_t j = k; j > s; --j) {
        uint32_t p = prop[j - 1];
        if (p & P16_CASE_IGN) continue;
        before = (p & P_CASED) != 0;
        break;
      }
      for (uint32_t j = k + 1; j < e; ++j) {
        uint32_t p = prop[j];
        if (p & P16_CASE_IGN) continue;
        after = (p & P_CASED) != 0;
        break;
      }
      lc = (before && !after) ? 0x3C2 : 0x3C3;
    } else {
      lc = ucd.lower(c);
    }
    int nb = utf8_encode(lc, buf);
    for (int q = 0; q < nb; ++q) push(buf[q]);
    if (c == 0x130) { push(0xCC); push(0x87); }
  }
}

// [s, e): the word's code points, [b0, b1): its bytes (Words::bs / be: no offset loads)
TB_HD bool is_stop_word(const UcdView& ucd, const DevStopSet& ss, const Cps& cv, uint32_t s, uint32_t e,
                        uint32_t b0, uint32_t b1) {
  // every code point lowercases to at least one byte
  if (ss.n == 0 || (int32_t)(e - s) > ss.max_len) return false;
  if (ss.lite_nslots > 0) {
    // ASCII word of <= 7 bytes (as many bytes as code points): its lowercase bytes are the key
    // of the set's fast table, which holds every ASCII entry of <= 7 bytes (devplan.h)
    const uint32_t nb = b1 - b0;
    if (nb <= 7u && nb == e - s) {
      uint64_t key = (uint64_t)nb << 56;
      for (uint32_t k = 0; k < nb; ++k) {
        uint32_t c = cv.b[b0 + k];
        if (c >= 'A' && c <= 'Z') c += 32;
        key |= (uint64_t)c << (8 * k);
      }
      const uint32_t ns = (uint32_t)ss.lite_nslots;
      uint32_t slot = stop_fast_slot(key, ns);
      while (true) {
        const uint64_t f = ss.fast_keys[slot];
        if (f == 0) return false;
        if (f == key) return true;
        slot = (slot + 1) & (ns - 1);
      }
    }
    if (ss.all_ascii7) {  // (devplan.h) no lowercase of this word is in the set without a Kelvin sign
      bool e2 = false;
      for (uint32_t k = b0; k < b1; ++k) e2 |= cv.b[k] == 0xE2;
      if (!e2) return false;
    }
  }
  uint64_t h = 0;
  uint32_t len = 0;
  lower_bytes(ucd, cv, s, e, [&](uint8_t v) { h = hash_push(h, v); ++len; });
  const uint64_t key = dev_key(h, len);
  uint32_t slot = (uint32_t)(key >> 17) & (kStopTableSize - 1);
  while (true) {
    const uint64_t k = ss.keys[slot];
    if (k == 0) return false;
    if (k == key) break;
    slot = (slot + 1) & (kStopTableSize - 1);
  }
  // An entry with this key and other bytes is not the answer: another entry with the same key may
  // follow it on the probe chain (add_stop_set puts it in the next free slot). Only the slot stays
  // live across the comparison: the key is read back from it, the length test is the walk's end.
  while (true) {
    const int32_t w = ss.idx[slot];
    const int32_t o1 = ss.off[w + 1];
    int32_t pos = ss.off[w];
    bool ok = true;
    lower_bytes(ucd, cv, s, e, [&](uint8_t v) {
      ok = ok && pos < o1 && ss.blob[pos] == v;
      ++pos;
    });
    if (ok && pos == o1) return true;
    const uint64_t same = ss.keys[slot];
    uint64_t k;
    do {
      slot = (slot + 1) & (kStopTableSize - 1);
      k = ss.keys[slot];
      if (k == 0) return false;
    } while (k != same);
  }
}

struct StageOut {
  int64_t* rec;     // record buffer (all steps of the stage)
  uint32_t ndocs;
  uint32_t doc;
  GrExport* gr_export = nullptr;  // non-null: split mode for this document (see GrExport)
  // non-null: this document's C4 line export (LineStat region, see export_line_stats), for the C4
  // pass of the same content version
  uint32_t* line_stats = nullptr;
  const PreDoc* pre = nullptr;  // non-null: decode and word-break marks were precomputed
  // the document's bytes in HBM (split mode exports them: the stage may read an LDS copy)
  const uint8_t* b_global = nullptr;
  // dictionary-script documents: where their words come from (DictIn)
  DictIn dict;
};

// C4 line export from the stage's words and lines (StageOut::line_stats): per Rust line its span
// trimmed of whitespace (in bytes), its word count and its longest word in code points. Words are
// assigned to the last line starting at or before their first code point (words never cross a
// line feed), word-parallel with LDS atomics on per-line counters. The header is written last;
// documents with more lines than the region holds, or whose counters do not fit the scratch,
// keep kLineStatsNone (the export never changes the stage's own results).
template <class P>
TB_HD void export_line_stats(DocCtx<P>& x, const Cps& c, const Words& w, const Lines& L, uint32_t n, uint32_t* out) {
  const uint32_t NL = L.n;
  if (NL > line_stats_cap(n) || x.overflow) return;
  const auto mark = x.mark();
  uint32_t* ls = x.template alloc_hot<uint32_t>(NL + 1);
  uint32_t* nw = x.template alloc_hot<uint32_t>(NL + 1);
  uint32_t* mx = x.template alloc_hot<uint32_t>(NL + 1);
  if (x.overflow) {
    x.overflow = false;
    x.reset(mark);
    return;
  }
  const PropArr prop = c.props();
  const OffArr off = c.offs();
  x.par.for_n(NL, [&](uint32_t k) { ls[k] = L.ls[k]; nw[k] = 0; mx[k] = 0; });
  x.par.sync();
  x.par.for_n(w.n, [&](uint32_t q) {
    const uint32_t cs = w.cs[q];
    uint32_t lo = 0, hi = NL;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (ls[mid] <= cs) lo = mid; else hi = mid;
    }
    P::add32(&nw[lo], 1u);
    P::max32(&mx[lo], w.ce[q] - cs);
  });
  x.par.sync();
  LineStat* st = (LineStat*)(out + 4);
  x.par.for_n(NL, [&](uint32_t k) {
    uint32_t s0 = ls[k], e0 = L.le[k];
    while (s0 < e0 && is_ws(prop[s0])) ++s0;
    while (e0 > s0 && is_ws(prop[e0 - 1])) --e0;
    st[k] = LineStat{off[s0], off[e0], nw[k], mx[k]};
  });
  x.par.sync();
  x.par.single([&]() { out[0] = NL; });
  x.reset(mark);
}

// GopherQuality's byte counts of b[0, n): '#' bytes (high half) and ellipses (low half: every
// U+2026 plus len / 3 for each maximal run of '.'). Items are groups of four aligned dwords (one
// dword of look-behind and one of look-ahead, issued together); a dword without '.' or 0xE2 costs
// three SWAR compares and a popcount. Same counts as the per-byte definition.
template <class P>
TB_HD uint64_t gq_byte_counts(DocCtx<P>& x, const uint8_t* b, uint32_t n) {
  const uintptr_t a0 = (uintptr_t)b & ~(uintptr_t)3;
  const uint32_t head = (uint32_t)((uintptr_t)b - a0);
  const uint32_t nd = (head + n + 3) >> 2;
  const uint32_t* w = (const uint32_t*)a0;
  auto dw = [&](int64_t k) -> uint32_t {  // dword k of the aligned stream, bytes outside the text zero
    if (k < 0 || k >= (int64_t)nd) return 0u;
    const int64_t e = 4 * k + 4 - head;
    if (e <= (int64_t)n && 4 * k >= (int64_t)head) return w[k];
    uint32_t v = 0;
    for (uint32_t j = 0; j < 4; ++j) {
      const int64_t sj = 4 * k + j - head;
      if (sj >= 0 && sj < (int64_t)n) v |= (uint32_t)b[sj] << (8 * j);
    }
    return v;
  };
  return x.par.template sum<uint64_t>((nd + 3) >> 2, [&](uint32_t g) {
    uint32_t d[6];  // d[0]: dword 4g - 1, d[1..4]: the group, d[5]: dword 4g + 4
#pragma unroll
    for (uint32_t i = 0; i < 6; ++i) d[i] = dw((int64_t)4 * g + i - 1);
    uint64_t acc = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
      const uint32_t v = d[i + 1];
      acc += (uint64_t)__builtin_popcount(swar_eq_mask(v, '#')) << 32;
      const uint32_t dots = swar_eq_mask(v, '.'), e2 = swar_eq_mask(v, 0xE2);
      if ((dots | e2) == 0) continue;
      const uint64_t v64 = (uint64_t)v | ((uint64_t)d[i + 2] << 32);
      for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t c0 = (v >> (8 * r)) & 0xFFu;
        if (c0 == 0xE2) {
          acc += ((v64 >> (8 * r + 8)) & 0xFFFFu) == 0xA680u ? 1u : 0u;
          continue;
        }
        if (c0 != '.') continue;
        const uint32_t prev = r ? (v >> (8 * r - 8)) & 0xFFu : d[i] >> 24;
        if (prev == '.') continue;  // not the start of its run
        uint32_t len = 1;
        while (r + len < 8 && ((v64 >> (8 * (r + len))) & 0xFFu) == '.') ++len;
        if (r + len == 8) {  // the run goes past the window: the rest byte by byte
          int64_t j = 4 * ((int64_t)4 * g + i) + r + len - head;
          while (j < (int64_t)n && b[j] == '.') { ++j; ++len; }
        }
        acc += len / 3;
      }
    }
    return acc;
  });
}

// kPre: the document comes with its pre-pass (StageOut::pre: code points, words, runs of '\n');
// a separate instantiation, so the common kernel carries no branch for it (a runtime branch
// doubled the workgroup kernel's register spill).
// kExport: the one-wave build for launches in split mode (gopher_rep_record): no in-stage n-gram
// code and no prefix hash, which nothing reads there.
template <class P, bool kWithLid = true, bool kPre = false, bool kExport = false>
TB_HD void analyze_stage(DocCtx<P>& x, const DevStage& st, const DevPlan& plan,
                         const LidTables& lid, const uint8_t* b, uint32_t n, StageOut& out) {
  bool need_words = false, need_lines = false, need_ph = false, need_lid = false;
  for (int s = 0; s < st.n_steps; ++s) {
    const int k = st.steps[s].kind;
    if (k == DK_GOPHER_QUALITY) need_words = need_lines = true;
    if (k == DK_GOPHER_REP) need_words = need_ph = true;
    if (k == DK_FINEWEB) need_words = need_lines = need_ph = true;
    if (k == DK_LANGID) need_lid = true;
  }
  if constexpr (P::kWaves == 1) {
    // One-wave documents: dup_spans (duplicated lines and paragraphs, FineWeb's duplicated lines)
    // compares the spans themselves, so the prefix hashes have one reader left, the word hashes of
    // a GopherRepetition step whose n-gram orders run in this kernel: not exported to the n-gram
    // kernels, because split mode is off or the stage has two such steps.
    int n_gr = 0;
    bool gr_ngrams = false;
    for (int s = 0; s < st.n_steps; ++s) {
      if (st.steps[s].kind != DK_GOPHER_REP) continue;
      ++n_gr;
      gr_ngrams |= st.steps[s].n_top + st.steps[s].n_dup > 0;
    }
    need_ph = !kExport && gr_ngrams && !(n_gr == 1 && out.gr_export);
  }
  x.stamp(PH_START);
  if (out.line_stats) x.par.single([&]() { out.line_stats[0] = kLineStatsNone; });
  uint32_t ndict = 0;
  Cps c;
  if constexpr (kPre) {
    c.n = out.pre->C;
    c.off = out.pre->off;
    c.prop = out.pre->prop;
    c.b = b;
    c.nb = n;
    ndict = out.pre->dict;
  } else {
    c = decode(x, b, n, true, &ndict);
  }
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  x.stamp(PH_DECODE);
  const uint32_t C = c.n;
  // Dictionary-script documents: their words come from the host's ICU segmentation (the word
  // marks of the original text), or — for a stage after C4 whose only word reader is FineWeb,
  // which needs just the count — from the word count C4 pass A left for the rewrite. Otherwise
  // (no marks, GopherQuality / GopherRepetition on a rewritten version, a pre-pass document) the
  // document goes to the ICU path (host) and is recomputed there, so nothing else is analysed
  // here. The language record needs no segmentation and is exact for every script (the device
  // computes it in its own kernel, and a document the language gate filters is not delegated),
  // so the emulation still produces it.
  // wfix: the word count a count-only document's FineWeb record takes (kNoWords: none); it is
  // applied after the steps, so no branch on it sits in the analysis (a branch there made the
  // compiler duplicate the step loop: 4x the register spills)
  const uint32_t* dict_marks = nullptr;
  uint32_t wfix = kNoWords;
  if (ndict && need_words) {  // (a stage without word segmentation reads no script-dependent data)
    bool fw_only = true;
    for (int s = 0; s < st.n_steps; ++s)
      fw_only &= st.steps[s].kind != DK_GOPHER_QUALITY && st.steps[s].kind != DK_GOPHER_REP;
    if (!kPre) dict_marks = out.dict.marks(out.doc);
    if (!kPre && !dict_marks && fw_only) wfix = out.dict.nwords(out.doc);
    if (!dict_marks && wfix == kNoWords) {
      if constexpr (kWithLid) {
        for (int s = 0; s < st.n_steps; ++s) {
          const DevStep& ds = st.steps[s];
          if (ds.kind == DK_LANGID && lid.E)
            langid_record(x, b, n, lid, out.rec + (int64_t)ds.rec_prefix * out.ndocs + (int64_t)out.doc * ds.width);
        }
      }
      x.set_flag(DOC_NEEDS_CPU);
      return;
    }
  }
  x.stamp(PH_DICT);
  PHView ph;
  if constexpr (!kExport) {
    if (need_ph) ph = prefix_hash8(x, b, n);
  }
  x.stamp(PH_PREFIX_HASH);
  Words w;
  if (need_words) {
    w = words(x, c, kPre ? out.pre : nullptr, dict_marks);
  }
  x.stamp(PH_WORDS);
  Lines L;
  if (need_lines) L = rust_lines(x, c);
  if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  x.stamp(PH_RUST_LINES);
  if (out.line_stats && need_words && need_lines) export_line_stats(x, c, w, L, n, out.line_stats);
  x.stamp(PH_LINES);
  const uint32_t W = w.n;
  const PropArr prop = c.props();
  const OffArr off = c.offs();

  // Records are independent: GopherRepetition runs after the other steps so that its n-gram
  // phase (the last user of the code point properties) can hand their LDS to its hash tables.
  int n_gr = 0;
  for (int s = 0; s < st.n_steps; ++s) n_gr += st.steps[s].kind == DK_GOPHER_REP;
  int gr_seen = 0;
  for (int so = 0; so < 2 * st.n_steps; ++so) {
    const int s = so % st.n_steps;
    const DevStep& ds = st.steps[s];
    if ((so < st.n_steps) == (ds.kind == DK_GOPHER_REP)) continue;
    int64_t* r = out.rec + (int64_t)ds.rec_prefix * out.ndocs + (int64_t)out.doc * ds.width;
    if (ds.kind == DK_GOPHER_QUALITY) {
      const DevStopSet& ss = plan.stops[ds.stop_set];
      const UcdView ucd = x.ucd;
      // Counts are packed two per 64-bit sum (each < 2^32: a document is < 4 GiB), so the seven
      // statistics take one pass over the words, one over the code points and one over the lines.
      auto lo32 = [](uint64_t v) { return (int64_t)(v & 0xFFFFFFFFull); };
      auto hi32 = [](uint64_t v) { return (int64_t)(v >> 32); };
      int64_t sum_chars = 0;
      const uint64_t as = x.par.template sum<uint64_t>(W, [&](uint32_t k) {
        const uint32_t a = w.cs[k], e = w.ce[k];
        return ((uint64_t)(e - a) << 32) | ((uint64_t)w.alpha[k] << 16) |
               (uint64_t)is_stop_word(ucd, ss, c, a, e, w.bs[k], w.be[k]);
      });
      // fields: chars (bits 32..63, <= C), alphabetic words (16..31) and stop words (0..15), both
      // <= W; documents with 2^16 words or more are counted field by field
      int64_t alpha, stop;
      if (W < 65536u) {
        sum_chars = hi32(as);
        alpha = (int64_t)((as >> 16) & 0xFFFFull);
        stop = (int64_t)(as & 0xFFFFull);
      } else {
        sum_chars = x.par.template sum<int64_t>(W, [&](uint32_t k) { return (int64_t)(w.ce[k] - w.cs[k]); });
        alpha = x.par.template sum<int64_t>(W, [&](uint32_t k) { return (int64_t)w.alpha[k]; });
        stop = x.par.template sum<int64_t>(W, [&](uint32_t k) {
          return (int64_t)is_stop_word(ucd, ss, c, w.cs[k], w.ce[k], w.bs[k], w.be[k]);
        });
      }
      x.stamp(PH_GQ_WORDS);
      // the same counts over the bytes ('#' and '.' are ASCII, U+2026 is E2 80 A6 and E2 is
      // always a lead byte): no code point offset loads, four bytes per SWAR test
      // (workgroup documents: the per-byte form, the SWAR groups cost their kernels ~50 spilled VGPRs)
      const uint64_t he = P::kWaves <= 1 ? gq_byte_counts(x, b, n) : x.par.template sum<uint64_t>(n, [&](uint32_t i) {
        const uint32_t c0 = b[i];
        if (c0 == '#') return (uint64_t)1 << 32;
        if (c0 == 0xE2) return (uint64_t)(i + 2 < n && b[i + 1] == 0x80 && b[i + 2] == 0xA6);
        if (c0 != '.' || (i > 0 && b[i - 1] == '.')) return (uint64_t)0;
        uint32_t j = i;
        while (j < n && b[j] == '.') ++j;
        return (uint64_t)((j - i) / 3);
      });
      x.stamp(PH_GQ_BYTES);
      const int64_t nhash = hi32(he), nell = lo32(he);
      const uint64_t be = x.par.template sum<uint64_t>(L.n, [&](uint32_t k) {
        const uint32_t ls = L.ls[k], le = L.le[k];
        uint32_t j = ls;
        while (j < le && is_ws(prop[j])) ++j;
        const uint32_t l0 = j < le ? c.lead(j) : 0u;
        const uint64_t bul = (l0 == '-' || (l0 == 0xE2 && c.cp(j) == 0x2022)) ? 1 : 0;
        j = le;
        while (j > ls && is_ws(prop[j - 1])) --j;
        const uint32_t E = off[j], S = off[ls];
        uint64_t ell = 0;
        if (E - S >= 3) {
          const bool dots = b[E - 3] == '.' && b[E - 2] == '.' && b[E - 1] == '.';
          const bool uell = b[E - 3] == 0xE2 && b[E - 2] == 0x80 && b[E - 1] == 0xA6;
          ell = (dots || uell) ? 1 : 0;
        }
        return (bul << 32) | ell;
      });
      const int64_t bullet = hi32(be), ell_lines = lo32(be);
      x.par.single([&]() {
        r[0] = W; r[1] = sum_chars; r[2] = nhash; r[3] = nell; r[4] = L.n;
        r[5] = bullet; r[6] = ell_lines; r[7] = alpha; r[8] = stop;
      });
      x.stamp(PH_GQ);
    } else if (ds.kind == DK_GOPHER_REP) {
      ++gr_seen;
      gopher_rep_record<P, kExport>(x, ds, b, c, ph, w, r, gr_seen == n_gr,
                                    n_gr == 1 ? out.gr_export : nullptr, kPre ? out.pre : nullptr, out.b_global, L);
    } else if (ds.kind == DK_FINEWEB) {
      const auto mark = x.mark();
      uint32_t* nb = x.template alloc<uint32_t>(L.n + 1);
      if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
      const uint32_t NB = x.par.template compact<int>(
          L.n,
          [&](uint32_t k, int&) {
            for (uint32_t j = L.ls[k]; j < L.le[k]; ++j) if (!is_ws(prop[j])) return true;
            return false;
          },
          [&](uint32_t k, uint32_t q, int&) { nb[q] = k; });
      x.par.sync();
      int64_t stop_end = x.par.template sum<int64_t>(NB, [&](uint32_t q) {
        uint32_t k = nb[q];
        uint32_t j = L.le[k];
        while (j > L.ls[k] && is_ws(prop[j - 1])) --j;
        uint32_t last = c.cp(j - 1);
        for (int t = 0; t < ds.n_stop_chars; ++t) if (ds.stop_chars[t] == last) return (int64_t)1;
        return (int64_t)0;
      });
      int64_t shrt = x.par.template sum<int64_t>(NB, [&](uint32_t q) {
        uint32_t k = nb[q];
        return (int64_t)((int64_t)(L.le[k] - L.ls[k]) <= ds.short_line_length);
      });
      int64_t dup_e = 0, dup_b = 0;
      dup_spans(x, b, ph, NB,
                [&](uint32_t q, uint32_t& s0, uint32_t& e0) { s0 = off[L.ls[nb[q]]]; e0 = off[L.le[nb[q]]]; },
                &dup_e, &dup_b);
      int64_t nl = x.par.template sum<int64_t>(C, [&](uint32_t i) { return (int64_t)c.is_lf(i); });
      x.par.single([&]() {
        r[0] = NB; r[1] = stop_end; r[2] = shrt; r[3] = dup_b; r[4] = (int64_t)C - nl; r[5] = nl; r[6] = W;
      });
      x.reset(mark);
      x.stamp(PH_FW);
    } else if (ds.kind == DK_LANGID) {
      // on the device this runs as a separate kernel (k_langid_mfma): lid.E == nullptr
      if constexpr (kWithLid)
        if (lid.E) langid_record(x, b, n, lid, r);
      x.stamp(PH_LID);
    }
    if (x.overflow) { x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW); return; }
  }
  if (wfix != kNoWords) {
    // a count-only document (dictionary script, FineWeb after C4): its words were segmented by the
    // rules above; FineWeb's word count is C4's ICU-based one, and its line export is withdrawn
    x.par.sync();
    x.par.single([&]() {
      for (int s = 0; s < st.n_steps; ++s) {
        const DevStep& ds = st.steps[s];
        if (ds.kind == DK_FINEWEB) out.rec[(int64_t)ds.rec_prefix * out.ndocs + (int64_t)out.doc * ds.width + 6] = wfix;
      }
      if (out.line_stats) out.line_stats[0] = kLineStatsNone;
    });
  }
}

}  // namespace tb
