// GopherRepetitionFilter: the in-stage record, its export, the split and n-gram kernels' orders.
#pragma once
#include <type_traits>
#include "devplan.h"
#include "doc_dedup.h"
#include "hash.h"

namespace tb {

// Wave documents with fewer words than this keep n-gram canonical ids in 16 bits (every
// canonicalisation slot index < 1.5 n + 2 fits); more words send the document to the CPU path.
constexpr uint32_t kWave16 = 43000;
TB_HD constexpr int rec_gr_fixed() { return 7; }

// SURVEY 5.7 intra-document split (documents over TB_SPLIT_DOC_BYTES): the stage workgroup
// computes everything except the duplicated n-gram orders and exports the per-word arrays those
// need (all in the document's HBM scratch slice); then one workgroup per (document, order) —
// k_gr_dup_split — canonicalises its order, marks repeats and runs its greedy walk, in parallel.
// One-wave documents export W, bs, be, b, free_base / free_cap and valid only (wid, WL, K, PB stay
// null): the n-gram kernels build their own word arrays on chip, and k_gr_words fills the four
// in for the documents that take the generic per-order code.
struct GrExport {
  const uint32_t* wid;   // canonical word ids
  const uint32_t* WL;    // byte prefix of word lengths
  const uint64_t* K;     // concatenation hash prefixes (see gopher_rep_record)
  const uint64_t* PB;    // B^WL
  const uint32_t* bs;    // word byte starts / ends
  const uint32_t* be;
  const uint8_t* b;      // document bytes
  char* free_base;       // unused rest of the document's scratch slice
  uint64_t free_cap;
  uint32_t W;
  uint32_t valid;        // 1: exported (0: the document returned early / was skipped)
  // duplicated lines / paragraphs (lines_valid: their arrays are in HBM and the stage left the
  // four fields to the split kernel): line break runs rs/rl [NR], paragraph breaks prs [NPR]
  // (indices into rs), trimmed code point span [tcs, tce), byte offsets, prefix hashes
  const uint32_t* rs;
  const uint32_t* rl;
  const uint32_t* prs;
  OffArr off;
  PHView ph;
  uint32_t NR, NPR, tcs, tce;
  uint32_t lines_valid;
};

// Line / paragraph spans of gopher_rep_record (byte ranges of the trimmed text between runs of
// '\n'): line k of NR + 1, paragraph q of NPR + 1.
TB_HD void gr_line_span(const uint32_t* rs, const uint32_t* rl, const OffArr& off, uint32_t tcs, uint32_t tce,
                        uint32_t NR, uint32_t k, uint32_t& s0, uint32_t& e0) {
  const uint32_t cs = k == 0 ? tcs : rs[k - 1] + rl[k - 1];
  const uint32_t ce = k == NR ? tce : rs[k];
  s0 = off[cs];
  e0 = off[ce];
}
TB_HD void gr_para_span(const uint32_t* rs, const uint32_t* rl, const uint32_t* prs, const OffArr& off,
                        uint32_t tcs, uint32_t tce, uint32_t NPR, uint32_t q, uint32_t& s0, uint32_t& e0) {
  const uint32_t cs = q == 0 ? tcs : rs[prs[q - 1]] + rl[prs[q - 1]];
  const uint32_t ce = q == NPR ? tce : rs[prs[q]];
  s0 = off[cs];
  e0 = off[ce];
}

// The duplicated n-gram key / equality of order n over the exported word arrays (one definition
// for the in-stage path and the split kernel): grams are equal iff their concatenations are.
struct DupGrams {
  const uint32_t* wid;
  const uint32_t* WL;
  const uint64_t* K;
  const uint64_t* PB;
  const uint32_t* bs;
  const uint32_t* be;
  const uint8_t* b;
  TB_HD uint64_t run_hash(uint32_t p, uint32_t n) const {
    return PB[p + n] * (K[p + n] - K[p]);
  }
  TB_HD uint64_t key(uint32_t p, uint32_t n) const { return dev_key(run_hash(p, n), WL[p + n] - WL[p]); }
  TB_HD bool eq(uint32_t p, uint32_t q, uint32_t n) const {
    if (WL[p + n] - WL[p] != WL[q + n] - WL[q]) return false;
    // same canonical word sequence => same concatenation (the common case); only different word
    // splits of equal-hash text need the byte comparison. All n id pairs are loaded before the
    // compare (no early exit), so the loads overlap instead of forming a dependent chain.
    uint32_t dw = 0;
#pragma unroll 5
    for (uint32_t k = 0; k < n; ++k) dw |= wid[p + k] ^ wid[q + k];
    if (dw == 0) return true;
    uint32_t wp = p, wq = q, bp = bs[p], bq = bs[q];
    const uint32_t L = WL[p + n] - WL[p];
    for (uint32_t i = 0; i < L; ++i) {
      while (bp == be[wp]) { ++wp; bp = bs[wp]; }
      while (bq == be[wq]) { ++wq; bq = bs[wq]; }
      if (b[bp] != b[bq]) return false;
      ++bp;
      ++bq;
    }
    return true;
  }
};

// Greedy duplicated-n-gram walk of one order (reference find_all_duplicate, utils/text.rs:
// 241-259) over canonical gram ids gc[0, G), repeat bitmap R (bit p: gram p occurs more than
// once) and the seen-bitmap sn (zeroed): bytes of the repeated grams the walk counts. A walk only
// stops at repeated grams; at a gram that occurs once it would mark an id nobody else has and
// advance by one, so it jumps from one set bit of R to the next.
template <class GcT>
TB_HD int64_t dup_walk(uint32_t G, uint32_t n, const GcT* gc, const uint32_t* R, uint32_t* sn,
                       const uint32_t* WL) {
  const uint32_t nw = (G + 31) >> 5;
  auto next_rep = [&](uint32_t from) -> uint32_t {  // first repeated position >= from, or G
    if (from >= G) return G;
    uint32_t wi = from >> 5;
    uint32_t bw = R[wi] & (~0u << (from & 31));
    while (!bw) {
      if (++wi >= nw) return G;
      bw = R[wi];
    }
    const uint32_t q = (wi << 5) + (uint32_t)__builtin_ctz(bw);
    return q < G ? q : G;
  };
  int64_t rep = 0;
  uint32_t idx = next_rep(0);
  while (idx < G) {
    const uint32_t g = gc[idx];
    if ((sn[g >> 5] >> (g & 31)) & 1u) {
      rep += (int64_t)(WL[idx + n] - WL[idx]);
      idx = next_rep(idx + n);
    } else {
      sn[g >> 5] |= 1u << (g & 31);
      idx = next_rep(idx + 1);
    }
  }
  return rep;
}

// dup_walk by one whole wave (every lane calls it with the same arguments; the result is
// uniform). The chain of the scalar walk pays a memory round trip per step (gc[idx], seen bit);
// here the wave takes a window of 64 positions starting at the next repeated one, its lanes load
// the window's canonical ids, seen bits and gram lengths together (one round trip per window),
// and the walk steps through the window's repeated positions in scalar registers: a first visit
// marks every lane holding the same id seen (one ballot), a repeat drops the lanes it jumps over.
// The window's first visits then set their seen bits and the counted lanes' lengths are summed.
// Same visits, same result as dup_walk.
template <class P, class GcT>
TB_HD int64_t dup_walk_wave(const P& par, uint32_t G, uint32_t n, const GcT* gc, const uint32_t* R,
                            uint32_t* sn, const uint32_t* WL) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t lane = par.lane;
  const uint32_t nw = (G + 31) >> 5;
  int64_t rep = 0;
  uint32_t idx = 0;
  while (idx < G) {
    uint32_t p0 = G;  // next repeated position >= idx: 64 bitmap words per ballot
    for (uint32_t base = idx >> 5; base < nw; base += 64) {
      const uint32_t w = base + lane;
      uint32_t bw = w < nw ? R[w] : 0u;
      if (w == (idx >> 5)) bw &= ~0u << (idx & 31);
      const uint64_t m = __ballot(bw != 0u);
      if (m) {
        const int l = __builtin_ctzll(m);
        p0 = ((base + (uint32_t)l) << 5) + (uint32_t)__builtin_ctz((uint32_t)__builtin_amdgcn_readlane((int)bw, l));
        break;
      }
    }
    if (p0 >= G) break;
    const uint32_t p = p0 + lane;
    const bool act = p < G && ((R[p >> 5] >> (p & 31)) & 1u);
    uint32_t g = 0xFFFFFFFFu, len = 0;
    if (act) {
      g = gc[p];
      len = WL[p + n] - WL[p];
    }
    const bool seen0 =
        act && ((__hip_atomic_load(&sn[g >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (g & 31)) & 1u);
    uint64_t A = __ballot(act), S = __ballot(seen0), cnt = 0, fv = 0;
    uint32_t next = p0 + 64;
    while (A) {
      const uint32_t k = (uint32_t)__builtin_ctzll(A);
      if ((S >> k) & 1ull) {
        cnt |= 1ull << k;
        const uint32_t j = k + n;
        A = j >= 64 ? 0ull : (A & (~0ull << j));
        if (p0 + j > next) next = p0 + j;
      } else {
        fv |= 1ull << k;
        S |= __ballot(g == (uint32_t)__builtin_amdgcn_readlane((int)g, (int)k));
        A &= A - 1;
      }
    }
    if ((fv >> lane) & 1ull) atomicOr(&sn[g >> 5], 1u << (g & 31));
    uint32_t add = ((cnt >> lane) & 1ull) ? len : 0u;
    for (int o = 32; o > 0; o >>= 1) add += (uint32_t)__shfl_xor((int)add, o);
    rep += add;
    // the next window's seen loads (other lanes) must observe these bits
    // (same wave, same CU: a workgroup-scope fence waits for the atomics; the seen loads read L2)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    idx = next;
  }
  return rep;
#else
  (void)par;
  return dup_walk(G, n, gc, R, sn, WL);
#endif
}

// kExport (one-wave kernel): the build for launches with an export (split mode, one GopherRepetition
// step with n-gram orders): the n-gram kernels compute every order, so the in-stage n-gram code is
// compiled out of it.
template <class P, bool kExport = false>
TB_HD void gopher_rep_record(DocCtx<P>& x, const DevStep& ds, const uint8_t* b, const Cps& c,
                             const PHView& ph, const Words& w, int64_t* r, bool release_props = false,
                             GrExport* ex = nullptr, const PreDoc* pre = nullptr,
                             const uint8_t* b_export = nullptr, Lines lines = Lines{}) {
  const uint32_t C = c.n;
  const PropArr prop = c.props();
  const OffArr off = c.offs();
  const int width = ds.width;
  uint32_t tcs, tce;
  trim_span(x, prop, C, tcs, tce);
  if (tcs >= tce) {
    x.par.single([&]() {
      for (int k = 0; k < width; ++k) r[k] = 0;
      r[0] = -1;
    });
    return;
  }
  const auto mark = x.mark();
  const uint32_t span = tce - tcs;
  uint32_t* rs;
  uint32_t* rl;
  uint32_t NR;
  if (pre) {
    // the pre-pass listed every run of '\n' (position, length): the runs inside [tcs, tce) are
    // a contiguous part of that list (a run starts after a non-'\n' code point, so none at tcs)
    const uint32_t a = pre->nl_a, e = pre->nl_e;  // (k_pre_wb: the runs inside [tcs, tce))
    rs = pre->nl_pos + a;
    rl = pre->nl_len + a;
    NR = e - a;
  } else if (lines.n > 0) {
    // From the stage's Rust lines (`lines`: their starts, ls[k] = one past a '\n' for k >= 1):
    // the line feeds are exactly the code points ls[k] - 1, and a run continues while the next
    // line is empty (ls[k + 1] == ls[k] + 1). The runs inside the trimmed span [tcs, tce) are
    // whole (its ends are not whitespace), and the '\n' a text may end with is outside it. One
    // compaction over the lines instead of one over the code points.
    const uint32_t* ls = lines.ls;
    const uint32_t NL = lines.n;
    // (workgroup documents: HBM, so that split mode can hand them to k_gr_dup_split)
    rs = P::kWaves == 1 ? x.template alloc_hot<uint32_t>(NL + 1) : x.template alloc<uint32_t>(NL + 1);
    rl = P::kWaves == 1 ? x.template alloc_hot<uint32_t>(NL + 1) : x.template alloc<uint32_t>(NL + 1);
    if (x.overflow) return;
    NR = x.par.template compact<int>(
        NL,
        [&](uint32_t k, int&) {
          if (k == 0) return false;
          const uint32_t p = ls[k] - 1;
          return p >= tcs && p < tce && (k == 1 || ls[k - 1] != p);
        },
        [&](uint32_t k, uint32_t q, int&) {
          uint32_t e = k;
          while (e + 1 < NL && ls[e + 1] == ls[e] + 1) ++e;
          rs[q] = ls[k] - 1;
          rl[q] = e - k + 1;
        });
    x.par.sync();
  } else {
    rs = x.template alloc<uint32_t>(span + 1);
    rl = x.template alloc<uint32_t>(span + 1);
    if (x.overflow) return;
    NR = x.par.template compact<int>(
        span,
        [&](uint32_t i, int&) {
          const uint32_t j = tcs + i;
          return c.is_lf(j) && !c.is_lf(j - 1);
        },
        [&](uint32_t i, uint32_t k, int&) {
          uint32_t j = tcs + i, q = j;
          while (c.is_lf(q)) ++q;
          rs[k] = j;
          rl[k] = q - j;
        });
    x.par.sync();
  }
  x.stamp(PH_GR_NL);
  uint32_t* prs = x.template alloc<uint32_t>(NR + 1);
  if (x.overflow) return;
  int64_t line_dup = 0, line_dup_b = 0, para_dup = 0, para_dup_b = 0;
  // split mode: the duplicated line / paragraph statistics go to k_gr_dup_split when everything
  // they read is in HBM (it outlives this kernel)
  // (wave documents never: their split kernels run only the n-gram orders)
  const bool split_lines = ex && P::kWaves != 1 && !x.in_lds(rs) && !x.in_lds(rl) && !x.in_lds(prs) &&
                           !x.in_lds(ph.ph8) && !x.in_lds(c.ent) && !x.in_lds(c.off);
  if (!split_lines)
    dup_spans(x, b, ph, NR + 1,
              [&](uint32_t k, uint32_t& s0, uint32_t& e0) { gr_line_span(rs, rl, off, tcs, tce, NR, k, s0, e0); },
              &line_dup, &line_dup_b);
  x.stamp(PH_GR_LINE_DUP);
  const uint32_t NPR = x.par.template compact<int>(
      NR, [&](uint32_t k, int&) { return rl[k] >= 2; }, [&](uint32_t k, uint32_t q, int&) { prs[q] = k; });
  x.par.sync();
  if (!split_lines)
    dup_spans(x, b, ph, NPR + 1,
              [&](uint32_t q, uint32_t& s0, uint32_t& e0) {
                gr_para_span(rs, rl, prs, off, tcs, tce, NPR, q, s0, e0);
              },
              &para_dup, &para_dup_b);
  if (ex) {
    x.par.single([&]() {
      ex->rs = rs; ex->rl = rl; ex->prs = prs; ex->off = off; ex->ph = ph;
      ex->NR = NR; ex->NPR = NPR; ex->tcs = tcs; ex->tce = tce;
      ex->lines_valid = split_lines ? 1u : 0u;
    });
  }
  x.stamp(PH_GR_LINES);
  x.par.single([&]() {
    r[0] = span;
    r[1] = NPR + 1;
    r[2] = para_dup;
    r[3] = para_dup_b;
    r[4] = NR + 1;
    r[5] = line_dup;
    r[6] = line_dup_b;
  });
  // ---- n-gram statistics over the words ----
  // Word-level arrays (LDS while they fit): wid = canonical word id (smallest index of an equal
  // word), WL = byte prefix of word lengths, and for concatenation hashes of any word run
  //   K[k] = sum_{j<k} H(word j) * B^-WL[j+1],  PB[k] = B^WL[k]
  //   H(words p .. p+n-1 concatenated) = PB[p+n] * (K[p+n] - K[p])
  // (the Horner hash of the concatenation), so a run costs one multiplication and no power
  // lookup; the powers are read once per word instead of once per (n, position). They are built
  // while the prefix hashes are still on chip; then the code point arrays and prefix hashes (top
  // of the LDS slice) are released, so the n-gram tables get that space.
  const uint32_t W = w.n;
  const bool ngrams = ds.n_top + ds.n_dup > 0;
  if constexpr (P::kWaves == 1) {
    if (ngrams && W >= kWave16) {
      x.set_flag(DOC_NEEDS_CPU);
      return;
    }
    if constexpr (kExport) {
      // (the launcher picks this build only with an export; anything else goes to the exact CPU path)
      if (!(ngrams && ex)) {
        x.set_flag(DOC_NEEDS_CPU);
        return;
      }
    }
    if (kExport || (ngrams && ex)) {
      // One-wave documents in split mode: the n-gram kernels rebuild everything word-level (ids,
      // byte prefix, concatenation hashes) from the word spans and the text, so nothing is hashed
      // or canonicalised here and only the spans are exported. (Nothing is allocated after this
      // point, so the top of the LDS slice needs no release.)
      const uint64_t base = (x.used + 255) & ~255ull;
      x.par.single([&]() {
        for (int t = 0; t < ds.n_top + ds.n_dup; ++t) r[rec_gr_fixed() + t] = 0;
        ex->bs = w.bs; ex->be = w.be;
        ex->b = b_export ? b_export : b;
        ex->free_base = x.scr + base;
        ex->free_cap = x.cap > base ? x.cap - base : 0;
        ex->W = W;
        ex->valid = x.overflow ? 0u : 1u;
      });
      x.par.sync();
      x.stamp(PH_GR_WORDS);
      x.reset(mark);
      return;
    }
  }
  if constexpr (!kExport) {
    uint32_t* wid = nullptr;
    uint32_t* WL = nullptr;
    uint64_t* K = nullptr;
    uint64_t* PB = nullptr;
    if (ngrams && pre && pre->wready) {
      // built by many workgroups before this one (k_pre_wcanon); a hash collision between unequal
      // words has flagged the document for the CPU path there
      wid = pre->wid;
      WL = pre->wl;
      K = pre->wk;
      PB = pre->wpb;
    } else if (ngrams) {
      // LDS only while a canonicalisation table for W elements (~6 W bytes) still fits next to them
      // (split mode: HBM, they outlive this kernel)
      const uint64_t tab_bytes = 6ull * W + 64;
      wid = ex ? x.template alloc<uint32_t>(W + 1) : x.template alloc_hot_keep<uint32_t>(W + 1, tab_bytes);
      WL = ex ? x.template alloc<uint32_t>(W + 1) : x.template alloc_hot_keep<uint32_t>(W + 1, tab_bytes);
      K = ex ? x.template alloc<uint64_t>(W + 1) : x.template alloc_hot_keep<uint64_t>(W + 1, tab_bytes);
      PB = ex ? x.template alloc<uint64_t>(W + 1) : x.template alloc_hot_keep<uint64_t>(W + 1, tab_bytes);
      const auto mw = x.mark();
      uint64_t* wh = x.template alloc_hot_hi<uint64_t>(W + 1);
      if (x.overflow) return;
      x.par.for_n(W, [&](uint32_t k) { wh[k] = span_hash8(x, ph, w.bs[k], w.be[k]); });
      x.par.sync();
      x.stamp(PH_GR_WH);
      canonicalize(
          x, W, [&](uint32_t k) { return dev_key(wh[k], w.be[k] - w.bs[k]); },
          [&](uint32_t i, uint32_t j) { return bytes_eq<P>(b, w.bs[i], w.be[i], w.bs[j], w.be[j]); }, wid);
      x.stamp(PH_GR_WCANON);
      const uint32_t totl = x.par.template scan<uint32_t>(
          W, 0u, [](uint32_t a, uint32_t c2) { return a + c2; },
          [&](uint32_t k) { return w.be[k] - w.bs[k]; }, [&](uint32_t k, uint32_t e) { WL[k] = e; });
      x.par.single([&]() { WL[W] = totl; });
      x.par.sync();
      x.par.for_n(W + 1, [&](uint32_t k) { PB[k] = x.powb(WL[k]); });
      const uint64_t ktot = x.par.template scan<uint64_t>(
          W, 0ull, [](uint64_t a, uint64_t c2) { return a + c2; },
          [&](uint32_t j) { return wh[j] * x.ipowb(WL[j + 1]); }, [&](uint32_t k, uint64_t e) { K[k] = e; });
      x.par.single([&]() { K[W] = ktot; });
      x.par.sync();
      x.reset(mw);  // wh
      if (x.overflow) return;
    }
    x.stamp(PH_GR_WORDS);
    // the n-gram statistics read words, bytes and the arrays above only: the top of the LDS slice
    // (code point arrays, prefix hashes) goes to their hash tables
    if (release_props) x.release_hi();
    if (ngrams) {
      const DupGrams dg{wid, WL, K, PB, w.bs, w.be, b};
      // Top n-grams (space-joined grams: equal iff their word sequences are equal). Canonical ids
      // of the n-grams are built incrementally: the n-gram at p is the pair (id of the (n-1)-gram
      // at p, id of word p+n-1), so each order is one exact pair canonicalisation (O(1) equality,
      // no hashing of the gram text).
      if (ds.n_top > 0 && ex) {
        // split mode: k_gr_dup_split computes each top order in its own workgroup
        x.par.single([&]() { for (int t = 0; t < ds.n_top; ++t) r[rec_gr_fixed() + t] = 0; });
      } else if (ds.n_top > 0) {
        int max_top = 0;
        for (int t = 0; t < ds.n_top; ++t) max_top = ds.top_n[t] > max_top ? ds.top_n[t] : max_top;
        const auto m2 = x.mark();
        // two id arrays in turn; the counts of order n go to the one the (n-1)-gram ids used
        uint32_t* ga = x.template alloc_hot_keep<uint32_t>(W + 1, 6ull * W + 64);
        uint32_t* gb = x.template alloc_hot_keep<uint32_t>(W + 1, 6ull * W + 64);
        if (x.overflow) return;
        x.par.single([&]() { for (int t = 0; t < ds.n_top; ++t) r[rec_gr_fixed() + t] = 0; });
        const uint32_t* gprev = wid;
        for (uint32_t n = 1; n <= (uint32_t)max_top && W >= n; ++n) {
          const uint32_t G = W - n + 1;
          const uint32_t* gc = wid;
          uint32_t* cnt = (n == 1 || !(n & 1)) ? ga : gb;
          if (n > 1) {
            uint32_t* gcur = (n & 1) ? ga : gb;
            canonicalize(
                x, G, [&](uint32_t p) { return mix64(((uint64_t)gprev[p] << 32) ^ (uint64_t)wid[p + n - 1] ^ ((uint64_t)n << 60)); },
                [&](uint32_t p, uint32_t q) { return gprev[p] == gprev[q] && wid[p + n - 1] == wid[q + n - 1]; }, gcur);
            gc = gcur;
            gprev = gcur;
            x.stamp(PH_GR_TOP_CANON);
          }
          bool wanted = false;
          for (int t = 0; t < ds.n_top; ++t) wanted |= ds.top_n[t] == (int32_t)n;
          if (!wanted) continue;
          x.par.for_n(G, [&](uint32_t p) { cnt[p] = 0; });
          x.par.sync();
          x.par.for_n(G, [&](uint32_t p) { P::add32(&cnt[gc[p]], 1u); });
          x.par.sync();
          const uint32_t maxc = x.par.template max<uint32_t>(G, 0u, [&](uint32_t p) { return cnt[p]; });
          int64_t v = 0;
          if (maxc > 1) {
            const uint32_t maxlen = x.par.template max<uint32_t>(G, 0u, [&](uint32_t p) {
              return cnt[p] == maxc ? (WL[p + n] - WL[p] + n - 1) : 0u;
            });
            v = (int64_t)maxlen * (int64_t)maxc;
          }
          x.par.single([&]() {
            for (int t = 0; t < ds.n_top; ++t) if (ds.top_n[t] == (int32_t)n) r[rec_gr_fixed() + t] = v;
          });
          x.par.sync();
        }
        x.reset(m2);
      }
      x.stamp(PH_GR_TOP);
      if (ex) {
        // split mode: export the word arrays; k_gr_dup_split finishes every order (top and
        // duplicated) in its own workgroup and writes the n-gram fields
        const uint64_t base = (x.used + 255) & ~255ull;
        x.par.single([&]() {
          for (int t = 0; t < ds.n_dup; ++t) r[rec_gr_fixed() + ds.n_top + t] = 0;
          ex->wid = wid; ex->WL = WL; ex->K = K; ex->PB = PB; ex->bs = w.bs; ex->be = w.be;
          ex->b = b_export ? b_export : b;
          ex->free_base = x.scr + base;
          ex->free_cap = x.cap > base ? x.cap - base : 0;
          ex->W = W;
          ex->valid = x.overflow ? 0u : 1u;
        });
        x.par.sync();
      } else if (ds.n_dup > 0) {
        // Two phases over all requested orders n (reference find_all_duplicate,
        // utils/text.rs:241-259):
        //   1. per n: canonicalise the n-gram concatenations into gc_n (exact: hash groups, then
        //      word-id / byte equality) and mark repeated positions in R_n (p with gc[p] != p, and
        //      their first occurrence gc[p]);
        //   2. the greedy walks of all orders run at once, one lane each (they are independent
        //      and sequential, so n walks cost about the longest one instead of their sum).
        // Arrays of all orders are packed back to back: gc_n at gbase(t), bitmaps at t * 2 * SW.
        const uint32_t SW = (W + 31) / 32 + 1;
        const int nd = ds.n_dup;
        auto gsize = [&](int t) -> uint32_t {
          const uint32_t n = (uint32_t)ds.dup_n[t];
          return (n == 0 || W < n) ? 0u : W - n + 1;
        };
        uint32_t gtot = 0;
        for (int t = 0; t < nd; ++t) gtot += gsize(t);
        const auto m3 = x.mark();
        uint32_t* bits = x.template alloc_hot<uint32_t>(2 * (uint64_t)SW * (uint64_t)nd);  // [sn | R] per order
        // wave documents keep the canonical ids in 16 bits (half the slice; W < kWave16)
        using GcT = std::conditional_t<P::kWaves == 1, uint16_t, uint32_t>;
        GcT* gcall = x.template alloc_hot_keep<GcT>((uint64_t)gtot + 1, 6ull * W + 64);
        if (x.overflow) return;
        x.par.for_n(2 * SW * (uint32_t)nd, [&](uint32_t i) { bits[i] = 0; });
        x.par.sync();
        uint32_t gb = 0;
        for (int t = 0; t < nd; ++t) {
          const uint32_t n = (uint32_t)ds.dup_n[t];
          const uint32_t G = gsize(t);
          if (G == 0) continue;
          GcT* gc = gcall + gb;
          uint32_t* R = bits + (uint32_t)t * 2 * SW + SW;
          gb += G;
          auto mark_rep = [&](uint32_t p, uint32_t g) {
            if (g != p) {  // repeated: the position and its first occurrence
              P::or32(&R[p >> 5], 1u << (p & 31));
              P::or32(&R[g >> 5], 1u << (g & 31));
            }
          };
          if constexpr (P::kWaves != 1) {
            // fused into the canonicalisation's last pass
            canonicalize_res(
                x, G, [&](uint32_t p) { return dg.key(p, n); }, [&](uint32_t p, uint32_t q) { return dg.eq(p, q, n); },
                gc, mark_rep);
            x.stamp(PH_GR_DUP_CANON);
          } else {
            // own pass in the one-wave kernel (the fused form costs it registers)
            canonicalize(
                x, G, [&](uint32_t p) { return dg.key(p, n); }, [&](uint32_t p, uint32_t q) { return dg.eq(p, q, n); },
                gc);
            x.stamp(PH_GR_DUP_CANON);
            x.par.for_n(G, [&](uint32_t p) { mark_rep(p, gc[p]); });
            x.par.sync();
          }
        }
        auto walk = [&](uint32_t t, bool wave) -> int64_t {
          const uint32_t G = gsize((int)t);
          if (G == 0) return 0;
          uint32_t base = 0;
          for (uint32_t u = 0; u < t; ++u) base += gsize((int)u);
          uint32_t* sn = bits + t * 2 * SW;
          const uint32_t n = (uint32_t)ds.dup_n[t];
          return wave ? dup_walk_wave(x.par, G, n, gcall + base, sn + SW, sn, WL)
                      : dup_walk(G, n, gcall + base, sn + SW, sn, WL);
        };
        if constexpr (P::kWaves > 1) {
          // one wave per order (whole-wave walks)
          for (uint32_t t = x.par.wave_index(); t < (uint32_t)nd; t += P::kWaves) {
            const int64_t rep = walk(t, true);
            if (x.par.lane == 0) r[rec_gr_fixed() + ds.n_top + t] = rep;
          }
        } else {
          // one lane per order: the orders' walks overlap (the whole-wave walk would run them
          // one after another)
          x.par.for_n((uint32_t)nd, [&](uint32_t t) { r[rec_gr_fixed() + ds.n_top + t] = walk(t, false); });
        }
        x.par.sync();
        x.stamp(PH_GR_DUP_WALK);
        x.reset(m3);
        x.stamp(PH_GR_DUP);
      }
    }
  }
  x.reset(mark);
}

// Repeat candidates of n elements: a superset of the elements equal to some other element. Every
// element sets bit h(key) of a bitmap (fetch-or); one that finds its bit already set sets it in a
// second bitmap. Equal elements have equal keys, so every repeated element lands on a bit of the
// second bitmap; an element whose bit no other element set is unique, and only the candidates need
// the exact canonicalisation (with 8 bitmap bits per element a unique one is a false candidate
// with probability ~1/8). Candidate indices go to list[0, nc) in increasing order; returns nc.
// `bm` holds 2 * bw words (bw a power of two), zeroed here.
template <class P, class KeyF>
TB_HD uint32_t repeat_candidates(DocCtx<P>& x, uint32_t n, KeyF&& key, uint32_t* bm, uint32_t bw, uint32_t* list) {
  const uint32_t mask = bw * 32u - 1u;
  uint32_t* once = bm;
  uint32_t* twice = bm + bw;
  x.par.for_n(2 * bw, [&](uint32_t i) { bm[i] = 0; });
  x.par.sync();
  x.par.for_n(n, [&](uint32_t i) {
    const uint32_t h = (uint32_t)(key(i) >> 20) & mask;
    const uint32_t bit = 1u << (h & 31u);
    if (P::fetch_or32(&once[h >> 5], bit) & bit) P::or32(&twice[h >> 5], bit);
  });
  x.par.sync();
  const uint32_t nc = x.par.template compact<int>(
      n,
      [&](uint32_t i, int&) {
        const uint32_t h = (uint32_t)(key(i) >> 20) & mask;
        return ((twice[h >> 5] >> (h & 31u)) & 1u) != 0;
      },
      [&](uint32_t i, uint32_t k, int&) { list[k] = i; });
  x.par.sync();
  return nc;
}

// Bitmap words of repeat_candidates for n elements (>= 8 bits per element, a power of two) and the
// scratch bytes the candidate path may take beyond the order's own arrays, for the capacity test
// that picks it (the full canonicalisation otherwise: results are the same either way).
TB_HD uint32_t cand_bitmap_words(uint32_t n) {
  uint32_t w = 32;
  while (w * 4u < n) w <<= 1;
  return w;
}
TB_HD uint64_t cand_path_bytes(uint32_t n) { return 8ull * cand_bitmap_words(n) + 16ull * n + 256; }
// (workgroup documents keep the full canonicalisation: with the candidate path their
// partitioned-table runs gave wrong top n-gram records on the GPU, unexplained; the sequential
// emulation of the same code, partitioned tables included, is exact)
template <class P>
TB_HD bool cand_path_fits(const DocCtx<P>& x, uint32_t n) {
  if (P::kWaves > 1) return false;
  const uint64_t need = cand_path_bytes(n);
  return x.cap >= x.used + need + 64 || (uint64_t)x.lds_free() >= need;
}

// Duplicated lines (which = 0: r[5], r[6]) or paragraphs (which = 1: r[2], r[3]) of a split
// document (k_gr_dup_split), over the arrays gopher_rep_record exported.
template <class P>
TB_HD void gr_lines_split(DocCtx<P>& x, int which, const GrExport& e, int64_t* r) {
  if (!e.lines_valid) return;  // computed in the stage
  int64_t elems = 0, bytes = 0;
  if (which == 0)
    dup_spans(x, e.b, e.ph, e.NR + 1,
              [&](uint32_t k, uint32_t& s0, uint32_t& e0) { gr_line_span(e.rs, e.rl, e.off, e.tcs, e.tce, e.NR, k, s0, e0); },
              &elems, &bytes);
  else
    dup_spans(x, e.b, e.ph, e.NPR + 1,
              [&](uint32_t q, uint32_t& s0, uint32_t& e0) {
                gr_para_span(e.rs, e.rl, e.prs, e.off, e.tcs, e.tce, e.NPR, q, s0, e0);
              },
              &elems, &bytes);
  if (x.overflow) return;
  x.par.single([&]() {
    r[which == 0 ? 5 : 2] = elems;
    r[which == 0 ? 6 : 3] = bytes;
  });
  x.par.sync();
}

// One top n-gram order of a split document (k_gr_dup_split): the n-grams of order n are grouped
// by their word-id tuples directly (equal space-joined grams <=> equal word sequences), so the
// orders are independent of each other (the in-stage path chains order n on order n - 1 instead).
// Writes r[7 + t], the same value as the in-stage path.
template <class P>
TB_HD void gr_top_one_order(DocCtx<P>& x, const DevStep& ds, int t, const GrExport& e, int64_t* r) {
  const uint32_t W = e.W, n = (uint32_t)ds.top_n[t];
  int64_t* out = r + rec_gr_fixed() + t;
  if (n == 0 || W < n) {
    x.par.single([&]() { *out = 0; });
    return;
  }
  const uint32_t G = W - n + 1;
  const uint32_t* wid = e.wid;
  const uint32_t* WL = e.WL;
  const auto mark = x.mark();
  auto key = [&](uint32_t p) {
    uint64_t h = (uint64_t)n << 56;
    for (uint32_t k = 0; k < n; ++k) h = (h ^ wid[p + k]) * 0x9E3779B97F4A7C15ull + k;
    return mix64(h);
  };
  auto eq = [&](uint32_t p, uint32_t q) {
    uint32_t dw = 0;
    for (uint32_t k = 0; k < n; ++k) dw |= wid[p + k] ^ wid[q + k];
    return dw == 0;
  };
  // Only the repeat candidates are grouped (every other gram occurs once): pos[c] = position of
  // candidate c, gc[c] = its canonical candidate, cnt[c] = the class size at the canonical one.
  // Without room for the candidate arrays every position is a candidate (the full grouping).
  uint32_t NC = G;
  const uint32_t* pos = nullptr;
  if (cand_path_fits(x, G)) {
    const uint32_t bw = cand_bitmap_words(G);
    uint32_t* bm = x.template alloc_hot<uint32_t>(2 * bw);
    uint32_t* list = x.template alloc_hot<uint32_t>((uint64_t)G + 1);
    if (x.overflow) return;
    NC = repeat_candidates(x, G, key, bm, bw, list);
    pos = list;
  }
  int64_t v = 0;
  if (NC >= 2) {
    uint32_t* gc = x.template alloc_hot_keep<uint32_t>((uint64_t)NC + 1, 6ull * NC + 64);
    uint32_t* cnt = x.template alloc_hot_keep<uint32_t>((uint64_t)NC + 1, 6ull * NC + 64);
    if (x.overflow) return;
    auto at = [&](uint32_t c) { return pos ? pos[c] : c; };
    canonicalize(
        x, NC, [&](uint32_t c) { return key(at(c)); }, [&](uint32_t c, uint32_t d) { return eq(at(c), at(d)); },
        gc);
    if (x.overflow) return;
    x.par.for_n(NC, [&](uint32_t c) { cnt[c] = 0; });
    x.par.sync();
    x.par.for_n(NC, [&](uint32_t c) { P::add32(&cnt[gc[c]], 1u); });
    x.par.sync();
    const uint32_t maxc = x.par.template max<uint32_t>(NC, 0u, [&](uint32_t c) { return cnt[c]; });
    if (maxc > 1) {
      const uint32_t maxlen = x.par.template max<uint32_t>(NC, 0u, [&](uint32_t c) {
        const uint32_t p = at(c);
        return cnt[c] == maxc ? (WL[p + n] - WL[p] + n - 1) : 0u;
      });
      v = (int64_t)maxlen * (int64_t)maxc;
    }
  }
  x.par.single([&]() { *out = v; });
  x.par.sync();
  x.reset(mark);
}

// One duplicated n-gram order of a split document (k_gr_dup_split): the in-stage dup phase for
// order t alone, over the arrays the stage workgroup exported. Writes r[7 + n_top + t].
template <class P>
TB_HD void gr_dup_one_order(DocCtx<P>& x, const DevStep& ds, int t, const GrExport& e, int64_t* r) {
  const uint32_t W = e.W, n = (uint32_t)ds.dup_n[t];
  const uint32_t G = (n == 0 || W < n) ? 0u : W - n + 1;
  int64_t* out = r + rec_gr_fixed() + ds.n_top + t;
  if (G == 0) {
    x.par.single([&]() { *out = 0; });
    return;
  }
  const DupGrams dg{e.wid, e.WL, e.K, e.PB, e.bs, e.be, e.b};
  const uint32_t SW = (G + 31) / 32 + 1;
  const auto mark = x.mark();
  uint32_t* bits = x.template alloc_hot<uint32_t>(2 * (uint64_t)SW);  // [sn | R]
  uint32_t* gc = x.template alloc_hot_keep<uint32_t>((uint64_t)G + 1, 6ull * G + 64);
  if (x.overflow) return;
  x.par.for_n(2 * SW, [&](uint32_t i) { bits[i] = 0; });
  x.par.sync();
  uint32_t* R = bits + SW;
  auto key = [&](uint32_t p) { return dg.key(p, n); };
  // Only the repeat candidates are canonicalised: a gram that is not a candidate occurs once, so
  // its position is never repeated and the walk never reads its gc entry. gc of a candidate
  // position = the class id (its canonical candidate's index).
  if (cand_path_fits(x, G)) {
    const uint32_t bw = cand_bitmap_words(G);
    uint32_t* bm = x.template alloc_hot<uint32_t>(2 * bw);
    uint32_t* list = x.template alloc_hot<uint32_t>((uint64_t)G + 1);
    if (x.overflow) return;
    const uint32_t nc = repeat_candidates(x, G, key, bm, bw, list);
    if (nc >= 2) {
      uint32_t* cc = x.template alloc_hot_keep<uint32_t>((uint64_t)nc + 1, 6ull * nc + 64);
      if (x.overflow) return;
      canonicalize_res(
          x, nc, [&](uint32_t c) { return key(list[c]); },
          [&](uint32_t c, uint32_t d) { return dg.eq(list[c], list[d], n); }, cc,
          [&](uint32_t c, uint32_t g) {
            const uint32_t p = list[c];
            gc[p] = g;
            if (g != c) {
              const uint32_t q = list[g];
              P::or32(&R[p >> 5], 1u << (p & 31));
              P::or32(&R[q >> 5], 1u << (q & 31));
            }
          });
    }
  } else {
    canonicalize_res(
        x, G, key, [&](uint32_t p, uint32_t q) { return dg.eq(p, q, n); }, gc,
        [&](uint32_t p, uint32_t g) {
          if (g != p) {
            P::or32(&R[p >> 5], 1u << (p & 31));
            P::or32(&R[g >> 5], 1u << (g & 31));
          }
        });
  }
  if (x.overflow) return;
  x.par.sync();
  if constexpr (P::kWaves > 0) {
    if (x.par.wave_index() == 0) {
      const int64_t rep = dup_walk_wave(x.par, G, n, gc, R, bits, e.WL);
      if (x.par.lane == 0) *out = rep;
    }
  } else {
    x.par.single([&]() { *out = dup_walk(G, n, gc, R, bits, e.WL); });
  }
  x.par.sync();
  x.reset(mark);
}

}  // namespace tb
