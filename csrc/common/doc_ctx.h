// The document context of every per-document algorithm (docproc.h: the map of the family headers).
#pragma once
#include "hash.h"
#include "par.h"
#include "ucd.h"

namespace tb {

// Phase ids for DocCtx::stamp (profiling only).
enum : int {
  PH_START = 0, PH_DECODE, PH_DICT, PH_PREFIX_HASH, PH_WORDS, PH_LINES, PH_GQ, PH_GR_LINES, PH_GR_WORDS,
  PH_GR_TOP, PH_GR_DUP, PH_FW, PH_LID, PH_GR_DUP_WALK, PH_GR_DUP_CANON, PH_GR_TOP_CANON,
  PH_C4_LOREM = 16, PH_C4_DECODE, PH_C4_LINES, PH_C4_CITE, PH_C4_WORDS, PH_C4_CODES, PH_C4_JOIN, PH_C4_SENT,
  // sub-phases of the stage kernel's GopherRepetition / GopherQuality work
  PH_GR_NL = 24, PH_GR_LINE_DUP, PH_GR_WH, PH_GR_WCANON, PH_GQ_WORDS, PH_GQ_BYTES, PH_RUST_LINES,
  kPhaseSlots = 32
};

enum : uint32_t {
  DOC_OK = 0,
  DOC_NEEDS_CPU = 1,    // dictionary script / hash collision / scratch overflow
  DOC_OVERFLOW = 2,
};

// Code points of a text: byte offsets and compact properties. The code point values themselves
// are not stored: ASCII tests read the lead byte (b[off[i]], equal to the code point below 0x80
// and >= 0xC0 otherwise), the rest re-decode from the bytes.
//
// Compact property layout (16 bits): the UCD word bits 0..13 and 15 (WB class, SB class, WS,
// ALPHA, PUNCT, EXTPICT, DIGIT, CASED) unchanged; bit 14 carries CASE_IGN (bit 16 of the full
// word). P_DICT is consumed while decoding (decode() reports it) and not kept.
constexpr uint32_t P16_CASE_IGN = 1u << 14;
TB_HD uint16_t compact_prop(uint32_t p) {
  return (uint16_t)((p & 0xBFFFu) | ((p & P_CASE_IGN) ? P16_CASE_IGN : 0u));
}

// Per-code-point arrays. Texts under 64 KiB keep one packed u32 per code point (byte offset in
// the low half, compact properties in the high half: 4 bytes, one load); longer ones (workgroup
// path) keep a u32 offset array and a u16 property array. The accessors below hide the layout
// (the choice is uniform per document, so the branch is a scalar one).
struct PropArr {
  const uint32_t* ent = nullptr;
  const uint16_t* p16 = nullptr;
  TB_HD uint32_t operator[](uint32_t i) const { return ent ? (ent[i] >> 16) : (uint32_t)p16[i]; }
  TB_HD PropArr operator+(uint32_t s) const { return PropArr{ent ? ent + s : nullptr, ent ? nullptr : p16 + s}; }
};
struct OffArr {
  const uint32_t* ent = nullptr;
  const uint32_t* o32 = nullptr;
  TB_HD uint32_t operator[](uint32_t i) const { return ent ? (ent[i] & 0xFFFFu) : o32[i]; }
};

struct Cps {
  uint32_t n = 0;
  uint32_t* ent = nullptr;    // packed [n+1] (texts < 64 KiB) ...
  uint32_t* off = nullptr;    // ... or [n+1] byte offsets (off[n] = byte length)
  uint16_t* prop = nullptr;   //     and [n+1] compact properties
  const uint8_t* b = nullptr; // the text
  uint32_t nb = 0;            // its byte length
  TB_HD PropArr props() const { return PropArr{ent, prop}; }
  TB_HD OffArr offs() const { return OffArr{ent, off}; }
  TB_HD uint32_t o(uint32_t i) const { return ent ? (ent[i] & 0xFFFFu) : off[i]; }
  TB_HD uint32_t p(uint32_t i) const { return ent ? (ent[i] >> 16) : (uint32_t)prop[i]; }
  TB_HD uint8_t lead(uint32_t i) const { return b[o(i)]; }
  // lead(i) == '\n' from the properties alone (U+000A is the only code point of word-break
  // class LF): one read of the per-code-point array (LDS on the wave path) instead of the
  // offset read followed by a dependent read of the text
  TB_HD bool is_lf(uint32_t i) const { return (p(i) & P_WB_MASK) == (uint32_t)WB_LF; }
  TB_HD uint32_t cp(uint32_t i) const {
    int len;
    return utf8_decode(b, o(i), nb, &len);
  }
};

struct CpsAcc {  // accessor for the UAX#29 rule templates over a sub-range
  PropArr prop;
  TB_HD uint32_t p(int i) const { return prop[(uint32_t)i]; }
};

// Prefix hashes of a text kept at every 8th byte only (PH8[k] = H(b[0..8k)), PHn = H(b)): a
// prefix at any position is at most 7 Horner steps away, so the table costs 1 byte per text byte
// (LDS-resident for typical documents) instead of 8.
struct PHView {
  const uint64_t* ph8 = nullptr;
  uint64_t phn = 0;
  const uint8_t* b = nullptr;
  uint32_t n = 0;
  TB_HD uint64_t at(uint32_t x) const {
    if (x >= n) return phn;
    uint64_t h = ph8[x >> 3];
    for (uint32_t j = x & ~7u; j < x; ++j) h = hash_push(h, b[j]);
    return h;
  }
};

// a very long document's code points and UAX#29 word-break marks, computed before
// its stage workgroup runs by many workgroups at once (prepass.hip k_pre_count / k_pre_decode /
// k_pre_wb): the non-packed Cps layout (documents of 64 KiB and more) plus the marks words()
// would compute.
struct PreDoc {
  uint32_t* off;     // [n + 1] byte offset of every code point (off[C] = n)
  uint16_t* prop;    // [n + 1] compact properties
  uint32_t* wbm;     // [mask_words(n + 1)] bit i: word boundary before code point i
  uint32_t* nl_pos;  // [n / 2 + 2] code point index of every run of '\n' (GopherRepetition lines)
  uint32_t* nl_len;  //   and its length
  uint32_t n;        // bytes
  uint32_t C;        // code points
  uint32_t dict;     // a dictionary-script code point occurs (the document goes to the CPU path)
  uint32_t NL;       // runs of '\n'
  uint32_t tcs;      // first non-whitespace code point (host: 0xFFFFFFFF)
  uint32_t tce;      // one past the last one (host: 0)
  uint32_t nl_a;     // the runs of '\n' inside [tcs, tce): nl_pos[nl_a, nl_e)
  uint32_t nl_e;
  // the words (words() of the same code points): W entries of cs / ce / bs / be / alpha, and the
  // per-64-code-point chunk scratch of their segmented scan (aggregate, carry-in: 3 words each;
  // word count, first word index)
  uint32_t* wtmp;
  uint32_t* wcs;
  uint32_t* wce;
  uint32_t* wbs;
  uint32_t* wbe;
  uint8_t* wal;
  uint32_t W;
  uint32_t pad;
  // GopherRepetition's word arrays (gopher_rep_record) built by many workgroups
  // (prepass.hip k_pre_wcanon): word hashes, the canonicalisation table (1.5 W + 2 64-bit slots)
  // and each word's slot, per-2048-word chunk sums and bases, and the results wid / WL / K / PB
  // (W + 1 entries each); wready = 1 once they are filled.
  uint64_t* wh;
  uint64_t* wtab;
  uint64_t* wk;
  uint64_t* wpb;
  uint64_t* wcsum;
  uint32_t* wslot;
  uint32_t* wid;
  uint32_t* wl;
  uint32_t wready;
  uint32_t pad2;
};

struct Words {
  uint32_t n = 0;
  uint32_t* cs = nullptr;  // first code point
  uint32_t* ce = nullptr;  // one past last code point
  uint32_t* bs = nullptr;  // byte start
  uint32_t* be = nullptr;  // byte end
  uint8_t* alpha = nullptr;
};

struct Lines {  // Rust str::lines() in code point space
  uint32_t n = 0;
  uint32_t* ls = nullptr;  // start cp
  uint32_t* le = nullptr;  // end cp (excludes '\n' and a '\r' right before it)
};

template <class P>
struct DocCtx {
  P par;
  UcdView ucd;
  const uint64_t* pw = nullptr;  // pw[k] = B^k, k <= pw_n; followed by ipw
  const uint64_t* ipw = nullptr; // ipw[k] = B^-k, k <= pw_n
  uint32_t pw_n = 0;
  const uint16_t* asc = nullptr; // compact UCD properties of code points < 256 (LDS copy), or null
  char* scr = nullptr;       // global (HBM) scratch arena of this document
  uint64_t cap = 0;
  uint64_t used = 0;
  uint64_t peak = 0;         // high-water mark of `used`, host emulation (sizes devplan.h kScratchPerByte)
  char* lds = nullptr;      // optional fast arena (the wave's LDS slice on the device)
  uint32_t lcap = 0;
  uint32_t lused = 0;        // bytes allocated from the bottom of the LDS slice
  uint32_t lhi = 0;          // bytes allocated from the top (temporaries, releasable props)
  uint32_t* flag = nullptr;  // per-document status word
  bool weak_keys = false;     // test hook: canonicalize() sees keys cut to 2 bits (forced collisions)
  bool overflow = false;
  uint64_t* prof = nullptr;  // optional per-document phase cycle counters (kPhaseSlots)
  uint64_t t_last = 0;

  // Phase timing (profiling builds of a run): cycles since the previous stamp go to `id`.
  TB_HD void stamp(int id) {
    if (!prof) return;
    const uint64_t t = P::clock();
    if (t_last && par.leader()) prof[id] += t - t_last;
    t_last = t;
  }

  struct Mark { uint64_t g; uint32_t l, h; };
  TB_HD Mark mark() const { return Mark{used, lused, lhi}; }
  TB_HD void reset(Mark m) { used = m.g; lused = m.l; lhi = m.h; }

  // Placement: big streaming per-code-point arrays live in the HBM scratch arena (alloc);
  // small randomly-accessed ones (hash tables, per-word / per-n-gram arrays, reduction
  // buffers) go to the wave's LDS slice while it has room (alloc_hot), then to HBM. Both are
  // addressed through generic pointers, so algorithm code is the same for either arena.
  template <class T>
  TB_HD T* alloc(uint64_t count) { return alloc_global<T>(count); }
  template <class T>
  TB_HD T* alloc_hot(uint64_t count) {
    if (lds) {
      const uint64_t a = (lused + 15u) & ~15u;
      const uint64_t e = a + count * sizeof(T);
      if (e + lhi <= lcap) {
        lused = (uint32_t)e;
        return (T*)(lds + a);
      }
    }
    return alloc_global<T>(count);
  }
  // Same, from the top of the LDS slice: short-lived tables (released by reset()) and the
  // property array, which the n-gram statistics no longer need (release_hi()), so the space
  // they held goes back to the hash tables of the later phases.
  template <class T>
  TB_HD T* alloc_hot_hi(uint64_t count) {
    if (lds) {
      const uint64_t bytes = (count * sizeof(T) + 15u) & ~15ull;
      const uint64_t lo = (lused + 15u) & ~15u;
      if (lo + lhi + bytes <= lcap) {
        lhi += (uint32_t)bytes;
        return (T*)(lds + (lcap - lhi));
      }
    }
    return alloc_global<T>(count);
  }
  TB_HD void release_hi() { lhi = 0; }
  TB_HD bool in_lds(const void* p) const {
    return lds && (const char*)p >= lds && (const char*)p < lds + lcap;
  }
  // bytes of the LDS slice still free between the bottom and top allocations
  TB_HD uint32_t lds_free() const {
    if (!lds) return 0;
    const uint32_t lo = (lused + 15u) & ~15u;
    return lo + lhi >= lcap ? 0u : lcap - lo - lhi;
  }
  // alloc_hot, but only while `keep` bytes of the slice stay free afterwards (for the hash
  // tables of a later phase, whose random accesses gain far more from the LDS than the
  // sequential scans of this array do); otherwise HBM
  template <class T>
  TB_HD T* alloc_hot_keep(uint64_t count, uint64_t keep) {
    if (lds && (uint64_t)lds_free() >= count * sizeof(T) + 16 + keep) return alloc_hot<T>(count);
    return alloc_global<T>(count);
  }
  template <class T>
  TB_HD T* alloc_global(uint64_t count) {
    uint64_t a = (used + 15) & ~15ull;
    uint64_t e = a + count * sizeof(T) + 16;
    if (e > cap) {
      overflow = true;
      return (T*)scr;  // callers check `overflow` before using results
    }
    used = a + count * sizeof(T);
    // host emulation only: one more live 64-bit value triples the long-document kernels' spills
    if constexpr (P::kWaves == 0) {
      if (used > peak) peak = used;
    }
    return (T*)(scr + a);
  }
  TB_HD void set_flag(uint32_t f) {
    if (flag) P::or32(flag, f);  // atomic: kernels of different steps may run concurrently
  }
  TB_HD uint64_t powb(uint32_t k) const { return k <= pw_n ? pw[k] : hpow(kHashBase, k); }
  TB_HD uint64_t ipowb(uint32_t k) const { return (ipw && k <= pw_n) ? ipw[k] : hpow(kHashBaseInv, k); }
  // `count` elements from the bottom of the LDS slice, or nullptr when they do not fit
  template <class T>
  TB_HD T* try_lds(uint64_t count) {
    if (!lds) return nullptr;
    const uint64_t a = (lused + 15u) & ~15u;
    const uint64_t e = a + count * sizeof(T);
    if (e + lhi > lcap) return nullptr;
    lused = (uint32_t)e;
    return (T*)(lds + a);
  }
};

TB_HD bool is_ws(uint32_t p) { return (p & P_WS) != 0; }

// [tcs, tce): the code points of [0, C) without leading / trailing whitespace (tcs >= tce: all
// whitespace). One wave searches chunk by chunk from each end and stops at the first chunk with a
// non-whitespace code point (usually the first and the last chunk) instead of reducing over all
// code points.
template <class P, class PA>
TB_HD void trim_span(DocCtx<P>& x, const PA& prop, uint32_t C, uint32_t& tcs, uint32_t& tce) {
#if defined(__HIPCC__)
  if constexpr (P::kWaves == 1) {
    const uint32_t lane = x.par.lane;
    tcs = C;
    for (uint32_t base = 0; base < C; base += 64) {
      const uint32_t j = base + lane;
      const uint64_t m = __ballot(j < C && !is_ws(prop[j]));
      if (m) { tcs = base + (uint32_t)__builtin_ctzll(m); break; }
    }
    tce = 0;
    if (tcs < C) {
      for (uint32_t base = (C - 1) & ~63u;; base -= 64) {
        const uint32_t j = base + lane;
        const uint64_t m = __ballot(j < C && !is_ws(prop[j]));
        if (m) { tce = base + (uint32_t)(64 - __clzll((long long)m)); break; }
        if (base == 0) break;
      }
    }
    return;
  }
#endif
  tcs = x.par.template min<uint32_t>(C, C, [&](uint32_t i) { return is_ws(prop[i]) ? C : i; });
  tce = x.par.template max<uint32_t>(C, 0u, [&](uint32_t i) { return is_ws(prop[i]) ? 0u : i + 1; });
}

// The C4 line export of one document: a header (line count, or kLineStatsNone while / when the
// stage did not export) and per Rust line its trimmed byte span, word count and longest word in
// code points. Region of document d at u32 index line_stats_base(off[d], d) of the batch buffer
// (4 * (total bytes / 8 + 16 * documents) + 16 u32): room for line_stats_cap(n) lines.
constexpr uint32_t kLineStatsNone = 0xFFFFFFFFu;
struct alignas(16) LineStat { uint32_t bs, be, nw, mx; };
TB_HD uint64_t line_stats_base(int64_t off_d, int64_t d) { return 4ull * ((uint64_t)off_d / 8u + 16ull * (uint64_t)d); }
TB_HD uint32_t line_stats_cap(uint32_t n) { return n / 8u + 15u; }
TB_HD uint64_t line_stats_words(const int64_t* off, int64_t ndocs) {  // buffer size in u32
  return line_stats_base(off[ndocs], ndocs) + 16u;
}

}  // namespace tb
