// Decode and segmentation of one text, once per content version, and the SWAR byte helpers.
#pragma once
#include "doc_ctx.h"
#include "uax29.h"

namespace tb {

template <class P>
TB_HD Cps decode(DocCtx<P>& x, const uint8_t* b, uint32_t n, bool hot = false, uint32_t* dict = nullptr) {
  Cps c;
  c.b = b;
  c.nb = n;
  // read by every later pass (rule look-around, trims, spans): with `hot` they go to the top of
  // the LDS slice when the document is small enough (released before the n-gram statistics)
  const bool packed = n < 65536u;
  if (packed) {
    c.ent = hot ? x.template alloc_hot_hi<uint32_t>(n + 1) : x.template alloc<uint32_t>(n + 1);
  } else {
    c.prop = hot ? x.template alloc_hot_hi<uint16_t>(n + 1) : x.template alloc<uint16_t>(n + 1);
    c.off = hot ? x.template alloc_hot_hi<uint32_t>(n + 1) : x.template alloc<uint32_t>(n + 1);
  }
  if (x.overflow) return c;
  const UcdView ucd = x.ucd;
  const uint16_t* asc = x.asc;
  uint32_t* ent = c.ent;
  uint32_t* off = c.off;
  uint16_t* pra = c.prop;
  uint32_t dl = 0;
  c.n = x.par.template compact<int>(
      n, [&](uint32_t i, int&) { return utf8_is_lead(b[i]); },
      [&](uint32_t i, uint32_t k, int&) {
        uint16_t cpk;
        const uint32_t c0 = b[i];
        // U+0000..U+00FF (ASCII, and C2 / C3 leads: Latin-1, e.g. æ ø å ä ö é) from the LDS table,
        // decoded inline; none of them is a dictionary script
        if (asc && (c0 < 0x80 || (c0 & 0xFEu) == 0xC2u)) {
          cpk = asc[c0 < 0x80 ? c0 : (((c0 & 0x1Fu) << 6) | (b[i + 1] & 0x3Fu))];
        } else {
          int len;
          const uint32_t p = ucd.props(utf8_decode(b, i, n, &len));
          cpk = compact_prop(p);
          dl |= (p & P_DICT) ? 1u : 0u;
        }
        if (packed) {
          ent[k] = i | ((uint32_t)cpk << 16);
        } else {
          off[k] = i;
          pra[k] = cpk;
        }
      });
  const uint32_t cn = c.n;
  x.par.single([&]() {
    if (packed) ent[cn] = n;
    else { off[cn] = n; pra[cn] = 0; }
  });
  if (dict) *dict = x.par.reduce_or(dl);
  x.par.sync();
  return c;
}

struct HL {
  uint64_t h;
  uint32_t len;
  uint32_t pad;
};

template <class P>
TB_HD uint64_t span_hash8(const DocCtx<P>& x, const PHView& v, uint32_t s, uint32_t e) {
  const uint64_t hs = v.at(s), he = v.at(e);
  return he - hs * x.powb(e - s);
}

template <class P>
TB_HD PHView prefix_hash8(DocCtx<P>& x, const uint8_t* b, uint32_t n) {
  PHView v;
  v.b = b;
  v.n = n;
  const uint32_t nblk = (n + 7) >> 3;
  // top of the slice: released with the code point arrays before the n-gram statistics
  uint64_t* ph8 = x.template alloc_hot_hi<uint64_t>(nblk + 1);
  if (x.overflow) return v;
  const uint64_t* pw = x.pw;
  const uint32_t pwn = x.pw_n;
  HL tot = x.par.template scan<HL>(
      nblk, HL{0, 0, 0},
      [&](const HL& a, const HL& c) {
        uint64_t m = c.len <= pwn ? pw[c.len] : hpow(kHashBase, c.len);
        return HL{a.h * m + c.h, a.len + c.len, 0};
      },
      [&](uint32_t k) {
        const uint32_t s0 = k << 3, e0 = s0 + 8 < n ? s0 + 8 : n;
        uint64_t h = 0;
        // (a sum of independent (v_j + 1) * B^(L-1-j) terms measured slower: 23.1 K -> 31.5 K
        // prefix_hash cycles/doc, the power loads)
        for (uint32_t j = s0; j < e0; ++j) h = hash_push(h, b[j]);
        return HL{h, e0 - s0, 0};
      },
      [&](uint32_t k, const HL& e) { ph8[k] = e.h; });
  x.par.single([&]() { ph8[nblk] = tot.h; });
  x.par.sync();
  v.ph8 = ph8;
  v.phn = tot.h;
  return v;
}

// UAX#29 word segments of code points [0, C) -> words (trimmed, with a word character).
// Segments are aggregated with one segmented scan over the code points (no per-lane walk over a
// segment): a segment's first code point carries the reset flag, the running element ORs the
// word-character / alphabetic bits and tracks the first and last non-whitespace code point.
struct WSeg {
  uint32_t bits;   // bit0: segment start (reset), bit1: has a word char, bit2: alphabetic
  uint32_t first;  // first non-whitespace cp (0xFFFFFFFF if none)
  uint32_t last;   // one past the last non-whitespace cp
};
TB_HD WSeg wseg_op(const WSeg& a, const WSeg& b) {
  if (b.bits & 1u) return b;
  return WSeg{a.bits | (b.bits & 6u), a.first < b.first ? a.first : b.first, a.last > b.last ? a.last : b.last};
}

// Word-boundary mark before code point i of [0, C) (sot and eot included). The rules are first
// decided from the properties of i-2 .. i+1 (wb_break_ctx: straight-line compares, no look-around
// loops); only windows holding Extend / Format / ZWJ / RI take the general rule walk, so a chunk
// with punctuation or digits does not serialise the wave on it.
#if defined(__HIPCC__)
// the word-break pair table (uax29.h kWbPairTab) in constant memory: the one-wave words() loads it
// into one register (lane k holds dword k) and reads a pair's dword from the lane that holds it;
// word_mark() on the device reads it directly
static __constant__ WbPairTab g_wb_pair_tab = kWbPairTab;
#endif
TB_HD bool word_mark(const PropArr& prop, uint32_t C, uint32_t i) {
  if (i == 0 || i == C) return true;
  {  // (a scope of its own: the look-around values are dead before the general rule walk)
    const uint32_t pm2 = i >= 2 ? prop[i - 2] : 0xFFFFFFFFu;
    const uint32_t pp1 = i + 1 < C ? prop[i + 1] : 0xFFFFFFFFu;
#if defined(__HIP_DEVICE_COMPILE__)
    const int r = wb_break_ctx_tab(pm2, prop[i - 1], prop[i], pp1, [](uint32_t k) { return g_wb_pair_tab.w[k]; });
#else
    const int r = wb_break_ctx_tab(pm2, prop[i - 1], prop[i], pp1);
#endif
    if (r != 2) return r != 0;
  }
  return wb_break(CpsAcc{prop}, (int)C, (int)i);
}

#if defined(__HIPCC__)
// words() for one wave (WavePar), in one pass over the code points instead of a mark pass and a
// scan pass: each chunk's packed entries are loaded once (the next chunk's while this one is
// processed, so the load is off the critical path), the neighbours the break rules look at come
// from DPP lane moves (wave_shr / wave_shl) plus a two-entry carry, and each word's extent comes
// from bit operations on the chunk's ballots (no segmented scan). Same words as the generic
// version (word_mark + the WSeg scan).
struct WSeg5 {  // the segment still open at a chunk's end
  uint32_t bits, first, last, fo, lo;  // WSeg bits + byte offsets of `first` / `last`
};
__device__ __forceinline__ uint32_t lane_prev(uint32_t v) {  // lane l gets lane l-1 (lane 0: v)
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t lane_next(uint32_t v) {  // lane l gets lane l+1 (lane 63: v)
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x130, 0xF, 0xF, false);
}
// The pair table dword of the pair (pm1, p0): read from the lane that holds it, by every lane of
// the wave at once (a lane read from a lane outside EXEC returns nothing useful, so this is never
// done under divergent control flow).
__device__ __forceinline__ uint32_t wb_pair_dword(uint32_t wbt, uint32_t pm1, uint32_t p0) {
  const uint32_t i = (pm1 & P_WB_MASK) * kWbClasses + (p0 & P_WB_MASK);
  return (uint32_t)__shfl((int)wbt, (int)(i >> 3));
}
// word_mark from the four properties around position i (sentinel 0xFFFFFFFF outside [0, C));
// tw: the pair table dword of (pm1, p0) (wb_pair_dword)
__device__ __forceinline__ bool word_mark4(const PropArr& prop, uint32_t C, uint32_t i, uint32_t pm2, uint32_t pm1,
                                           uint32_t p0, uint32_t pp1, uint32_t tw) {
  if (i == 0 || i >= C) return true;
  const int r = wb_break_ctx_tab(pm2, pm1, p0, pp1, [&](uint32_t) { return tw; });
  if (r != 2) return r != 0;
  return wb_break(CpsAcc{prop}, (int)C, (int)i);
}
template <class P>
__device__ Words words_wave(DocCtx<P>& x, const Cps& c, const uint32_t* marks) {
  Words w;
  const uint32_t C = c.n;
  w.cs = x.template alloc<uint32_t>(C + 1);
  w.ce = x.template alloc<uint32_t>(C + 1);
  w.bs = x.template alloc<uint32_t>(C + 1);
  w.be = x.template alloc<uint32_t>(C + 1);
  w.alpha = x.template alloc<uint8_t>(C + 1);
  if (x.overflow) return w;
  const PropArr prop = c.props();
  const uint32_t lane = x.par.lane;
  const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  // The word arrays are in the HBM arena (alloc): typed as global, their stores are global_store
  // (vmcnt only) instead of flat stores, which the next chunk's flat loads would have to wait for.
  typedef __attribute__((address_space(1))) uint32_t g32;
  typedef __attribute__((address_space(1))) uint8_t g8;
  g32 *cs = (g32*)w.cs, *ce = (g32*)w.ce, *bs = (g32*)w.bs, *be = (g32*)w.be;
  g8* al = (g8*)w.alpha;
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  // entry i <= C: property (entry C: 0) and byte offset (entry C: the byte length)
  uint32_t cp = 0, co = 0, np = 0, no = 0;
  if (lane <= C) { cp = c.p(lane); co = c.o(lane); }
  const uint32_t wbt = lane < (uint32_t)kWbTabWords ? g_wb_pair_tab.w[lane] : 0u;
  uint32_t c1 = kNone, c2 = kNone;  // properties of the two code points before the chunk
  WSeg5 carry{0u, kNone, 0u, kNone, 0u};
  uint32_t k = 0;
  for (uint32_t base = 0; base < C; base += 64) {
    const uint32_t j = base + lane;
    const uint32_t jn = j + 64;
    if (jn <= C) { np = c.p(jn); no = c.o(jn); }  // prefetch of the next chunk
    // neighbours: i-1, i-2 (carry for the first lanes), i+1 (the next chunk's first for lane 63)
    const uint32_t n0p = (uint32_t)__builtin_amdgcn_readfirstlane((int)np);
    const uint32_t n1p = (uint32_t)__builtin_amdgcn_readlane((int)np, 1);
    const uint32_t n0o = (uint32_t)__builtin_amdgcn_readfirstlane((int)no);
    uint32_t pm1 = lane_prev(cp);
    if (lane == 0) pm1 = c1;
    uint32_t pm2 = lane_prev(pm1);
    if (lane == 0) pm2 = c2;
    uint32_t pp1 = lane_next(cp), on = lane_next(co);
    if (lane == 63) { pp1 = base + 64 <= C ? n0p : kNone; on = n0o; }
    // positions past C-1 do not exist for the rules (word_mark's sentinels)
    const uint32_t pm2s = j >= 2 ? pm2 : kNone;
    const uint32_t pp1s = j + 1 < C ? pp1 : kNone;
    // the mark at base + 64 (lane 63's successor): from the last two code points and the next
    // chunk's first two (uniform); with host marks (dictionary scripts, ICU) both from the bitmap
    const uint32_t l62 = (uint32_t)__builtin_amdgcn_readlane((int)cp, 62);
    const uint32_t l63 = (uint32_t)__builtin_amdgcn_readlane((int)cp, 63);
    const uint32_t i64 = base + 64;
    const uint32_t tw = wb_pair_dword(wbt, pm1, cp), tw64 = wb_pair_dword(wbt, l63, n0p);  // (all lanes)
    bool mk = j < C && word_mark4(prop, C, j, pm2s, pm1, cp, pp1s, tw);
    bool mk64 = i64 >= C || word_mark4(prop, C, i64, l62, l63, n0p, i64 + 1 < C ? n1p : kNone, tw64);
    if (marks) {  // host record: ICU marks (first bitmap) where its mask (second bitmap) is set
      const uint32_t* hm = marks + mask_words(C + 1);
      if (j < C && ((hm[j >> 5] >> (j & 31)) & 1u)) mk = ((marks[j >> 5] >> (j & 31)) & 1u) != 0;
      if (i64 < C && ((hm[i64 >> 5] >> (i64 & 31)) & 1u)) mk64 = ((marks[i64 >> 5] >> (i64 & 31)) & 1u) != 0;
    }
    // Segment aggregates from ballots instead of a scan: a lane's segment runs from the last mark
    // at or below it (or, with none, from an earlier chunk: the carry); its first / last
    // non-whitespace code point and its word-character / alphabetic bits are bit operations on
    // the chunk's masks, the byte offsets two lane reads (ds_bpermute).
    const bool valid = j < C;
    const bool ws = is_ws(cp);
    const uint64_t M = __ballot(mk);  // (mk implies j < C)
    const uint64_t NW = __ballot(valid && !ws);
    const uint64_t WC = __ballot(valid && !ws && !(cp & P_PUNCT));
    const uint64_t AL = __ballot(valid && (cp & P_ALPHA));
    const bool mnext = lane == 63 ? mk64 : (((M >> (lane + 1)) & 1ull) != 0 || j + 1 >= C);
    const uint64_t le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);  // lanes 0 .. lane
    const uint64_t mb = M & le;
    const bool fc = mb == 0;  // the segment began in an earlier chunk
    const uint64_t seg = fc ? le : (le & (~0ull << (63 - __clzll((long long)mb))));
    const uint64_t nws = NW & seg;
    const bool hasw = (WC & seg) != 0 || (fc && (carry.bits & 2u));
    const int f = nws ? __builtin_ctzll(nws) : 0;
    const int l = nws ? 63 - __clzll((long long)nws) : 0;
    const uint32_t fo_l = (uint32_t)__shfl((int)co, f);
    const uint32_t lo_l = (uint32_t)__shfl((int)on, l);
    const bool sel = valid && mnext && hasw;
    const uint64_t sm = __ballot(sel);
    if (sel) {
      const uint32_t q = k + (uint32_t)__popcll(sm & lt);
      const bool cf = fc && carry.first != kNone;
      const uint32_t w0 = cf ? carry.first : base + (uint32_t)f, w1 = nws ? base + (uint32_t)l + 1u : carry.last;
      const uint32_t b0 = cf ? carry.fo : fo_l, b1 = nws ? lo_l : carry.lo;
      const bool alpha = (AL & seg) != 0 || (fc && (carry.bits & 4u));
      cs[q] = w0;
      bs[q] = b0;
      ce[q] = w1;
      be[q] = b1;
      al[q] = alpha ? 1 : 0;
    }
    k += (uint32_t)__popcll(sm);
    {  // carry: the segment open at the chunk's end (uniform)
      const bool rs = M != 0;
      const uint64_t sg = rs ? (~0ull << (63 - __clzll((long long)M))) : ~0ull;
      const uint64_t nwc = NW & sg;
      const uint32_t keep = rs ? 0u : carry.bits;
      carry.bits = (keep & 6u) | ((WC & sg) ? 2u : 0u) | ((AL & sg) ? 4u : 0u);
      if (rs || carry.first == kNone) {
        if (nwc) {
          const int f2 = __builtin_ctzll(nwc);
          carry.first = base + (uint32_t)f2;
          carry.fo = (uint32_t)__builtin_amdgcn_readlane((int)co, f2);
        } else {
          carry.first = kNone;
        }
      }
      if (nwc) {
        const int l2 = 63 - __clzll((long long)nwc);
        carry.last = base + (uint32_t)l2 + 1u;
        carry.lo = (uint32_t)__builtin_amdgcn_readlane((int)on, l2);
      } else if (rs) {
        carry.last = 0u;
        carry.lo = 0u;
      }
    }
    c2 = l62;
    c1 = l63;
    cp = np;
    co = no;
  }
  w.n = k;
  x.par.sync();
  return w;
}
#endif

template <class P>
// `marks`: a host record of the code points [0, C] (dictionary scripts: ICU's dictionary
// segmentation of their lines, text.h dict_word_marks): its marks replace word_mark where its mask
// is set.
TB_HD Words words(DocCtx<P>& x, const Cps& c, const PreDoc* pre = nullptr, const uint32_t* marks = nullptr) {
  Words w;
  if (pre) {  // the pre-pass segmented this document already (k_pre_words)
    w.n = pre->W;
    w.cs = pre->wcs;
    w.ce = pre->wce;
    w.bs = pre->wbs;
    w.be = pre->wbe;
    w.alpha = pre->wal;
    return w;
  }
#if defined(__HIPCC__)
  if constexpr (P::kWaves == 1) return words_wave(x, c, marks);
#endif
  const uint32_t C = c.n;
  w.cs = x.template alloc<uint32_t>(C + 1);
  w.ce = x.template alloc<uint32_t>(C + 1);
  w.bs = x.template alloc<uint32_t>(C + 1);
  w.be = x.template alloc<uint32_t>(C + 1);
  w.alpha = x.template alloc<uint8_t>(C + 1);
  const auto mark = x.mark();
  // word-break positions as a bitmask (C/8 bytes, LDS): one rule evaluation per position, no
  // per-code-point arrays; the segment scan and the word compaction run in one fused pass
  uint32_t* wbm = x.template alloc_hot_hi<uint32_t>(mask_words(C + 1));
  if (x.overflow) return w;
  const PropArr prop = c.props();
  const OffArr off = c.offs();
  if (marks) {  // host record: ICU marks where its mask says so, the rules elsewhere
    const uint32_t* hm = marks + mask_words(C + 1);
    x.par.mask_bits(C + 1, [&](uint32_t i) {
      return ((hm[i >> 5] >> (i & 31)) & 1u) ? ((marks[i >> 5] >> (i & 31)) & 1u) != 0 : word_mark(prop, C, i);
    }, wbm);
  } else {
    x.par.mask_bits(C + 1, [&](uint32_t i) { return word_mark(prop, C, i); }, wbm);
  }
  x.par.sync();
  auto bit = [&](uint32_t i) { return (wbm[i >> 5] >> (i & 31)) & 1u; };
  uint32_t *cs = w.cs, *ce = w.ce, *bs = w.bs, *be = w.be;
  uint8_t* al = w.alpha;
  w.n = x.par.template scan_compact<WSeg>(
      C, WSeg{0u, 0xFFFFFFFFu, 0u} /* two-sided identity */, wseg_op,
      [&](uint32_t j) {
        const uint32_t p = prop[j];
        const bool ws = is_ws(p);
        WSeg e;
        e.bits = bit(j) | ((!(p & P_PUNCT) && !ws) ? 2u : 0u) | ((p & P_ALPHA) ? 4u : 0u);
        e.first = ws ? 0xFFFFFFFFu : j;
        e.last = ws ? 0u : j + 1;
        return e;
      },
      [&](uint32_t j, const WSeg& in) { return bit(j + 1) && (in.bits & 2u); },
      [&](uint32_t, uint32_t k, const WSeg& in) {
        cs[k] = in.first;
        ce[k] = in.last;
        bs[k] = off[in.first];
        be[k] = off[in.last];
        al[k] = (in.bits & 4u) ? 1 : 0;
      });
  x.par.sync();
  x.reset(mark);
  return w;
}

// Rust str::lines() of the whole text, in code point space.
template <class P>
TB_HD Lines rust_lines(DocCtx<P>& x, const Cps& c) {
  Lines L;
  const uint32_t C = c.n;
  L.ls = x.template alloc<uint32_t>(C + 1);
  L.le = x.template alloc<uint32_t>(C + 1);
  if (x.overflow) return L;
  uint32_t* ls = L.ls;
  uint32_t* le = L.le;
  L.n = x.par.template compact<int>(
      C, [&](uint32_t i, int&) { return i == 0 || c.is_lf(i - 1); },
      [&](uint32_t i, uint32_t k, int&) { ls[k] = i; });
  x.par.sync();
  const uint32_t NL = L.n;
  x.par.for_n(NL, [&](uint32_t k) {
    uint32_t e = (k + 1 < NL) ? ls[k + 1] - 1 : (c.is_lf(C - 1) ? C - 1 : C);
    uint32_t ce = e;
    if (e < C && ce > ls[k] && c.lead(ce - 1) == '\r') --ce;
    le[k] = ce;
  });
  x.par.sync();
  return L;
}

// ASCII 'A'..'Z' -> 'a'..'z' in all 8 bytes of v (other bytes unchanged).
TB_HD uint64_t swar_lower8(uint64_t v) {
  constexpr uint64_t k7F = 0x7F7F7F7F7F7F7F7Full, k80 = 0x8080808080808080ull;
  const uint64_t ge_a = (v & k7F) + 0x3F3F3F3F3F3F3F3Full;  // bit 7 set: byte & 0x7F >= 'A'
  const uint64_t gt_z = (v & k7F) + 0x2525252525252525ull;  // bit 7 set: byte & 0x7F > 'Z'
  const uint64_t upper = ge_a & ~gt_z & ~v & k80;
  return v | (upper >> 2);
}

// The four bytes b[q, q + 4) of the text b[0, n), little endian, for a position q at which b + q
// is dword aligned; bytes outside [0, n) read as zero. Only a dword that lies wholly inside the
// text is loaded as one: the first and last dwords of a text's aligned span are read byte by
// byte, since the bytes around a text need not be readable (the last document of a batch, a
// host buffer sized to the text).
TB_HD uint32_t text_dword(const uint8_t* b, uint32_t n, int64_t q) {
  if (q >= 0 && q + 4 <= (int64_t)n) return *(const uint32_t*)(b + q);
  uint32_t v = 0;
  for (uint32_t j = 0; j < 4; ++j) {
    const int64_t sj = q + j;
    if (sj >= 0 && sj < (int64_t)n) v |= (uint32_t)b[sj] << (8 * j);
  }
  return v;
}

// Up to eight bytes of the string p[0, len) from index `from`, packed little endian.
TB_HD constexpr uint64_t pack_le(const char* p, int len, int from = 0) {
  uint64_t v = 0;
  for (int k = 0; k < 8 && from + k < len; ++k) v |= (uint64_t)(uint8_t)p[from + k] << (8 * k);
  return v;
}
TB_HD constexpr uint32_t pack3(const char* p) { return (uint32_t)pack_le(p, 3); }
TB_HD constexpr uint64_t pack5(const char* p) { return pack_le(p, 5); }

// Bytes of v equal to c: bit 7 of each such byte set (exact, no carries between bytes).
TB_HD uint32_t swar_eq_mask(uint32_t v, uint32_t c) {
  const uint32_t t = v ^ (c * 0x01010101u);
  return ~(((t & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | t | 0x7F7F7F7Fu);
}

}  // namespace tb
