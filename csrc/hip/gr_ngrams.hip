// GopherRepetition n-gram orders of the wave documents, from the word spans the stage kernel
// exports (tb_gr_split_wave). (kernel_common.h: the families, the launch ABI.)
#include "kernel_common.h"

#include "../common/gopher_rep.h"

namespace {

// ---- n-gram orders of wave documents, one workgroup per document (k_gr_ngrams) ---------------
// The stage kernel exports only each wave document's word byte spans (GrExport: W, bs, be, text).
// Here kNgWaves waves share one document. They copy its text into LDS (coalesced dwords) and
// build the word-level arrays on chip (ng_build): canonical word ids `wid` (smallest index of an
// equal word, the definition of canonicalize), the 16-bit byte prefix `WL` and one prefix array
// `Q` of a concatenation hash that needs no powers and no multiplications. Then each wave takes
// whole orders (duplicated, then top), one gram per lane at a time, with its table in the wave's
// own LDS region; every LDS array comes from __shared__ declarations (ds_* instructions).
// Records equal gr_dup_one_order / gr_top_one_order (the canonical id of a gram is the smallest
// index of an equal gram however the table is probed and whatever the key function is: equality
// is always decided exactly). Three instantiations cover the wave documents: 256 words for the
// documents up to ngram_big_bytes, 512 words for the longer ones, and 1024 words for the
// documents of either launch with more words than that (a list the first two leave, k_gr_ngrams_list).
// What fits none of them (more than 1024 words, more than kNgTextBytes of text) gets the generic
// arrays from k_gr_words and runs the generic per-order code (k_gr_ngrams_rest).
// Occupancy (LDS per workgroup 12.6 / 25.1 / 50.1 KB): 10 / 6 / 3 workgroups per CU.
// Three waves share the nine orders of the default pipeline evenly (three rounds, no idle wave):
// GPU busy 16.8 -> 16.1-16.4 ms per step against four (profiles/gr_words_onchip/).
#ifndef TB_NG_WAVES
#define TB_NG_WAVES 3
#endif
constexpr int kNgWaves = TB_NG_WAVES;
// text bytes (first word's start to last word's end) a workgroup stages, per instantiation (TEXTB):
// the wave documents' 4 KB, half of it for the 256-word class (its launch takes the documents up
// to ngram_big_bytes); also keeps WL in 16 bits
constexpr uint32_t kNgTextBytes = 4096;
constexpr uint32_t kNgTextSmall = 2048;

// LDS of one document's workgroup for documents of at most MAXW words: the word arrays and one
// region per wave, the larger of the duplicated-order layout (u32 table, u16 canonical ids,
// candidate positions and slots, seen / repeat bitmaps) and the top-order layout (u32 table, u16
// candidate positions, u32 counts packed with slots). The table's space first holds the two
// candidate bitmaps of the order (ng_candidates). Before the orders run, the regions together
// hold the build's arrays (NgBuild).
template <uint32_t MAXW, uint32_t TEXTB>
struct NgBuild {
  static constexpr uint32_t kTextW = TEXTB / 4 + 2;  // dwords (unaligned start, tail)
  static constexpr uint32_t kCap = MAXW + MAXW / 2 + 4;
  uint64_t T[256];         // byte mixing table of the concatenation hash
  uint64_t wkey[MAXW];     // word keys (packed bytes or hash)
  uint32_t txt[kTextW];    // the text
  uint32_t tab[kCap];      // word table: fingerprint << 16 | (word index + 1)
  uint16_t ws[MAXW];       // word starts (byte index into txt)
  uint16_t slot[MAXW];     // the table slot of each word
};

template <uint32_t MAXW, uint32_t TEXTB = (MAXW <= 256 ? kNgTextSmall : kNgTextBytes)>
struct NgShared {
  static_assert(MAXW % 64 == 0, "whole waves of grams");
  static constexpr uint32_t kMaxW = MAXW;
  static constexpr uint32_t kTextBytes = TEXTB;
  static constexpr uint32_t kCap = MAXW + MAXW / 2 + 4;  // table slots (1.5 G + 2, rounded)
  static constexpr uint32_t kSW = (MAXW + 31) / 32 + 1;
  // candidate bitmaps: two arrays of kBW words (a power of two, >= 16 bits per gram) in the table
  static constexpr uint32_t kBW = MAXW / 2;
  static_assert(2 * kBW <= kCap && (kBW & (kBW - 1)) == 0, "bitmaps fit the table space");
  static constexpr uint32_t kDupBytes = 4 * kCap + 3 * 2 * MAXW + 4 * 2 * ((kSW + 3) & ~3u);
  static constexpr uint32_t kTopBytes = 4 * kCap + 2 * MAXW + 4 * MAXW;
  static constexpr uint32_t kRegion = ((kDupBytes > kTopBytes ? kDupBytes : kTopBytes) + 15) & ~15u;
  static_assert(sizeof(NgBuild<MAXW, TEXTB>) <= kNgWaves * kRegion, "the build's arrays fit the regions");
  static_assert(kCap <= 0xFFFFu && TEXTB + 8 <= 0xFFFFu, "16-bit slots, word starts and byte prefixes");
  uint64_t Q[MAXW + 1];
  uint16_t wid[MAXW + 1];
  uint16_t WL[MAXW + 1];
  uint4 region[kNgWaves][kRegion / 16];
};

__device__ __forceinline__ uint32_t ng_home(uint32_t k, uint32_t capn) {
  return (uint32_t)(((uint64_t)k * capn) >> 32);
}

__device__ __forceinline__ uint32_t ng_mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ uint64_t ng_rotl(uint64_t x, uint32_t r) { return (x << (r & 63u)) | (x >> ((64u - r) & 63u)); }
__device__ __forceinline__ uint64_t ng_rotr(uint64_t x, uint32_t r) { return (x >> (r & 63u)) | (x << ((64u - r) & 63u)); }

// The concatenation hash of a byte string s[0, L): H(s) = XOR_i rotl(T[s_i], kNgRot * (L - 1 - i)),
// every byte's table value rotated by the number of bytes after it. So H(a || b) =
// rotl(H(a), kNgRot * len(b)) ^ H(b): the hash of a run of words is a function of its concatenated
// bytes alone, whatever the word split -- the one property a duplicated-gram key needs (grams are
// equal iff their concatenations are; equality itself is decided exactly by ng_dup_eq). With
//   Q[k] = XOR_{j < k} rotr(H(word j), kNgRot * WL[j + 1])
// (a plain XOR prefix) the run of words [p, p + n) hashes to rotl(Q[p + n] ^ Q[p], kNgRot * WL[p + n]):
// no powers, no multiplications. The rotation count is taken mod 64 and kNgRot is odd, so bytes 64
// apart share a rotation; such collisions only cost an exact comparison.
constexpr uint32_t kNgRot = 5;

// Builds S.wid, S.WL, S.Q of the document's W words (1 <= W <= MAXW, text within NS::kTextBytes,
// the caller checked both) in the regions' space. All kNgWaves waves call it.
//  - word keys: a word of <= 8 bytes is keyed by its bytes packed little-endian (with its length
//    the key is injective: equal key = equal word, no byte comparison); a longer word by its
//    concatenation hash, and a fingerprint hit compares the bytes in the LDS copy of the text;
//  - wid from an open-addressing table (the style of ng_top_order: a slot keeps the smallest
//    index of its word through atomicMin, whatever order the lanes arrive in).
template <class NS>
__device__ __forceinline__ void ng_build(NS& S, const GrExport& e, uint32_t W, uint32_t bs0, uint32_t tid) {
  using NB = NgBuild<NS::kMaxW, NS::kTextBytes>;
  NB& B = *(NB*)&S.region[0][0];
  constexpr uint32_t NT = 64 * kNgWaves;
  const uint32_t lane = tid & 63;
  // text: whole dwords from the aligned address at or before the first word (the batch buffers
  // are padded, so the up to 3 bytes read past the document's end stay inside the allocation)
  const uint8_t* g0 = e.b + bs0;
  const uintptr_t a0 = (uintptr_t)g0 & ~(uintptr_t)3;
  const uint32_t head = (uint32_t)((uintptr_t)g0 - a0);
  const uint32_t nd = (head + (e.be[W - 1] - bs0) + 3) >> 2;
  const uint32_t* src = (const uint32_t*)a0;
  for (uint32_t i = tid; i < nd; i += NT) B.txt[i] = src[i];
  for (uint32_t c = tid; c < 256; c += NT)
    B.T[c] = ((uint64_t)ng_mix32(2 * c + 1) << 32) | ng_mix32(2 * c + 0x9E3779B2u);
  const uint32_t capn = W + (W >> 1) + 2;
  for (uint32_t i = tid; i < capn; i += NT) B.tab[i] = 0;
  __syncthreads();
  const uint8_t* t8 = (const uint8_t*)B.txt;
#pragma unroll 1
  for (uint32_t k = tid; k < W; k += NT) {
    const uint32_t s = e.bs[k] - bs0 + head, len = e.be[k] - e.bs[k];
    uint64_t h = 0, pk = 0;
    for (uint32_t i = 0; i < len; ++i) {
      const uint32_t c = t8[s + i];
      h = ng_rotl(h, kNgRot) ^ B.T[c];
      if (i < 8) pk |= (uint64_t)c << (8 * i);
    }
    B.ws[k] = (uint16_t)s;
    B.wkey[k] = len <= 8 ? pk : h;
    S.Q[k + 1] = h;
    S.WL[k + 1] = (uint16_t)len;
  }
  __syncthreads();
  // wave 0: byte prefix WL (sum) and hash prefix Q (XOR), 64 words per step, in place
  if (tid < 64) {
    uint32_t cl = 0;
    uint64_t cq = 0;
    if (lane == 0) { S.WL[0] = 0; S.Q[0] = 0; }
#pragma unroll 1
    for (uint32_t base = 0; base < W; base += 64) {
      const uint32_t k = base + lane;
      uint32_t l = k < W ? (uint32_t)S.WL[k + 1] : 0u;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)l, o);
        if ((int)lane >= o) l += v;
      }
      l += cl;
      uint64_t q = k < W ? ng_rotr(S.Q[k + 1], kNgRot * l) : 0ull;
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)q, o), hi = (uint32_t)__shfl_up((int)(uint32_t)(q >> 32), o);
        if ((int)lane >= o) q ^= ((uint64_t)hi << 32) | lo;
      }
      q ^= cq;
      if (k < W) { S.WL[k + 1] = (uint16_t)l; S.Q[k + 1] = q; }
      cl = (uint32_t)__shfl((int)l, 63);
      cq = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(q >> 32), 63) << 32) | (uint32_t)__shfl((int)(uint32_t)q, 63);
    }
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t k = tid; k < W; k += NT) {
    const uint64_t key = B.wkey[k];
    const uint32_t len = (uint32_t)(S.WL[k + 1] - S.WL[k]);
    const uint32_t hk = ng_mix32((uint32_t)key + (uint32_t)(key >> 32) * 0x9E3779B1u + len);
    const uint32_t fp = hk & 0xFFFFu;
    const uint32_t mine = (fp << 16) | (k + 1);
    uint32_t sl = ng_home(hk, capn);
    while (true) {
      uint32_t cur = B.tab[sl];
      if (cur == 0) {
        cur = atomicCAS(&B.tab[sl], 0u, mine);
        if (cur == 0) break;
      }
      if ((cur >> 16) == fp) {
        const uint32_t q = (cur & 0xFFFFu) - 1u;
        bool same = B.wkey[q] == key && (uint32_t)(S.WL[q + 1] - S.WL[q]) == len;
        if (same && len > 8) {
          const uint32_t sa = B.ws[k], sb = B.ws[q];
          for (uint32_t i = 8; i < len && same; ++i) same = t8[sa + i] == t8[sb + i];
          // (the first 8 bytes too: the key of a long word is its hash, not its bytes)
          for (uint32_t i = 0; i < 8 && same; ++i) same = t8[sa + i] == t8[sb + i];
        }
        if (same) {
          if (q > k) atomicMin(&B.tab[sl], mine);
          break;
        }
      }
      if (++sl == capn) sl = 0;
    }
    B.slot[k] = (uint16_t)sl;
  }
  __syncthreads();
  for (uint32_t k = tid; k <= W; k += NT) S.wid[k] = k < W ? (uint16_t)((B.tab[B.slot[k]] & 0xFFFFu) - 1u) : (uint16_t)0;
  __syncthreads();
}

// Repeat candidates of one order: a superset of the positions whose gram occurs more than once.
// Every gram sets bit h(key) of `once` (fetch-or); a gram that finds its bit already set sets it
// in `twice`. Equal grams have equal keys, so every repeated gram lands on a bit of `twice`; a
// gram whose bit no other gram set occurs once (it cannot repeat), and only the candidates go
// through the exact canonicalisation. With >= 16 bits per gram a unique gram is a false candidate
// with probability < 1/16. Both bitmaps (kBW words each) must be zero on entry. Candidate
// positions land in `list` in increasing order; returns their number (wave-uniform).
template <class NS, class KeyF>
__device__ __forceinline__ uint32_t ng_candidates(uint32_t G, uint32_t lane, uint32_t* once, uint32_t* twice,
                                                  uint16_t* hbuf, uint16_t* list, KeyF&& key) {
  constexpr uint32_t kMask = NS::kBW * 32u - 1u;
  static_assert(kMask <= 0xFFFFu, "bit index in 16 bits");
  // (each position's bit index goes through hbuf, not registers: the kernel is register-bound)
#pragma unroll 1
  for (uint32_t p = lane; p < G; p += 64) {
    const uint32_t h = key(p) & kMask;
    hbuf[p] = (uint16_t)h;
    const uint32_t bit = 1u << (h & 31u);
    if (atomicOr(&once[h >> 5], bit) & bit) atomicOr(&twice[h >> 5], bit);
  }
  __builtin_amdgcn_wave_barrier();
  const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint32_t nc = 0;
#pragma unroll 1
  for (uint32_t base = 0; base < G; base += 64) {
    const uint32_t p = base + lane;
    bool c = false;
    if (p < G) {
      const uint32_t h = hbuf[p];
      c = (twice[h >> 5] >> (h & 31u)) & 1u;
    }
    const uint64_t m = __ballot(c);
    if (c) list[nc + (uint32_t)__popcll(m & lt)] = (uint16_t)p;
    nc += (uint32_t)__popcll(m);
  }
  __builtin_amdgcn_wave_barrier();
  return nc;
}

// gram equality of order n (DupGrams::eq over the LDS arrays; the byte comparison of two grams of
// L bytes with different word sequences walks the exported word spans and the text in HBM)
// (out of line: the byte comparison of different word splits with equal hashes practically never
// runs, and inlined its array pointers stay live in registers through the whole order)
__device__ __attribute__((noinline)) bool ng_dup_eq_bytes(const GrExport* ep, uint32_t p, uint32_t q, uint32_t L) {
  const uint32_t* bs = ep->bs;
  const uint32_t* be = ep->be;
  const uint8_t* b = ep->b;
  uint32_t wp = p, wq = q, bp = bs[p], bq = bs[q];
  for (uint32_t i = 0; i < L; ++i) {
    while (bp == be[wp]) { ++wp; bp = bs[wp]; }
    while (bq == be[wq]) { ++wq; bq = bs[wq]; }
    if (b[bp] != b[bq]) return false;
    ++bp;
    ++bq;
  }
  return true;
}
template <class NS>
__device__ __forceinline__ bool ng_dup_eq(const NS& S, const GrExport* ep, uint32_t p, uint32_t q, uint32_t n) {
  const uint32_t L = (uint32_t)(S.WL[p + n] - S.WL[p]);
  if (L != (uint32_t)(S.WL[q + n] - S.WL[q])) return false;
  uint32_t dw = 0;
  for (uint32_t k = 0; k < n; ++k) dw |= (uint32_t)(S.wid[p + k] ^ S.wid[q + k]);
  if (dw == 0) return true;
  return ng_dup_eq_bytes(ep, p, q, L);
}

template <class NS>
__device__ __forceinline__ int64_t ng_dup_order(NS& S, const GrExport* ep, uint32_t W, uint32_t n, uint32_t lane,
                                                uint4* region, bool prof, uint64_t& c_canon, uint64_t& c_walk) {
  const uint64_t t0 = prof ? __builtin_amdgcn_s_memtime() : 0;
  const uint32_t G = W - n + 1;
  const uint32_t SW = (G + 31) / 32 + 1;
  const uint32_t SWa = (SW + 3u) & ~3u;
  uint32_t* tab = (uint32_t*)region;
  uint16_t* gc = (uint16_t*)(tab + NS::kCap);   // per position: canonical candidate index
  uint16_t* list = gc + NS::kMaxW;              // candidate positions
  uint16_t* gsl = list + NS::kMaxW;             // per candidate: its table slot
  uint32_t* sn = (uint32_t*)(gsl + NS::kMaxW);
  uint32_t* R = sn + SWa;
  for (uint32_t i = lane; i < 2 * NS::kBW; i += 64) tab[i] = 0;
  for (uint32_t i = lane; i < 2 * SWa; i += 64) sn[i] = 0;
  __builtin_amdgcn_wave_barrier();
  // the run's concatenation hash (see kNgRot) and its length, mixed to 32 bits: the low bits pick
  // the candidate bit, the high bits the table's home slot
  auto key = [&](uint32_t p) {
    const uint32_t e = S.WL[p + n];
    const uint64_t h = ng_rotl(S.Q[p + n] ^ S.Q[p], kNgRot * e);
    return ng_mix32((uint32_t)h + (uint32_t)(h >> 32) * 0x9E3779B1u + (e - (uint32_t)S.WL[p]));
  };
  const uint32_t nc = ng_candidates<NS>(G, lane, tab, tab + NS::kBW, gc, list, key);
  if (nc < 2) {  // no gram occurs twice: nothing repeats, the walk counts nothing
    if (prof) c_canon += __builtin_amdgcn_s_memtime() - t0;
    return 0;
  }
  // exact canonicalisation of the candidates: slot value (fp << 16) | (candidate index + 1)
  const uint32_t capn = nc + (nc >> 1) + 2;
  for (uint32_t i = lane; i < capn; i += 64) tab[i] = 0;
  __builtin_amdgcn_wave_barrier();
#pragma unroll 1
  for (uint32_t c = lane; c < nc; c += 64) {
    const uint32_t p = list[c];
    const uint32_t k = key(p);
    const uint32_t fp = (k >> 12) & 0xFFFFu;
    const uint32_t mine = (fp << 16) | (c + 1);
    uint32_t sl = ng_home(k, capn);
    while (true) {
      uint32_t cur = tab[sl];
      if (cur == 0) {
        cur = atomicCAS(&tab[sl], 0u, mine);
        if (cur == 0) break;
      }
      if ((cur >> 16) == fp && ng_dup_eq(S, ep, p, list[(cur & 0xFFFFu) - 1u], n)) {
        if ((cur & 0xFFFFu) > c + 1u) atomicMin(&tab[sl], mine);
        break;
      }
      if (++sl == capn) sl = 0;
    }
    gsl[c] = (uint16_t)sl;
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll 1
  for (uint32_t c = lane; c < nc; c += 64) {
    const uint32_t g = (tab[gsl[c]] & 0xFFFFu) - 1u;
    const uint32_t p = list[c];
    gc[p] = (uint16_t)g;
    if (g != c) {
      const uint32_t q = list[g];
      atomicOr(&R[p >> 5], 1u << (p & 31));
      atomicOr(&R[q >> 5], 1u << (q & 31));
    }
  }
  __builtin_amdgcn_wave_barrier();
  const uint64_t t1 = prof ? __builtin_amdgcn_s_memtime() : 0;
  c_canon += t1 - t0;
  // greedy walk (reference find_all_duplicate, utils/text.rs:241-259; dup_walk_wave over LDS):
  // it only stops at repeated positions (candidates), whose gc holds the class id
  const uint32_t nw = (G + 31) >> 5;
  int64_t rep = 0;
  uint32_t idx = 0;
  while (idx < G) {
    uint32_t p0 = G;
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
    uint32_t g = 0xFFFFFFFFu, l = 0;
    if (act) {
      g = gc[p];
      l = (uint32_t)(S.WL[p + n] - S.WL[p]);
    }
    const bool seen0 = act && ((sn[g >> 5] >> (g & 31)) & 1u);
    uint64_t A = __ballot(act), Sm = __ballot(seen0), cnt = 0, fv = 0;
    uint32_t next = p0 + 64;
    while (A) {
      const uint32_t k = (uint32_t)__builtin_ctzll(A);
      if ((Sm >> k) & 1ull) {
        cnt |= 1ull << k;
        const uint32_t jj = k + n;
        A = jj >= 64 ? 0ull : (A & (~0ull << jj));
        if (p0 + jj > next) next = p0 + jj;
      } else {
        fv |= 1ull << k;
        Sm |= __ballot(g == (uint32_t)__builtin_amdgcn_readlane((int)g, (int)k));
        A &= A - 1;
      }
    }
    if ((fv >> lane) & 1ull) atomicOr(&sn[g >> 5], 1u << (g & 31));
    uint32_t add = ((cnt >> lane) & 1ull) ? l : 0u;
    for (int o = 32; o > 0; o >>= 1) add += (uint32_t)__shfl_xor((int)add, o);
    rep += add;
    __builtin_amdgcn_wave_barrier();
    idx = next;
  }
  if (prof) c_walk += __builtin_amdgcn_s_memtime() - t1;
  return rep;
}

// top n-gram order (reference find_top_duplicate, utils/text.rs:211-238): space-joined grams are
// equal iff their word sequences are, so grams are grouped by their canonical word-id tuples
// (fingerprint table, exact tuple comparison on a match) and counted per canonical gram. Only the
// repeat candidates (ng_candidates) are grouped: every other gram occurs once.
template <class NS>
__device__ __forceinline__ int64_t ng_top_order(NS& S, uint32_t W, uint32_t n, uint32_t lane, uint4* region) {
  const uint32_t G = W - n + 1;
  uint32_t* tab = (uint32_t*)region;
  uint16_t* list = (uint16_t*)(tab + NS::kCap);
  uint32_t* cnt = (uint32_t*)(list + NS::kMaxW);  // per candidate: slot << 16 | count
  for (uint32_t i = lane; i < 2 * NS::kBW; i += 64) tab[i] = 0;
  __builtin_amdgcn_wave_barrier();
  auto key = [&](uint32_t p) {
    uint32_t h = n;
    for (uint32_t k = 0; k < n; ++k) h = (h ^ S.wid[p + k]) * 0x9E3779B1u + k;
    return ng_mix32(h);
  };
  const uint32_t nc = ng_candidates<NS>(G, lane, tab, tab + NS::kBW, (uint16_t*)cnt, list, key);
  if (nc < 2) return 0;  // every gram occurs once
  const uint32_t capn = nc + (nc >> 1) + 2;
  for (uint32_t i = lane; i < capn; i += 64) tab[i] = 0;
  __builtin_amdgcn_wave_barrier();
#pragma unroll 1
  for (uint32_t c = lane; c < nc; c += 64) {
    const uint32_t p = list[c];
    const uint32_t k = key(p);
    const uint32_t fp = (k >> 12) & 0xFFFFu;
    const uint32_t mine = (fp << 16) | (c + 1);
    uint32_t sl = ng_home(k, capn);
    while (true) {
      uint32_t cur = tab[sl];
      if (cur == 0) {
        cur = atomicCAS(&tab[sl], 0u, mine);
        if (cur == 0) break;
      }
      if ((cur >> 16) == fp) {
        const uint32_t qc = (cur & 0xFFFFu) - 1u;
        const uint32_t q = list[qc];
        uint32_t dw = 0;
        for (uint32_t k2 = 0; k2 < n; ++k2) dw |= (uint32_t)(S.wid[p + k2] ^ S.wid[q + k2]);
        if (dw == 0) {
          if (qc > c) atomicMin(&tab[sl], mine);
          break;
        }
      }
      if (++sl == capn) sl = 0;
    }
    cnt[c] = sl << 16;
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll 1
  for (uint32_t c = lane; c < nc; c += 64) {
    const uint32_t g = (tab[cnt[c] >> 16] & 0xFFFFu) - 1u;
    atomicAdd(&cnt[g], 1u);  // low half: counts <= nc <= MAXW never carry into the slot
  }
  __builtin_amdgcn_wave_barrier();
  uint32_t mx = 0;
  for (uint32_t c = lane; c < nc; c += 64) mx = (cnt[c] & 0xFFFFu) > mx ? (cnt[c] & 0xFFFFu) : mx;
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t v = (uint32_t)__shfl_xor((int)mx, o);
    mx = v > mx ? v : mx;
  }
  if (mx <= 1) return 0;
  uint32_t ml = 0;
  for (uint32_t c = lane; c < nc; c += 64) {
    if ((cnt[c] & 0xFFFFu) != mx) continue;
    const uint32_t p = list[c];
    const uint32_t len = (uint32_t)(S.WL[p + n] - S.WL[p]) + n - 1;
    ml = len > ml ? len : ml;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t w = (uint32_t)__shfl_xor((int)ml, o);
    ml = w > ml ? w : ml;
  }
  return (int64_t)ml * (int64_t)mx;
}

#ifndef TB_NG_WPE
#define TB_NG_WPE 8  // 2.51 -> 2.29 ms/step vs 6 (profiles/r8_wpe/)
#endif
// A document the workgroup's arrays do not hold (more than MAXW words, more text than
// NgShared::kTextBytes) is not run by that instantiation: its launch position goes to a list after the export
// array (NgRest). The documents the 256- and 512-word launches leave go to `big`, which the
// 1024-word kernel works off (k_gr_ngrams_list); what that one leaves goes to `pos`, for which
// k_gr_words builds the generic word arrays and k_gr_ngrams_rest runs the orders with the generic
// per-order code. Keeping that code out of these kernels keeps its registers (and the profiling
// counters, kProf) off the hot path.
struct NgRest {
  uint32_t count;         // documents in `pos`
  uint32_t cursor;        // k_gr_ngrams_rest's task cursor
  uint32_t count_big;     // documents in `big`
  uint32_t cursor_big;    // k_gr_ngrams_list's cursor
  uint32_t cursor_words;  // k_gr_words' cursor
  uint32_t pad[3];
  // followed by uint32_t pos[n_docs], big[n_docs]
};
__host__ __device__ inline NgRest* ng_rest(const GrExport* ex, int32_t n_docs) {
  return (NgRest*)((char*)ex + (size_t)n_docs * sizeof(GrExport));
}

// One document (launch position k) by the calling workgroup; false: it does not fit MAXW.
template <uint32_t MAXW, bool kProf>
__device__ __forceinline__ bool ng_document(NgShared<MAXW>& S, const DevStage* __restrict__ stage, int32_t gr_step,
                                            const int32_t* __restrict__ perm, int32_t ndocs,
                                            const GrExport* __restrict__ ex, int k, int64_t* rec, uint64_t* prof) {
  const int doc = perm[k];
  if (doc >= ndocs) return true;
  const GrExport& e = ex[k];
  if (!e.valid) return true;  // dead, returned early (flagged for the CPU path) or no n-grams
  const uint32_t W = e.W;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t bs0 = W ? e.bs[0] : 0u;
  if (W > MAXW || (W && e.be[W - 1] - bs0 > NgShared<MAXW>::kTextBytes)) return false;
  const DevStep& ds = stage->steps[gr_step];
  int64_t* r = rec + (int64_t)ds.rec_prefix * ndocs + (int64_t)doc * ds.width;
  const int nt = ds.n_dup + ds.n_top;
  uint64_t* pf = kProf ? prof + (size_t)doc * kPhaseSlots : nullptr;
  const uint64_t t0 = kProf ? __builtin_amdgcn_s_memtime() : 0;
  if (W) ng_build(S, e, W, bs0, tid);
  if (kProf && tid == 0) atomicAdd((unsigned long long*)&pf[PH_GR_DUP], (unsigned long long)(__builtin_amdgcn_s_memtime() - t0));
  uint64_t c_canon = 0, c_walk = 0, c_top = 0;  // (profiling: this wave's cycles per phase)
  for (int t = (int)wv; t < nt; t += kNgWaves) {
    int64_t v = 0;
    if (t < ds.n_dup) {
      const uint32_t n = (uint32_t)ds.dup_n[t];
      if (n > 0 && W >= n) v = ng_dup_order(S, ex + k, W, n, lane, S.region[wv], kProf, c_canon, c_walk);
    } else {
      const uint32_t n = (uint32_t)ds.top_n[t - ds.n_dup];
      const uint64_t ts = kProf ? __builtin_amdgcn_s_memtime() : 0;
      if (n > 0 && W >= n) v = ng_top_order(S, W, n, lane, S.region[wv]);
      if (kProf) c_top += __builtin_amdgcn_s_memtime() - ts;
    }
    // record: the top orders first, then the duplicated orders
    if (lane == 0) r[rec_gr_fixed() + (t < ds.n_dup ? ds.n_top + t : t - ds.n_dup)] = v;
  }
  if (kProf && lane == 0) {
    atomicAdd((unsigned long long*)&pf[PH_GR_DUP_CANON], (unsigned long long)c_canon);
    atomicAdd((unsigned long long*)&pf[PH_GR_DUP_WALK], (unsigned long long)c_walk);
    atomicAdd((unsigned long long*)&pf[PH_GR_TOP_CANON], (unsigned long long)c_top);
  }
  return true;
}

// One workgroup per launch position k0 + blockIdx.x.
template <uint32_t MAXW, bool kProf>
__global__ __launch_bounds__(64 * kNgWaves) __attribute__((amdgpu_waves_per_eu(TB_NG_WPE, 8))) void k_gr_ngrams(
    const DevStage* __restrict__ stage, int32_t gr_step, const int32_t* __restrict__ perm, int32_t ndocs,
    const GrExport* __restrict__ ex, int32_t k0, int32_t n_docs, NgRest* rest, int64_t* rec, uint64_t* prof) {
  __shared__ NgShared<MAXW> S;
  const int k = k0 + (int)blockIdx.x;
  if (!ng_document<MAXW, kProf>(S, stage, gr_step, perm, ndocs, ex, k, rec, prof) && threadIdx.x == 0)
    ((uint32_t*)(rest + 1))[n_docs + atomicAdd(&rest->count_big, 1u)] = (uint32_t)k;
}

// The same for the longer documents' launch (512-word arrays: its LDS, not its registers, sets
// the occupancy; a kernel name of its own for the resource budget).
template <uint32_t MAXW, bool kProf>
__global__ __launch_bounds__(64 * kNgWaves) __attribute__((amdgpu_waves_per_eu(TB_NG_WPE, 8))) void k_gr_ngrams_big(
    const DevStage* __restrict__ stage, int32_t gr_step, const int32_t* __restrict__ perm, int32_t ndocs,
    const GrExport* __restrict__ ex, int32_t k0, int32_t n_docs, NgRest* rest, int64_t* rec, uint64_t* prof) {
  __shared__ NgShared<MAXW> S;
  const int k = k0 + (int)blockIdx.x;
  if (!ng_document<MAXW, kProf>(S, stage, gr_step, perm, ndocs, ex, k, rec, prof) && threadIdx.x == 0)
    ((uint32_t*)(rest + 1))[n_docs + atomicAdd(&rest->count_big, 1u)] = (uint32_t)k;
}

// The documents of NgRest's `big` list, with the largest arrays. Persistent: a fixed grid, every
// workgroup takes the next document from the cursor until the list is empty.
template <uint32_t MAXW, bool kProf>
__global__ __launch_bounds__(64 * kNgWaves) __attribute__((amdgpu_waves_per_eu(TB_NG_WPE, 8))) void k_gr_ngrams_list(
    const DevStage* __restrict__ stage, int32_t gr_step, const int32_t* __restrict__ perm, int32_t ndocs,
    const GrExport* __restrict__ ex, int32_t n_docs, NgRest* rest, int64_t* rec, uint64_t* prof) {
  __shared__ NgShared<MAXW> S;
  __shared__ uint32_t s_next;
  const uint32_t total = __hip_atomic_load(&rest->count_big, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint32_t* pos = (uint32_t*)(rest + 1);
  // The document that did not fit is listed by thread 0 at the top of the next round, in the one
  // lane-dependent branch of the loop. (Listed right after ng_document, the branch on
  // threadIdx.x sat between the workgroup barriers and the loop's back edge, and the compiled loop
  // sent the other lanes round again, barriers included, without thread 0: it never ended.)
  constexpr uint32_t kNone = 0xFFFFFFFFu;
  uint32_t misfit = kNone;
  while (true) {
    if (threadIdx.x == 0) {
      if (misfit != kNone) pos[atomicAdd(&rest->count, 1u)] = misfit;
      s_next = atomicAdd(&rest->cursor_big, 1u);
    }
    __syncthreads();
    const uint32_t i = s_next;
    __syncthreads();  // (s_next and S are rewritten for the next document)
    if (i >= total) break;
    const int k = (int)pos[n_docs + i];
    misfit = ng_document<MAXW, kProf>(S, stage, gr_step, perm, ndocs, ex, k, rec, prof) ? kNone : (uint32_t)k;
  }
}

// The generic word arrays (canonical ids, byte prefix WL, concatenation hash prefixes K / PB, see
// gopher_rep_record) of documents the stage kernel exported without them, one wave per document,
// from the unused rest of the document's scratch slice; the export descriptor then describes what
// the generic per-order code reads. Documents: NgRest's `pos` list (persistent, from a cursor) or,
// with n_all > 0, launch positions [0, n_all), one per block.
__global__ __launch_bounds__(64) void k_gr_words(const int32_t* __restrict__ perm, int32_t ndocs, GrExport* ex,
                                                 NgRest* rest, int32_t n_all, const uint64_t* __restrict__ pw,
                                                 uint32_t pw_n, DevTables tabs, uint32_t* flags) {
  const uint32_t total =
      n_all > 0 ? 0u : __hip_atomic_load(&rest->count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t* pos = (const uint32_t*)(rest + 1);
  while (true) {
    int k = (int)blockIdx.x;
    if (n_all <= 0) {
      uint32_t i = 0;
      if (threadIdx.x == 0) i = atomicAdd(&rest->cursor_words, 1u);
      i = (uint32_t)__builtin_amdgcn_readfirstlane((int)i);
      if (i >= total) break;
      k = (int)pos[i];
    }
    const int doc = perm[k];
    GrExport& e = ex[k];
    if (doc < ndocs && e.valid) {
      const uint32_t W = e.W;
      const uint32_t* bs = e.bs;
      const uint32_t* be = e.be;
      const uint8_t* b = e.b;
      DocCtx<WavePar> x;
      x.prof = nullptr;
      x.lds = nullptr;
      x.lcap = 0;
      x.lused = 0;
      x.ucd = UcdView{tabs.s1, tabs.s2, tabs.l1, tabs.l2};
      x.pw = pw;
      x.pw_n = pw_n;
      x.ipw = pw ? pw + pw_n + 1 : nullptr;
      x.scr = e.free_base;
      x.cap = e.free_cap;
      x.used = 0;
      x.flag = flags + doc;
      uint32_t* wid = x.template alloc<uint32_t>(W + 1);
      uint32_t* WL = x.template alloc<uint32_t>(W + 1);
      uint64_t* K = x.template alloc<uint64_t>(W + 1);
      uint64_t* PB = x.template alloc<uint64_t>(W + 1);
      const uint64_t keep = x.used;
      uint64_t* wh = x.template alloc<uint64_t>(W + 1);
      if (!x.overflow) {
        x.par.for_n(W, [&](uint32_t j) {
          uint64_t h = 0;
          for (uint32_t i = bs[j]; i < be[j]; ++i) h = hash_push(h, b[i]);
          wh[j] = h;
        });
        x.par.sync();
        canonicalize(
            x, W, [&](uint32_t j) { return dev_key(wh[j], be[j] - bs[j]); },
            [&](uint32_t i, uint32_t j) { return bytes_eq<WavePar>(b, bs[i], be[i], bs[j], be[j]); }, wid);
      }
      if (!x.overflow) {
        const uint32_t totl = x.par.template scan<uint32_t>(
            W, 0u, [](uint32_t a, uint32_t c2) { return a + c2; }, [&](uint32_t j) { return be[j] - bs[j]; },
            [&](uint32_t j, uint32_t v) { WL[j] = v; });
        x.par.single([&]() { WL[W] = totl; });
        x.par.sync();
        x.par.for_n(W + 1, [&](uint32_t j) { PB[j] = x.powb(WL[j]); });
        const uint64_t ktot = x.par.template scan<uint64_t>(
            W, 0ull, [](uint64_t a, uint64_t c2) { return a + c2; },
            [&](uint32_t j) { return wh[j] * x.ipowb(WL[j + 1]); }, [&](uint32_t j, uint64_t v) { K[j] = v; });
        x.par.single([&]() { K[W] = ktot; });
        x.par.sync();
      }
      if (x.overflow) x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW);
      const uint64_t base = (keep + 255) & ~255ull;
      const bool ok = !x.overflow && base <= e.free_cap;
      x.par.single([&]() {
        e.wid = wid; e.WL = WL; e.K = K; e.PB = PB;
        if (ok) {
          e.free_base += base;
          e.free_cap -= base;
        }
        e.valid = ok ? 1u : 0u;  // (0: the per-order kernels skip it; flagged for the CPU path)
      });
    }
    if (n_all > 0) break;
  }
}

// The orders of the documents in NgRest's `pos` list (they fit none of the k_gr_ngrams
// instantiations; k_gr_words has built their generic arrays): one
// wave per (document, order) task from an atomic cursor, the generic per-order code over the
// document's HBM scratch (each order in its own share of the unused slice). Persistent: a fixed
// grid, every wave leaves once the cursor passes the last task.
__global__ __launch_bounds__(64) void k_gr_ngrams_rest(
    const DevStage* __restrict__ stage, int32_t gr_step, const int32_t* __restrict__ perm, int32_t ndocs,
    const GrExport* __restrict__ ex, NgRest* rest, const uint64_t* __restrict__ pw, uint32_t pw_n, DevTables tabs,
    int64_t* rec, uint32_t* flags) {
  const DevStep& ds = stage->steps[gr_step];
  const int nt = ds.n_dup + ds.n_top;
  const uint32_t total = __hip_atomic_load(&rest->count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) * (uint32_t)nt;
  const uint32_t* pos = (const uint32_t*)(rest + 1);
  while (true) {
    uint32_t task = 0;
    if (threadIdx.x == 0) task = atomicAdd(&rest->cursor, 1u);
    task = (uint32_t)__builtin_amdgcn_readfirstlane((int)task);
    if (task >= total) break;
    const int k = (int)pos[task / (uint32_t)nt], t = (int)(task % (uint32_t)nt);
    const int doc = perm[k];
    const GrExport e = ex[k];
    if (!e.valid) continue;  // k_gr_words ran out of scratch: flagged for the CPU path
    int64_t* r = rec + (int64_t)ds.rec_prefix * ndocs + (int64_t)doc * ds.width;
    DocCtx<WavePar> x;
    x.prof = nullptr;
    x.lds = nullptr;
    x.lcap = 0;
    x.lused = 0;
    x.ucd = UcdView{tabs.s1, tabs.s2, tabs.l1, tabs.l2};
    x.pw = pw;
    x.pw_n = pw_n;
    x.ipw = pw ? pw + pw_n + 1 : nullptr;
    const uint64_t region = (e.free_cap / (uint64_t)nt) & ~255ull;
    x.scr = e.free_base + (uint64_t)t * region;
    x.cap = region;
    x.used = 0;
    x.flag = flags + doc;
    if (t < ds.n_dup) gr_dup_one_order(x, ds, t, e, r);
    else gr_top_one_order(x, ds, t - ds.n_dup, e, r);
    if (x.overflow) x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW);
  }
}

// The n-gram orders of wave documents with the generic code (tb_gr_split_wave with block == 0,
// after k_gr_words; the default run has no document here): one wave per
// (document, task), task = duplicated n-gram order t < n_dup, then top order t - n_dup. Block k
// handles launch position k / n_tasks of the wave launch (its export slot) and task k % n_tasks;
// every task works in its own share of the document's unused scratch slice (tables stay in the
// LDS slice for wave-sized documents). Same records as the in-stage path.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_gr_split_wave(
    const DevStage* __restrict__ stage, int32_t gr_step, const int32_t* __restrict__ perm, int32_t n_tasks,
    int32_t ndocs, const GrExport* __restrict__ ex, const uint64_t* __restrict__ pw, uint32_t pw_n, DevTables tabs,
    int64_t* rec, uint32_t* flags, uint32_t lds_bytes) {
  const int k = (int)blockIdx.x / n_tasks, t = (int)blockIdx.x % n_tasks;
  const int doc = perm[k];
  if (doc >= ndocs) return;
  const GrExport e = ex[k];
  if (!e.valid) return;  // not exported: dead, returned early (flagged for the CPU path) or no n-grams
  DocCtx<WavePar> x;
  x.prof = nullptr;
  x.lds = lds_bytes ? (char*)g_lds_arena : nullptr;
  x.lcap = lds_bytes;
  x.lused = 0;
  x.ucd = UcdView{tabs.s1, tabs.s2, tabs.l1, tabs.l2};
  x.pw = pw;
  x.pw_n = pw_n;
  x.ipw = pw ? pw + pw_n + 1 : nullptr;
  const uint64_t region = (e.free_cap / (uint64_t)n_tasks) & ~255ull;
  x.scr = e.free_base + (uint64_t)t * region;
  x.cap = region;
  x.used = 0;
  x.flag = flags + doc;
  const DevStep& ds = stage->steps[gr_step];
  int64_t* r = rec + (int64_t)ds.rec_prefix * ndocs + (int64_t)doc * ds.width;
  if (t < ds.n_dup) gr_dup_one_order(x, ds, t, e, r);
  else if (t < ds.n_dup + ds.n_top) gr_top_one_order(x, ds, t - ds.n_dup, e, r);
  if (x.overflow) x.set_flag(DOC_NEEDS_CPU | DOC_OVERFLOW);
}

// The k_gr_ngrams launches of tb_gr_split_wave (block != 0) over n_docs launch positions.
template <bool kProf>
static void launch_gr_ngrams(hipStream_t stream, const DevStage* stage, int32_t gr_step, const int32_t* perm,
                             int32_t ndocs, const GrExport* ex, int32_t n_docs, int32_t n_big, NgRest* rest,
                             int64_t* rec, uint64_t* prof, uint32_t list_grid) {
  const dim3 nt(64 * kNgWaves);
  if (n_big > 0)
    hipLaunchKernelGGL((k_gr_ngrams_big<512, kProf>), dim3((uint32_t)n_big), nt, 0, stream, stage, gr_step, perm, ndocs,
                       ex, 0, n_docs, rest, rec, prof);
  if (n_docs > n_big)
    hipLaunchKernelGGL((k_gr_ngrams<256, kProf>), dim3((uint32_t)(n_docs - n_big)), nt, 0, stream, stage, gr_step,
                       perm, ndocs, ex, n_big, n_docs, rest, rec, prof);
  hipLaunchKernelGGL((k_gr_ngrams_list<1024, kProf>), dim3(list_grid), nt, 0, stream, stage, gr_step,
                     perm, ndocs, ex, n_docs, rest, rec, prof);
}

}  // namespace

extern "C" {

size_t tb_sizeof_gr_export() { return sizeof(GrExport); }

// Wave documents in split mode (tb_stage_analyze with gr_export): n_docs export slots, n_tasks =
// the GopherRepetition step's duplicated + top n-gram orders. Launch positions (the host puts the
// longer documents first), with block != 0 one workgroup per document: [0, n_big) k_gr_ngrams_big<512>,
// the rest k_gr_ngrams<256>, what they leave k_gr_ngrams_list<1024>, what that leaves the generic
// code (k_gr_words, k_gr_ngrams_rest). block == 0: the generic code for all, one wave per
// (document, order) (k_gr_words, k_gr_split_wave).
int tb_gr_split_wave(hipStream_t stream, const void* stage, int32_t gr_step, const TbDocs* d, int32_t n_tasks,
                     const void* gr_export, const TbWork* w, const TbTables* tb, int32_t block, int32_t n_big) {
  const int32_t* perm = d->perm;
  const int32_t n_docs = d->n_launch, ndocs = d->ndocs;
  const DevTables& t = tb->ucd;
  const uint64_t* pw = tb->pw;
  const uint32_t pw_n = tb->pw_n, lds_bytes = w->lds_bytes;
  int64_t* rec = w->rec;
  uint32_t* flags = w->flags;
  uint64_t* prof = w->prof;
  if (n_docs <= 0 || n_tasks <= 0) return 0;
  if (!perm || !gr_export || gr_step < 0 || gr_step >= kMaxStageSteps || n_tasks > 2 * kMaxNgramEntries ||
      lds_bytes > kMaxLdsPerDoc || n_big < 0 || n_big > n_docs)
    return (int)hipErrorInvalidValue;
  GrExport* ex = (GrExport*)gr_export;
  // (the export buffer carries NgRest + 2 * n_docs positions after the descriptors, zeroed)
  NgRest* rest = ng_rest(ex, n_docs);
  if (!block) {
    if (lds_bytes > 65536)
      (void)hipFuncSetAttribute((const void*)k_gr_split_wave, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds_bytes);
    hipLaunchKernelGGL(k_gr_words, dim3((uint32_t)n_docs), dim3(64), 0, stream, perm, ndocs, ex, rest, n_docs, pw, pw_n,
                       t, flags);
    hipLaunchKernelGGL(k_gr_split_wave, dim3((uint32_t)n_docs * (uint32_t)n_tasks), dim3(64), lds_bytes, stream,
                       (const DevStage*)stage, gr_step, perm, n_tasks, ndocs, ex, pw, pw_n, t, rec, flags, lds_bytes);
    return (int)hipGetLastError();
  }
  // (k_gr_ngrams_list is persistent: three workgroups of its 49 KB of LDS fit a CU)
  const uint32_t list_grid = 3u * (uint32_t)device_cus();
  if (prof)
    launch_gr_ngrams<true>(stream, (const DevStage*)stage, gr_step, perm, ndocs, ex, n_docs, n_big, rest, rec, prof, list_grid);
  else
    launch_gr_ngrams<false>(stream, (const DevStage*)stage, gr_step, perm, ndocs, ex, n_docs, n_big, rest, rec, nullptr,
                            list_grid);
  hipLaunchKernelGGL(k_gr_words, dim3(256), dim3(64), 0, stream, perm, ndocs, ex, rest, 0, pw, pw_n, t, flags);
  hipLaunchKernelGGL(k_gr_ngrams_rest, dim3(512), dim3(64), 0, stream, (const DevStage*)stage, gr_step, perm, ndocs,
                     ex, rest, pw, pw_n, t, rec, flags);
  return (int)hipGetLastError();
}

}  // extern "C"
