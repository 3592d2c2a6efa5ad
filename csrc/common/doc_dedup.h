// Exact (byte-verified) duplicate detection: canonicalize, dup_spans.
#pragma once
#include "devplan.h"
#include "doc_text.h"

namespace tb {

// canon[i] = smallest j with element j == element i (key() groups candidates, eq() verifies).
//
// Up to 65534 elements (every wave-path document): open addressing over ~1.5 n packed 32-bit
// slots (16-bit fingerprint from the key's high bits | smallest index + 1; 0 = empty), half the
// LDS of 64-bit slots, so the table stays on chip. An element joins a slot whose fingerprint
// matches only after eq() against the slot's member says they are equal (a fingerprint
// collision keeps probing), so the grouping is exact and no document is sent to the CPU for it;
// a 32-bit atomic min keeps the smallest index. Larger inputs (workgroup path) use 64-bit slots
// with a 32-bit fingerprint and a verification pass, where a collision between unequal elements
// sends the document to the CPU oracle.
// Zeroes the u32 table t[0, count rounded up to 4) (allocated that large): 16-byte stores.
struct alignas(16) Zero4 { uint32_t v[4]; };
template <class P>
TB_HD void zero_table(DocCtx<P>& x, uint32_t* t, uint32_t count) {
  const uint32_t q = (count + 3u) >> 2;
  // (not in the one-wave kernel: the 16-byte stores cost it registers, measured slower there)
  if (P::kWaves != 1 && (((uintptr_t)t) & 15u) == 0) {
    Zero4* t4 = (Zero4*)t;
    x.par.for_n(q, [&](uint32_t i) { t4[i] = Zero4{{0u, 0u, 0u, 0u}}; });
  } else {
    x.par.for_n(count, [&](uint32_t i) { t[i] = 0; });
  }
}

struct NoResolve {
  TB_HD void operator()(uint32_t, uint32_t) const {}
};

template <class P, class KeyF, class EqF, class CT>
TB_HD void canonicalize(DocCtx<P>& x, uint32_t n, KeyF&& key, EqF&& eq, CT* canon);

// Same, and res(i, canon[i]) for every element once its canonical index is final (fused into
// the last pass, so callers need no extra pass over canon[]).
// canon may be 16-bit (wave documents: n < 43000, so every slot index fits) or 32-bit.
template <class P, class KeyF, class EqF, class CT, class ResF>
TB_HD void canonicalize_res(DocCtx<P>& x, uint32_t n, KeyF&& key, EqF&& eq, CT* canon, ResF&& res) {
  const uint32_t capn = n + (n >> 1) + 2;
  // allocated slots: whole 16-byte groups for zero_table's wide stores (exact in the one-wave kernel)
  const uint32_t capa = P::kWaves == 1 ? capn : (capn + 3u) & ~3u;
  const auto mark = x.mark();
  if (n < 65535u) {
    // The table's random probes want the LDS. When the whole table does not fit the free part
    // of the slice (long documents), the slot range is cut into parts that do: part q holds
    // the elements whose home slot falls in [q*capp, (q+1)*capp), and the parts are built one
    // after another in the same LDS table, from keys computed once into HBM. Equal elements
    // share a home slot, hence a part, so the grouping stays exact.
    const uint32_t fit = x.lds_free() >= 64u ? (x.lds_free() - 32u) / 4u : 0u;
    uint32_t parts = 1;
    if (P::kPartTables && x.lds && capn > fit && fit >= 2048u) parts = (capn + fit - 1) / fit;
    if (P::kPartTables && parts > 1) {
      const uint32_t capp = (capn + parts - 1) / parts;
      uint32_t* tab = x.template alloc_hot_hi<uint32_t>(P::kWaves == 1 ? capp : (capp + 3u) & ~3u);
      uint64_t* keys = x.template alloc<uint64_t>(n);
      if (x.overflow) return;
      x.par.for_n(n, [&](uint32_t i) { keys[i] = x.weak_keys ? (key(i) & 3ull) : key(i); });
      x.par.sync();
      bool full = false;
      for (uint32_t q = 0; q < parts; ++q) {
        zero_table(x, tab, capp);
        x.par.sync();
        x.par.for_n(n, [&](uint32_t i) {
          const uint64_t k = keys[i];
          const uint32_t home = (uint32_t)(((k & 0xFFFFFFFFull) * capn) >> 32);
          if (home / capp != q) return;
          const uint32_t fp = (uint32_t)(k >> 48);
          const uint32_t mine = (fp << 16) | (i + 1);
          uint32_t slot = home - q * capp;
          for (uint32_t probes = 0;; ++probes) {
            if (probes >= capp) {  // a part ran full (never for hashed keys): exact CPU path
              full = true;
              slot = 0;
              break;
            }
            uint32_t cur = tab[slot];
            if (cur == 0) {
              cur = P::cas32(&tab[slot], 0u, mine);
              if (cur == 0) break;
            }
            if ((cur >> 16) == fp && eq(i, (cur & 0xFFFFu) - 1u)) {
              // the slot's index only decreases: no atomic when it is already below mine
              if ((cur & 0xFFFFu) > i + 1u) P::min32(&tab[slot], mine);
              break;
            }
            if (++slot == capp) slot = 0;
          }
          canon[i] = slot;
        });
        x.par.sync();
        x.par.for_n(n, [&](uint32_t i) {
          const uint32_t home = (uint32_t)(((keys[i] & 0xFFFFFFFFull) * capn) >> 32);
          if (home / capp == q) {
            const uint32_t c = (tab[canon[i]] & 0xFFFFu) - 1u;
            canon[i] = c;
            res(i, c);
          }
        });
        x.par.sync();
      }
      if (x.par.reduce_or(full ? 1u : 0u)) {  // uniform: every lane takes the branch together
        // (the document goes to the CPU oracle: res() results are discarded with it)
        x.set_flag(DOC_NEEDS_CPU);
        x.par.for_n(n, [&](uint32_t i) { canon[i] = i; });
        x.par.sync();
      }
      x.reset(mark);
      return;
    }
    uint32_t* tab = x.template alloc_hot_hi<uint32_t>(capa);
    if (x.overflow) return;
    zero_table(x, tab, capn);
    x.par.sync();
    x.par.for_n(n, [&](uint32_t i) {
      const uint64_t k = x.weak_keys ? (key(i) & 3ull) : key(i);
      const uint32_t fp = (uint32_t)(k >> 48);
      const uint32_t mine = (fp << 16) | (i + 1);
      uint32_t slot = (uint32_t)(((k & 0xFFFFFFFFull) * capn) >> 32);
      while (true) {
        uint32_t cur = tab[slot];
        if (cur == 0) {
          cur = P::cas32(&tab[slot], 0u, mine);
          if (cur == 0) break;
        }
        if ((cur >> 16) == fp && eq(i, (cur & 0xFFFFu) - 1u)) {
          if ((cur & 0xFFFFu) > i + 1u) P::min32(&tab[slot], mine);
          break;
        }
        if (++slot == capn) slot = 0;
      }
      canon[i] = slot;
    });
    x.par.sync();
    x.par.for_n(n, [&](uint32_t i) {
      const uint32_t c = (tab[canon[i]] & 0xFFFFu) - 1u;
      canon[i] = c;
      res(i, c);
    });
    x.par.sync();
    x.reset(mark);
    return;
  }
  uint64_t* tab = x.template alloc_hot_hi<uint64_t>(capa);
  if (x.overflow) return;
  zero_table(x, (uint32_t*)tab, 2u * capn);
  x.par.sync();
  x.par.for_n(n, [&](uint32_t i) {
    const uint64_t k = x.weak_keys ? (key(i) & 3ull) : key(i);
    const uint64_t fp = (k >> 32) | 1ull;
    const uint64_t mine = (fp << 32) | (uint64_t)(i + 1);
    uint32_t slot = (uint32_t)(((k & 0xFFFFFFFFull) * capn) >> 32);
    while (true) {
      uint64_t cur = tab[slot];
      if (cur == 0) {
        cur = P::cas64(&tab[slot], 0, mine);
        if (cur == 0) break;
      }
      if ((cur >> 32) == fp) {
        if ((cur & 0xFFFFFFFFull) > (uint64_t)i + 1u) P::min64(&tab[slot], mine);
        break;
      }
      if (++slot == capn) slot = 0;
    }
    canon[i] = slot;
  });
  x.par.sync();
  bool collided = false;
  x.par.for_n(n, [&](uint32_t i) {
    uint32_t c = (uint32_t)(tab[canon[i]] & 0xFFFFFFFFull) - 1u;
    if (c != i && !eq(i, c)) { collided = true; c = i; }
    canon[i] = c;
    res(i, c);
  });
  if (collided) x.set_flag(DOC_NEEDS_CPU);
  x.par.sync();
  x.reset(mark);  // the table is scratch; canon[] lives in the caller's allocation
}

template <class P, class KeyF, class EqF, class CT>
TB_HD void canonicalize(DocCtx<P>& x, uint32_t n, KeyF&& key, EqF&& eq, CT* canon) {
  canonicalize_res(x, n, key, eq, canon, NoResolve{});
}

template <class P>
TB_HD bool bytes_eq(const uint8_t* b, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
  if (a1 - a0 != b1 - b0) return false;
  const uint32_t n = a1 - a0;
  // 16 independent byte loads per side before any compare: one memory round trip per 16 bytes
  // instead of one per byte (the equal case — a verified duplicate — reads everything anyway)
  uint32_t i = 0;
  for (; i + 16 <= n; i += 16) {
    uint32_t diff = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) diff |= (uint32_t)(b[a0 + i + k] ^ b[b0 + i + k]);
    if (diff) return false;
  }
  uint32_t diff = 0;
  for (; i < n; ++i) diff |= (uint32_t)(b[a0 + i] ^ b[b0 + i]);
  return diff == 0;
}

// Table key of a byte span taken from the span itself: its length and its first and last
// min(8, len) bytes (spans of up to 16 bytes are covered whole). Equal spans get equal keys; unequal
// spans with one key only cost a byte comparison.
TB_HD uint64_t span_ends_key(const uint8_t* b, uint32_t s, uint32_t e) {
  const uint32_t len = e - s, m = len < 8u ? len : 8u;
  uint64_t head = 0, tail = 0;
  for (uint32_t k = 0; k < m; ++k) {
    head |= (uint64_t)b[s + k] << (8u * k);
    tail |= (uint64_t)b[e - m + k] << (8u * k);
  }
  return dev_key(head ^ (tail * kHashBase), len);
}

#if defined(__HIPCC__)
// dup_spans of a one-wave document with at most 64 spans: lane j keeps span j's start, length and
// first min(8, len) bytes in registers, and a uniform loop over i broadcasts span i to the lanes
// j > i. A lane that is still its own canonical element and has the same length and first bytes
// compares the rest of the bytes and, if they are equal, becomes a repeat of i. i only grows, so
// the first hit is the smallest equal index (canonicalize's definition), and an i that is itself a
// repeat is skipped: its equals were taken by its canonical element. No table, no canon[] array,
// no allocation. Every lane read and ballot sits in wave-uniform control flow (wb_pair_dword's
// rule); only the byte comparison runs divergent.
template <class P, class SpanF>
__device__ __forceinline__ void dup_spans_lanes(DocCtx<P>& x, const uint8_t* b, uint32_t n, SpanF&& span,
                                                int64_t* out_elems, int64_t* out_bytes) {
  const uint32_t lane = x.par.lane;
  uint32_t s = 0, len = 0, lo = 0, hi = 0;
  if (lane < n) {
    uint32_t e;
    span(lane, s, e);
    len = e - s;
    const uint32_t m = len < 8u ? len : 8u;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      if (k < m) lo |= (uint32_t)b[s + k] << (8u * k);
      if (k + 4 < m) hi |= (uint32_t)b[s + k + 4] << (8u * k);
    }
  }
  uint64_t dup = 0;  // bit j: span j repeats an earlier one (uniform)
  for (uint32_t i = 0; i + 1 < n; ++i) {
    if ((dup >> i) & 1ull) continue;
    const uint32_t si = (uint32_t)__builtin_amdgcn_readlane((int)s, (int)i);
    const uint32_t li = (uint32_t)__builtin_amdgcn_readlane((int)len, (int)i);
    const uint32_t loi = (uint32_t)__builtin_amdgcn_readlane((int)lo, (int)i);
    const uint32_t hii = (uint32_t)__builtin_amdgcn_readlane((int)hi, (int)i);
    bool hit = lane > i && lane < n && !((dup >> lane) & 1ull) && len == li && lo == loi && hi == hii;
    // The first 8 bytes are the signature: equal already. A plain byte loop, not bytes_eq: its
    // 16 loads in flight per side, inlined at the three call sites next to the table path's own
    // copy, took the kernel from 128 to 141 spilled VGPRs.
    if (hit) {
      uint32_t diff = 0;
#pragma unroll 1
      for (uint32_t k = 8; k < li; ++k) diff |= (uint32_t)(b[si + k] ^ b[s + k]);
      hit = diff == 0;
    }
    dup |= __ballot(hit);
  }
  *out_elems = (int64_t)__popcll(dup);
  *out_bytes = (int64_t)x.par.template wave_sum<uint32_t>(((dup >> lane) & 1ull) ? len : 0u);
}
#endif

// find_duplicates over byte spans [s[i], e[i]): (#repeats, sum of repeat byte lengths).
// The prefix hashes `ph` key the table of the workgroup kernels and of the host emulation. A
// one-wave document never reads them: up to 64 spans are compared lane against lane
// (dup_spans_lanes), more go through the same table keyed by the spans' own ends (span_ends_key).
// The key decides nothing either way: every table hit is verified by bytes_eq.
template <class P, class SpanF>
TB_HD void dup_spans(DocCtx<P>& x, const uint8_t* b, const PHView& ph, uint32_t n, SpanF&& span,
                     int64_t* out_elems, int64_t* out_bytes) {
  if (n <= 1) {  // one span (a single line / paragraph) repeats nothing: no table, no scans
    *out_elems = 0;
    *out_bytes = 0;
    return;
  }
#if defined(__HIPCC__)
  if constexpr (P::kWaves == 1) {
    if (n <= 64) {
      dup_spans_lanes(x, b, n, span, out_elems, out_bytes);
      return;
    }
  }
#endif
  const auto mark = x.mark();
  uint32_t* canon = x.template alloc_hot<uint32_t>(n + 1);
  if (x.overflow) return;
  canonicalize(
      x, n,
      [&](uint32_t i) {
        uint32_t s, e;
        span(i, s, e);
        if constexpr (P::kWaves == 1) return span_ends_key(b, s, e);
        else return dev_key(span_hash8(x, ph, s, e), e - s);
      },
      [&](uint32_t i, uint32_t j) {
        uint32_t s0, e0, s1, e1;
        span(i, s0, e0);
        span(j, s1, e1);
        return bytes_eq<P>(b, s0, e0, s1, e1);
      },
      canon);
  *out_elems = x.par.template sum<int64_t>(n, [&](uint32_t i) { return canon[i] != i ? (int64_t)1 : (int64_t)0; });
  *out_bytes = x.par.template sum<int64_t>(n, [&](uint32_t i) {
    if (canon[i] == i) return (int64_t)0;
    uint32_t s, e;
    span(i, s, e);
    return (int64_t)(e - s);
  });
  x.reset(mark);
}

}  // namespace tb
