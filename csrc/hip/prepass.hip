// The hash power table, and the pre-pass of very long documents: their code points, word-break
// marks and GopherRepetition word arrays, spread over many workgroups before their stage
// workgroups run. (kernel_common.h: the families, the launch ABI.)
#include "kernel_common.h"

#include "../common/doc_dedup.h"
#include "../common/doc_text.h"

namespace {

__global__ void k_pow_table(uint64_t* pw, uint32_t n) {
  // pw[i] = B^i and pw[n + 1 + i] = B^-i, computed independently per element (exact modular
  // arithmetic); the buffer holds 2n + 2 entries
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n) {
    pw[i] = hpow(kHashBase, i);
    pw[n + 1 + i] = hpow(kHashBaseInv, i);
  }
}

}  // namespace

extern "C" {

int tb_pow_table(hipStream_t stream, uint64_t* pw, uint32_t n) {
  hipLaunchKernelGGL(k_pow_table, dim3((n + 256) / 256), dim3(256), 0, stream, pw, n);
  return (int)hipGetLastError();
}

}  // extern "C"

namespace {

// the code points and UAX#29 word-break marks of very long documents, spread over
// many workgroups before their stage workgroups run (StageOut::pre). Launch grids are
// (tile or chunk, document): k_pre_count counts the lead bytes of every 16 KB tile, k_pre_decode
// writes each tile's code points at the offset its earlier tiles give (the non-packed Cps layout
// decode() produces for documents of 64 KiB and more), k_pre_wb evaluates word_mark() for 64 code
// points per wave (the rules look across tile borders freely: the whole property array exists).
constexpr uint32_t kPreTile = 16384;
constexpr uint32_t kPreThreads = 256;  // 64 bytes per thread

__global__ __launch_bounds__(kPreThreads) void k_pre_count(const uint8_t* __restrict__ bytes,
                                                           const int64_t* __restrict__ off,
                                                           const int32_t* __restrict__ perm,
                                                           const uint8_t* __restrict__ dead,
                                                           const PreDoc* __restrict__ pre, uint32_t tiles_max,
                                                           int64_t* __restrict__ cnt) {
  __shared__ uint32_t red[kPreThreads / 64];
  const uint32_t j = blockIdx.x, s = blockIdx.y;
  const int doc = perm[s];
  const uint32_t n = pre[s].n;
  const uint32_t b0 = j * kPreTile;
  if (b0 >= n || (dead && dead[doc]) || off[doc + 1] - off[doc] != (int64_t)n) return;
  const uint8_t* b = bytes + off[doc];
  const uint32_t e = b0 + kPreTile < n ? b0 + kPreTile : n;
  // code points (low half) and runs of '\n' (high half)
  uint32_t c = 0;
  for (uint32_t i = b0 + threadIdx.x; i < e; i += kPreThreads) {
    const uint8_t v = b[i];
    c += utf8_is_lead(v) ? 1u : 0u;
    if (v == '\n' && (i == 0 || b[i - 1] != '\n')) c += 1u << 16;
  }
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (uint32_t w = 0; w < kPreThreads / 64; ++w) t += red[w];
    cnt[(size_t)s * tiles_max + j] = t;  // both halves < 2^16: a tile is 16 KB
  }
}

__global__ __launch_bounds__(kPreThreads) void k_pre_decode(const uint8_t* __restrict__ bytes,
                                                            const int64_t* __restrict__ off,
                                                            const int32_t* __restrict__ perm,
                                                            const uint8_t* __restrict__ dead, PreDoc* pre,
                                                            uint32_t tiles_max, const int64_t* __restrict__ cnt,
                                                            DevTables tabs) {
  __shared__ uint32_t xs[kPreThreads + 1];
  __shared__ uint32_t ys[kPreThreads + 1];
  const uint32_t j = blockIdx.x, s = blockIdx.y;
  const int doc = perm[s];
  const PreDoc d = pre[s];
  const uint32_t n = d.n;
  const uint32_t b0 = j * kPreTile;
  if (b0 >= n || (dead && dead[doc]) || off[doc + 1] - off[doc] != (int64_t)n) return;
  const uint8_t* b = bytes + off[doc];
  const UcdView ucd{tabs.s1, tabs.s2, tabs.l1, tabs.l2};
  // this thread's 64 bytes, loaded at once (16 independent loads): lead count, then the
  // block's exclusive scan of the counts
  const uint32_t t0 = b0 + 64 * threadIdx.x;
  const uint32_t t1 = t0 + 64 < n ? t0 + 64 : n;
  uint32_t v[16];
#pragma unroll
  for (uint32_t q = 0; q < 16; ++q) {
    uint32_t w = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t i = t0 + 4 * q + k;
      w |= (i < t1 ? (uint32_t)b[i] : 0u) << (8 * k);
    }
    v[q] = w;
  }
  auto byte_of = [&](uint32_t i) -> uint32_t { return (v[(i - t0) >> 2] >> (8 * ((i - t0) & 3))) & 0xFFu; };
  uint32_t prev = (t0 > 0 && t0 < n) ? (uint32_t)b[t0 - 1] : 0u;
  uint32_t c = 0, pv = prev;
  for (uint32_t i = t0; i < t1; ++i) {
    const uint32_t c0 = byte_of(i);
    c += utf8_is_lead((uint8_t)c0) ? 1u : 0u;
    if (c0 == '\n' && (i == 0 || pv != '\n')) c += 1u << 16;
    pv = c0;
  }
  xs[threadIdx.x] = c;  // code points | runs << 16 (< 2^16 each: 64 bytes)
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t bc = 0, br = 0;
    for (uint32_t q = 0; q < j; ++q) {
      const uint32_t t = (uint32_t)cnt[(size_t)s * tiles_max + q];
      bc += t & 0xFFFFu;
      br += t >> 16;
    }
    for (uint32_t q = 0; q < kPreThreads; ++q) {
      const uint32_t t = xs[q];
      xs[q] = bc;
      ys[q] = br;
      bc += t & 0xFFFFu;
      br += t >> 16;
    }
    xs[kPreThreads] = bc;  // code points and runs before the next tile
    ys[kPreThreads] = br;
  }
  __syncthreads();
  uint32_t k = xs[threadIdx.x], kr = ys[threadIdx.x];
  bool dict = false;
  uint32_t fs = 0xFFFFFFFFu, le = 0;  // first / one past the last non-whitespace code point
  pv = prev;
  for (uint32_t i = t0; i < t1; ++i) {
    const uint32_t c0 = byte_of(i);
    const uint32_t last = pv;
    pv = c0;
    if (!utf8_is_lead((uint8_t)c0)) continue;
    if (c0 == '\n' && (i == 0 || last != '\n')) {  // a run of '\n' starts at code point k
      uint32_t q = i + 1;
      while (q < n && b[q] == '\n') ++q;
      d.nl_pos[kr] = k;
      d.nl_len[kr] = q - i;
      ++kr;
    }
    int len;
    const uint32_t p = ucd.props(c0 < 0x80 ? c0 : utf8_decode(b, i, n, &len));
    d.off[k] = i;
    d.prop[k] = compact_prop(p);
    dict |= (p & P_DICT) != 0;
    if (!is_ws(compact_prop(p))) {
      fs = k < fs ? k : fs;
      le = k + 1;
    }
    ++k;
  }
  if (dict) atomicOr(&pre[s].dict, 1u);
  if (le) {
    atomicMin(&pre[s].tcs, fs);
    atomicMax(&pre[s].tce, le);
  }
  if (threadIdx.x == 0 && b0 + kPreTile >= n) {  // the last tile closes the arrays
    const uint32_t C = xs[kPreThreads];
    d.off[C] = n;
    d.prop[C] = 0;
    pre[s].C = C;
    pre[s].NL = ys[kPreThreads];
  }
}

__global__ __launch_bounds__(64) void k_pre_wb(const int32_t* __restrict__ perm, const uint8_t* __restrict__ dead,
                                               PreDoc* pre) {
  const uint32_t j = blockIdx.x, s = blockIdx.y;
  const PreDoc d = pre[s];
  const uint32_t C = d.C;
  if (64 * j > C || (dead && dead[perm[s]])) return;
  if (j == 0 && threadIdx.x == 0) {  // the runs of '\n' inside [tcs, tce) (gopher_rep_record)
    auto lower = [&](uint32_t v) {
      uint32_t lo = 0, hi = d.NL;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (d.nl_pos[mid] < v) lo = mid + 1; else hi = mid;
      }
      return lo;
    };
    pre[s].nl_a = lower(d.tcs);
    pre[s].nl_e = lower(d.tce);
  }
  const uint32_t i = 64 * j + threadIdx.x;
  const bool m = i <= C && word_mark(PropArr{nullptr, d.prop}, C, i);
  const uint64_t bits = __ballot(m);
  if (threadIdx.x < 2) d.wbm[2 * j + threadIdx.x] = threadIdx.x ? (uint32_t)(bits >> 32) : (uint32_t)bits;
}

// The pre-pass words (words() over the precomputed code points and marks), as a segmented scan
// spread over waves: MODE 0 writes every 64-code-point chunk's scan aggregate, k_pre_words_scan
// turns them into per-chunk carry-ins (one wave per document), MODE 1 counts the chunk's words,
// k_pre_words_scan (counts) gives each chunk its first word index, MODE 2 writes the words.
__device__ __forceinline__ WSeg pre_wseg_in(const PreDoc& d, uint32_t j) {
  const uint32_t p = d.prop[j];
  const bool ws = is_ws(p);
  const uint32_t bit = (d.wbm[j >> 5] >> (j & 31)) & 1u;
  return WSeg{bit | ((!(p & P_PUNCT) && !ws) ? 2u : 0u) | ((p & P_ALPHA) ? 4u : 0u), ws ? 0xFFFFFFFFu : j,
              ws ? 0u : j + 1};
}

template <int MODE>
__global__ __launch_bounds__(64) void k_pre_words(const int32_t* __restrict__ perm, const uint8_t* __restrict__ dead,
                                                  const PreDoc* __restrict__ pre) {
  const uint32_t c = blockIdx.x, s = blockIdx.y;
  const PreDoc d = pre[s];
  const uint32_t C = d.C;
  const uint32_t nch = (C + 63) / 64;
  if (c >= nch || (dead && dead[perm[s]])) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t j = 64 * c + lane;
  const WSeg id{0u, 0xFFFFFFFFu, 0u};
  const WSeg x = j < C ? pre_wseg_in(d, j) : id;
  const WSeg loc = pardetail::wave_incl_scan(x, lane, [](const WSeg& a, const WSeg& b) { return wseg_op(a, b); });
  if (MODE == 0) {
    if (lane == 63) {
      d.wtmp[3 * c] = loc.bits;
      d.wtmp[3 * c + 1] = loc.first;
      d.wtmp[3 * c + 2] = loc.last;
    }
    return;
  }
  const uint32_t* cin = d.wtmp + 3 * (size_t)nch;
  const WSeg carry{cin[3 * c], cin[3 * c + 1], cin[3 * c + 2]};
  const WSeg in = wseg_op(carry, loc);
  const bool sel = j < C && ((d.wbm[(j + 1) >> 5] >> ((j + 1) & 31)) & 1u) && (in.bits & 2u);
  const uint64_t m = __ballot(sel);
  uint32_t* wcnt = d.wtmp + 6 * (size_t)nch;
  if (MODE == 1) {
    if (lane == 0) wcnt[c] = (uint32_t)__popcll(m);
    return;
  }
  if (sel) {
    const uint32_t* wbase = wcnt + nch;
    const uint32_t k = wbase[c] + (uint32_t)__popcll(m & (lane ? (~0ull >> (64 - lane)) : 0ull));
    d.wcs[k] = in.first;
    d.wce[k] = in.last;
    d.wbs[k] = d.off[in.first];
    d.wbe[k] = d.off[in.last];
    d.wal[k] = (in.bits & 4u) ? 1 : 0;
  }
}

// One wave per document: MODE 0 scans the chunk aggregates into carry-ins (exclusive), MODE 1 the
// word counts into first word indices (and W).
template <int MODE>
__global__ __launch_bounds__(64) void k_pre_words_scan(const int32_t* __restrict__ perm,
                                                       const uint8_t* __restrict__ dead, PreDoc* pre) {
  const uint32_t s = blockIdx.x;
  const PreDoc d = pre[s];
  if (dead && dead[perm[s]]) return;
  const uint32_t nch = (d.C + 63) / 64;
  const uint32_t lane = threadIdx.x;
  if (MODE == 0) {
    const WSeg id{0u, 0xFFFFFFFFu, 0u};
    auto op = [](const WSeg& a, const WSeg& b) { return wseg_op(a, b); };
    WSeg carry = id;
    uint32_t* cin = d.wtmp + 3 * (size_t)nch;
    for (uint32_t b0 = 0; b0 < nch; b0 += 64) {
      const uint32_t q = b0 + lane;
      const WSeg v = q < nch ? WSeg{d.wtmp[3 * q], d.wtmp[3 * q + 1], d.wtmp[3 * q + 2]} : id;
      const WSeg incl = pardetail::wave_incl_scan(v, lane, op);
      WSeg excl = pardetail::shfl_up_t(incl, 1);
      if (lane == 0) excl = id;
      const WSeg e = op(carry, excl);
      if (q < nch) {
        cin[3 * q] = e.bits;
        cin[3 * q + 1] = e.first;
        cin[3 * q + 2] = e.last;
      }
      carry = op(carry, pardetail::bcast63(incl));
    }
  } else {
    uint32_t* wcnt = d.wtmp + 6 * (size_t)nch;
    uint32_t* wbase = wcnt + nch;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < nch; b0 += 64) {
      const uint32_t q = b0 + lane;
      const uint32_t v = q < nch ? wcnt[q] : 0u;
      const uint32_t incl = pardetail::wave_incl_scan(v, lane, [](uint32_t a, uint32_t b) { return a + b; });
      if (q < nch) wbase[q] = carry + incl - v;
      carry += pardetail::bcast63(incl);
    }
    if (lane == 0) pre[s].W = carry;
  }
}

}  // namespace

extern "C" {

size_t tb_sizeof_pre_doc() { return sizeof(PreDoc); }

// Decode + word-break marks of the first npre launch positions of the long-document launch
// (`pre`: npre descriptors with n / off / prop / wbm set, C and dict zeroed; cnt: int64
// [npre * tiles_max], tiles_max >= ceil(max n / 16 KB)).
int tb_pre_decode(hipStream_t stream, const TbDocs* d, void* pre, uint32_t tiles_max, int64_t* cnt,
                  const TbTables* tb) {
  const uint8_t *bytes = d->bytes, *dead = d->dead;
  const int64_t* off = d->off;
  const int32_t* perm = d->perm;
  const int32_t npre = d->n_launch;
  if (npre <= 0) return 0;
  if (!perm || !pre || !cnt || tiles_max == 0 || npre > 65535) return (int)hipErrorInvalidValue;
  const dim3 g(tiles_max, (uint32_t)npre);
  hipLaunchKernelGGL(k_pre_count, g, dim3(kPreThreads), 0, stream, bytes, off, perm, dead, (const PreDoc*)pre,
                     tiles_max, cnt);
  hipLaunchKernelGGL(k_pre_decode, g, dim3(kPreThreads), 0, stream, bytes, off, perm, dead, (PreDoc*)pre, tiles_max,
                     (const int64_t*)cnt, tb->ucd);
  // chunks of 64 code points: C + 1 <= n + 1 positions
  const uint32_t chunks = tiles_max * (kPreTile / 64) + 1;
  hipLaunchKernelGGL(k_pre_wb, dim3(chunks, (uint32_t)npre), dim3(64), 0, stream, perm, dead, (PreDoc*)pre);
  const dim3 gw(chunks, (uint32_t)npre);
  hipLaunchKernelGGL(k_pre_words<0>, gw, dim3(64), 0, stream, perm, dead, (const PreDoc*)pre);
  hipLaunchKernelGGL(k_pre_words_scan<0>, dim3((uint32_t)npre), dim3(64), 0, stream, perm, dead, (PreDoc*)pre);
  hipLaunchKernelGGL(k_pre_words<1>, gw, dim3(64), 0, stream, perm, dead, (const PreDoc*)pre);
  hipLaunchKernelGGL(k_pre_words_scan<1>, dim3((uint32_t)npre), dim3(64), 0, stream, perm, dead, (PreDoc*)pre);
  hipLaunchKernelGGL(k_pre_words<2>, gw, dim3(64), 0, stream, perm, dead, (const PreDoc*)pre);
  return (int)hipGetLastError();
}

}  // extern "C"

namespace {

// SURVEY 5.7, GopherRepetition's word arrays of the pre-pass documents over many workgroups
// (gopher_rep_record computes the same in the document's own workgroup for the others): per
// chunk of 2048 words (256 threads, 8 consecutive words each)
//   MODE 0  zero the canonicalisation table (1.5 W + 2 slots of 64 bits)
//   MODE 1  word hash (the polynomial hash of its bytes = span_hash8), insert into the table
//           (fingerprint | smallest index + 1, CAS + atomic min: canonicalize()'s 64-bit path),
//           chunk sum of the word lengths
//   MODE 2  canonical id (verified byte-equal; a collision flags the document for the CPU path),
//           WL / PB from the chunk's length base, chunk sum of wh[k] B^-WL[k+1]
//   MODE 3  K from the chunk's base of those terms
// with k_pre_wsum (one wave per document) turning chunk sums into bases between the passes.
constexpr uint32_t kPreWChunk = 2048;
constexpr uint32_t kPreWThreads = 256;
constexpr uint32_t kPreWPer = kPreWChunk / kPreWThreads;
constexpr uint32_t kPreWTabChunk = 3072;  // table slots zeroed per workgroup (1.5 x a chunk)

__device__ __forceinline__ uint64_t pow_at(const uint64_t* pw, uint32_t pw_n, uint32_t k) {
  return k <= pw_n ? pw[k] : hpow(kHashBase, k);
}
__device__ __forceinline__ uint64_t ipow_at(const uint64_t* pw, uint32_t pw_n, uint32_t k) {
  return k <= pw_n ? pw[pw_n + 1 + k] : hpow(kHashBaseInv, k);
}

// exclusive block scan (kPreWThreads threads) of one value per thread; *tot = the block total
template <class T>
__device__ __forceinline__ T pre_block_scan(T v, T* sh, T* tot) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const T incl = pardetail::wave_incl_scan(v, lane, [](T a, T b) { return a + b; });
  if (lane == 63) sh[w] = incl;
  __syncthreads();
  T base = 0, all = 0;
#pragma unroll
  for (uint32_t q = 0; q < kPreWThreads / 64; ++q) {
    if (q < w) base += sh[q];
    all += sh[q];
  }
  __syncthreads();
  *tot = all;
  return base + incl - v;
}

template <int MODE>
__global__ __launch_bounds__(kPreWThreads) void k_pre_wcanon(const uint8_t* __restrict__ bytes,
                                                             const int64_t* __restrict__ off,
                                                             const int32_t* __restrict__ perm,
                                                             const uint8_t* __restrict__ dead,
                                                             const PreDoc* __restrict__ pre,
                                                             const uint64_t* __restrict__ pw, uint32_t pw_n,
                                                             uint32_t* flags) {
  __shared__ uint64_t sh[kPreWThreads / 64];
  const uint32_t c = blockIdx.x, s = blockIdx.y;
  const int doc = perm[s];
  if (dead && dead[doc]) return;
  const PreDoc d = pre[s];
  const uint32_t W = d.W;
  const uint32_t nch = (W + kPreWChunk - 1) / kPreWChunk;
  const uint32_t capn = W + (W >> 1) + 2;
  if (MODE == 0) {
    const uint32_t a = c * kPreWTabChunk;
    for (uint32_t i = a + threadIdx.x; i < capn && i < a + kPreWTabChunk; i += kPreWThreads) d.wtab[i] = 0;
    return;
  }
  if (c >= (nch ? nch : 1u)) return;  // (W == 0: chunk 0 writes the closing entries)
  const uint8_t* b = bytes + off[doc];
  const uint32_t t0 = c * kPreWChunk + threadIdx.x * kPreWPer;
  uint32_t len[kPreWPer];
  uint32_t lsum = 0;
#pragma unroll
  for (uint32_t j = 0; j < kPreWPer; ++j) {
    const uint32_t k = t0 + j;
    len[j] = k < W ? d.wbe[k] - d.wbs[k] : 0u;
    lsum += len[j];
  }
  if (MODE == 1) {
#pragma unroll
    for (uint32_t j = 0; j < kPreWPer; ++j) {
      const uint32_t k = t0 + j;
      if (k >= W) break;
      const uint32_t bs = d.wbs[k], be = d.wbe[k];
      uint64_t h = 0;
      for (uint32_t q = bs; q < be; ++q) h = hash_push(h, b[q]);
      d.wh[k] = h;
      const uint64_t key = dev_key(h, be - bs);
      const uint64_t fp = (key >> 32) | 1ull;
      const uint64_t mine = (fp << 32) | (uint64_t)(k + 1);
      uint32_t slot = (uint32_t)(((key & 0xFFFFFFFFull) * capn) >> 32);
      while (true) {
        unsigned long long cur = d.wtab[slot];
        if (cur == 0) {
          cur = atomicCAS((unsigned long long*)&d.wtab[slot], 0ull, (unsigned long long)mine);
          if (cur == 0) break;
        }
        if ((cur >> 32) == fp) {
          if ((cur & 0xFFFFFFFFull) > (uint64_t)k + 1u) atomicMin((unsigned long long*)&d.wtab[slot], mine);
          break;
        }
        if (++slot == capn) slot = 0;
      }
      d.wslot[k] = slot;
    }
    uint64_t tot;
    (void)pre_block_scan<uint64_t>(lsum, sh, &tot);
    if (threadIdx.x == 0) d.wcsum[c] = tot;
    return;
  }
  // MODE 2 / 3: this thread's first word's WL from the chunk base + the block scan
  uint64_t tot;
  const uint64_t lbase = (nch ? d.wcsum[nch + c] : 0ull) + pre_block_scan<uint64_t>(lsum, sh, &tot);
  if (MODE == 2) {
    uint32_t wl = (uint32_t)lbase;
    uint64_t tsum = 0;
    bool bad = false;
#pragma unroll
    for (uint32_t j = 0; j < kPreWPer; ++j) {
      const uint32_t k = t0 + j;
      if (k >= W) break;
      d.wl[k] = wl;
      d.wpb[k] = pow_at(pw, pw_n, wl);
      uint32_t cc = (uint32_t)(d.wtab[d.wslot[k]] & 0xFFFFFFFFull) - 1u;
      if (cc != k && !bytes_eq<WavePar>(b, d.wbs[k], d.wbe[k], d.wbs[cc], d.wbe[cc])) {
        bad = true;
        cc = k;
      }
      d.wid[k] = cc;
      wl += len[j];
      tsum += d.wh[k] * ipow_at(pw, pw_n, wl);
    }
    if (bad) atomicOr(&flags[doc], DOC_NEEDS_CPU);
    uint64_t ttot;
    (void)pre_block_scan<uint64_t>(tsum, sh, &ttot);
    if (threadIdx.x == 0) {
      if (nch) d.wcsum[2 * nch + c] = ttot;
      if (c + 1 >= nch) {  // the closing entries
        const uint32_t total = (uint32_t)((nch ? d.wcsum[nch + c] : 0ull) + tot);
        d.wl[W] = total;
        d.wpb[W] = pow_at(pw, pw_n, total);
      }
    }
    return;
  }
  // MODE 3
  uint32_t wl = (uint32_t)lbase;
  uint64_t t[kPreWPer];
  uint64_t tsum = 0;
#pragma unroll
  for (uint32_t j = 0; j < kPreWPer; ++j) {
    const uint32_t k = t0 + j;
    wl += len[j];
    t[j] = k < W ? d.wh[k] * ipow_at(pw, pw_n, wl) : 0ull;
    tsum += t[j];
  }
  uint64_t ttot;
  uint64_t kb = (nch ? d.wcsum[3 * nch + c] : 0ull) + pre_block_scan<uint64_t>(tsum, sh, &ttot);
#pragma unroll
  for (uint32_t j = 0; j < kPreWPer; ++j) {
    const uint32_t k = t0 + j;
    if (k >= W) break;
    d.wk[k] = kb;
    kb += t[j];
  }
  if (threadIdx.x == 0 && c + 1 >= nch) d.wk[W] = (nch ? d.wcsum[3 * nch + c] : 0ull) + ttot;
}

// One wave per document: exclusive scans of the chunk sums (MODE 0: lengths [0, nch) -> [nch, 2 nch);
// MODE 1: K terms [2 nch, 3 nch) -> [3 nch, 4 nch)); MODE 1 also marks the arrays ready.
template <int MODE>
__global__ __launch_bounds__(64) void k_pre_wsum(const int32_t* __restrict__ perm, const uint8_t* __restrict__ dead,
                                                 PreDoc* pre) {
  const uint32_t s = blockIdx.x;
  if (dead && dead[perm[s]]) return;
  const PreDoc d = pre[s];
  const uint32_t nch = (d.W + kPreWChunk - 1) / kPreWChunk;
  const uint32_t lane = threadIdx.x;
  const uint64_t* in = d.wcsum + (MODE ? 2 * nch : 0);
  uint64_t* out = d.wcsum + (MODE ? 3 * nch : nch);
  uint64_t carry = 0;
  for (uint32_t b0 = 0; b0 < nch; b0 += 64) {
    const uint32_t q = b0 + lane;
    const uint64_t v = q < nch ? in[q] : 0ull;
    const uint64_t incl = pardetail::wave_incl_scan(v, lane, [](uint64_t a, uint64_t b) { return a + b; });
    if (q < nch) out[q] = carry + incl - v;
    carry += pardetail::bcast63(incl);
  }
  if (MODE == 1 && lane == 0) pre[s].wready = 1;
}

}  // namespace

extern "C" {

// GopherRepetition word arrays of the npre pre-pass documents (after tb_pre_decode; the
// descriptors' wh / wtab / wk / wpb / wcsum / wslot / wid / wl hold [W + 1]-sized buffers,
// wtab [1.5 W + 2], wcsum [4 chunks]; chunks_max >= ceil(max W / 2048)).
int tb_pre_wcanon(hipStream_t stream, const TbDocs* d, void* pre, uint32_t chunks_max, const TbTables* tb,
                  uint32_t* flags) {
  const uint8_t *bytes = d->bytes, *dead = d->dead;
  const int64_t* off = d->off;
  const int32_t* perm = d->perm;
  const int32_t npre = d->n_launch;
  const uint64_t* pw = tb->pw;
  const uint32_t pw_n = tb->pw_n;
  if (npre <= 0) return 0;
  if (!perm || !pre || !pw || !flags || chunks_max == 0 || npre > 65535) return (int)hipErrorInvalidValue;
  const PreDoc* p = (const PreDoc*)pre;
  const dim3 gz(chunks_max + 1, (uint32_t)npre), g(chunks_max, (uint32_t)npre);
  hipLaunchKernelGGL(k_pre_wcanon<0>, gz, dim3(kPreWThreads), 0, stream, bytes, off, perm, dead, p, pw, pw_n, flags);
  hipLaunchKernelGGL(k_pre_wcanon<1>, g, dim3(kPreWThreads), 0, stream, bytes, off, perm, dead, p, pw, pw_n, flags);
  hipLaunchKernelGGL(k_pre_wsum<0>, dim3((uint32_t)npre), dim3(64), 0, stream, perm, dead, (PreDoc*)pre);
  hipLaunchKernelGGL(k_pre_wcanon<2>, g, dim3(kPreWThreads), 0, stream, bytes, off, perm, dead, p, pw, pw_n, flags);
  hipLaunchKernelGGL(k_pre_wsum<1>, dim3((uint32_t)npre), dim3(64), 0, stream, perm, dead, (PreDoc*)pre);
  hipLaunchKernelGGL(k_pre_wcanon<3>, g, dim3(kPreWThreads), 0, stream, bytes, off, perm, dead, p, pw, pw_n, flags);
  return (int)hipGetLastError();
}

}  // extern "C"
