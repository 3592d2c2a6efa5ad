// TokenCounter on the device (csrc/common/bpe.h): token counts of the kept outputs of K16.
//
// One wave per document (grid-stride over the documents). After k_compact the kept documents'
// final contents sit contiguously at the front of the output buffer, in document order; their
// number is the last entry of the kept-count scan, read here on the device, so counting follows
// compaction on the same stream with no host round trip. Each lane takes a 1/64 byte range of the
// document, finds the first pre-token start in it from the local boundary rules
// (bpe_first_start), and tokenizes + merges the pre-tokens that start in its range; the counts
// are summed across the wave. A lane's merge arrays live in LDS, interleaved by lane (element i
// of lane t at i * 64 + t: consecutive lanes, consecutive banks), 32 KB per 64-lane workgroup.
// A pre-token over those 64-byte arrays marks the document kBpeLong; k_bpe_long then recounts it
// with one wave per long pre-token (merge arrays of kBpeMaxLong entries, the minimum search spread
// over the wave).
//
// Both kernels are written once over the pre-tokenizer policy (csrc/common/bpe.h): k_bpe_count /
// k_bpe_long are the GPT-2 instantiation, k_bpe_split_count / k_bpe_split_long the split-regex
// one (csrc/common/bpe_split.h: Llama-3, cl100k_base, Qwen2), whose lanes start at their range's
// first sync point and stop at the next lane's. k_bpe_split_count_nfc is k_bpe_split_count for a
// tokenizer whose normalizer is NFC: each lane also runs the quick check (bpe_nfc_range) over the
// code points of its byte range, and a document that fails it goes to the host; the check is a
// compile-time parameter of the body, so the other kernels carry none of it. k_bpe_case_count /
// k_bpe_case_count_nfc / k_bpe_case_long are the instantiation for the case-aware patterns of
// o200k_base and Tekken (csrc/common/bpe_case.h). k_bpe_sp_count / k_bpe_sp_long are the one for the
// character-level BPE of the SentencePiece conversions (csrc/common/bpe_sp.h: Llama-2, Mistral,
// Gemma): chunk starts are local, as GPT-2's, and the policy supplies a chunk's initial symbols
// (code points looked up through the cache, <0xNN> ids for the others, the prepended U+2581).
//
// The parameter block DevBpe comes ready from the host module (csrc/host/tok_params.h
// bpe_fill_params, the filler of the host emulation's block too, here with HBM addresses);
// tb_bpe_count only asks bpe_params_ok (csrc/common/bpe.h) whether the kernels can run on it.
#include <hip/hip_runtime.h>

#include "../common/bpe_case.h"
#include "../common/bpe_sp.h"

using namespace tb;

namespace {

constexpr int kBpeLanes = 64;
constexpr int kBpeMinChunk = 16;  // bytes per lane at least (short documents use fewer lanes)
constexpr int kBpeGrid = 8192;

// next lane's value (the last lane: its own)
__device__ __forceinline__ int64_t lane_next_i64(int64_t x) {
  const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)x, 1, kBpeLanes);
  const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)((uint64_t)x >> 32), 1, kBpeLanes);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

// A lane's tokens start in [lo, hi): BpeGpt2 finds lo locally and stops at its byte range's end;
// BpeSplit (csrc/common/bpe_split.h) has lo = sync(s0) and hi = the next lane's lo, passed down
// the wave instead of searched twice (lanes past the document hold len). -1 in *lo: invalid UTF-8.
template <class P>
__device__ __forceinline__ void lane_span(const DevBpe& T, const uint8_t* b, int64_t len, int64_t s0, int64_t s1,
                                          int t, int64_t* lo, int64_t* hi) {
  if (!P::kSyncSplit) {
    *lo = s0;  // (bpe_count_range resolves both ends)
    *hi = s1;
    return;
  }
  int64_t a = len;
  if (s0 < len) a = t == 0 ? 0 : P::first_start(T, b, len, s0);
  const int64_t nx = lane_next_i64(a < 0 ? len : a);
  *lo = a;
  *hi = t == kBpeLanes - 1 ? len : nx;
}

template <bool kMerge, class P, class LongF>
__device__ __forceinline__ int64_t lane_count(const DevBpe& T, const uint8_t* b, int64_t len, int64_t lo, int64_t hi,
                                              BpeArr c, BpeArr r, LongF&& on_long) {
  if (!P::kSyncSplit) return bpe_count_range<kMerge, P>(T, b, len, lo, hi, c, r, on_long);
  if (lo < 0) return -1;
  return bpe_count_span<kMerge, P>(T, b, len, lo, hi, c, r, on_long);
}

template <class P, bool kNfc = false>
__device__ __forceinline__ void bpe_count_body(const DevBpe& T, const uint8_t* __restrict__ text,
                                               const int64_t* __restrict__ off, const int64_t* __restrict__ n_dev,
                                               int32_t n_max, int32_t* __restrict__ counts) {
  __shared__ uint32_t cs[kBpeMaxWord * kBpeLanes];
  __shared__ uint32_t rs[kBpeMaxWord * kBpeLanes];
  const int t = threadIdx.x;
  int64_t n = n_max;
  if (n_dev != nullptr) n = min(n, *n_dev);
  for (int64_t k = blockIdx.x; k < n; k += gridDim.x) {
    const int64_t s = off[k];
    const int64_t len = off[k + 1] - s;
    const uint8_t* b = text + s;
    const int64_t chunk = max((int64_t)kBpeMinChunk, (len + kBpeLanes - 1) / kBpeLanes);
    const int64_t s0 = (int64_t)t * chunk;
    const int64_t s1 = min(len, s0 + chunk);
    long long cnt = 0;
    int bad = 0, lng = 0;
    int64_t lo, hi;
    lane_span<P>(T, b, len, s0, s1, t, &lo, &hi);
    if (s0 < len) {
      if (T.n_added && P::has_added(T, b, len, s0, s1)) {
        bad = 1;
      } else if (kNfc && bpe_nfc_range(T, b, len, s0, s1) != 1) {
        bad = 1;
      } else {
        const int64_t x = lane_count<true, P>(T, b, len, lo, hi, BpeArr{cs + t, kBpeLanes}, BpeArr{rs + t, kBpeLanes},
                                              [&](int64_t, int64_t) -> int64_t {
                                                lng = 1;
                                                return 0;
                                              });
        if (x < 0) bad = 1;
        else cnt = x;
      }
    }
    const bool any_bad = __ballot(bad) != 0, any_long = __ballot(lng) != 0;
    for (int o = kBpeLanes / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, kBpeLanes);
    if (t == 0) {
      const long long tot = cnt + T.post_add;
      // (long pre-tokens: the tokens of the others travel in the count, k_bpe_long adds theirs)
      counts[k] = (any_bad || tot > 0x7FFFFFFF) ? kBpeHost : any_long ? (int32_t)(kBpeLong - tot) : (int32_t)tot;
    }
  }
}

__global__ __launch_bounds__(kBpeLanes) void k_bpe_count(DevBpe T, const uint8_t* __restrict__ text,
                                                         const int64_t* __restrict__ off,
                                                         const int64_t* __restrict__ n_dev, int32_t n_max,
                                                         int32_t* __restrict__ counts) {
  bpe_count_body<BpeGpt2>(T, text, off, n_dev, n_max, counts);
}

// k_bpe_count for the split-regex family (patterns A and B, T.kind)
__global__ __launch_bounds__(kBpeLanes) void k_bpe_split_count(DevBpe T, const uint8_t* __restrict__ text,
                                                               const int64_t* __restrict__ off,
                                                               const int64_t* __restrict__ n_dev, int32_t n_max,
                                                               int32_t* __restrict__ counts) {
  bpe_count_body<BpeSplit>(T, text, off, n_dev, n_max, counts);
}

// k_bpe_split_count behind the NFC gate (T.nfc)
__global__ __launch_bounds__(kBpeLanes) void k_bpe_split_count_nfc(DevBpe T, const uint8_t* __restrict__ text,
                                                                   const int64_t* __restrict__ off,
                                                                   const int64_t* __restrict__ n_dev, int32_t n_max,
                                                                   int32_t* __restrict__ counts) {
  bpe_count_body<BpeSplit, true>(T, text, off, n_dev, n_max, counts);
}

// k_bpe_count for the case-aware split patterns (C and D, T.kind), and behind the NFC gate
__global__ __launch_bounds__(kBpeLanes) void k_bpe_case_count(DevBpe T, const uint8_t* __restrict__ text,
                                                              const int64_t* __restrict__ off,
                                                              const int64_t* __restrict__ n_dev, int32_t n_max,
                                                              int32_t* __restrict__ counts) {
  bpe_count_body<BpeCase>(T, text, off, n_dev, n_max, counts);
}

__global__ __launch_bounds__(kBpeLanes) void k_bpe_case_count_nfc(DevBpe T, const uint8_t* __restrict__ text,
                                                                  const int64_t* __restrict__ off,
                                                                  const int64_t* __restrict__ n_dev, int32_t n_max,
                                                                  int32_t* __restrict__ counts) {
  bpe_count_body<BpeCase, true>(T, text, off, n_dev, n_max, counts);
}

// k_bpe_count for the SentencePiece-style character-level BPE (T.sp_flags: the layout)
__global__ __launch_bounds__(kBpeLanes) void k_bpe_sp_count(DevBpe T, const uint8_t* __restrict__ text,
                                                            const int64_t* __restrict__ off,
                                                            const int64_t* __restrict__ n_dev, int32_t n_max,
                                                            int32_t* __restrict__ counts) {
  bpe_count_body<BpeSp>(T, text, off, n_dev, n_max, counts);
}

constexpr int kBpeLongList = 32;  // long pre-tokens of one document counted on the device

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t x) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t y = ((uint64_t)(uint32_t)__shfl_xor((int)(x >> 32), o) << 32) | (uint32_t)__shfl_xor((int)x, o);
    x = y < x ? y : x;
  }
  return x;
}

// The initial symbols of a BpeSp chunk (csrc/common/bpe_sp.h) for bpe_word_long_wave, the lanes
// taking code points side by side: the symbol of the code point at byte i sits at slot i + lead
// (slot 0: the prepended U+2581), linked to the slot after its last byte; the slots of its other
// bytes are dead (nx = -1, no pair) unless it falls back to one <0xNN> symbol per byte. Returns
// the number of symbols (the same in every lane); Lt = L + lead slots are in use.
__device__ int bpe_sp_symbols_wave(const DevBpe& T, const uint8_t* w, int L, int lead, uint32_t* c, uint64_t* v,
                                   int16_t* nx, int16_t* pv, int lane) {
  const int Lt = L + lead;
  int cnt = 0;
  if (lane == 0) {
    pv[0] = -1;
    if (lead) {
      c[0] = T.sp_id;
      nx[0] = 1;
      cnt = 1;
    }
  }
  for (int i = lane; i < L; i += 64) {
    if ((w[i] & 0xC0) == 0x80) continue;  // (the chunk is valid UTF-8: its code point's lane writes this slot)
    int l = 1;
    const int32_t cp = bpe_decode(w, i, L, &l);
    const uint32_t id = cp < 0 ? kBpeSpNone : bpe_sp_symbol(T, (uint32_t)cp);
    const int q = i + lead;
    if (id != kBpeSpNone) {
      c[q] = id;
      nx[q] = (int16_t)(q + l);
      for (int j = 1; j < l; ++j) nx[q + j] = -1;
      ++cnt;
    } else {
      for (int j = 0; j < l; ++j) {
        c[q + j] = T.byte_id[w[i + j]];
        nx[q + j] = (int16_t)(q + j + 1);
      }
      cnt += l;
    }
  }
  __syncthreads();
  for (int i = lane; i < Lt; i += 64) {
    const int j = nx[i];
    if (j >= 0 && j < Lt) pv[j] = (int16_t)i;  // (every live slot but the first has one predecessor)
    v[i] = (j >= 0 && j < Lt) ? bpe_lookup(T, c[i], c[j]) : ~0ull;
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, kBpeLanes);
  return cnt;
}

// bpe_word_long (csrc/common/bpe.h) by one wave: the same linked-list merges, the search for the
// leftmost lowest-rank pair spread over the lanes; lane 0 applies each merge
template <class P>
__device__ int bpe_word_long_wave(const DevBpe& T, const uint8_t* w, int L, int lead, uint32_t* c, uint64_t* v,
                                  int16_t* nx, int16_t* pv, int lane) {
  int m;
  if constexpr (P::kByteSymbols) {
    if (L <= 1) return L;
    for (int i = lane; i < L; i += 64) {
      c[i] = T.byte_id[w[i]];
      nx[i] = (int16_t)(i + 1);
      pv[i] = (int16_t)(i - 1);
    }
    __syncthreads();
    for (int i = lane; i < L; i += 64) v[i] = i + 1 < L ? bpe_lookup(T, c[i], c[i + 1]) : ~0ull;
    m = L;
  } else {
    m = bpe_sp_symbols_wave(T, w, L, lead, c, v, nx, pv, lane);
    L += lead;
  }
  __syncthreads();
  while (m > 1) {
    uint64_t best = ~0ull;
    for (int i = lane; i < L; i += 64) {
      const uint64_t r = v[i] >> 32;
      if (r != kBpeNoRank) {
        const uint64_t key = (r << 32) | (uint32_t)i;  // rank, then position: the leftmost
        best = key < best ? key : best;
      }
    }
    best = wave_min_u64(best);
    if (best == ~0ull) break;
    if (lane == 0) {
      const int bi = (int)(uint32_t)best, j = nx[bi];
      c[bi] = (uint32_t)v[bi];
      nx[bi] = nx[j];
      if (nx[j] < L) pv[nx[j]] = (int16_t)bi;
      v[j] = ~0ull;
      v[bi] = nx[bi] < L ? bpe_lookup(T, c[bi], c[nx[bi]]) : ~0ull;
      if (pv[bi] >= 0) v[pv[bi]] = bpe_lookup(T, c[pv[bi]], c[bi]);
    }
    --m;
    __syncthreads();
  }
  return m;
}

// Documents k_bpe_count marked (count <= kBpeLong): the lanes delimit their ranges' pre-tokens
// again without merging the short ones (their tokens are in the mark), collect the long ones (up
// to kBpeLongList per document) and the wave merges them one after another.
template <class P>
__device__ __forceinline__ void bpe_long_body(const DevBpe& T, const uint8_t* __restrict__ text,
                                              const int64_t* __restrict__ off, const int64_t* __restrict__ n_dev,
                                              int32_t n_max, int32_t* __restrict__ counts) {
  __shared__ uint32_t lc[kBpeMaxLong];
  __shared__ uint64_t lv[kBpeMaxLong];
  __shared__ int16_t lnx[kBpeMaxLong];
  __shared__ int16_t lpv[kBpeMaxLong];
  __shared__ int64_t ls[kBpeLongList], le[kBpeLongList];
  __shared__ uint32_t nlong;
  const int t = threadIdx.x;
  int64_t n = n_max;
  if (n_dev != nullptr) n = min(n, *n_dev);
  for (int64_t k = blockIdx.x; k < n; k += gridDim.x) {
    const int32_t mark = counts[k];
    if (mark > kBpeLong) continue;  // (uniform: one wave per block)
    const int64_t s = off[k];
    const int64_t len = off[k + 1] - s;
    const uint8_t* b = text + s;
    const int64_t chunk = max((int64_t)kBpeMinChunk, (len + kBpeLanes - 1) / kBpeLanes);
    const int64_t s0 = (int64_t)t * chunk;
    if (t == 0) nlong = 0;
    __syncthreads();
    long long cnt = 0;
    int bad = 0;
    int64_t lo, hi;
    lane_span<P>(T, b, len, s0, min(len, s0 + chunk), t, &lo, &hi);
    if (s0 < len) {
      const int64_t x = lane_count<false, P>(T, b, len, lo, hi, BpeArr{nullptr, 0}, BpeArr{nullptr, 0},
                                             [&](int64_t a, int64_t e) -> int64_t {
                                          if (e - a + P::lead(T, b, len, a) > kBpeMaxLong) return -1;
                                          const uint32_t q = atomicAdd(&nlong, 1u);
                                          if (q >= (uint32_t)kBpeLongList) return -1;
                                          ls[q] = a;
                                          le[q] = e;
                                          return 0;
                                        });
      if (x < 0) bad = 1;
    }
    bool any_bad = __ballot(bad) != 0;
    cnt = (long long)kBpeLong - mark;  // the short pre-tokens' tokens and the post-processor's
    __syncthreads();
    const uint32_t nl = nlong < (uint32_t)kBpeLongList ? nlong : (uint32_t)kBpeLongList;
    for (uint32_t q = 0; q < nl && !any_bad; ++q)
      cnt += bpe_word_long_wave<P>(T, b + ls[q], (int)(le[q] - ls[q]), P::lead(T, b, len, ls[q]), lc, lv, lnx, lpv, t);
    if (t == 0) counts[k] = (any_bad || cnt > 0x7FFFFFFF) ? kBpeHost : (int32_t)cnt;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kBpeLanes) void k_bpe_long(DevBpe T, const uint8_t* __restrict__ text,
                                                        const int64_t* __restrict__ off,
                                                        const int64_t* __restrict__ n_dev, int32_t n_max,
                                                        int32_t* __restrict__ counts) {
  bpe_long_body<BpeGpt2>(T, text, off, n_dev, n_max, counts);
}

// k_bpe_long for the split-regex family (a long pre-token that is a vocabulary entry under
// ignore_merges was counted by k_bpe_split_count and is not listed here)
__global__ __launch_bounds__(kBpeLanes) void k_bpe_split_long(DevBpe T, const uint8_t* __restrict__ text,
                                                              const int64_t* __restrict__ off,
                                                              const int64_t* __restrict__ n_dev, int32_t n_max,
                                                              int32_t* __restrict__ counts) {
  bpe_long_body<BpeSplit>(T, text, off, n_dev, n_max, counts);
}

// k_bpe_long for the case-aware split patterns
__global__ __launch_bounds__(kBpeLanes) void k_bpe_case_long(DevBpe T, const uint8_t* __restrict__ text,
                                                             const int64_t* __restrict__ off,
                                                             const int64_t* __restrict__ n_dev, int32_t n_max,
                                                             int32_t* __restrict__ counts) {
  bpe_long_body<BpeCase>(T, text, off, n_dev, n_max, counts);
}

// k_bpe_long for the SentencePiece-style character-level BPE
__global__ __launch_bounds__(kBpeLanes) void k_bpe_sp_long(DevBpe T, const uint8_t* __restrict__ text,
                                                           const int64_t* __restrict__ off,
                                                           const int64_t* __restrict__ n_dev, int32_t n_max,
                                                           int32_t* __restrict__ counts) {
  bpe_long_body<BpeSp>(T, text, off, n_dev, n_max, counts);
}

}  // namespace

// counts[k] for documents k < min(*n_dev, n_max) (n_dev may be null): text + off[k] .. off[k + 1]
extern "C" int tb_bpe_count(hipStream_t stream, const DevBpe* T, const uint8_t* text, const int64_t* off,
                            const int64_t* n_dev, int32_t n_max, int32_t* counts) {
  if (n_max <= 0) return 0;
  if (T == nullptr || !bpe_params_ok(*T)) return (int)hipErrorInvalidValue;
  const bool sp = T->kind == kBpeSp, cased = bpe_kind_case(T->kind);
  const bool split = bpe_kind_mem_added(T->kind);  // (sp: its added tokens are the split family's)
  const int grid = n_max < kBpeGrid ? n_max : kBpeGrid;
  // the documents with pre-tokens over kBpeMaxWord bytes (grid-stride; the others are skipped)
  const int grid_long = n_max < kBpeGrid / 4 ? n_max : kBpeGrid / 4;
  if (cased) {
    if (T->nfc)
      hipLaunchKernelGGL(k_bpe_case_count_nfc, dim3(grid), dim3(kBpeLanes), 0, stream, *T, text, off, n_dev, n_max,
                         counts);
    else
      hipLaunchKernelGGL(k_bpe_case_count, dim3(grid), dim3(kBpeLanes), 0, stream, *T, text, off, n_dev, n_max, counts);
    hipLaunchKernelGGL(k_bpe_case_long, dim3(grid_long), dim3(kBpeLanes), 0, stream, *T, text, off, n_dev, n_max,
                       counts);
  } else if (sp) {
    hipLaunchKernelGGL(k_bpe_sp_count, dim3(grid), dim3(kBpeLanes), 0, stream, *T, text, off, n_dev, n_max, counts);
    hipLaunchKernelGGL(k_bpe_sp_long, dim3(grid_long), dim3(kBpeLanes), 0, stream, *T, text, off, n_dev, n_max, counts);
  } else if (split) {
    if (T->nfc)
      hipLaunchKernelGGL(k_bpe_split_count_nfc, dim3(grid), dim3(kBpeLanes), 0, stream, *T, text, off, n_dev, n_max,
                         counts);
    else
      hipLaunchKernelGGL(k_bpe_split_count, dim3(grid), dim3(kBpeLanes), 0, stream, *T, text, off, n_dev, n_max, counts);
    hipLaunchKernelGGL(k_bpe_split_long, dim3(grid_long), dim3(kBpeLanes), 0, stream, *T, text, off, n_dev, n_max,
                       counts);
  } else {
    hipLaunchKernelGGL(k_bpe_count, dim3(grid), dim3(kBpeLanes), 0, stream, *T, text, off, n_dev, n_max, counts);
    hipLaunchKernelGGL(k_bpe_long, dim3(grid_long), dim3(kBpeLanes), 0, stream, *T, text, off, n_dev, n_max, counts);
  }
  return (int)hipGetLastError();
}

extern "C" size_t tb_sizeof_bpe() { return sizeof(DevBpe); }
