// TokenCounter on the device for WordPiece tokenizers (csrc/common/wordpiece.h): token counts of
// the kept outputs of K16, under tb_bpe_count's contract.
//
// One wave per document (grid-stride over the documents). After k_compact the kept documents'
// final contents sit contiguously at the front of the output buffer, in document order; their
// number is the last entry of the kept-count scan, read here on the device. Each lane takes a 1/64
// byte range of the document and counts the words that start in it (wp_count_range: word starts
// are a local property of the text, so a lane finds its first one without the lanes before it);
// a word is followed to its end wherever that is, so neither words nor documents have a size
// limit. Everything a lane needs is in registers: the longest-first search takes bytes off a
// polynomial hash instead of storing prefix hashes, and the vocabulary table and the piece pool
// are read through the cache (a 30,000-piece vocabulary is about 1 MB). No LDS.
#include <hip/hip_runtime.h>

#include "../common/wordpiece.h"

using namespace tb;

namespace {

constexpr int kWpLanes = 64;
constexpr int kWpMinChunk = 16;  // bytes per lane at least (short documents use fewer lanes)
constexpr int kWpGrid = 8192;

__global__ __launch_bounds__(kWpLanes) void k_wp_count(DevWp T, const uint8_t* __restrict__ text,
                                                       const int64_t* __restrict__ off,
                                                       const int64_t* __restrict__ n_dev, int32_t n_max,
                                                       int32_t* __restrict__ counts) {
  const int t = threadIdx.x;
  int64_t n = n_max;
  if (n_dev != nullptr) n = min(n, *n_dev);
  for (int64_t k = blockIdx.x; k < n; k += gridDim.x) {
    const int64_t s = off[k];
    const int64_t len = off[k + 1] - s;
    const uint8_t* b = text + s;
    const int64_t chunk = max((int64_t)kWpMinChunk, (len + kWpLanes - 1) / kWpLanes);
    const int64_t s0 = (int64_t)t * chunk;
    long long cnt = 0;
    int bad = 0;
    if (s0 < len) {
      const int64_t s1 = min(len, s0 + chunk);
      if (T.n_added && wp_has_added(T, b, len, s0, s1)) {
        bad = 1;
      } else {
        const int64_t x = wp_count_range(T, b, len, s0, s1);
        if (x < 0) bad = 1;
        else cnt = x;
      }
    }
    const bool any_bad = __ballot(bad) != 0;
    for (int o = kWpLanes / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, kWpLanes);
    if (t == 0) {
      const long long tot = cnt + T.post_add;
      counts[k] = (any_bad || tot > 0x7FFFFFFF) ? kBpeHost : (int32_t)tot;
    }
  }
}

// k_wp_count for tokenizers with lowercase / strip_accents: the same launch shape and lane split
// over the folding counter (wpf_count_range: classes, hashes and search positions over the
// normalizer's output, read from the fold tables through the cache). A kernel of its own name, so
// that its registers are budgeted apart from k_wp_count's.
__global__ __launch_bounds__(kWpLanes) void k_wp_count_fold(DevWp T, const uint8_t* __restrict__ text,
                                                            const int64_t* __restrict__ off,
                                                            const int64_t* __restrict__ n_dev, int32_t n_max,
                                                            int32_t* __restrict__ counts) {
  const int t = threadIdx.x;
  int64_t n = n_max;
  if (n_dev != nullptr) n = min(n, *n_dev);
  for (int64_t k = blockIdx.x; k < n; k += gridDim.x) {
    const int64_t s = off[k];
    const int64_t len = off[k + 1] - s;
    const uint8_t* b = text + s;
    const int64_t chunk = max((int64_t)kWpMinChunk, (len + kWpLanes - 1) / kWpLanes);
    const int64_t s0 = (int64_t)t * chunk;
    long long cnt = 0;
    int bad = 0;
    if (s0 < len) {
      const int64_t s1 = min(len, s0 + chunk);
      if (T.n_added && wp_has_added(T, b, len, s0, s1)) {
        bad = 1;
      } else {
        const int64_t x = wp_count_range_t<true>(T, b, len, s0, s1);
        if (x < 0) bad = 1;
        else cnt = x;
      }
    }
    const bool any_bad = __ballot(bad) != 0;
    for (int o = kWpLanes / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, kWpLanes);
    if (t == 0) {
      const long long tot = cnt + T.post_add;
      counts[k] = (any_bad || tot > 0x7FFFFFFF) ? kBpeHost : (int32_t)tot;
    }
  }
}

}  // namespace

// counts[k] for documents k < min(*n_dev, n_max) (n_dev may be null): text + off[k] .. off[k + 1]
extern "C" int tb_wp_count(hipStream_t stream, const DevWp* T, const uint8_t* text, const int64_t* off,
                           const int64_t* n_dev, int32_t n_max, int32_t* counts) {
  if (n_max <= 0) return 0;
  if (T == nullptr || !wp_params_ok(*T)) return (int)hipErrorInvalidValue;
  const int grid = n_max < kWpGrid ? n_max : kWpGrid;
  if (T->fold1 != nullptr)
    hipLaunchKernelGGL(k_wp_count_fold, dim3(grid), dim3(kWpLanes), 0, stream, *T, text, off, n_dev, n_max, counts);
  else
    hipLaunchKernelGGL(k_wp_count, dim3(grid), dim3(kWpLanes), 0, stream, *T, text, off, n_dev, n_max, counts);
  return (int)hipGetLastError();
}

extern "C" size_t tb_sizeof_wp() { return sizeof(DevWp); }
