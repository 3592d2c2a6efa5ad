// TokenCounter on the device for Unigram tokenizers (csrc/common/unigram.h): token counts of the
// kept outputs of K16, under tb_bpe_count's contract.
//
// One wave per document (grid-stride over the documents), a 1/64 byte range per lane as in
// k_wp_count: a lane counts the words that start in its range (uni_count_range) and follows a word
// to its end wherever that is, so neither words nor documents have a size limit. The Viterbi state
// of the word a lane is in - a ring of (longest piece in code points + 1) entries of score and
// token count - sits in dynamic LDS sized from the tokenizer, laid out [entry][lane]: the 64 lanes
// of an access hit 64 consecutive 8-byte (scores) or 4-byte (counts) words, so no two lanes share a
// bank. For a longest piece of 16 code points that is 17 * 64 * 12 = 13,056 bytes per wave. The
// vocabulary table, the piece pool and the class table are read through the cache.
//
// k_uni_count_map is the same launch over a block with a map (unigram.h unim_*): the lanes walk the
// normalised text through the normalizer's replacement records, read through the cache as well.
#include <hip/hip_runtime.h>

#include "../common/unigram.h"

using namespace tb;

namespace {

constexpr int kUniLanes = 64;
constexpr int kUniMinChunk = 16;  // bytes per lane at least (short documents use fewer lanes)
constexpr int kUniGrid = 8192;

// bytes of dynamic LDS for a ring of nr entries: the scores, then the counts
constexpr size_t uni_lds_bytes(int nr) { return (size_t)nr * kUniLanes * (sizeof(double) + sizeof(uint32_t)); }

__global__ __launch_bounds__(kUniLanes) void k_uni_count(DevUni T, const uint8_t* __restrict__ text,
                                                         const int64_t* __restrict__ off,
                                                         const int64_t* __restrict__ n_dev, int32_t n_max,
                                                         int32_t* __restrict__ counts) {
  extern __shared__ double uni_lds[];
  const int t = threadIdx.x;
  const int nr = T.longest_cp + 1;
  const UniRing R{uni_lds + t, reinterpret_cast<uint32_t*>(uni_lds + (size_t)nr * kUniLanes) + t, kUniLanes};
  int64_t n = n_max;
  if (n_dev != nullptr) n = min(n, *n_dev);
  for (int64_t k = blockIdx.x; k < n; k += gridDim.x) {
    const int64_t s = off[k];
    const int64_t len = off[k + 1] - s;
    const uint8_t* b = text + s;
    const int64_t chunk = max((int64_t)kUniMinChunk, (len + kUniLanes - 1) / kUniLanes);
    const int64_t s0 = (int64_t)t * chunk;
    long long cnt = 0;
    int bad = 0;
    if (s0 < len) {
      const int64_t s1 = min(len, s0 + chunk);
      if (T.n_added && uni_has_added(T, b, len, s0, s1)) {
        bad = 1;
      } else {
        const int64_t x = uni_count_range(T, b, len, s0, s1, R);
        if (x < 0) bad = 1;
        else cnt = x;
      }
    }
    const bool any_bad = __ballot(bad) != 0;
    for (int o = kUniLanes / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, kUniLanes);
    if (t == 0) {
      const long long tot = cnt + T.post_add;
      counts[k] = (any_bad || tot > 0x7FFFFFFF) ? kBpeHost : (int32_t)tot;
    }
  }
}

// k_uni_count for a block with a map: a lane counts the words whose first output code point comes
// from an input code point that begins in its range (unim_count_range). A kernel of its own and not
// a shared template body: with one, the compiler schedules k_uni_count differently.
__global__ __launch_bounds__(kUniLanes) void k_uni_count_map(DevUni T, const uint8_t* __restrict__ text,
                                                             const int64_t* __restrict__ off,
                                                             const int64_t* __restrict__ n_dev, int32_t n_max,
                                                             int32_t* __restrict__ counts) {
  extern __shared__ double uni_lds[];
  const int t = threadIdx.x;
  const int nr = T.longest_cp + 1;
  const UniRing R{uni_lds + t, reinterpret_cast<uint32_t*>(uni_lds + (size_t)nr * kUniLanes) + t, kUniLanes};
  int64_t n = n_max;
  if (n_dev != nullptr) n = min(n, *n_dev);
  for (int64_t k = blockIdx.x; k < n; k += gridDim.x) {
    const int64_t s = off[k];
    const int64_t len = off[k + 1] - s;
    const uint8_t* b = text + s;
    const int64_t chunk = max((int64_t)kUniMinChunk, (len + kUniLanes - 1) / kUniLanes);
    const int64_t s0 = (int64_t)t * chunk;
    long long cnt = 0;
    int bad = 0;
    if (s0 < len) {
      const int64_t s1 = min(len, s0 + chunk);
      if (T.n_added && uni_has_added(T, b, len, s0, s1)) {
        bad = 1;
      } else {
        const int64_t x = unim_count_range(T, b, len, s0, s1, R);
        if (x < 0) bad = 1;
        else cnt = x;
      }
    }
    const bool any_bad = __ballot(bad) != 0;
    for (int o = kUniLanes / 2; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, kUniLanes);
    if (t == 0) {
      const long long tot = cnt + T.post_add;
      counts[k] = (any_bad || tot > 0x7FFFFFFF) ? kBpeHost : (int32_t)tot;
    }
  }
}

}  // namespace

// counts[k] for documents k < min(*n_dev, n_max) (n_dev may be null): text + off[k] .. off[k + 1]
extern "C" int tb_uni_count(hipStream_t stream, const DevUni* T, const uint8_t* text, const int64_t* off,
                            const int64_t* n_dev, int32_t n_max, int32_t* counts) {
  if (n_max <= 0) return 0;
  if (T == nullptr || !uni_params_ok(*T)) return (int)hipErrorInvalidValue;
  const int grid = n_max < kUniGrid ? n_max : kUniGrid;
  hipLaunchKernelGGL(uni_has_map(*T) ? k_uni_count_map : k_uni_count, dim3(grid), dim3(kUniLanes),
                     uni_lds_bytes(T->longest_cp + 1), stream, *T, text, off, n_dev, n_max, counts);
  return (int)hipGetLastError();
}

extern "C" size_t tb_sizeof_uni() { return sizeof(DevUni); }
