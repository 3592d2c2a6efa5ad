// What the token counters' standalone self-tests share: a tokenizer's tables in std::vectors, the
// spec view over them, and the parameter block from the project's own validator and filler
// (csrc/host/tok_params.h), so that the sanitizer builds of the self-tests cover those too.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../csrc/host/tok_params.h"

namespace tb {

template <class T>
TokSpan<T> span_of(const std::vector<T>& v) {
  return {v.data(), v.size()};
}
inline TokSpan<uint8_t> span_of(const std::string& s) {
  return {reinterpret_cast<const uint8_t*>(s.data()), s.size()};
}

struct BpeSelfTables {
  std::vector<uint32_t> byte_id, sp_ascii;
  std::vector<uint64_t> keys, vals, vslots, sp_cp;
  std::vector<uint8_t> vpool;
  std::string added;
  std::vector<int32_t> aoff;
  BpeSpecView spec;  // the scalars; params() points its spans at the vectors above

  // merge i: (a[i], b[i]) -> nid[i] at rank i
  void set_merges(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, const std::vector<uint32_t>& nid) {
    std::vector<uint32_t> rank(a.size());
    for (size_t i = 0; i < rank.size(); ++i) rank[i] = (uint32_t)i;
    const size_t cap = tok_table_cap(a.size());
    keys.resize(cap);
    vals.resize(cap);
    if (!bpe_fill_pairs(a.data(), b.data(), rank.data(), nid.data(), a.size(), keys.data(), vals.data(), cap - 1)) {
      std::fprintf(stderr, "FAIL: a merge is the reserved pair\n");
      std::exit(1);
    }
    spec.mask = (uint32_t)(cap - 1);
  }

  // the whole-piece table of ignore_merges over the entries' raw bytes (any iterable of strings)
  template <class Words>
  void set_vocabulary(const Words& words) {
    std::vector<int64_t> voff{0};
    std::vector<uint8_t> cont;
    for (const std::string& w : words) {
      vpool.insert(vpool.end(), w.begin(), w.end());
      voff.push_back((int64_t)vpool.size());
      cont.push_back(0);
    }
    const size_t cap = tok_table_cap(cont.size());
    std::vector<WpSlot> slots(cap, WpSlot{0, kWpEmpty});
    spec.vlongest = (int32_t)wp_fill_slots(vpool.data(), voff.data(), cont.data(), cont.size(), slots.data(), cap - 1);
    vslots.clear();
    for (const WpSlot& s : slots) {
      vslots.push_back(s.key);
      vslots.push_back(s.val);
    }
    spec.vmask = (uint32_t)(cap - 1);
  }

  // the block over host addresses, as the host emulation builds it
  DevBpe params() {
    spec.byte_id = span_of(byte_id);
    spec.keys = span_of(keys);
    spec.vals = span_of(vals);
    spec.added = span_of(added);
    spec.added_off = span_of(aoff);
    spec.vslots = span_of(vslots);
    spec.vpool = span_of(vpool);
    spec.sp_ascii = span_of(sp_ascii);
    spec.sp_cp = span_of(sp_cp);
    if (const char* e = bpe_spec_error(spec)) {
      std::fprintf(stderr, "FAIL: the spec is refused: %s\n", e);
      std::exit(1);
    }
    return bpe_fill_params(spec, bpe_host_ptrs(spec));
  }
};

struct WpSelfTables {
  std::vector<uint8_t> pool;
  std::vector<uint64_t> slots;
  std::string added;
  std::vector<int32_t> aoff;
  WpSpecView spec;

  // pieces i = (cont[i], pool[off[i]:off[i + 1]])
  void set_pieces(const std::vector<int64_t>& off, const std::vector<uint8_t>& cont) {
    const size_t cap = tok_table_cap(cont.size());
    std::vector<WpSlot> table(cap, WpSlot{0, kWpEmpty});
    spec.longest = (int32_t)wp_fill_slots(pool.data(), off.data(), cont.data(), cont.size(), table.data(), cap - 1);
    slots.clear();
    for (const WpSlot& s : table) {
      slots.push_back(s.key);
      slots.push_back(s.val);
    }
    spec.mask = (uint32_t)(cap - 1);
  }

  DevWp params() {
    spec.slots = span_of(slots);
    spec.pool = span_of(pool);
    spec.added = span_of(added);
    spec.added_off = span_of(aoff);
    if (const char* e = wp_spec_error(spec)) {
      std::fprintf(stderr, "FAIL: the spec is refused: %s\n", e);
      std::exit(1);
    }
    return wp_fill_params(spec, wp_host_ptrs(spec));
  }
};

}  // namespace tb
