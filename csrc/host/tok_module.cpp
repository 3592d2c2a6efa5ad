// The token counters' part of _tbhost: table builders, the host emulation of the counting kernels
// (csrc/common/bpe.h, wordpiece.h, unigram.h; device kernels csrc/hip/bpe.hip, wordpiece.hip,
// unigram.hip) and the kernels' parameter blocks as bytes. Every entry point takes the Python spec
// object (models/tokenizer.py BpeSpec / WordPieceSpec / UnigramSpec); tok_params.h validates it and
// fills the block, here as there.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>

#include <unicode/uchar.h>

#include "np_util.h"
#include "tok_params.h"

namespace py = pybind11;
using namespace tb;

namespace {

template <class T>
using Arr = py::array_t<T, py::array::c_style>;

// spec.<name> as a span over an array that ``keep`` holds; None = absent
template <class T>
TokSpan<T> spec_array(const py::object& spec, const char* name, Arr<T>& keep) {
  const py::object o = spec.attr(name);
  if (o.is_none()) return {};
  keep = Arr<T>::ensure(o);
  if (!keep) {
    PyErr_Clear();
    throw std::invalid_argument(std::string("token counter spec: ") + name + " is not an array of its type");
  }
  return {keep.data(), (size_t)keep.size()};
}

struct BpeSpecArrays {
  Arr<uint32_t> byte_id, sp_ascii;
  Arr<uint64_t> keys, vals, vslots, sp_cp;
  Arr<uint8_t> added, vpool;
  std::vector<int32_t> added_off;
};
struct WpSpecArrays {
  Arr<uint64_t> slots;
  Arr<uint8_t> pool, added;
  std::vector<int32_t> added_off;
};

struct UniSpecArrays {
  Arr<uint64_t> slots;
  Arr<uint8_t> pool, added, cls2, sp;
  Arr<uint16_t> cls1, map1, map2;
  Arr<uint32_t> map_rec;
  Arr<uint8_t> map_pool;
  std::vector<int32_t> added_off;
};

UniSpecView uni_view(const py::object& s, UniSpecArrays& a) {
  UniSpecView v;
  v.slots = spec_array(s, "slots", a.slots);
  v.pool = spec_array(s, "pool", a.pool);
  v.added = spec_array(s, "added", a.added);
  v.cls1 = spec_array(s, "cls1", a.cls1);
  v.cls2 = spec_array(s, "cls2", a.cls2);
  v.sp = spec_array(s, "sp", a.sp);
  a.added_off = s.attr("added_off").cast<std::vector<int32_t>>();
  v.added_off = {a.added_off.data(), a.added_off.size()};
  v.mask = s.attr("mask").cast<uint32_t>();
  v.flags = s.attr("flags").cast<uint32_t>();
  v.longest_cp = s.attr("longest_cp").cast<int32_t>();
  v.longest = s.attr("longest").cast<int32_t>();
  v.post_add = s.attr("post_add").cast<int32_t>();
  v.unk_score = s.attr("unk_score").cast<double>();
  v.map1 = spec_array(s, "map1", a.map1);
  v.map2 = spec_array(s, "map2", a.map2);
  v.map_rec = spec_array(s, "map_rec", a.map_rec);
  v.map_pool = spec_array(s, "map_pool", a.map_pool);
  return v;
}

BpeSpecView bpe_view(const py::object& s, BpeSpecArrays& a) {
  BpeSpecView v;
  v.byte_id = spec_array(s, "byte_id", a.byte_id);
  v.keys = spec_array(s, "keys", a.keys);
  v.vals = spec_array(s, "vals", a.vals);
  v.added = spec_array(s, "added", a.added);
  a.added_off = s.attr("added_off").cast<std::vector<int32_t>>();
  v.added_off = {a.added_off.data(), a.added_off.size()};
  v.vslots = spec_array(s, "vslots", a.vslots);
  v.vpool = spec_array(s, "vpool", a.vpool);
  v.sp_ascii = spec_array(s, "sp_ascii", a.sp_ascii);
  v.sp_cp = spec_array(s, "sp_cp", a.sp_cp);
  v.mask = s.attr("mask").cast<uint32_t>();
  v.post_add = s.attr("post_add").cast<int32_t>();
  v.kind = s.attr("kind").cast<int32_t>();
  v.ignore_merges = s.attr("ignore_merges").cast<bool>();
  v.vmask = s.attr("vmask").cast<uint32_t>();
  v.vlongest = s.attr("vlongest").cast<int32_t>();
  v.nfc = s.attr("nfc").cast<bool>();
  v.sp_mask = s.attr("sp_mask").cast<uint32_t>();
  v.sp_id = s.attr("sp_id").cast<uint32_t>();
  v.sp_flags = s.attr("sp_flags").cast<int32_t>();
  return v;
}

WpSpecView wp_view(const py::object& s, WpSpecArrays& a) {
  WpSpecView v;
  v.slots = spec_array(s, "slots", a.slots);
  v.pool = spec_array(s, "pool", a.pool);
  v.added = spec_array(s, "added", a.added);
  a.added_off = s.attr("added_off").cast<std::vector<int32_t>>();
  v.added_off = {a.added_off.data(), a.added_off.size()};
  v.mask = s.attr("mask").cast<uint32_t>();
  v.flags = s.attr("flags").cast<uint32_t>();
  v.cls_shift = s.attr("cls_shift").cast<uint32_t>();
  v.self_bit = s.attr("self_bit").cast<uint32_t>();
  v.max_chars = s.attr("max_chars").cast<int32_t>();
  v.longest = s.attr("longest").cast<int32_t>();
  v.post_add = s.attr("post_add").cast<int32_t>();
  v.fold = s.attr("fold").cast<int32_t>();
  return v;
}

// ptrs[name] as an address (an integer that is never dereferenced here); absent = null
template <class T>
void addr(const py::dict& ptrs, const char* name, const T*& out) {
  out = ptrs.contains(name) ? reinterpret_cast<const T*>(ptrs[name].cast<uintptr_t>()) : nullptr;
}

// a block as bytes, up to the end of its last field (what follows is padding: left zero)
template <class Block>
py::bytes block_bytes(const Block& T, size_t used) {
  std::string out(sizeof(Block), '\0');
  std::memcpy(&out[0], &T, used);
  return py::bytes(out);
}

// a block of kind ``kind`` with the static tables and an empty vocabulary: the pre-tokenizer alone
DevBpe bpe_pattern_params(int kind) {
  static const uint32_t ids[256] = {};
  static const uint64_t no_key[1] = {kBpeEmpty}, no_val[1] = {~0ull};
  BpeSpecView v;
  v.byte_id = {ids, 256};
  v.keys = {no_key, 1};
  v.vals = {no_val, 1};
  v.kind = kind;
  return bpe_fill_params(v, bpe_host_ptrs(v));
}

int count_threads(int nthreads, int64_t nd) { return std::max(1, std::min<int>(nthreads, (int)(nd / 256) + 1)); }

}  // namespace

void register_tok(py::module_& m) {
  m.attr("SIZEOF_DEV_BPE") = sizeof(DevBpe);
  m.attr("SIZEOF_DEV_WP") = sizeof(DevWp);
  {
    // byte offset of every field, for tests that read a block built by bpe_params / wp_params
    py::dict b, w;
#define TB_OFF(d, S, f) d[#f] = offsetof(S, f)
    TB_OFF(b, DevBpe, byte_id); TB_OFF(b, DevBpe, keys); TB_OFF(b, DevBpe, vals); TB_OFF(b, DevBpe, cls1);
    TB_OFF(b, DevBpe, cls2); TB_OFF(b, DevBpe, added); TB_OFF(b, DevBpe, mask); TB_OFF(b, DevBpe, n_added);
    TB_OFF(b, DevBpe, added_off); TB_OFF(b, DevBpe, post_add); TB_OFF(b, DevBpe, aoff); TB_OFF(b, DevBpe, vslots);
    TB_OFF(b, DevBpe, vpool); TB_OFF(b, DevBpe, nfc1); TB_OFF(b, DevBpe, nfc2); TB_OFF(b, DevBpe, ccls1);
    TB_OFF(b, DevBpe, ccls2); TB_OFF(b, DevBpe, amask); TB_OFF(b, DevBpe, vmask); TB_OFF(b, DevBpe, vlongest);
    TB_OFF(b, DevBpe, kind); TB_OFF(b, DevBpe, ignore_merges); TB_OFF(b, DevBpe, nfc); TB_OFF(b, DevBpe, sp_flags);
    TB_OFF(b, DevBpe, sp_ascii); TB_OFF(b, DevBpe, sp_cp); TB_OFF(b, DevBpe, sp_mask); TB_OFF(b, DevBpe, sp_id);
    TB_OFF(w, DevWp, slots); TB_OFF(w, DevWp, pool); TB_OFF(w, DevWp, cls1); TB_OFF(w, DevWp, cls2);
    TB_OFF(w, DevWp, added); TB_OFF(w, DevWp, fold1); TB_OFF(w, DevWp, fold2); TB_OFF(w, DevWp, foldp);
    TB_OFF(w, DevWp, asc0); TB_OFF(w, DevWp, asc1); TB_OFF(w, DevWp, asc2); TB_OFF(w, DevWp, asc3);
    TB_OFF(w, DevWp, mask); TB_OFF(w, DevWp, flags); TB_OFF(w, DevWp, cls_shift); TB_OFF(w, DevWp, self_bit);
    TB_OFF(w, DevWp, max_chars); TB_OFF(w, DevWp, longest); TB_OFF(w, DevWp, post_add); TB_OFF(w, DevWp, n_added);
    TB_OFF(w, DevWp, added_off);
#undef TB_OFF
    m.attr("DEV_BPE_OFFSETS") = b;
    m.attr("DEV_WP_OFFSETS") = w;
    // the constants models/tokenizer.py mirrors (tests pin the copies to these)
    py::dict c;
    c["BPE_GPT2"] = (int)kBpeGpt2; c["BPE_SPLIT_A"] = (int)kBpeSplitA; c["BPE_SPLIT_B"] = (int)kBpeSplitB;
    c["BPE_CASE_C"] = (int)kBpeCaseC; c["BPE_CASE_D"] = (int)kBpeCaseD; c["BPE_SP"] = (int)kBpeSp;
    c["MAX_ADDED"] = kBpeMaxAdded; c["SPLIT_MAX_ADDED"] = kBpeSplitMaxAdded;
    c["SPLIT_MAX_ADDED_BYTES"] = kBpeSplitMaxAddedBytes; c["SP_PREPEND_NONE"] = 0;
    c["SP_PREPEND_ALWAYS"] = (int)kBpeSpPrependAlways; c["SP_PREPEND_UNLESS_SPACE"] = (int)kBpeSpPrependUnlessSpace;
    c["SP_SPLIT"] = (int)kBpeSpSplit; c["WP_LOWER"] = kWpLower; c["WP_CHINESE"] = kWpChinese;
    m.attr("TOK_CONSTANTS") = c;
    py::dict u, uc;
#define TB_OFF(d, S, f) d[#f] = offsetof(S, f)
    TB_OFF(u, DevUni, slots); TB_OFF(u, DevUni, pool); TB_OFF(u, DevUni, cls1); TB_OFF(u, DevUni, cls2);
    TB_OFF(u, DevUni, added); TB_OFF(u, DevUni, aoff); TB_OFF(u, DevUni, asc0); TB_OFF(u, DevUni, asc1);
    TB_OFF(u, DevUni, asc2); TB_OFF(u, DevUni, asc3); TB_OFF(u, DevUni, amask); TB_OFF(u, DevUni, unk_score);
    TB_OFF(u, DevUni, mask); TB_OFF(u, DevUni, flags); TB_OFF(u, DevUni, sp_bytes); TB_OFF(u, DevUni, sp_len);
    TB_OFF(u, DevUni, longest_cp); TB_OFF(u, DevUni, longest); TB_OFF(u, DevUni, post_add); TB_OFF(u, DevUni, n_added);
    TB_OFF(u, DevUni, map1); TB_OFF(u, DevUni, map2); TB_OFF(u, DevUni, mrec); TB_OFF(u, DevUni, mpool);
#undef TB_OFF
    m.attr("DEV_UNI_OFFSETS") = u;
    m.attr("SIZEOF_DEV_UNI") = sizeof(DevUni);
    uc["UNI_KEEP"] = (int)UNI_KEEP; uc["UNI_SPACE"] = (int)UNI_SPACE; uc["UNI_HOST"] = (int)UNI_HOST;
    uc["UNI_BYTE_FALLBACK"] = kUniByteFallback; uc["UNI_MAX_PIECE_CP"] = kUniMaxPieceCp;
    uc["UNI_MAX_PIECE_BYTES"] = kUniMaxPieceBytes;
    uc["UNI_MAP"] = (int)UNI_MAP; uc["UNI_MAX_MAP_BYTES"] = kUniMaxMapBytes; uc["UNI_MAP_NONE"] = (int)kUniMapNone;
    uc["UNI_REC_LEN"] = kUniRecLen; uc["UNI_REC_JOIN"] = kUniRecJoin;
    m.attr("UNI_CONSTANTS") = uc;
  }
  // ---- byte-level BPE token counting (csrc/common/bpe.h; device kernel csrc/hip/bpe.hip) ----
  m.def("bpe_classes", []() {
    std::vector<uint16_t> c1(TB_BPE_CLS_STAGE1, TB_BPE_CLS_STAGE1 + sizeof(TB_BPE_CLS_STAGE1) / 2);
    std::vector<uint32_t> c2(TB_BPE_CLS_STAGE2, TB_BPE_CLS_STAGE2 + sizeof(TB_BPE_CLS_STAGE2) / 4);
    return py::make_tuple(to_numpy(std::move(c1)), to_numpy(std::move(c2)));
  });
  m.def("bpe_build_table", [](Arr<uint32_t> a, Arr<uint32_t> b, Arr<uint32_t> rank, Arr<uint32_t> nid) {
    // the merge table (bpe_fill_pairs), load <= 1/2
    const size_t n = (size_t)a.size();
    if ((size_t)b.size() != n || (size_t)rank.size() != n || (size_t)nid.size() != n)
      throw std::invalid_argument("bpe_build_table: the four lists differ in length");
    const size_t cap = tok_table_cap(n);
    std::vector<uint64_t> keys(cap), vals(cap);
    if (!bpe_fill_pairs(a.data(), b.data(), rank.data(), nid.data(), n, keys.data(), vals.data(), cap - 1))
      throw std::invalid_argument("bpe_build_table: reserved pair");
    return py::make_tuple(to_numpy(std::move(keys)), to_numpy(std::move(vals)), (uint32_t)(cap - 1));
  });
  m.def("bpe_count", [](Arr<uint8_t> data, Arr<int64_t> off, py::object spec, int nthreads, int64_t chunk) {
    // host emulation of k_bpe_count / k_bpe_split_count / k_bpe_sp_count (kind: BpeKind): per document the token
    // count, or kBpeHost. chunk > 0: the wave split — the pre-tokens starting in each chunk-byte
    // range counted independently (bpe_count_range), as the kernel's lanes do. nfc: behind the NFC
    // gate (bpe_nfc_range, per range in the chunk mode), as k_bpe_split_count_nfc
    BpeSpecArrays arrays;
    const BpeSpecView view = bpe_view(spec, arrays);
    const DevBpe T = bpe_fill_params(view, bpe_host_ptrs(view));
    const int64_t nd = off.size() - 1;
    std::vector<int32_t> out(nd > 0 ? nd : 0);
    const uint8_t* d = data.data();
    const int64_t* o = off.data();
    auto run = [&](auto policy) {
      using P = decltype(policy);
      py::gil_scoped_release nogil;
      const int nt = count_threads(nthreads, nd);
      std::vector<std::thread> th;
      for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t]() {
          uint32_t cbuf[kBpeMaxWord], rbuf[kBpeMaxWord];
          std::vector<uint32_t> lc(kBpeMaxLong);
          std::vector<uint64_t> lv(kBpeMaxLong);
          std::vector<int32_t> lnx(kBpeMaxLong), lpv(kBpeMaxLong);
          const uint8_t* b = nullptr;
          int64_t n = 0;
          // pre-tokens over kBpeMaxWord bytes: merged over arrays of their own length (as
          // k_bpe_long does), up to kBpeMaxLong bytes
          auto on_long = [&](int64_t s, int64_t e) -> int64_t {
            const int lead = P::lead(T, b, n, s);
            if (e - s + lead > kBpeMaxLong) return -1;
            return bpe_word_long<P>(T, b + s, (int)(e - s), lc.data(), lv.data(), lnx.data(), lpv.data(), lead);
          };
          for (int64_t k = t; k < nd; k += nt) {
            b = d + o[k];
            n = o[k + 1] - o[k];
            if (chunk <= 0) {
              out[k] = bpe_count_doc<P>(T, b, n, BpeArr{cbuf, 1}, BpeArr{rbuf, 1}, on_long);
              continue;
            }
            int64_t tot = T.post_add;
            bool bad = T.n_added && P::has_added(T, b, n, 0, n);
            for (int64_t s0 = 0; s0 < n && !bad; s0 += chunk) {
              if (T.nfc && bpe_nfc_range(T, b, n, s0, std::min(n, s0 + chunk)) != 1) {
                bad = true;
                break;
              }
              const int64_t x = bpe_count_range<true, P>(T, b, n, s0, std::min(n, s0 + chunk), BpeArr{cbuf, 1},
                                                         BpeArr{rbuf, 1}, on_long);
              if (x < 0) bad = true;
              tot += x;
            }
            out[k] = (bad || tot > 0x7FFFFFFF) ? kBpeHost : (int32_t)tot;
          }
        });
      for (auto& x : th) x.join();
    };
    if (bpe_kind_case(T.kind)) run(BpeCase{});
    else if (T.kind == kBpeSp) run(BpeSp{});
    else if (bpe_kind_split(T.kind)) run(BpeSplit{});
    else run(BpeGpt2{});
    return to_numpy(std::move(out));
  }, py::arg("data"), py::arg("off"), py::arg("spec"), py::arg("nthreads") = 8, py::arg("chunk") = 0);
  m.def("bpe_params", [](py::object spec, py::dict ptrs) {
    // DevBpe for the kernels: the spec's scalars and the HBM addresses ``ptrs`` names
    // (array name -> address; the spec's arrays, its added_off as "aoff", and the static tables)
    BpeSpecArrays arrays;
    const BpeSpecView view = bpe_view(spec, arrays);
    BpePtrs p;
    addr(ptrs, "byte_id", p.byte_id); addr(ptrs, "keys", p.keys); addr(ptrs, "vals", p.vals);
    addr(ptrs, "added", p.added); addr(ptrs, "aoff", p.aoff); addr(ptrs, "vslots", p.vslots);
    addr(ptrs, "vpool", p.vpool); addr(ptrs, "sp_ascii", p.sp_ascii); addr(ptrs, "sp_cp", p.sp_cp);
    addr(ptrs, "cls1", p.cls1); addr(ptrs, "cls2", p.cls2); addr(ptrs, "ccls1", p.ccls1);
    addr(ptrs, "ccls2", p.ccls2); addr(ptrs, "nfc1", p.nfc1); addr(ptrs, "nfc2", p.nfc2);
    const DevBpe T = bpe_fill_params(view, p);
    return block_bytes(T, offsetof(DevBpe, sp_id) + sizeof T.sp_id);
  }, py::arg("spec"), py::arg("ptrs"));
  m.def("bpe_sp_build_table", [](Arr<uint32_t> cps, Arr<uint32_t> ids) {
    // DevBpe::sp_cp (csrc/common/bpe_sp.h): code point -> id of the single-character vocabulary
    // entries above ASCII
    const size_t n = (size_t)cps.size();
    if ((size_t)ids.size() != n) throw std::invalid_argument("bpe_sp_build_table: the two lists differ in length");
    for (size_t i = 0; i < n; ++i)
      if (cps.data()[i] < 128 || cps.data()[i] > 0x10FFFF) throw std::invalid_argument("bpe_sp_build_table: code point");
    const size_t cap = tok_table_cap(n);
    std::vector<uint64_t> slots(cap);
    bpe_sp_fill(cps.data(), ids.data(), n, slots.data(), (uint32_t)(cap - 1));
    return py::make_tuple(to_numpy(std::move(slots)), (uint32_t)(cap - 1));
  });
  m.def("nfc_qc", []() {
    // the NFC gate's two-stage table (csrc/common/nfc_qc.inc)
    std::vector<uint8_t> t1(TB_NFC_QC_STAGE1, TB_NFC_QC_STAGE1 + sizeof(TB_NFC_QC_STAGE1));
    std::vector<uint8_t> t2(TB_NFC_QC_STAGE2, TB_NFC_QC_STAGE2 + sizeof(TB_NFC_QC_STAGE2));
    return py::make_tuple(to_numpy(std::move(t1)), to_numpy(std::move(t2)));
  });
  m.def("bpe_case_classes", []() {
    std::vector<uint16_t> c1(TB_BPE_CASE_STAGE1, TB_BPE_CASE_STAGE1 + sizeof(TB_BPE_CASE_STAGE1) / 2);
    std::vector<uint32_t> c2(TB_BPE_CASE_STAGE2, TB_BPE_CASE_STAGE2 + sizeof(TB_BPE_CASE_STAGE2) / 4);
    return py::make_tuple(to_numpy(std::move(c1)), to_numpy(std::move(c2)));
  });
  m.def("bpe_split_ends", [](py::bytes text, int kind) -> py::object {
    // the pre-tokens of pattern A / B (bpe_split_next_token) or C / D (bpe_case_next_token): their
    // end offsets in bytes, None on invalid UTF-8 (for tests and tools that compare the rules with
    // the library's Split)
    if (!bpe_kind_split(kind)) throw std::invalid_argument("bpe_split_ends: kind");
    const std::string s = text;
    const DevBpe T = bpe_pattern_params(kind);
    std::vector<int64_t> ends;
    const int64_t n = (int64_t)s.size();
    for (int64_t p = 0; p < n;) {
      const uint8_t* u = reinterpret_cast<const uint8_t*>(s.data());
      const int64_t e = bpe_kind_case(kind) ? bpe_case_next_token(T, u, n, p) : bpe_split_next_token(T, u, n, p);
      if (e <= p) return py::none();
      ends.push_back(e);
      p = e;
    }
    return to_numpy(std::move(ends));
  });
  // ---- WordPiece token counting (csrc/common/wordpiece.h; device kernel csrc/hip/wordpiece.hip) ----
  m.def("wp_classes", []() {
    std::vector<uint16_t> c1(TB_WP_CLS_STAGE1, TB_WP_CLS_STAGE1 + sizeof(TB_WP_CLS_STAGE1) / 2);
    std::vector<uint8_t> c2(TB_WP_CLS_STAGE2, TB_WP_CLS_STAGE2 + sizeof(TB_WP_CLS_STAGE2));
    return py::make_tuple(to_numpy(std::move(c1)), to_numpy(std::move(c2)));
  });
  m.def("wp_ascii", [](uint32_t shift) {
    std::vector<uint64_t> a(4);
    wp_ascii_classes(TB_WP_CLS_STAGE1, TB_WP_CLS_STAGE2, shift, a.data());
    return to_numpy(std::move(a));
  });
  m.def("wp_fold_tables", []() {
    // wp_fold.inc for upload: stage 1 of the three modes (lowercase, strip_accents, both), the
    // shared stage 2 and the record pool
    std::vector<uint16_t> f1(TB_WP_FOLD_STAGE1, TB_WP_FOLD_STAGE1 + sizeof(TB_WP_FOLD_STAGE1) / 2);
    std::vector<uint16_t> f2(TB_WP_FOLD_STAGE2, TB_WP_FOLD_STAGE2 + sizeof(TB_WP_FOLD_STAGE2) / 2);
    std::vector<uint8_t> fp(TB_WP_FOLD_POOL, TB_WP_FOLD_POOL + sizeof(TB_WP_FOLD_POOL));
    return py::make_tuple(to_numpy(std::move(f1)).attr("reshape")(3, TB_WP_FOLD_NSTAGE1), to_numpy(std::move(f2)),
                          to_numpy(std::move(fp)));
  });
  m.def("wp_build_table", [](Arr<uint8_t> pool, Arr<int64_t> off, Arr<uint8_t> cont) {
    // pieces i = (cont[i], pool[off[i]:off[i + 1]]), distinct; open addressing, load <= 1/2.
    // Returns the slots as uint64 pairs (WpSlot), the mask and the longest piece's bytes.
    const size_t n = (size_t)cont.size();
    if ((size_t)off.size() != n + 1 || n >= (1u << 30)) throw std::invalid_argument("wp_build_table: off needs one entry more than cont");
    const int64_t* o = off.data();
    for (size_t i = 0; i < n; ++i)
      if (o[i] < 0 || o[i + 1] <= o[i] || o[i + 1] > pool.size() || o[i + 1] - o[i] >= (1ll << 31) ||
          o[i] >= (1ll << 32) || cont.data()[i] > 1)
        throw std::invalid_argument("wp_build_table: piece offsets");
    const size_t cap = tok_table_cap(n);
    static_assert(sizeof(WpSlot) == 16, "WpSlot is two uint64");
    std::vector<uint64_t> slots(2 * cap, kWpEmpty);
    const uint64_t mask = cap - 1;
    const int64_t longest =
        wp_fill_slots(pool.data(), o, cont.data(), n, reinterpret_cast<WpSlot*>(slots.data()), mask);
    return py::make_tuple(to_numpy(std::move(slots)), (uint32_t)mask, longest);
  });
  m.def("wp_count", [](Arr<uint8_t> data, Arr<int64_t> off, py::object spec, int nthreads, int64_t chunk) {
    // host emulation of k_wp_count (fold 0) / k_wp_count_fold (fold 1 lowercase, 2 strip_accents,
    // 3 both: wp_fold.inc): per document the token count, or kBpeHost. chunk > 0: the wave split -
    // the words starting in each chunk-byte range counted independently (wp_count_range), as the
    // kernel's lanes do
    WpSpecArrays arrays;
    const WpSpecView view = wp_view(spec, arrays);
    const DevWp T = wp_fill_params(view, wp_host_ptrs(view));
    const bool fold = T.fold1 != nullptr;
    const int64_t nd = off.size() - 1;
    std::vector<int32_t> out(nd > 0 ? nd : 0);
    const uint8_t* d = data.data();
    const int64_t* o = off.data();
    {
      py::gil_scoped_release nogil;
      const int nt = count_threads(nthreads, nd);
      std::vector<std::thread> th;
      for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t]() {
          for (int64_t k = t; k < nd; k += nt) {
            const uint8_t* b = d + o[k];
            const int64_t n = o[k + 1] - o[k];
            if (chunk <= 0) {
              out[k] = fold ? wp_count_doc_t<true>(T, b, n) : wp_count_doc(T, b, n);
              continue;
            }
            int64_t tot = T.post_add;
            bool bad = T.n_added && wp_has_added(T, b, n, 0, n);
            for (int64_t s0 = 0; s0 < n && !bad; s0 += chunk) {
              const int64_t s1 = std::min(n, s0 + chunk);
              const int64_t x = fold ? wpf_count_range(T, b, n, s0, s1) : wp_count_range(T, b, n, s0, s1);
              if (x < 0) bad = true;
              tot += x;
            }
            out[k] = (bad || tot > 0x7FFFFFFF) ? kBpeHost : (int32_t)tot;
          }
        });
      for (auto& x : th) x.join();
    }
    return to_numpy(std::move(out));
  }, py::arg("data"), py::arg("off"), py::arg("spec"), py::arg("nthreads") = 8, py::arg("chunk") = 0);
  m.def("wp_params", [](py::object spec, py::dict ptrs) {
    // DevWp for the kernels (as bpe_params; "fold1": stage 1 of all three modes, as wp_fold_tables
    // returns it)
    WpSpecArrays arrays;
    const WpSpecView view = wp_view(spec, arrays);
    WpPtrs p;
    addr(ptrs, "slots", p.slots); addr(ptrs, "pool", p.pool); addr(ptrs, "added", p.added);
    addr(ptrs, "cls1", p.cls1); addr(ptrs, "cls2", p.cls2); addr(ptrs, "fold1", p.fold1);
    addr(ptrs, "fold2", p.fold2); addr(ptrs, "foldp", p.foldp);
    const DevWp T = wp_fill_params(view, p);
    return block_bytes(T, offsetof(DevWp, added_off) + sizeof T.added_off);
  }, py::arg("spec"), py::arg("ptrs"));
  // ---- Unigram token counting (csrc/common/unigram.h; device kernel csrc/hip/unigram.hip) ----
  m.def("uni_grapheme_joiners", []() {
    // one byte per code point: 1 when its Grapheme_Cluster_Break (ICU) is Extend, ZWJ, SpacingMark,
    // Prepend, L, V or T - the code points that can share a grapheme with a neighbour other than
    // CR LF, which the Precompiled normalizer maps as a whole
    std::vector<uint8_t> out(0x110000, 0);
    for (UChar32 c = 0; c < 0x110000; ++c) {
      const int32_t g = u_getIntPropertyValue(c, UCHAR_GRAPHEME_CLUSTER_BREAK);
      out[(size_t)c] = g == U_GCB_EXTEND || g == U_GCB_ZWJ || g == U_GCB_SPACING_MARK || g == U_GCB_PREPEND ||
                       g == U_GCB_L || g == U_GCB_V || g == U_GCB_T;
    }
    return to_numpy(std::move(out));
  });
  m.def("uni_build_table", [](Arr<uint8_t> pool, Arr<int64_t> off, Arr<double> score, int64_t unk) {
    // pieces i = pool[off[i]:off[i + 1]] of score[i], distinct; open addressing, load <= 1/2.
    // Returns the slots as uint64 triples (UniSlot) and the mask.
    const size_t n = (size_t)score.size();
    if ((size_t)off.size() != n + 1 || n >= (1u << 30)) throw std::invalid_argument("uni_build_table: off needs one entry more than score");
    const int64_t* o = off.data();
    for (size_t i = 0; i < n; ++i)
      if (o[i] < 0 || o[i + 1] <= o[i] || o[i + 1] > pool.size() || o[i + 1] - o[i] >= (1ll << 31) || o[i] >= (1ll << 32))
        throw std::invalid_argument("uni_build_table: piece offsets");
    const size_t cap = tok_table_cap(n);
    std::vector<uint64_t> slots(3 * cap, kWpEmpty);
    uni_fill_slots(pool.data(), o, score.data(), n, unk < 0 ? n : (size_t)unk, reinterpret_cast<UniSlot*>(slots.data()),
                   cap - 1);
    return py::make_tuple(to_numpy(std::move(slots)), (uint32_t)(cap - 1));
  });
  m.def("uni_count", [](Arr<uint8_t> data, Arr<int64_t> off, py::object spec, int nthreads, int64_t chunk) {
    // host emulation of k_uni_count, and of k_uni_count_map for a spec with a map: per document the
    // token count, or kBpeHost. chunk > 0: the wave split - the words starting in each chunk-byte
    // range counted independently (uni_count_range / unim_count_range), as the kernel's lanes do
    UniSpecArrays arrays;
    const UniSpecView view = uni_view(spec, arrays);
    const DevUni T = uni_fill_params(view, uni_host_ptrs(view));
    const bool map = uni_has_map(T);
    const int64_t nd = off.size() - 1;
    std::vector<int32_t> out(nd > 0 ? nd : 0);
    const uint8_t* d = data.data();
    const int64_t* o = off.data();
    {
      py::gil_scoped_release nogil;
      const int nt = count_threads(nthreads, nd);
      std::vector<std::thread> th;
      for (int t = 0; t < nt; ++t)
        th.emplace_back([&, t]() {
          double rs[kUniMaxPieceCp + 1];
          uint32_t rm[kUniMaxPieceCp + 1];
          const UniRing R{rs, rm, 1};
          for (int64_t k = t; k < nd; k += nt) {
            const uint8_t* b = d + o[k];
            const int64_t n = o[k + 1] - o[k];
            if (chunk <= 0) {
              out[k] = map ? unim_count_doc(T, b, n, R) : uni_count_doc(T, b, n, R);
              continue;
            }
            int64_t tot = T.post_add;
            bool bad = T.n_added && uni_has_added(T, b, n, 0, n);
            for (int64_t s0 = 0; s0 < n && !bad; s0 += chunk) {
              const int64_t s1 = std::min(n, s0 + chunk);
              const int64_t x = map ? unim_count_range(T, b, n, s0, s1, R) : uni_count_range(T, b, n, s0, s1, R);
              if (x < 0) bad = true;
              tot += x;
            }
            out[k] = (bad || tot > 0x7FFFFFFF) ? kBpeHost : (int32_t)tot;
          }
        });
      for (auto& x : th) x.join();
    }
    return to_numpy(std::move(out));
  }, py::arg("data"), py::arg("off"), py::arg("spec"), py::arg("nthreads") = 8, py::arg("chunk") = 0);
  m.def("uni_params", [](py::object spec, py::dict ptrs) {
    // DevUni for the kernel (as bpe_params; the spec's added_off as "aoff")
    UniSpecArrays arrays;
    const UniSpecView view = uni_view(spec, arrays);
    UniPtrs p;
    addr(ptrs, "slots", p.slots); addr(ptrs, "pool", p.pool); addr(ptrs, "added", p.added);
    addr(ptrs, "cls1", p.cls1); addr(ptrs, "cls2", p.cls2); addr(ptrs, "aoff", p.aoff);
    addr(ptrs, "map1", p.map1); addr(ptrs, "map2", p.map2); addr(ptrs, "map_rec", p.map_rec);
    addr(ptrs, "map_pool", p.map_pool);
    const DevUni T = uni_fill_params(view, p);
    return block_bytes(T, offsetof(DevUni, mpool) + sizeof T.mpool);
  }, py::arg("spec"), py::arg("ptrs"));
}
