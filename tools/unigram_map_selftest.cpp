// Standalone self-test of the Unigram token counter over a normalizer's replacements
// (csrc/common/unigram.h unim_*), built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_unigram_map_sanitizers.py:
//
//   * the small vocabulary of unigram_selftest.cpp, and a class table with keep, space, host and
//     map code points whose records are: outputs of one to three code points that spell pieces
//     (full-width a, b, c; a ligature for "abc"; U+2026 for "..."), an output that begins with a
//     separator (U+00A8), ends with one (U+2024) or has one inside (U+2025), outputs of unknown
//     characters (U+00BD), drops (U+0001..0008), the characters that spell the unk piece's text,
//     one output of exactly the cap, and a space code point that joins the grapheme in front of it
//     (U+200C: a document with a map code point directly before it goes to the host); with and
//     without byte_fallback
//   * adversarial documents in exactly sized heap buffers, the map's tables in exactly sized
//     vectors (a read past the end of either is a report)
//   * unim_count_doc against a plain std::string implementation: the normalised text materialised,
//     cut into words at U+0020, each word encoded as U+2581 + word by a Viterbi over whole arrays
//     with back pointers, then backtracked with fuse_unk and byte_fallback; a document whose
//     normalised text spells the unk piece goes to the host
//   * and against the sum of unim_count_range over chunks of 1, 2, 3, 5, 16, 17 and 64 bytes (the
//     kernel's lane split)
//   * the validator's refusals: a record past the pool, a length over the cap, a stage-2 block past
//     its array, a map code point without a record
//
// Exits non-zero on any mismatch; sanitizer reports abort the run.
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "tok_selftest.h"

using namespace tb;

static int g_fail = 0;
static const std::string kSp = "\xE2\x96\x81";
static const std::string kLongest = kSp + "abcabcabcabcabc";  // 16 code points

// code point -> what the normalizer makes of it (separators as 0x20)
static const std::map<uint32_t, std::string>& replacements() {
  static const std::map<uint32_t, std::string> m = {
      {0xFF41, "a"}, {0xFF42, "b"}, {0xFF43, "c"}, {0xFB01, "abc"}, {0x2026, "..."}, {0xA8, " \xCC\x88"},
      {0x2024, "a "}, {0x2025, "a b"}, {0xBD, "1\xE2\x81\x84" "2"}, {0x2122, "x"},
      {0x01, ""}, {0x02, ""}, {0x03, ""}, {0x08, ""}, {0xAD, ""},
      {0xFF1C, "<"}, {0xFF1E, ">"}, {0xFF55, "u"}, {0xFF4E, "n"}, {0xFF4B, "k"},
      {0x3300, std::string("\xE3\x81\x82\xE3\x81\x82\xE3\x81\x82\xE3\x81\x82\xE3\x81\x82\xE3\x81\x82\xE3\x81\x82\xE3\x81\x82"
                           "\xE3\x81\x82\xE3\x81\x82" "ab")},  // 32 bytes: the cap
  };
  return m;
}

static const uint32_t kJoin = 0x200C;  // a space that joins the grapheme in front of it

struct Tok {
  std::vector<uint8_t> pool, cls2, map_pool;
  std::vector<uint16_t> cls1, map1, map2;
  std::vector<uint32_t> map_rec;
  std::vector<uint64_t> slots;
  std::string added = "<s></s><unk>";
  std::vector<int32_t> aoff = {0, 3, 7, 12};
  std::map<std::string, double> score;  // the reference's view of the vocabulary
  double unk_score = 0;
  bool byte_fallback;
  UniSpecView spec;
  DevUni T{};

  static int cls_of(uint32_t c) {
    if (c == ' ' || c == '\n' || c == '\t' || c == 0xA0 || c == 0x3000 || c == kJoin) return UNI_SPACE;
    if (replacements().count(c)) return UNI_MAP;
    if (c < 0x20 || c == 0x7F || c == 0x2581 || (c >= 0x300 && c < 0x370) || c == 0x200D || (c >= 0xD800 && c < 0xE000))
      return UNI_HOST;
    return UNI_KEEP;
  }

  explicit Tok(bool bf) : byte_fallback(bf) {
    const std::vector<std::pair<std::string, double>> vocab = {
        {"<unk>", 0.0}, {kSp, -2.0}, {"a", -3.0}, {"b", -3.5}, {"c", -4.0}, {"ab", -4.5}, {"bc", -5.0},
        {"aa", -6.0}, {"abc", -7.5}, {kSp + "a", -5.0}, {kSp + "ab", -6.0}, {"\xC3\xA9", -6.0}, {"a\xC3\xA9", -8.5},
        {"\xE3\x81\x82", -7.0}, {"\xE3\x81\x82\xE3\x81\x82\xE3\x81\x82", -9.0}, {kLongest, -11.0},
        {"cabcabcabcabcabc", -30.25}, {".", -4.25}, {"..", -8.0}, {"x", -12.5}, {"</s>", 0.0}, {"<", -9.0}};
    std::vector<int64_t> off{0};
    std::vector<double> sc;
    double lo = 0;
    int longest = 0, longest_cp = 0;
    for (const auto& v : vocab) {
      pool.insert(pool.end(), v.first.begin(), v.first.end());
      off.push_back((int64_t)pool.size());
      sc.push_back(v.second);
      score[v.first] = v.second;
      lo = v.second < lo ? v.second : lo;
      int cp = 0;
      for (char ch : v.first) cp += ((uint8_t)ch & 0xC0) != 0x80;
      longest = std::max(longest, (int)v.first.size());
      longest_cp = std::max(longest_cp, cp);
    }
    unk_score = lo - 10.0;
    const size_t cap = tok_table_cap(vocab.size());
    std::vector<UniSlot> table(cap, UniSlot{0, kWpEmpty, 0});
    uni_fill_slots(pool.data(), off.data(), sc.data(), vocab.size(), 0, table.data(), cap - 1);
    for (const UniSlot& s : table) {
      slots.push_back(s.key);
      slots.push_back(s.val);
      slots.push_back(s.score);
    }
    cls1.resize(kUniClsStage1);
    cls2.assign(kUniClsStage1 * 32, 0);
    for (uint32_t c = 0; c < 0x110000; ++c) {
      cls1[c >> 7] = (uint16_t)(c >> 7);
      cls2[(size_t)(c >> 7) * 32 + ((c & 127) >> 2)] |= (uint8_t)(cls_of(c) << (2 * (c & 3)));
    }
    // the map: block 0 is empty, every block with a record gets its own
    map1.assign(kUniClsStage1, 0);
    map2.assign(128, kUniMapNone);
    auto record = [&](uint32_t c, uint32_t rec) {
      if (map1[c >> 7] == 0) {
        map1[c >> 7] = (uint16_t)(map2.size() / 128);
        map2.insert(map2.end(), 128, kUniMapNone);
      }
      map2[(size_t)map1[c >> 7] * 128 + (c & 127)] = (uint16_t)map_rec.size();
      map_rec.push_back(rec);
    };
    for (const auto& r : replacements()) {
      record(r.first, (uint32_t)(map_pool.size() << 8) | (uint32_t)r.second.size());
      map_pool.insert(map_pool.end(), r.second.begin(), r.second.end());
    }
    record(kJoin, kUniRecJoin);
    spec.slots = span_of(slots);
    spec.pool = span_of(pool);
    spec.cls1 = span_of(cls1);
    spec.cls2 = span_of(cls2);
    spec.added = span_of(added);
    spec.added_off = span_of(aoff);
    spec.sp = span_of(kSp);
    spec.mask = (uint32_t)(cap - 1);
    spec.flags = bf ? kUniByteFallback : 0;
    spec.longest_cp = longest_cp;
    spec.longest = longest;
    spec.post_add = 1;
    spec.unk_score = unk_score;
    spec.map1 = span_of(map1);
    spec.map2 = span_of(map2);
    spec.map_rec = span_of(map_rec);
    spec.map_pool = span_of(map_pool);
    if (const char* e = uni_spec_error(spec)) {
      std::fprintf(stderr, "FAIL: the spec is refused: %s\n", e);
      std::exit(1);
    }
    T = uni_fill_params(spec, uni_host_ptrs(spec));
    if (!uni_has_map(T)) {
      std::fprintf(stderr, "FAIL: the block has no map\n");
      std::exit(1);
    }
  }
};

// the code points of s as strings, false on invalid UTF-8
static bool chars_of(const std::string& s, std::vector<std::string>* out, std::vector<uint32_t>* cps) {
  const uint8_t* b = reinterpret_cast<const uint8_t*>(s.data());
  const int64_t n = (int64_t)s.size();
  for (int64_t i = 0; i < n;) {
    int l;
    const int32_t c = bpe_decode(b, i, n, &l);
    if (c < 0) return false;
    out->push_back(s.substr((size_t)i, (size_t)l));
    cps->push_back((uint32_t)c);
    i += l;
  }
  return true;
}

// tokens of one word: the library's encode_optimized over U+2581 + word, then tokenize
static int64_t ref_word(const Tok& V, const std::vector<std::string>& word) {
  std::vector<std::string> ch{kSp};
  ch.insert(ch.end(), word.begin(), word.end());
  const size_t n = ch.size();
  std::vector<double> best(n + 1, 0.0);
  std::vector<int> from(n + 1, -1);
  std::vector<bool> unk(n + 1, false);
  for (size_t s = 0; s < n; ++s) {
    bool single = false;
    std::string piece;
    for (size_t e = s + 1; e <= n; ++e) {  // increasing length, as the trie's common prefix search
      piece += ch[e - 1];
      const auto it = V.score.find(piece);
      if (it == V.score.end()) continue;
      const double cand = it->second + best[s];
      if (from[e] < 0 || cand > best[e]) {
        best[e] = cand;
        from[e] = (int)s;
        unk[e] = false;
      }
      if (e == s + 1) single = true;
    }
    if (!single) {
      const double cand = V.unk_score + best[s];
      if (from[s + 1] < 0 || cand > best[s + 1]) {
        best[s + 1] = cand;
        from[s + 1] = (int)s;
        unk[s + 1] = true;
      }
    }
  }
  int64_t tokens = 0;
  std::string fused;
  auto flush = [&]() {
    if (fused.empty()) return;
    tokens += V.byte_fallback ? (int64_t)fused.size() : 1;  // an unknown string: its bytes, or one unk
    fused.clear();
  };
  for (size_t e = n; e > 0; e = (size_t)from[e]) {
    if (unk[e]) {
      for (size_t k = (size_t)from[e]; k < e; ++k) fused += ch[k];
    } else {
      flush();
      ++tokens;
    }
  }
  flush();
  return tokens;
}

// the document as the steps behind the normalizer see it (separators as U+0020); false: host
static bool normalised(const std::string& doc, std::string* out) {
  for (const char* a : {"<s>", "</s>", "<unk>"})
    if (doc.find(a) != std::string::npos) return false;
  std::vector<std::string> ch;
  std::vector<uint32_t> cps;
  if (!chars_of(doc, &ch, &cps)) return false;
  for (size_t i = 0; i < ch.size(); ++i) {
    const int k = Tok::cls_of(cps[i]);
    if (k == UNI_HOST) return false;
    if (k == UNI_MAP && i + 1 < ch.size() && cps[i + 1] == kJoin) return false;  // the map code point swallows it
    *out += k == UNI_SPACE ? std::string(" ") : (k == UNI_MAP ? replacements().at(cps[i]) : ch[i]);
  }
  return out->find("<unk>") == std::string::npos;
}

static int32_t ref_count(const Tok& V, const std::string& doc) {
  std::string text;
  if (!normalised(doc, &text)) return kBpeHost;
  std::vector<std::string> ch;
  std::vector<uint32_t> cps;
  if (!chars_of(text, &ch, &cps)) return kBpeHost;
  int64_t total = 0;
  std::vector<std::string> word;
  for (size_t i = 0; i <= ch.size(); ++i) {
    if (i == ch.size() || cps[i] == ' ') {
      if (!word.empty()) total += ref_word(V, word);
      word.clear();
    } else {
      word.push_back(ch[i]);
    }
  }
  return (int32_t)(total + V.T.post_add);
}

static void check_doc(const Tok& V, const std::string& doc, const char* what) {
  const int64_t n = (int64_t)doc.size();
  std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)n]);  // exactly n bytes
  if (n) std::memcpy(buf.get(), doc.data(), (size_t)n);
  std::unique_ptr<double[]> rs(new double[(size_t)V.T.longest_cp + 1]);
  std::unique_ptr<uint32_t[]> rm(new uint32_t[(size_t)V.T.longest_cp + 1]);
  const UniRing R{rs.get(), rm.get(), 1};
  const int32_t want = ref_count(V, doc);
  const int32_t got = unim_count_doc(V.T, buf.get(), n, R);
  if (got != want) {
    ++g_fail;
    std::fprintf(stderr, "FAIL %s (byte_fallback %d, %lld bytes): counter %d, reference %d\n", what, (int)V.byte_fallback,
                 (long long)n, got, want);
  }
  for (int64_t chunk : {1, 2, 3, 5, 16, 17, 64}) {
    int64_t tot = V.T.post_add;
    bool bad = uni_has_added(V.T, buf.get(), n, 0, n);
    for (int64_t s0 = 0; s0 < n && !bad; s0 += chunk) {
      const int64_t x = unim_count_range(V.T, buf.get(), n, s0, std::min(n, s0 + chunk), R);
      if (x < 0) bad = true;
      tot += x;
    }
    const int32_t split = bad ? kBpeHost : (int32_t)tot;
    if (split != got) {
      ++g_fail;
      std::fprintf(stderr, "FAIL %s (byte_fallback %d, %lld bytes): chunks of %lld give %d, the document %d\n", what,
                   (int)V.byte_fallback, (long long)n, (long long)chunk, split, got);
    }
  }
}

static void expect_refused(Tok V, const char* what, void (*change)(Tok&)) {
  change(V);
  V.spec.map1 = span_of(V.map1);
  V.spec.map2 = span_of(V.map2);
  V.spec.map_rec = span_of(V.map_rec);
  V.spec.map_pool = span_of(V.map_pool);
  V.spec.cls2 = span_of(V.cls2);
  if (uni_spec_error(V.spec) == nullptr) {
    ++g_fail;
    std::fprintf(stderr, "FAIL: the validator accepts %s\n", what);
  }
}

int main(int argc, char** argv) {
  const int n_random = argc > 1 ? std::atoi(argv[1]) : 2000;
  const std::string E = "\xC3\xA9", A = "\xE3\x81\x82", U2 = "\xC3\xBC", U3 = "\xE6\x97\xA5", U4 = "\xF0\x9F\x98\x80";
  const std::string FA = "\xEF\xBD\x81", FB = "\xEF\xBD\x82", FC = "\xEF\xBD\x83", LIG = "\xEF\xAC\x81", ELL = "\xE2\x80\xA6",
                    DIA = "\xC2\xA8", ONE = "\xE2\x80\xA4", TWO = "\xE2\x80\xA5", HALF = "\xC2\xBD", TM = "\xE2\x84\xA2",
                    SHY = "\xC2\xAD", LT = "\xEF\xBC\x9C", GT = "\xEF\xBC\x9E", FU = "\xEF\xBD\x95", FN = "\xEF\xBD\x8E",
                    FK = "\xEF\xBD\x8B", CAP = "\xE3\x8C\x80", ZWNJ = "\xE2\x80\x8C";
  auto rep = [](const std::string& s, int k) {
    std::string o;
    for (int i = 0; i < k; ++i) o += s;
    return o;
  };
  const std::string longest_fw = rep(FA + FB + FC, 5);  // the longest piece's word in full-width letters
  std::vector<std::pair<std::string, const char*>> docs = {
      {"", "empty"}, {"a", "one piece"}, {"ab abc  a\nb", "words"}, {FA, "a full-width piece"}, {FA + FB + FC, "a full-width tie"},
      {longest_fw, "the longest piece in full-width letters"}, {longest_fw + "a", "... and one more"},
      {rep(longest_fw, 9), "... repeated"}, {"abc" + rep(LIG, 4), "the longest piece from ligatures"},
      {rep(LIG, 300), "a word of 300 ligatures"}, {"a" + DIA + "b", "a word starts inside an output"}, {DIA, "that output alone"},
      {"a" + DIA, "... at the end"}, {DIA + DIA + "a", "... twice"}, {"a\x01" "b", "a drop inside a word"},
      {"a" + rep("\x01", 40) + "b", "forty drops inside a word"}, {"\x01\x02\x03", "drops only"}, {"a \x01\x08 b", "drops between spaces"},
      {"\x01" "a", "a drop first"}, {"a\x01", "a drop last"}, {SHY + "a" + SHY + SHY + "b" + SHY, "two-byte drops"},
      {ELL + "a", "an ellipsis first"}, {"a" + ELL, "an ellipsis last"}, {"a" + ELL + ELL + "b", "an ellipsis doubled"},
      {rep(ELL, 700), "700 ellipses"}, {HALF, "an output of unknowns"}, {"a" + HALF + "b", "... inside a word"}, {"x" + TM, "a rare piece"},
      {ONE, "an output that ends with a separator"}, {ONE + "b", "... before a word"}, {"b" + ONE + ONE + "b", "... twice"},
      {TWO, "an output with a separator inside"}, {"b" + TWO + "b", "... inside a word"}, {rep(TWO, 50), "... fifty times"},
      {"\x01" + TWO + "\x02" + DIA + "\x03" + ONE + "\x08", "drops around outputs"}, {CAP, "an output of the cap"},
      {"a" + CAP + CAP + "b", "... twice inside a word"}, {"a" + LT + FU + FN + FK + GT + "b", "the unk piece's text spelled"},
      {LT + "unk>", "... with one replacement"}, {"<un" + FK + GT, "... at its end"}, {LT + "/s>", "an added token's text spelled"},
      {LT + "s>", "another one, no piece"}, {"a" + LT + "/s" + GT + "b", "... inside a word"},
      {"hi </s> there", "an added token"}, {"<unk>", "the unk piece's text"}, {"a\x7f", "a host control"},
      {"e\xCC\x81", "a combining mark"}, {"a" + kSp + "b", "a literal U+2581"}, {"abc \xff def", "a stray byte"},
      {"abc \xc3", "a truncated sequence at the end"}, {"\x80" "abc", "a continuation first"},
      {rep("x", 15) + "\xc3\xa9\xa9", "a stray continuation at a lane edge"}, {ELL.substr(0, 2), "a truncated ellipsis"},
      {"ab" + ELL.substr(1), "continuation bytes of an ellipsis"}, {"a" + ZWNJ + "b", "a joining space behind a keep code point"},
      {"a" + DIA + ZWNJ + "b", "... behind a map code point"}, {"a\x01" + ZWNJ + "b", "... behind a drop"},
      {ZWNJ + DIA + " " + ZWNJ, "... in front of one, and behind a space"}, {"a" + DIA + ZWNJ.substr(0, 2), "... truncated"},
  };
  for (int lead = 12; lead < 19; ++lead) {  // replacements across the edge of 16-byte ranges
    docs.push_back({rep("a", lead) + ELL + "b", "an ellipsis at a lane edge"});
    docs.push_back({rep("a", lead) + DIA + "b", "a word start inside an output at a lane edge"});
    docs.push_back({rep("a", lead) + TWO + "b", "a separator inside an output at a lane edge"});
    docs.push_back({rep("a", lead) + rep("\x01", 17) + "b", "a lane of drops"});
    docs.push_back({rep("a", lead) + " " + rep(SHY, 20) + "b", "a lane of drops behind a space"});
    docs.push_back({rep("a", lead) + " " + longest_fw + " b", "the full-width longest piece at a lane edge"});
  }
  const std::vector<std::string> pool = {"a", "b", "c", "ab", "abc", "x", ".", " ", "  ", "\n", E, A, U2, U3, U4, "z", FA, FB, FC,
                                         LIG, ELL, DIA, ONE, TWO, HALF, TM, "\x01", "\x02\x03", SHY, CAP, longest_fw, ZWNJ, "<", LT, GT,
                                         FU + FN + FK, "/s", "unk", ">", "</s>", "\x7f", "\xff", "\xCC\x81"};
  std::mt19937 rng(12345);
  int checked = 0;
  for (int bf = 0; bf < 2; ++bf) {
    const Tok V(bf != 0);
    for (const auto& d : docs) {
      check_doc(V, d.first, d.second);
      ++checked;
    }
    for (int i = 0; i < n_random; ++i) {
      std::string s;
      // mostly countable text; every eighth document may hold a host or invalid entry
      const size_t top = i % 8 == 0 ? pool.size() : pool.size() - 4;
      for (int k = (int)(rng() % 48); k > 0; --k) s += pool[rng() % top];
      check_doc(V, s, "random");
      ++checked;
    }
  }
  const Tok V(false);
  expect_refused(V, "a record past the pool", [](Tok& t) { t.map_rec.back() = (uint32_t)(t.map_pool.size() << 8) | 1; });
  expect_refused(V, "a length over the cap", [](Tok& t) { t.map_rec[0] = kUniMaxMapBytes + 1; });
  expect_refused(V, "a stage-2 block past its array", [](Tok& t) { t.map2.resize(t.map2.size() - 1); });
  expect_refused(V, "a record number past the records", [](Tok& t) { t.map2[0] = (uint16_t)t.map_rec.size(); });
  expect_refused(V, "a map code point without a record", [](Tok& t) {
    for (auto& r : t.map2) r = kUniMapNone;
  });
  expect_refused(V, "a map code point with a joining space's record", [](Tok& t) { t.map_rec[1] |= kUniRecJoin; });
  expect_refused(V, "a record of a keep code point", [](Tok& t) { t.map2[(size_t)t.map1[0] * 128 + 'a'] = 1; });
  expect_refused(V, "a map without a pool", [](Tok& t) { t.map_pool.clear(); });
  std::printf("%d documents, %d failures\n", checked, g_fail);
  return g_fail ? 1 : 0;
}
