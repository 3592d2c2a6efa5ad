// Standalone self-test of the Unigram token counter (csrc/common/unigram.h), built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_unigram_sanitizers.py:
//
//   * a small vocabulary with scores in the open-addressed piece table (pieces of one to three
//     bytes per character, a longest piece of 16 code points, pieces whose scores tie with the sum
//     of their parts), a class table with keep, space and host code points, two added tokens and
//     the unk piece's text behind the first-byte mask; with and without byte_fallback
//   * adversarial words and documents in exactly sized heap buffers (a read past the end is a
//     report): words far longer than the ring, runs of unknown characters of 2 to 4 bytes next to
//     known text, the longest piece alone and repeated, space runs, host code points, added-token
//     text, truncated and stray UTF-8
//   * uni_count_doc against a plain std::string implementation of what the library does: the text
//     cut into words at the space code points, each word encoded as U+2581 + word by a Viterbi over
//     whole arrays with back pointers (the shortest piece wins a tie, the unknown edge where no
//     piece of one character matched), then backtracked with fuse_unk and byte_fallback
//   * and against the sum of uni_count_range over chunks of 1, 2, 3, 5, 16, 17 and 64 bytes (the
//     kernel's lane split)
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

struct Tok {
  std::vector<uint8_t> pool, cls2;
  std::vector<uint16_t> cls1;
  std::vector<uint64_t> slots;
  std::string added = "<s></s><unk>";
  std::vector<int32_t> aoff = {0, 3, 7, 12};
  std::map<std::string, double> score;  // the reference's view of the vocabulary
  double unk_score = 0;
  bool byte_fallback;
  UniSpecView spec;
  DevUni T{};

  static int cls_of(uint32_t c) {
    if (c == ' ' || c == '\n' || c == '\t' || c == 0xA0 || c == 0x3000) return UNI_SPACE;
    if (c < 0x20 || c == 0x7F || c == 0x2026 || c == 0x2581 || (c >= 0x300 && c < 0x370) || c == 0x200D ||
        (c >= 0xD800 && c < 0xE000))
      return UNI_HOST;
    return UNI_KEEP;
  }

  explicit Tok(bool bf) : byte_fallback(bf) {
    const std::vector<std::pair<std::string, double>> vocab = {
        {"<unk>", 0.0}, {kSp, -2.0}, {"a", -3.0}, {"b", -3.5}, {"c", -4.0}, {"ab", -4.5}, {"bc", -5.0},
        {"aa", -6.0},  // ties with a + a: the shorter piece's path stays
        {"abc", -7.5},  // ties with a + bc... and ab + c is -8.5
        {kSp + "a", -5.0},  // ties with U+2581 + a
        {kSp + "ab", -6.0}, {"\xC3\xA9", -6.0}, {"a\xC3\xA9", -8.5}, {"\xE3\x81\x82", -7.0},
        {"\xE3\x81\x82\xE3\x81\x82\xE3\x81\x82", -9.0}, {kLongest, -11.0}, {"cabcabcabcabcabc", -30.25}, {".", -4.25},
        {"x", -12.5}};
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
    if (const char* e = uni_spec_error(spec)) {
      std::fprintf(stderr, "FAIL: the spec is refused: %s\n", e);
      std::exit(1);
    }
    T = uni_fill_params(spec, uni_host_ptrs(spec));
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

static int32_t ref_count(const Tok& V, const std::string& doc) {
  for (const char* a : {"<s>", "</s>", "<unk>"})
    if (doc.find(a) != std::string::npos) return kBpeHost;
  std::vector<std::string> ch;
  std::vector<uint32_t> cps;
  if (!chars_of(doc, &ch, &cps)) return kBpeHost;
  for (uint32_t c : cps)
    if (Tok::cls_of(c) == UNI_HOST) return kBpeHost;
  int64_t total = 0;
  std::vector<std::string> word;
  for (size_t i = 0; i <= ch.size(); ++i) {
    if (i == ch.size() || Tok::cls_of(cps[i]) == UNI_SPACE) {
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
  // a ring of exactly longest_cp + 1 entries
  std::unique_ptr<double[]> rs(new double[(size_t)V.T.longest_cp + 1]);
  std::unique_ptr<uint32_t[]> rm(new uint32_t[(size_t)V.T.longest_cp + 1]);
  const UniRing R{rs.get(), rm.get(), 1};
  const int32_t want = ref_count(V, doc);
  const int32_t got = uni_count_doc(V.T, buf.get(), n, R);
  if (got != want) {
    ++g_fail;
    std::fprintf(stderr, "FAIL %s (byte_fallback %d, %lld bytes): counter %d, reference %d\n", what, (int)V.byte_fallback,
                 (long long)n, got, want);
  }
  for (int64_t chunk : {1, 2, 3, 5, 16, 17, 64}) {
    int64_t tot = V.T.post_add;
    bool bad = uni_has_added(V.T, buf.get(), n, 0, n);
    for (int64_t s0 = 0; s0 < n && !bad; s0 += chunk) {
      const int64_t x = uni_count_range(V.T, buf.get(), n, s0, std::min(n, s0 + chunk), R);
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

int main(int argc, char** argv) {
  const int n_random = argc > 1 ? std::atoi(argv[1]) : 2000;
  const std::string E = "\xC3\xA9", A = "\xE3\x81\x82", U2 = "\xC3\xBC", U3 = "\xE6\x97\xA5", U4 = "\xF0\x9F\x98\x80";
  auto rep = [](const std::string& s, int k) {
    std::string o;
    for (int i = 0; i < k; ++i) o += s;
    return o;
  };
  const std::string longest_word = kLongest.substr(3);
  std::vector<std::pair<std::string, const char*>> docs = {
      {"", "empty"}, {" ", "a space"}, {" \n\t\xC2\xA0\xE3\x80\x80 ", "white space"}, {"a", "one piece"},
      {"aa", "a tie of pieces"}, {"abc", "a tie of paths"}, {"ab abc  a\nb", "words"}, {longest_word, "the longest piece"},
      {longest_word + "a", "the longest piece and one more"}, {rep(longest_word, 9), "the longest piece repeated"},
      {longest_word.substr(0, 14), "the longest piece cut short"}, {"bcabcabcabcabcabcab", "a longest piece inside a word"},
      {rep("a", 700), "a word of 700 known characters"}, {rep("abc", 1000) + U3, "a word of 3000 bytes"},
      {rep(U3, 100), "a run of unknown characters"}, {rep(U4, 70) + "a" + rep(U2, 3), "unknown runs around a piece"},
      {"a" + U2 + "b" + U3 + U3 + "c" + U4, "unknowns between pieces"}, {U2, "one unknown"}, {"zzz", "unknown ASCII"},
      {"a" + E + " " + E + E + A + A + A + A, "pieces of two and three bytes"}, {"x" + rep(A, 40), "forty of a piece"},
      {"ab\xE2\x80\xA6", "a host code point"}, {"e\xCC\x81", "a combining mark"}, {"a\x01", "a control"},
      {"a" + kSp + "b", "a literal U+2581"}, {"hi </s> there", "an added token"}, {"<unk>", "the unk piece's text"},
      {"<un k> <s", "almost added tokens"}, {rep("a ", 40) + "</s>", "an added token at the end"},
      {"abc \xff def", "a stray byte"}, {"abc \xc3", "a truncated sequence at the end"}, {"\x80" "abc", "a continuation first"},
      {"ab \xe2\x82 cd", "a truncated sequence inside"}, {rep("x", 15) + "\xc3\xa9\xa9", "a stray continuation at a lane edge"},
      {"\xed\xa0\x80", "a surrogate"}, {"\xf4\x90\x80\x80", "past U+10FFFF"}, {"\xc0\xaf", "an overlong form"},
  };
  const std::vector<std::string> pool = {"a",  "b",  "c",  "ab", "abc", "x", ".", " ", "  ", "\n", "\xC2\xA0", E,  A,
                                         U2,   U3,   U4,   "z",  longest_word, "aa", "<", "<s", "</s>", "\xE2\x80\xA6",
                                         "\xff", "\xCC\x81"};
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
  std::printf("%d documents, %d failures\n", checked, g_fail);
  return g_fail ? 1 : 0;
}
