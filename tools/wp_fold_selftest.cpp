// Standalone self-test of the folding WordPiece token counter (csrc/common/wordpiece.h wpf_*, the
// tables of wp_fold.inc), built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_wordpiece_fold_sanitizers.py:
//
//   * a small vocabulary with jamo, accent-stripped and lower-cased pieces, in each of the three
//     fold modes (lowercase, strip_accents, both), with max_chars 100 and 3
//   * adversarial documents in exactly sized heap buffers (an over-read is a report): stripped
//     marks and drops between letters, words of marks only, piece boundaries inside a Hangul
//     syllable and inside U+0130's two output code points, classes that come from the output,
//     99 / 102 output characters, context-dependent code points, added-token text, broken UTF-8
//   * wp_count_doc_t<true> against a plain std::string implementation of the same rules, and
//     against the sum of wpf_count_range over chunks of 1, 7, 16 and 64 bytes (the lane split)
//
// Exits non-zero on any mismatch; sanitizer reports abort the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "tok_selftest.h"

using namespace tb;

static int g_fail = 0;

struct Vocab {
  WpSelfTables tab;
  std::vector<int64_t> off{0};
  std::vector<uint8_t> cont;
  std::set<std::pair<int, std::string>> pieces;
  DevWp T{};

  void add(int c, const std::string& s) {
    if (!pieces.insert({c, s}).second) return;
    tab.pool.insert(tab.pool.end(), s.begin(), s.end());
    off.push_back((int64_t)tab.pool.size());
    cont.push_back((uint8_t)c);
  }

  void finish(int fold, int max_chars) {
    tab.set_pieces(off, cont);
    tab.added = "[CLS][MASK]";
    tab.aoff = {0, 5, 11};
    tab.spec.fold = fold;
    tab.spec.flags = kWpChinese | ((fold & 1) ? kWpLower : 0);
    tab.spec.max_chars = max_chars;
    tab.spec.post_add = 2;
    T = tab.params();
  }
};

// the same rules over std::string: normalise code point by code point, split into words of output
// characters, then greedy longest-first matching in a set
static int32_t reference(const Vocab& V, const uint8_t* b, int64_t n) {
  const std::string doc(reinterpret_cast<const char*>(b), (size_t)n);
  if (doc.find("[CLS]") != std::string::npos || doc.find("[MASK]") != std::string::npos) return kBpeHost;
  std::vector<std::vector<std::string>> words;  // each a list of output characters
  bool open = false;
  for (int64_t i = 0; i < n;) {
    const WpOut c = wpf_cp(V.T, b, i, n);
    if (c.cls < 0) return kBpeHost;
    if (c.cls == WP_KEEP) {
      std::string out;
      for (int j = 0; j < c.nb; ++j) out += (char)wpf_byte(V.T, b, i, c, j);
      if (!open) words.emplace_back();
      open = true;
      for (size_t j = 0; j < out.size();) {
        const int l = wp_u8len((uint8_t)out[j]);
        words.back().push_back(out.substr(j, (size_t)l));
        j += (size_t)l;
      }
    } else if (c.cls != WP_DROP) {
      open = false;
      if (c.cls == WP_ISO) words.push_back({"?"});
    }
    i += c.len;
  }
  int64_t total = V.T.post_add;
  for (const auto& w : words) {
    if ((int64_t)w.size() > V.T.max_chars) { ++total; continue; }
    if (w.size() == 1 && w[0] == "?") { ++total; continue; }  // an isolate: one token, known or not
    size_t pos = 0;
    int64_t pieces = 0;
    while (pos < w.size()) {
      size_t e = w.size();
      for (; e > pos; --e) {
        std::string s;
        for (size_t j = pos; j < e; ++j) s += w[j];
        if (V.pieces.count({pos > 0, s})) break;
      }
      if (e == pos) { pieces = 1; break; }
      ++pieces;
      pos = e;
    }
    total += pieces;
  }
  return (int32_t)total;
}

#define GA "\xEA\xB0\x80"   // U+AC00: two jamo
#define GAK "\xEA\xB0\x81"  // U+AC01: three jamo
#define JG "\xE1\x84\x80"   // U+1100
#define JA "\xE1\x85\xA1"   // U+1161
#define JK "\xE1\x86\xA8"   // U+11A8
#define ACUTE "\xCC\x81"    // U+0301
#define SHY "\xC2\xAD"      // U+00AD
#define IDOT "\xC4\xB0"     // U+0130
#define DOT "\xCC\x87"      // U+0307

static std::string rep(const std::string& s, int k) {
  std::string r;
  for (int i = 0; i < k; ++i) r += s;
  return r;
}

static std::string random_doc(std::mt19937_64& rng) {
  static const char* parts[] = {"the", "The", "ing", "s", "a", "e", "x", "i", "I", " ", " ", "\n", SHY, ACUTE,
                                "\xCC\x88", "\xC3\xA9", "\xC3\x89", "\xC3\xA5", "\xC3\x85", "\xC3\x86", "\xE2\x84\xAB",
                                GA, GAK, "\xED\x9E\xA3", JG, JA, IDOT, DOT, "\xCD\xBE", "\xE2\x89\xA0", "\xE1\xBF\xAF",
                                ";", "=", "\xE4\xBD\xA0", "\xEF\xA4\x80", "\xE3\x81\x8C", "\xE0\xB8\x81\xE0\xB9\x88",
                                "\xE2\x80\x8B", "\xC2\xA0", "\xE2\x80\x80", "!", "[CL", "S]", "\xCE\xA3",
                                "\xCF\x82", "\xEF\xAC\x81", "\xC7\x85", "\xF0\x9F\x98\x80"};
  static const char* broken[] = {"\xFF", "\xC3", "\x80", "\xE2\x82", "\xEA\xB0", "\xED\xA0\x80", "\xC0\xAF", "[CLS]"};
  std::string s;
  const int n = (int)(rng() % 50);
  for (int i = 0; i < n; ++i) {
    s += parts[rng() % (sizeof(parts) / sizeof(*parts))];
    if (rng() % 211 == 0) s += "\xE3\x80\xAE";  // U+302E: to the host in the strip modes
    if (rng() % 97 == 0) s += broken[rng() % (sizeof(broken) / sizeof(*broken))];
  }
  return s;
}

static void run(const Vocab& V, const char* name, int ndocs, uint64_t seed) {
  std::mt19937_64 rng(seed);
  std::vector<std::string> docs = {
      "", " ", "e" ACUTE "x", "a" ACUTE SHY ACUTE "b", ACUTE "\xCC\x88" ACUTE, "x " ACUTE " y", GA GAK, GAK, "a" GA "b",
      IDOT "stanbul", "a" IDOT, IDOT IDOT, "x\xCD\xBEy", "a\xE2\x89\xA0" "b", "\xE1\xBF\xAF", rep(GAK, 33),
      rep(GAK, 34),
      rep(GA, 50), rep(GA, 51), rep("\xC3\xA9", 100), rep("\xC3\xA9", 101), "\xE2\x84\xAB", "\xE3\x81\x8C",
      "a\xE3\x80\xAE" "b", "[CLS]" GA, GAK "[MASK]", "\xEF\xA4\x80 a\xEF\xA4\x80" "b", std::string(5000, 'x'),
      rep(GAK, 700)};
  for (int k = 0; k < 9; ++k) docs.push_back(std::string((size_t)k, 'x') + rep(GAK, 8));
  for (int i = 0; i < 40; ++i) docs.push_back(std::string((size_t)i, 'a') + "e" ACUTE GAK IDOT "the");
  for (int i = 0; i < ndocs; ++i) docs.push_back(random_doc(rng));
  int host = 0;
  for (const std::string& d : docs) {
    const int64_t n = (int64_t)d.size();
    std::unique_ptr<uint8_t[]> buf(new uint8_t[d.size()]);  // no slack: reads past n are reports
    std::memcpy(buf.get(), d.data(), d.size());
    const uint8_t* b = buf.get();
    const int32_t want = reference(V, b, n), got = wp_count_doc_t<true>(V.T, b, n);
    host += got == kBpeHost;
    if (got != want) {
      std::fprintf(stderr, "FAIL %s: doc of %lld bytes: %d, reference %d\n", name, (long long)n, got, want);
      ++g_fail;
    }
    for (int64_t chunk : {1, 7, 16, 64}) {
      int64_t tot = V.T.post_add;
      bool bad = wp_has_added(V.T, b, n, 0, n);
      for (int64_t s0 = 0; s0 < n && !bad; s0 += chunk) {
        const int64_t x = wpf_count_range(V.T, b, n, s0, s0 + chunk < n ? s0 + chunk : n);
        if (x < 0) bad = true;
        tot += x;
      }
      const int32_t split = bad ? kBpeHost : (int32_t)tot;
      if (split != got) {
        std::fprintf(stderr, "FAIL %s: chunk %lld: %d, whole %d\n", name, (long long)chunk, split, got);
        ++g_fail;
      }
    }
  }
  std::printf("%s: %zu documents, %d to the host\n", name, docs.size(), host);
}

int main(int argc, char** argv) {
  const int ndocs = argc > 1 ? std::atoi(argv[1]) : 2000;
  static const char* names[] = {"lowercase", "strip_accents", "both"};
  for (int fold = 1; fold <= 3; ++fold) {
    Vocab V;
    for (const char* w : {"the", "a", "aa", "e", "x", "i", "s", "t", "th", "ex", "ab", JG, JG JA, JG JA JK JG,
                          "istanbul",
                          "i" DOT, "\xC3\xA9", "\xC3\xA5", "\xC3\xA6", "\xE3\x81\x8B", "\xE0\xB8\x81", "\xCF\x83", "!",
                          ";", "=", "fi", "\xC7\x86", "xxxxxxxxxxxx" JG})
      V.add(0, w);
    if (!(fold & 1)) for (const char* w : {"The", "I", "E", "A", "\xC3\x89", "\xCE\xA3"}) V.add(0, w);
    for (const char* w : {"ing", "s", "a", "e", "x", "b", "i", JA, JK, JG, JA JK, JK JG JA, DOT, DOT "stanbul",
                          "stanbul",
                          "\xC3\xA9", "\xCF\x83", "\xCF\x82", "the"})
      V.add(1, w);
    V.finish(fold, 100);
    run(V, names[fold - 1], ndocs, 7 + (uint64_t)fold);
    V.finish(fold, 3);
    run(V, "3 characters", ndocs / 4, 11 + (uint64_t)fold);
  }
  std::printf("%d failures\n", g_fail);
  return g_fail ? 1 : 0;
}
