// Standalone self-test of the WordPiece token counter (csrc/common/wordpiece.h), built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_wordpiece_sanitizers.py:
//
//   * a small vocabulary in the open-addressed table (wp_fill_slots), cased and lowercase flags
//   * adversarial documents in exactly sized heap buffers (an over-read is a report): words of
//     the vocabulary, dropped / space / isolated code points, 2-4-byte code points, long words,
//     added-token text, truncated and stray UTF-8
//   * wp_count_doc against a plain std::string implementation of the same rules, and against
//     the sum of wp_count_range over chunks of 1, 7, 16 and 64 bytes (the kernel's lane split)
//
// Exits non-zero on any mismatch; sanitizer reports abort the run.
#include <cstdio>
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

  void finish(uint32_t flags, uint32_t self_bit, int max_chars) {
    tab.set_pieces(off, cont);
    tab.added = "[CLS][MASK]";
    tab.aoff = {0, 5, 11};
    tab.spec.flags = flags;
    tab.spec.self_bit = self_bit;
    tab.spec.max_chars = max_chars;
    tab.spec.post_add = 2;
    T = tab.params();
  }
};

// the same rules over std::string: words first, then greedy longest-first matching in a set
static int32_t reference(const Vocab& V, const uint8_t* b, int64_t n) {
  const std::string doc(reinterpret_cast<const char*>(b), (size_t)n);
  if (doc.find("[CLS]") != std::string::npos || doc.find("[MASK]") != std::string::npos) return kBpeHost;
  std::vector<std::vector<std::string>> words;  // each a list of characters
  bool open = false;
  for (int64_t i = 0; i < n;) {
    int l;
    const int k = wp_cp(V.T, b, i, n, &l);
    if (k < 0) return kBpeHost;
    std::string ch(doc, (size_t)i, (size_t)l);
    if (l == 1) ch[0] = (char)wp_byte(V.T, (uint8_t)ch[0]);
    if (k == WP_KEEP) {
      if (!open) words.emplace_back();
      open = true;
      words.back().push_back(ch);
    } else if (k != WP_DROP) {
      open = false;
      if (k == WP_ISO) words.push_back({ch});
    }
    i += l;
  }
  int64_t total = V.T.post_add;
  for (const auto& w : words) {
    if ((int64_t)w.size() > V.T.max_chars) { ++total; continue; }
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

static std::string random_doc(std::mt19937_64& rng) {
  static const char* parts[] = {"the", "The", "ing", "s", "un", "known", "word", "xyzzy", " ", " ", "  ", "\n", "\t",
                                "\xC2\xAD", "\xE2\x80\x8B", "\xC2\x85", "\x1c", "\xC2\xA0", "\xE3\x80\x80", "_", "$",
                                "\xE2\x80\x94", "!", "...", "\xE4\xBD\xA0", "\xF0\xA0\x80\x80", "\xC3\xA9", "\xCC\x81",
                                "\xCD\xB8", "\xF0\x9F\x98\x80", "\xC3\x9F", "1", "aaaaaaaaaaaaaaaaaaaaaaaa", "[CL", "S]",
                                "\xEF\xBF\xBD"};
  static const char* broken[] = {"\xFF", "\xC3", "\x80", "\xE2\x82", "\xF0\x9F\x98", "\xED\xA0\x80", "\xC0\xAF", "[CLS]"};
  std::string s;
  const int n = (int)(rng() % 60);
  for (int i = 0; i < n; ++i) {
    s += parts[rng() % (sizeof(parts) / sizeof(*parts))];
    if (rng() % 97 == 0) s += broken[rng() % (sizeof(broken) / sizeof(*broken))];
  }
  return s;
}

static void run(const Vocab& V, const char* name, int ndocs, uint64_t seed) {
  std::mt19937_64 rng(seed);
  std::vector<std::string> docs = {"", " ", "the", std::string(5000, 'x'), std::string(300, '!'),
                                   "unknownword theing", "the\xCD\xB8", "\xC3\xA9", "[CLS] hi"};
  for (int i = 0; i < 150; ++i) docs.push_back(std::string((size_t)i, 'a') + "\xC3\xA9" + "the");
  for (int i = 0; i < ndocs; ++i) docs.push_back(random_doc(rng));
  int host = 0;
  for (const std::string& d : docs) {
    const int64_t n = (int64_t)d.size();
    std::unique_ptr<uint8_t[]> buf(new uint8_t[d.size()]);  // no slack: reads past n are reports
    std::memcpy(buf.get(), d.data(), d.size());
    const uint8_t* b = buf.get();
    const int32_t want = reference(V, b, n), got = wp_count_doc(V.T, b, n);
    host += got == kBpeHost;
    if (got != want) {
      std::fprintf(stderr, "FAIL %s: doc of %lld bytes: %d, reference %d\n", name, (long long)n, got, want);
      ++g_fail;
    }
    for (int64_t chunk : {1, 7, 16, 64}) {
      int64_t tot = V.T.post_add;
      bool bad = wp_has_added(V.T, b, n, 0, n);
      for (int64_t s0 = 0; s0 < n && !bad; s0 += chunk) {
        const int64_t x = wp_count_range(V.T, b, n, s0, s0 + chunk < n ? s0 + chunk : n);
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
  for (int lower = 0; lower < 2; ++lower) {
    Vocab V;
    for (const char* w : {"the", "un", "known", "word", "a", "aa", "aaaa", "x", "1", "!", ".", "_", "$", "s",
                          "\xE4\xBD\xA0", "\xC3\xA9", "\xC3\x9F", "th", "t", "\xE2\x80\x94"})
      V.add(0, w);
    if (!lower) V.add(0, "The");
    for (const char* w : {"ing", "s", "known", "word", "a", "aa", "\xC3\xA9", "e", "h"}) V.add(1, w);
    V.finish(kWpChinese | (lower ? kWpLower : 0), lower ? 1u << 6 : 0, 100);
    run(V, lower ? "uncased" : "cased", ndocs, 7 + lower);
    V.finish(kWpChinese | (lower ? kWpLower : 0), lower ? 1u << 6 : 0, 3);
    run(V, lower ? "uncased, 3 characters" : "cased, 3 characters", ndocs / 4, 11 + lower);
  }
  std::printf("%d failures\n", g_fail);
  return g_fail ? 1 : 0;
}
