// Standalone self-test of the split-regex BPE token counter (csrc/common/bpe_split.h), built with
// AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_bpe_split_sanitizers.py:
//
//   * a small merge list in the open-addressed pair table, its vocabulary in the whole-piece table
//     (wp_fill_slots), two added tokens behind the first-byte mask; patterns A and B, ignore_merges
//     on and off
//   * adversarial documents in exactly sized heap buffers (a lookahead past the end is a report):
//     contractions in both cases and with U+017F, number runs, punctuation-led words, newlines in
//     whitespace runs, 2-4-byte code points, pre-tokens around 64 and 2048 bytes, added-token
//     text, truncated and stray UTF-8
//   * bpe_count_doc<BpeSplit> against a plain std::string implementation: the pattern's
//     alternatives tried in order with their backtracking over the decoded code points, then
//     lowest-rank-first merges over strings
//   * and against the sum of bpe_count_range<true, BpeSplit> over chunks of 1, 2, 3, 5, 16, 17 and
//     64 bytes (the kernels' lane split)
//
// Exits non-zero on any mismatch; sanitizer reports abort the run.
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "tok_selftest.h"

using namespace tb;

static int g_fail = 0;

struct Tok {
  BpeSelfTables tab;
  std::map<std::pair<std::string, std::string>, int> rank;  // the reference's view of the merges
  std::map<std::string, uint32_t> ids;
  std::set<std::string> vocab;
  DevBpe T{};

  Tok(int kind, bool ignore_merges, const std::vector<std::pair<std::string, std::string>>& merges) {
    for (int i = 0; i < 256; ++i) {
      tab.byte_id.push_back((uint32_t)i);
      ids[std::string(1, (char)i)] = (uint32_t)i;
      vocab.insert(std::string(1, (char)i));
    }
    std::vector<uint32_t> ma, mb, mid;
    for (size_t i = 0; i < merges.size(); ++i) {
      const std::string ab = merges[i].first + merges[i].second;
      const uint32_t next_id = (uint32_t)ids.size();
      if (!ids.count(ab)) ids[ab] = next_id;
      rank[merges[i]] = (int)i;
      vocab.insert(ab);
      ma.push_back(ids[merges[i].first]);
      mb.push_back(ids[merges[i].second]);
      mid.push_back(ids[ab]);
    }
    tab.set_merges(ma, mb, mid);
    vocab.insert("abc");  // an entry no merge order reaches ("b c" goes first)
    vocab.insert(std::string(70, '-'));  // and one over the lanes' 64-byte arrays
    tab.set_vocabulary(vocab);
    tab.added = "<|bot|><eot>";
    tab.aoff = {0, 7, 12};
    tab.spec.post_add = 1;
    tab.spec.kind = kind;
    tab.spec.ignore_merges = ignore_merges;
    T = tab.params();
  }
};

struct Cp {
  int32_t c;
  int k;
  int64_t at;
};

// the pattern's alternatives in order, with their backtracking, over the decoded code points:
// the index after the match that starts at i
static size_t ref_match(const std::vector<Cp>& d, size_t i, int kind) {
  const size_t m = d.size();
  auto is = [&](size_t j, int k) { return j < m && d[j].k == k; };
  auto nl = [&](size_t j) { return j < m && (d[j].c == '\r' || d[j].c == '\n'); };
  auto low = [&](size_t j) -> int32_t {
    if (j >= m) return -1;
    if (d[j].c == 0x17F) return 's';
    return (d[j].c >= 'A' && d[j].c <= 'Z') ? d[j].c + 32 : d[j].c;
  };
  // (?i:'s|'t|'re|'ve|'m|'ll|'d)
  if (d[i].c == '\'') {
    for (const char* w : {"s", "t", "re", "ve", "m", "ll", "d"}) {
      const size_t L = std::strlen(w);
      bool ok = true;
      for (size_t j = 0; j < L; ++j) ok = ok && low(i + 1 + j) == w[j];
      if (ok) return i + 1 + L;
    }
  }
  // [^\r\n\p{L}\p{N}]?\p{L}+
  for (int opt = 1; opt >= 0; --opt) {
    size_t j = i;
    if (opt) {
      if (nl(j) || is(j, BPE_L) || is(j, BPE_N)) continue;
      ++j;
    }
    if (!is(j, BPE_L)) continue;
    while (is(j, BPE_L)) ++j;
    return j;
  }
  // \p{N}{1,3} / \p{N}
  if (is(i, BPE_N)) {
    size_t j = i + 1;
    while (j < i + (kind == kBpeSplitA ? 3 : 1) && is(j, BPE_N)) ++j;
    return j;
  }
  //  ?[^\s\p{L}\p{N}]+[\r\n]*
  for (int opt = 1; opt >= 0; --opt) {
    size_t j = i;
    if (opt) {
      if (d[j].c != ' ') continue;
      ++j;
    }
    if (!is(j, BPE_O)) continue;
    while (is(j, BPE_O)) ++j;
    while (nl(j)) ++j;
    return j;
  }
  size_t k = i;  // the greedy \s* / \s+
  while (is(k, BPE_W)) ++k;
  // \s*[\r\n]+
  for (size_t p = k + 1; p-- > i;) {
    size_t q = p;
    while (nl(q)) ++q;
    if (q > p) return q;
  }
  // \s+(?!\S)
  for (size_t p = k; p > i; --p)
    if (p == m || d[p].k == BPE_W) return p;
  // \s+
  return k > i ? k : i;
}

static int64_t ref_merge(const Tok& V, const std::string& w) {
  if (V.T.ignore_merges && V.vocab.count(w)) return 1;
  std::vector<std::string> s;
  for (char ch : w) s.emplace_back(1, ch);
  for (;;) {
    int best = 1 << 30;
    size_t bi = 0;
    for (size_t i = 0; i + 1 < s.size(); ++i) {
      const auto it = V.rank.find({s[i], s[i + 1]});
      if (it != V.rank.end() && it->second < best) { best = it->second; bi = i; }
    }
    if (best == 1 << 30) break;
    s[bi] += s[bi + 1];
    s.erase(s.begin() + (long)bi + 1);
  }
  return (int64_t)s.size();
}

static int32_t reference(const Tok& V, const uint8_t* b, int64_t n) {
  const std::string doc(reinterpret_cast<const char*>(b), (size_t)n);
  if (doc.find("<|bot|>") != std::string::npos || doc.find("<eot>") != std::string::npos) return kBpeHost;
  std::vector<Cp> d;
  for (int64_t i = 0; i < n;) {
    int l;
    const int32_t c = bpe_decode(b, i, n, &l);
    if (c < 0) return kBpeHost;
    d.push_back({c, bpe_cls(V.T, (uint32_t)c), i});
    i += l;
  }
  int64_t total = V.T.post_add;
  for (size_t i = 0; i < d.size();) {
    const size_t e = ref_match(d, i, V.T.kind);
    if (e <= i) return kBpeHost;
    const int64_t a = d[i].at, z = e < d.size() ? d[e].at : n;
    if (z - a > kBpeMaxLong) return kBpeHost;
    total += ref_merge(V, doc.substr((size_t)a, (size_t)(z - a)));
    i = e;
  }
  return (int32_t)total;
}

static std::string random_doc(std::mt19937_64& rng) {
  static const char* parts[] = {"a", "b", "c", "abc", "ab", "the", "'", "s", "S", "t", "re", "RE", "vE", "ll", "LL", "m", "d",
                                "\xC5\xBF", "\xE2\x84\xAA", " ", " ", "  ", "\n", "\r", "\r\n", "\t", "\xC2\xA0",
                                "\xE3\x80\x80", "\xC2\x85", "1", "42", "1234567", "\xC2\xB2", "\xD9\xA3", "!", "?", "...",
                                "-", "_", "\xCC\x81", "\xC3\xA9", "\xE6\x97\xA5", "\xF0\x9F\x98\x80", "\xE2\x92\xB6",
                                "\xCD\x85", "<|bo", "t|>", "<eo", "--------------------------------"};
  static const char* broken[] = {"\xFF", "\xC3", "\x80", "\xE2\x82", "\xF0\x9F\x98", "\xED\xA0\x80", "\xC0\xAF", "<eot>"};
  std::string s;
  const int n = (int)(rng() % 60);
  for (int i = 0; i < n; ++i) {
    s += parts[rng() % (sizeof(parts) / sizeof(*parts))];
    if (rng() % 97 == 0) s += broken[rng() % (sizeof(broken) / sizeof(*broken))];
  }
  return s;
}

static void run(const Tok& V, const char* name, int ndocs, uint64_t seed) {
  std::mt19937_64 rng(seed);
  std::vector<std::string> docs = {"", "'", "'s", "x'", "x'l", "x'L", "x'\xC5", "12", "1234", " ", " \n", "\n ", "! ",
                                   " !", "abc", " abc", std::string(70, '-'), std::string(71, '-'),
                                   "<|bot|>", "ab<eot>cd", std::string(2048, 'a'), std::string(2049, 'b'),
                                   std::string(3000, ' ') + "x", "1234567,.;: 89!? 1234567,.;: 89!? 1234567,.;: 89!?"};
  for (int i = 0; i < 140; ++i) docs.push_back(std::string((size_t)i, 'a') + "\xC3\xA9" + "'LL\n \n1234 !x");
  for (int i = 0; i < ndocs; ++i) docs.push_back(random_doc(rng));
  std::vector<uint32_t> lc(kBpeMaxLong);
  std::vector<uint64_t> lv(kBpeMaxLong);
  std::vector<int32_t> lnx(kBpeMaxLong), lpv(kBpeMaxLong);
  uint32_t cbuf[kBpeMaxWord], rbuf[kBpeMaxWord];
  int host = 0;
  for (const std::string& d : docs) {
    const int64_t n = (int64_t)d.size();
    std::unique_ptr<uint8_t[]> buf(new uint8_t[d.size()]);  // no slack: reads past n are reports
    std::memcpy(buf.get(), d.data(), d.size());
    const uint8_t* b = buf.get();
    auto on_long = [&](int64_t s, int64_t e) -> int64_t {
      if (e - s > kBpeMaxLong) return -1;
      return bpe_word_long(V.T, b + s, (int)(e - s), lc.data(), lv.data(), lnx.data(), lpv.data());
    };
    const int32_t want = reference(V, b, n);
    const int32_t got = bpe_count_doc<BpeSplit>(V.T, b, n, BpeArr{cbuf, 1}, BpeArr{rbuf, 1}, on_long);
    host += got == kBpeHost;
    if (got != want) {
      std::fprintf(stderr, "FAIL %s: doc of %lld bytes: %d, reference %d\n", name, (long long)n, got, want);
      ++g_fail;
    }
    for (int64_t chunk : {1, 2, 3, 5, 16, 17, 64}) {
      if (n > 4096 && chunk < 16) continue;  // (quadratic without a sync point)
      int64_t tot = V.T.post_add;
      bool bad = BpeSplit::has_added(V.T, b, n, 0, n);
      for (int64_t s0 = 0; s0 < n && !bad; s0 += chunk) {
        const int64_t x = bpe_count_range<true, BpeSplit>(V.T, b, n, s0, s0 + chunk < n ? s0 + chunk : n,
                                                          BpeArr{cbuf, 1}, BpeArr{rbuf, 1}, on_long);
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
  const std::vector<std::pair<std::string, std::string>> merges = {
      {"b", "c"}, {"a", "b"}, {"ab", "c"}, {"t", "h"}, {"th", "e"}, {" ", "a"}, {"-", "-"}, {"--", "--"}, {"'", "s"},
      {"1", "2"}, {"12", "3"}, {"\xC3", "\xA9"}, {" ", " "}, {"a", "a"}, {"aa", "aa"}, {"\r", "\n"}, {"!", "\n"}};
  int v = 0;
  for (int kind : {(int)kBpeSplitA, (int)kBpeSplitB})
    for (int im = 0; im < 2; ++im) {
      const Tok V(kind, im != 0, merges);
      char name[64];
      std::snprintf(name, sizeof name, "pattern %c, ignore_merges %d", kind == kBpeSplitA ? 'A' : 'B', im);
      run(V, name, ndocs, 7 + (uint64_t)v++);
    }
  std::printf("%d failures\n", g_fail);
  return g_fail ? 1 : 0;
}
