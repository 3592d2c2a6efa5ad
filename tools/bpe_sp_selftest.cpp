// Standalone self-test of the SentencePiece-style BPE token counter (csrc/common/bpe_sp.h), built
// with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_bpe_sp_sanitizers.py:
//
//   * a small vocabulary (the 256 <0xNN> tokens, single characters of one to three bytes, U+2581)
//     and merge list in the open-addressed pair table, the single characters in the direct ASCII
//     array and the code point table, two added tokens behind the first-byte mask; the prepend
//     rules none / always / unless-space, a chunk per word and a chunk at every space
//   * adversarial documents in exactly sized heap buffers (a read past the end is a report): space
//     runs, literal U+2581 next to spaces, characters of 2 to 4 bytes in and out of the vocabulary,
//     chunks around 64 and 2048 bytes at offset 0 and after a word, added-token text, truncated and
//     stray UTF-8
//   * bpe_count_doc<BpeSp> against a plain std::string implementation of what the library does: the
//     text normalised (U+0020 -> U+2581, the prepend), cut at every U+2581 when the layout splits
//     and left whole when it does not, lowest-rank-first merges over strings; the chunk rule, also
//     over std::string, only decides which documents go to the host (a chunk over 2048 bytes). So
//     without the split the whole-document merge checks that chunks merge independently
//   * and against the sum of bpe_count_range<true, BpeSp> over chunks of 1, 2, 3, 5, 16, 17 and 64
//     bytes (the kernels' lane split)
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

static std::string byte_token(uint8_t x) {
  char buf[8];
  std::snprintf(buf, sizeof buf, "<0x%02X>", x);
  return buf;
}

struct Tok {
  BpeSelfTables tab;
  std::map<std::pair<std::string, std::string>, int> rank;  // the reference's view of the merges
  std::map<std::string, uint32_t> ids;
  DevBpe T{};

  Tok(int flags, const std::vector<std::pair<std::string, std::string>>& merges) {
    for (int i = 0; i < 256; ++i) {
      tab.byte_id.push_back((uint32_t)i);
      ids[byte_token((uint8_t)i)] = (uint32_t)i;
    }
    tab.sp_ascii.assign(128, kBpeSpNone);
    std::vector<uint32_t> cps, cids;
    // the single characters: é and あ are entries, ü, 日 and the emoji are not; '<' is, 'z' is not
    for (const char* s : {"a", "b", "c", "e", "h", "q", "t", "s", "<", ">", "/", "1", "2", "\n", ".", "\xC3\xA9",
                          "\xE3\x81\x82", "\xE2\x96\x81"}) {
      const uint32_t id = (uint32_t)ids.size();
      ids[s] = id;
      int l;
      const int32_t c = bpe_decode(reinterpret_cast<const uint8_t*>(s), 0, (int64_t)std::strlen(s), &l);
      if (c < 128) {
        tab.sp_ascii[(size_t)c] = id;
      } else if (c == (int32_t)kBpeSpSpace) {
        tab.spec.sp_id = id;
      } else {
        cps.push_back((uint32_t)c);
        cids.push_back(id);
      }
    }
    const size_t ccap = tok_table_cap(cps.size());
    tab.sp_cp.resize(ccap);
    bpe_sp_fill(cps.data(), cids.data(), cps.size(), tab.sp_cp.data(), (uint32_t)(ccap - 1));
    tab.spec.sp_mask = (uint32_t)(ccap - 1);
    std::vector<uint32_t> ma, mb, mid;
    for (size_t i = 0; i < merges.size(); ++i) {
      const std::string ab = merges[i].first + merges[i].second;
      const uint32_t next_id = (uint32_t)ids.size();
      if (!ids.count(ab)) ids[ab] = next_id;
      rank[merges[i]] = (int)i;
      ma.push_back(ids.at(merges[i].first));
      mb.push_back(ids.at(merges[i].second));
      mid.push_back(ids[ab]);
    }
    tab.set_merges(ma, mb, mid);
    tab.spec.sp_flags = flags;
    tab.added = "<s></s>";
    tab.aoff = {0, 3, 7};
    tab.spec.post_add = 1;
    tab.spec.kind = kBpeSp;
    T = tab.params();
  }
};

// the code points of s as strings, "" on invalid UTF-8
static bool chars_of(const std::string& s, std::vector<std::string>* out) {
  const uint8_t* b = reinterpret_cast<const uint8_t*>(s.data());
  const int64_t n = (int64_t)s.size();
  for (int64_t i = 0; i < n;) {
    int l;
    if (bpe_decode(b, i, n, &l) < 0) return false;
    out->push_back(s.substr((size_t)i, (size_t)l));
    i += l;
  }
  return true;
}

// the word's tokens: a character that is an entry is a symbol, any other one <0xNN> per byte; then
// the lowest-rank pair, leftmost on ties, until none is left
static int64_t ref_merge(const Tok& V, const std::vector<std::string>& chars) {
  std::vector<std::string> s;
  for (const std::string& ch : chars) {
    if (V.ids.count(ch)) {
      s.push_back(ch);
    } else {
      for (char x : ch) s.push_back(byte_token((uint8_t)x));
    }
  }
  const int none = 1 << 30;
  auto rank_at = [&](size_t i) {  // of the pair (s[i], s[i + 1])
    if (i + 1 >= s.size()) return none;
    const auto it = V.rank.find({s[i], s[i + 1]});
    return it == V.rank.end() ? none : it->second;
  };
  std::vector<int> r(s.size());
  for (size_t i = 0; i < s.size(); ++i) r[i] = rank_at(i);
  for (;;) {
    int best = none;
    size_t bi = 0;
    for (size_t i = 0; i + 1 < s.size(); ++i)
      if (r[i] < best) { best = r[i]; bi = i; }
    if (best == none) break;
    s[bi] += s[bi + 1];
    s.erase(s.begin() + (long)bi + 1);
    r.erase(r.begin() + (long)bi + 1);
    r[bi] = rank_at(bi);
    if (bi > 0) r[bi - 1] = rank_at(bi - 1);
  }
  return (int64_t)s.size();
}

static int32_t reference(const Tok& V, const std::string& doc) {
  if (doc.find("<s>") != std::string::npos || doc.find("</s>") != std::string::npos) return kBpeHost;
  std::vector<std::string> raw;
  if (!chars_of(doc, &raw)) return kBpeHost;
  const bool split = (V.T.sp_flags & kBpeSpSplit) != 0;
  const int mode = V.T.sp_flags & kBpeSpPrependMask;
  // the normaliser / Metaspace: U+0020 -> U+2581, then the prepend
  std::vector<std::string> norm;
  for (const std::string& ch : raw) norm.push_back(ch == " " ? kSp : ch);
  const bool lead = !norm.empty() && (mode == kBpeSpPrependAlways || (mode == kBpeSpPrependUnlessSpace && norm[0] != kSp));
  // the chunk rule decides only what the counter may hand to the host: bytes of the raw text, plus
  // one for the prepended symbol in the chunk at offset 0
  size_t bytes = lead ? 1 : 0;
  for (size_t i = 0; i < raw.size(); ++i) {
    if (i > 0 && norm[i] == kSp && (split || norm[i - 1] != kSp)) bytes = 0;  // a chunk starts here
    bytes += raw[i].size();
    if (bytes > (size_t)kBpeMaxLong) return kBpeHost;
  }
  if (lead) norm.insert(norm.begin(), kSp);
  int64_t total = V.T.post_add;
  if (!split) return (int32_t)(total + ref_merge(V, norm));  // one word, as the library merges it
  std::vector<std::string> piece;  // MergedWithNext: a piece starts at every U+2581
  for (const std::string& ch : norm) {
    if (ch == kSp && !piece.empty()) {
      total += ref_merge(V, piece);
      piece.clear();
    }
    piece.push_back(ch);
  }
  if (!piece.empty()) total += ref_merge(V, piece);
  return (int32_t)total;
}

static std::string random_doc(std::mt19937_64& rng) {
  static const char* parts[] = {" ", " ", " ", "  ", "   ", "\xE2\x96\x81", "\xE2\x96\x81\xE2\x96\x81", " \xE2\x96\x81",
                                "\xE2\x96\x81 ", "a", "b", "ab", "abc", "the", "t", "h", "e", "q", "qq", "qqqq", "z",
                                "\n", "\t", ".", "1", "12", "\xC3\xA9", "\xC3\xBC", "\xE3\x81\x82", "\xE6\x97\xA5",
                                "\xF0\x9F\xA6\x80", "\xCC\x81", "<", "s>", "</", "s", ">",
                                "qqqqqqqqqqqqqqqqqqqqqqqqqqqqqqqq", "                                "};
  static const char* broken[] = {"\xFF", "\xC3", "\x80", "\xE2\x96", "\xF0\x9F\xA6", "\xED\xA0\x80", "\xC0\xAF", "<s>"};
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
  std::vector<std::string> docs = {"", " ", kSp, "a", " a", kSp + "a", "  a", " " + kSp + "a", "a ", "a" + kSp, "ab abc the",
                                   "\xC3\xA9", "\xC3\xBC", "\xF0\x9F\xA6\x80", "a\xE3\x81\x82\xF0\x9F\xA6\x80", "<s>", "ab</s>cd",
                                   "<s", "\xE2\x96", "a \xE2", "word \xE2\x96 word"};
  for (int n : {62, 63, 64, 65, 2046, 2047, 2048, 2049}) {
    docs.push_back(std::string((size_t)n, 'q'));
    docs.push_back(std::string((size_t)n, 'q') + " ab");
    docs.push_back("ab " + std::string((size_t)n - 1, 'q'));
    docs.push_back(" " + std::string((size_t)n - 1, 'q'));
    docs.push_back(kSp + std::string((size_t)n - 3, 'q'));
    docs.push_back("ab" + std::string((size_t)n - 1, ' ') + "q");
    docs.push_back(std::string((size_t)n, ' '));
    docs.push_back(std::string((size_t)n - 2, 'a') + "\xC3\xBC");  // byte fallback at the limit
    std::string cjk;
    while (cjk.size() + 3 <= (size_t)n) cjk += "\xE3\x81\x82";      // fewer symbols than bytes
    docs.push_back(cjk + std::string((size_t)n - cjk.size(), 'b'));
  }
  for (int i = 0; i < 140; ++i)  // every rule across every chunk edge
    docs.push_back(std::string((size_t)i, 'a') + " " + kSp + "\xC3\xBC  the\xF0\x9F\xA6\x80" + kSp + kSp + " ab");
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
      const int lead = BpeSp::lead(V.T, b, n, s);
      if (e - s + lead > kBpeMaxLong) return -1;
      return bpe_word_long<BpeSp>(V.T, b + s, (int)(e - s), lc.data(), lv.data(), lnx.data(), lpv.data(), lead);
    };
    const int32_t want = reference(V, d);
    const int32_t got = bpe_count_doc<BpeSp>(V.T, b, n, BpeArr{cbuf, 1}, BpeArr{rbuf, 1}, on_long);
    host += got == kBpeHost;
    if (got != want) {
      std::fprintf(stderr, "FAIL %s: doc of %lld bytes: %d, reference %d\n", name, (long long)n, got, want);
      ++g_fail;
    }
    for (int64_t chunk : {1, 2, 3, 5, 16, 17, 64}) {
      if (n > 4096 && chunk < 16) continue;
      int64_t tot = V.T.post_add;
      bool bad = BpeSp::has_added(V.T, b, n, 0, n);
      for (int64_t s0 = 0; s0 < n && !bad; s0 += chunk) {
        const int64_t x = bpe_count_range<true, BpeSp>(V.T, b, n, s0, s0 + chunk < n ? s0 + chunk : n,
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
  const std::string ue1 = byte_token(0xC3), ue2 = byte_token(0xBC);
  // no merge joins a piece that ends in another character than U+2581 to one that starts with it
  std::vector<std::pair<std::string, std::string>> merges = {
      {"b", "c"}, {"a", "b"}, {"ab", "c"}, {"t", "h"}, {"th", "e"}, {kSp, "a"}, {kSp + "a", "b"}, {kSp, "t"},
      {kSp, kSp}, {kSp + kSp, kSp + kSp}, {"q", "q"}, {"qq", "qq"}, {"qqqq", "qqqq"}, {ue1, ue2}, {"\xC3\xA9", "a"},
      {"\xE3\x81\x82", "\xE3\x81\x82"}, {kSp + kSp, "a"}, {"1", "2"}, {kSp, "\xC3\xA9"}, {"<", "s"}, {"s", ">"}};
  int v = 0;
  for (int split = 0; split < 2; ++split) {
    // where every U+2581 starts a piece, a merge across the space can never apply
    if (split) merges.push_back({"a", kSp});
    for (int mode : {0, (int)kBpeSpPrependAlways, (int)kBpeSpPrependUnlessSpace}) {
      if (split && mode == kBpeSpPrependAlways) continue;  // (no layout: Metaspace looks at the first character)
      const Tok V(mode | (split ? (int)kBpeSpSplit : 0), merges);
      char name[64];
      std::snprintf(name, sizeof name, "prepend %d, split %d", mode, split);
      run(V, name, ndocs, 11 + (uint64_t)v++);
    }
  }
  std::printf("%d failures\n", g_fail);
  return g_fail ? 1 : 0;
}
