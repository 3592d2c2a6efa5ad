// Stand-alone self-test of C4 pass A's byte scan and of the stop-word fast path (csrc/common/c4_pass_a.h
// and stage_analyze.h on the host), built with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_c4_scan_selftest.py:
//
//   * c4_byte_scan's bits against ci_contains per phrase over the whole text and the per-byte
//     definitions of the curly-bracket and citation tests, and c4_phrases_at / c4_lorem_at at
//     every byte position against ci_starts_with per phrase
//   * is_stop_word's fast path (ASCII words of up to 7 bytes) against a std::set, with the words at
//     the first and last bytes of exactly sized texts
//
// Every text lies at the end of a heap buffer that ends with the text, at each of the four dword
// alignments, so a read past the text is a sanitizer report. With an argument, the texts are
// written to that file (u32 length + bytes each) for the Python tests, which push them through the
// engines.
#include <cstdio>
#include <cstring>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "../csrc/common/c4_pass_a.h"
#include "../csrc/common/stage_analyze.h"

using namespace tb;

static int g_fail = 0;
static long g_checks = 0;
#define CHECK(c, ...)                                          \
  do {                                                         \
    ++g_checks;                                                \
    if (!(c)) {                                                \
      if (g_fail < 50) {                                       \
        std::fprintf(stderr, "FAIL %s:%d ", __FILE__, __LINE__); \
        std::fprintf(stderr, __VA_ARGS__);                     \
        std::fprintf(stderr, "\n");                            \
      }                                                        \
      ++g_fail;                                                \
    }                                                          \
  } while (0)

static const char* const kPhrases[8] = {"javascript",   "terms of use",   "privacy policy", "cookie policy",
                                        "uses cookies", "use of cookies", "use cookies",    "lorem ipsum"};
static const char kKelvin[] = "\xE2\x84\xAA";

static std::string printable(const std::string& s) {
  std::string o;
  for (size_t i = 0; i < s.size() && i < 80; ++i) {
    char buf[8];
    const unsigned char c = (unsigned char)s[i];
    if (c >= 0x20 && c < 0x7F) o += (char)c;
    else { std::snprintf(buf, sizeof buf, "\\x%02X", c); o += buf; }
  }
  return o;
}

// ---- the texts -----------------------------------------------------------------------------
static std::string upper(std::string s) {
  for (auto& c : s) if (c >= 'a' && c <= 'z') c = (char)(c - 32);
  return s;
}
static std::string mixed(std::string s) {
  for (size_t i = 0; i < s.size(); i += 2) if (s[i] >= 'a' && s[i] <= 'z') s[i] = (char)(s[i] - 32);
  return s;
}
// filler without any phrase; `tease`: full of the phrases' 3-byte prefixes
static std::string filler(size_t n, bool tease) {
  static const char plain[] = "ab de. ";
  static const char teasing[] = "ter use coo pri jav lor user term cook uses usec ";
  const char* src = tease ? teasing : plain;
  const size_t m = std::strlen(src);
  std::string s;
  for (size_t i = 0; i < n; ++i) s += src[i % m];
  return s;
}

static std::vector<std::string> make_texts() {
  std::vector<std::string> t;
  std::vector<std::string> variants;  // phrases, their case variants, Kelvin forms and near misses
  for (const char* p : kPhrases) {
    const std::string s = p;
    variants.push_back(s);
    variants.push_back(upper(s));
    variants.push_back(mixed(s));
    for (size_t i = 0; i < s.size(); ++i)
      if (s[i] == 'k') {
        variants.push_back(s.substr(0, i) + kKelvin + s.substr(i + 1));
        variants.push_back(upper(s.substr(0, i)) + kKelvin + s.substr(i + 1));
        variants.push_back(s.substr(0, i) + "\xE2\x84\xAB" + s.substr(i + 1));  // not the Kelvin sign
        variants.push_back(s.substr(0, i) + "\xE2" + s.substr(i + 1));
      }
    std::string miss = s;  // passes the long prefix, fails in the last byte
    miss.back() = (char)(miss.back() == 'd' ? 'e' : miss.back() + 1);
    variants.push_back(miss);
    miss = s;
    miss[5] = '_';
    variants.push_back(miss);
  }
  variants.push_back("terms of usd");
  variants.push_back("use cookiex");
  variants.push_back("lorem ipsun");
  variants.push_back("use of cookiez");
  variants.push_back("cook policy");
  variants.push_back("coo\xE2\x84\xAAie polic");

  for (const std::string& v : variants) {
    // at offset 0 and ending at n, after 0..3 bytes, alone and inside filler
    for (size_t pre = 0; pre < 4; ++pre) {
      t.push_back(filler(pre, false) + v);
      t.push_back(filler(pre, false) + v + filler(9 + pre, true));
      t.push_back(filler(29 + pre, true) + v);
    }
    // cut by the end of the text after each of its bytes
    for (size_t cut = 1; cut < v.size(); ++cut) {
      t.push_back(v.substr(0, cut));
      t.push_back(filler(13, true) + v.substr(0, cut));
    }
    // straddling a lane's 16-byte item
    for (size_t j = 1; j < v.size(); ++j) t.push_back(filler(32 - j, false) + v + filler(5, false));
  }
  // straddling the wave's 1024-byte iteration and the workgroup strides (256 and 512 lanes)
  for (size_t bound : {(size_t)1024, (size_t)4096, (size_t)8192})
    for (const char* p : kPhrases) {
      const std::string s = p;
      std::string k = s;
      const size_t kp = s.find('k');
      if (kp != std::string::npos) k = s.substr(0, kp) + kKelvin + s.substr(kp + 1);
      for (size_t j = 1; j < s.size(); ++j) {
        t.push_back(filler(bound - j, j & 1) + s + filler(3, false));
        if (kp != std::string::npos && (j % 3 == 0 || j == kp || j == kp + 1 || j == kp + 2))
          t.push_back(filler(bound - j, false) + k);
      }
    }
  // n = 0..5
  for (size_t n = 0; n <= 5; ++n) {
    for (const char* p : kPhrases) t.push_back(std::string(p).substr(0, n));
    t.push_back(std::string("{[1}]").substr(0, n));
    t.push_back(std::string("[\xC3\xA9 [").substr(0, n));
  }
  // '[' followed by a digit, by a byte >= 0x80, by something else, and as the last byte
  for (size_t pre = 0; pre < 20; ++pre) {
    t.push_back(filler(pre, false) + "[7] x");
    t.push_back(filler(pre, false) + "[\xC3\xA9] x");
    t.push_back(filler(pre, false) + "[a] x");
    t.push_back(filler(pre, false) + "[");
    t.push_back(filler(pre, false) + "[0");
  }
  // '{' and '}' at every position of a dword
  for (size_t pre = 0; pre < 20; ++pre)
    for (const char* c : {"{", "}"}) {
      t.push_back(filler(pre, false) + c);
      t.push_back(filler(pre, false) + c + filler(7, true));
    }
  return t;
}

// ---- references ----------------------------------------------------------------------------
static uint32_t scan_reference(const DevC4& c4, const uint8_t* b, uint32_t n) {
  uint32_t bits = 0;
  if (c4.filter_lorem_ipsum && ci_contains(b, n, "lorem ipsum", 11)) bits |= C4S_LOREM;
  if (c4.filter_javascript && ci_contains(b, n, "javascript", 10)) bits |= C4F_JS;
  if (c4.filter_policy)
    for (int p = 1; p <= 6; ++p)
      if (ci_contains(b, n, kPhrases[p], (int)std::strlen(kPhrases[p]))) bits |= C4F_POLICY;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c0 = b[i], c1 = i + 1 < n ? b[i + 1] : 0u;
    if (c4.filter_curly_bracket && (c0 == '{' || c0 == '}')) bits |= C4S_CURLY;
    if (c0 == '[' && ((c1 >= '0' && c1 <= '9') || c1 >= 0x80)) bits |= C4S_CITE;
  }
  return bits;
}

static DevC4 c4_config(bool js, bool policy, bool lorem, bool curly) {
  DevC4 c{};
  c.split_paragraph = c.remove_citations = c.filter_no_terminal_punct = 1;
  c.filter_javascript = js;
  c.filter_policy = policy;
  c.filter_lorem_ipsum = lorem;
  c.filter_curly_bracket = curly;
  c.min_words_per_line = 3;
  c.max_word_length = 1000;
  c.min_num_sentences = 5;
  return c;
}

// The text at dword alignment `al`, in a buffer that ends with it.
struct Placed {
  std::unique_ptr<uint8_t[]> buf;
  uint8_t* b;
  Placed(const std::string& s, uint32_t al) {
    // operator new[] returns 16-byte aligned memory: the text starts `al` past a dword
    const size_t pad = 16 + al;
    buf.reset(new uint8_t[pad + s.size()]);
    std::memset(buf.get(), '{', pad);  // a read before the text would see a bracket and a phrase
    std::memcpy(buf.get() + 4, "javascript ", 11);
    b = buf.get() + pad;
    if (!s.empty()) std::memcpy(b, s.data(), s.size());
  }
};

static void check_scan(const std::string& s) {
  static const DevC4 cfgs[3] = {c4_config(true, true, true, true), c4_config(true, false, false, true),
                                c4_config(false, true, true, false)};
  const uint32_t n = (uint32_t)s.size();
  for (uint32_t al = 0; al < 4; ++al) {
    Placed pl(s, al);
    const uint8_t* b = pl.b;
    for (const DevC4& c4 : cfgs) {
      DocCtx<SeqPar> x;
      const uint32_t got = c4_byte_scan(x, c4, b, n), want = scan_reference(c4, b, n);
      CHECK(got == want, "scan bits %u want %u (align %u, n %u): %s", got, want, al, n, printable(s).c_str());
    }
    // every position: the phrase bits and lorem ipsum against the byte-wise prefix test
    DocCtx<SeqPar> x;
    uint32_t visited = 0;
    scan_bytes16(x, b, n, [&](uint32_t p, uint32_t c0, uint32_t c1, uint64_t lw) {
      ++visited;
      CHECK(c0 == b[p] && c1 == (p + 1 < n ? b[p + 1] : 0u), "bytes at %u (align %u): %s", p, al, printable(s).c_str());
      uint32_t want = 0;
      if (ci_starts_with(b + p, n - p, "javascript", 10)) want |= C4F_JS;
      for (int q = 1; q <= 6; ++q)
        if (ci_starts_with(b + p, n - p, kPhrases[q], (int)std::strlen(kPhrases[q]))) want |= C4F_POLICY;
      const uint32_t got = c4_phrase_prefix(lw) ? c4_phrases_at(cfgs[0], b, n, p, lw) : 0u;
      CHECK(got == want, "phrase bits %u want %u at %u (align %u): %s", got, want, p, al, printable(s).c_str());
      CHECK(c4_lorem_at(b, n, p, lw) == ci_starts_with(b + p, n - p, "lorem ipsum", 11), "lorem at %u (align %u): %s", p,
            al, printable(s).c_str());
    });
    CHECK(visited == n, "visited %u of %u positions", visited, n);
  }
}

// ---- stop words ----------------------------------------------------------------------------
static uint64_t byte_loop_key(const uint8_t* b, uint32_t b0, uint32_t nb) {
  uint64_t key = (uint64_t)nb << 56;
  for (uint32_t k = 0; k < nb; ++k) {
    uint32_t c = b[b0 + k];
    if (c >= 'A' && c <= 'Z') c += 32;
    key |= (uint64_t)c << (8 * k);
  }
  return key;
}

static void check_stop_words() {
  static const char* const kStops[] = {"a", "of", "the", "with", "their", "should", "because", "z", "zzzzzzz"};
  std::set<std::string> stops(std::begin(kStops), std::end(kStops));
  std::unique_ptr<DevStopSet> ss(new DevStopSet());
  std::memset(ss.get(), 0, sizeof(DevStopSet));
  ss->n = (int32_t)stops.size();
  ss->max_len = 7;
  ss->lite_nslots = 64;
  ss->all_ascii7 = 1;
  for (const std::string& w : stops) {
    const uint64_t key = byte_loop_key((const uint8_t*)w.data(), 0, (uint32_t)w.size());
    uint32_t slot = stop_fast_slot(key, 64);
    while (ss->fast_keys[slot]) slot = (slot + 1) & 63;
    ss->fast_keys[slot] = key;
  }
  std::vector<std::string> cands(std::begin(kStops), std::end(kStops));
  for (const char* w : {"b", "ab", "thy", "wits", "there", "shoulx", "becausf", "becauses", "thethethe", "of@", "[\\]^_`",
                        "@AZ[az{"})
    cands.push_back(w);
  const size_t base = cands.size();
  for (size_t i = 0; i < base; ++i) {
    cands.push_back(upper(cands[i]));
    cands.push_back(mixed(cands[i]));
    for (size_t k = 0; k <= cands[i].size() && cands[i].size() < 8; ++k)  // a two-byte code point at each position
      cands.push_back(cands[i].substr(0, k) + "\xC3\xA9" + cands[i].substr(k));
  }
  const UcdView ucd{};
  for (const std::string& w : cands) {
    uint32_t cps = 0;
    for (unsigned char c : w) cps += (c & 0xC0) != 0x80;
    std::string low = w;
    for (auto& c : low) if (c >= 'A' && c <= 'Z') c = (char)(c + 32);
    const bool want = cps == w.size() && stops.count(low) > 0;
    // the word at the first bytes, in the middle and at the last bytes of the text
    for (int where = 0; where < 4; ++where) {
      const std::string pre = where == 0 || where == 3 ? "" : filler(where == 1 ? 5 : 6, false);
      const std::string post = where == 1 || where == 3 ? "" : " xyz";
      const std::string text = pre + w + post;
      for (uint32_t al = 0; al < 4; ++al) {
        Placed pl(text, al);
        const uint32_t n = (uint32_t)text.size(), b0 = (uint32_t)pre.size(), nb = (uint32_t)w.size();
        Cps cv;
        cv.b = pl.b;
        cv.nb = n;
        const bool got = is_stop_word(ucd, *ss, cv, 100, 100 + cps, b0, b0 + nb);
        CHECK(got == want, "is_stop_word %d want %d (align %u, place %d): %s", (int)got, (int)want, al, where,
              printable(w).c_str());
      }
    }
  }
}

int main(int argc, char** argv) {
  const std::vector<std::string> texts = make_texts();
  if (argc > 1) {
    std::FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    for (const std::string& s : texts) {
      const uint32_t n = (uint32_t)s.size();
      std::fwrite(&n, 4, 1, f);
      if (n) std::fwrite(s.data(), 1, n, f);
    }
    std::fclose(f);
  }
  for (const std::string& s : texts) check_scan(s);
  check_stop_words();
  std::printf("c4 scan selftest: %zu texts, %ld checks, %d failures\n", texts.size(), g_checks, g_fail);
  return g_fail ? 1 : 0;
}
