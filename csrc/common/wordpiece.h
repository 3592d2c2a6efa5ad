// WordPiece (BERT) token counting (TokenCounter, reference src/pipeline/token/token_counter.rs:31-42:
// ``tokenizer.encode(text, true).get_tokens().len()``) for tokenizers made of BertNormalizer +
// BertPreTokenizer + a WordPiece model, plus the tokens the post-processor adds. Shared by the HIP
// kernel (csrc/hip/wordpiece.hip: one wave per kept document, a byte range per lane) and its host
// emulation (csrc/host/tok_module.cpp wp_count), which CPU tests pin to the `tokenizers` library.
//
// Words. Every code point has a class (wp_classes.inc, generated from the library): keep, drop
// (removed, so its neighbours join), space, isolate (punctuation and CJK ideographs: a word of its
// own). A word is a maximal run of keep code points with the drops between them taken out, or one
// isolate. So word starts are a local property of the text: a keep code point starts a word iff
// the nearest code point before it that is not a drop is a space or an isolate, or there is none.
// A lane counts the words that start in its byte range, wherever they end.
//
// Normalisation. Cased tokenizers need none beyond the classes. With lowercase / strip_accents
// ASCII is folded here; the identity counter (wp_*) then needs every other code point to carry the
// "normalises to itself" bit of its combination and counts a document with one that does not on
// the host (kBpeHost), as it does documents with invalid UTF-8 or the text of an added token (the
// library splits on those first). The folding counter (wpf_*, below) reads what the normalizer
// makes of such a code point from wp_fold.inc and counts those documents too.
//
// Pieces. The vocabulary is an open-addressed table keyed by a 64-bit hash of (continuation flag,
// piece bytes); the piece bytes themselves sit in a pool, and every slot whose key matches is
// compared byte for byte before it counts (two pieces with one key occupy two slots). The hash is
// polynomial, so the longest-first search at a position is cheap without storage: hash the longest
// candidate - whole code points up to min(word end, position + longest piece), exact because no
// longer piece exists - then take the last code point's bytes off again (multiply by the inverse
// of the base) after each miss. A position with no match makes the whole word one token, as does a
// word over max_input_chars_per_word characters.
#pragma once
#include <cstddef>

#include "bpe.h"

namespace tb {

enum WpCls : int { WP_KEEP = 0, WP_DROP = 1, WP_SPACE = 2, WP_ISO = 3 };
constexpr uint32_t kWpLower = 1;    // fold ASCII upper case
constexpr uint32_t kWpChinese = 2;  // handle_chinese_chars: CJK ideographs are isolated
constexpr uint64_t kWpEmpty = ~0ull;  // WpSlot::val of a free slot
constexpr uint64_t kWpBase = 0x9E3779B97F4A7C15ull;

constexpr uint64_t wp_inv64(uint64_t a) {  // a^-1 mod 2^64 (a odd), Newton's iteration
  uint64_t x = a;
  for (int i = 0; i < 6; ++i) x *= 2 - a * x;
  return x;
}
constexpr uint64_t kWpBaseInv = wp_inv64(kWpBase);
static_assert(kWpBase * kWpBaseInv == 1, "inverse of the hash base");

struct WpSlot {
  uint64_t key;  // wp_key of the piece
  uint64_t val;  // pool offset << 32 | continuation << 31 | bytes; kWpEmpty = free
};

struct DevWp {
  const WpSlot* slots;   // [mask + 1], at most half full
  const uint8_t* pool;   // piece bytes (continuation pieces without their prefix)
  const uint16_t* cls1;  // wp_classes.inc two-stage table, one byte per code point
  const uint8_t* cls2;
  const uint8_t* added;  // contents of the added tokens, concatenated
  const uint16_t* fold1;  // wp_fold.inc of the tokenizer's mode: stage 1, null = no folding beyond ASCII
  const uint16_t* fold2;  // stage 2: 0 identity, kWpFoldHost, kWpFoldHangul, else 1 + record offset
  const uint8_t* foldp;   // records: header (bytes | class << 4 | unclean class << 6), output bytes
  uint64_t asc0, asc1, asc2, asc3;  // classes of U+0000..7F, 2 bits each, for this cls_shift
  uint32_t mask;
  uint32_t flags;        // kWpLower | kWpChinese
  uint32_t cls_shift;    // 0: clean_text, 2: not
  uint32_t self_bit;     // the table bit every non-ASCII code point must carry, 0 = none (cased)
  int32_t max_chars;     // max_input_chars_per_word
  int32_t longest;       // bytes of the longest piece
  int32_t post_add;      // tokens the post-processor adds to every encoding
  int32_t n_added;
  int32_t added_off[kBpeMaxAdded + 1];
};

// Can the counters run on this block? (host: tb_wp_count before it launches, wp_fill_params before
// it returns.) fold1 set selects the folding kernel, which reads all three fold tables.
inline bool wp_params_ok(const DevWp& T) {
  if (T.n_added < 0 || T.n_added > kBpeMaxAdded || T.longest < 1 || T.max_chars < 0) return false;
  return T.fold1 == nullptr || (T.fold2 != nullptr && T.foldp != nullptr);
}

// hash state of a byte string: h(s + c) = h(s) * B + c + 1, h("") = 0
TB_HD uint64_t wp_push(uint64_t h, uint32_t byte) { return h * kWpBase + byte + 1; }
TB_HD uint64_t wp_pop(uint64_t h, uint32_t byte) { return (h - (byte + 1)) * kWpBaseInv; }
TB_HD uint64_t wp_key(uint64_t h, uint32_t nbytes, uint32_t cont) {
  return bpe_hash(h + (((uint64_t)cont << 31) | nbytes) * 0xD6E8FEB86659FD93ull);
}
TB_HD uint64_t wp_val(uint64_t off, uint32_t nbytes, uint32_t cont) { return (off << 32) | (cont << 31) | nbytes; }

TB_HD bool wp_is_cjk(uint32_t c) {
  return (c >= 0x4E00 && c <= 0x9FFF) || (c >= 0x3400 && c <= 0x4DBF) || (c >= 0x20000 && c <= 0x2A6DF) ||
         (c >= 0x2A700 && c <= 0x2B73F) || (c >= 0x2B740 && c <= 0x2B81F) || (c >= 0x2B920 && c <= 0x2CEAF) ||
         (c >= 0xF900 && c <= 0xFAFF) || (c >= 0x2F800 && c <= 0x2FA1F);
}

// Class of the code point at b[i] (i < n), *len its bytes; -1: invalid UTF-8, or a code point the
// tokenizer's lowercase / strip_accents would change (the document goes to the host).
TB_HD int wp_cp(const DevWp& T, const uint8_t* b, int64_t i, int64_t n, int* len) {
  const uint32_t c0 = b[i];
  if (c0 < 0x80) {
    *len = 1;
    const uint64_t w = c0 < 64 ? (c0 < 32 ? T.asc0 : T.asc1) : (c0 < 96 ? T.asc2 : T.asc3);
    return (int)((w >> (2 * (c0 & 31))) & 3);
  }
  const int32_t c = bpe_decode(b, i, n, len);
  if (c < 0) return -1;
  const uint32_t e = T.cls2[(uint32_t)T.cls1[c >> 7] * 128 + (c & 127)];
  if (T.self_bit != 0 && (e & T.self_bit) == 0) return -1;
  const int k = (int)((e >> T.cls_shift) & 3);
  if (k == WP_ISO && !(T.flags & kWpChinese) && wp_is_cjk((uint32_t)c)) return WP_KEEP;
  return k;
}

// a text byte as the normalizer leaves it (only ASCII changes on the device)
TB_HD uint32_t wp_byte(const DevWp& T, uint32_t x) {
  return ((T.flags & kWpLower) && x - 'A' < 26u) ? (x | 0x20) : x;
}

// start of the code point that ends at e (e > lo; valid UTF-8 between lo and e)
TB_HD int64_t wp_back(const uint8_t* b, int64_t e, int64_t lo) {
  int64_t s = e - 1;
  for (int k = 0; k < 3 && s > lo && (b[s] & 0xC0) == 0x80; ++k) --s;
  return s;
}

// Is the piece (cont, the nb normalised bytes from the kept code point at pos) in the vocabulary?
// h: their wp_push state. [pos, ...) is known to be valid (wp_word's first pass).
TB_HD bool wp_find(const DevWp& T, const uint8_t* b, int64_t n, int64_t pos, uint64_t h, int nb, uint32_t cont) {
  const uint64_t key = wp_key(h, (uint32_t)nb, cont);
  const uint32_t lo = (cont << 31) | (uint32_t)nb;
  uint32_t s = (uint32_t)key & T.mask;
  for (;;) {
    const WpSlot e = T.slots[s];
    if (e.val == kWpEmpty) return false;
    if (e.key == key && (uint32_t)e.val == lo) {
      const uint8_t* w = T.pool + (e.val >> 32);
      bool same = true;
      int m = 0;
      for (int64_t q = pos; m < nb && q < n;) {
        int l;
        const int k = wp_cp(T, b, q, n, &l);
        if (k < 0) return false;
        if (k == WP_KEEP) {
          for (int j = 0; j < l && m + j < nb; ++j) same = same && w[m + j] == wp_byte(T, b[q + j]);
          m += l;
        }
        q += l;
      }
      if (same && m == nb) return true;
    }
    s = (s + 1) & T.mask;
  }
}

// Tokens of the word whose first kept code point starts at ws; *end: the first byte after it (a
// space, an isolate, or n). -1: count the document on the host.
TB_HD int64_t wp_word(const DevWp& T, const uint8_t* b, int64_t n, int64_t ws, int64_t* end) {
  int64_t we = ws, nch = 0, rem = 0;  // kept characters and their bytes
  while (we < n) {
    int l;
    const int k = wp_cp(T, b, we, n, &l);
    if (k < 0) return -1;
    if (k >= WP_SPACE) break;
    if (k == WP_KEEP) {
      ++nch;
      rem += l;
    }
    we += l;
  }
  *end = we;
  if (nch > T.max_chars) return 1;
  int64_t pieces = 0, pos = ws;
  uint32_t cont = 0;
  while (rem > 0) {
    // the longest candidate: whole kept code points from pos, at most T.longest bytes; e: its end
    uint64_t h = 0;
    int nb = 0;
    int64_t e = pos;
    for (int64_t q = pos; q < we;) {
      int l;
      const int k = wp_cp(T, b, q, n, &l);
      if (k == WP_KEEP) {
        if (nb + l > T.longest) break;
        for (int j = 0; j < l; ++j) h = wp_push(h, wp_byte(T, b[q + j]));
        nb += l;
        e = q + l;
      }
      q += l;
    }
    bool hit = false;
    while (nb > 0) {
      if (wp_find(T, b, n, pos, h, nb, cont)) {
        hit = true;
        break;
      }
      // take the last kept code point off, then the drops before it
      const int64_t s = wp_back(b, e, pos);
      for (int64_t j = e - 1; j >= s; --j) h = wp_pop(h, wp_byte(T, b[j]));
      nb -= (int)(e - s);
      e = s;
      while (e > pos) {
        const int64_t s2 = wp_back(b, e, pos);
        int l;
        if (wp_cp(T, b, s2, n, &l) != WP_DROP) break;
        e = s2;
      }
    }
    if (!hit) return 1;  // no piece at pos: the whole word is the unknown token
    ++pieces;
    rem -= nb;
    pos = e;
    cont = 1;
  }
  return pieces;
}

// does the text of an added token start at a byte in [s0, s1)?
TB_HD bool wp_has_added(const DevWp& T, const uint8_t* b, int64_t n, int64_t s0, int64_t s1) {
  for (int a = 0; a < T.n_added; ++a) {
    const uint8_t* t = T.added + T.added_off[a];
    const int64_t tl = T.added_off[a + 1] - T.added_off[a];
    if (tl <= 0 || tl > n) continue;
    for (int64_t i = s0; i < s1 && i + tl <= n; ++i) {
      if (b[i] != t[0]) continue;
      int64_t j = 1;
      while (j < tl && b[i + j] == t[j]) ++j;
      if (j == tl) return true;
    }
  }
  return false;
}

// Tokens of the words that start in [s0, s1) (s0 < n); -1: count the document on the host. The
// ranges of a partition of [0, n) see every code point once, so their sum is the document's count
// and any of them finds invalid UTF-8.
TB_HD int64_t wp_count_range(const DevWp& T, const uint8_t* b, int64_t n, int64_t s0, int64_t s1) {
  int64_t p = s0;
  if (p > 0) {
    if ((b[p] & 0xC0) == 0x80) {  // inside a code point that starts in the range before
      const int64_t q = wp_back(b, p + 1, 0);
      int l;
      if (bpe_decode(b, q, n, &l) < 0 || q + l <= p) return -1;
      p = q + l;
    }
    // a word that runs into p started before it: find the nearest code point that is no drop
    bool inword = false;
    for (int64_t e = p; e > 0;) {
      const int64_t q = wp_back(b, e, 0);
      int l;
      const int k = wp_cp(T, b, q, n, &l);
      if (k < 0 || q + l != e) return -1;
      if (k != WP_DROP) {
        inword = k == WP_KEEP;
        break;
      }
      e = q;
    }
    while (inword && p < n) {
      int l;
      const int k = wp_cp(T, b, p, n, &l);
      if (k < 0) return -1;
      if (k >= WP_SPACE) break;
      p += l;
    }
  }
  int64_t total = 0;
  while (p < n && p < s1) {
    int l;
    const int k = wp_cp(T, b, p, n, &l);
    if (k < 0) return -1;
    if (k == WP_KEEP) {
      int64_t e;
      const int64_t w = wp_word(T, b, n, p, &e);
      if (w < 0) return -1;
      total += w;
      p = e;
    } else {
      total += k == WP_ISO;
      p += l;
    }
  }
  return total;
}

// Token count of one document (kBpeHost: count it on the host), sequentially.
TB_HD int32_t wp_count_doc(const DevWp& T, const uint8_t* b, int64_t n) {
  if (T.n_added && wp_has_added(T, b, n, 0, n)) return kBpeHost;
  const int64_t k = n > 0 ? wp_count_range(T, b, n, 0, n) : 0;
  if (k < 0 || k + T.post_add > 0x7FFFFFFF) return kBpeHost;
  return (int32_t)(k + T.post_add);
}

// ---- folding variant: lowercase / strip_accents beyond ASCII (wp_fold.inc) -------------------------
// One input code point becomes 0 to 3 output code points (at most 12 bytes), read from the fold
// table of the tokenizer's mode, or by arithmetic for a Hangul syllable. Its effective class is the
// output's (an empty output is a drop); pieces are hashed and compared over output bytes, and a
// search position is a pair (input byte offset of a code point, byte offset into its output), so
// a piece may end between the jamo of one syllable. A code point whose place depends on context
// (kWpFoldHost in the table) sends the document to the host.
constexpr uint32_t kWpFoldHost = 0xFFFF;
constexpr uint32_t kWpFoldHangul = 0xFFFE;

struct WpOut {
  int cls;       // effective class; -1: invalid UTF-8 or a host code point
  int len;       // input bytes
  int nb;        // output bytes when cls == WP_KEEP, else 0
  uint32_t src;  // where they are: 0 the input bytes, bit 31 | Hangul syllable index, else fold pool offset
};

TB_HD int wp_u8len(uint32_t lead) { return lead < 0x80 ? 1 : (lead < 0xE0 ? 2 : (lead < 0xF0 ? 3 : 4)); }

// output byte j (< c.nb) of the code point c = wpf_cp(T, b, q, n)
TB_HD uint32_t wpf_byte(const DevWp& T, const uint8_t* b, int64_t q, const WpOut& c, int j) {
  if (c.src == 0) return wp_byte(T, b[q + j]);
  if (c.src & 0x80000000u) {
    // NFD of a syllable: U+1100 + L, U+1161 + V and, if T != 0, U+11A7 + T; in UTF-8 E1 84..87 80..BF
    const uint32_t s = c.src & 0x7FFFFFFFu;
    const int t = j / 3, r = j - 3 * t;
    const uint32_t cp = t == 0 ? 0x1100 + s / 588 : (t == 1 ? 0x1161 + (s % 588) / 28 : 0x11A7 + s % 28);
    return r == 0 ? 0xE1u : (r == 1 ? 0x80 | ((cp >> 6) & 0x3F) : 0x80 | (cp & 0x3F));
  }
  return T.foldp[c.src + j];
}

// The code point at b[i] (i < n) as the folding normalizer leaves it.
TB_HD WpOut wpf_cp(const DevWp& T, const uint8_t* b, int64_t i, int64_t n) {
  WpOut r;
  r.nb = 0;
  r.src = 0;
  const uint32_t c0 = b[i];
  if (c0 < 0x80) {
    r.len = 1;
    const uint64_t w = c0 < 64 ? (c0 < 32 ? T.asc0 : T.asc1) : (c0 < 96 ? T.asc2 : T.asc3);
    r.cls = (int)((w >> (2 * (c0 & 31))) & 3);
    r.nb = r.cls == WP_KEEP;
    return r;
  }
  int len;
  const int32_t c = bpe_decode(b, i, n, &len);
  r.len = len;
  if (c < 0) {
    r.cls = -1;
    return r;
  }
  const uint32_t e = T.fold2[(uint32_t)T.fold1[c >> 7] * 128 + (c & 127)];
  if (e == 0) {
    int k = (int)((T.cls2[(uint32_t)T.cls1[c >> 7] * 128 + (c & 127)] >> T.cls_shift) & 3);
    if (k == WP_ISO && !(T.flags & kWpChinese) && wp_is_cjk((uint32_t)c)) k = WP_KEEP;
    r.cls = k;
    if (k == WP_KEEP) r.nb = len;
    return r;
  }
  if (e == kWpFoldHost) {
    r.cls = -1;
    return r;
  }
  if (e == kWpFoldHangul) {
    const uint32_t s = (uint32_t)c - 0xAC00;
    r.cls = WP_KEEP;
    r.nb = s % 28 ? 9 : 6;
    r.src = 0x80000000u | s;
    return r;
  }
  const uint32_t h = T.foldp[e - 1];
  int k = (int)((h >> (T.cls_shift ? 6 : 4)) & 3);
  if (k == WP_ISO && !(T.flags & kWpChinese) && wp_is_cjk((uint32_t)c)) k = WP_KEEP;
  r.cls = k;
  if (k == WP_KEEP) {
    // a kept output carries no spaces; an ideograph kept only for want of handle_chinese_chars
    // was recorded with the two spaces around it
    const int sp = (h & 15) > 0 && T.foldp[e] == ' ';
    r.nb = (int)(h & 15) - 2 * sp;
    r.src = e + sp;
  }
  return r;
}

TB_HD bool wpf_find(const DevWp& T, const uint8_t* b, int64_t n, int64_t pq, int pk, uint64_t h, int nb,
                    uint32_t cont) {
  const uint64_t key = wp_key(h, (uint32_t)nb, cont);
  const uint32_t lo = (cont << 31) | (uint32_t)nb;
  uint32_t s = (uint32_t)key & T.mask;
  for (;;) {
    const WpSlot e = T.slots[s];
    if (e.val == kWpEmpty) return false;
    if (e.key == key && (uint32_t)e.val == lo) {
      const uint8_t* w = T.pool + (e.val >> 32);
      bool same = true;
      int m = 0;
      for (int64_t q = pq; m < nb && q < n;) {
        const WpOut c = wpf_cp(T, b, q, n);
        if (c.cls < 0) return false;
        for (int j = q == pq ? pk : 0; j < c.nb && m < nb; ++j, ++m) same = same && w[m] == wpf_byte(T, b, q, c, j);
        q += c.len;
      }
      if (same && m == nb) return true;
    }
    s = (s + 1) & T.mask;
  }
}

// wp_word over the folded text: ws is the first code point with a kept, non-empty output.
TB_HD int64_t wpf_word(const DevWp& T, const uint8_t* b, int64_t n, int64_t ws, int64_t* end) {
  int64_t we = ws, nch = 0, rem = 0;  // output characters and their bytes
  while (we < n) {
    const WpOut c = wpf_cp(T, b, we, n);
    if (c.cls < 0) return -1;
    if (c.cls >= WP_SPACE) break;
    for (int j = 0; j < c.nb; ++j) nch += (wpf_byte(T, b, we, c, j) & 0xC0) != 0x80;
    rem += c.nb;
    we += c.len;
  }
  *end = we;
  if (nch > T.max_chars) return 1;
  int64_t pieces = 0, pq = ws;
  int pk = 0;
  uint32_t cont = 0;
  while (rem > 0) {
    // the longest candidate: whole output code points from (pq, pk), at most T.longest bytes;
    // (eq, ek): the input code point its last one came from and the output offset behind it
    uint64_t h = 0;
    int nb = 0, ek = pk;
    int64_t eq = pq;
    bool full = false;
    for (int64_t q = pq; q < we && !full;) {
      const WpOut c = wpf_cp(T, b, q, n);
      for (int k = q == pq ? pk : 0; k < c.nb;) {
        const int l = wp_u8len(wpf_byte(T, b, q, c, k));
        if (nb + l > T.longest) {
          full = true;
          break;
        }
        for (int j = 0; j < l; ++j) h = wp_push(h, wpf_byte(T, b, q, c, k + j));
        nb += l;
        k += l;
        eq = q;
        ek = k;
      }
      q += c.len;
    }
    bool hit = false;
    while (nb > 0) {
      if (wpf_find(T, b, n, pq, pk, h, nb, cont)) {
        hit = true;
        break;
      }
      // take the last output code point off; at the front of an input code point's output go
      // back to the nearest one before it that has output
      WpOut c = wpf_cp(T, b, eq, n);
      int s = ek - 1;
      while (s > 0 && (wpf_byte(T, b, eq, c, s) & 0xC0) == 0x80) --s;
      for (int j = ek - 1; j >= s; --j) h = wp_pop(h, wpf_byte(T, b, eq, c, j));
      nb -= ek - s;
      ek = s;
      while (nb > 0 && ek == 0) {
        eq = wp_back(b, eq, pq);
        c = wpf_cp(T, b, eq, n);
        ek = c.nb;
      }
    }
    if (!hit) return 1;  // no piece at the position: the whole word is the unknown token
    ++pieces;
    rem -= nb;
    pq = eq;
    pk = ek;
    cont = 1;
  }
  return pieces;
}

TB_HD int64_t wpf_count_range(const DevWp& T, const uint8_t* b, int64_t n, int64_t s0, int64_t s1) {
  int64_t p = s0;
  if (p > 0) {
    if ((b[p] & 0xC0) == 0x80) {  // inside a code point that starts in the range before
      const int64_t q = wp_back(b, p + 1, 0);
      int l;
      if (bpe_decode(b, q, n, &l) < 0 || q + l <= p) return -1;
      p = q + l;
    }
    // a word that runs into p started before it: find the nearest code point that is no drop
    bool inword = false;
    for (int64_t e = p; e > 0;) {
      const int64_t q = wp_back(b, e, 0);
      const WpOut c = wpf_cp(T, b, q, n);
      if (c.cls < 0 || q + c.len != e) return -1;
      if (c.cls != WP_DROP) {
        inword = c.cls == WP_KEEP;
        break;
      }
      e = q;
    }
    while (inword && p < n) {
      const WpOut c = wpf_cp(T, b, p, n);
      if (c.cls < 0) return -1;
      if (c.cls >= WP_SPACE) break;
      p += c.len;
    }
  }
  int64_t total = 0;
  while (p < n && p < s1) {
    const WpOut c = wpf_cp(T, b, p, n);
    if (c.cls < 0) return -1;
    if (c.cls == WP_KEEP) {
      int64_t e;
      const int64_t w = wpf_word(T, b, n, p, &e);
      if (w < 0) return -1;
      total += w;
      p = e;
    } else {
      total += c.cls == WP_ISO;
      p += c.len;
    }
  }
  return total;
}

// The counter by policy: Fold = false is the identity path above, unchanged.
template <bool Fold>
TB_HD int64_t wp_count_range_t(const DevWp& T, const uint8_t* b, int64_t n, int64_t s0, int64_t s1) {
  if (Fold) return wpf_count_range(T, b, n, s0, s1);
  return wp_count_range(T, b, n, s0, s1);
}

template <bool Fold>
TB_HD int32_t wp_count_doc_t(const DevWp& T, const uint8_t* b, int64_t n) {
  if (T.n_added && wp_has_added(T, b, n, 0, n)) return kBpeHost;
  const int64_t k = n > 0 ? wp_count_range_t<Fold>(T, b, n, 0, n) : 0;
  if (k < 0 || k + T.post_add > 0x7FFFFFFF) return kBpeHost;
  return (int32_t)(k + T.post_add);
}

#ifndef __HIP_DEVICE_COMPILE__
// Fills the free slots[0 .. mask] (val = kWpEmpty, mask + 1 >= 2 n a power of two) with the n
// distinct pieces (cont[i], pool[off[i] .. off[i + 1])); returns the longest piece's bytes.
inline int64_t wp_fill_slots(const uint8_t* pool, const int64_t* off, const uint8_t* cont, size_t n, WpSlot* slots,
                             uint64_t mask) {
  int64_t longest = 1;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t nb = (uint32_t)(off[i + 1] - off[i]);
    uint64_t h = 0;
    for (uint32_t j = 0; j < nb; ++j) h = wp_push(h, pool[off[i] + j]);
    const uint64_t key = wp_key(h, nb, cont[i]);
    uint64_t s = (uint32_t)key & mask;
    while (slots[s].val != kWpEmpty) s = (s + 1) & mask;
    slots[s].key = key;
    slots[s].val = wp_val((uint64_t)off[i], nb, cont[i]);
    if (nb > longest) longest = nb;
  }
  return longest;
}

// the ASCII class words of DevWp (asc0..asc3) for a cls_shift, from the table
inline void wp_ascii_classes(const uint16_t* cls1, const uint8_t* cls2, uint32_t shift, uint64_t out[4]) {
  for (int w = 0; w < 4; ++w) out[w] = 0;
  for (uint32_t c = 0; c < 128; ++c) {
    const uint64_t k = (cls2[(uint32_t)cls1[0] * 128 + c] >> shift) & 3;
    out[c >> 5] |= k << (2 * (c & 31));
  }
}
#endif

}  // namespace tb
