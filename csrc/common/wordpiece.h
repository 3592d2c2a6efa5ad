// WordPiece (BERT) token counting (TokenCounter, reference src/pipeline/token/token_counter.rs:31-42:
// ``tokenizer.encode(text, true).get_tokens().len()``) for tokenizers made of BertNormalizer +
// BertPreTokenizer + a WordPiece model, plus the tokens the post-processor adds. Shared by the HIP
// kernel (csrc/hip/wordpiece.hip: one wave per kept document, a byte range per lane) and its host
// emulation (csrc/host/module.cpp wp_count), which CPU tests pin to the `tokenizers` library.
//
// Words. Every code point has a class (wp_classes.inc, generated from the library): keep, drop
// (removed, so its neighbours join), space, isolate (punctuation and CJK ideographs: a word of its
// own). A word is a maximal run of keep code points with the drops between them taken out, or one
// isolate. So word starts are a local property of the text: a keep code point starts a word iff
// the nearest code point before it that is not a drop is a space or an isolate, or there is none.
// A lane counts the words that start in its byte range, wherever they end.
//
// Normalisation. Cased tokenizers need none beyond the classes. With lowercase / strip_accents
// ASCII is folded here and every other code point must carry the "normalises to itself" bit of its
// combination; a document with one that does not is counted on the host (kBpeHost), as are
// documents with invalid UTF-8 or the text of an added token (the library splits on those first).
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
