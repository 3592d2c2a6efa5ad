// Unigram (T5, mT5, XLM-R) token counting (TokenCounter, reference src/pipeline/token/token_counter.rs:31-42:
// ``tokenizer.encode(text, true).get_tokens().len()``) for tokenizers made of a Precompiled
// normalizer, white-space splitting, Metaspace and a Unigram model, plus the tokens the
// post-processor adds. Shared by the HIP kernel (csrc/hip/unigram.hip: one wave per kept document, a
// byte range per lane) and its host emulation (csrc/host/tok_module.cpp uni_count), which CPU tests
// pin to the `tokenizers` library.
//
// Words. Every code point has a class (2 bits in a two-stage table that models/tokenizer.py probes
// from the file's own normalizer): keep (the normalizer leaves it as it is), space (it becomes
// U+0020, or the pre-tokenizer splits on it) and host (anything else: the document is counted on
// the host, kBpeHost, as are documents with invalid UTF-8, the text of an added token or the unk
// piece's own text). A word is a maximal run of keep code points, so word starts are a local
// property of the text and a lane counts the words that start in its byte range, wherever they end.
// The library encodes each word on its own as U+2581 + word.
//
// Pieces. The vocabulary is an open-addressed table keyed by wordpiece.h's polynomial hash of the
// piece's bytes; every slot whose key matches is compared byte for byte against the piece pool
// before it counts. A slot carries the piece's f64 score.
//
// The count of a word is that of the library's Viterbi (tokenizers 0.22 Unigram::encode_optimized
// + tokenize) without its backtracking. Nodes are the code point boundaries of U+2581 + word. From
// every node in turn, pieces of 1, 2, .. code points that start there propose score + best[node]
// (one f64 add) to the node where they end, and where no piece of one code point matched the
// unknown edge proposes unk_score + best[node] to the next node; a node takes a proposal when it
// has none yet or when the proposal is strictly greater. A node has all its proposals before it is
// used as a start, so the token count of its best path, and whether that path ends in an unknown,
// travel with the score: an unknown behind an unknown adds no token (fuse_unk), and with
// byte_fallback an unknown code point adds its bytes. Only the nodes up to the longest piece ahead
// are live, so the state is a ring of (longest piece in code points + 1) entries whatever the
// word's length: words and documents have no size limit.
//
// Replacements (a block with a map: DevUni::map1 .. mpool, built by models/tokenizer.py
// unigram_map; the unim_* functions, k_uni_count_map). A fourth class, map, marks a code point that
// is a grapheme of its own and that the normalizer replaces by up to kUniMaxMapBytes bytes or
// drops. Its record holds the output as the library's later steps see it, white space as 0x20. The
// counter then runs over the normalised text without materialising it: a position (UniCur) is an
// input byte offset plus a byte offset into that code point's output, where a keep code point's
// output is its own bytes. The output's code points are not classified again (the library does not
// normalise twice): 0x20 separates words and every other byte is word text. A word starts at an
// output code point other than 0x20 whose nearest predecessor in the output, across dropped code
// points, is 0x20 or nothing - possibly in the middle of an output - and belongs to the lane in
// whose range its input code point begins. The ring's nodes are the code point boundaries of the
// output; longest_cp and longest bound candidates in output code points and bytes. Replacements can
// spell the unk piece's text where the raw text has none (the library then hands the characters to
// the model, and what it makes of them depends on the neighbours): a candidate that matches the unk
// piece sends the document to the host. And the normalizer looks a whole grapheme under 6 bytes up
// at once and replaces all of it by the output of its first code point: a map code point swallows a
// joiner behind it that on its own would have become a space (U+200C behind nmt_nfkc). Such
// joiners keep their class, space, and carry a record with kUniRecJoin; a map code point directly
// in front of one sends the document to the host.
#pragma once
#include <cstddef>

#include "wordpiece.h"

namespace tb {

enum UniCls : int { UNI_KEEP = 0, UNI_SPACE = 1, UNI_HOST = 2, UNI_MAP = 3 };
constexpr uint32_t kUniByteFallback = 1;  // DevUni::flags: an unknown code point counts its bytes
constexpr int kUniMaxPieceCp = 32;        // the ring's capacity: the longest piece in code points
constexpr int kUniMaxPieceBytes = 128;    // ... and in bytes
constexpr uint32_t kUniNone = ~0u;        // ring entry without a proposal
constexpr uint32_t kUniMaxCount = 0x7FFFFF00u;  // a word with more tokens goes to the host
constexpr int kUniMaxMapBytes = 32;       // the longest replacement a record holds
constexpr uint16_t kUniMapNone = 0xFFFF;  // DevUni::map2: the code point has no record
constexpr uint32_t kUniRecLen = 0x7F;     // DevUni::mrec: the bits of the length
constexpr uint32_t kUniRecJoin = 0x80;    // ... a space code point that joins the grapheme in front of it

struct UniSlot {
  uint64_t key;    // wp_key of the piece's bytes
  uint64_t val;    // pool offset << 32 | (id == unk_id) << 31 | bytes; kWpEmpty = free
  uint64_t score;  // the piece's f64 score, as bits
};

struct DevUni {
  const UniSlot* slots;  // [mask + 1], at most half full
  const uint8_t* pool;   // piece bytes
  const uint16_t* cls1;  // class table: stage 1 by code point >> 7
  const uint8_t* cls2;   // stage 2: 32 bytes per block, 2 bits per code point
  const uint8_t* added;  // contents of the added tokens and the unk piece, concatenated
  const int32_t* aoff;   // [n_added + 1] offsets into added
  uint64_t asc0, asc1, asc2, asc3;  // classes of U+0000..7F, 2 bits each
  uint64_t amask[4];     // bit x: an added token starts with byte x
  double unk_score;      // min(score) - 10
  uint32_t mask;
  uint32_t flags;        // kUniByteFallback
  uint32_t sp_bytes;     // UTF-8 of the replacement character (U+2581), first byte lowest
  int32_t sp_len;
  int32_t longest_cp;    // code points of the longest piece
  int32_t longest;       // bytes of the longest piece
  int32_t post_add;      // tokens the post-processor adds to every encoding
  int32_t n_added;
  // the normalizer's replacements; all null: a block without a map (k_uni_count)
  const uint16_t* map1;   // stage 1 by code point >> 7
  const uint16_t* map2;   // stage 2: 128 record numbers per block, kUniMapNone = none
  const uint32_t* mrec;   // records: offset in mpool << 8 | kUniRecJoin | bytes (0: the code point is dropped)
  const uint8_t* mpool;   // the outputs' bytes
};

TB_HD bool uni_has_map(const DevUni& T) { return T.map1 != nullptr; }

// Can the counter run on this block? (host: tb_uni_count before it launches, uni_fill_params
// before it returns.)
inline bool uni_params_ok(const DevUni& T) {
  if (T.slots == nullptr || T.pool == nullptr || T.cls1 == nullptr || T.cls2 == nullptr) return false;
  if (T.n_added < 0 || T.n_added > kBpeSplitMaxAdded || (T.n_added && (T.added == nullptr || T.aoff == nullptr)))
    return false;
  if (T.longest_cp < 1 || T.longest_cp > kUniMaxPieceCp || T.longest < 1 || T.longest > kUniMaxPieceBytes) return false;
  const int maps = (T.map1 != nullptr) + (T.map2 != nullptr) + (T.mrec != nullptr) + (T.mpool != nullptr);
  if (maps != 0 && maps != 4) return false;  // a map has all four tables
  return T.sp_len >= 1 && T.sp_len <= 4;
}

// The counter's state of one word: entry i at s[i * stride], m[i * stride] (stride = wave width in
// LDS, 1 on the host), longest_cp + 1 entries. m: tokens << 1 | the path ends in an unknown.
struct UniRing {
  double* s;
  uint32_t* m;
  int stride;
};

// Class of the code point at b[i] (i < n), *len its bytes; -1: invalid UTF-8 or a host code point.
TB_HD int uni_cp(const DevUni& T, const uint8_t* b, int64_t i, int64_t n, int* len) {
  const uint32_t c0 = b[i];
  int k;
  if (c0 < 0x80) {
    *len = 1;
    const uint64_t w = c0 < 64 ? (c0 < 32 ? T.asc0 : T.asc1) : (c0 < 96 ? T.asc2 : T.asc3);
    k = (int)((w >> (2 * (c0 & 31))) & 3);
  } else {
    const int32_t c = bpe_decode(b, i, n, len);
    if (c < 0) return -1;
    k = (T.cls2[(uint32_t)T.cls1[c >> 7] * 32 + ((c & 127) >> 2)] >> (2 * (c & 3))) & 3;
  }
  return k >= UNI_HOST ? -1 : k;
}

// byte j of the replacement character
TB_HD uint32_t uni_sp_byte(const DevUni& T, int j) { return (T.sp_bytes >> (8 * j)) & 0xFF; }

// The slot of the piece made of the replacement character (lead) and the text bytes b[p ..), nb
// bytes in all with the wp_push state h; null when it is not in the vocabulary.
TB_HD const UniSlot* uni_find(const DevUni& T, const uint8_t* b, int64_t p, bool lead, uint64_t h, int nb) {
  const uint64_t key = wp_key(h, (uint32_t)nb, 0);
  uint32_t s = (uint32_t)key & T.mask;
  for (;;) {
    const UniSlot* e = T.slots + s;
    const uint64_t v = e->val;
    if (v == kWpEmpty) return nullptr;
    if (e->key == key && ((uint32_t)v & 0x7FFFFFFFu) == (uint32_t)nb) {
      const uint8_t* w = T.pool + (v >> 32);
      const int pre = lead ? T.sp_len : 0;
      bool same = true;
      for (int j = 0; j < pre; ++j) same = same && w[j] == uni_sp_byte(T, j);
      for (int j = pre; j < nb; ++j) same = same && w[j] == b[p + (j - pre)];
      if (same) return e;
    }
    s = (s + 1) & T.mask;
  }
}

TB_HD double uni_score(const UniSlot* e) {
  union {
    uint64_t u;
    double d;
  } x;
  x.u = e->score;
  return x.d;
}

TB_HD void uni_propose(const UniRing& R, int slot, double score, uint32_t m) {
  const int i = slot * R.stride;
  if (R.m[i] == kUniNone || score > R.s[i]) {
    R.s[i] = score;
    R.m[i] = m;
  }
}

// Tokens of the word whose first code point starts at ws (a keep code point); *end: the first byte
// after it (a space, or n). -1: count the document on the host.
TB_HD int64_t uni_word(const DevUni& T, const uint8_t* b, int64_t n, int64_t ws, int64_t* end, const UniRing& R) {
  const int nr = T.longest_cp + 1;
  for (int i = 0; i < nr; ++i) R.m[i * R.stride] = kUniNone;
  double best = 0.0;  // the node that is expanded: its score, its tokens << 1 | unknown
  uint32_t meta = 0;
  int slot = 0;
  int64_t p = ws;    // where the text goes on behind the node
  bool lead = true;  // the first node: the replacement character stands between it and b[ws]
  for (;;) {
    uint64_t h = 0;
    int nb = 0, k = 0, first = 0;  // bytes and code points of the candidate, bytes of its first code point
    int64_t q = p;
    bool single = false;
    int ts = slot;
    if (lead) {
      for (int j = 0; j < T.sp_len; ++j) h = wp_push(h, uni_sp_byte(T, j));
      nb = first = T.sp_len;
    }
    for (;;) {
      if (!(lead && k == 0)) {  // the next code point of the text
        int l = 0;
        const int c = q < n ? uni_cp(T, b, q, n, &l) : UNI_SPACE;
        if (c < 0) return -1;
        if (c == UNI_SPACE) {
          if (k == 0) {  // the node is the word's end
            *end = p;
            return (int64_t)(meta >> 1);
          }
          break;
        }
        if (k == 0) first = l;
        if (nb + l > T.longest) break;
        for (int j = 0; j < l; ++j) h = wp_push(h, b[q + j]);
        nb += l;
        q += l;
      }
      ++k;
      ts = ts + 1 == nr ? 0 : ts + 1;
      const UniSlot* e = uni_find(T, b, p, lead, h, nb);
      if (e != nullptr) {
        const bool unk = (e->val >> 31) & 1;  // the unk piece's own text: an unknown of one token
        uni_propose(R, ts, uni_score(e) + best, unk ? (((meta >> 1) + !(meta & 1)) << 1) | 1 : ((meta >> 1) + 1) << 1);
        single = single || k == 1;
      }
      if (k >= T.longest_cp) break;
    }
    slot = slot + 1 == nr ? 0 : slot + 1;
    if (!single) {
      const uint32_t add = (T.flags & kUniByteFallback) ? (uint32_t)first : !(meta & 1);
      uni_propose(R, slot, T.unk_score + best, (((meta >> 1) + add) << 1) | 1);
    }
    if (!lead) p += first;
    lead = false;
    best = R.s[slot * R.stride];
    meta = R.m[slot * R.stride];
    R.m[slot * R.stride] = kUniNone;  // the entry of the node longest_cp + 1 ahead
    if ((meta >> 1) > kUniMaxCount) return -1;
  }
}

// does the text of an added token (or of the unk piece) start at a byte in [s0, s1)?
TB_HD bool uni_has_added(const DevUni& T, const uint8_t* b, int64_t n, int64_t s0, int64_t s1) {
  for (int64_t i = s0; i < s1; ++i) {
    const uint32_t x = b[i];
    if (!((T.amask[x >> 6] >> (x & 63)) & 1)) continue;
    for (int a = 0; a < T.n_added; ++a) {
      const int32_t o = T.aoff[a];
      const int64_t tl = T.aoff[a + 1] - o;
      if (tl <= 0 || i + tl > n || T.added[o] != x) continue;
      int64_t j = 1;
      while (j < tl && b[i + j] == T.added[o + j]) ++j;
      if (j == tl) return true;
    }
  }
  return false;
}

// Tokens of the words that start in [s0, s1) (s0 < n); -1: count the document on the host. The
// ranges of a partition of [0, n) see every code point once, so their sum is the document's count
// and any of them finds invalid UTF-8 or a host code point.
TB_HD int64_t uni_count_range(const DevUni& T, const uint8_t* b, int64_t n, int64_t s0, int64_t s1,
                              const UniRing& R) {
  int64_t p = s0;
  if (p > 0) {
    if ((b[p] & 0xC0) == 0x80) {  // inside a code point that starts in the range before
      const int64_t q = wp_back(b, p + 1, 0);
      int l;
      if (bpe_decode(b, q, n, &l) < 0 || q + l <= p) return -1;
      p = q + l;
    }
    // a word that runs into p started before it
    const int64_t q = wp_back(b, p, 0);
    int l;
    int k = uni_cp(T, b, q, n, &l);
    if (k < 0 || q + l != p) return -1;
    while (k == UNI_KEEP && p < n) {
      k = uni_cp(T, b, p, n, &l);
      if (k < 0) return -1;
      if (k == UNI_KEEP) p += l;
    }
  }
  int64_t total = 0;
  while (p < n && p < s1) {
    int l;
    const int k = uni_cp(T, b, p, n, &l);
    if (k < 0) return -1;
    if (k == UNI_KEEP) {
      int64_t e;
      const int64_t w = uni_word(T, b, n, p, &e, R);
      if (w < 0) return -1;
      total += w;
      p = e;
    } else {
      p += l;
    }
  }
  return total;
}

// Token count of one document (kBpeHost: count it on the host), sequentially.
TB_HD int32_t uni_count_doc(const DevUni& T, const uint8_t* b, int64_t n, const UniRing& R) {
  if (T.n_added && uni_has_added(T, b, n, 0, n)) return kBpeHost;
  const int64_t k = n > 0 ? uni_count_range(T, b, n, 0, n, R) : 0;
  if (k < 0 || k + T.post_add > 0x7FFFFFFF) return kBpeHost;
  return (int32_t)(k + T.post_add);
}

// ---- the same over the normalised text of a block with a map (uni_has_map) ----

// A position in the normalised text: byte o of the output of the input code point at b[i].
struct UniCur {
  int64_t i;
  int o;
};

// The input code point at b[i] (i < n): its class (keep, space or map; -1: invalid UTF-8 or a host
// code point), *len its bytes, and for keep and map its output src[0 .. *ol) - its own bytes, or
// its record's (none: it is dropped).
TB_HD int unim_in(const DevUni& T, const uint8_t* b, int64_t i, int64_t n, int* len, const uint8_t** src, int* ol) {
  const uint32_t c0 = b[i];
  int32_t c = (int32_t)c0;
  int k;
  if (c0 < 0x80) {
    *len = 1;
    const uint64_t w = c0 < 64 ? (c0 < 32 ? T.asc0 : T.asc1) : (c0 < 96 ? T.asc2 : T.asc3);
    k = (int)((w >> (2 * (c0 & 31))) & 3);
  } else {
    c = bpe_decode(b, i, n, len);
    if (c < 0) return -1;
    k = (T.cls2[(uint32_t)T.cls1[c >> 7] * 32 + ((c & 127) >> 2)] >> (2 * (c & 3))) & 3;
  }
  if (k == UNI_HOST) return -1;
  *src = b + i;
  *ol = *len;
  if (k == UNI_MAP) {
    const uint32_t r = T.map2[(uint32_t)T.map1[c >> 7] * 128 + (c & 127)];
    if (r == kUniMapNone) return -1;  // the validator rules it out
    const uint32_t e = T.mrec[r];
    *src = T.mpool + (e >> 8);
    *ol = (int)(e & kUniRecLen);
    const int64_t j = i + *len;
    if (j < n && b[j] >= 0x80) {  // a space that would join this code point's grapheme?
      int l2;
      const int32_t c2 = bpe_decode(b, j, n, &l2);
      if (c2 < 0) return -1;
      const uint32_t r2 = T.map2[(uint32_t)T.map1[c2 >> 7] * 128 + (c2 & 127)];
      if (r2 != kUniMapNone && (T.mrec[r2] & kUniRecJoin)) return -1;
    }
  }
  return k;
}

// The output code point at or behind *c. UNI_KEEP: word text, its bytes src[0 .. *l); UNI_SPACE: a
// separator, or the end of the document (then c->i == n); -1: count the document on the host. *c
// moves over dropped code points to where the code point was read, *nx is the position behind it.
TB_HD int unim_next(const DevUni& T, const uint8_t* b, int64_t n, UniCur* c, const uint8_t** src, int* l, UniCur* nx) {
  for (;;) {
    if (c->i >= n) {
      *l = 0;
      *nx = *c;
      return UNI_SPACE;
    }
    int il, ol;
    const uint8_t* s;
    const int k = unim_in(T, b, c->i, n, &il, &s, &ol);
    if (k < 0) return -1;
    if (k == UNI_SPACE) {
      *l = 1;
      nx->i = c->i + il;
      nx->o = 0;
      return UNI_SPACE;
    }
    if (c->o < ol) {
      const uint32_t x = s[c->o];
      int w = x < 0xC0 ? 1 : (x < 0xE0 ? 2 : (x < 0xF0 ? 3 : 4));
      if (w > ol - c->o) w = ol - c->o;  // whatever the record holds, no byte behind it is read
      *src = s + c->o;
      *l = w;
      const bool last = c->o + w >= ol;
      nx->i = last ? c->i + il : c->i;
      nx->o = last ? 0 : c->o + w;
      return x == 0x20 ? UNI_SPACE : UNI_KEEP;
    }
    c->i += il;  // dropped
    c->o = 0;
  }
}

// uni_find over the normalised text from p
TB_HD const UniSlot* unim_find(const DevUni& T, const uint8_t* b, int64_t n, UniCur p, bool lead, uint64_t h, int nb) {
  const uint64_t key = wp_key(h, (uint32_t)nb, 0);
  uint32_t s = (uint32_t)key & T.mask;
  for (;;) {
    const UniSlot* e = T.slots + s;
    const uint64_t v = e->val;
    if (v == kWpEmpty) return nullptr;
    if (e->key == key && ((uint32_t)v & 0x7FFFFFFFu) == (uint32_t)nb) {
      const uint8_t* w = T.pool + (v >> 32);
      int j = lead ? T.sp_len : 0;
      bool same = true;
      for (int t = 0; t < j; ++t) same = same && w[t] == uni_sp_byte(T, t);
      UniCur c = p;
      while (same && j < nb) {  // the candidate's nb bytes were read from p on: word text all of them
        const uint8_t* x;
        int l;
        UniCur nx;
        if (unim_next(T, b, n, &c, &x, &l, &nx) != UNI_KEEP) return nullptr;
        for (int t = 0; t < l && j < nb; ++t, ++j) same = same && w[j] == x[t];
        c = nx;
      }
      if (same) return e;
    }
    s = (s + 1) & T.mask;
  }
}

// uni_word from the output code point at ws (word text); *end: the separator behind the word, or
// the end of the document.
TB_HD int64_t unim_word(const DevUni& T, const uint8_t* b, int64_t n, UniCur ws, UniCur* end, const UniRing& R) {
  const int nr = T.longest_cp + 1;
  for (int i = 0; i < nr; ++i) R.m[i * R.stride] = kUniNone;
  double best = 0.0;
  uint32_t meta = 0;
  int slot = 0;
  UniCur p = ws;
  bool lead = true;
  for (;;) {
    uint64_t h = 0;
    int nb = 0, k = 0, first = 0;
    UniCur q = p, p1 = p;  // p1: behind the node's first code point
    bool single = false;
    int ts = slot;
    if (lead) {
      for (int j = 0; j < T.sp_len; ++j) h = wp_push(h, uni_sp_byte(T, j));
      nb = first = T.sp_len;
    }
    for (;;) {
      if (!(lead && k == 0)) {
        const uint8_t* x;
        int l;
        UniCur nx;
        const int c = unim_next(T, b, n, &q, &x, &l, &nx);
        if (c < 0) return -1;
        if (c == UNI_SPACE) {
          if (k == 0) {
            *end = q;
            return (int64_t)(meta >> 1);
          }
          break;
        }
        if (k == 0) {
          first = l;
          p1 = nx;
        }
        if (nb + l > T.longest) break;
        for (int j = 0; j < l; ++j) h = wp_push(h, x[j]);
        nb += l;
        q = nx;
      }
      ++k;
      ts = ts + 1 == nr ? 0 : ts + 1;
      const UniSlot* e = unim_find(T, b, n, p, lead, h, nb);
      if (e != nullptr) {
        // the raw text has no unk text (uni_has_added): a replacement spelled it
        if ((e->val >> 31) & 1) return -1;
        uni_propose(R, ts, uni_score(e) + best, ((meta >> 1) + 1) << 1);
        single = single || k == 1;
      }
      if (k >= T.longest_cp) break;
    }
    slot = slot + 1 == nr ? 0 : slot + 1;
    if (!single) {
      const uint32_t add = (T.flags & kUniByteFallback) ? (uint32_t)first : !(meta & 1);
      uni_propose(R, slot, T.unk_score + best, (((meta >> 1) + add) << 1) | 1);
    }
    if (!lead) p = p1;
    lead = false;
    best = R.s[slot * R.stride];
    meta = R.m[slot * R.stride];
    R.m[slot * R.stride] = kUniNone;
    if ((meta >> 1) > kUniMaxCount) return -1;
  }
}

// uni_count_range: tokens of the words whose first output code point comes from an input code
// point that begins in [s0, s1).
TB_HD int64_t unim_count_range(const DevUni& T, const uint8_t* b, int64_t n, int64_t s0, int64_t s1,
                               const UniRing& R) {
  int64_t p = s0;
  bool inword = false;  // the nearest output code point before p is word text
  if (p > 0) {
    if ((b[p] & 0xC0) == 0x80) {  // inside a code point that starts in the range before
      const int64_t q = wp_back(b, p + 1, 0);
      int l;
      if (bpe_decode(b, q, n, &l) < 0 || q + l <= p) return -1;
      p = q + l;
    }
    for (int64_t e = p; e > 0;) {  // back over dropped code points
      const int64_t q = wp_back(b, e, 0);
      int il, ol;
      const uint8_t* s;
      const int k = unim_in(T, b, q, n, &il, &s, &ol);
      if (k < 0 || q + il != e) return -1;
      if (k == UNI_SPACE) break;
      if (ol > 0) {
        inword = s[ol - 1] != 0x20;
        break;
      }
      e = q;
    }
  }
  const int64_t stop = s1 < n ? s1 : n;
  UniCur c{p, 0};
  int64_t total = 0;
  for (;;) {
    const uint8_t* x;
    int l;
    UniCur nx;
    const int k = unim_next(T, b, n, &c, &x, &l, &nx);
    if (k < 0) return -1;
    if (c.i >= stop) return total;
    if (k == UNI_SPACE || inword) {
      inword = k != UNI_SPACE;
      c = nx;
      continue;
    }
    const int64_t w = unim_word(T, b, n, c, &c, R);  // ends at a separator, or at n
    if (w < 0) return -1;
    total += w;
  }
}

TB_HD int32_t unim_count_doc(const DevUni& T, const uint8_t* b, int64_t n, const UniRing& R) {
  if (T.n_added && uni_has_added(T, b, n, 0, n)) return kBpeHost;
  const int64_t k = n > 0 ? unim_count_range(T, b, n, 0, n, R) : 0;
  if (k < 0 || k + T.post_add > 0x7FFFFFFF) return kBpeHost;
  return (int32_t)(k + T.post_add);
}

#ifndef __HIP_DEVICE_COMPILE__
// Fills the free slots[0 .. mask] (val = kWpEmpty, mask + 1 >= 2 n a power of two) with the n
// distinct pieces pool[off[i] .. off[i + 1]) of score[i]; unk: the index of the unk piece.
inline void uni_fill_slots(const uint8_t* pool, const int64_t* off, const double* score, size_t n, size_t unk,
                           UniSlot* slots, uint64_t mask) {
  for (size_t i = 0; i < n; ++i) {
    const uint32_t nb = (uint32_t)(off[i + 1] - off[i]);
    uint64_t h = 0;
    for (uint32_t j = 0; j < nb; ++j) h = wp_push(h, pool[off[i] + j]);
    const uint64_t key = wp_key(h, nb, 0);
    uint64_t s = (uint32_t)key & mask;
    while (slots[s].val != kWpEmpty) s = (s + 1) & mask;
    slots[s].key = key;
    slots[s].val = wp_val((uint64_t)off[i], nb, i == unk);
    static_assert(sizeof(double) == sizeof(uint64_t), "f64 scores");
    __builtin_memcpy(&slots[s].score, &score[i], 8);
  }
}
#endif

}  // namespace tb
