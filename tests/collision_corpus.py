"""Constructed 64-bit collisions of the two string hashes, the documents that carry them to every
exact-equality hash site, and a string-set reference of the record fields those sites feed.

Two collision families, built with no hooks and no search:

* polynomial hash (csrc/common/hash.h, H(s) = sum (s_i + 1) B^(|s|-1-i) mod 2^64): the Thue-Morse
  word of length 2^10 over two byte values and its complement. Their difference is
  +-(a - b) prod_{j<10} (1 - B^(2^j)), whose 2-adic valuation is at least 64 for every odd B;
* XOR-rotate concatenation hash (csrc/hip/gr_ngrams.hip, H(s) = XOR rotl(T[s_i], 5 (|s|-1-i)) with the
  rotation taken mod 64): two strings that differ by exchanging two bytes 64 positions apart.

The pure-Python mirrors of both hashes below only prove that the pairs collide and that the control
twins do not; the reference computes every expected number from Python strings, sets and dicts.

Every document is ASCII letters, single spaces and '\\n', so its words are ``line.split()`` and
UAX#29 plays no part."""
import functools
import re

M64 = (1 << 64) - 1
HASH_BASE = 0x9E3779B97F4A7C15
DOC_NEEDS_CPU = 1
SLOT64_WORDS = 65535  # canonicalize_res: tables of this many elements and more have 64-bit slots


# ---- mirrors of the two hashes ------------------------------------------------------------------

def hash_bytes(s: bytes) -> int:
    """hash.h hash_bytes."""
    h = 0
    for c in s:
        h = (h * HASH_BASE + c + 1) & M64
    return h


def _mix32(x: int) -> int:
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


NG_ROT = 5
NG_TABLE = [(_mix32(2 * c + 1) << 32) | _mix32(2 * c + 0x9E3779B2) for c in range(256)]


def _rotl(x: int, r: int) -> int:
    r &= 63
    return ((x << r) | (x >> ((64 - r) & 63))) & M64


def ng_hash(s: bytes) -> int:
    """gr_ngrams.hip: the concatenation hash of ng_build (h = rotl(h, kNgRot) ^ T[c] per byte)."""
    h = 0
    for c in s:
        h = _rotl(h, NG_ROT) ^ NG_TABLE[c]
    return h


# ---- collision builders -------------------------------------------------------------------------

def tm_pair(k: int = 10, a: bytes = b"a", b: bytes = b"b"):
    """The Thue-Morse word of length 2^k over the bytes a, b and its complement."""
    t = bytes(a[0] if bin(i).count("1") % 2 == 0 else b[0] for i in range(1 << k))
    c = bytes(b[0] if v == a[0] else a[0] for v in t)
    return t, c


def swap64_pair(s: bytes, i: int):
    """s and s with its bytes i and i + 64 exchanged."""
    assert s[i] != s[i + 64]
    t = bytearray(s)
    t[i], t[i + 64] = t[i + 64], t[i]
    return bytes(s), bytes(t)


def one_letter_changed(s: bytes, i: int) -> bytes:
    """The control twin's partner: same length, unequal, no collision (asserted by the CPU suite)."""
    t = bytearray(s)
    t[i] = ord("z") if t[i] != ord("z") else ord("y")
    return bytes(t)


T, TC = (x.decode() for x in tm_pair())
TZ = one_letter_changed(T.encode(), 517).decode()  # twin partner of T in place of TC

_XBASE = "".join("cdefghijklmnopqrstuvw"[(7 * i + i // 5) % 21] for i in range(70))
X, XS = (x.decode() for x in swap64_pair(_XBASE.encode(), 3))  # a 70-byte word and its swap
XZ = one_letter_changed(X.encode(), 67).decode()


def cut(s: str, n: int):
    """s cut into n words (the last takes the rest)."""
    k = len(s) // n
    return [s[i * k:(i + 1) * k] for i in range(n - 1)] + [s[(n - 1) * k:]]


# polynomial gram collision: five words that concatenate to T / TC / TZ
T5, TC5, TZ5 = cut(T, 5), cut(TC, 5), cut(TZ, 5)
# XOR-rotate gram collision: ten 7-byte words, and the same ten with bytes 0 and 64 of their
# concatenation exchanged (word 0's first byte, word 9's second byte)
_G10 = "".join("bcdfghjklmnpqrstvwxyz"[(5 * i + i // 7) % 21] for i in range(70))
G10 = cut(_G10, 10)
G10S = cut(swap64_pair(_G10.encode(), 0)[1].decode(), 10)
G10Z = cut(one_letter_changed(_G10.encode(), 64).decode(), 10)


def filler(n: int, start: int = 0, width: int = 4):
    """n words that never repeat: a base-26 counter in upper case (no other word has capitals)."""
    out = []
    for i in range(start, start + n):
        w = ""
        for _ in range(width):
            w = chr(ord("A") + i % 26) + w
            i //= 26
        assert i == 0
        out.append(w)
    return out


def filler2(n: int):
    """n two-letter words (they repeat after 676): the cheapest way to many words."""
    return [chr(ord("A") + (i // 26) % 26) + chr(ord("A") + i % 26) for i in range(n)]


# ---- string-set reference -----------------------------------------------------------------------

def ref_top(words, n):
    """find_top_duplicate over the space-joined n-grams (reference utils/text.rs)."""
    if n == 0 or len(words) < n:
        return 0
    cnt = {}
    for i in range(len(words) - n + 1):
        g = " ".join(words[i:i + n])
        cnt[g] = cnt.get(g, 0) + 1
    m = max(cnt.values())
    return 0 if m <= 1 else max(len(g.encode()) * m for g, c in cnt.items() if c == m)


def ref_all_dup(words, n):
    """find_all_duplicate: the greedy walk over the concatenated n-grams."""
    if n == 0 or len(words) < n:
        return 0
    seen, rep, i = set(), 0, 0
    while i + n <= len(words):
        g = "".join(words[i:i + n])
        if g in seen:
            rep += len(g.encode())
            i += n
        else:
            seen.add(g)
            i += 1
    return rep


def ref_duplicates(items):
    """find_duplicates: (number, bytes) of the items seen before."""
    seen, k, nb = set(), 0, 0
    for it in items:
        if it in seen:
            k += 1
            nb += len(it.encode())
        else:
            seen.add(it)
    return k, nb


def ref_gopher_rep(text, top_ns, dup_ns):
    """The GopherRepetition record (gopher_rep_record's r[0..6], then top orders, then duplicated)."""
    return list(_ref_gopher_rep(text, tuple(top_ns), tuple(dup_ns)))


@functools.lru_cache(maxsize=None)
def _ref_gopher_rep(text, top_ns, dup_ns):
    t = text.strip()
    paras = re.split(r"\n{2,}", t)
    lines = re.split(r"\n+", t)
    words = text.split()
    pd, pb = ref_duplicates(paras)
    ld, lb = ref_duplicates(lines)
    return ([len(t), len(paras), pd, pb, len(lines), ld, lb] + [ref_top(words, n) for n in top_ns] +
            [ref_all_dup(words, n) for n in dup_ns])


def ref_fineweb(text, stop_chars, short_line_length):
    """The FineWebQuality record: non-blank lines, lines ending in a stop character, short lines,
    duplicated line bytes, characters that are no line feed, line feeds, words."""
    lines = [ln for ln in text.split("\n") if ln.strip()]
    ends = sum(1 for ln in lines if ln.rstrip()[-1] in stop_chars)
    short = sum(1 for ln in lines if len(ln) <= short_line_length)
    nl = text.count("\n")
    return [len(lines), ends, short, ref_duplicates(lines)[1], len(text) - nl, nl, len(text.split())]


# ---- named documents ----------------------------------------------------------------------------

class Doc:
    """text, the route it is built for, the flag the device must raise (flag) and the flag of the
    host emulation (emu_flag: it has no pre-pass, so it verifies where k_pre_wcanon cannot)."""

    def __init__(self, text, route, flag=0, emu_flag=None):
        self.text, self.route, self.flag = text, route, flag
        self.emu_flag = flag if emu_flag is None else emu_flag


def _w(a, b):
    """W: two words with one hash, each alone and then again, around one filler word: every top
    and duplicated order depends on telling them apart."""
    f = filler(12)
    return " ".join([a, f[0], b, f[0], a, f[0], b] + f[1:])


def _w_short(a, b):
    """W for documents with room for three long words: a, b, a, each before the same four words, so
    the 5-grams (a f f f f) and (b f f f f) collide as well and only the first repeats."""
    f = filler(16)
    return " ".join([a] + f[:4] + [f[4], b] + f[:4] + [f[5], a] + f[:4] + f[6:])


def _g(ga, gb):
    """G: two n-grams of different words with one concatenation hash; the first repeats. A trusted
    hash would count the second as a repeat too."""
    f = filler(40)
    return " ".join(ga + f[:1] + gb + f[1:2] + ga + f[2:])


def _l(a, b):
    """L: single-word paragraphs a, b, a (lines as well), then a paragraph of three lines."""
    f = filler(8)
    return "\n\n".join([a, b, a, f[0]]) + "\n" + f[1] + "\n" + " ".join(f[2:])


def _pad(text, nwords=0, nbytes=0, width=4):
    """text followed by a line of filler that brings it to at least nwords words / nbytes bytes
    (width 2: two-letter words, which repeat; wider ones never do)."""
    need = max(nwords - len(text.split()), (nbytes - len(text) + width) // (width + 1), 0)
    pad = filler2(need) if width == 2 else filler(need, 1000, width)
    return text + ("\n" + " ".join(pad) if pad else "")


def _twins(name, build, a, b, bz, route, flag=0, emu_flag=None, **pad):
    """The colliding document and its control twin (partner b replaced by the non-colliding bz)."""
    return {name: Doc(_pad(build(a, b), **pad), route, flag, emu_flag),
            name + "_twin": Doc(_pad(build(a, bz), **pad), route)}


# a word of 9..64 bytes next to the 70-byte colliding words and the <= 8-byte packed keys of ng_build
MID = "midlengthwordofthirtytwobytesxyz"


def _xw(a, b):
    f = filler(12)
    return " ".join([a, f[0], b, f[0], a, f[0], b, MID, "tiny", MID, "tiny"] + f[1:])


def default_documents():
    """Documents of the default operating points. Routes:
    ng256 / ng512 / ng1024  the k_gr_ngrams classes (XOR-rotate W and G)
    ng512 (wave_*)           one-wave documents with 1 KB words: the in-stage n-grams (WavePar
                             canonicalize) of two GopherRepetition steps, polynomial W and G
    blk                      4-32 KB workgroup documents (polynomial W, G, L)
    blk_part                 a workgroup document whose word table is cut into LDS parts
    split                    documents over split_doc_bytes (k_gr_dup_split; W, G, L)
    slot64                   at least 65,535 words: 64-bit slots, W flags DOC_NEEDS_CPU"""
    d = {}
    d.update(_twins("ng256_W", _xw, X, XS, XZ, "ng256"))
    d.update(_twins("ng256_G", _g, G10, G10S, G10Z, "ng256"))
    d.update(_twins("ng512_W", _xw, X, XS, XZ, "ng512", nbytes=1500))
    d.update(_twins("ng512_G", _g, G10, G10S, G10Z, "ng512", nbytes=1500))
    d.update(_twins("ng1024_W", _xw, X, XS, XZ, "ng1024", nwords=700, width=3))
    d.update(_twins("ng1024_G", _g, G10, G10S, G10Z, "ng1024", nwords=700, width=3))
    d.update(_twins("wave_W", _w_short, T, TC, TZ, "ng512"))
    d.update(_twins("wave_G", _g, T5, TC5, TZ5, "ng512"))
    d.update(_twins("wave_L", _l, T, TC, TZ, "ng512"))
    d.update(_twins("blk_W", _w, T, TC, TZ, "blk", nbytes=4200))
    d.update(_twins("blk_G", _g, T5, TC5, TZ5, "blk", nbytes=4200))
    d.update(_twins("blk_L", _l, T, TC, TZ, "blk", nbytes=4200))
    d.update(_twins("blk_part_W", _w, T, TC, TZ, "blk_part", nwords=8300, width=2))
    d.update(_twins("split_W", _w, T, TC, TZ, "split", nbytes=34000))
    d.update(_twins("split_G", _g, T5, TC5, TZ5, "split", nbytes=34000))
    d.update(_twins("split_L", _l, T, TC, TZ, "split", nbytes=34000))
    d.update(_twins("slot64_W", _w, T, TC, TZ, "slot64", nwords=SLOT64_WORDS + 40, width=2, flag=DOC_NEEDS_CPU))
    return d


def rest_documents():
    """One-wave documents of more than 1024 words (long_doc_bytes raised to 8 KB so that 1 KB words
    fit): k_gr_words + k_gr_ngrams_rest, polynomial W and G."""
    d = {}
    d.update(_twins("rest_W", _w_short, T, TC, TZ, "rest", nwords=1100, width=3))
    d.update(_twins("rest_G", _g, T5, TC5, TZ5, "rest", nwords=1100, width=3))
    return d


def pre_documents():
    """Pre-pass documents (pre_doc_bytes=65536): k_pre_wcanon joins words on a fingerprint and can
    only flag a collision; the emulation has no pre-pass and verifies inline instead."""
    d = {}
    d.update(_twins("pre_W", _w, T, TC, TZ, "pre", nbytes=70000, flag=DOC_NEEDS_CPU, emu_flag=0))
    d["pre_small"] = Doc(_pad(_w(T, TC), nbytes=4200), "blk")
    return d


def route_of(runner, text):
    """The route a document takes, from the runner's own thresholds."""
    words = text.split()
    n, nw = len(text.encode()), len(words)
    span = text.rindex(words[-1]) + len(words[-1]) - text.index(words[0])
    if runner.pre_doc_bytes > 0 and n >= runner.pre_doc_bytes:
        return "pre"
    if n > runner.long_doc_bytes:
        if nw >= SLOT64_WORDS:
            assert n > runner.split_doc_bytes
            return "slot64"
        if n > runner.split_doc_bytes > 0:
            return "split"
        # the word table (1.5 W + 2 slots of 4 bytes) exceeds the whole LDS slice: LDS parts
        return "blk_part" if 4 * (nw + nw // 2 + 2) > runner.lds_bytes_blk else "blk"
    # the k_gr_ngrams classes (gr_ngrams.hip: 256 words / 2 KB of text up to ngram_big_bytes, 512
    # words / 4 KB above, what fits neither 1024 words / 4 KB, the rest the generic code)
    if n <= runner.ngram_big_bytes and nw <= 256 and span <= 2048:
        return "ng256"
    if n > runner.ngram_big_bytes and nw <= 512 and span <= 4096:
        return "ng512"
    return "ng1024" if nw <= 1024 and span <= 4096 else "rest"


def stop_word_case():
    """GopherQuality with the colliding pair as its stop words: documents with T, with its partner,
    with neither."""
    f = " ".join(filler(30))
    return [T + " " + f, TC + " " + f, f]
