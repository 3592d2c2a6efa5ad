"""Documents for the tests of the case-aware split patterns and the NFC gate (tests/test_bpe_case.py
on the host emulation, tests/test_gpu_bpe_case.py on the kernels): bpe_split_corpus's sets, a fuzz
pool extended with the code points the case classes turn on, the table of cases the rules were
written from, and a unit string that holds every rule of pattern C once."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bpe_split_corpus as bc  # noqa: E402

ADDED, EDGES, HOST_DOCS = bc.ADDED, bc.EDGES, bc.HOST_DOCS
# '/', a titlecase letter, a letter without case, a modifier letter, a combining mark, a capital
# whose lower case is two code points, and runs in either case
POOL = bc.POOL + ["/", "ǅ", "あ", "ʰ", "́", "İ", "ABC", "abc", "Ab", "DEF", "gh", "A", "b",
                  "'LL", "'s"]

# (text, pieces of pattern C in the library)
CASES = [
    ("AあB", ["Aあ", "B"]),
    ("あAあB", ["あAあ", "B"]),
    ("ABC", ["ABC"]),
    ("!ABC", ["!ABC"]),
    ("AbcDEFgh", ["Abc", "DEFgh"]),
    ("DON'T'S", ["DON'T", "'S"]),
    ("a'r!", ["a", "'r", "!"]),
    ("it'ſ x", ["it'ſ", " x"]),
    ("ab́'ll", ["ab́'ll"]),
    ("́abc", ["́abc"]),
    ("1́", ["1", "́"]),
    ("!\n/\nx", ["!\n/\n", "x"]),
    ("\n/x", ["\n", "/x"]),
    ("a/b", ["a", "/b"]),
    ("  \n  a", ["  \n", " ", " a"]),
    # a mark after one punctuation mark starts a letter run behind it; after two it joins them
    ("!́a", ["!́a"]),
    ("!!́a", ["!!́", "a"]),
    ("́ABC", ["́", "ABC"]),
]

# every rule of C once, to be cut at every byte: a case boundary, a run given back to a caseless
# letter, a contraction as a suffix in upper case, a space-led number run cut in threes, a
# punctuation run that swallows "/" and newlines, a mark-led word, newlines inside whitespace,
# U+00A0 leading a word, U+017F closing a contraction
UNIT = "AbcDEF gh AあB DON'T 12345 !x,\n/\n ́ab\n\n  dé, e it'ſ "


def fuzz(n, seed):
    rng = random.Random(seed)
    return ["".join(rng.choice(POOL) for _ in range(rng.randint(0, 40))) for _ in range(n)]


def prefixes():
    """Every prefix of 0 to 130 bytes of the unit string repeated that ends at a code point."""
    b = (UNIT * 3).encode("utf-8")
    out = []
    for k in range(131):
        try:
            out.append(b[:k].decode("utf-8"))
        except UnicodeDecodeError:
            pass
    return out


def base_corpus():
    return bc.base_corpus()


def corpus():
    """(documents, indices of the ones built to come back -2 whatever the normalizer)."""
    docs = (base_corpus() + bc.fuzz(1500, 5) + fuzz(3000, 6) + EDGES + bc.prefixes() + prefixes()
            + [t for t, _ in CASES])
    host = list(range(len(docs), len(docs) + len(HOST_DOCS)))
    return docs + HOST_DOCS, host


# short samples in NFC that the gate must let through: Thai, Hebrew with points, Arabic with harakat,
# Vietnamese, Korean
NFC_CLEAN = [
    "ภาษาไทย น้ำ ที่นี่",
    "\u05e9\u05b8\u05c1\u05dc\u05d5\u05b9\u05dd \u05e2\u05b2\u05dc\u05b5\u05d9\u05db\u05b6\u05dd",  # shalom aleichem, pointed
    "مَرْحَبًا بِالْعَالَمِ",
    "Tiếng Việt rất đẹp",
    "한국어 텍스트",
]
