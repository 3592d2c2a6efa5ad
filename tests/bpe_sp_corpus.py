"""Documents for the tests of the SentencePiece-style BPE counter (tests/test_bpe_sp.py on the host
emulation, tests/test_gpu_bpe_sp.py on the kernels): the tokenizer variants, the synthetic corpora,
fuzz text over what the layouts treat specially, the edge documents around the merge arrays' sizes,
and the rule, stated in Python, for which documents the counter hands to the host tokenizer."""
import os
import re
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from textblaster_amd.models.tokenizer import (SP_PREPEND_ALWAYS, SP_PREPEND_NONE,  # noqa: E402
                                              SP_PREPEND_UNLESS_SPACE, train_synthetic_sp_bpe)
from textblaster_amd.utils import synth  # noqa: E402

SP = "▁"
ADDED = ["<unk>", "<s>", "</s>"]
MAX_WORD, MAX_LONG = 64, 2048  # csrc/common/bpe.h kBpeMaxWord, kBpeMaxLong

# name -> (arguments of train_synthetic_sp_bpe, the spec's sp_prepend, sp_split)
VARIANTS = {
    "L-prepend": (dict(layout="L"), SP_PREPEND_ALWAYS, False),
    "L-plain": (dict(layout="L", prepend=False), SP_PREPEND_NONE, False),
    "M-always-split": (dict(layout="M", prepend_scheme="always", split=True), SP_PREPEND_UNLESS_SPACE, True),
    "M-first-split": (dict(layout="M", prepend_scheme="first", split=True), SP_PREPEND_UNLESS_SPACE, True),
    "M-first-whole": (dict(layout="M", prepend_scheme="first", split=False), SP_PREPEND_UNLESS_SPACE, False),
    "M-never-split": (dict(layout="M", prepend_scheme="never", split=True), SP_PREPEND_NONE, True),
}


def tokenizer(tok_dir, name):
    """The 4,000-entry file of the variant (one training run each per directory)."""
    return train_synthetic_sp_bpe(os.path.join(str(tok_dir), f"sp4k_{name}.json"), vocab_size=4000, n_docs=1500,
                                  seed=2, **VARIANTS[name][0])


# spaces and runs of them, other whitespace, Latin-1 (two bytes, in no vocabulary trained here), CJK,
# a 4-byte emoji the training corpus does not hold, a literal U+2581 alone, doubled and next to a
# space, combining marks, a capital, a digit run, pieces of the added tokens, and characters of two,
# three and four bytes that the training corpus does hold (IN_VOCAB: one symbol each)
EMOJI = "\U0001f980"
IN_VOCAB = ["ä", "…", "\U0001f600"]
POOL = IN_VOCAB + [" ", " ", " ", "  ", "   ", "\n", "\t", "é", "ü", "あ", "日本", EMOJI, SP, SP + SP,
        " " + SP, SP + " ", "́", "é", "the", "and", "a", "b", "ing", "Word", "1234", ".", ", ", "!", "<", "s>",
        "</", "unk"]


# every rule once, to be cut at every byte: words, a space run, a U+2581 next to a space, characters
# of two, three and four bytes outside the vocabulary, a combining mark, other whitespace
UNIT = "ab  cd " + SP + "é あ" + EMOJI + " " + SP + SP + "x\n\tý the "


def fuzz(n, seed):
    rng = random.Random(seed)
    return ["".join(rng.choice(POOL) for _ in range(rng.randint(0, 40))) for _ in range(n)]


def synthetic():
    """The part of which at most 2 % may go to the host."""
    return synth.make_corpus(1500, 1024, seed=3) + synth.make_corpus(400, 1024, seed=4, vocab="zipf")


def edge_docs():
    """Empty and one-space documents, a leading space and a leading U+2581 (Metaspace prepends in
    front of neither), and chunks of 62 to 65 and 2047 to 2049 bytes at offset 0, where a prepended
    symbol counts towards the merge arrays, and after a word."""
    out = ["", " ", SP, " a", SP + "a", "  a", " " + SP + "a", "a", "a ", "a" + SP, "é", EMOJI, "aあ" + EMOJI]
    out += ["".join(IN_VOCAB) * k + "q" for k in (1, 7, 8, 100)]  # a long chunk with fewer symbols than bytes
    for n in (62, 63, 64, 65, 2047, 2048, 2049):
        out += ["q" * n, "q" * n + " tail", "head " + "q" * (n - 1), " " + "q" * (n - 1), SP + "q" * (n - 3),
                "head" + " " * (n - 1) + "q", " " * n]
    return out


HOST_DOCS = ["b" * 2100, "</s>", "ab<s>cd", "x <unk>", "word " * 10 + "z" * 3000]
INVALID = [b"ab\xffcd", b"\xe2\x96", b"word \xe2\x96 word", b"\xc3", b"a\xed\xa0\x80", b"ok \xf0\x9f\xa6"]


def corpus():
    return synthetic() + fuzz(3000, 5) + edge_docs() + HOST_DOCS


def pack(docs):
    """synth.pack for documents given as str or as bytes."""
    enc = [d if isinstance(d, bytes) else d.encode("utf-8") for d in docs]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum([len(e) for e in enc], out=off[1:])
    return np.frombuffer(b"".join(enc) or b"", dtype=np.uint8).copy(), off


def chunks(text, split):
    """The pieces the counter merges on their own: with Metaspace's split one space (U+0020 or
    U+2581) and the characters up to the next; else a run of spaces and the characters after it."""
    return [m.group(0) for m in re.finditer(f"[ {SP}]?[^ {SP}]+|[ {SP}]" if split else f"[ {SP}]*[^ {SP}]+|[ {SP}]+\\Z",
                                            text)]


def lead(text, prepend):
    """1 when the layout puts a U+2581 in front of this text."""
    if not text or prepend == SP_PREPEND_NONE:
        return 0
    return 1 if prepend == SP_PREPEND_ALWAYS or text[0] not in (" ", SP) else 0


def to_host(doc, prepend, split):
    """The rule: a document goes to the host tokenizer when it is not UTF-8, holds the text of an
    added token, or has a chunk of more than 2048 bytes, the prepended symbol counted as one."""
    try:
        text = doc.decode("utf-8") if isinstance(doc, bytes) else doc
    except UnicodeDecodeError:
        return True
    if any(a in text for a in ADDED):
        return True
    ch = chunks(text, split)
    assert "".join(ch) == text
    return any(len(c.encode("utf-8")) + (lead(text, prepend) if k == 0 else 0) > MAX_LONG for k, c in enumerate(ch))
