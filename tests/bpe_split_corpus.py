"""Documents for the split-regex BPE counter's tests (tests/test_bpe_split.py on the host
emulation, tests/test_gpu_bpe_split.py on the kernels): the synthetic corpora, the adversarial pool,
fuzz text over the corner cases of patterns A and B, the edge documents, and the documents built
to go to the host tokenizer (an added token's text, a pre-token over 2048 bytes)."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adversarial import adversarial_corpus  # noqa: E402
from test_bpe import POOL as GPT2_POOL  # noqa: E402

from textblaster_amd.utils import synth  # noqa: E402

ADDED = "<|reserved_special_token_7|>"
POOL = GPT2_POOL + ["\r", "\r\n", "\u00a0", "S", "VE", "\u017f", "\u212a", "1234567", "-", "_", "\u0301"]
EDGES = ["", "'", "12", "1234", "a" * 63, "a" * 64, "a" * 65, "x" * 200, "a" * 2048]
# built to come back -2: kept out of the host-share cap and asserted one by one
HOST_DOCS = ["b" * 2049, ADDED, "ab" + ADDED + "cd"]

# every rule once, to be cut at every byte: letters, a space-led number run cut in threes, a
# contraction in upper case, a punctuation-led word, newlines inside whitespace, a two-byte letter,
# U+00A0 leading a word, U+017F
UNIT = "ab 12345 c'LL !x\n\n  d\u00e9,\u00a0e \u017f "


def fuzz(n, seed):
    rng = random.Random(seed)
    return ["".join(rng.choice(POOL) for _ in range(rng.randint(0, 40))) for _ in range(n)]


def prefixes():
    """Every prefix of 0 to 130 bytes of the unit string repeated that ends at a code point."""
    b = (UNIT * 5).encode("utf-8")
    out = []
    for k in range(131):
        try:
            out.append(b[:k].decode("utf-8"))
        except UnicodeDecodeError:
            pass
    return out


def base_corpus():
    """The three sets of which at most 1 % may go to the host."""
    return (synth.make_corpus(1500, 1024, seed=3) + synth.make_corpus(400, 1024, seed=4, vocab="zipf")
            + adversarial_corpus())


def corpus():
    """(documents, indices of the ones built to come back -2)."""
    docs = base_corpus() + fuzz(3000, 5) + EDGES + prefixes()
    host = list(range(len(docs), len(docs) + len(HOST_DOCS)))
    return docs + HOST_DOCS, host
