"""Documents shared by the WordPiece token-counter tests (tests/test_wordpiece.py on the host
emulation, tests/test_gpu_wordpiece.py on k_wp_count)."""
import random

from adversarial import adversarial_corpus

from textblaster_amd.utils import synth

# what BertNormalizer / BertPreTokenizer join, drop, turn into a space or isolate, and text the
# lowercase / strip_accents normalisation changes
POOL = ["a", "b", "the", "ing", "Word", " ", "  ", "\n", "\t", "\r\n", "\u00a0", "\u2028", "\u3000",
        "\u0085", "\u00ad", "\u200b", "\ue000", "\u180e", "\x1c", "\x00", "\ufffd", "\u0378", "_", "$", "-",
        "\u2014", "!", "?", "...", "don't", "\u4f60", "\u65e5\u672c", "\U00020000", "\u00e9", "e\u0301", "\u0301",
        "\u0308a", "\U0001F600", "\u00df", "\ufb01", "\u0663", "\u0130", "\u03a3", "1", "42", "\u00e6\u00f8\u00e5"]

ASCII_POOL = [p for p in POOL if p.isascii()]


def fuzz(n, seed, pool=POOL):
    rng = random.Random(seed)
    return ["".join(rng.choice(pool) for _ in range(rng.randint(0, 40))) for _ in range(n)]


def big_doc(nbytes, seed):
    out, size = [], 0
    for t in synth.make_corpus(4 * nbytes // 1024 + 8, 1024, seed=seed):
        out.append(t)
        size += len(t.encode("utf-8")) + 1
        if size >= nbytes:
            break
    return "\n".join(out)


def edge_docs(known_word):
    return ["", " ", "a" * 100, "a" * 101, "\u00e9" * 100, "\u00e9" * 101, "x" * 5000, "!" * 300,
            known_word + "\u0378", "[CLS] hi [MASK]", big_doc(300 * 1024, 31)]


ADDED_DOC = "[CLS] hi [MASK]"


def corpus(known_word):
    return (synth.make_corpus(1500, 1024, seed=3) + synth.make_corpus(400, 1024, seed=4, vocab="zipf")
            + adversarial_corpus() + fuzz(3000, 5) + edge_docs(known_word))


def ascii_corpus():
    base = synth.make_corpus(600, 1024, seed=6, vocab="zipf") + fuzz(1500, 7, ASCII_POOL)
    return [t for t in base if t.isascii()] + ["", "HELLO World", "A" * 101, "x" * 5000]
