"""Tokenizers and documents shared by the folding WordPiece counter's tests (tests/
test_wordpiece_fold.py on the host emulation, tests/test_gpu_wordpiece_fold.py on k_wp_count_fold)."""
import json
import os
import random
import unicodedata

from textblaster_amd.utils import synth

LVT, LV = "\uac01", "\uac00"  # U+AC01 (3 jamo), U+AC00 (2 jamo)

# the smallest inputs at which each piece of the folding logic can go wrong
POOL = [
    "e\u0301x", "a\u0301\u00ad\u0301b",             # a stripped mark, then a drop, before the next letter
    "\u0301\u0308\u0301", "x \u0301\u0308 y", "\u0301",  # words that are only marks
    LV + LVT, LV, LVT, "a" + LV + "b", LVT + LV + "x",  # piece boundaries inside a syllable
    "\u0130stanbul", "a\u0130", "\u0130", "\u0130\u0130 \u0130",  # lower-only: i + U+0307
    "x\u037ey", "a\u2260b", "\u1fef", "a\u1fefb", "a\u226eb\u226fc",  # the class comes from the output
    LVT * 33, LVT * 34, "x" + LVT * 33, LV * 50, LV * 51,  # 99 / 102 / 100 / 100 / 102 output characters
    "\u00e9" * 100, "\u00e9" * 101,
    "\u212b", "\u212bngstr\u00f6m", "\u00c5re \u00c6r\u00f8 \u00d8l \u00c4\u00d6\u00e4\u00f6\u00e5",
    "\u304c", "\u304c\u304f\u3076", "\u0e01\u0e48\u0e32\u0e19 \u0e19\u0e49\u0e33 \u0e17\u0e35\u0e48",
    "\u0391\u0392\u0393 \u03a3\u039f\u03a6\u039f\u03a3 \u0386\u03c2", "\u1e9e \ufb01 \u01c5 \u0149",
    "\uf900 a\uf900b \U0002f800", " a ", "\ub098\ub77c", "\ud55c\uad6d\uc5b4 \ub9d0",  # syllables the trainer never saw
] + ["x" * k + LVT * 8 for k in range(9)]  # the longest candidate is cut inside a syllable for some k

# U+302E (combining class 224, not Mn) survives strip_accents and NFD may move it: host in the
# strip modes, native in lower-only
CONTEXT = ["a\u302eb", "\u1b44", "x\U0001d15ey"]


def pool_docs():
    base = POOL + CONTEXT
    return base + [t + "[MASK]" for t in base] + ["[CLS]" + t for t in base]


def needs_host(strip, path):
    """doc -> bool: it holds the text of an added token of the tokenizer file, or (strip modes) a code
    point whose NFD holds
    one with a non-zero combining class that is not a nonspacing mark."""
    with open(path, encoding="utf-8") as f:
        added = [a["content"] for a in json.load(f).get("added_tokens") or []]
    memo = {}

    def ctx(c):
        if c not in memo:
            memo[c] = any(unicodedata.combining(x) and unicodedata.category(x) != "Mn"
                          for x in unicodedata.normalize("NFD", c))
        return memo[c]

    return lambda t: any(a in t for a in added) or (strip and any(ctx(c) for c in set(t) if ord(c) >= 128))


def training_extras(seed=5):
    """Danish and Swedish letters, accented Latin, Greek capitals, Hangul words and U+0130 for the
    trainer, so that non-ASCII pieces enter the vocabulary."""
    rng = random.Random(seed)
    syll = [chr(0xAC00 + rng.randrange(11172)) for _ in range(40)] + [LV, LVT]
    hangul = ["".join(rng.choice(syll) for _ in range(rng.randint(1, 4))) for _ in range(300)]
    latin = ["\u00c5rhus", "\u00c6bler\u00f8d", "\u00d8ster", "sm\u00f6rg\u00e5s", "\u00c4lv", "\u00d6l",
             "caf\u00e9", "na\u00efve", "\u00fcber", "\u0130stanbul", "fa\u00e7ade", "\u00d1and\u00fa",
             "\u0141\u00f3d\u017a", "\u0391\u0398\u0397\u039d\u0391", "\u03a3\u039f\u03a6\u0399\u0391",
             "\u039b\u039f\u0393\u039f\u03a3", "\u304c\u304f", "\u00e9t\u00e9"]
    return [" ".join(rng.choice(hangul if rng.random() < 0.5 else latin) for _ in range(30)) for _ in range(200)]


def train(path, lowercase, strip_accents):
    """A 4,000-entry BERT-format tokenizer with the given normalizer settings (kept if present)."""
    if os.path.isfile(path):
        return path
    from tokenizers import Tokenizer, decoders, models, normalizers, pre_tokenizers, processors, trainers

    texts = synth.make_corpus(1500, 1024, seed=2, vocab="zipf") + training_extras()
    tok = Tokenizer(models.WordPiece(unk_token="[UNK]"))
    tok.normalizer = normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True,
                                                strip_accents=strip_accents, lowercase=lowercase)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tok.decoder = decoders.WordPiece(prefix="##")
    special = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    tok.train_from_iterator(texts, trainers.WordPieceTrainer(vocab_size=4000, special_tokens=special,
                                                             show_progress=False))
    tok.post_processor = processors.TemplateProcessing(
        single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
        special_tokens=[("[CLS]", tok.token_to_id("[CLS]")), ("[SEP]", tok.token_to_id("[SEP]"))])
    tok.save(path)
    return path


def variant(path, out, **normalizer):
    """The tokenizer file with other normalizer settings."""
    with open(path, encoding="utf-8") as f:
        tj = json.load(f)
    tj["normalizer"].update(normalizer)
    with open(out, "w", encoding="utf-8") as f:
        json.dump(tj, f)
    return out


def splits_a_syllable(tok):
    """Does the vocabulary hold a piece that ends between the jamo of a syllable, and does the
    tokenizer use one on the pool's unseen Hangul words (a piece that begins with a vowel or a
    trailing consonant: the piece before it ended inside the syllable)?"""
    vocab = tok.get_vocab()
    in_vocab = any(0x1100 <= ord(p[-1]) <= 0x115F for p in vocab if not p.startswith("["))
    toks = tok.encode("\ub098\ub77c \ud55c\uad6d\uc5b4", add_special_tokens=False).tokens
    used = any(t.startswith("##") and 0x1161 <= ord(t[2]) <= 0x11FF for t in toks)
    return in_vocab and used
