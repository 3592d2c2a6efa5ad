"""Trains a Unigram tokenizer with ``sentencepiece`` on the synthetic Zipf corpus and writes it as a
``tokenizer.json`` laid out like the T5 / mT5 / XLM-R files (models/tokenizer.py
train_synthetic_unigram): the offline stand-in for them, for ``bench.py --config
config/bench_pipeline_tokens.yaml --vocab zipf --tokenizer FILE`` and the CLI's ``--tokenizer-dir``.
No network is used.

    python tools/make_unigram_tokenizer.py OUT.json [--layout H|C] [--rule nmt_nfkc|nfkc|identity]
        [--byte-fallback] [--vocab-size 32000] [--prepend-scheme always|first] [--docs 20000] [--seed 1]
        [--check] [--mapped]

``--check`` verifies the class table the device counter gets for the file (models/tokenizer.py
unigram_classes) against the file's own normalizer and pre-tokenizer and prints the result: for every
code point x that is not of the host class, ``normalize_str("a" + x + "b")`` must be the
concatenation of what the normalizer makes of "a", x and "b" on their own, and random strings over
keep and space code points must be cut into the words the table predicts.

``--check --mapped`` does the same for the tables of the mapped spec (unigram_map: the replacements
the counter applies itself, TB_TUNE=uni_map=1): it prints their sizes, and random strings built from
keep, space and map code points, drops among them, must give the words that the records predict -
each map code point replaced by its record's bytes, the text cut at space code points and at 0x20.
"""
import argparse
import json
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def check(path: str, n_strings: int = 20000, seed: int = 1) -> int:
    import numpy as np
    from tokenizers import Tokenizer

    from textblaster_amd.models.tokenizer import (UNI_HOST, UNI_KEEP, UNI_SPACE, _unigram_layout, unigram_classes,
                                                  unigram_probe)

    with open(path, encoding="utf-8") as f:
        layout, charsmap = _unigram_layout(json.load(f))
    tok = Tokenizer.from_file(path)
    cls = unigram_classes(charsmap, layout)
    single = unigram_probe(charsmap)
    counts = {name: int((cls == k).sum()) for name, k in (("keep", UNI_KEEP), ("space", UNI_SPACE), ("host", UNI_HOST))}
    print(f"{path}: layout {layout}, charsmap {'none' if charsmap is None else f'{len(charsmap) * 3 // 4} bytes'}")
    print(f"classes over 1,114,112 code points: {counts}")
    print("space:", " ".join(f"U+{c:04X}" for c in np.nonzero(cls == UNI_SPACE)[0].tolist()))
    # 1. in context every non-host code point normalises as it does alone
    nz = tok.normalizer
    bad = []
    if charsmap is not None:
        import base64

        from tokenizers import normalizers

        pre = normalizers.Precompiled(base64.b64decode(charsmap)).normalize_str
        for c in np.nonzero(cls != UNI_HOST)[0].tolist():
            if pre("a" + chr(c) + "b") != single[0x61] + single[c] + single[0x62]:
                bad.append(c)
    print(f"context probe a+x+b over {counts['keep'] + counts['space']} non-host code points: {len(bad)} differ"
          + ("".join(f" U+{c:04X}" for c in bad[:20])))
    # 2. random strings over keep and space code points split into the predicted words
    rng = random.Random(seed)
    keep = np.nonzero(cls == UNI_KEEP)[0]
    space = np.nonzero(cls == UNI_SPACE)[0]
    common = [c for c in keep.tolist() if c < 0x3000]
    wrong = 0
    for _ in range(n_strings):
        s = "".join(chr(int(rng.choice(space)) if rng.random() < 0.3 else
                        (rng.choice(common) if rng.random() < 0.7 else int(rng.choice(keep))))
                    for _ in range(rng.randint(0, 24)))
        words, cur = [], ""
        for ch in s:
            if cls[ord(ch)] == UNI_SPACE:
                if cur:
                    words.append(cur)
                cur = ""
            else:
                cur += ch
        if cur:
            words.append(cur)
        pre = [w for w, _ in tok.pre_tokenizer.pre_tokenize_str(nz.normalize_str(s))]
        if pre != ["\u2581" + w for w in words]:
            wrong += 1
            if wrong <= 5:
                print("  split differs:", ascii(s), ascii(pre))
    print(f"word split of {n_strings} random strings over keep / space code points: {wrong} differ")
    return len(bad) + wrong


def check_mapped(path: str, n_strings: int = 20000, seed: int = 1) -> int:
    import numpy as np
    from tokenizers import Tokenizer

    from textblaster_amd.models.tokenizer import (UNI_KEEP, UNI_MAP, UNI_SPACE, _two_stage_map, _unigram_layout,
                                                  unigram_map)

    with open(path, encoding="utf-8") as f:
        layout, charsmap = _unigram_layout(json.load(f))
    tok = Tokenizer.from_file(path)
    cls, outputs, joins = unigram_map(charsmap, layout)
    map1, map2, rec, pool = _two_stage_map(outputs, joins)
    lens = [len(o) for o in outputs.values()]
    print(f"{path}: layout {layout}, mapped")
    print(f"map code points: {int((cls == UNI_MAP).sum())}, of them dropped: {sum(1 for n in lens if n == 0)}; "
          f"output bytes 1..{max(lens, default=0)}, with a separator: {sum(1 for o in outputs.values() if b' ' in o)}")
    print("space code points that join the grapheme before them:", " ".join(f"U+{c:04X}" for c in joins) or "none")
    print(f"tables: map1 {map1.nbytes} B, map2 {map2.nbytes} B ({len(map2) // 128} blocks), {len(rec)} records "
          f"{rec.nbytes} B, pool {pool.nbytes} B: {map1.nbytes + map2.nbytes + rec.nbytes + pool.nbytes} B in all")
    rng = random.Random(seed)
    keep = [c for c in np.nonzero(cls == UNI_KEEP)[0].tolist() if c < 0x3000]
    space = np.nonzero(cls == UNI_SPACE)[0].tolist()
    maps = sorted(c for c, o in outputs.items() if o)
    drops = sorted(c for c, o in outputs.items() if not o)
    nz = tok.normalizer
    wrong = to_host = 0
    for _ in range(n_strings):
        s = ""
        for _ in range(rng.randint(0, 24)):
            r = rng.random()
            kind = space if r < 0.2 else (maps if r < 0.55 and maps else (drops if r < 0.65 and drops else keep))
            s += chr(rng.choice(kind))
        if any(ord(a) in outputs and ord(b) in joins for a, b in zip(s, s[1:])):
            to_host += 1  # a map code point swallows the joiner: the counter does not count this one
            continue
        text = b"".join(b" " if cls[ord(ch)] == UNI_SPACE else outputs.get(ord(ch), ch.encode("utf-8")) for ch in s)
        words = ["\u2581" + w for w in text.decode("utf-8").split(" ") if w]
        got = [w for w, _ in tok.pre_tokenizer.pre_tokenize_str(nz.normalize_str(s))]
        if got != words:
            wrong += 1
            if wrong <= 5:
                print("  words differ:", ascii(s), ascii(got), ascii(words))
    print(f"words of {n_strings} random strings over keep / space / map code points and drops: {wrong} differ "
          f"({to_host} left to the host: a map code point in front of a joining space)")
    return wrong


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--layout", default="H", choices=["H", "C"])
    ap.add_argument("--rule", default="nmt_nfkc", choices=["nmt_nfkc", "nfkc", "identity"])
    ap.add_argument("--byte-fallback", action="store_true")
    ap.add_argument("--vocab-size", type=int, default=32000)
    ap.add_argument("--prepend-scheme", default="always", choices=["always", "first"], help="layout C only")
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--check", action="store_true", help="verify the class table against the library")
    ap.add_argument("--mapped", action="store_true", help="with --check: verify the mapped spec's tables instead")
    a = ap.parse_args()
    from textblaster_amd.models.tokenizer import TokenCounterModel, train_synthetic_unigram

    path = train_synthetic_unigram(a.out, a.vocab_size, a.layout, a.rule, a.byte_fallback, a.prepend_scheme, a.docs,
                                   a.seed)
    sp = TokenCounterModel(path).unigram_spec()
    print(f"{path}: layout {sp.layout}, {'byte_fallback, ' if sp.flags else ''}device table of {sp.mask + 1} slots "
          f"({(sp.slots.nbytes + sp.pool.nbytes) / 1e6:.2f} MB with the piece pool), longest piece {sp.longest_cp} "
          f"code points / {sp.longest} bytes, class table {sp.cls1.nbytes + sp.cls2.nbytes} bytes")
    if a.check:
        sys.exit(1 if (check_mapped(path) if a.mapped else check(path)) else 0)


if __name__ == "__main__":
    main()
