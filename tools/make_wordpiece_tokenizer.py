"""Trains a BERT-format WordPiece tokenizer on the synthetic Zipf corpus and writes it as a
``tokenizer.json`` (models/tokenizer.py train_synthetic_wordpiece): the offline stand-in for
bert-base-cased / bert-base-uncased, for ``bench.py --config config/bench_pipeline_tokens.yaml
--tokenizer FILE`` and the CLI's ``--tokenizer-dir``.

    python tools/make_wordpiece_tokenizer.py OUT.json [--vocab-size 30522] [--docs 20000] [--seed 1]
        [--uncased] [--keep-accents]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--vocab-size", type=int, default=30522)
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--uncased", action="store_true", help="BertNormalizer lowercase (and strip_accents) on")
    ap.add_argument("--keep-accents", action="store_true",
                    help="strip_accents false (with --uncased: the lowercase-only mode of the folding counter)")
    a = ap.parse_args()
    from textblaster_amd.models.tokenizer import TokenCounterModel, train_synthetic_wordpiece

    path = train_synthetic_wordpiece(a.out, a.vocab_size, a.docs, a.seed, lowercase=a.uncased,
                                     strip_accents=False if a.keep_accents else None)
    sp = TokenCounterModel(path).wordpiece_fold_spec()
    print(f"{path}: {'uncased' if a.uncased else 'cased'}, fold mode {sp.fold}, device table of {sp.mask + 1} slots, "
          f"longest piece {sp.longest} bytes")


if __name__ == "__main__":
    main()
