"""Trains a Llama-3-format byte-level BPE tokenizer on the synthetic Zipf corpus and writes it as a
``tokenizer.json`` (models/tokenizer.py train_synthetic_split_bpe: Split(pattern A, B, C or D, Isolated) +
ByteLevel(use_regex=false), ``ignore_merges``, ``<|begin_of_text|>`` and reserved specials as added
tokens): the offline stand-in for Llama-3 / cl100k_base (pattern A) and Qwen2 (pattern B with
``--nfc``, the NFC normalizer its files carry), o200k_base (pattern C) and Tekken (pattern D), for
``bench.py --config config/bench_pipeline_tokens.yaml --tokenizer FILE`` and the CLI's
``--tokenizer-dir``.

    python tools/make_split_bpe_tokenizer.py OUT.json [--pattern A|B|C|D] [--vocab-size 32000] [--docs 20000]
                                             [--seed 1] [--added 256] [--no-ignore-merges] [--nfc]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--pattern", choices=["A", "B", "C", "D"], default="A")
    ap.add_argument("--vocab-size", type=int, default=32000)
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--added", type=int, default=256, help="added (special) tokens, Llama-3 carries 256")
    ap.add_argument("--no-ignore-merges", action="store_true", help="model.ignore_merges false (cl100k_base, Qwen2)")
    ap.add_argument("--nfc", action="store_true", help="normalizer NFC (Qwen2)")
    a = ap.parse_args()
    from textblaster_amd.models.tokenizer import TokenCounterModel, train_synthetic_split_bpe

    path = train_synthetic_split_bpe(a.out, a.vocab_size, a.pattern, not a.no_ignore_merges, a.added, a.docs, a.seed,
                                     a.nfc)
    sp = TokenCounterModel(path).bpe_spec()
    print(f"{path}: pattern {a.pattern}{', NFC' if sp.nfc else ''}, merge table of {sp.mask + 1} slots, {len(sp.added_off) - 1} added tokens, "
          + (f"vocabulary table of {sp.vmask + 1} slots, longest entry {sp.vlongest} bytes" if sp.ignore_merges
             else "ignore_merges off"))


if __name__ == "__main__":
    main()
