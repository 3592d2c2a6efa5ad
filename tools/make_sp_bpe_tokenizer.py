"""Trains a SentencePiece-style character-level BPE tokenizer on the synthetic Zipf corpus and writes
it as a ``tokenizer.json`` (models/tokenizer.py train_synthetic_sp_bpe: trained behind
Metaspace(split=true) with ``<unk>``, ``<s>``, ``</s>`` and the 256 ``<0xNN>`` byte tokens, written
with ``byte_fallback`` and a template that puts ``<s>`` in front): the offline stand-in for the
files of Llama-2, Mistral-7B v0.1-0.3, TinyLlama, Phi-3 and Gemma (layout L: normalizer
Sequence[Prepend, Replace], no pre-tokenizer) and for files that keep the Metaspace pre-tokenizer
(layout M), for ``bench.py --config config/bench_pipeline_tokens.yaml --tokenizer FILE`` and the
CLI's ``--tokenizer-dir``. Nothing is downloaded.

    python tools/make_sp_bpe_tokenizer.py OUT.json [--layout L|M] [--no-prepend]
                                          [--prepend-scheme always|first|never] [--no-split]
                                          [--vocab-size 32000] [--docs 20000] [--seed 1]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--layout", choices=["L", "M"], default="L")
    ap.add_argument("--no-prepend", action="store_true", help="layout L: the Replace normalizer alone")
    ap.add_argument("--prepend-scheme", choices=["always", "first", "never"], default="first",
                    help="layout M: Metaspace's prepend_scheme")
    ap.add_argument("--no-split", action="store_true", help="layout M: Metaspace with split false")
    ap.add_argument("--vocab-size", type=int, default=32000)
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    from textblaster_amd.models.tokenizer import TokenCounterModel, train_synthetic_sp_bpe

    path = train_synthetic_sp_bpe(a.out, a.vocab_size, a.layout, not a.no_prepend, a.prepend_scheme, not a.no_split,
                                  a.docs, a.seed)
    sp = TokenCounterModel(path).bpe_spec()
    if sp is None:
        sys.exit(f"{path}: no device spec (a merge joins a word to the space after it?)")
    print(f"{path}: layout {a.layout}, prepend rule {sp.sp_prepend}, "
          f"{'a chunk at every space' if sp.sp_split else 'a chunk per word and the spaces before it'}, "
          f"merge table of {sp.mask + 1} slots, {int((sp.sp_ascii != 0xFFFFFFFF).sum())} ASCII and "
          f"{int((sp.sp_cp != 2 ** 64 - 1).sum())} other single-character entries")


if __name__ == "__main__":
    main()
