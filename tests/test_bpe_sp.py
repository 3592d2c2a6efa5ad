"""TokenCounter's counter for the SentencePiece-style character-level BPE files (csrc/common/bpe_sp.h:
Llama-2 / Mistral / Gemma's layout L, and the Metaspace layout M; kernels k_bpe_sp_count /
k_bpe_sp_long).

Which files get a spec, and with which flags; the native counter (the kernels' algorithm compiled for
the host) against the `tokenizers` library's ``len(encode(text, add_special_tokens=True).tokens)``
for tokenizers trained here, in every layout; the documents it hands to the host tokenizer against
the rule stated in Python (tests/bpe_sp_corpus.py to_host); and the lane split at arbitrary cuts."""
import copy
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bpe_sp_corpus as sc  # noqa: E402

from textblaster_amd.models.tokenizer import (BPE_SP, SP_PREPEND_ALWAYS, SP_PREPEND_NONE,  # noqa: E402
                                              SP_PREPEND_UNLESS_SPACE, TokenCounterModel, build_bpe_spec,
                                              count_spec)
from textblaster_amd.utils import synth  # noqa: E402

SP = sc.SP


@pytest.fixture(scope="module")
def toks(tmp_path_factory):
    d = tmp_path_factory.mktemp("tok")
    return {name: sc.tokenizer(d, name) for name in sc.VARIANTS}


@pytest.fixture(scope="module")
def docs():
    return sc.corpus()


def raw_counts(model, packed, chunk=0):
    sp = model.bpe_spec()
    assert sp is not None and sp.kind == BPE_SP
    return count_spec(sp, packed[0], packed[1], 4, chunk)


# ---- 1. which files get a spec ------------------------------------------------------------------
def test_spec_acceptance(toks):
    for name, (_, prepend, split) in sc.VARIANTS.items():
        tj = json.load(open(toks[name]))
        assert tj["model"]["byte_fallback"] is True and tj["model"]["fuse_unk"] is True
        assert (tj["pre_tokenizer"] is None) == name.startswith("L")
        sp = build_bpe_spec(tj)
        assert sp is not None and sp.kind == BPE_SP, name
        assert (sp.sp_prepend, sp.sp_split) == (prepend, split), name
        assert sp.post_add == 1 and len(sp.added_off) == 4 and not sp.ignore_merges and not sp.nfc
        vocab = tj["model"]["vocab"]
        assert sp.sp_id == vocab[SP] and sp.byte_id.tolist() == [vocab[f"<0x{b:02X}>"] for b in range(256)]
        assert sp.sp_ascii[ord("a")] == vocab["a"] and sp.sp_ascii[0] == 0xFFFFFFFF
        # the corpus has characters of either kind: entries of the code point table, and byte fallback
        table = {int(e) >> 32: int(e) & 0xFFFFFFFF for e in sp.sp_cp if int(e) != 2 ** 64 - 1}
        assert all(table[ord(c)] == vocab[c] for c in sc.IN_VOCAB)
        assert not any(c in vocab for c in ("é", "あ", sc.EMOJI, "ý", "\u0301"))
        m = TokenCounterModel(toks[name])
        assert m.device_spec() is m.bpe_spec() and m.bpe_spec().kind == BPE_SP
    assert {v[1] for v in sc.VARIANTS.values()} == {SP_PREPEND_NONE, SP_PREPEND_ALWAYS, SP_PREPEND_UNLESS_SPACE}


def test_no_spec(toks):
    tj = json.load(open(toks["L-prepend"]))
    mj = json.load(open(toks["M-first-whole"]))
    ms = json.load(open(toks["M-first-split"]))

    def model(t, **kw):
        return dict(t, model=dict(t["model"], **kw))

    vocab, merges = tj["model"]["vocab"], tj["model"]["merges"]
    # a merge that joins a piece ending in a letter to one starting with the space, added by hand
    x, y = "e", SP + "a"
    assert x in vocab and y in vocab and (x + y) not in vocab
    crossing = dict(vocab, **{x + y: len(vocab)})
    cross_merge = merges + [[x, y] if not isinstance(merges[0], str) else f"{x} {y}"]
    prepend, replace = tj["normalizer"]["normalizers"]
    added = tj["added_tokens"]
    none = {
        "crossing merge, L": model(tj, vocab=crossing, merges=cross_merge),
        "crossing merge, M without split": model(mj, vocab=crossing, merges=cross_merge),
        "a byte token missing": model(tj, vocab={k: v for k, v in vocab.items() if k != "<0x7F>"}),
        "no U+2581": model(tj, vocab={k: v for k, v in vocab.items() if k != SP},
                           merges=[]),
        "ignore_merges": model(tj, ignore_merges=True),
        "dropout": model(tj, dropout=0.1),
        "end_of_word_suffix": model(tj, end_of_word_suffix="</w>"),
        "NFKC in the sequence": dict(tj, normalizer={"type": "Sequence", "normalizers": [
            prepend, replace, {"type": "NFKC"}]}),
        "NFKC in front": dict(tj, normalizer={"type": "Sequence", "normalizers": [{"type": "NFKC"}, prepend, replace]}),
        "Replace of another string": dict(tj, normalizer=dict(replace, pattern={"String": "\t"})),
        "Replace by another string": dict(tj, normalizer=dict(replace, content="_")),
        "Replace of a regex": dict(tj, normalizer=dict(replace, pattern={"Regex": " "})),
        "Prepend of another string": dict(tj, normalizer={"type": "Sequence", "normalizers": [
            dict(prepend, prepend="_"), replace]}),
        "normalised added token with a space": dict(tj, added_tokens=added + [
            dict(added[0], id=len(vocab), content="two words", normalized=True, special=False)]),
        "normalised added token with U+2581": dict(tj, added_tokens=added + [
            dict(added[0], id=len(vocab), content=SP + "word", normalized=True, special=False)]),
        "truncation": dict(tj, truncation={"direction": "Right", "max_length": 512, "strategy": "LongestFirst",
                                           "stride": 0}),
        "unknown post-processor": dict(tj, post_processor={"type": "Mystery"}),
        "Metaspace behind a normalizer": dict(ms, normalizer=replace),
        "Metaspace with another replacement": dict(ms, pre_tokenizer=dict(ms["pre_tokenizer"], replacement="_")),
        "no byte_fallback": model(tj, byte_fallback=False),
    }
    for why, v in none.items():
        assert build_bpe_spec(v, nfc=True) is None, why
    # the same crossing merge is harmless where Metaspace splits at every space
    assert build_bpe_spec(model(ms, vocab=crossing, merges=cross_merge)).sp_split
    # an added token matched on normalised text without a space in it is the same statement on the raw text
    ok = build_bpe_spec(dict(tj, added_tokens=added + [
        dict(added[0], id=len(vocab), content="<tool>", normalized=True, special=False)]))
    assert ok is not None and len(ok.added_off) == 5
    assert build_bpe_spec(copy.deepcopy(tj)).kind == BPE_SP


# ---- 2. counts against the library, the host set against the rule -------------------------------
@pytest.mark.parametrize("name", list(sc.VARIANTS))
def test_counts_equal_tokenizers(toks, docs, name):
    _, prepend, split = sc.VARIANTS[name]
    m = TokenCounterModel(toks[name])
    raw = raw_counts(m, sc.pack(docs + sc.INVALID))
    assert set(raw[raw < 0].tolist()) <= {-2}
    want_host = np.array([sc.to_host(d, prepend, split) for d in docs + sc.INVALID])
    diff = np.nonzero((raw == -2) != want_host)[0]
    assert not len(diff), [((docs + sc.INVALID)[k][:40], int(raw[k])) for k in diff[:5]]
    assert want_host[-len(sc.INVALID):].all() and want_host[len(docs) - len(sc.HOST_DOCS):len(docs)].all()
    ref = np.array(m.count(docs))
    raw = raw[:len(docs)]
    bad = np.nonzero((raw >= 0) & (raw != ref))[0]
    assert not len(bad), [(docs[k][:60], int(raw[k]), int(ref[k])) for k in bad[:5]]
    data, off = synth.pack(docs)
    np.testing.assert_array_equal(m.count_native(data, off, 4), ref)
    by_text = {t: int(raw[k]) for k, t in enumerate(docs)}
    assert by_text[""] == 1
    assert by_text[" "] == (3 if prepend == SP_PREPEND_ALWAYS else 2)
    # the prepended symbol counts towards the 2048 of the merge arrays, at offset 0 only
    at0 = prepend != SP_PREPEND_NONE
    assert (by_text["q" * 2048] == -2) == at0 and by_text["q" * 2047] > 0 and by_text["q" * 2049] == -2
    assert by_text["head " + "q" * 2047] > 0 and by_text["head " + "q" * 2048] == -2
    assert (by_text[" " * 2049] == -2) == (not split) and by_text[" " * 2048] == (-2 if prepend == SP_PREPEND_ALWAYS
                                                                                 else 2049)


def test_synthetic_documents_stay_on_the_device(toks):
    """At most 2 % of the synthetic part may come back -2; the rule alone gives none, the longest
    chunk being far below 2048 bytes."""
    syn = sc.synthetic() + synth.make_corpus(500, 1024, seed=5, vocab="zipf")
    longest = max(len(c.encode("utf-8")) for t in syn for c in sc.chunks(t, False))
    print(f"longest chunk of the synthetic part: {longest} bytes")
    assert longest < sc.MAX_LONG
    for name in ("L-prepend", "M-first-split"):
        raw = raw_counts(TokenCounterModel(toks[name]), sc.pack(syn))
        assert (raw < 0).mean() <= 0.02
        assert not any(sc.to_host(t, *sc.VARIANTS[name][1:]) for t in syn) and (raw >= 0).all()


def test_library_prepend_rule(toks):
    """Layout L prepends in front of every text that is not empty, Metaspace (always / first) unless
    the text starts with a space or U+2581, "never" never: the counter's lead symbol is the library's."""
    from tokenizers import Tokenizer

    for name, (_, prepend, _) in sc.VARIANTS.items():
        tok = Tokenizer.from_file(toks[name])
        for text in ["", "a", " a", SP + "a", "é", " ", SP, "\na"]:
            got = "".join(tok.encode(text, add_special_tokens=False).tokens)
            body = text.replace(" ", SP)
            assert got.replace("<0xC3><0xA9>", "é") == SP * sc.lead(text, prepend) + body, (name, text, got)


# ---- 3. the lane split --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.VARIANTS))
def test_lane_ranges_sum_to_the_document(toks, docs, name):
    """The chunks that start in each c-byte range, counted on their own, sum to the sequential count:
    cuts fall inside multi-byte characters, inside space runs and between a space and a U+2581."""
    m = TokenCounterModel(toks[name])
    lane = docs + sc.INVALID + ["a " + SP + " " + SP + "b" * 20 + "  " + SP + SP + " あ" + sc.EMOJI * 3 + "é " * 9,
                                ("あ" + sc.EMOJI) * 40, (" " + SP) * 30 + "x", "word  " * 50]
    packed = sc.pack(lane)
    raw = raw_counts(m, packed)
    for chunk in (16, 17, 32):
        np.testing.assert_array_equal(raw_counts(m, packed, chunk), raw)
    small = sc.pack(sc.fuzz(500, 8) + [d for d in sc.edge_docs() if len(d) < 200] + sc.INVALID)
    raw = raw_counts(m, small)
    for chunk in (1, 2, 3, 5):
        np.testing.assert_array_equal(raw_counts(m, small, chunk), raw)


# ---- 4. the emulated device pipeline ------------------------------------------------------------
def test_emulated_device_token_counts_equal_cpu(toks):
    from test_bpe import _cfg
    from test_emulated_device_path import outputs

    from textblaster_amd.pipeline.engine import Engine
    from textblaster_amd.utils import metrics

    tok = toks["L-prepend"]
    data, off = synth.pack(synth.make_corpus(2500, 900, seed=12))
    eng = Engine(_cfg(), backend="emulate", nthreads=4, keep_reasons=True, tokenizer_file=tok)
    assert eng.device_runner.bpe
    h0, d0 = metrics.BPE_HOST_DOCS_TOTAL._value.get(), metrics.BPE_DEVICE_DOCS_TOTAL._value.get()
    a = eng.process(data, off)
    nh = metrics.BPE_HOST_DOCS_TOTAL._value.get() - h0
    nd = metrics.BPE_DEVICE_DOCS_TOTAL._value.get() - d0
    assert nh == 0 and nd == a.n_kept > 0
    b = Engine(_cfg(), backend="cpu", nthreads=4, keep_reasons=True, tokenizer_file=tok,
               segmentation="icu").process(data, off)
    np.testing.assert_array_equal(a.status, b.status)
    assert outputs(a) == outputs(b)
