"""TokenCounter's Unigram counter (csrc/common/unigram.h; device kernel k_uni_count).

The native counter (the kernel's algorithm compiled for the host) must give exactly the
`tokenizers` library's ``len(encode(text, add_special_tokens=True).tokens)`` - the reference's
TokenCounter (src/pipeline/token/token_counter.rs:31-42) - for Unigram tokenizers trained here with
``sentencepiece`` and written in the two serialisation layouts of T5 / mT5 / XLM-R files, with and
without a Precompiled normalizer and byte_fallback. It sends exactly the documents of the
per-document rule (tests/unigram_corpus.py to_host) to the library and counts every other one.
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unigram_corpus as uc  # noqa: E402

from textblaster_amd import native  # noqa: E402
from textblaster_amd.config import load_pipeline_config_str  # noqa: E402
from textblaster_amd.models import tokenizer as T  # noqa: E402
from textblaster_amd.models.tokenizer import (TokenCounterModel, UnigramSpec, build_unigram_spec,  # noqa: E402
                                              count_spec)
from textblaster_amd.utils import synth  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("uni")


def test_constants_equal_the_header():
    c = native.host().UNI_CONSTANTS
    assert (c["UNI_KEEP"], c["UNI_SPACE"], c["UNI_HOST"]) == (T.UNI_KEEP, T.UNI_SPACE, T.UNI_HOST)
    assert c["UNI_BYTE_FALLBACK"] == T.UNI_BYTE_FALLBACK
    assert (c["UNI_MAX_PIECE_CP"], c["UNI_MAX_PIECE_BYTES"]) == (T.UNI_MAX_PIECE_CP, T.UNI_MAX_PIECE_BYTES)
    assert T.UNI_MAX_PIECE_CP >= 16 and T.UNI_MAX_PIECE_BYTES >= 64


# ---- 1. specs -----------------------------------------------------------------------------------
def test_accepted_layouts(tok_dir):
    for variant, flags, layout in (("H-nmt", 0, "H"), ("C-nmt-first", 0, "C"), ("C-nmt-always", 0, "C"),
                                   ("H-nmt-bytefallback", T.UNI_BYTE_FALLBACK, "H"), ("H-identity", 0, "H")):
        m = TokenCounterModel(uc.tokenizer(variant, tok_dir))
        sp = m.unigram_spec()
        assert isinstance(sp, UnigramSpec) and m.bpe_spec() is None and m.wordpiece_spec() is None
        assert m.device_spec() is sp
        assert (sp.flags, sp.layout, sp.post_add) == (flags, layout, 1)
        tj = json.load(open(m.path))
        scores = [s for _, s in tj["model"]["vocab"]]
        assert sp.unk_score == min(scores) - 10.0
        assert sp.longest_cp == max(len(p) for p, _ in tj["model"]["vocab"]) <= T.UNI_MAX_PIECE_CP
        assert sp.longest == max(len(p.encode()) for p, _ in tj["model"]["vocab"])
        assert bytes(sp.sp) == "\u2581".encode()
        # the unk piece's text is one more added-token string
        assert bytes(sp.added) == b"<pad></s><unk>" and sp.added_off == [0, 5, 9, 14]
    # the older serialisation of Metaspace, and a file without the Precompiled normalizer
    tj = json.load(open(uc.tokenizer("H-nmt", tok_dir)))
    tj["pre_tokenizer"]["pretokenizers"][1] = {"type": "Metaspace", "replacement": "\u2581", "add_prefix_space": True}
    assert build_unigram_spec(tj) is not None
    tj["normalizer"]["normalizers"].pop(0)
    assert build_unigram_spec(tj) is not None


def test_refusals(tok_dir):
    tj = json.load(open(uc.tokenizer("H-nmt", tok_dir)))
    cj = json.load(open(uc.tokenizer("C-nmt-first", tok_dir)))
    bj = json.load(open(uc.tokenizer("H-nmt-bytefallback", tok_dir)))
    cache = str(tok_dir)
    assert build_unigram_spec(tj, cache) is not None and build_unigram_spec(cj, cache) is not None

    def model(j, **kw):
        return dict(j, model=dict(j["model"], **kw))

    def meta(**kw):
        return dict(cj["pre_tokenizer"], **kw)

    vocab = tj["model"]["vocab"]
    pre, squeeze = tj["normalizer"]["normalizers"]
    tok0 = tj["added_tokens"][0]
    none = [
        model(tj, type="BPE"),
        model(tj, unk_id=None),
        model(tj, unk_id=len(vocab)),
        model(tj, vocab=vocab + [vocab[10]]),  # a duplicate piece
        model(tj, vocab=vocab + [["x" * (T.UNI_MAX_PIECE_CP + 1), -20.0]]),  # longer than the ring
        model(tj, vocab=vocab + [["\U00020000" * T.UNI_MAX_PIECE_CP + "\u00e9", -20.0]]),  # ... in bytes
        model(bj, vocab=[v for v in bj["model"]["vocab"] if v[0] != "<0x7F>"]),  # byte_fallback without a byte
        dict(tj, truncation={"max_length": 8, "strategy": "LongestFirst", "stride": 0, "direction": "Right"}),
        dict(tj, padding={"strategy": "BatchLongest"}),
        dict(tj, post_processor={"type": "SomethingElse"}),
        dict(tj, added_tokens=[dict(tok0, content=f"<t{i}>") for i in range(T.SPLIT_MAX_ADDED + 1)]),
        dict(tj, added_tokens=[dict(tok0, content="x" * 40000), dict(tok0, content="y" * 40000)]),
        dict(tj, added_tokens=[dict(tok0, normalized=True)]),
        # ALBERT's chain, no normalizer, a normalizer that is no Sequence
        dict(tj, normalizer={"type": "Sequence", "normalizers": [
            {"type": "Replace", "pattern": {"String": "``"}, "content": '"'}, {"type": "NFKD"}, {"type": "StripAccents"},
            {"type": "Lowercase"}, pre, squeeze]}),
        dict(tj, normalizer=None),
        dict(tj, normalizer=pre),
        dict(tj, normalizer={"type": "Sequence", "normalizers": [pre, squeeze, {"type": "Lowercase"}]}),
        # the whole-document Replace(" ", "▁") layout without a pre-tokenizer
        dict(tj, normalizer={"type": "Sequence", "normalizers": [
            pre, {"type": "Replace", "pattern": {"String": " "}, "content": "\u2581"}]}, pre_tokenizer=None),
        dict(tj, pre_tokenizer=None),
        dict(tj, pre_tokenizer={"type": "WhitespaceSplit"}),
        dict(tj, pre_tokenizer=cj["pre_tokenizer"]),  # layout H's normalizer with layout C's pre-tokenizer
        dict(cj, pre_tokenizer=tj["pre_tokenizer"]),
        dict(cj, pre_tokenizer=meta(prepend_scheme="never")),
        dict(cj, pre_tokenizer=meta(split=False)),
        dict(cj, pre_tokenizer=meta(replacement="_")),
        dict(tj, pre_tokenizer={"type": "Sequence", "pretokenizers": [{"type": "WhitespaceSplit"},
                                                                      meta(prepend_scheme="first")]}),
        dict(cj, normalizer={"type": "Sequence", "normalizers": [
            pre, {"type": "Strip", "strip_left": True, "strip_right": True}, cj["normalizer"]["normalizers"][2]]}),
    ]
    for k, v in enumerate(none):
        assert build_unigram_spec(v, cache) is None, k
    gpt2 = os.path.join(REPO, "tests", "fixtures", "tokenizers", "gpt2", "tokenizer.json")
    m = TokenCounterModel(gpt2)
    assert m.unigram_spec() is None and m.device_spec() is m.bpe_spec()


def test_parameter_block_validator(tok_dir):
    import copy

    h = native.host()
    sp = TokenCounterModel(uc.tokenizer("H-nmt", tok_dir)).unigram_spec()
    data, off = uc.pack(["a b"])
    assert count_spec(sp, data, off)[0] > 0
    for change in (dict(longest_cp=T.UNI_MAX_PIECE_CP + 1), dict(longest=0), dict(mask=sp.mask - 1),
                   dict(cls1=sp.cls1[:-1]), dict(cls2=sp.cls2[:-1]), dict(sp=np.zeros(5, np.uint8)), dict(flags=2),
                   dict(unk_score=float("inf")), dict(added_off=[0, 5, 9, 99]), dict(pool=sp.pool[:10])):
        bad = copy.copy(sp)
        for k, v in change.items():
            setattr(bad, k, v)
        with pytest.raises(ValueError):
            h.uni_count(data, off, bad, 1, 0)
        with pytest.raises(ValueError):
            h.uni_params(bad, {})
    with pytest.raises(ValueError):  # every table the counter reads needs an address
        h.uni_params(sp, {"slots": 16, "pool": 16, "cls1": 16, "added": 16, "aoff": 16})
    block = h.uni_params(sp, {"slots": 16, "pool": 32, "cls1": 48, "cls2": 64, "added": 80, "aoff": 96})
    assert len(block) == h.SIZEOF_DEV_UNI
    o = h.DEV_UNI_OFFSETS
    assert int.from_bytes(block[o["cls2"]:o["cls2"] + 8], "little") == 64
    assert int.from_bytes(block[o["longest_cp"]:o["longest_cp"] + 4], "little") == sp.longest_cp
    assert np.frombuffer(block[o["unk_score"]:o["unk_score"] + 8], np.float64)[0] == sp.unk_score


# ---- 2. the class table -------------------------------------------------------------------------
def _classes(sp):
    cps = np.arange(0x110000)
    return (sp.cls2[sp.cls1[cps >> 7].astype(np.int64) * 32 + ((cps & 127) >> 2)] >> (2 * (cps & 3))) & 3


def test_class_table_of_nmt_nfkc(tok_dir):
    import unicodedata

    m = TokenCounterModel(uc.tokenizer("H-nmt", tok_dir))
    cls = _classes(m.unigram_spec())
    space = {9, 10, 12, 13, 0x20, 0xA0, 0x1680, *range(0x2000, 0x200D), 0x200E, 0x200F, 0x2028, 0x2029, 0x202F, 0x205F,
             0x2581, 0x3000, 0xFEFF, 0xFFFD}
    # ... which the charsmap maps to U+0020 (and U+0020); U+0085 it keeps, and WhitespaceSplit separates on it
    assert len(space) == 30 and set(np.nonzero(cls == T.UNI_SPACE)[0].tolist()) == space | {0x85}
    keep = np.nonzero(cls == T.UNI_KEEP)[0]
    assert len(keep) > 250_000
    joiners = [c for c in keep.tolist() if uc.JOINER.match(chr(c)) or unicodedata.category(chr(c)) in ("Mn", "Me", "Mc", "Cn")]
    assert not joiners, [hex(c) for c in joiners[:10]]
    for c in (0x2026, 0xFB01, 0x01, 0x9F, 0x0301, 0x200D, 0x1161, 0xD800, 0xFF21):
        assert cls[c] == T.UNI_HOST, hex(c)
    for c in (0x61, 0x201C, 0x2014, 0x4F60, 0x1F600, 0xAC00, 0xE9):
        assert cls[c] == T.UNI_KEEP, hex(c)
    # layout C: the same but for kept white space; without Precompiled: white space by the layout, marks kept
    c_cls = _classes(TokenCounterModel(uc.tokenizer("C-nmt-first", tok_dir)).unigram_spec())
    assert np.nonzero(c_cls != cls)[0].tolist() == [0x85] and c_cls[0x85] == T.UNI_HOST
    ident = _classes(TokenCounterModel(uc.tokenizer("H-identity", tok_dir)).unigram_spec())
    assert ident[0x0A] == ident[0xA0] == ident[0x85] == T.UNI_SPACE and ident[0x2581] == T.UNI_HOST
    assert ident[0x0301] == ident[0x2026] == ident[0x01] == T.UNI_KEEP
    c_ident = T.unigram_classes(None, "C")
    assert c_ident[0x0A] == c_ident[0xA0] == T.UNI_HOST and c_ident[0x20] == T.UNI_SPACE


def test_class_table_cache(tok_dir):
    path = uc.tokenizer("H-nmt", tok_dir)
    a = TokenCounterModel(path).unigram_spec()
    cached = [f for f in os.listdir(tok_dir) if f.startswith("unigram_classes.") and f.endswith(".npz")]
    assert cached
    b = TokenCounterModel(path).unigram_spec()  # read back from the cache
    assert (a.cls1 == b.cls1).all() and (a.cls2 == b.cls2).all()
    fresh = build_unigram_spec(json.load(open(path)))  # no cache directory: probed
    assert (a.cls1 == fresh.cls1).all() and (a.cls2 == fresh.cls2).all()


# ---- 3. counts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(uc.VARIANTS))
def test_counts_equal_tokenizers(tok_dir, variant):
    path = uc.tokenizer(variant, tok_dir)
    m = TokenCounterModel(path)
    sp = m.unigram_spec()
    word, top = uc.longest_word(path)
    assert top == sp.longest_cp and m.tok.encode(word, add_special_tokens=False).tokens == ["\u2581" + word]
    cats = uc.categories(word)
    docs = uc.corpus(word)
    data, off = uc.pack(docs)
    raw = count_spec(sp, data, off, 4)
    ref = np.array(m.count(docs))
    rule = uc.to_host(path, variant)
    host = np.array([rule(t) for t in docs])
    print(f"{variant}: {len(docs)} documents, {int(host.sum())} to the host by the rule, "
          f"{int((raw < 0).sum())} by the counter, {int(((raw >= 0) & (raw != ref)).sum())} counts differ")
    assert set(raw[raw < 0].tolist()) <= {-2}
    wrong = np.nonzero((raw < 0) != host)[0]
    assert not len(wrong), [(docs[k][:60], int(raw[k]), bool(host[k])) for k in wrong[:5]]
    bad = np.nonzero(~host & (raw != ref))[0]
    assert not len(bad), [(docs[k][:60], int(raw[k]), int(ref[k])) for k in bad[:5]]
    np.testing.assert_array_equal(count_spec(sp, data, off, 4, chunk=16), raw)
    np.testing.assert_array_equal(count_spec(sp, data, off, 4, chunk=1), raw)
    np.testing.assert_array_equal(m.count_native(data, off, 4), ref)
    # every category is counted on the device, except what the rule sends to the host
    by_text = {t: int(raw[k]) for k, t in enumerate(docs)}
    for name in ("zipf", "unknown", "longest", "empty"):
        assert any(by_text[t] >= 0 for t in cats[name]), name
    assert all(by_text[t] == -2 for t in cats["added"])
    nmt = VARIANTS_NMT[variant]
    # what nmt_nfkc replaces, drops or joins is counted only without it; U+2581 only where it becomes a space
    assert [by_text[t] >= 0 for t in cats["normalizer"]] == [not nmt] * 6 + [nmt] * 2
    assert by_text[""] == 1 and by_text[" "] == 1 and by_text[word] == 2
    # "▁" + a fused unknown run, the pieces of "▁the" + an unknown, </s>; with byte_fallback an
    # unknown code point counts its bytes
    the = int(count_spec(sp, *uc.pack(["the"]))[0]) - 1
    emoji = by_text["\U0001F600\U0001F600 the\U0001F600"]
    assert emoji == (1 + 8) + (the + 4) + 1 if variant == "H-nmt-bytefallback" else emoji == (1 + 1) + (the + 1) + 1


VARIANTS_NMT = {v: kw["rule"] != "identity" for v, kw in uc.VARIANTS.items()}


def test_invalid_utf8_goes_to_the_host(tok_dir):
    m = TokenCounterModel(uc.tokenizer("H-nmt", tok_dir))
    sp, fine = m.unigram_spec(), m.count(["fine text"])[0]
    data = np.frombuffer(b"".join(uc.INVALID), dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(d) for d in uc.INVALID]).astype(np.int64)
    for chunk in (0, 1, 16):
        out = count_spec(sp, data, off, 1, chunk)
        assert out.tolist() == [-2 if h else fine for h in uc.INVALID_HOST]


def test_words_and_documents_have_no_size_limit(tok_dir):
    m = TokenCounterModel(uc.tokenizer("H-nmt", tok_dir))
    docs = ["x" * 5000, "the" * 3000, "\u4f60" * 3000, "\U0001F600" * 2500 + "a", "a " * 40000]
    data, off = uc.pack(docs)
    raw = count_spec(m.unigram_spec(), data, off, 4)
    np.testing.assert_array_equal(raw, m.count(docs))
    np.testing.assert_array_equal(count_spec(m.unigram_spec(), data, off, 4, chunk=16), raw)


# ---- 4. the emulated device pipeline ------------------------------------------------------------
def _cfg():
    return load_pipeline_config_str(
        "pipeline:\n"
        "  - {type: C4QualityFilter, split_paragraph: true, remove_citations: true, filter_no_terminal_punct: false,"
        " min_num_sentences: 1, min_words_per_line: 1, max_word_length: 1000, filter_lorem_ipsum: true,"
        " filter_javascript: true, filter_curly_bracket: true, filter_policy: true}\n"
        "  - {type: GopherQualityFilter, min_doc_words: 20, max_doc_words: 100000, min_avg_word_length: 2.0,"
        " max_avg_word_length: 12.0, max_symbol_word_ratio: 0.2, max_bullet_lines_ratio: 0.9,"
        " max_ellipsis_lines_ratio: 0.5, max_non_alpha_words_ratio: 0.9, min_stop_words: 0, stop_words: []}\n"
        "  - {type: TokenCounter, tokenizer_name: t5-small}\n")


def test_emulated_device_token_counts_equal_cpu(tok_dir, monkeypatch):
    """Engine(emulate) with a trailing Unigram TokenCounter: the counts come from the kernel's
    algorithm over the kept outputs, the documents of the rule from the library, and the outputs
    equal the CPU path's."""
    from test_emulated_device_path import outputs

    from textblaster_amd.pipeline.engine import Engine
    from textblaster_amd.utils import metrics

    tok = uc.tokenizer("H-nmt", tok_dir)
    docs = synth.make_corpus(2500, 900, seed=12) + uc.fuzz(200, 13)
    data, off = synth.pack(docs)
    delegated = uc.watch_delegated(monkeypatch)
    eng = Engine(_cfg(), backend="emulate", nthreads=4, keep_reasons=True, tokenizer_file=tok)
    assert eng.device_runner.resolve_blob is not None and eng.device_runner.bpe
    h0, d0 = metrics.BPE_HOST_DOCS_TOTAL._value.get(), metrics.BPE_DEVICE_DOCS_TOTAL._value.get()
    a = eng.process(data, off)
    nh = metrics.BPE_HOST_DOCS_TOTAL._value.get() - h0
    nd = metrics.BPE_DEVICE_DOCS_TOTAL._value.get() - d0
    b = Engine(_cfg(), backend="cpu", nthreads=4, keep_reasons=True, tokenizer_file=tok,
               segmentation="icu").process(data, off)
    np.testing.assert_array_equal(a.status, b.status)
    oa, ob = outputs(a), outputs(b)
    assert oa == ob
    # a document handed to the CPU path as a whole is counted there and by neither counter
    kept, want = uc.rule_count(uc.to_host(tok, "H-nmt"), docs, oa, delegated)
    assert nd > 0 and nh == want > 0 and nh + nd == kept <= a.n_kept
