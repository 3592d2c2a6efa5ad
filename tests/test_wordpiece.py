"""TokenCounter's WordPiece counter (csrc/common/wordpiece.h; device kernel k_wp_count).

The native counter (the kernel's algorithm compiled for the host) must give exactly the
`tokenizers` library's ``len(encode(text, add_special_tokens=True).tokens)`` - the reference's
TokenCounter (src/pipeline/token/token_counter.rs:31-42) - for BERT-style tokenizers trained here
(cased and uncased) and the checked-in bert-base-uncased fixture, over the synthetic corpora, the
adversarial pool, fuzz text of the normalizer's join / drop / space / isolate cases and the edge
documents. Cased tokenizers count every document natively; uncased ones send exactly the documents
with a code point the normalizer would change beyond ASCII case to the library. The emulated device
pipeline's token counts and metadata column must equal the CPU path's.
"""
import importlib.util
import json
import os
import random
import sys
import unicodedata

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wordpiece_corpus as wc  # noqa: E402

from textblaster_amd import native  # noqa: E402
from textblaster_amd.config import load_pipeline_config_str  # noqa: E402
from textblaster_amd.models.tokenizer import (MAX_ADDED, TokenCounterModel, build_wordpiece_spec,  # noqa: E402
                                              count_spec, train_synthetic_wordpiece)
from textblaster_amd.utils import synth  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BERT_FIXTURE = os.path.join(REPO, "tests", "fixtures", "tokenizers", "bert-base-uncased", "tokenizer.json")


@pytest.fixture(scope="module")
def cased(tmp_path_factory):
    return train_synthetic_wordpiece(str(tmp_path_factory.mktemp("tok") / "wp4k.json"), vocab_size=4000, n_docs=1500,
                                     seed=2)


@pytest.fixture(scope="module")
def uncased(tmp_path_factory):
    return train_synthetic_wordpiece(str(tmp_path_factory.mktemp("tok") / "wp4k_uncased.json"), vocab_size=4000,
                                     n_docs=1500, seed=2, lowercase=True)


def known_word(model):
    """A word of several letters that is one piece of the vocabulary."""
    for w in ("the", "and", "that", "with"):
        if model.tok.encode(w, add_special_tokens=False).tokens == [w]:
            return w
    raise AssertionError("no common word is a single piece of the trained vocabulary")


@pytest.fixture(scope="module")
def texts(cased):
    return wc.corpus(known_word(TokenCounterModel(cased)))


_REF = {}


def library_counts(model, docs, key):
    """``tokenizers`` counts, computed once per (tokenizer, corpus) and shared."""
    if key not in _REF:
        _REF[key] = np.array(model.count(docs))
        _REF[key].setflags(write=False)
    return _REF[key]


def raw_and_full(model, docs, chunk=0):
    data, off = synth.pack(docs)
    sp = model.wordpiece_spec()
    assert sp is not None
    return count_spec(sp, data, off, 4, chunk), model.count_native(data, off, 4)


def check_exact(model, docs, key, host_expected):
    """Every native count equals the library's, the documents left to the host are exactly
    ``host_expected`` (indices), and after the fallback all counts are the library's."""
    raw, full = raw_and_full(model, docs)
    ref = library_counts(model, docs, key)
    ok = raw >= 0
    bad = np.nonzero(ok & (raw != ref))[0]
    assert not len(bad), [(docs[k][:60], int(raw[k]), int(ref[k])) for k in bad[:5]]
    assert set(raw[~ok].tolist()) <= {-2}
    assert sorted(np.nonzero(~ok)[0].tolist()) == sorted(host_expected)
    np.testing.assert_array_equal(full, ref)
    return raw


def has_added(model, t):
    with open(model.path, encoding="utf-8") as f:
        return any(a["content"] in t for a in json.load(f).get("added_tokens") or [])


def changed_by_normalizer(model):
    """doc -> bool: it holds a non-ASCII code point that the tokenizer's lowercase / strip_accents
    change, or whose place NFD may change (a combining class), probed on the library."""
    from tokenizers import normalizers

    with open(model.path, encoding="utf-8") as f:
        nz = json.load(f)["normalizer"]
    lower = nz["lowercase"]
    strip = lower if nz["strip_accents"] is None else nz["strip_accents"]
    plain = normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=False, lowercase=False)
    fold = normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=strip, lowercase=lower)
    memo = {}

    def bad_char(c):
        if c not in memo:
            memo[c] = ord(c) >= 128 and (unicodedata.combining(c) != 0
                                         or fold.normalize_str(c) != plain.normalize_str(c))
        return memo[c]

    return lambda t: any(bad_char(c) for c in set(t))


# ---- 1. cased: everything on the device path --------------------------------------------------
def test_cased_counts_equal_tokenizers(cased, texts):
    m = TokenCounterModel(cased)
    assert m.bpe_spec() is None and m.wordpiece_spec() is not None
    sp = m.wordpiece_spec()
    assert sp.self_bit == 0 and sp.flags == 2 and sp.post_add == 2 and sp.max_chars == 100
    added = [k for k, t in enumerate(texts) if has_added(m, t)]
    assert [texts[k] for k in added] == [wc.ADDED_DOC]
    raw = check_exact(m, texts, "cased", added)
    by_text = {t: int(raw[k]) for k, t in enumerate(texts)}
    w = known_word(m)
    assert by_text[""] == 2 and by_text[" "] == 2
    assert by_text["a" * 101] == 3 and by_text["\u00e9" * 101] == 3 and by_text["x" * 5000] == 3  # over max_chars
    assert by_text["!" * 300] == 302
    assert by_text[w + "\u0378"] == 3  # the piece matches, U+0378 does not: the whole word is [UNK]


def test_lane_ranges_sum_to_the_document(cased, uncased, texts):
    """wp_count_range over a partition of the document (the kernel's lanes; here chunks of 1, 3, 16
    and 1000 bytes) gives the sequential count: word starts are local, words are followed past the
    range end, code points and drops that straddle a range edge are seen once."""
    docs = texts[-3500:] + ["a\u00ad" * 40 + "b", "\u00ad" * 70 + "x\u00ad\u00ad", "\u00e9" * 200,
                            "ab\u200b\u200b\u200bcd " * 9, "\U00020000" * 33]
    for path in (cased, uncased):
        m = TokenCounterModel(path)
        raw, _ = raw_and_full(m, docs)
        for chunk in (1, 3, 16, 1000):
            np.testing.assert_array_equal(raw_and_full(m, docs, chunk)[0], raw)


def test_invalid_utf8_goes_to_the_host(cased):
    m = TokenCounterModel(cased)
    sp, fine = m.wordpiece_spec(), m.count(["fine text"])[0]
    docs = [b"abc \xff def", b"abc \xc3", b"\x80abc", b"ab \xe2\x82 cd" + b"x" * 40, b"fine text",
            b"x" * 15 + b"\xc3\xa9\xa9"]
    data = np.frombuffer(b"".join(docs), dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)
    for chunk in (0, 1, 16):
        out = count_spec(sp, data, off, 1, chunk)
        assert out.tolist() == [-2, -2, -2, -2, fine, -2]


# ---- 2. uncased: ASCII folded on the device, other changes to the host --------------------------
def test_uncased_ascii_is_all_native(uncased):
    docs = wc.ascii_corpus()
    assert len(docs) > 1500
    for key, m in (("uncased-ascii", TokenCounterModel(uncased)), ("fixture-ascii", TokenCounterModel(BERT_FIXTURE))):
        assert m.wordpiece_spec().self_bit == 1 << 6 and m.wordpiece_spec().flags == 3
        check_exact(m, docs, key, [])


def test_uncased_counts_equal_tokenizers(uncased, texts):
    for key, m in (("uncased", TokenCounterModel(uncased)), ("fixture", TokenCounterModel(BERT_FIXTURE))):
        changed = changed_by_normalizer(m)
        host = [k for k, t in enumerate(texts) if changed(t) or has_added(m, t)]
        raw = check_exact(m, texts, key, host)
        assert 0 < len(host) < len(texts) and (raw >= 0).sum() > 1000


# ---- 3. specs -----------------------------------------------------------------------------------
def _variant(tj, tmp_path, name, **model_or_norm):
    tj = json.loads(json.dumps(tj))
    for k, v in model_or_norm.items():
        (tj["model"] if k in tj["model"] else tj["normalizer"])[k] = v
    p = tmp_path / f"{name}.json"
    p.write_text(json.dumps(tj))
    return TokenCounterModel(str(p))


def test_spec_variants_stay_exact(cased, tmp_path):
    tj = json.load(open(cased))
    docs = synth.make_corpus(300, 600, seed=8) + wc.fuzz(800, 9) + ["", "abcdefghij", "abcdefghijk", "\u00e9" * 11]
    docs = [t for t in docs if "[" not in t]
    m = _variant(tj, tmp_path, "max10", max_input_chars_per_word=10)
    assert m.wordpiece_spec().max_chars == 10
    check_exact(m, docs, "max10", [])
    m = _variant(tj, tmp_path, "noclean", clean_text=False)
    assert m.wordpiece_spec().cls_shift == 2
    check_exact(m, docs, "noclean", [])
    m = _variant(tj, tmp_path, "nochinese", handle_chinese_chars=False)
    assert m.wordpiece_spec().flags == 0
    check_exact(m, docs, "nochinese", [])
    m = _variant(tj, tmp_path, "strip", strip_accents=True)
    assert m.wordpiece_spec().self_bit == 1 << 5
    changed = changed_by_normalizer(m)
    check_exact(m, docs, "strip", [k for k, t in enumerate(docs) if changed(t)])
    # another continuation prefix: the vocabulary renamed with it
    tj2 = json.loads(json.dumps(tj))
    tj2["model"]["continuing_subword_prefix"] = "@@"
    tj2["model"]["vocab"] = {("@@" + k[2:] if k.startswith("##") else k): v for k, v in tj["model"]["vocab"].items()}
    tj2["decoder"]["prefix"] = "@@"
    m = _variant(tj2, tmp_path, "prefix")
    a = check_exact(m, docs, "prefix", [])
    np.testing.assert_array_equal(a, raw_and_full(TokenCounterModel(cased), docs)[0])
    # a prefix made of letters: "xx" + piece is also a word-initial piece of its own
    tj3 = json.loads(json.dumps(tj))
    tj3["model"]["continuing_subword_prefix"] = "xx"
    tj3["model"]["vocab"] = {("xx" + k[2:] if k.startswith("##") else k): v for k, v in tj["model"]["vocab"].items()}
    tj3["decoder"]["prefix"] = "xx"
    check_exact(_variant(tj3, tmp_path, "xx"), docs + ["xxing xxs axxb xx"], "xx", [])


def test_template_post_processor_and_unsupported_variants(cased):
    tj = json.load(open(cased))
    assert tj["post_processor"]["type"] == "TemplateProcessing"
    assert build_wordpiece_spec(tj).post_add == 2
    assert build_wordpiece_spec(dict(tj, post_processor=None)).post_add == 0
    none = [
        dict(tj, truncation={"max_length": 8, "strategy": "LongestFirst", "stride": 0, "direction": "Right"}),
        dict(tj, padding={"strategy": "BatchLongest"}),
        dict(tj, normalizer={"type": "Lowercase"}),
        dict(tj, normalizer=None),
        dict(tj, normalizer={"type": "Sequence", "normalizers": [tj["normalizer"]]}),
        dict(tj, pre_tokenizer={"type": "Whitespace"}),
        dict(tj, pre_tokenizer=None),
        dict(tj, model=dict(tj["model"], unk_token="[NOPE]")),
        dict(tj, model=dict(tj["model"], type="BPE")),
        dict(tj, post_processor={"type": "SomethingElse"}),
        dict(tj, added_tokens=[dict(tj["added_tokens"][0], content=f"[T{i}]") for i in range(MAX_ADDED + 1)]),
        dict(tj, added_tokens=[dict(tj["added_tokens"][0], normalized=True)]),
    ]
    for v in none:
        assert build_wordpiece_spec(v) is None
    gpt2 = os.path.join(REPO, "tests", "fixtures", "tokenizers", "gpt2", "tokenizer.json")
    m = TokenCounterModel(gpt2)
    assert m.wordpiece_spec() is None and m.device_spec() is m.bpe_spec()


# ---- 4. the class table -------------------------------------------------------------------------
def test_class_table_equals_a_fresh_probe():
    spec = importlib.util.spec_from_file_location("gen_wp_classes", os.path.join(REPO, "tools", "gen_wp_classes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    c1, c2 = native.host().wp_classes()
    rng = random.Random(11)
    cps = list(range(0x3001)) + [rng.randrange(0x110000) for _ in range(20000)]
    table = bytes(int(c2[int(c1[c >> 7]) * 128 + (c & 127)]) for c in cps)
    fresh = gen.probe(cps)
    diff = [(hex(c), t, f) for c, t, f in zip(cps, table, fresh) if t != f]
    assert not diff, diff[:10]
    # the cases the normalizer is known for: drop, space, isolate, keep (unassigned U+0378 is kept)
    cls = {c: table[cps.index(c)] & 3 for c in (0x85, 0xAD, 0x200B, 0x1C, 0xA0, 0x2028, 0x3000, 0x5F, 0x24, 0x2014,
                                                0x378, 0x61)}
    assert cls == {0x85: 1, 0xAD: 1, 0x200B: 1, 0x1C: 1, 0xA0: 2, 0x2028: 2, 0x3000: 2, 0x5F: 3, 0x24: 3, 0x2014: 3,
                   0x378: 0, 0x61: 0}
    asc = native.host().wp_ascii(0)
    assert [(int(asc[c >> 5]) >> (2 * (c & 31))) & 3 for c in range(128)] == [t & 3 for t in table[:128]]


# ---- 5. the emulated device pipeline ------------------------------------------------------------
def _cfg():
    return load_pipeline_config_str(
        "pipeline:\n"
        "  - {type: C4QualityFilter, split_paragraph: true, remove_citations: true, filter_no_terminal_punct: false,"
        " min_num_sentences: 1, min_words_per_line: 1, max_word_length: 1000, filter_lorem_ipsum: true,"
        " filter_javascript: true, filter_curly_bracket: true, filter_policy: true}\n"
        "  - {type: GopherQualityFilter, min_doc_words: 20, max_doc_words: 100000, min_avg_word_length: 2.0,"
        " max_avg_word_length: 12.0, max_symbol_word_ratio: 0.2, max_bullet_lines_ratio: 0.9,"
        " max_ellipsis_lines_ratio: 0.5, max_non_alpha_words_ratio: 0.9, min_stop_words: 0, stop_words: []}\n"
        "  - {type: TokenCounter, tokenizer_name: bert-base-cased}\n")


def test_emulated_device_token_counts_equal_cpu(cased):
    """Engine(emulate) with a trailing WordPiece TokenCounter: the counts come from the kernel's
    algorithm over the kept outputs, K18 formats the metadata column (no host fallback), and the
    outputs equal the CPU path's."""
    from test_emulated_device_path import outputs

    from textblaster_amd.pipeline.engine import Engine
    from textblaster_amd.utils import metrics

    docs = synth.make_corpus(2500, 900, seed=12) + wc.fuzz(200, 13)
    data, off = synth.pack(docs)
    eng = Engine(_cfg(), backend="emulate", nthreads=4, keep_reasons=True, tokenizer_file=cased)
    assert eng.device_runner.resolve_blob is not None and eng.device_runner.bpe
    assert eng.device_runner.meta_blob is not None
    res = eng.submit(data, off)
    assert res.dev.resolved is not None and res.dev.resolved.tokens
    h0, d0 = metrics.BPE_HOST_DOCS_TOTAL._value.get(), metrics.BPE_DEVICE_DOCS_TOTAL._value.get()
    f0 = metrics.DEVICE_META_FALLBACK_TOTAL._value.get()
    a = eng.finish(res)
    nh = metrics.BPE_HOST_DOCS_TOTAL._value.get() - h0
    nd = metrics.BPE_DEVICE_DOCS_TOTAL._value.get() - d0
    assert nd > 0 and nh == 0 and nh + nd == a.n_kept
    assert metrics.DEVICE_META_FALLBACK_TOTAL._value.get() == f0
    b = Engine(_cfg(), backend="cpu", nthreads=4, keep_reasons=True, tokenizer_file=cased,
               segmentation="icu").process(data, off)
    np.testing.assert_array_equal(a.status, b.status)
    oa, ob = outputs(a), outputs(b)
    assert oa == ob
    kept_meta = [m for k, t, m in oa.values() if k == "kept"]
    assert kept_meta and all(b'"token_count"' in m for m in kept_meta)


def test_device_tokens_off_leaves_wordpiece_to_the_host(cased, monkeypatch):
    from textblaster_amd.pipeline.engine import Engine

    monkeypatch.setenv("TB_TUNE", "device_tokens=0")
    eng = Engine(_cfg(), backend="emulate", nthreads=2, tokenizer_file=cased)
    assert not eng.device_runner.bpe
