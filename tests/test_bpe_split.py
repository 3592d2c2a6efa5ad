"""TokenCounter's counter for split-regex byte-level BPE tokenizers (csrc/common/bpe_split.h; device
kernels k_bpe_split_count / k_bpe_split_long): Llama-3, cl100k_base and Qwen2 layouts.

The native counter (the kernels' algorithm compiled for the host) must give exactly the `tokenizers`
library's ``len(encode(text, add_special_tokens=True).tokens)`` - the reference's TokenCounter
(src/pipeline/token/token_counter.rs:31-42) - for tokenizers trained here in the Llama-3 layout
(patterns A and B, ignore_merges on and off, 256 added tokens), over the synthetic corpora, the
adversarial pool, fuzz text of the patterns' corner cases and the edge documents; the lane split
must be exact; the rules' contraction set and character classes must be the library's; and the
emulated device pipeline's token counts and metadata column must equal the CPU path's.
"""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bpe_split_corpus as bc  # noqa: E402

from textblaster_amd import native  # noqa: E402
from textblaster_amd.models.tokenizer import (BPE_SPLIT_A, BPE_SPLIT_B, SPLIT_PATTERN_A, SPLIT_PATTERN_B,  # noqa: E402
                                              TokenCounterModel, build_bpe_spec, bytes_to_unicode, count_spec,
                                              train_synthetic_split_bpe)
from textblaster_amd.utils import synth  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [("A", True), ("A", False), ("B", True), ("B", False)]


@pytest.fixture(scope="module")
def toks(tmp_path_factory):
    d = tmp_path_factory.mktemp("tok")
    return {(p, im): train_synthetic_split_bpe(str(d / f"split4k_{p}{int(im)}.json"), vocab_size=4000, pattern=p,
                                               ignore_merges=im, n_docs=1500, seed=2) for p, im in VARIANTS}


@pytest.fixture(scope="module")
def docs_host():
    return bc.corpus()


def raw_and_full(model, docs, chunk=0):
    data, off = synth.pack(docs)
    sp = model.bpe_spec()
    assert sp is not None
    return count_spec(sp, data, off, 4, chunk), model.count_native(data, off, 4)


# ---- 1. specs -----------------------------------------------------------------------------------
def test_spec_accepts_the_layout_and_rejects_its_variants(toks):
    for (p, im), path in toks.items():
        tj = json.load(open(path))
        assert len(tj["added_tokens"]) == 256 and tj["model"]["ignore_merges"] is im
        assert tj["pre_tokenizer"]["pretokenizers"][0]["pattern"]["Regex"] == {"A": SPLIT_PATTERN_A,
                                                                               "B": SPLIT_PATTERN_B}[p]
        sp = build_bpe_spec(tj)
        assert sp is not None and sp.kind == {"A": BPE_SPLIT_A, "B": BPE_SPLIT_B}[p] and sp.ignore_merges is im
        assert len(sp.added_off) == 257 and sp.post_add == 1
        assert (sp.vslots is not None and sp.vlongest >= 2) if im else sp.vslots is None
        m = TokenCounterModel(path)
        assert m.device_spec() is m.bpe_spec() and m.wordpiece_spec() is None
    tj = json.load(open(toks[("A", True)]))
    split, bl = tj["pre_tokenizer"]["pretokenizers"]

    def with_pre(s=split, b=bl):
        return dict(tj, pre_tokenizer=dict(tj["pre_tokenizer"], pretokenizers=[s, b]))

    assert build_bpe_spec(with_pre()) is not None
    none = [
        with_pre(s=dict(split, pattern={"Regex": SPLIT_PATTERN_A.replace("{1,3}", "{1,4}")})),
        with_pre(s=dict(split, pattern={"Regex": SPLIT_PATTERN_A + "|x"})),
        with_pre(s=dict(split, pattern={"String": SPLIT_PATTERN_A})),
        with_pre(s=dict(split, behavior="Removed")),
        with_pre(s=dict(split, invert=True)),
        with_pre(b=dict(bl, add_prefix_space=True)),
        with_pre(b=dict(bl, use_regex=True)),
        dict(tj, pre_tokenizer=dict(tj["pre_tokenizer"], pretokenizers=[bl, split])),
        dict(tj, pre_tokenizer=split),
        dict(tj, normalizer={"type": "NFC"}),
        dict(tj, truncation={"max_length": 8, "strategy": "LongestFirst", "stride": 0, "direction": "Right"}),
        dict(tj, model=dict(tj["model"], byte_fallback=True)),
        dict(tj, model=dict(tj["model"], dropout=0.1)),
        dict(tj, post_processor={"type": "SomethingElse"}),
        dict(tj, added_tokens=[dict(tj["added_tokens"][0], content=f"<|t{i}|>", id=5000 + i) for i in range(1025)]),
        dict(tj, added_tokens=[dict(tj["added_tokens"][0], content="x" * 65537)]),
    ]
    for v in none:
        assert build_bpe_spec(v) is None
    assert build_bpe_spec(dict(tj, added_tokens=[dict(tj["added_tokens"][0], content=f"<|t{i}|>", id=5000 + i)
                                                 for i in range(1024)])) is not None


def test_gpt2_family_keeps_its_spec():
    gpt2 = os.path.join(REPO, "tests", "fixtures", "tokenizers", "gpt2", "tokenizer.json")
    sp = TokenCounterModel(gpt2).bpe_spec()
    assert sp.kind == 0 and not sp.ignore_merges and sp.vslots is None
    tj = json.load(open(gpt2))
    assert build_bpe_spec(dict(tj, model=dict(tj["model"], ignore_merges=True))) is None


# ---- 2. counts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern,ignore_merges", VARIANTS)
def test_counts_equal_tokenizers(toks, docs_host, pattern, ignore_merges):
    docs, host = docs_host
    m = TokenCounterModel(toks[(pattern, ignore_merges)])
    raw, full = raw_and_full(m, docs)
    ref = np.array(m.count(docs))
    ok = raw >= 0
    bad = np.nonzero(ok & (raw != ref))[0]
    assert not len(bad), [(docs[k][:60], int(raw[k]), int(ref[k])) for k in bad[:5]]
    assert set(raw[~ok].tolist()) <= {-2}
    np.testing.assert_array_equal(full, ref)
    # the documents built to go to the host do; of the others at most 1 % may (the reference alone
    # sends none: no pre-token over 2048 bytes, no added-token text)
    assert all(raw[k] == -2 for k in host)
    nbase = len(bc.base_corpus())
    assert nbase > 2500 and (~ok[:nbase]).mean() <= 0.01
    rest = np.setdiff1d(np.arange(len(docs)), host)
    assert (~ok[rest]).mean() <= 0.01
    by_text = {t: int(raw[k]) for k, t in enumerate(docs)}
    assert by_text[""] == 1 and by_text["'"] == 2 and by_text["a" * 2048] > 0  # (<|begin_of_text|> counts)
    # pattern A cuts number runs in threes, B into single numbers
    d3 = m.count(["123"])[0] - 1
    assert by_text["1234"] == 1 + (d3 + 1 if pattern == "A" else 4)


def test_invalid_utf8_goes_to_the_host(toks):
    m = TokenCounterModel(toks[("A", True)])
    sp, fine = m.bpe_spec(), m.count(["fine text"])[0]
    docs = [b"abc \xff def", b"abc \xc3", b"\x80abc", b"ab \xe2\x82 cd" + b"x" * 40, b"fine text",
            b"x" * 15 + b"\xc3\xa9\xa9", b"12345678901234567\xed\xa0\x80"]
    data = np.frombuffer(b"".join(docs), dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(d) for d in docs]).astype(np.int64)
    for chunk in (0, 1, 16):
        assert count_spec(sp, data, off, 1, chunk).tolist() == [-2, -2, -2, -2, fine, -2, -2]


# ---- 3. the lane split --------------------------------------------------------------------------
@pytest.mark.parametrize("pattern,ignore_merges", [("A", True), ("B", False)])
def test_lane_ranges_sum_to_the_document(toks, pattern, ignore_merges):
    """The tokens that start in [sync(s0), sync(s1)) over a partition of the document give the
    sequential count: sync points are token starts whatever precedes them."""
    docs = bc.fuzz(3000, 5) + bc.prefixes() + bc.EDGES + bc.HOST_DOCS + ["1234567,.;: 89!? " * 40]
    m = TokenCounterModel(toks[(pattern, ignore_merges)])
    raw, _ = raw_and_full(m, docs)
    for chunk in (1, 2, 3, 5, 16, 17, 64):
        np.testing.assert_array_equal(raw_and_full(m, docs, chunk)[0], raw)


# ---- 4. ignore_merges ---------------------------------------------------------------------------
def _unreachable_words(path):
    """Vocabulary entries (as text) that the merges alone do not reach."""
    from tokenizers import Tokenizer

    tj = json.load(open(path))
    tj["model"]["ignore_merges"] = False
    plain = Tokenizer.from_str(json.dumps(tj))
    u2b = {ch: i for i, ch in enumerate(bytes_to_unicode())}
    out = []
    for w in tj["model"]["vocab"]:
        try:
            t = bytes(u2b[ch] for ch in w).decode("utf-8")
        except (KeyError, UnicodeDecodeError):
            continue
        if len(t) > 1 and t.isalpha() and len(plain.encode(t, add_special_tokens=False).tokens) > 1:
            out.append(t)
    return out


def test_ignore_merges_is_honoured(toks, tmp_path):
    # a hand-written vocabulary: "abc" = "ab" + "c" is an entry, but "b c" merges first
    tj = json.load(open(toks[("A", True)]))
    vocab = {ch: i for i, ch in enumerate(bytes_to_unicode())}
    for w in ("bc", "ab", "abc"):
        vocab[w] = len(vocab)
    tj["model"].update(vocab=vocab, merges=[["b", "c"], ["a", "b"], ["ab", "c"]])
    tj.update(added_tokens=[], post_processor=None)
    words = ["abc", " abc", "abcabc", "xabc abc!"]
    for im, want in ((True, 1), (False, 2)):
        tj["model"]["ignore_merges"] = im
        p = tmp_path / f"hand{int(im)}.json"
        p.write_text(json.dumps(tj))
        m = TokenCounterModel(str(p))
        raw, _ = raw_and_full(m, words)
        assert raw.tolist() == m.count(words) and raw[0] == want
    # and in the trained vocabulary, where training left such an entry
    for t in _unreachable_words(toks[("A", True)])[:20]:
        on, off_ = TokenCounterModel(toks[("A", True)]), TokenCounterModel(toks[("A", False)])
        a, b = raw_and_full(on, [t])[0], raw_and_full(off_, [t])[0]
        assert a[0] == on.count([t])[0] == 2 and b[0] == off_.count([t])[0] > 2


# ---- 5. the rules' contraction set and classes ---------------------------------------------------
def _ends(text, kind):
    e = native.host().bpe_split_ends(text.encode("utf-8"), kind)
    return None if e is None else e.tolist()


def _library_ends(sp, text):
    cum = np.cumsum([0] + [len(c.encode("utf-8")) for c in text])
    return [int(cum[e]) for _, (_, e) in sp.pre_tokenize_str(text)]


def test_contractions_fold_case_as_the_library_does():
    """(?i:...) over every code point whose case mappings change it, probed as "x'" + c + "t": the
    pieces are the library's, and the code points that close a contraction there are the ASCII
    letters and U+017F."""
    from tokenizers import Regex, pre_tokenizers

    c1, c2 = native.host().bpe_classes()

    def is_letter(cp):
        return (int(c2[int(c1[cp >> 7]) * 8 + ((cp & 127) >> 4)]) >> (2 * (cp & 15))) & 3 == 1

    for kind, pat in ((BPE_SPLIT_A, SPLIT_PATTERN_A), (BPE_SPLIT_B, SPLIT_PATTERN_B)):
        sp = pre_tokenizers.Split(Regex(pat), behavior="isolated", invert=False)
        hits = []
        for cp in range(0x110000):
            if 0xD800 <= cp < 0xE000:
                continue
            c = chr(cp)
            if c.lower() == c and c.upper() == c and c.casefold() == c:
                continue
            t = "x'" + c + "t"
            want = _library_ends(sp, t)
            assert _ends(t, kind) == want, hex(cp)
            if want[:2] == [1, 2 + len(c.encode("utf-8"))] and len(want) == 3 and is_letter(cp):
                hits.append(c)
        # (for a letter c, "x'" + c + "t" has the pieces x, 'c, t only when 'c is a contraction: a
        # letter that closes none joins the run 'ct. Circled letters and U+0345 are no letters to
        # the regex: 'c is then a run of other code points)
        assert sorted(hits) == sorted("sStTmMdD\u017f")
    for t in ("x'S", "x'LL", "x'Re y'vE", "x'ſt", "'Ⓐ", "x'\u0345t", "'\u212a", "I'Ll"):
        assert _ends(t, BPE_SPLIT_A) == _library_ends(sp, t), t


def test_rules_examples():
    """The examples the rules were written from."""
    def pieces(t, kind=BPE_SPLIT_A):
        b, s, out = t.encode("utf-8"), 0, []
        for e in _ends(t, kind):
            out.append(b[s:e].decode("utf-8"))
            s = e
        return out

    assert pieces("x'ſt") == ["x", "'ſ", "t"]
    assert pieces("!abc") == ["!abc"] and pieces("\tabc") == ["\tabc"] and pieces("\u00a0b") == ["\u00a0b"]
    assert pieces("x!abc") == ["x", "!abc"] and pieces("!!abc") == ["!!", "abc"] and pieces(" !abc") == [" !", "abc"]
    assert pieces("12345") == ["123", "45"] and pieces("12345", BPE_SPLIT_B) == list("12345")
    assert pieces(" 12") == [" ", "12"] and pieces("²٣") == ["²٣"]
    assert pieces("\n\n  abc  \n x") == ["\n\n", " ", " abc", "  \n", " x"]
    assert pieces(" !!\r\n\nx") == [" !!\r\n\n", "x"]


def test_class_table_equals_a_probe_of_the_split_pattern():
    """bpe_classes.inc was generated from the ByteLevel regex; the Split patterns run in the same
    engine. A sample: every code point the table classes whitespace or number, and every 61st of
    the rest (tools/gen_bpe_classes.py --check-split compares them all)."""
    spec = importlib.util.spec_from_file_location("gen_bpe_classes", os.path.join(REPO, "tools", "gen_bpe_classes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    c1, c2 = native.host().bpe_classes()
    c1, c2 = c1.astype(np.int64), c2.astype(np.int64)
    cp = np.arange(0x110000)
    table = (c2[c1[cp >> 7] * 8 + ((cp & 127) >> 4)] >> (2 * (cp & 15))) & 3
    cps = [int(c) for c in cp if not 0xD800 <= c < 0xE000 and (table[c] >= 2 or c % 61 == 0 or c < 0x300)]
    assert len(cps) > 15000
    fresh = gen.probe_split(cps)
    diff = [(hex(c), int(table[c]), f) for c, f in zip(cps, fresh) if table[c] != f]
    assert not diff, diff[:10]


# ---- 6. the emulated device pipeline ------------------------------------------------------------
def test_emulated_device_token_counts_equal_cpu(toks):
    """Engine(emulate) with a trailing TokenCounter on a pattern A tokenizer: the counts come from
    the kernels' algorithm over the kept outputs, K18 formats the metadata column (no host
    fallback), and the outputs equal the CPU path's."""
    from test_bpe import _cfg
    from test_emulated_device_path import outputs

    from textblaster_amd.pipeline.engine import Engine
    from textblaster_amd.utils import metrics

    tok = toks[("A", True)]
    docs = synth.make_corpus(2500, 900, seed=12) + bc.fuzz(200, 13)
    data, off = synth.pack(docs)
    eng = Engine(_cfg(), backend="emulate", nthreads=4, keep_reasons=True, tokenizer_file=tok)
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
    b = Engine(_cfg(), backend="cpu", nthreads=4, keep_reasons=True, tokenizer_file=tok,
               segmentation="icu").process(data, off)
    np.testing.assert_array_equal(a.status, b.status)
    oa, ob = outputs(a), outputs(b)
    assert oa == ob
    kept_meta = [m for k, t, m in oa.values() if k == "kept"]
    assert kept_meta and all(b'"token_count"' in m for m in kept_meta)


def test_device_tokens_off_leaves_split_bpe_to_the_host(toks, monkeypatch):
    from test_bpe import _cfg

    from textblaster_amd.pipeline.engine import Engine

    monkeypatch.setenv("TB_TUNE", "device_tokens=0")
    eng = Engine(_cfg(), backend="emulate", nthreads=2, tokenizer_file=toks[("A", True)])
    assert not eng.device_runner.bpe
