"""TokenCounter's counter for the case-aware split patterns (csrc/common/bpe_case.h: o200k_base = C,
Tekken = D; kernels k_bpe_case_count / k_bpe_case_long) and the NFC gate of the split-regex family
(csrc/common/bpe.h bpe_nfc_range, csrc/common/nfc_qc.inc: Qwen2's files; the _nfc count kernels).

The native counter (the kernels' algorithm compiled for the host) must give exactly the `tokenizers`
library's ``len(encode(text, add_special_tokens=True).tokens)`` for tokenizers trained here, its
pre-token boundaries must be the library's Split's, the lane split must be exact, and behind an NFC
normalizer every document the library's NFC changes must come back -2, while text that is in NFC
and holds no code point that may compose must be counted."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bpe_case_corpus as cc  # noqa: E402
import bpe_split_corpus as bc  # noqa: E402
from adversarial import adversarial_corpus  # noqa: E402

from textblaster_amd import native  # noqa: E402
from textblaster_amd.models.tokenizer import (BPE_CASE_C, BPE_CASE_D, BPE_SPLIT_A, BPE_SPLIT_B,  # noqa: E402
                                              SPLIT_PATTERN_C, SPLIT_PATTERN_D, TokenCounterModel, build_bpe_spec,
                                              count_spec, train_synthetic_split_bpe)
from textblaster_amd.utils import synth  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [("C", True), ("C", False), ("D", True), ("D", False)]
KIND = {"A": BPE_SPLIT_A, "B": BPE_SPLIT_B, "C": BPE_CASE_C, "D": BPE_CASE_D}


@pytest.fixture(scope="module")
def toks(tmp_path_factory):
    d = tmp_path_factory.mktemp("tok")
    out = {(p, im, False): train_synthetic_split_bpe(str(d / f"case4k_{p}{int(im)}.json"), vocab_size=4000, pattern=p,
                                                     ignore_merges=im, n_docs=1500, seed=2) for p, im in VARIANTS}
    for p in "ABC":
        out[(p, False, True)] = train_synthetic_split_bpe(str(d / f"nfc4k_{p}.json"), vocab_size=4000, pattern=p,
                                                          ignore_merges=False, n_docs=1500, seed=2, nfc=True)
    return out


@pytest.fixture(scope="module")
def docs_host():
    return cc.corpus()


@pytest.fixture(scope="module")
def nfc():
    from tokenizers import normalizers

    return normalizers.NFC().normalize_str


def raw_counts(model, docs, chunk=0):
    data, off = synth.pack(docs)
    sp = model.bpe_spec()
    assert sp is not None
    return count_spec(sp, data, off, 4, chunk)


# ---- 1. specs -----------------------------------------------------------------------------------
def test_spec_detection(toks):
    for (p, im, nf), path in toks.items():
        tj = json.load(open(path))
        assert (tj["normalizer"] == {"type": "NFC"}) if nf else tj["normalizer"] is None
        sp = build_bpe_spec(tj, nfc=True)
        assert sp is not None and sp.kind == KIND[p] and sp.nfc is nf and sp.ignore_merges is im
        # without the gate asked for, a normalizer means no spec
        assert (build_bpe_spec(tj) is None) if nf else (build_bpe_spec(tj).kind == KIND[p])
        assert len(sp.added_off) == 257 and sp.post_add == 1
        m = TokenCounterModel(path)
        assert m.device_spec() is m.bpe_spec() and m.bpe_spec().kind == KIND[p] and m.bpe_spec().nfc is nf
    tj = json.load(open(toks[("C", True, False)]))
    assert tj["pre_tokenizer"]["pretokenizers"][0]["pattern"]["Regex"] == SPLIT_PATTERN_C
    assert build_bpe_spec(dict(tj, normalizer={"type": "NFC"}), nfc=True).nfc
    split, bl = tj["pre_tokenizer"]["pretokenizers"]
    none = [
        dict(tj, normalizer={"type": "NFKC"}),
        dict(tj, normalizer={"type": "Sequence", "normalizers": [{"type": "NFC"}]}),
        dict(tj, normalizer={"type": "NFC", "extra": 1}),
        dict(tj, pre_tokenizer=dict(tj["pre_tokenizer"], pretokenizers=[
            dict(split, pattern={"Regex": SPLIT_PATTERN_C.replace("/]*", "]*")}), bl])),
        dict(tj, pre_tokenizer=dict(tj["pre_tokenizer"], pretokenizers=[
            dict(split, pattern={"Regex": SPLIT_PATTERN_D + "|x"}), bl])),
        dict(tj, normalizer={"type": "NFC"},
             added_tokens=[dict(tj["added_tokens"][0], normalized=True)] + tj["added_tokens"][1:]),
        dict(tj, model=dict(tj["model"], byte_fallback=True)),
    ]
    for v in none:
        assert build_bpe_spec(v, nfc=True) is None
    # without a normalizer a token matched on normalised text is matched on the text itself
    assert build_bpe_spec(dict(tj, added_tokens=[dict(tj["added_tokens"][0], normalized=True)]), nfc=True) is not None
    # a GPT-2 ByteLevel file with a normalizer stays on the host
    gpt2 = json.load(open(os.path.join(REPO, "tests", "fixtures", "tokenizers", "gpt2", "tokenizer.json")))
    assert build_bpe_spec(gpt2, nfc=True) is not None
    assert build_bpe_spec(dict(gpt2, normalizer={"type": "NFC"}), nfc=True) is None


# ---- 2. counts and boundaries -------------------------------------------------------------------
@pytest.mark.parametrize("pattern,ignore_merges", VARIANTS)
def test_counts_equal_tokenizers(toks, docs_host, pattern, ignore_merges):
    docs, host = docs_host
    m = TokenCounterModel(toks[(pattern, ignore_merges, False)])
    raw = raw_counts(m, docs)
    ref = np.array(m.count(docs))
    ok = raw >= 0
    bad = np.nonzero(ok & (raw != ref))[0]
    assert not len(bad), [(docs[k][:60], int(raw[k]), int(ref[k])) for k in bad[:5]]
    assert set(raw[~ok].tolist()) <= {-2}
    data, off = synth.pack(docs)
    np.testing.assert_array_equal(m.count_native(data, off, 4), ref)
    assert all(raw[k] == -2 for k in host)
    rest = np.setdiff1d(np.arange(len(docs)), host)
    assert (~ok[rest]).mean() <= 0.01
    by_text = {t: int(raw[k]) for k, t in enumerate(docs)}
    assert by_text[""] == 1 and by_text["a" * 2048] > 0
    d3 = m.count(["123"])[0] - 1
    assert by_text["1234"] == 1 + (d3 + 1 if pattern == "C" else 4)


def _ends(text, kind):
    e = native.host().bpe_split_ends(text.encode("utf-8"), kind)
    return None if e is None else e.tolist()


def _library_ends(sp, text):
    cum = np.cumsum([0] + [len(c.encode("utf-8")) for c in text])
    return [int(cum[e]) for _, (_, e) in sp.pre_tokenize_str(text)]


def test_table_of_cases():
    from tokenizers import Regex, pre_tokenizers

    sp = pre_tokenizers.Split(Regex(SPLIT_PATTERN_C), behavior="isolated", invert=False)
    for text, pieces in cc.CASES:
        assert [p for p, _ in sp.pre_tokenize_str(text)] == pieces, text
        b, s, got = text.encode("utf-8"), 0, []
        for e in _ends(text, BPE_CASE_C):
            got.append(b[s:e].decode("utf-8"))
            s = e
        assert got == pieces, text


@pytest.mark.parametrize("kind,pat", [(BPE_CASE_C, SPLIT_PATTERN_C), (BPE_CASE_D, SPLIT_PATTERN_D)], ids=["C", "D"])
def test_boundaries_equal_the_library(kind, pat):
    """Pre-token boundaries, not only their number: a wrong split that gives the same count fails."""
    from tokenizers import Regex, pre_tokenizers

    sp = pre_tokenizers.Split(Regex(pat), behavior="isolated", invert=False)
    texts = [t for t, _ in cc.CASES] + cc.fuzz(3000, 6) + bc.fuzz(1000, 5) + cc.prefixes() + bc.prefixes()
    bad = [t for t in texts if _ends(t, kind) != _library_ends(sp, t)]
    assert not bad, [(t, _ends(t, kind), _library_ends(sp, t)) for t in bad[:3]]


def test_class_table_equals_a_probe_of_pattern_c():
    """bpe_case_classes.inc against a fresh probe: every code point the table classes U, l, M, number
    or whitespace, everything below U+0300, and every 61st of the rest (tools/gen_bpe_classes.py
    --check-case compares them all)."""
    spec = importlib.util.spec_from_file_location("gen_bpe_classes", os.path.join(REPO, "tools", "gen_bpe_classes.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    c1, c2 = native.host().bpe_case_classes()
    c1, c2 = c1.astype(np.int64), c2.astype(np.int64)
    cp = np.arange(0x110000)
    table = (c2[c1[cp >> 7] * 16 + ((cp & 127) >> 3)] >> (4 * (cp & 7))) & 15
    cps = [int(c) for c in cp if not 0xD800 <= c < 0xE000 and (table[c] not in (0, 3) or c % 61 == 0 or c < 0x300)]
    assert len(cps) > 20000 and set(table.tolist()) == set(range(7))
    fresh = gen.probe_case(cps)
    diff = [(hex(c), int(table[c]), f) for c, f in zip(cps, fresh) if table[c] != f]
    assert not diff, diff[:10]


# ---- 3. the lane split --------------------------------------------------------------------------
@pytest.mark.parametrize("key", [("C", True, False), ("D", False, False), ("B", False, True), ("C", False, True)],
                         ids=["C", "D", "B-nfc", "C-nfc"])
def test_lane_ranges_sum_to_the_document(toks, docs_host, key):
    """The tokens that start in [sync(s0), sync(s1)) over a partition of the document give the
    sequential count, and the NFC gate over the partition decides as over the whole document."""
    docs = docs_host[0] + cc.NFC_CLEAN + ["1234567,.;: 89!? " * 40, "ab'cd'ef'gh'" * 30, "AbcDEFgh" * 20, "あAあB" * 20]
    m = TokenCounterModel(toks[key])
    raw = raw_counts(m, docs)
    for chunk in (16, 17, 32, 100):
        np.testing.assert_array_equal(raw_counts(m, docs, chunk), raw)
    small = cc.fuzz(600, 8) + cc.prefixes() + [t for t, _ in cc.CASES] + cc.NFC_CLEAN
    raw = raw_counts(m, small)
    for chunk in (1, 2, 3, 5):
        np.testing.assert_array_equal(raw_counts(m, small, chunk), raw)


# ---- 4. the NFC gate ----------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["A", "B", "C"])
def test_nfc_soundness(toks, docs_host, nfc, pattern):
    """Every document the library's NFC changes comes back -2; the counted ones equal the library."""
    docs = docs_host[0] + ["é", "aְִ", "가", "Å", "ẋ̣", "ẋ̣"]
    m = TokenCounterModel(toks[(pattern, False, True)])
    raw = raw_counts(m, docs)
    changed = np.array([nfc(t) != t for t in docs])
    assert changed.sum() > 100 and not (changed & (raw >= 0)).any()
    ref = np.array(m.count(docs))
    ok = raw >= 0
    assert ok.sum() > 2000 and not (ok & (raw != ref)).any()
    data, off = synth.pack(docs)
    np.testing.assert_array_equal(m.count_native(data, off, 4), ref)


def test_nfc_tightness(toks, nfc):
    """The gate may not pass by sending everything to the host."""
    m = TokenCounterModel(toks[("B", False, True)])
    for docs in (synth.make_corpus(1500, 1024, seed=3), synth.make_corpus(400, 1024, seed=4, vocab="zipf")):
        assert (raw_counts(m, docs) >= 0).all()
    adv = [t for t in adversarial_corpus() if nfc(t) == t]
    # those with invalid UTF-8 or an added token's text go to the host without a normalizer too
    plain = raw_counts(TokenCounterModel(train_synthetic_split_bpe(
        os.path.join(os.path.dirname(toks[("B", False, True)]), "plain4k_B.json"), vocab_size=4000, pattern="B",
        ignore_merges=False, n_docs=1500, seed=2)), adv)
    raw = raw_counts(m, adv)
    share = float(((raw < 0) & (plain >= 0)).mean())
    print(f"adversarial documents in NFC: {len(adv)}, on the host because of the gate: "
          f"{int(((raw < 0) & (plain >= 0)).sum())} ({100 * share:.1f} %), for other reasons: {int((plain < 0).sum())}")
    assert len(adv) > 400 and float((raw < 0).mean()) <= 0.15
    assert all(nfc(t) == t for t in cc.NFC_CLEAN)
    assert (raw_counts(m, cc.NFC_CLEAN) >= 0).all()
    assert nfc("क़") == "क़" and raw_counts(m, ["क़"]).tolist() == [-2]  # a Maybe


def test_nfc_table_rule_equals_the_gate(toks, docs_host):
    """The generated table read from Python (tools/gen_nfc_qc.py identity) decides as the compiled gate."""
    spec = importlib.util.spec_from_file_location("gen_nfc_qc", os.path.join(REPO, "tools", "gen_nfc_qc.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    tab = gen.read_inc()
    t1, t2 = native.host().nfc_qc()
    assert t1.tolist() == list(tab[0]) and t2.tobytes() == tab[1]
    docs = docs_host[0]
    plain = raw_counts(TokenCounterModel(toks[("C", False, False)]), docs)
    gated = raw_counts(TokenCounterModel(toks[("C", False, True)]), docs)
    want = np.where(np.array([gen.identity(tab, t) for t in docs]), plain, -2)
    np.testing.assert_array_equal(gated, want)


# ---- 5. the emulated device pipeline ------------------------------------------------------------
@pytest.mark.parametrize("key", [("B", False, True), ("C", True, False)], ids=["B-nfc", "C"])
def test_emulated_device_token_counts_equal_cpu(toks, key):
    from test_bpe import _cfg
    from test_emulated_device_path import outputs

    from textblaster_amd.pipeline.engine import Engine
    from textblaster_amd.utils import metrics

    tok = toks[key]
    docs = synth.make_corpus(2500, 900, seed=12)
    data, off = synth.pack(docs)
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
