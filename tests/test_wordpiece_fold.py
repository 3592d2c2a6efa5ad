"""The folding WordPiece counter (csrc/common/wordpiece.h wpf_*; device kernel k_wp_count_fold):
uncased / accent-stripping BERT tokenizers counted natively beyond ASCII.

The fold table (csrc/common/wp_fold.inc) must equal a fresh probe of the `tokenizers` library. The
native counter with the folding spec must give exactly the library's token counts for tokenizers
trained here in every mode (lowercase + strip_accents, lowercase alone, strip_accents alone, without
clean_text, without handle_chinese_chars) and the checked-in bert-base-uncased fixture, and leave to
the host exactly the documents with an added token's text or a code point whose place NFD may
change - so that a fallback cannot hide a miscount. The lane split must equal the sequential
count, and the emulated device pipeline must send no document of the synthetic corpus to the host
tokenizer."""
import importlib.util
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wordpiece_corpus as wc  # noqa: E402
import wordpiece_fold_corpus as fc  # noqa: E402

from textblaster_amd import native  # noqa: E402
from textblaster_amd.models.tokenizer import TokenCounterModel, count_spec  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BERT_FIXTURE = os.path.join(REPO, "tests", "fixtures", "tokenizers", "bert-base-uncased", "tokenizer.json")


@pytest.fixture(scope="module")
def toks(tmp_path_factory):
    """name -> (tokenizer file, strip_accents in force)."""
    d = tmp_path_factory.mktemp("tok")
    both = fc.train(str(d / "both.json"), True, None)
    return {
        "both": (both, True),
        "lower": (fc.train(str(d / "lower.json"), True, False), False),
        "strip": (fc.train(str(d / "strip.json"), False, True), True),
        "noclean": (fc.variant(both, str(d / "noclean.json"), clean_text=False), True),
        "nochinese": (fc.variant(both, str(d / "nochinese.json"), handle_chinese_chars=False), True),
        "fixture": (BERT_FIXTURE, True),
    }


@pytest.fixture(scope="module")
def docs():
    synthetic = synth.make_corpus(1500, 1024, seed=21, vocab="zipf", mixed_script=True)
    return wc.corpus("the"), synthetic, fc.pool_docs()


def _gen():
    spec = importlib.util.spec_from_file_location("gen_wp_fold", os.path.join(REPO, "tools", "gen_wp_fold.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


# ---- 1. the table -------------------------------------------------------------------------------
CLASS_CHANGERS = [0x1FEF, 0x2260, 0x226E, 0x226F]


def test_fold_table_equals_a_fresh_probe():
    import unicodedata

    gen = _gen()
    f1, f2, fp = native.host().wp_fold_tables()
    assert f1.shape == (3, 0x110000 // 128) and f1.dtype == np.uint16 and f2.dtype == np.uint16
    tables = (f1.reshape(-1), f2, bytes(fp))
    context = [cp for cp in range(0x80, 0x110000) if not 0xD800 <= cp < 0xE000
               and unicodedata.combining(chr(cp)) and unicodedata.category(chr(cp)) != "Mn"]
    rng = random.Random(17)
    cps = (list(range(0x3001)) + list(range(0xAC00, 0xAC81)) + CLASS_CHANGERS + context
           + [rng.randrange(0x110000) for _ in range(20000)])
    fresh = gen.probe(cps)
    diff = [(hex(c), m, gen.lookup(tables, m, c), row[m]) for c, row in zip(cps, fresh) for m in range(3)
            if gen.lookup(tables, m, c) != row[m]]
    assert not diff, diff[:10]
    by = dict(zip(cps, fresh))
    # the committed file is what the module was built from
    assert tuple(bytes(np.asarray(t)) if not isinstance(t, bytes) else t for t in tables) == tuple(
        bytes(np.asarray(t, dtype=np.uint16)) if i < 2 else t for i, t in enumerate(gen.read_inc()))
    # the known shapes: a -> a, drop, two jamo, i + U+0307 in lower-only, class from the output
    assert by[0xE5] == (None, (b"a", 0, 0), (b"a", 0, 0)) and by[0xC6][0] == ("\u00e6".encode(), 0, 0)
    assert by[0x301] == (None, (b"", 1, 1), (b"", 1, 1))
    assert by[0xAC00][0] is None and by[0xAC00][2] == ("\u1100\u1161".encode(), 0, 0)
    assert by[0x130] == (("i\u0307".encode(), 0, 0), (b"I", 0, 0), (b"i", 0, 0))
    for c, o in zip(CLASS_CHANGERS, (b"`", b"=", b"<", b">")):
        assert by[c][2] == (o, 3, 3), hex(c)
    # code points NFD may move: those the library's tables know are "host"; one that is newer than
    # its tables must stay where it is between two marks the library would otherwise reorder
    for c in (0x1B44, 0x1BAA, 0x1BF2, 0x1BF3, 0x302E, 0x302F, 0xA953, 0xA9C0, 0x111C0):
        assert by[c] == (None, "host", "host"), hex(c)
    strip = gen.normalizer(False, False, True).normalize_str
    for c in context:
        if by[c][1] != "host":
            s = "\u302f" + chr(c) + "\u1b44"
            assert by[c] == (None, None, None) and strip(s) == s, hex(c)
    assert sum(by[c][1] == "host" for c in context) >= 20
    differing, compared = gen.concat_differences(lambda m, c: gen.lookup(tables, m, c), 5000, 3)
    assert compared > 10000 and differing == 0


# ---- 2. counts ----------------------------------------------------------------------------------
_REF = {}


def library_counts(model, texts, key):
    if key not in _REF:
        _REF[key] = np.array(model.count(texts))
        _REF[key].setflags(write=False)
    return _REF[key]


def check_exact(model, texts, key, strip):
    """Raw folding counts equal the library's wherever they are >= 0, and the documents left to
    the host are exactly the predicted ones."""
    sp = model.wordpiece_fold_spec()
    assert sp is not None and sp.fold == (1 if sp.flags & 1 else 0) + (2 if strip else 0) and sp.self_bit == 0
    data, off = synth.pack(texts)
    raw = count_spec(sp, data, off, 4)
    ref = library_counts(model, texts, key)
    ok = raw >= 0
    bad = np.nonzero(ok & (raw != ref))[0]
    assert not len(bad), [(texts[k][:60], int(raw[k]), int(ref[k])) for k in bad[:5]]
    assert set(raw[~ok].tolist()) <= {-2}
    host = fc.needs_host(strip, model.path)
    assert np.nonzero(~ok)[0].tolist() == [k for k, t in enumerate(texts) if host(t)]
    return raw


def test_vocabulary_splits_syllables(toks):
    from tokenizers import Tokenizer

    for name in ("both", "strip"):
        assert fc.splits_a_syllable(Tokenizer.from_file(toks[name][0])), name
    lower = Tokenizer.from_file(toks["lower"][0]).get_vocab()
    assert "\u00e5" in lower or "##\u00e5" in lower  # non-ASCII pieces exist in the lower-only vocabulary
    assert "##\u0307" in lower


@pytest.mark.parametrize("name", ["both", "lower", "strip", "noclean", "nochinese", "fixture"])
def test_fold_counts_equal_tokenizers(toks, docs, name):
    path, strip = toks[name]
    m = TokenCounterModel(path)
    general, synthetic, pool = docs
    check_exact(m, general, name + "-general", strip)
    raw = check_exact(m, synthetic, name + "-synth", strip)
    assert (raw >= 0).all()  # nothing of the synthetic corpus is left to the host
    check_exact(m, pool, name + "-pool", strip)
    host = fc.needs_host(strip, path)
    assert [t for t in pool if host(t) and "[" not in t] == (fc.CONTEXT if strip else [])
    # what the identity spec leaves to the host and the folding spec counts (lowercase alone
    # changes only the capitals among the non-ASCII letters, so the corpus in capitals as well)
    upper = [t.upper() for t in synthetic]
    raw_upper = check_exact(m, upper, name + "-upper", strip)
    assert (raw_upper >= 0).all()
    data, off = synth.pack(synthetic + upper)
    ident = count_spec(m.wordpiece_spec(), data, off, 4)
    assert ((ident == -2) & (np.concatenate([raw, raw_upper]) >= 0)).sum() > 1000
    data, off = synth.pack(synthetic)
    assert m.device_spec() is m.wordpiece_fold_spec()
    np.testing.assert_array_equal(m.count_native(data, off, 4), library_counts(m, synthetic, name + "-synth"))


def test_cased_spec_is_unchanged(tmp_path):
    from textblaster_amd.models.tokenizer import train_synthetic_wordpiece

    m = TokenCounterModel(train_synthetic_wordpiece(str(tmp_path / "cased.json"), vocab_size=1000, n_docs=300, seed=2))
    assert m.wordpiece_fold_spec() is m.wordpiece_spec() and m.wordpiece_spec().fold == 0


# ---- 3. the lane split --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["both", "lower", "strip"])
def test_lane_ranges_sum_to_the_document(toks, docs, name):
    m = TokenCounterModel(toks[name][0])
    sp = m.wordpiece_fold_spec()
    texts = docs[2] + docs[0][-600:]
    data, off = synth.pack(texts)
    raw = count_spec(sp, data, off, 4)
    for chunk in (1, 3, 16, 1000):
        np.testing.assert_array_equal(count_spec(sp, data, off, 4, chunk), raw)


def test_invalid_utf8_goes_to_the_host(toks):
    m = TokenCounterModel(toks["both"][0])
    sp, fine = m.wordpiece_fold_spec(), m.count(["fin\u00e9 t\u00c5xt"])[0]
    texts = [b"abc \xff def", b"abc \xc3", b"\x80abc", b"ab \xe2\x82 cd" + b"x" * 40, "fin\u00e9 t\u00c5xt".encode(),
             b"x" * 15 + b"\xc3\xa9\xa9", b"\xea\xb0"]
    data = np.frombuffer(b"".join(texts), dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(d) for d in texts]).astype(np.int64)
    for chunk in (0, 1, 16):
        assert count_spec(sp, data, off, 1, chunk).tolist() == [-2, -2, -2, -2, fine, -2, -2]


# ---- 4. the emulated device pipeline ------------------------------------------------------------
def test_emulated_engine_counts_uncased_text_natively(toks):
    from test_emulated_device_path import outputs
    from test_wordpiece import _cfg

    from textblaster_amd.pipeline.engine import Engine
    from textblaster_amd.utils import metrics

    tok = toks["both"][0]
    texts = synth.make_corpus(2500, 900, seed=12)
    nordic = "\u00e5\u00e4\u00f6\u00c5\u00c4\u00d6\u00c6\u00d8\u00e6\u00f8"
    assert sum(any(c in t for c in nordic) for t in texts) > 1000
    data, off = synth.pack(texts)
    eng = Engine(_cfg(), backend="emulate", nthreads=4, keep_reasons=True, tokenizer_file=tok)
    assert eng.device_runner.resolve_blob is not None and eng.device_runner.bpe
    res = eng.submit(data, off)
    h0, d0 = metrics.BPE_HOST_DOCS_TOTAL._value.get(), metrics.BPE_DEVICE_DOCS_TOTAL._value.get()
    f0 = metrics.DEVICE_META_FALLBACK_TOTAL._value.get()
    a = eng.finish(res)
    nh = metrics.BPE_HOST_DOCS_TOTAL._value.get() - h0
    nd = metrics.BPE_DEVICE_DOCS_TOTAL._value.get() - d0
    assert nh == 0 and nd == a.n_kept and nd > 1000
    assert metrics.DEVICE_META_FALLBACK_TOTAL._value.get() == f0
    b = Engine(_cfg(), backend="cpu", nthreads=4, keep_reasons=True, tokenizer_file=tok,
               segmentation="icu").process(data, off)
    np.testing.assert_array_equal(a.status, b.status)
    oa, ob = outputs(a), outputs(b)
    assert oa == ob
    kept_meta = [m for k, t, m in oa.values() if k == "kept"]
    assert kept_meta and all(b'"token_count"' in m for m in kept_meta)
