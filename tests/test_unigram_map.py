"""The Unigram counter with the normalizer's replacements applied by the counter itself
(csrc/common/unigram.h unim_*; device kernel k_uni_count_map; TB_TUNE=uni_map=1).

The mapped spec's counter must give exactly the `tokenizers` library's count for every document it
counts, and hand exactly the documents of tests/unigram_map_corpus.py to_host to the library. What
is callable without the map (unigram_spec, device_spec()) stays what it was.
"""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unigram_corpus as uc  # noqa: E402
import unigram_map_corpus as um  # noqa: E402

from textblaster_amd import native  # noqa: E402
from textblaster_amd.models import tokenizer as T  # noqa: E402
from textblaster_amd.models.tokenizer import TokenCounterModel, count_spec  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("unimap")


def _classes(sp):
    cps = np.arange(0x110000)
    return (sp.cls2[sp.cls1[cps >> 7].astype(np.int64) * 32 + ((cps & 127) >> 2)] >> (2 * (cps & 3))) & 3


def _output(sp, c):
    """The record of code point ``c`` in the mapped spec, or None."""
    r = int(sp.map2[int(sp.map1[c >> 7]) * 128 + (c & 127)])
    if r == T.UNI_MAP_NONE:
        return None
    e = int(sp.map_rec[r])
    return bytes(sp.map_pool[e >> 8:(e >> 8) + (e & T.UNI_REC_LEN)])


def test_constants_equal_the_header():
    c = native.host().UNI_CONSTANTS
    assert (c["UNI_MAP"], c["UNI_MAX_MAP_BYTES"], c["UNI_MAP_NONE"]) == (T.UNI_MAP, T.UNI_MAX_MAP_BYTES, T.UNI_MAP_NONE)
    assert (c["UNI_REC_LEN"], c["UNI_REC_JOIN"]) == (T.UNI_REC_LEN, T.UNI_REC_JOIN)
    assert (T.UNI_MAP, T.UNI_MAX_MAP_BYTES, um.MAX_MAP_BYTES) == (3, 32, 32)
    assert c["UNI_HOST"] == 2 and c["UNI_MAX_PIECE_CP"] == T.UNI_MAX_PIECE_CP  # the existing keys stay


# ---- 1. specs -----------------------------------------------------------------------------------
def test_unmapped_spec_is_unchanged(tok_dir):
    for variant in ("H-nmt", "C-nmt-first"):
        m = TokenCounterModel(uc.tokenizer(variant, tok_dir))
        sp = m.unigram_spec()
        before = (sp.cls1.copy(), sp.cls2.copy())
        mp = m.unigram_map_spec()
        assert mp is not sp and mp is m.unigram_map_spec() and mp.mapped and not sp.mapped
        assert m.device_spec() is sp and m.unigram_spec() is sp and m.device_spec(uni_map=True) is mp
        assert (sp.cls1 == before[0]).all() and (sp.cls2 == before[1]).all()
        assert len(sp.map1) == len(sp.map2) == len(sp.map_rec) == len(sp.map_pool) == 0
        assert (_classes(sp) != T.UNI_MAP).all()
        for name in ("slots", "pool", "added", "sp"):
            assert (getattr(sp, name) == getattr(mp, name)).all()
        assert (sp.mask, sp.flags, sp.unk_score, sp.longest_cp, sp.longest, sp.added_off, sp.post_add, sp.layout) == (
            mp.mask, mp.flags, mp.unk_score, mp.longest_cp, mp.longest, mp.added_off, mp.post_add, mp.layout)
    gpt2 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "tokenizers", "gpt2", "tokenizer.json")
    m = TokenCounterModel(gpt2)
    assert m.unigram_map_spec() is None and m.device_spec(uni_map=True) is m.bpe_spec()


def test_class_table_of_the_mapped_spec(tok_dir):
    m = TokenCounterModel(uc.tokenizer("H-nmt", tok_dir))
    old, sp = _classes(m.unigram_spec()), m.unigram_map_spec()
    cls = _classes(sp)
    for c in (0x2026, 0xFB01, 0x01, 0xFF21, 0xA8, 0x958):
        assert cls[c] == T.UNI_MAP and old[c] == T.UNI_HOST, hex(c)
    for c in (0x0301, 0x200D, 0x1161, 0xFDFA, 0xD800):  # joiners, the output over the cap, a surrogate
        assert cls[c] == T.UNI_HOST, hex(c)
    for k in (T.UNI_KEEP, T.UNI_SPACE):
        assert ((cls == k) == (old == k)).all()
    assert ((cls == T.UNI_MAP) <= (old == T.UNI_HOST)).all()
    n_map = int((cls == T.UNI_MAP).sum())
    print(f"nmt_nfkc, layout H: {n_map} map code points, {len(sp.map_rec)} records, pool {len(sp.map_pool)} B, "
          f"map1 {sp.map1.nbytes} B, map2 {sp.map2.nbytes} B")
    assert 4000 < n_map < 5000  # 4,770 + 30 by the probe of all scalar values, less what fails a condition
    # records: the output as the later steps see it, white space as 0x20; a drop is empty
    assert _output(sp, 0x2026) == b"..." and _output(sp, 0xFB01) == b"fi" and _output(sp, 0xFF21) == b"A"
    assert _output(sp, 0x01) == b"" and _output(sp, 0xA8) == b" \xcc\x88"
    assert _output(sp, 0x958) == "\u0915\u093c".encode() and _output(sp, 0x61) is None and _output(sp, 0xFDFA) is None
    assert max(int(e) & T.UNI_REC_LEN for e in sp.map_rec) <= T.UNI_MAX_MAP_BYTES
    # every map code point has a record, and nothing else has but U+200C: a space of its own that a
    # map code point in front of it swallows
    join = int(sp.map_rec[sp.map2[int(sp.map1[0x200C >> 7]) * 128 + (0x200C & 127)]])
    assert cls[0x200C] == T.UNI_SPACE and join == T.UNI_REC_JOIN
    cps = np.arange(0x110000)
    has = sp.map2[sp.map1[cps >> 7].astype(np.int64) * 128 + (cps & 127)] != T.UNI_MAP_NONE
    assert (has == ((cls == T.UNI_MAP) | (cps == 0x200C))).all()
    # layout C: an output with white space other than U+0020 stays host
    c_cls = _classes(TokenCounterModel(uc.tokenizer("C-nmt-first", tok_dir)).unigram_map_spec())
    diff = np.nonzero(c_cls != cls)[0].tolist()
    assert 0x85 in diff and all(c_cls[c] == T.UNI_HOST for c in diff)
    # without Precompiled nothing is replaced
    ident = TokenCounterModel(uc.tokenizer("H-identity", tok_dir))
    isp = ident.unigram_map_spec()
    assert isp.mapped and (_classes(isp) == _classes(ident.unigram_spec())).all()
    assert (isp.map2 == T.UNI_MAP_NONE).all()


def test_map_table_cache(tok_dir):
    path = uc.tokenizer("H-nmt", tok_dir)
    a = TokenCounterModel(path).unigram_map_spec()
    names = os.listdir(tok_dir)
    assert [f for f in names if f.startswith("unigram_map.") and f.endswith(".npz")]
    b = TokenCounterModel(path).unigram_map_spec()  # read back from the cache
    for name in ("cls1", "cls2", "map1", "map2", "map_rec", "map_pool"):
        assert (getattr(a, name) == getattr(b, name)).all(), name
    TokenCounterModel(path).unigram_spec()
    assert [f for f in os.listdir(tok_dir) if f.startswith("unigram_classes.")]  # a file of its own


def test_parameter_block_validator(tok_dir):
    h = native.host()
    sp = TokenCounterModel(uc.tokenizer("H-nmt", tok_dir)).unigram_map_spec()
    data, off = uc.pack(["a\u2026 b"])
    assert count_spec(sp, data, off)[0] > 0
    past = sp.map_rec.copy()
    past[-1] = (len(sp.map_pool) << 8) | 1  # a record past the pool
    long = sp.map_rec.copy()
    long[0] = (0 << 8) | (T.UNI_MAX_MAP_BYTES + 1)  # a length over the cap
    for change in (dict(map_rec=past), dict(map_rec=long),
                   dict(map2=np.full_like(sp.map2, T.UNI_MAP_NONE)),  # class-3 code points without a record
                   dict(map2=sp.map2[:-1]), dict(map1=sp.map1[:-1]), dict(map2=np.full_like(sp.map2, len(sp.map_rec))),
                   dict(map_pool=np.zeros(0, np.uint8)), dict(flags=2)):
        bad = copy.copy(sp)
        for k, v in change.items():
            setattr(bad, k, v)
        with pytest.raises(ValueError):
            h.uni_count(data, off, bad, 1, 0)
        with pytest.raises(ValueError):
            h.uni_params(bad, {})
    six = {"slots": 16, "pool": 32, "cls1": 48, "cls2": 64, "added": 80, "aoff": 96}
    with pytest.raises(ValueError):  # a mapped spec needs the addresses of its map
        h.uni_params(sp, six)
    with pytest.raises(ValueError):
        h.uni_params(sp, {**six, "map1": 112, "map2": 128, "map_rec": 144})
    block = h.uni_params(sp, {**six, "map1": 112, "map2": 128, "map_rec": 144, "map_pool": 160})
    o = h.DEV_UNI_OFFSETS
    assert len(block) == h.SIZEOF_DEV_UNI
    assert [int.from_bytes(block[o[f]:o[f] + 8], "little") for f in ("cls2", "map1", "map2", "mrec", "mpool")] == [
        64, 112, 128, 144, 160]
    plain = h.uni_params(TokenCounterModel(uc.tokenizer("H-nmt", tok_dir)).unigram_spec(), six)  # today's six
    assert [int.from_bytes(plain[o[f]:o[f] + 8], "little") for f in ("map1", "map2", "mrec", "mpool")] == [0] * 4


# ---- 2. counts ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def counted(tok_dir):
    """variant -> (model, documents, the mapped counter's raw result, the library's counts, the
    rule's host flags): computed once."""
    memo = {}

    def get(variant):
        if variant not in memo:
            path = uc.tokenizer(variant, tok_dir)
            m = TokenCounterModel(path)
            word, _ = uc.longest_word(path)
            docs = uc.corpus(word) + um.constructed(word) + um.lane_edge_docs(word)
            data, off = uc.pack(docs)
            raw = count_spec(m.unigram_map_spec(), data, off, 4)
            rule = um.to_host(path, variant)
            memo[variant] = (m, docs, data, off, raw, np.array(m.count(docs)), np.array([rule(t) for t in docs]))
        return memo[variant]

    return get


@pytest.mark.parametrize("variant", list(uc.VARIANTS))
def test_counts_equal_tokenizers(tok_dir, counted, variant):
    m, docs, data, off, raw, ref, host = counted(variant)
    old = count_spec(m.unigram_spec(), data, off, 4)
    print(f"{variant}: {len(docs)} documents, {int(host.sum())} to the host by the rule, {int((raw < 0).sum())} by "
          f"the counter ({int((old < 0).sum())} without the map), {int(((raw >= 0) & (raw != ref)).sum())} counts differ")
    assert set(raw[raw < 0].tolist()) <= {-2}
    wrong = np.nonzero((raw < 0) != host)[0]
    assert not len(wrong), [(docs[k][:60], int(raw[k]), bool(host[k])) for k in wrong[:5]]
    bad = np.nonzero(~host & (raw != ref))[0]
    assert not len(bad), [(docs[k][:60], int(raw[k]), int(ref[k])) for k in bad[:5]]
    # what the unmapped counter counts, the mapped one counts the same
    assert ((old < 0) | (old == raw)).all()
    by_text = {t: int(raw[k]) for k, t in enumerate(docs)}
    nmt = uc.VARIANTS[variant]["rule"] != "identity"
    for t in ("wait\u2026 what", "\ufb01ne", "a\x01b"):
        assert by_text[t] >= 0, t
    for t in ("e\u0301", "\U0001F468\u200d\U0001F469", "\u1161"):
        assert (by_text[t] == -2) == nmt, t
    if nmt:
        assert int((raw < 0).sum()) < int((old < 0).sum())
        assert by_text["\ufdfa"] == -2 and by_text["a\uff1c\uff55\uff4e\uff4b\uff1eb"] == -2 and by_text["a\uff1c\uff0f\uff53\uff1eb"] >= 0
        assert by_text["\x01\x01\x01"] == by_text[""] == 1
        # "the" spelled in full-width letters is "the"; U+00A8 alone is a word of one unknown
        assert by_text[um.full_width("the")] == by_text["the"] and by_text["\u00a8"] >= 2
    else:
        assert (_classes(m.unigram_map_spec()) != T.UNI_MAP).all()
        assert ((raw < 0) == (old < 0)).all()


@pytest.mark.parametrize("variant", list(uc.VARIANTS))
def test_lane_split_equals_sequential(counted, variant):
    m, docs, data, off, raw, _, _ = counted(variant)
    sp = m.unigram_map_spec()
    np.testing.assert_array_equal(count_spec(sp, data, off, 4, chunk=16), raw)
    np.testing.assert_array_equal(count_spec(sp, data, off, 4, chunk=1), raw)
    np.testing.assert_array_equal(count_spec(sp, data, off, 4, chunk=7), raw)


def test_invalid_utf8_goes_to_the_host(tok_dir):
    m = TokenCounterModel(uc.tokenizer("H-nmt", tok_dir))
    sp, fine = m.unigram_map_spec(), m.count(["fine text"])[0]
    data = np.frombuffer(b"".join(uc.INVALID), dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(d) for d in uc.INVALID]).astype(np.int64)
    for chunk in (0, 1, 16):
        assert count_spec(sp, data, off, 1, chunk).tolist() == [-2 if h else fine for h in uc.INVALID_HOST]


# ---- 3. the emulated device pipeline ------------------------------------------------------------
def test_emulated_device_token_counts_equal_cpu(tok_dir, monkeypatch):
    """Engine(emulate) under TB_TUNE=uni_map=1: outputs equal the CPU path's, and the host tokenizer
    counts the documents of the new rule only - fewer than the old rule's on the same input."""
    from test_emulated_device_path import outputs
    from test_unigram import _cfg

    from textblaster_amd.pipeline.engine import Engine
    from textblaster_amd.utils import metrics

    monkeypatch.setenv("TB_TUNE", "uni_map=1")
    tok = uc.tokenizer("H-nmt", tok_dir)
    docs = synth.make_corpus(2500, 900, seed=12) + uc.fuzz(200, 13)
    data, off = synth.pack(docs)
    delegated = uc.watch_delegated(monkeypatch)
    eng = Engine(_cfg(), backend="emulate", nthreads=4, keep_reasons=True, tokenizer_file=tok)
    assert eng.tune.uni_map and eng.device_runner.resolve_blob is not None and eng.device_runner.bpe
    h0, d0 = metrics.BPE_HOST_DOCS_TOTAL._value.get(), metrics.BPE_DEVICE_DOCS_TOTAL._value.get()
    a = eng.process(data, off)
    nh = metrics.BPE_HOST_DOCS_TOTAL._value.get() - h0
    nd = metrics.BPE_DEVICE_DOCS_TOTAL._value.get() - d0
    b = Engine(_cfg(), backend="cpu", nthreads=4, keep_reasons=True, tokenizer_file=tok,
               segmentation="icu").process(data, off)
    np.testing.assert_array_equal(a.status, b.status)
    oa = outputs(a)
    assert oa == outputs(b)
    kept, want = uc.rule_count(um.to_host(tok, "H-nmt"), docs, oa, delegated)
    _, want_old = uc.rule_count(uc.to_host(tok, "H-nmt"), docs, oa, delegated)
    print(f"kept {kept}: host tokenizer {nh} (the rule: {want}; without the map: {want_old}), device {nd}")
    assert nd > 0 and nh == want and nh + nd == kept <= a.n_kept
    assert want < want_old
