"""Constructed 64-bit hash collisions on the CPU (tests/collision_corpus.py): the CPU oracle and the
host emulation of the device algorithms against a string-set reference. A hash hit between unequal
elements must never be trusted: records stay those of exact string equality, and only the two sites
that cannot verify inline raise DOC_NEEDS_CPU. The device runs of the same documents are in
tests/test_gpu_hash_collisions.py."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collision_corpus as cc  # noqa: E402

from textblaster_amd import native  # noqa: E402
from textblaster_amd.config import load_pipeline_config  # noqa: E402
from textblaster_amd.pipeline.engine import Engine  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402
from textblaster_amd.utils.text import find_all_duplicate, find_duplicates  # noqa: E402


def config(kind):
    cfg = load_pipeline_config("config/bench_pipeline.yaml")
    gr = [s for s in cfg.pipeline if s.type == "GopherRepetitionFilter"]
    fw = [s for s in cfg.pipeline if s.type == "FineWebQualityFilter"]
    assert len(gr) == 1 and len(fw) == 1
    cfg.pipeline = {"gr": gr, "fw": fw, "gr2": [gr[0], copy.deepcopy(gr[0])]}[kind]
    return cfg


def orders(cfg):
    s = [s for s in cfg.pipeline if s.type == "GopherRepetitionFilter"][0].native_dict()
    return [int(n) for n, _ in s["top_n_grams"]], [int(n) for n, _ in s["dup_n_grams"]]


def reference_records(kind, cfg, texts):
    """[step][document] -> the record of the string-set reference."""
    if kind == "fw":
        s = cfg.pipeline[0].native_dict()
        chars = s.get("stop_chars") or []
        return [[cc.ref_fineweb(t, chars, int(s["short_line_length"])) for t in texts]]
    top, dup = orders(cfg)
    recs = [cc.ref_gopher_rep(t, top, dup) for t in texts]
    return [recs] * len(cfg.pipeline)


def compare(names, got, want, skip=()):
    """got: stage records [steps * ndocs * width] (step-major), want: reference_records()."""
    n, steps = len(names), len(want)
    g = np.asarray(got).reshape(steps, n, -1)
    bad = [(names[i], s, g[s, i].tolist(), want[s][i]) for s in range(steps) for i in range(n)
           if names[i] not in skip and g[s, i].tolist() != want[s][i]]
    assert not bad, bad[:4]


def all_documents():
    d = {}
    d.update(cc.default_documents())
    d.update(cc.rest_documents())
    d.update(cc.pre_documents())
    return d


def test_built_pairs_collide_and_twins_do_not():
    """Under the mirrors of both hashes. The compiled hash_bytes has no binding of its own; the path
    to it is emulate_stage's 64-bit-slot table, which joins words on their compiled keys and raises
    DOC_NEEDS_CPU exactly when two unequal words share one (test_emulation_..., slot64_W)."""
    t, c = cc.T.encode(), cc.TC.encode()
    assert t != c and len(t) == len(c) == 1024
    assert cc.hash_bytes(t) == cc.hash_bytes(c)
    assert cc.hash_bytes(t) != cc.hash_bytes(cc.TZ.encode()) and len(cc.TZ) == 1024
    a, b = cc.tm_pair(9)
    assert cc.hash_bytes(a) != cc.hash_bytes(b)  # the length is needed: 2^9 does not collide
    a, b = cc.tm_pair(10, b"q", b"Z")
    assert cc.hash_bytes(a) == cc.hash_bytes(b)
    for x in (cc.T5, cc.TC5, cc.TZ5):
        assert len(x) == 5 and all(x)
    assert cc.hash_bytes("".join(cc.T5).encode()) == cc.hash_bytes("".join(cc.TC5).encode())
    assert not set(cc.T5) & set(cc.TC5) and "".join(cc.T5) != "".join(cc.TC5)
    assert cc.hash_bytes("".join(cc.T5).encode()) != cc.hash_bytes("".join(cc.TZ5).encode())
    # XOR-rotate: a long word and a ten-word gram, bytes 64 apart exchanged
    assert cc.X != cc.XS and len(cc.X) == len(cc.XS) == len(cc.XZ) == 70
    assert cc.ng_hash(cc.X.encode()) == cc.ng_hash(cc.XS.encode())
    assert cc.ng_hash(cc.X.encode()) != cc.ng_hash(cc.XZ.encode())
    g, gs, gz = ("".join(x).encode() for x in (cc.G10, cc.G10S, cc.G10Z))
    assert all(len(w) == 7 for x in (cc.G10, cc.G10S, cc.G10Z) for w in x)
    assert g != gs and cc.ng_hash(g) == cc.ng_hash(gs) and cc.ng_hash(g) != cc.ng_hash(gz)
    assert cc.G10[0] != cc.G10S[0] and cc.G10[9] != cc.G10S[9] and cc.G10[1:9] == cc.G10S[1:9]
    # swapping closer than 64 does not collide
    s = bytearray(g)
    s[0], s[63] = s[63], s[0]
    assert cc.ng_hash(bytes(s)) != cc.ng_hash(g)
    assert len(set(cc.filler(3000) + cc.filler(3000, 1000, 3))) == 6000


def test_cpu_oracle_equals_string_reference():
    """find_top_duplicate, find_all_duplicate and find_duplicates of the host library (keyed by the
    polynomial hash) over the W, G and L word lists, every order of the default configuration."""
    top = native.host().find_top_duplicate
    docs = all_documents()
    for name in ("blk_W", "blk_G", "blk_L", "wave_W", "wave_G", "ng256_W", "ng256_G", "blk_W_twin", "split_G"):
        text = docs[name].text
        words = text.split()
        for n in range(1, 11):
            assert top(words, n) == cc.ref_top(words, n), (name, n)
            assert find_all_duplicate(words, n) == cc.ref_all_dup(words, n), (name, n)
        for items in (text.strip().split("\n"), text.strip().split("\n\n"), words):
            assert find_duplicates(items) == cc.ref_duplicates(items), name
    # the collisions are live: with T's partner taken for T these numbers would differ
    w = docs["blk_W"].text.split()
    merged = [cc.T if x == cc.TC else x for x in w]
    assert cc.ref_top(w, 2) != cc.ref_top(merged, 2)
    g = docs["blk_G"].text.split()
    assert cc.ref_all_dup(g, 5) == 1024
    assert find_duplicates([cc.T, cc.TC, cc.T]) == (1, 1024)


@pytest.fixture(scope="module")
def emulated():
    docs = all_documents()
    data, off = synth.pack([d.text for d in docs.values()])
    out = {}
    for kind in ("gr", "fw", "gr2"):
        cfg = config(kind)
        out[kind] = (cfg, Engine(cfg, backend="emulate", nthreads=4).device_runner.run(data, off))
    return docs, out


@pytest.mark.parametrize("kind", ["gr", "fw", "gr2"])
def test_emulation_equals_string_reference(emulated, kind):
    """Engine(backend="emulate") records of every named document, field by field; flags exactly the
    expected ones (the 64-bit-slot document, by design; its twin and everything else 0)."""
    docs, out = emulated
    cfg, res = out[kind]
    names = list(docs)
    want_flags = [d.emu_flag if kind != "fw" else 0 for d in docs.values()]
    assert res.flags.tolist() == want_flags, [(n, int(f)) for n, f in zip(names, res.flags) if f]
    assert len(res.stage_recs) == 1
    flagged = {n for n, f in zip(names, want_flags) if f}
    compare(names, res.stage_recs[0], reference_records(kind, cfg, [d.text for d in docs.values()]), skip=flagged)
    if kind != "fw":
        assert flagged == {"slot64_W"}


def test_documents_differ_from_their_twins_where_a_trusted_hash_would_not(emulated):
    """The reference itself tells every colliding document from the record a trusted hash would give:
    replacing the partner by the word it collides with changes the record."""
    docs, out = emulated
    top, dup = orders(out["gr"][0])
    for name, d in docs.items():
        if name.endswith("_twin") or name == "pre_small":
            continue
        merged = d.text.replace(cc.TC, cc.T).replace(cc.XS, cc.X)
        for a, b in zip(cc.TC5 + cc.G10S, cc.T5 + cc.G10):
            merged = merged.replace(a, b)
        assert cc.ref_gopher_rep(merged, top, dup) != cc.ref_gopher_rep(d.text, top, dup), name


STOP_CFG = """pipeline:
  - type: GopherQualityFilter
    min_doc_words: 1
    max_doc_words: 100000
    min_stop_words: 1
    stop_words: ["%s", "%s"]
"""


def stop_config(tmp_path_factory, order):
    a, b = (cc.T, cc.TC) if order == 0 else (cc.TC, cc.T)
    p = tmp_path_factory.mktemp("cfg") / f"stop{order}.yaml"
    p.write_text(STOP_CFG % (a, b), encoding="utf-8")
    return load_pipeline_config(str(p))


@pytest.mark.parametrize("order", [0, 1])
def test_colliding_stop_words_are_both_found(tmp_path_factory, order):
    """Two stop words with one 64-bit key sit in consecutive slots of the device table; a word that
    matches the first slot's key but not its bytes must go on to the second (is_stop_word)."""
    cfg = stop_config(tmp_path_factory, order)
    data, off = synth.pack(cc.stop_word_case())
    a = Engine(cfg, backend="emulate", nthreads=2, keep_reasons=True).process(data, off)
    b = Engine(cfg, backend="cpu", segmentation="icu", nthreads=2, keep_reasons=True).process(data, off)
    assert a.n_delegated == 0
    np.testing.assert_array_equal(a.status, b.status)
    np.testing.assert_array_equal(a.fail_step, b.fail_step)
    assert a.reasons == b.reasons
    assert sorted(b.reasons) == [2] and "gopher_too_few_stop_words (found 0, required 1)" in b.reasons[2]
