"""Constructed 64-bit hash collisions on the device (tests/collision_corpus.py): every named document
takes the route it was built for, device records equal the host emulation bit for bit and the
string-set reference for every unflagged document, and exactly the two documents that reach a site
which cannot verify inline (k_pre_wcanon, the 64-bit-slot table of canonicalize_res) are flagged and
come back with the CPU oracle's answer. Needs an MI355X.

ng_top_order (gr_ngrams.hip) and the generic top orders key their tables by canonical word ids only,
so no text collision reaches them directly: they depend on the W documents' word ids being exact.
The kPartTables branch of canonicalize_res is in reach below split_doc_bytes: blk_part_W has 8,300
two-letter words, so its word table exceeds the whole LDS slice of a long-document workgroup. The
branch also asks for 8 KB of the slice to be free at that point, which the host cannot see; the
route test asserts the table size only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import collision_corpus as cc  # noqa: E402
from test_emulated_device_path import outputs  # noqa: E402
from test_hash_collisions import compare, config, reference_records, stop_config  # noqa: E402

from textblaster_amd.utils import synth  # noqa: E402

pytestmark = pytest.mark.gpu

# TB_TUNE setting -> (documents, configurations run under it)
SETTINGS = {
    "default": ("", cc.default_documents, ("gr", "fw", "gr2")),
    # one-wave documents of more than 1024 words next to 1 KB words
    "rest": ("long_doc_bytes=8192", cc.rest_documents, ("gr", "gr2")),
    "pre": ("pre_doc_bytes=65536", cc.pre_documents, ("gr",)),
}


@pytest.fixture(scope="module")
def runs(host):
    from textblaster_amd.ops import hiprt
    from textblaster_amd.pipeline.engine import Engine

    assert hiprt.device_count() > 0
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        for setting, (tune, build, kinds) in SETTINGS.items():
            mp.setenv("TB_TUNE", tune)
            docs = build()
            data, off = synth.pack([d.text for d in docs.values()])
            for kind in kinds:
                cfg = config(kind)
                dev = Engine(cfg, backend="cuda", device="cuda:0").device_runner
                emu = Engine(cfg, backend="emulate", nthreads=8).device_runner
                out[setting, kind] = (cfg, docs, dev, [dev.run(data, off), dev.run(data, off)], emu.run(data, off))
    return out


CASES = [(s, k) for s, (_, _, kinds) in SETTINGS.items() for k in kinds]


def test_documents_take_their_routes(runs):
    """From the runner's own thresholds: every listed route, both DOC_NEEDS_CPU sites included."""
    seen = set()
    for (setting, kind), (cfg, docs, dev, _, _) in runs.items():
        assert bool(dev.gr_split) == (kind == "gr"), "one GopherRepetition step: split mode"
        if setting == "pre":
            assert dev.pre_doc_bytes == 65536 and dev.pre_wcanon
        else:
            assert dev.pre_doc_bytes > max(len(d.text) for d in docs.values()), "pre-pass off"
        assert dev.ngram_block
        for name, d in docs.items():
            assert cc.route_of(dev, d.text) == d.route, (setting, name)
            seen.add((kind, d.route))
    for route in ("ng256", "ng512", "ng1024", "rest", "blk", "blk_part", "split", "slot64", "pre"):
        assert ("gr", route) in seen, route
    for route in ("ng512", "rest", "blk", "blk_part", "split", "slot64"):  # in-stage n-grams, no export
        assert ("gr2", route) in seen, route
    for route in ("ng512", "blk", "split"):
        assert ("fw", route) in seen, route
    slot64 = runs["default", "gr"][1]["slot64_W"].text
    assert len(slot64.split()) >= cc.SLOT64_WORDS


@pytest.mark.parametrize("setting,kind", CASES)
def test_flags_are_exactly_the_expected_ones(runs, setting, kind):
    """No mask: the by-design documents are flagged, their twins and everything else are not. (The
    emulation has no pre-pass: it verifies the pre-pass document's words inline and does not flag.)"""
    cfg, docs, dev, (a, _), e = runs[setting, kind]
    names = list(docs)
    fw = kind == "fw"
    assert a.flags.tolist() == [0 if fw else d.flag for d in docs.values()], \
        [(n, int(f)) for n, f in zip(names, a.flags) if f]
    assert e.flags.tolist() == [0 if fw else d.emu_flag for d in docs.values()], \
        [(n, int(f)) for n, f in zip(names, e.flags) if f]
    if setting == "default" and not fw:
        assert [n for n, f in zip(names, a.flags) if f] == ["slot64_W"]
    if setting == "pre":
        assert [n for n, f in zip(names, a.flags) if f] == ["pre_W"]


@pytest.mark.parametrize("setting,kind", CASES)
def test_records_equal_emulation_and_string_reference(runs, setting, kind):
    cfg, docs, dev, (a, _), e = runs[setting, kind]
    names = list(docs)
    flagged = {n for n, d in docs.items() if d.flag and kind != "fw"}
    assert len(a.stage_recs) == len(e.stage_recs) == 1
    x = np.asarray(a.stage_recs[0]).reshape(len(cfg.pipeline), len(names), -1)
    y = np.asarray(e.stage_recs[0]).reshape(x.shape)
    bad = [(names[i], x[s, i].tolist(), y[s, i].tolist()) for s, i in np.argwhere(~np.all(x == y, axis=2))
           if names[i] not in flagged or docs[names[i]].emu_flag]
    assert not bad, bad[:4]
    compare(names, a.stage_recs[0], reference_records(kind, cfg, [d.text for d in docs.values()]), skip=flagged)


@pytest.mark.parametrize("setting,kind", CASES)
def test_two_runs_are_identical(runs, setting, kind):
    """The colliding elements race for one slot with atomicMin: records and flags do not depend on
    the winner."""
    _, _, _, (a, b), _ = runs[setting, kind]
    np.testing.assert_array_equal(a.flags, b.flags)
    for x, y in zip(a.stage_recs, b.stage_recs):
        np.testing.assert_array_equal(x, y)


def _equal_end_to_end(a, b):
    assert (a.n_kept, a.n_excluded) == (b.n_kept, b.n_excluded)
    np.testing.assert_array_equal(a.status, b.status)
    np.testing.assert_array_equal(a.fail_step, b.fail_step)
    assert a.reasons == b.reasons
    oa, ob = outputs(a), outputs(b)
    assert oa.keys() == ob.keys()
    assert not [k for k in oa if oa[k] != ob[k]]


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_end_to_end_equals_cpu_oracle(host, setting, monkeypatch):
    """Status, failing step, reasons and output bytes of the whole corpus; the flagged documents come
    back with the oracle's answer, and nothing else is recomputed on the CPU."""
    from textblaster_amd.pipeline.engine import Engine

    tune, build, _ = SETTINGS[setting]
    monkeypatch.setenv("TB_TUNE", tune)
    docs = build()
    data, off = synth.pack([d.text for d in docs.values()])
    cfg = config("gr")
    a = Engine(cfg, backend="cuda", device="cuda:0", keep_reasons=True).process(data, off)
    b = Engine(cfg, backend="cpu", segmentation="icu", nthreads=8, keep_reasons=True).process(data, off)
    _equal_end_to_end(a, b)
    assert a.n_delegated == sum(1 for d in docs.values() if d.flag)
    assert len(set(a.status.tolist())) > 1  # some documents are filtered, some kept


@pytest.mark.parametrize("order", [0, 1])
def test_colliding_stop_words_on_the_device(host, tmp_path_factory, order):
    from textblaster_amd.pipeline.engine import Engine

    cfg = stop_config(tmp_path_factory, order)
    data, off = synth.pack(cc.stop_word_case())
    a = Engine(cfg, backend="cuda", device="cuda:0", keep_reasons=True).process(data, off)
    b = Engine(cfg, backend="cpu", segmentation="icu", nthreads=2, keep_reasons=True).process(data, off)
    assert a.n_delegated == 0
    _equal_end_to_end(a, b)
    assert sorted(b.reasons) == [2]
