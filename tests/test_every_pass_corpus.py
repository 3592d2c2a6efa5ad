"""The every-pass corpus (tests/every_pass_corpus.py) on the CPU, before anyone needs a GPU: with
the step gates off the host emulation of the device kernels overflows no arena and flags exactly
the documents the routing rule sends to the CPU path by design (two dictionary-script documents of
EDGE: ep.expected_flags), the emulation equals the ICU oracle filter by filter (a pipeline of one
filter has no earlier gate, so every document reaches it), and the corpus covers
every route at least twice while the gates as shipped would keep most of it away from the later
passes. ``python tests/test_every_pass_corpus.py`` prints the coverage table of
profiles/every_pass/coverage.txt."""
import collections
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.join(REPO, "tests"), REPO) if p not in sys.path]  # (run as a script too)
import every_pass_corpus as ep  # noqa: E402
from test_emulated_device_path import outputs  # noqa: E402

from textblaster_amd.config import load_pipeline_config  # noqa: E402
from textblaster_amd.pipeline import tuning  # noqa: E402
from textblaster_amd.pipeline.engine import Engine  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402

CFG = os.path.join(REPO, "config", "bench_pipeline.yaml")
DOC_OVERFLOW = 2  # doc_ctx.h
TUNE_OFF = "gate=0"
TUNE_PRE = "gate=0,pre_doc_bytes=65536"

# the per-filter pipelines: config/bench_pipeline.yaml with only these step types kept
FILTERS = [("LanguageDetectionFilter",), ("GopherRepetitionFilter",), ("GopherQualityFilter",),
           ("C4QualityFilter",), ("FineWebQualityFilter",), ("C4QualityFilter", "FineWebQualityFilter")]


# the two dictionary-script documents of EDGE ("日本語のテキストです。", "mixed 日本 text. ...")
BY_DESIGN = ("edge12", "edge13")


def by_design_cpu(h, docs, dict_marks, types):
    """Names of the documents a pipeline of these step types sends to the CPU path by design
    (ep.expected_flags): none for language ID, the mostly-CJK document where a stage segments
    words with host ICU marks, both dictionary-script documents where only C4 segments."""
    segments = any(t != "LanguageDetectionFilter" for t in types)
    names = [n for n, f in zip(docs, ep.expected_flags(h, docs.values(), dict_marks, segments)) if f]
    assert names == list(BY_DESIGN[:len(names)])
    assert len(names) == (0 if not segments else 1 if dict_marks else 2)
    return names


def filter_config(types):
    cfg = load_pipeline_config(CFG)
    cfg.pipeline = [s for s in cfg.pipeline if s.type in types]
    assert [s.type for s in cfg.pipeline] == list(types)
    return cfg


def corpus_docs():
    """The corpus as the tests run it: thresholds of the shipped tuning, pre-pass from 64 KB."""
    return ep.every_pass_corpus(tuning.parse(TUNE_PRE))


def live_pairs(res, n_passes):
    """(document, pass) pairs in which the document is analysed: all of them without a gate, else
    those of the passes before the one its gate code names (dead = k: passes >= k skip it)."""
    n = len(res.flags)
    if res.dead is None:
        return n * n_passes
    dead = np.asarray(res.dead).astype(np.int64)
    return int(sum(np.count_nonzero(~((dead != 0) & (dead <= p))) for p in range(n_passes)))


def emulated(tune, texts, cfg=None):
    old = os.environ.get("TB_TUNE")
    os.environ["TB_TUNE"] = tune
    try:
        runner = Engine(cfg or load_pipeline_config(CFG), backend="emulate", nthreads=8).device_runner
    finally:
        if old is None:
            del os.environ["TB_TUNE"]
        else:
            os.environ["TB_TUNE"] = old
    data, off = synth.pack(texts)
    return runner, runner.run(data, off)


@pytest.fixture(scope="module")
def docs():
    return corpus_docs()


@pytest.fixture(scope="module")
def runs(docs):
    texts = list(docs.values())
    return {"gated": emulated("", texts), "off": emulated(TUNE_OFF, texts)}


def test_corpus_is_small_and_every_route_occurs_twice(docs):
    sizes = [ep.nbytes(t) for t in docs.values()]
    assert 900 <= len(docs) <= 1000 and sum(sizes) < 2_000_000, (len(docs), sum(sizes))
    # the same classifier for both runs of the GPU test: without the pre-pass and with it from 64 KB
    tu = tuning.parse(TUNE_OFF)
    by = collections.Counter(ep.route(tu, t) for t in docs.values())
    assert sorted(by) == sorted(r for r in ep.ROUTES if r != "pre") and min(by.values()) >= 2, by
    tu = tuning.parse(TUNE_PRE)
    by = collections.Counter(ep.route(tu, t) for t in docs.values())
    assert set(by) <= set(ep.ROUTES) and by["pre"] >= 2 and by["split"] >= 2 and by["blk"] >= 2, by
    # both sides of every threshold, byte for byte
    have = set(sizes)
    for t in (tu.ngram_big_bytes, tu.long_doc_bytes, 8192, ep.MID_DOC_BYTES, tu.split_doc_bytes):
        assert {t, t + 1} <= have, t
    assert {tu.pre_doc_bytes - 1, tu.pre_doc_bytes} <= have
    assert 69000 <= ep.nbytes(docs["join_para_longest"]) <= 71000


def test_motifs_straddle_the_workgroup_and_tile_edges(docs):
    tu = tuning.parse(TUNE_PRE)
    for name, text in docs.items():
        if name.startswith("wg_"):
            motif = [ep.MOTIFS[int(name[-2:])]]
            assert tu.long_doc_bytes < ep.nbytes(text) <= 8192, name
            assert all(ep.straddles(text, motif, e, True) for e in ep.WG_EDGES), name
            if name.startswith("wg_2byte") and len(motif[0]) >= 2:
                # (2-byte padding: the code point edges lie elsewhere than the byte edges)
                assert all(ep.straddles(text, motif, e, False) for e in ep.WG_EDGES), name
                assert len(text[:1024].encode()) > 1024 + 256
        elif name.startswith("tile_"):
            assert ep.nbytes(text) >= tu.pre_doc_bytes
            assert all(ep.straddles(text, ep.MOTIFS, e, True)
                       for e in range(ep.PRE_TILE, tu.pre_doc_bytes, ep.PRE_TILE)), name
            if name.startswith("tile_2byte"):
                # (the motif of one code point ends at the edge instead)
                assert all(ep.straddles(text, ep.MOTIFS, e, False) or text[e - 1] in ep.MOTIFS
                           for e in (ep.PRE_TILE, 2 * ep.PRE_TILE)), name
    # every motif occurs in each of the four families
    for prefix in ("wg_ascii", "wg_2byte", "tile_ascii", "tile_2byte"):
        family = "".join(t for n, t in docs.items() if n.startswith(prefix))
        assert all(m in family for m in ep.MOTIFS), prefix


def test_emulation_flags_no_document_with_gates_off(host, docs, runs):
    """No arena overflow and no unverifiable collision anywhere; the one flag is the mostly-CJK
    document of EDGE, which the host gives no ICU marks by design (ep.expected_flags)."""
    runner, res = runs["off"]
    assert not runner.gates and res.dead is None and runner.dict_marks
    names = list(docs)
    flagged = [(names[i], int(res.flags[i])) for i in np.nonzero(res.flags)[0]]
    assert not (np.asarray(res.flags) & DOC_OVERFLOW).any(), flagged[:10]
    assert flagged == [(n, f) for n, f in zip(names, ep.expected_flags(host, docs.values(), True)) if f], flagged[:10]
    assert flagged == [(BY_DESIGN[0], ep.DOC_NEEDS_CPU)]
    # every other document has a status of the device resolve
    st = np.asarray(res.resolved.status)
    assert [names[i] for i in np.nonzero(st == 3)[0]] == [BY_DESIGN[0]] and set(np.unique(st).tolist()) <= {0, 1, 3}


def test_gates_as_shipped_keep_most_documents_from_the_later_passes(docs, runs):
    """The gap this corpus closes: with the gates on, fewer than a third of it is live in the C4
    pass (and in the FineWeb stage after it)."""
    runner, res = runs["gated"]
    assert res.dead is not None and not np.asarray(res.flags).any()
    c4 = [p for p, (kind, _) in enumerate(runner.passes) if kind == "c4"]
    assert len(c4) == 1
    dead = np.asarray(res.dead)
    live_c4 = np.count_nonzero(~((dead != 0) & (dead <= c4[0])))
    assert 3 * live_c4 < len(docs), live_c4
    # ... and with them off every (document, pass) pair is compared
    off_runner, off = runs["off"]
    assert live_pairs(off, len(off_runner.passes)) == len(docs) * len(off_runner.passes)
    assert live_pairs(res, len(runner.passes)) < live_pairs(off, len(off_runner.passes))


@pytest.mark.parametrize("types", FILTERS, ids=["+".join(t[:-13] for t in f) for f in FILTERS])
def test_emulation_equals_icu_oracle_filter_by_filter(host, docs, types, monkeypatch):
    monkeypatch.delenv("TB_TUNE", raising=False)
    names = list(docs)
    data, off = synth.pack(list(docs.values()))
    emu = Engine(filter_config(types), backend="emulate", nthreads=8, keep_reasons=True)
    a = emu.process(data, off)
    b = Engine(filter_config(types), backend="cpu", segmentation="icu", nthreads=8, keep_reasons=True).process(data, off)
    assert a.n_delegated == len(by_design_cpu(host, docs, emu.device_runner.dict_marks, types))
    assert (a.n_kept, a.n_excluded) == (b.n_kept, b.n_excluded)
    bad = np.nonzero((a.status != b.status) | (a.fail_step != b.fail_step))[0]
    assert len(bad) == 0, [(names[k], int(a.fail_step[k]), int(b.fail_step[k])) for k in bad[:5]]
    diff = [k for k in sorted(set(a.reasons) | set(b.reasons)) if a.reasons.get(k) != b.reasons.get(k)]
    assert not diff, [(names[k], a.reasons.get(k), b.reasons.get(k)) for k in diff[:5]]
    oa, ob = outputs(a), outputs(b)
    assert oa.keys() == ob.keys() and len(oa) == len(names)
    diff = [k for k in oa if oa[k] != ob[k]]
    assert not diff, [(names[k], oa[k][0], ob[k][0], oa[k][2], ob[k][2]) for k in diff[:3]]


def coverage_report():
    """The table of profiles/every_pass/coverage.txt (CPU only: the emulated runner has the device's
    plan and gates)."""
    from test_gpu_kernels import kernels_corpus

    lines = ["(document, pass) pairs with a live comparison, from the emulated runner (same plan and gates as",
             "the device). A gated run has one pass more: the language-ID pass in front of its stage.", ""]
    cfg = load_pipeline_config(os.path.join(REPO, "config", "pipeline_config.yaml"))
    cfg.pipeline = [s for s in cfg.pipeline if s.type != "TokenCounter"]
    texts = list(corpus_docs().values())
    for label, tune, tx, c in (("test_gpu_kernels corpus, gated", "", kernels_corpus(), cfg),
                               ("every-pass corpus, gated", "", texts, None),
                               ("every-pass corpus, gates off", TUNE_OFF, texts, None)):
        runner, res = emulated(tune, tx, c)
        n, np_ = len(tx), len(runner.passes)
        live = live_pairs(res, np_)
        per = [n if res.dead is None else int(np.count_nonzero(~((res.dead != 0) & (res.dead <= p)))) for p in range(np_)]
        lines.append(f"{label}: {n} documents x {np_} passes = {n * np_} pairs, {live} live ({100.0 * live / (n * np_):.1f} %)")
        lines.append("    live documents per pass: " + ", ".join(f"{k}{x}={v}" for (k, x), v in zip(runner.passes, per)))
        names = [f"document {i}" for i in np.nonzero(res.flags)[0]] if c is not None else \
            [n for n, f in zip(corpus_docs(), res.flags) if f]
        lines.append(f"    flagged documents: {len(names)}" + (f" ({', '.join(names)}: mostly dictionary script, for the "
                                                              "CPU path by design; the tests pin its flag)" if names else ""))
    return "\n".join(lines)


if __name__ == "__main__":
    print(coverage_report())
