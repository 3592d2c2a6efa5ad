"""Every device pass on every document of the every-pass corpus (tests/every_pass_corpus.py:
adversarial text at every routing class, boundary constructs at the workgroup kernels' own chunk
edges and at the pre-pass tile edges). The step gates are off (TB_TUNE gate=0), so no kernel is
spared the documents an earlier step would have filtered, and nothing is masked out of a
comparison: flags, every stage and C4 record array (the language-ID confidence bit for bit), every
content version, status, first failing step and output bytes of every document equal the host
emulation; with the pre-pass from 64 KB also the device run without it. The flag vector is pinned
to the routing rule's (ep.expected_flags: one mostly-CJK document of EDGE, nothing else). A second
leg, independent of the shared kernel source, runs the device engine against the CPU ICU oracle
one filter at a time, where no earlier gate exists. A launch spy asserts that every kernel family
got its documents. Needs an MI355X."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import every_pass_corpus as ep  # noqa: E402
from test_emulated_device_path import outputs  # noqa: E402
from test_every_pass_corpus import (BY_DESIGN, CFG, FILTERS, TUNE_OFF, TUNE_PRE, by_design_cpu, corpus_docs,  # noqa: E402
                                    filter_config)
from test_gpu_blk_mid import _outputs, launch_split  # noqa: E402

from textblaster_amd.config import load_pipeline_config  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402

pytestmark = pytest.mark.gpu

MID = ep.MID_DOC_BYTES


def _spy(dev):
    """Records (kernel family, documents launched) of the workgroup-path launches of ``dev``."""
    k, calls = dev.k, []
    blk, dup, pre, wcanon, c4a = k.stage_analyze_blk, k.gr_dup_split, k.pre_decode, k.pre_wcanon, k.c4_pass_a

    def stage_analyze_blk(plan, stage, docs, work, tables, gr_export=None, n_split=0, split_bytes=0,
                          line_stats=None, pre=None, dict_in=None, mid=False):
        calls.append(("blk_mid" if mid else "blk_pre" if pre is not None else "blk", int(docs.n_launch), int(n_split)))
        return blk(plan, stage, docs, work, tables, gr_export, n_split, split_bytes, line_stats, pre, dict_in, mid=mid)

    def gr_dup_split(stage, gr_step, docs, *args, **kw):
        calls.append(("gr_dup_split", int(docs.n_launch), 0))
        return dup(stage, gr_step, docs, *args, **kw)

    def pre_decode(docs, *args, **kw):
        calls.append(("pre_decode", int(docs.n_launch), 0))
        return pre(docs, *args, **kw)

    def pre_wcanon(docs, *args, **kw):
        calls.append(("pre_wcanon", int(docs.n_launch), 0))
        return wcanon(docs, *args, **kw)

    def c4_pass_a(c4, docs, *args, **kw):
        if kw.get("blk"):
            calls.append(("c4_blk", int(docs.n_launch), 0))
        return c4a(c4, docs, *args, **kw)

    k.stage_analyze_blk, k.gr_dup_split, k.pre_decode, k.pre_wcanon, k.c4_pass_a = \
        stage_analyze_blk, gr_dup_split, pre_decode, pre_wcanon, c4_pass_a
    return calls


def _runner(mp, tune, backend):
    from textblaster_amd.pipeline.engine import Engine

    mp.setenv("TB_TUNE", tune)
    kw = dict(device="cuda:0") if backend == "cuda" else dict(nthreads=8)
    return Engine(load_pipeline_config(CFG), backend=backend, **kw).device_runner


@pytest.fixture(scope="module")
def runs(host):
    from textblaster_amd.ops import hiprt

    assert hiprt.device_count() > 0
    docs = corpus_docs()
    names, texts = list(docs), list(docs.values())
    lens = np.array([ep.nbytes(t) for t in texts])
    # the mid-size workgroup kernel takes a batch's workgroup documents only when none of them is
    # longer than MID_DOC_BYTES: the same documents once more without the longer ones
    short = [i for i in range(len(texts)) if lens[i] <= MID]
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        dev, emu = _runner(mp, TUNE_OFF, "cuda"), _runner(mp, TUNE_OFF, "emulate")
        pre = _runner(mp, TUNE_PRE, "cuda")
        assert not dev.gating and not pre.gating and not emu.gates
        assert dev.pre_doc_bytes > lens.max() and pre.pre_doc_bytes == 65536 and pre.pre_wcanon
        for key, runner, idx in (("all", dev, None), ("mid", dev, short), ("pre", pre, None)):
            nm = names if idx is None else [names[i] for i in idx]
            tx = texts if idx is None else [texts[i] for i in idx]
            data, off = synth.pack(tx)
            calls = _spy(runner) if key != "mid" else out["all"]["calls_ref"]
            del calls[:]
            a = runner.run(data, off)
            out[key] = dict(host=host, names=nm, texts=tx, lens=np.diff(off), dev=runner, a=a, calls=list(calls),
                            calls_ref=calls,
                            e=emu.run(data, off) if key != "pre" else out["all"]["e"])
        yield out


def _doc(run, d):
    return f"{run['names'][d]} ({ep.route(run['dev'], run['texts'][d])}, {int(run['lens'][d])} bytes)"


def _assert_equal(run, a, b):
    """Every array of two runs, whole; a difference names its documents and their routes."""
    dev, n = run["dev"], len(run["names"])
    fa, fb = np.asarray(a.flags), np.asarray(b.flags)
    want = np.array(ep.expected_flags(run["host"], run["texts"], dev.dict_marks), dtype=fa.dtype)
    assert np.array_equal(fa, want), [(_doc(run, d), int(fa[d])) for d in np.nonzero(fa != want)[0][:8]]
    assert np.array_equal(fb, want), [(_doc(run, d), int(fb[d])) for d in np.nonzero(fb != want)[0][:8]]
    assert [run["names"][d] for d in np.nonzero(fa)[0]] == [BY_DESIGN[0]]
    assert len(a.stage_recs) == len(b.stage_recs) == 2
    for s, (x, y) in enumerate(zip(a.stage_recs, b.stage_recs)):
        x, y = np.asarray(x), np.asarray(y)
        width_total, layout = dev.stage_layout[s]
        assert x.shape == y.shape == (width_total * n,)
        # (step-major layout: step k's fields of document d at prefix[k] * n + d * width[k]; the
        # language-ID confidence is the bit pattern of a double in one of these fields)
        for step_i, (kind, width, prefix) in zip(dev.plan.stages[s], layout):
            xs = x[prefix * n:(prefix + width) * n].reshape(n, width)
            ys = y[prefix * n:(prefix + width) * n].reshape(n, width)
            bad = np.nonzero((xs != ys).any(axis=1))[0]
            assert len(bad) == 0, (dev.plan.steps[step_i].type, len(bad),
                                   [(_doc(run, d), xs[d].tolist(), ys[d].tolist()) for d in bad[:3]])
        assert np.array_equal(x, y)
    assert sorted(a.c4_recs) == sorted(b.c4_recs) and len(a.c4_recs) == 1
    for i in a.c4_recs:
        x, y = np.asarray(a.c4_recs[i]).reshape(n, 7), np.asarray(b.c4_recs[i]).reshape(n, 7)
        bad = np.nonzero((x != y).any(axis=1))[0]
        assert len(bad) == 0, [(_doc(run, d), x[d].tolist(), y[d].tolist()) for d in bad[:3]]
    assert sorted(a.versions) == sorted(b.versions) == [1]
    for v in sorted(a.versions):
        (xd, xo), (yd, yo) = a.versions[v], b.versions[v]
        xd, xo, yd, yo = np.asarray(xd), np.asarray(xo), np.asarray(yd), np.asarray(yo)
        bad = [d for d in range(n) if xo[d + 1] - xo[d] != yo[d + 1] - yo[d]
               or bytes(xd[xo[d]:xo[d + 1]]) != bytes(yd[yo[d]:yo[d + 1]])]
        assert not bad, [_doc(run, d) for d in bad[:5]]
        assert np.array_equal(xo, yo) and np.array_equal(xd[:xo[-1]], yd[:yo[-1]])
    for field in ("status", "fail"):
        x, y = np.asarray(getattr(a.resolved, field)), np.asarray(getattr(b.resolved, field))
        bad = np.nonzero(x != y)[0]
        assert len(bad) == 0, (field, [(_doc(run, d), int(x[d]), int(y[d])) for d in bad[:5]])
    oa, ob = _outputs(a), _outputs(b)
    # (every document but the one for the CPU path has its output)
    assert sorted(oa) == sorted(ob) == [d for d in range(n) if not fa[d]]
    bad = [d for d in oa if oa[d] != ob[d]]
    assert not bad, [(_doc(run, d), oa[d][0], ob[d][0]) for d in bad[:5]]


@pytest.mark.parametrize("key", ["all", "mid", "pre"])
def test_device_equals_emulation_with_gates_off(runs, key):
    run = runs[key]
    assert run["a"].dead is None and run["e"].dead is None
    _assert_equal(run, run["a"], run["e"])
    # with the gates off every stage and the C4 pass analysed documents of every route
    rec = [np.asarray(r).any() for r in run["a"].stage_recs]
    assert all(rec) and np.asarray(next(iter(run["a"].c4_recs.values()))).any()


def test_pre_pass_run_equals_the_run_without_it(runs):
    """The emulation has no pre-pass: the run with it is also compared with the device's own run
    of the same batch without it."""
    assert runs["pre"]["names"] == runs["all"]["names"]
    _assert_equal(runs["pre"], runs["pre"]["a"], runs["all"]["a"])


def test_every_kernel_family_got_its_documents(runs):
    """From the launches themselves: the workgroup stage kernel (full-size, mid-size, and behind the
    pre-pass), k_gr_dup_split, the pre-pass and the C4 workgroup pass, each with the number of
    documents the runner's thresholds give them (launch_split of test_gpu_blk_mid.py)."""
    for key in ("all", "mid", "pre"):
        run = runs[key]
        dev, lens = run["dev"], run["lens"]
        n_long, n_split, n_mid = launch_split(lens, dev.long_doc_bytes, dev.split_doc_bytes, MID)
        n_pre = int(np.count_nonzero(lens >= dev.pre_doc_bytes)) if key == "pre" else 0
        assert n_long >= 40 and (n_split >= 10) == (key != "mid") and (n_pre >= 10) == (key == "pre")
        stage = [c for c in run["calls"] if c[0].startswith("blk")]
        other = sorted(c for c in run["calls"] if not c[0].startswith("blk"))
        if key == "mid":
            # every workgroup document is mid-sized: one launch per stage of the 256-thread kernel
            assert n_mid == n_long and stage == [("blk_mid", n_long, 0)] * 2
            assert other == [("c4_blk", n_long, 0)]
        elif key == "all":
            # a split document in the batch: the full-size kernel takes them all; k_gr_dup_split
            # runs for the stage with the GopherRepetition step
            assert n_mid == 0 and stage == [("blk", n_long, n_split), ("blk", n_long, 0)]
            assert other == [("c4_blk", n_long, 0), ("gr_dup_split", n_split, 0)]
        else:
            # the original text's stage: the pre-pass documents first, then the rest; the stage
            # over the rewritten text knows no pre-pass
            assert stage == [("blk_pre", n_pre, n_pre), ("blk", n_long - n_pre, n_split - n_pre), ("blk", n_long, 0)]
            assert other == [("c4_blk", n_long, 0), ("gr_dup_split", n_split, 0), ("pre_decode", n_pre, 0),
                             ("pre_wcanon", n_pre, 0)]
        # the wave kernels got the rest
        assert len(lens) - n_long >= 800


@pytest.mark.parametrize("types", FILTERS, ids=["+".join(t[:-6] for t in f) for f in FILTERS])
def test_device_equals_icu_oracle_filter_by_filter(host, types, monkeypatch):
    """One filter (or C4 and FineWeb) of config/bench_pipeline.yaml alone: no earlier gate, so every
    document reaches it. Device engine against the CPU engine with ICU segmentation."""
    from textblaster_amd.pipeline.engine import Engine

    monkeypatch.delenv("TB_TUNE", raising=False)
    docs = corpus_docs()
    names = list(docs)
    data, off = synth.pack(list(docs.values()))
    eng = Engine(filter_config(types), backend="cuda", device="cuda:0", keep_reasons=True)
    a = eng.process(data, off)
    b = Engine(filter_config(types), backend="cpu", segmentation="icu", nthreads=8, keep_reasons=True).process(data, off)

    def doc(k):
        return f"{names[k]} ({ep.route(eng.device_runner, docs[names[k]])})"

    assert a.n_delegated == len(by_design_cpu(host, docs, eng.device_runner.dict_marks, types))
    assert (a.n_kept, a.n_excluded) == (b.n_kept, b.n_excluded)
    bad = np.nonzero((a.status != b.status) | (a.fail_step != b.fail_step))[0]
    assert len(bad) == 0, [(doc(k), int(a.fail_step[k]), int(b.fail_step[k])) for k in bad[:5]]
    diff = [k for k in sorted(set(a.reasons) | set(b.reasons)) if a.reasons.get(k) != b.reasons.get(k)]
    assert not diff, [(doc(k), a.reasons.get(k), b.reasons.get(k)) for k in diff[:5]]
    oa, ob = outputs(a), outputs(b)  # (kept / excluded, text bytes, metadata bytes)
    assert oa.keys() == ob.keys() and len(oa) == len(names)
    diff = [k for k in oa if oa[k] != ob[k]]
    assert not diff, [(doc(k), oa[k][0], ob[k][0], oa[k][2], ob[k][2]) for k in diff[:3]]
