"""C4 pass A's byte scan on the GPU: k_c4_pass_a / k_c4_pass_a_blk match phrases from packed
bytes; the stage kernels in front of them count stop words. About 2,000 documents of 0-2,100 bytes
from tests/c4_scan_corpus.py (phrases at every alignment, cut by the end of the text, across a
lane's 16 bytes and a wave's 1,024, the Kelvin sign for each 'k', near misses, brackets, stop-word
candidates at a document's first and last bytes) and a few of 5-9 KB whose phrases straddle the
workgroup kernels' strides (4,096 and 8,192 bytes); documents of odd lengths in front of each other
give every start alignment. Device records, flags and output bytes must equal the host
emulation's, with GopherQuality in front of C4 and with C4 in front, and no document may be
delegated. Needs an MI355X, and g++: the corpus comes from tools/c4_scan_selftest.cpp, which the
fixture compiles (a machine without a compiler fails the test, it does not skip it)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import c4_scan_corpus as corpus  # noqa: E402

from textblaster_amd.config import load_pipeline_config_str  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402

pytestmark = pytest.mark.gpu

CONFIGS = {"gq_c4": corpus.CFG_GQ_C4, "c4_first": corpus.CFG_C4_FIRST}


@pytest.fixture(scope="module")
def runs(host):
    from textblaster_amd.ops import hiprt
    from textblaster_amd.pipeline.engine import Engine

    assert hiprt.device_count() > 0
    docs = corpus.documents(small_every=3, wrapped_every=3, big=12)
    data, off = synth.pack(docs)
    out = {}
    for name, text in CONFIGS.items():
        dev = Engine(load_pipeline_config_str(text, name + ".yaml"), backend="cuda", device="cuda:0").device_runner
        emu = Engine(load_pipeline_config_str(text, name + ".yaml"), backend="emulate", nthreads=4).device_runner
        out[name] = (dev, dev.run(data, off), emu.run(data, off))
    return docs, off, out


def _outputs(res):
    r = res.resolved
    assert r is not None and r.err == 0
    out = {}
    for side, parts in zip(("kept", "excluded"), r.parts()):
        for rows, off, text in parts:
            for k, d in enumerate(np.asarray(rows).tolist()):
                out[d] = (side, bytes(text[int(off[k]):int(off[k + 1])]))
    return out


def test_documents_cover_the_paths(runs):
    docs, off, out = runs
    lens = np.diff(off)
    dev = out["gq_c4"][0]
    assert 1800 <= len(docs) <= 2600
    assert set((off[:-1] % 4).tolist()) == {0, 1, 2, 3}
    big = lens[lens > dev.long_doc_bytes]
    assert 8 <= len(big) <= 16 and big.min() >= 5120 and big.max() < 9216  # the workgroup kernels
    assert np.count_nonzero(lens <= 2300) >= len(docs) - 16 and lens.min() == 0
    # phrases that start in one wave iteration (1,024 bytes) and end in the next
    assert np.count_nonzero((lens > 1024) & (lens < 1200)) > 50


@pytest.mark.parametrize("name", list(CONFIGS))
def test_records_flags_and_texts_equal_host_emulation(runs, name):
    docs, _, out = runs
    _, a, b = out[name]
    fa, fb = np.asarray(a.flags), np.asarray(b.flags)
    assert not fa.any(), [docs[i][:60] for i in np.nonzero(fa)[0][:4]]  # none delegated
    assert not fb.any(), [docs[i][:60] for i in np.nonzero(fb)[0][:4]]
    assert len(a.stage_recs) == len(b.stage_recs)
    for s, (x, y) in enumerate(zip(a.stage_recs, b.stage_recs)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape
        bad = np.nonzero(x != y)[0]
        assert len(bad) == 0, (s, bad[:8].tolist(), x[bad[:8]].tolist(), y[bad[:8]].tolist())
    assert sorted(a.c4_recs) == sorted(b.c4_recs) and len(a.c4_recs) == 1
    for i in a.c4_recs:
        x, y = np.asarray(a.c4_recs[i]).reshape(len(docs), -1), np.asarray(b.c4_recs[i]).reshape(len(docs), -1)
        bad = np.nonzero((x != y).any(axis=1))[0]
        assert len(bad) == 0, [(docs[d][:80], x[d].tolist(), y[d].tolist()) for d in bad[:4]]
        # the filters under test decide: lorem ipsum, curly brackets (fields 0 and 1)
        assert x[:, 0].sum() > 20 and x[:, 1].sum() > 20
    np.testing.assert_array_equal(a.resolved.status, b.resolved.status)
    np.testing.assert_array_equal(a.resolved.fail, b.resolved.fail)
    oa, ob = _outputs(a), _outputs(b)
    assert sorted(oa) == sorted(ob)
    bad = [d for d in oa if oa[d] != ob[d]]
    assert not bad, [(docs[d][:80], oa[d][1][:80], ob[d][1][:80]) for d in bad[:3]]
    # C4 rewrote documents: lines with a javascript / policy phrase are gone
    changed = sum(1 for d, (side, t) in oa.items() if side == "kept" and t != docs[d].encode())
    assert changed > 100
