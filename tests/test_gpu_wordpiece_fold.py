"""k_wp_count_fold on the GPU (csrc/hip/wordpiece.hip): array for array against its host emulation
(which tests/test_wordpiece_fold.py pins to the `tokenizers` library) in the three fold modes, and
the device pipeline with a trailing uncased WordPiece TokenCounter against the CPU path. Every
launch runs twice on one input and must give the same result (races)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tok_device  # noqa: E402
import wordpiece_corpus as wc  # noqa: E402
import wordpiece_fold_corpus as fc  # noqa: E402

from textblaster_amd.models.tokenizer import TokenCounterModel, count_spec  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402

pytestmark = pytest.mark.gpu

BACKEND = "cuda"
MODES = {"both": (True, None), "lower": (True, False), "strip": (False, True)}


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("tok")


def lane_edge_docs():
    """A document of every length 0..130 bytes cut from a unit in which multi-output code points
    (U+AC01: 9 output bytes, U+0130: 2 code points in lower-only), empty outputs (U+0301, U+00AD)
    and an isolated ideograph straddle every 16-byte lane edge, and one 200 KB document (lane
    ranges over 3 KB)."""
    unit = "\u00e5b \u00c9\uac01e\u0301f \u00adg\u0130;ij\u4f60m\uac00 "
    docs = []
    for n in range(131):
        docs.append((unit * 8).encode("utf-8")[:n].decode("utf-8", "ignore"))
    return docs + [wc.big_doc(200 * 1024, 33)]


@pytest.mark.parametrize("mode", list(MODES))
def test_fold_kernel_equals_host(tok_dir, mode):
    from textblaster_amd import native

    lower, strip = MODES[mode]
    m = TokenCounterModel(fc.train(str(tok_dir / f"{mode}.json"), lower, strip))
    synthetic = synth.make_corpus(2000, 1024, seed=23, vocab="zipf", mixed_script=True)
    # (in capitals as well: lowercase alone changes only the capitals among the non-ASCII letters)
    texts = fc.pool_docs() + lane_edge_docs() + synthetic + [t.upper() for t in synthetic[:800]]
    data, off = synth.pack(texts)
    sp = m.wordpiece_fold_spec()
    assert sp.fold == {"both": 3, "lower": 1, "strip": 2}[mode]
    raw = count_spec(sp, data, off, 8)
    ident = count_spec(m.wordpiece_spec(), data, off, 8)
    assert (raw >= 0).sum() >= 1000
    assert ((raw >= 0) & (ident == -2)).sum() >= 500
    tabs = tok_device.assert_kernels_equal(sp, data, off, raw, runs=2, tables="wp_tables", count="wp_count")
    offsets = native.host().DEV_WP_OFFSETS
    assert all(tok_device.block_pointer(tabs.block, offsets, f) for f in ("fold1", "fold2", "foldp"))


def test_device_engine_counts_uncased_text(tok_dir):
    from test_emulated_device_path import outputs
    from test_wordpiece import _cfg

    from textblaster_amd.ops import hiprt
    from textblaster_amd.pipeline.engine import Engine
    from textblaster_amd.utils import metrics

    assert BACKEND != "cuda" or hiprt.device_count() > 0
    tok = fc.train(str(tok_dir / "both.json"), True, None)
    pad = " og det er en god dag i dag, vi skal ud at g\u00e5 en tur i skoven med hunden." * 3
    pool = [t + pad for t in fc.pool_docs()]  # long enough to pass the quality filters
    texts = synth.make_corpus(6000, 1000, seed=14) + pool
    data, off = synth.pack(texts)
    b = Engine(_cfg(), backend="cpu", nthreads=8, keep_reasons=True, tokenizer_file=tok,
               segmentation="icu").process(data, off)
    host = fc.needs_host(True, tok)
    eng = Engine(_cfg(), backend=BACKEND, keep_reasons=True, tokenizer_file=tok)
    assert eng.device_runner.bpe
    seen = []
    host_step = eng._host_step

    def spy(bs, i, ndocs, resolved=None, matched=None):
        if resolved is not None:  # the device's kept outputs and their counts, as the TokenCounter step gets them
            seen.append(resolved)
        return host_step(bs, i, ndocs, resolved, matched)

    eng._host_step = spy
    for _ in range(2):
        del seen[:]
        h0, d0 = metrics.BPE_HOST_DOCS_TOTAL._value.get(), metrics.BPE_DEVICE_DOCS_TOTAL._value.get()
        a = eng.process(data, off)
        nh = metrics.BPE_HOST_DOCS_TOTAL._value.get() - h0
        nd = metrics.BPE_DEVICE_DOCS_TOTAL._value.get() - d0
        np.testing.assert_array_equal(a.status, b.status)
        assert outputs(a) == outputs(b)
        # the documents the device left to the host tokenizer are exactly the kept outputs (of the
        # documents it did not delegate to the CPU path as a whole) with added-token text or a
        # context-dependent code point
        assert seen
        n_pred = n_kept = n_pool = 0
        for rs in seen:
            nk = rs.counts()[0]
            toks = np.asarray(rs.kept_tokens(2))
            kept = [bytes(rs.out[rs.out_off[k]:rs.out_off[k + 1]]).decode("utf-8") for k in range(nk)]
            predicted = [k for k, t in enumerate(kept) if host(t)]
            assert len(toks) == nk and np.nonzero(toks == -2)[0].tolist() == predicted and (toks >= -2).all()
            n_pred, n_kept = n_pred + len(predicted), n_kept + nk
            n_pool += sum(1 for k, t in enumerate(kept) if t.endswith(pad) and toks[k] >= 0)
        assert n_pred > 50 and nh == n_pred and nh + nd == n_kept and nd > 1000
        assert n_pool > 20  # pool documents counted by the kernel
