"""K18 on the GPU: k_meta_size / k_meta_write (csrc/hip/resolve.hip) against their host emulation
over the record matrices of tests/meta_matrix.py, and the DeviceRunner's metadata column against
BatchState.assemble over the records it downloaded. Needs an MI355X."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meta_matrix as mm  # noqa: E402

from textblaster_amd import native  # noqa: E402
from textblaster_amd.pipeline import tuning  # noqa: E402
from textblaster_amd.utils import metrics, synth  # noqa: E402

pytestmark = pytest.mark.gpu

LDS_SLICE = 260  # resolve.hip kMetaSlice: longer rows are written straight to the column


@pytest.fixture(scope="module")
def kern():
    from textblaster_amd.ops import hiprt
    from textblaster_amd.ops.kernels import Kernels

    assert hiprt.device_count() > 0
    hiprt.set_device(0)
    return Kernels(0), hiprt


@pytest.fixture(scope="module")
def base_case():
    return mm.default_case()


def run_kernels(kern, c, row_cap=0):
    """tb_resolve over the case's records (empty texts), then tb_meta_format; returns the column
    (bytes, offsets, validity, error word) cut to the nk + nx output rows."""
    k, rt = kern
    n = c.n
    h = native.host()
    mblob = c.plan(row_cap)
    rp, mp = rt.to_device(c.resolve), rt.to_device(mblob)
    recs = [rt.to_device(r) for r in c.recs]
    flags, vb, vo = rt.zeros(n, np.uint32), rt.zeros(16, np.uint8), rt.zeros(n + 1, np.int64)
    fail, status, fver = rt.empty(n, np.int32), rt.empty(n, np.uint8), rt.empty(n, np.uint8)
    lanes, sc = rt.empty(4 * n, np.int64), rt.empty(4 * n, np.int64)
    out, out_off, rows, err = rt.zeros(16, np.uint8), rt.zeros(n + 1, np.int64), rt.zeros(n, np.int32), rt.zeros(1, np.int32)
    k.resolve(rp, recs, n, flags, [(vb, vo)], fail, status, fver, lanes, sc, out, out_off, rows, err)
    hfail, _, hrows, nk, nx = c.host_resolve()
    np.testing.assert_array_equal(fail.to_host(), hfail)
    np.testing.assert_array_equal(rows.to_host()[:nk + nx], hrows[:nk + nx])
    assert int(err.to_host()[0]) == 0
    toks = []
    for t in c.kept_tokens(hrows, nk):
        pad = np.full(n, -7, dtype=np.int32)
        pad[:nk] = t
        toks.append(rt.to_device(pad))
    cap = max(h.meta_plan_row_cap(mblob) * n, 1)
    lens, off, valid = rt.empty(n, np.int64), rt.zeros(n + 1, np.int64), rt.empty(n, np.uint8)
    col, merr = rt.empty(cap, np.uint8), rt.zeros(1, np.int32)
    k.meta_format(rp, mp, recs, n, fail, rows, sc, toks, lens, off, valid, col, merr)
    o = off.to_host()
    merr = int(merr.to_host()[0])
    total = int(o[nk + nx]) if not merr & h.META_ERR_OVERFLOW else 0
    return bytes(col.to_host()[:total]), o[:nk + nx + 1], valid.to_host()[:nk + nx], merr, o


def assert_equals_emulation(kern, c, row_cap=0):
    md, mo, mv, err, full_off = run_kernels(kern, c, row_cap)
    emd, emo, emv, eerr = c.emulate(row_cap)
    assert err == eerr == 0
    np.testing.assert_array_equal(mo, emo)
    np.testing.assert_array_equal(mv, emv)
    assert md == bytes(emd)
    # rows past the last output row have length 0
    assert np.all(full_off[len(mo) - 1:] == full_off[len(mo) - 1])
    return md, mo, mv


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4001])
def test_kernels_equal_emulation_on_the_matrix(kern, base_case, n):
    c = base_case if n == base_case.n else base_case.tiled(n)
    md, mo, mv = assert_equals_emulation(kern, c)
    if n >= base_case.n:
        # and the emulation is the host assembly (tests/test_device_meta.py), checked here once more
        # on the bytes the device wrote
        emd, emo, emv, _ = c.expected()
        assert md == emd and np.array_equal(mo, emo) and np.array_equal(mv, emv)
        lens = np.diff(mo)
        assert lens.max() > LDS_SLICE and 0 < lens[lens > 0].min() <= LDS_SLICE  # both write paths ran


@pytest.mark.parametrize("name", ["LanguageDetectionFilter", "GopherRepetitionFilter", "GopherQualityFilter",
                                  "C4QualityFilter", "FineWebQualityFilter", "FineWeb_exclude_zero_flipped",
                                  "fineweb_tokens"])
def test_kernels_equal_emulation_per_step_kind(kern, name):
    c = mm.all_cases()[name]
    md, mo, mv = assert_equals_emulation(kern, c)
    emd, emo, emv, _ = c.expected()
    assert md == emd and np.array_equal(mo, emo) and np.array_equal(mv, emv)


def test_all_null_batch(kern):
    cfg = mm.default_cfg()
    cfg.pipeline = [s for s in cfg.pipeline if s.type == "FineWebQualityFilter"]
    c = mm.Case(cfg, [[mm.PASS["FineWebQualityFilter"]] * 130])
    md, mo, mv = assert_equals_emulation(kern, c)
    assert md == b"" and not mo.any() and not mv.any() and len(mv) == 130


def test_every_row_past_the_lds_slice(kern):
    """Only long rows (every GopherRepetition order and fraction firing): each lane writes its
    row straight to the column."""
    cfg = mm.default_cfg()
    cfg.pipeline = [s for s in cfg.pipeline if s.type == "GopherRepetitionFilter"]
    row = [1000, 5, 5, 900, 10, 9, 800, 500, 400, 300, 900, 800, 700, 600, 500, 400]
    c = mm.Case(cfg, [[row] * 200])
    # (these rows average more than the plan's capacity per row: the test sets its own)
    md, mo, mv = assert_equals_emulation(kern, c, row_cap=1024)
    assert np.diff(mo).min() > LDS_SLICE
    assert md == c.expected()[0]


def test_overflow_and_unformattable_set_the_error_word(kern, base_case):
    h = native.host()
    md, mo, mv, err, _ = run_kernels(kern, base_case, row_cap=1)
    assert err == h.META_ERR_OVERFLOW and err == base_case.emulate(1)[3] and md == b""
    c = mm.token_only_case()
    c.tokens = np.array([5, -2, 7, -1, 9], dtype=np.int64)
    assert run_kernels(kern, c)[3] == h.META_ERR_UNFORMATTABLE == c.emulate()[3]


def test_device_runner_metadata_equals_host_assembly(tmp_path_factory):
    """DeviceRunner end to end with the default configuration (its TokenCounter counted by
    k_bpe_count with a locally trained byte-level BPE): the downloaded metadata column equals
    assemble(rows, False) over the same downloaded records on both sides, and a second submission
    of the batch gives identical buffers."""
    from test_gpu_kernels import EDGE

    from textblaster_amd.models.tokenizer import train_synthetic_bpe
    from textblaster_amd.pipeline.engine import Engine

    tok = train_synthetic_bpe(str(tmp_path_factory.mktemp("tok") / "bpe2k.json"), vocab_size=2000, n_docs=600, seed=2)
    data, off = synth.pack(synth.make_corpus(3000, 1024, seed=11) + EDGE)
    eng = Engine(mm.default_cfg(), backend="cuda", device="cuda:0", tokenizer_file=tok,
                 tune=tuning.parse("device_meta=1"))
    assert eng.device_runner.meta_t is not None and eng.device_runner.bpe

    def submit():
        sub = eng.submit(data, off)
        sub.dev = sub.dev.wait()
        return sub

    sub = submit()
    r = sub.dev.resolved
    assert r is not None and r.meta is not None
    nk, nx = r.counts()
    host_counted = int(np.count_nonzero(r.tokens[max(r.tokens)][:nk] < 0))
    assert (r.meta_err != 0) == (host_counted > 0)  # only a count left to the host tokenizer is unformattable
    before = metrics.DEVICE_META_FALLBACK_TOTAL._value.get()
    a = eng.finish(sub)
    assert metrics.DEVICE_META_FALLBACK_TOTAL._value.get() == before + (1 if r.meta_err else 0)
    # the same records without the device column: BatchState.assemble(rows, False)
    sub.dev = dataclasses.replace(sub.dev, resolved=dataclasses.replace(r, meta=None, meta_err=0, moved=None))
    b = eng.finish(sub)
    assert a.n_kept == b.n_kept > 0 and a.n_excluded == b.n_excluded > 0
    for pa, pb in zip(a.kept + a.excluded, b.kept + b.excluded):
        np.testing.assert_array_equal(pa.rows, pb.rows)
        np.testing.assert_array_equal(pa.meta_off, pb.meta_off)
        np.testing.assert_array_equal(pa.meta_valid, pb.meta_valid)
        assert bytes(pa.meta_data) == bytes(pb.meta_data)
    if not r.meta_err:
        # (with a host-counted document the comparison above went through the host on both sides:
        # compare the device column of the rows that have their counts directly as well)
        md, mo, mv = r.meta
        kept = b.kept[0]
        assert bytes(md[:int(mo[nk])]) == bytes(kept.meta_data)
    md, mo, mv = (np.array(x) for x in r.meta)
    r2 = submit().dev.resolved
    assert r2.meta_err == r.meta_err
    np.testing.assert_array_equal(r2.meta[1][:nk + nx + 1], mo[:nk + nx + 1])
    np.testing.assert_array_equal(r2.meta[2][:nk + nx], mv[:nk + nx])
    if not r.meta_err & native.host().META_ERR_OVERFLOW:
        tot = int(mo[nk + nx])
        assert bytes(r2.meta[0][:tot]) == bytes(md[:tot])
