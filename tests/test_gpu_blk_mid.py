"""Mid-sized workgroup documents run the 256-thread build of the workgroup stage kernel
(k_stage_analyze_blk_mid) when all of a batch's workgroup documents are at most
device.MID_DOC_BYTES long, and the full-size kernel when one is longer. Every batch goes through the default pipeline on the GPU and through the
host emulation, which knows neither kernel: stage and C4 records, flags, status, first failing
step and output bytes must be equal document for document, with the step gates as shipped and
with them off (so that the stage kernels also analyse documents an earlier step filtered).
Documents at every routing threshold, documents whose code points, lines and words straddle the
edges of a 256-lane pass, repeated text. The launch split is a pure function (no GPU needed)."""
import numpy as np
import pytest

from textblaster_amd.config import load_pipeline_config
from textblaster_amd.pipeline import device as devmod
from textblaster_amd.utils import synth

MID = devmod.MID_DOC_BYTES


def _sized(nbytes, seed):
    """Synthetic text of exactly ``nbytes`` UTF-8 bytes."""
    text = "\n".join(synth.make_corpus(64, 1024, seed=seed, langs=("eng",)))
    while len(text.encode()) < nbytes:
        text += "\n" + text
    cut = text.encode()[:nbytes].decode("utf-8", errors="ignore")
    cut += "x" * (nbytes - len(cut.encode()))
    assert len(cut.encode()) == nbytes
    return cut


def _routing_sizes():
    # longest first: the launch order sorts 16-byte buckets and keeps the input order inside one
    return sorted({32769, 32768, MID + 1, MID, MID - 1, 4097, 4096, 1024}, reverse=True)


def _routing_batch(split=True):
    """Documents at every routing threshold; without the split document (32,769 bytes) the
    workgroup documents all take the mid-size kernel, with it the full-size one."""
    return {f"bytes{n}": _sized(n, seed=n) for n in _routing_sizes() if split or n <= 32768}


def _partition_batch():
    para = ("The quick brown fox jumps over the lazy dog near the bank of the river, and the dog does not "
            "mind it at all. Then it rains for a while and everyone goes home to read the paper again.")
    eols = ["\r\n", "\n", "\n\n", "\r\n\r\n"]
    docs = {
        # one byte, then 4-byte code points: every sequence straddles a 4-byte boundary, and one
        # straddles every 64-byte and every 256-lane chunk edge
        "cp4": "a" + "".join(chr(0x1F600 + i % 64) for i in range(1536)),
        # 1-, 2- and 3-byte code points in a 7-byte period (coprime to 64)
        "cp123": "aé€ " * 880,
        "one_line_no_space": "abcdefghij" * 615,
        # more lines than threads, with empty lines and CRLF
        "lines600": "".join(f"line {i}" + eols[i % 4] for i in range(600)),
        # more than 2,048 words of one and two letters
        "words2200": "a bc " * 1100,
        # one repeated paragraph: duplicated lines / paragraphs and the in-stage n-gram tables
        "repeated_paragraph": "\n\n".join([para] * 28),
    }
    return docs


def launch_split(lens, long_doc_bytes, split_doc_bytes, mid_doc_bytes):
    """(n_long, n_split, n_mid) of a batch as DeviceRunner launches it (no pre-pass documents)."""
    lens = np.asarray(lens, dtype=np.int64)
    lp = lens[devmod.launch_order(lens)]
    n_long = int(np.count_nonzero(lens > long_doc_bytes))
    huge = np.nonzero(lp[:n_long] > split_doc_bytes)[0]
    n_split = int(huge[-1]) + 1 if len(huge) else 0
    return n_long, n_split, devmod.blk_mid_count(lp[:n_long], 0, n_split, mid_doc_bytes)


def test_blk_mid_count_is_all_or_none():
    f = devmod.blk_mid_count
    lens = np.array([32768, 8193, 8192, 8191, 4097])
    assert f(lens, 0, 0, 32768) == 5
    assert f(lens, 0, 0, 32767) == 0 and f(lens, 0, 0, 8192) == 0  # one longer document: none
    assert f(lens, 0, 1, 32768) == 0  # a split document outside the pre-pass prefix: none
    assert f(lens, 0, 0, 0) == 0 and f(lens[:0], 0, 0, 32768) == 0
    # pre-pass documents have a launch of their own and do not count, split or not
    big = np.array([400000, 300000, 32768, 5000])
    assert f(big, 2, 2, 32768) == 2 and f(big, 2, 0, 32768) == 2
    assert f(big, 1, 2, 32768) == 0 and f(big, 0, 0, 32768) == 0
    assert f(big, 4, 4, 32768) == 0 and f(big, 3, 3, 32768) == 1


def test_routing_sizes_take_their_paths():
    sizes = _routing_sizes()
    n_long, n_split, n_mid = launch_split(sizes, 4096, 32768, MID)
    assert n_long == sum(s > 4096 for s in sizes) and n_split == 1 and n_mid == 0  # 32,769 bytes: split
    n_long, n_split, n_mid = launch_split(sizes[1:], 4096, 32768, MID)
    assert n_long == sum(4096 < s <= 32768 for s in sizes) and n_split == 0
    assert n_mid == (n_long if MID >= 32768 else 0)


def _engines(monkeypatch_ctx, tune):
    from textblaster_amd.pipeline.engine import Engine

    if tune:
        monkeypatch_ctx.setenv("TB_TUNE", tune)
    else:
        monkeypatch_ctx.delenv("TB_TUNE", raising=False)
    cfg = load_pipeline_config("config/bench_pipeline.yaml")
    dev = Engine(cfg, backend="cuda", device="cuda:0").device_runner
    emu = Engine(load_pipeline_config("config/bench_pipeline.yaml"), backend="emulate", nthreads=4).device_runner
    return dev, emu


def _spy(dev):
    """Records (n_launch, mid) of every workgroup stage launch of ``dev``."""
    orig, calls = dev.k.stage_analyze_blk, []

    def stage_analyze_blk(plan, stage, docs, *args, **kw):
        calls.append((int(docs.n_launch), bool(kw.get("mid", False))))
        return orig(plan, stage, docs, *args, **kw)

    dev.k.stage_analyze_blk = stage_analyze_blk
    return calls


@pytest.fixture(scope="module", params=["", "gate=0"], ids=["gated", "gate_off"])
def runs(host, request):
    from textblaster_amd.ops import hiprt

    assert hiprt.device_count() > 0
    with pytest.MonkeyPatch.context() as mp:
        dev, emu = _engines(mp, request.param)
        out = {}
        spied = _spy(dev)
        for name, docs in (("routing", _routing_batch()), ("routing_mid", _routing_batch(split=False)),
                           ("partition", _partition_batch())):
            data, off = synth.pack(list(docs.values()))
            del spied[:]
            a = dev.run(data, off)
            calls = list(spied)
            again = dev.run(data, off) if name == "routing_mid" else None
            out[name] = (docs, np.diff(off), calls, a, emu.run(data, off), again)
        yield dev, out


def _outputs(res):
    r = res.resolved
    assert r is not None and r.err == 0
    out = {}
    for side, parts in zip(("kept", "excluded"), r.parts()):
        for rows, off, text in parts:
            for k, d in enumerate(np.asarray(rows).tolist()):
                out[d] = (side, bytes(text[int(off[k]):int(off[k + 1])]))
    return out


def _assert_equal(names, a, b):
    n = len(names)
    np.testing.assert_array_equal(np.asarray(a.flags), np.asarray(b.flags))
    assert not np.asarray(a.flags).any(), [names[i] for i in np.nonzero(np.asarray(a.flags))[0]]
    assert len(a.stage_recs) == len(b.stage_recs) >= 2
    for s, (x, y) in enumerate(zip(a.stage_recs, b.stage_recs)):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and len(x) % n == 0
        # (step-major layout: step k's fields of document d at rec_prefix[k] * n + d * width[k])
        bad = np.nonzero(x != y)[0]
        assert len(bad) == 0, (s, bad[:8].tolist(), x[bad[:8]].tolist(), y[bad[:8]].tolist())
    assert sorted(a.c4_recs) == sorted(b.c4_recs)
    for i in a.c4_recs:
        np.testing.assert_array_equal(np.asarray(a.c4_recs[i]), np.asarray(b.c4_recs[i]))
    np.testing.assert_array_equal(a.resolved.status, b.resolved.status)
    np.testing.assert_array_equal(a.resolved.fail, b.resolved.fail)
    oa, ob = _outputs(a), _outputs(b)
    assert sorted(oa) == sorted(ob)
    for d in oa:
        assert oa[d] == ob[d], names[d]


@pytest.mark.gpu
@pytest.mark.parametrize("batch", ["routing", "routing_mid"])
def test_routing_edges_equal_host_emulation(runs, batch):
    dev, out = runs
    docs, lens, calls, a, b, _ = out[batch]
    assert lens.tolist() == [n for n in _routing_sizes() if batch == "routing" or n <= 32768]
    assert dev.long_doc_bytes == 4096 and dev.split_doc_bytes == 32768
    n_long, n_split, n_mid = launch_split(lens, dev.long_doc_bytes, dev.split_doc_bytes, MID)
    assert n_split == (batch == "routing") and 1024 in lens and 4096 in lens  # (two wave documents)
    # every stage launches the workgroup documents once: full size with the split document, else mid
    assert n_mid == (0 if batch == "routing" else n_long) and n_long == len(lens) - 2
    assert calls == [(n_long, n_mid > 0)] * len(a.stage_recs)
    _assert_equal(list(docs), a, b)
    if not dev.gating:
        # with the gates off every stage kernel analysed every document
        assert np.asarray(a.stage_recs[0]).any() and np.asarray(a.stage_recs[1]).any()


@pytest.mark.gpu
def test_partition_edges_equal_host_emulation(runs):
    dev, out = runs
    docs, lens, calls, a, b, _ = out["partition"]
    by = dict(zip(docs, lens.tolist()))
    assert all(dev.long_doc_bytes < n <= min(MID, 8192) for n in by.values()), by
    assert 6000 <= by["cp4"] <= 6400 and 6000 <= by["cp123"] <= 6400 and 6000 <= by["one_line_no_space"] <= 6400
    assert docs["lines600"].count("\n") > 512 and "\r\n" in docs["lines600"] and "\n\n" in docs["lines600"]
    assert len(docs["words2200"].split()) > 2048
    assert 5000 <= by["repeated_paragraph"] <= 5400
    # all of them are mid-size documents: one launch per stage, of the 256-thread kernel
    assert calls == [(len(docs), True)] * len(a.stage_recs)
    _assert_equal(list(docs), a, b)


@pytest.mark.gpu
def test_two_runs_give_the_same_records(runs):
    _, out = runs
    _, _, _, a, _, again = out["routing_mid"]
    np.testing.assert_array_equal(np.asarray(a.flags), np.asarray(again.flags))
    for x, y in zip(a.stage_recs, again.stage_recs):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    for i in a.c4_recs:
        np.testing.assert_array_equal(np.asarray(a.c4_recs[i]), np.asarray(again.c4_recs[i]))
    np.testing.assert_array_equal(a.resolved.status, again.resolved.status)
    np.testing.assert_array_equal(a.resolved.fail, again.resolved.fail)
    assert _outputs(a) == _outputs(again)
