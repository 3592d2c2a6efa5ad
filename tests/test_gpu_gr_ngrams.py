"""GopherRepetition n-gram fields of wave documents: the k_gr_ngrams kernels build the word ids,
byte prefixes and concatenation hashes on chip from the word spans the stage kernel exports. Their
records and flags must equal the host emulation, which keeps the generic word arrays. Hand-built
documents around every boundary of the on-chip build. Needs an MI355X."""
import numpy as np
import pytest

from textblaster_amd.config import load_pipeline_config
from textblaster_amd.utils import synth

pytestmark = pytest.mark.gpu

# word capacities of the k_gr_ngrams instantiations (csrc/hip/gr_ngrams.hip, launch_gr_ngrams)
MAXW = (256, 512, 1024)


def _words(rng, n, vocab, block=12):
    """n words drawn from ``vocab``; the first ``block`` words recur twice more, so every order up
    to 10 has repeats and the greedy walk of the duplicated orders skips."""
    w = [vocab[i] for i in rng.integers(0, len(vocab), n)]
    for rep in (n // 3, 2 * n // 3):
        if rep + block <= n and rep >= block:
            w[rep:rep + block] = w[:block]
    return w


def _documents():
    rng = np.random.default_rng(17)
    short = ["a", "b", "ab", "ba", "c", "ca", "d", "e", "ee", "f"]       # <= 3 bytes with the space
    mid = ["alpha", "beta", "gamma", "delta", "eps", "zeta", "eta", "theta", "iota", "kappa", "la", "mu"]
    docs = {}
    # around every order (top 2-4, duplicated 5-10) and around the 64 lanes
    for n in (0, 1, 4, 5, 9, 10, 11, 63, 64, 65):
        docs[f"words{n}"] = " ".join(_words(rng, n, mid))
    # around the capacity of every instantiation; 1025 words fit none (the generic fallback).
    # 255-257 short words stay below ngram_big_bytes (the 256-word launch), the others above it.
    for m in MAXW:
        for n in (m - 1, m, m + 1):
            docs[f"maxw{n}"] = " ".join(_words(rng, n, short if m != 512 else mid))
    # packed-key boundary: 7, 8, 9 and 17 bytes; equal and unequal long words with one 8-byte prefix
    pk = ["abcdefg", "abcdefgh", "abcdefghi", "abcdefghj", "abcdefghi", "abcdefghijklmnopq",
          "abcdefghijklmnopr", "abcdefghijklmnopq", "abcdefgx", "abcdefg"]
    docs["packed"] = " ".join(_words(rng, 90, pk))
    docs["nonascii"] = " ".join(_words(rng, 80, ["æøå", "é", "blåbærgrød", "café", "e", "æøa", "æøå!", "naïve"]))
    docs["identical"] = " ".join(["same"] * 120)
    line = "the quick brown fox jumps over the lazy dog and runs far away today"
    docs["lines3"] = "\n".join([line] * 3)
    # equal concatenations, different word ids
    docs["split_pair"] = "ab c d e f g h i j k\na bc d e f g h i j k"
    docs["split_pair_long"] = " ".join(["ab c d e f g h i j k", "x y z", "a bc d e f g h i j k"] * 4)
    # byte prefix of the words just past 16 bits (a workgroup-path document)
    n16 = 0x10000 // 5 + 2
    docs["wl_overflow"] = " ".join(_words(rng, n16, ["abcde", "fghij", "klmno", "pqrst"]))
    assert sum(len(w) for w in docs["wl_overflow"].split()) > 0xFFFF
    return docs


@pytest.fixture(scope="module")
def runs(host):
    from textblaster_amd.ops import hiprt
    from textblaster_amd.pipeline.engine import Engine

    assert hiprt.device_count() > 0
    cfg = load_pipeline_config("config/bench_pipeline.yaml")
    cfg.pipeline = [s for s in cfg.pipeline if s.type == "GopherRepetitionFilter"]
    assert len(cfg.pipeline) == 1
    docs = _documents()
    data, off = synth.pack(list(docs.values()))
    dev = Engine(cfg, backend="cuda", device="cuda:0").device_runner
    emu = Engine(cfg, backend="emulate", nthreads=4).device_runner
    assert dev.gr_split, "the wave documents' n-gram orders must run in the n-gram kernels"
    return docs, np.diff(off), dev, dev.run(data, off), emu.run(data, off)


def test_documents_cover_the_routes(runs):
    docs, lens, dev, _, _ = runs
    by = dict(zip(docs, lens))
    assert by["maxw257"] <= dev.ngram_big_bytes < by["maxw511"]
    assert all(by[f"maxw{n}"] <= dev.long_doc_bytes for m in MAXW for n in (m - 1, m, m + 1))
    assert by["wl_overflow"] > dev.long_doc_bytes
    for name, text in docs.items():
        if name.startswith("maxw"):
            assert len(text.split()) == int(name[4:])


def test_records_and_flags_equal_host_emulation(runs):
    docs, lens, dev, a, b = runs
    names = list(docs)
    n = len(names)
    np.testing.assert_array_equal(a.flags, b.flags)
    assert not a.flags.any(), [names[i] for i in np.nonzero(a.flags)[0]]
    assert len(a.stage_recs) == len(b.stage_recs) == 1
    width = len(a.stage_recs[0]) // n
    x = a.stage_recs[0].reshape(n, width)
    y = b.stage_recs[0].reshape(n, width)
    bad = np.nonzero(~np.all(x == y, axis=1))[0]
    assert len(bad) == 0, [(names[i], x[i].tolist(), y[i].tolist()) for i in bad[:4]]
    # the documents do exercise the n-gram fields (7..: top orders, then duplicated orders)
    rec = dict(zip(names, x))
    for name in ("words65", "maxw256", "maxw513", "maxw1025", "packed", "nonascii", "identical", "lines3"):
        assert rec[name][7:].any(), name
    assert rec["split_pair_long"][7 + 3:].any()
