"""Duplicated lines and paragraphs of one-wave documents: the wave stage kernel compares up to 64
spans lane against lane in registers and keys its table by the spans' own ends above that, with no
prefix hash of the text. The host emulation keeps the prefix-hash keys and the table, so it is an
independent oracle: records and flags must be equal for GopherRepetition in split mode, for
FineWebQuality, and for two GopherRepetition steps (no export: the kernel keeps its prefix hash and
the in-stage n-gram code). Hand-built documents around the lane limit, around the 8-byte signature
and on the table path. Needs an MI355X."""
import copy

import numpy as np
import pytest

from textblaster_amd.config import load_pipeline_config
from textblaster_amd.utils import synth

pytestmark = pytest.mark.gpu

COUNTS = (0, 1, 2, 3, 63, 64, 65, 66, 129)


def _distinct(n):
    """n different lines; seven groups share their first 8 bytes and most of them a length, so the
    lane path compares bytes and finds them unequal."""
    return [f"row {i % 7} of tab, entry {i}" for i in range(n)]


def _documents():
    docs = {}
    # span counts around the 64 lanes: no repeats, one repeat at either end, all equal
    for n in COUNTS:
        docs[f"lines{n}_distinct"] = "\n".join(_distinct(n))
        docs[f"lines{n}_equal"] = "\n".join(["the very same line of text"] * n)
        if n >= 2:
            d = _distinct(n - 1)
            docs[f"lines{n}_first_again_last"] = "\n".join(d + [d[0]])
            docs[f"lines{n}_last_again_first"] = "\n".join([d[-1]] + d)
    # signature collisions on the lane path: one length, the same first and last 8 bytes
    mid = [f"HEADHEAD{i:04d}TAILTAIL" for i in range(12)]
    docs["sig_middle_differs"] = "\n".join(mid)
    docs["sig_middle_one_pair"] = "\n".join(mid[:8] + [mid[3]] + mid[8:])
    docs["sig_short"] = "\n".join(["a", "b", "ab", "a", "abc", "abcdefg", "abcdefh", "abcdefg", "ab", "ba"])
    docs["sig_last_byte"] = "\n".join([f"the same line up to its end {c}" for c in "ABCDBEFA"])
    lens = []
    for k in (7, 8, 9, 16, 17):
        base = "abcdefghijklmnopqrstuvwxyz"[:k]
        lens += [base, base[:-1] + "#", base, base[:k // 2] + "#" + base[k // 2 + 1:]]
    docs["sig_lengths"] = "\n".join(lens)
    # the same lengths on the table path (more than 64 spans), keyed by the spans' ends
    docs["table_lengths"] = "\n".join(lens * 4 + [f"filler {i}" for i in range(20)])
    # a collision chain on the table path: one length, one head, one tail, some equal pairs
    al = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
    chain = []
    for i in range(215):
        j = i - 5 if i % 10 == 9 else i
        chain.append("ABCDEFGH" + al[j // 62] + al[j % 62] + "STUVWXYZ")
    assert all(len(c) == 18 for c in chain)
    docs["table_chain"] = "\n".join(chain)
    docs["table_all_equal"] = "a\n" * 2000
    # paragraphs
    docs["paras_runs"] = "para one\nsecond line\n\nother\n\n\npara one\nsecond line\n\n\nother\n\nlast"
    docs["paras_equal_line"] = "alpha\n\nalpha\nbeta\n\nbeta\n\nalpha"
    for n in (63, 64, 65):
        p = [f"p{i} text" for i in range(n - 2)]
        docs[f"paras{n}"] = "\n\n".join(p[:5] + [p[2]] + p[5:] + [p[0]])
        docs[f"paras{n}_distinct"] = "\n\n\n".join(f"q{i} body" for i in range(n))
    # trimmed ends, separators, non-ASCII, case
    docs["trim"] = "   first line\nsecond\nfirst line\n\nsecond\n\n"
    docs["crlf"] = "one\r\ntwo\r\none\r\ntwo\r\n\r\none\r\nend"
    docs["nonascii"] = "æøå\n…\n\næøå\n…\n\nÆØÅ\n…"
    docs["case"] = "Hello World\nhello world\n\nHello World\nhello world\n\nhello World\nhello world"
    # FineWeb's spans are the non-blank lines
    docs["blank_between"] = "x line\n\n   \nx line\n \t \ny line\nx line\n\n\ny line"
    for n in (64, 65):
        d = _distinct(n - 1)
        docs[f"nonblank{n}"] = "\n \n".join(d[:10] + [d[4]] + d[10:])
    # the unchanged workgroup path
    docs["workgroup"] = "\n".join(_distinct(165) + _distinct(25)) + "\n\n" + "\n".join(_distinct(20))
    return docs


# documents built with repeated lines / paragraphs / non-blank lines
LINE_REPEATS = ["lines2_equal", "lines64_equal", "lines129_equal", "lines3_first_again_last", "lines64_last_again_first",
                "lines65_first_again_last", "lines129_last_again_first", "sig_middle_one_pair", "sig_short",
                "sig_last_byte", "sig_lengths", "table_lengths", "table_chain", "table_all_equal", "trim", "crlf",
                "nonascii", "case", "blank_between", "nonblank64", "nonblank65", "workgroup"]
PARA_REPEATS = ["paras_runs", "paras_equal_line", "paras63", "paras64", "paras65", "nonascii", "case"]


def _config(kind):
    cfg = load_pipeline_config("config/bench_pipeline.yaml")
    gr = [s for s in cfg.pipeline if s.type == "GopherRepetitionFilter"]
    fw = [s for s in cfg.pipeline if s.type == "FineWebQualityFilter"]
    assert len(gr) == 1 and len(fw) == 1
    cfg.pipeline = {"gr": gr, "fw": fw, "gr2": [gr[0], copy.deepcopy(gr[0])]}[kind]
    return cfg


@pytest.fixture(scope="module")
def runs(host):
    from textblaster_amd.ops import hiprt
    from textblaster_amd.pipeline.engine import Engine

    assert hiprt.device_count() > 0
    docs = _documents()
    data, off = synth.pack(list(docs.values()))
    out = {}
    for kind in ("gr", "fw", "gr2"):
        dev = Engine(_config(kind), backend="cuda", device="cuda:0").device_runner
        emu = Engine(_config(kind), backend="emulate", nthreads=4).device_runner
        out[kind] = (dev, dev.run(data, off), emu.run(data, off))
    return docs, np.diff(off), out


def test_documents_cover_the_routes(runs):
    docs, lens, out = runs
    by = dict(zip(docs, lens))
    dev = out["gr"][0]
    assert dev.gr_split, "one GopherRepetition step: split mode"
    assert not out["gr2"][0].gr_split, "two GopherRepetition steps: no export"
    for name, n in by.items():
        if name == "workgroup":
            assert n > dev.long_doc_bytes
        else:
            assert n <= dev.long_doc_bytes, name
    assert 4800 <= by["workgroup"] <= 6000
    for n in COUNTS:
        assert docs[f"lines{n}_distinct"].count("\n") == max(n - 1, 0)
    assert docs["table_chain"].count("\n") + 1 > 64


@pytest.mark.parametrize("kind", ["gr", "fw", "gr2"])
def test_records_and_flags_equal_host_emulation(runs, kind):
    docs, lens, out = runs
    _, a, b = out[kind]
    names = list(docs)
    n = len(names)
    # no document may be flagged: a flagged one would leave the comparison
    assert not a.flags.any(), [names[i] for i in np.nonzero(a.flags)[0]]
    assert not b.flags.any(), [names[i] for i in np.nonzero(b.flags)[0]]
    assert len(a.stage_recs) == len(b.stage_recs) == 1
    steps = 2 if kind == "gr2" else 1
    width = len(a.stage_recs[0]) // (n * steps)
    x = np.asarray(a.stage_recs[0]).reshape(steps, n, width)
    y = np.asarray(b.stage_recs[0]).reshape(steps, n, width)
    assert x.shape == y.shape
    bad = np.argwhere(~np.all(x == y, axis=2))
    assert len(bad) == 0, [(names[i], x[s, i].tolist(), y[s, i].tolist()) for s, i in bad[:4]]
    # the documents do exercise the duplicate fields
    for s in range(steps):
        rec = dict(zip(names, x[s]))
        if kind == "fw":
            for name in LINE_REPEATS:
                assert rec[name][3] > 0, name
        else:
            for name in LINE_REPEATS:
                assert rec[name][5] > 0 and rec[name][6] > 0, name
            for name in PARA_REPEATS:
                assert rec[name][2] > 0 and rec[name][3] > 0, name
