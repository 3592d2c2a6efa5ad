"""k_bpe_case_count / k_bpe_case_long and the NFC-gated count kernels on the GPU (csrc/hip/bpe.hip,
csrc/common/bpe_case.h, bpe_nfc_range of csrc/common/bpe.h): array for array against the host
emulation (which tests/test_bpe_case.py pins to the `tokenizers` library), and the device pipeline
with a trailing TokenCounter on a Qwen2-layout (pattern B + NFC) and an o200k-layout (pattern C)
tokenizer against the CPU path."""
import importlib.util
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bpe_case_corpus as cc  # noqa: E402
import bpe_split_corpus as bc  # noqa: E402
import tok_device  # noqa: E402

from textblaster_amd.models.tokenizer import TokenCounterModel, count_spec, train_synthetic_split_bpe  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("tok")


def _tokenizer(tok_dir, pattern, ignore_merges, nfc=False):
    return train_synthetic_split_bpe(str(tok_dir / f"case4k_{pattern}{int(ignore_merges)}{int(nfc)}.json"),
                                     vocab_size=4000, pattern=pattern, ignore_merges=ignore_merges, n_docs=1500, seed=2,
                                     nfc=nfc)


def _cut(text, nbytes):
    return text.encode("utf-8")[:nbytes].decode("utf-8", "ignore")


def lane_edge_docs():
    """Documents whose rules straddle the lane ranges: 1,100 bytes (chunks over 16 bytes) and 200 KB,
    of pattern C's unit string (it holds U+0301: to the host behind the NFC gate) and of patterns
    A / B's (no code point from U+0300 up), 3 KB without a sync point (digits and punctuation on one line; letters with an apostrophe as
    the only non-letter), case runs repeated to 2,048 bytes so that the case state crosses every
    lane edge, the punctuation tail repeated, pre-tokens around the 64-byte lane arrays and the
    2048-byte limit, and an added token's text across the edge of lanes 0 and 1."""
    nosync = ("1234567,.;: 89!? " * 200)[:3072]
    assert "\n" not in nosync and not any(c.isalpha() for c in nosync)
    apos = ("ab'cd'ef'" * 400)[:3072]
    return ([_cut(cc.UNIT * 40, 1100), _cut(cc.UNIT * 4000, 200 * 1024), _cut(bc.UNIT * 40, 1100),
             _cut(bc.UNIT * 9000, 200 * 1024), nosync, apos,
             _cut("AbcDEFgh" * 300, 2048), _cut("あAあB" * 300, 2048), "!\n/\n/\nx" * 120]
            + ["q" * n + " tail" for n in (64, 65, 2048, 2049)] + ["Q" * 2048 + "q tail", "Qq" + "あ" * 700]
            + ["0123456789" + cc.ADDED + " and more text after it", "0123 " + cc.ADDED[:-1] + " not one"])


def nfc_edge_docs():
    """2,048 bytes (32-byte chunks) with two NFC_QC=Yes marks of different non-zero class on either
    side of the edge of lanes 3 and 4 (byte 128): U+05B4 (class 14) then U+05B0 (class 10), out of
    order, and the two in order; and a Maybe (U+093C) as the first code point of a lane."""
    def doc(base, first, second):
        head = ("word " * 40)[:128 - len((base + first).encode("utf-8"))] + base + first
        assert len(head.encode("utf-8")) == 128
        t = head + second
        t += " tail" * ((2048 - len(t.encode("utf-8"))) // 5)
        assert 1985 <= len(t.encode("utf-8")) <= 2048
        return t
    return [doc("\u05d0", "\u05b4", "\u05b0"), doc("\u05d0", "\u05b0", "\u05b4"), doc("\u0915", "", "\u093c")]


CASES = [("C", True, False), ("D", False, False), ("B", False, True), ("C", False, True)]


@pytest.mark.parametrize("pattern,ignore_merges,nfc", CASES, ids=["C-ignore_merges", "D-merges", "B-nfc", "C-nfc"])
def test_case_and_nfc_kernels_equal_host(tok_dir, pattern, ignore_merges, nfc):
    """The kernels directly on packed documents (no K16 count pointer) vs the host emulation."""
    from tokenizers import normalizers

    m = TokenCounterModel(_tokenizer(tok_dir, pattern, ignore_merges, nfc))
    docs, host = cc.corpus()
    edges = lane_edge_docs()
    texts = docs + edges + cc.NFC_CLEAN + (nfc_edge_docs() if nfc else [])
    data, off = synth.pack(texts)
    sp = m.bpe_spec()
    assert sp is not None and sp.kind == {"B": 2, "C": 3, "D": 4}[pattern] and sp.nfc is nfc
    assert sp.ignore_merges == ignore_merges
    raw = count_spec(sp, data, off, 8)
    by_text = {t: int(raw[k]) for k, t in enumerate(texts)}
    assert all(raw[k] == -2 for k in host)
    assert by_text["q" * 2049 + " tail"] == -2 and by_text["q" * 2048 + " tail"] > 0
    assert by_text["0123456789" + cc.ADDED + " and more text after it"] == -2
    assert all(by_text[t] >= 0 for t in edges[2:9] + cc.NFC_CLEAN)
    assert all((by_text[t] == -2) if nfc else (by_text[t] > 0) for t in edges[:2])
    if nfc:
        nz = normalizers.NFC().normalize_str
        bad_order, in_order, maybe = nfc_edge_docs()
        assert nz(bad_order) != bad_order and nz(in_order) == in_order
        assert by_text[bad_order] == -2 and by_text[in_order] > 0 and by_text[maybe] == -2
        assert not any(r >= 0 and nz(t) != t for r, t in zip(raw.tolist(), texts))
    else:
        assert (raw >= 0).sum() >= len(texts) - len(host) - 5
    tok_device.assert_kernels_equal(sp, data, off, raw)


@pytest.mark.parametrize("pattern,ignore_merges,nfc", [("B", False, True), ("C", True, False)], ids=["B-nfc", "C"])
def test_device_token_counts_equal_cpu(tok_dir, pattern, ignore_merges, nfc):
    """Engine(cuda) with a trailing TokenCounter: the host tokenizer sees exactly the kept documents
    that NFC changes or that hold a code point the gate does not resolve (none without the
    normalizer, none in the synthetic part), and statuses and outputs equal the CPU path's."""
    from test_bpe import _cfg
    from tokenizers import normalizers

    tok = _tokenizer(tok_dir, pattern, ignore_merges, nfc)
    synth_docs = synth.make_corpus(6000, 1000, seed=14)
    texts = synth_docs + cc.fuzz(400, 15)
    data, off = synth.pack(texts)
    a, oa, nh, nd = tok_device.device_and_cpu(_cfg, tok, data, off)
    want = 0
    if nfc:
        spec = importlib.util.spec_from_file_location("gen_nfc_qc", os.path.join(REPO, "tools", "gen_nfc_qc.py"))
        gen = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(gen)
        tab, nz = gen.read_inc(), normalizers.NFC().normalize_str
        kept = [t.decode("utf-8") for kind, t, _ in oa.values() if kind == "kept"]
        assert len(kept) == a.n_kept
        not_proved = [t for t in kept if not gen.identity(tab, t)]
        assert all(gen.identity(tab, t) for t in synth_docs)
        assert all(nz(t) == t for t in kept if gen.identity(tab, t))  # changed or Maybe: exactly the others
        want = len(not_proved)
    assert nh == want and nd == a.n_kept - want and nd > 0
