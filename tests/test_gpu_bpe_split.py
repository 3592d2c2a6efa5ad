"""k_bpe_split_count / k_bpe_split_long on the GPU (csrc/hip/bpe.hip, csrc/common/bpe_split.h): array
for array against the host emulation (which tests/test_bpe_split.py pins to the `tokenizers`
library), and the device pipeline with a trailing TokenCounter on a Llama-3-format tokenizer against
the CPU path."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bpe_split_corpus as bc  # noqa: E402
import tok_device  # noqa: E402

from textblaster_amd.models.tokenizer import TokenCounterModel, count_spec, train_synthetic_split_bpe  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("tok")


def _tokenizer(tok_dir, pattern, ignore_merges):
    return train_synthetic_split_bpe(str(tok_dir / f"split4k_{pattern}{int(ignore_merges)}.json"), vocab_size=4000,
                                     pattern=pattern, ignore_merges=ignore_merges, n_docs=1500, seed=2)


def lane_edge_docs():
    """Documents whose rules straddle the lane ranges: a 1,100-byte one (chunks over 16 bytes), one
    of 200 KB, 3 KB of digits and punctuation on one line (no sync point: lane 0 counts it alone),
    pre-tokens around the 64-byte lane arrays and the 2048-byte limit, and an added token's text
    across the edge of lanes 0 and 1."""
    big = (bc.UNIT * (200 * 1024 // len(bc.UNIT.encode("utf-8")) + 1)).encode("utf-8")[:200 * 1024].decode("utf-8",
                                                                                                         "ignore")
    nosync = ("1234567,.;: 89!? " * 200)[:3072]
    assert "\n" not in nosync and not any(c.isalpha() for c in nosync)
    return ([(bc.UNIT * 40)[:1100], big, nosync] + ["q" * n + " tail" for n in (64, 65, 200, 2048, 2049)]
            + ["0123456789" + bc.ADDED + " and more text after it", "0123 " + bc.ADDED[:-1] + " not one"])


@pytest.mark.parametrize("pattern,ignore_merges", [("A", True), ("B", False)], ids=["A-ignore_merges", "B-merges"])
def test_split_kernel_equals_host(tok_dir, pattern, ignore_merges):
    """The kernels directly on packed documents (no K16 count pointer) vs the host emulation."""
    m = TokenCounterModel(_tokenizer(tok_dir, pattern, ignore_merges))
    docs, host = bc.corpus()
    texts = docs + lane_edge_docs()
    data, off = synth.pack(texts)
    sp = m.bpe_spec()
    assert sp is not None and sp.kind == (1 if pattern == "A" else 2) and sp.ignore_merges == ignore_merges
    raw = count_spec(sp, data, off, 8)
    by_text = {t: int(raw[k]) for k, t in enumerate(texts)}
    assert all(raw[k] == -2 for k in host) and (raw >= 0).sum() >= len(texts) - len(host) - 2
    assert by_text["q" * 2049 + " tail"] == -2 and by_text["q" * 2048 + " tail"] > 0
    assert by_text["0123456789" + bc.ADDED + " and more text after it"] == -2
    tok_device.assert_kernels_equal(sp, data, off, raw)


def test_device_token_counts_equal_cpu(tok_dir):
    from test_bpe import _cfg

    tok = _tokenizer(tok_dir, "A", True)
    texts = synth.make_corpus(6000, 1000, seed=14) + bc.fuzz(400, 15)
    data, off = synth.pack(texts)
    a, _, nh, nd = tok_device.device_and_cpu(_cfg, tok, data, off)
    assert nh == 0 and nd == a.n_kept > 0  # every kept document counted by the kernels
