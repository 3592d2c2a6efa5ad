"""k_wp_count on the GPU (csrc/hip/wordpiece.hip): array for array against its host emulation
(which tests/test_wordpiece.py pins to the `tokenizers` library), and the device pipeline with a
trailing WordPiece TokenCounter against the CPU path."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tok_device  # noqa: E402
import wordpiece_corpus as wc  # noqa: E402

from textblaster_amd.models.tokenizer import TokenCounterModel, count_spec, train_synthetic_wordpiece  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("tok")


def _tokenizer(tok_dir, lowercase):
    return train_synthetic_wordpiece(str(tok_dir / f"wp4k_{int(lowercase)}.json"), vocab_size=4000, n_docs=1500, seed=2,
                                     lowercase=lowercase)


def lane_edge_docs():
    """A document of every length 0..130 bytes (the lane ranges are 16 bytes up to 1 KB, so words,
    2-byte code points and dropped code points straddle every range edge), a 200-byte word of
    U+00E9 and one 200 KB document."""
    unit = "ab cd\u00e9f \u00adgh,ij\u200bk l\u4f60m "
    docs = []
    for n in range(131):
        b = (unit * 8).encode("utf-8")[:n]
        docs.append(b.decode("utf-8", "ignore"))
    return docs + ["x " + "\u00e9" * 100 + " y", wc.big_doc(200 * 1024, 33)]


@pytest.mark.parametrize("lowercase", [False, True], ids=["cased", "uncased"])
def test_wp_kernel_equals_host(tok_dir, lowercase):
    """k_wp_count directly on packed documents (no K16 count pointer) vs the host emulation."""
    m = TokenCounterModel(_tokenizer(tok_dir, lowercase))
    texts = wc.corpus("the") + lane_edge_docs()
    data, off = synth.pack(texts)
    sp = m.wordpiece_spec()
    raw = count_spec(sp, data, off, 8)
    assert (raw >= 0).sum() > 1000
    tok_device.assert_kernels_equal(sp, data, off, raw, tables="wp_tables", count="wp_count")


def test_device_token_counts_equal_cpu(tok_dir):
    from test_wordpiece import _cfg

    tok = _tokenizer(tok_dir, False)
    texts = synth.make_corpus(6000, 1000, seed=14) + wc.fuzz(400, 15)
    data, off = synth.pack(texts)
    tok_device.device_and_cpu(_cfg, tok, data, off)
