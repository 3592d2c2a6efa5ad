"""k_bpe_sp_count / k_bpe_sp_long on the GPU (csrc/hip/bpe.hip, csrc/common/bpe_sp.h): array for
array against the host emulation (which tests/test_bpe_sp.py pins to the `tokenizers` library), and
the device pipeline with a trailing TokenCounter on a Llama-2-layout and a Metaspace-layout tokenizer
against the CPU path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bpe_sp_corpus as sc  # noqa: E402
import tok_device  # noqa: E402

from textblaster_amd.models.tokenizer import BPE_SP, TokenCounterModel, count_spec  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402

pytestmark = pytest.mark.gpu

SP = sc.SP


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("tok")


def _cut(text, nbytes):
    return text.encode("utf-8")[:nbytes].decode("utf-8", "ignore")


NO_SPACE = ("0123456789abcdefghijklmnopqrstuvwxyz,.;:" * 80)[:3072]
SPACES = " " * 3072
CJK_EMOJI = _cut(("あ" + sc.EMOJI) * 300, 2048)
ADDED_ACROSS = "0123456789abcd<s> and more text after it"


def lane_edge_docs():
    """Documents whose rules straddle the lane ranges: 1,100 bytes (a lane's range exceeds 16 bytes)
    and 200 KB of the unit string, 3 KB without a space and 3 KB of spaces (one chunk over the 2048
    of the merge arrays, unless every space starts one), a three-byte and a four-byte character
    outside the vocabulary repeated to 2,048 bytes (characters and byte-fallback runs across every
    lane edge), a run of U+2581 and spaces, and an added token's text across the edge of lanes 0
    and 1 (the chunks around 64 and 2048 bytes at offset 0 and after a space are in the corpus)."""
    assert " " not in NO_SPACE and len(ADDED_ACROSS.encode()) <= 1024 and ADDED_ACROSS.index("<s>") == 14
    return [_cut(sc.UNIT * 40, 1100), _cut(sc.UNIT * 6000, 200 * 1024), NO_SPACE, SPACES, CJK_EMOJI,
            (SP + " ") * 300 + "x", "word " * 400, ADDED_ACROSS, "0123456789abc<s not one"]


@pytest.mark.parametrize("name", ["L-prepend", "L-plain", "M-first-split"])
def test_sp_kernels_equal_host(tok_dir, name):
    """The kernels directly on packed documents (no K16 count pointer) vs the host emulation."""
    _, prepend, split = sc.VARIANTS[name]
    m = TokenCounterModel(sc.tokenizer(tok_dir, name))
    texts = sc.corpus() + lane_edge_docs() + sc.INVALID
    data, off = sc.pack(texts)
    sp = m.bpe_spec()
    assert sp is not None and sp.kind == BPE_SP and (sp.sp_prepend, sp.sp_split) == (prepend, split)
    raw = count_spec(sp, data, off, 8)
    want_host = np.array([sc.to_host(t, prepend, split) for t in texts])
    np.testing.assert_array_equal(raw == -2, want_host)
    by_text = {t: int(raw[k]) for k, t in enumerate(texts)}
    assert by_text[NO_SPACE] == -2 and by_text[ADDED_ACROSS] == -2 and by_text["0123456789abc<s not one"] > 0
    assert by_text[SPACES] == (3073 if split else -2)
    assert by_text[CJK_EMOJI] > 2048 // 7 * 4 and by_text[_cut(sc.UNIT * 6000, 200 * 1024)] > 10000
    assert (by_text["q" * 64] > 0) and (by_text["q" * 2048] == -2) == (prepend != 0)
    tok_device.assert_kernels_equal(sp, data, off, raw)


@pytest.mark.parametrize("name", ["L-prepend", "M-first-split"])
def test_device_token_counts_equal_cpu(tok_dir, name):
    """Engine(cuda) with a trailing TokenCounter: the host tokenizer sees exactly the kept documents
    the rule names (an added token's text, a chunk over 2048 bytes), the device counts the rest, and
    statuses and outputs equal the CPU path's."""
    from test_bpe import _cfg

    _, prepend, split = sc.VARIANTS[name]
    tok = sc.tokenizer(tok_dir, name)
    texts = synth.make_corpus(6000, 1000, seed=14) + sc.fuzz(400, 15)
    texts += [t.replace(" ", " </s> ", 1) for t in texts[:60]]  # kept documents for the host tokenizer
    data, off = synth.pack(texts)
    a, oa, nh, nd = tok_device.device_and_cpu(_cfg, tok, data, off)
    kept = [t.decode("utf-8") for kind, t, _ in oa.values() if kind == "kept"]
    assert len(kept) == a.n_kept
    want = sum(sc.to_host(t, prepend, split) for t in kept)
    print(f"{name}: kept {a.n_kept}, on the host tokenizer {nh} (the rule: {want}), on the device {nd}")
    assert nh == want > 0 and nd == a.n_kept - want and nd > 0
