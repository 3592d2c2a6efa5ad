"""k_uni_count on the GPU (csrc/hip/unigram.hip): array for array against its host emulation (which
tests/test_unigram.py pins to the `tokenizers` library), and the device pipeline with a trailing
Unigram TokenCounter against the CPU path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tok_device  # noqa: E402
import unigram_corpus as uc  # noqa: E402

from textblaster_amd.models.tokenizer import TokenCounterModel, count_spec  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("uni")


def lane_edge_docs(word, rule):
    """The smallest documents at which the lane split can go wrong (a lane's range is 16 bytes up to
    1 KB, then 1/64 of the document); ``word``: U+2581 + word is a longest piece, ``rule``: to_host."""
    unit = "ab cd\u00e9f gh \u4f60m "
    docs = ["the"]
    docs.append((unit * 80).encode("utf-8")[:1100].decode("utf-8", "ignore"))  # ranges over 16 bytes
    docs.append("x" * 3072)  # one lane follows the word across every other lane's range
    for lead in range(17):  # the longest piece across the edge of lanes 0 and 1
        docs.append("a" * lead + " " + word + " b")
    docs.append("\u4f60" * 683)  # a three-byte and a four-byte character the vocabulary lacks, to
    docs.append("\U0001F600" * 512)  # 2,048 bytes: unknown runs and byte fallback cross every lane edge
    docs.append(" \u00a0\n" * 300 + "x")
    for lead in range(12, 17):  # an added token's text across a lane edge
        docs.append("a" * lead + "</s> b")
    # one 200 KB document of text the counter counts itself
    big = "\n".join([t for t in synth.make_corpus(1200, 1024, seed=33, vocab="zipf") if not rule(t)][:310])
    assert len(big.encode("utf-8")) > 200 * 1024
    docs.append(big)
    return docs


@pytest.mark.parametrize("variant", list(uc.VARIANTS))
def test_uni_kernel_equals_host(tok_dir, variant):
    """k_uni_count directly on packed documents (no K16 count pointer) vs the host emulation."""
    path = uc.tokenizer(variant, tok_dir)
    m = TokenCounterModel(path)
    sp = m.unigram_spec()
    word, _ = uc.longest_word(path)
    edge = lane_edge_docs(word, uc.to_host(path, variant))
    texts = [t.encode("utf-8") for t in uc.corpus(word) + edge] + uc.INVALID
    data = np.frombuffer(b"".join(texts), dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(t) for t in texts]).astype(np.int64)
    raw = count_spec(sp, data, off, 8)
    assert (raw >= 0).sum() > 300 and (raw == -2).sum() > 100
    host_edge = [t for t, r in zip(edge, raw[len(texts) - len(uc.INVALID) - len(edge):]) if r < 0]
    assert all("</s>" in t for t in host_edge) and len(host_edge) == 5  # every other edge document is counted
    assert raw[len(texts) - len(uc.INVALID):].tolist() == [-2 if h else int(raw[-2]) for h in uc.INVALID_HOST]
    tok_device.assert_kernels_equal(sp, data, off, raw)


def _cfg():
    from test_unigram import _cfg as cfg

    return cfg()


@pytest.mark.parametrize("variant", ["H-nmt", "C-nmt-first"])
def test_device_token_counts_equal_cpu(tok_dir, variant, monkeypatch):
    """Statuses and outputs (the token counts in the metadata column among them) equal the CPU
    path's; of the kept documents that went through the device path the host tokenizer counted
    exactly those of the rule, the kernel all others. (A document the engine hands to its CPU path
    as a whole is counted there and by neither.)"""
    tok = uc.tokenizer(variant, tok_dir)
    base = synth.make_corpus(6000, 1000, seed=14)
    spliced = [t[:len(t) // 2] + " </s> " + t[len(t) // 2:] for t in base[:60]]
    texts = base + uc.fuzz(400, 15) + spliced
    data, off = synth.pack(texts)
    delegated = uc.watch_delegated(monkeypatch)
    a, oa, nh, nd = tok_device.device_and_cpu(_cfg, tok, data, off)
    kept, want = uc.rule_count(uc.to_host(tok, variant), texts, oa, delegated)
    print(f"{variant}: kept {a.n_kept}, {kept} of them on the device path: host tokenizer {nh} "
          f"(the rule: {want}), device {nd}")
    assert a.n_kept - kept <= len(delegated) < 400
    assert nh == want > 0 and nd == kept - want > 0
