"""k_uni_count_map on the GPU (csrc/hip/unigram.hip): array for array against its host emulation
(which tests/test_unigram_map.py pins to the `tokenizers` library), and the device pipeline under
TB_TUNE=uni_map=1 against the CPU path."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tok_device  # noqa: E402
import unigram_corpus as uc  # noqa: E402
import unigram_map_corpus as um  # noqa: E402

from textblaster_amd.models.tokenizer import TokenCounterModel, count_spec  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tok_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("unimap")


@pytest.mark.parametrize("variant", list(uc.VARIANTS))
def test_uni_map_kernel_equals_host(tok_dir, variant):
    """k_uni_count_map directly on packed documents (no K16 count pointer) vs the host emulation:
    the CPU corpus, the lane-edge documents (a lane's range is 16 bytes up to 1 KB, then 1/64 of
    the document) and one 200 KB document of synthetic text with its U+2026 left in."""
    path = uc.tokenizer(variant, tok_dir)
    m = TokenCounterModel(path)
    sp = m.unigram_map_spec()
    assert sp.mapped
    word, _ = uc.longest_word(path)
    rule = um.to_host(path, variant)
    big = "\n".join([t for t in synth.make_corpus(1200, 1024, seed=33, vocab="zipf") if not rule(t)][:310])
    assert len(big.encode("utf-8")) > 200 * 1024
    edge = um.lane_edge_docs(word) + [big]
    texts = [t.encode("utf-8") for t in uc.corpus(word) + um.constructed(word) + edge] + uc.INVALID
    data = np.frombuffer(b"".join(texts), dtype=np.uint8).copy()
    off = np.cumsum([0] + [len(t) for t in texts]).astype(np.int64)
    raw = count_spec(sp, data, off, 8)
    assert (raw >= 0).sum() > 300 and (raw == -2).sum() > 100
    edge_raw = raw[len(texts) - len(uc.INVALID) - len(edge):len(texts) - len(uc.INVALID)]
    assert (edge_raw >= 0).all()  # every edge document is counted, the big one among them
    if uc.VARIANTS[variant]["rule"] != "identity":
        assert "\u2026" in big and int(count_spec(m.unigram_spec(), *uc.pack([big]))[0]) == -2
    assert raw[len(texts) - len(uc.INVALID):].tolist() == [-2 if h else int(raw[-2]) for h in uc.INVALID_HOST]
    tok_device.assert_kernels_equal(sp, data, off, raw)


def _cfg():
    from test_unigram import _cfg as cfg

    return cfg()


@pytest.mark.parametrize("variant", ["H-nmt", "C-nmt-first"])
def test_device_token_counts_equal_cpu(tok_dir, variant, monkeypatch):
    """TB_TUNE=uni_map=1 on the input of tests/test_gpu_unigram.py's engine test: statuses and
    outputs equal the CPU path's; the host tokenizer counts exactly the documents of the new rule
    (above 0: the spliced </s>), the kernel all others, and no kept document whose only code point
    of the old rule is U+2026 is on the host tokenizer."""
    monkeypatch.setenv("TB_TUNE", "uni_map=1")
    tok = uc.tokenizer(variant, tok_dir)
    base = synth.make_corpus(6000, 1000, seed=14)
    spliced = [t[:len(t) // 2] + " </s> " + t[len(t) // 2:] for t in base[:60]]
    texts = base + uc.fuzz(400, 15) + spliced
    data, off = synth.pack(texts)
    delegated = uc.watch_delegated(monkeypatch)
    a, oa, nh, nd = tok_device.device_and_cpu(_cfg, tok, data, off)
    rule, old_rule = um.to_host(tok, variant), uc.to_host(tok, variant)
    kept, want = uc.rule_count(rule, texts, oa, delegated)
    _, want_old = uc.rule_count(old_rule, texts, oa, delegated)
    print(f"{variant}: kept {a.n_kept}, {kept} of them on the device path: host tokenizer {nh} "
          f"(the rule: {want}; without the map: {want_old}), device {nd}")
    assert a.n_kept - kept <= len(delegated) < 400
    assert nh == want > 0 and nd == kept - want > 0 and want < want_old
    # the kept documents with U+2026 that nothing else of the rule holds: counted by the kernel
    # (nh == want, and the rule sends none of them to the host)
    ell = []
    for i, (k, t, _) in oa.items():
        t = t.decode("utf-8") if isinstance(t, bytes) else t
        if k == "kept" and texts[i].encode("utf-8") not in delegated and "\u2026" in t and not rule(t.replace("\u2026", "")):
            ell.append(t)
    assert ell and all(old_rule(t) and not rule(t) for t in ell)
