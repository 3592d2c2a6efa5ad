"""C4 pass A's byte scan (c4_pass_a.h c4_byte_scan, c4_phrases_at: phrases matched from packed bytes)
and the stop-word fast path (is_stop_word) inside whole runs: the texts of
tools/c4_scan_selftest.cpp and documents built around them (tests/c4_scan_corpus.py) through the
host emulation of the device algorithms and through the CPU ICU oracle. Status, first failing step,
reason and rewritten text must be equal, with GopherQuality in front of C4 (the line-export path)
and with C4 in front (its general path)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import c4_scan_corpus as corpus  # noqa: E402
from test_emulated_device_path import outputs  # noqa: E402

from textblaster_amd.config import load_pipeline_config_str  # noqa: E402
from textblaster_amd.pipeline.engine import Engine  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402


@pytest.fixture(scope="module")
def docs():
    return corpus.documents(big=60)


@pytest.mark.parametrize("name", ["gq_c4", "c4_first"])
def test_emulation_equals_cpu_oracle(docs, name):
    text = {"gq_c4": corpus.CFG_GQ_C4, "c4_first": corpus.CFG_C4_FIRST}[name]
    cfg = load_pipeline_config_str(text, name + ".yaml")
    data, off = synth.pack(docs)
    a = Engine(cfg, backend="emulate", keep_reasons=True).process(data, off)
    b = Engine(cfg, backend="cpu", segmentation="icu", keep_reasons=True).process(data, off)
    np.testing.assert_array_equal(a.status, b.status)
    np.testing.assert_array_equal(a.fail_step, b.fail_step)
    assert a.reasons == b.reasons
    oa, ob = outputs(a), outputs(b)
    bad = [k for k in oa if oa[k] != ob[k]]
    assert not bad, [(k, docs[k][:120]) for k in bad[:3]]
    # the documents exercise the scan: C4 rejects some for lorem ipsum and for curly brackets,
    # rewrites others without their javascript / policy lines, and GopherQuality's stop-word
    # count decides too
    reasons = " ".join(r for r in b.reasons.values()) if isinstance(b.reasons, dict) else " ".join(map(str, b.reasons))
    assert "lorem" in reasons.lower() and "curly" in reasons.lower()
    changed = sum(1 for k, (kind, t, _) in ob.items() if kind == "kept" and t != docs[k].encode())
    assert changed > 100
    if name == "gq_c4":
        assert "stop" in reasons.lower()
