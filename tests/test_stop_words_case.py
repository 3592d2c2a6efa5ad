"""GopherQualityFilter stop words with mixed-case and non-ASCII config entries (reference
gopher_quality.rs: ``stop_words.contains(&w.to_lowercase())`` against the raw entries). The device
code has two lookups — an ASCII fast table for words of <= 7 bytes and the hashed lowercase-bytes
table (csrc/common/stage_analyze.h is_stop_word) — and both must follow that rule: a capitalised entry
("The") never matches, since no lowercased word is capitalised; "I" matches the entry "i";
"Über" / "NAÏVE" match "über" / "naïve" through the slow path. The emulated device path must equal
the CPU ICU oracle, and the counts are pinned."""
import re

import pytest

from textblaster_amd.config import load_pipeline_config
from textblaster_amd.pipeline.engine import Engine
from textblaster_amd.utils import synth

CFG = """pipeline:
  - type: GopherQualityFilter
    min_doc_words: 1
    max_doc_words: 100000
    min_stop_words: 100
    stop_words: ["The", "i", "naïve", "über", "OF", "straße"]
"""

# (text, stop words found under the reference rule)
CASES = [
    ("THE the The tHe", 0),                 # "the" is not an entry; "The" can never match
    ("I i", 2),                             # both lowercase to "i"
    ("Über über ÜBER", 3),                  # non-ASCII: the hashed slow path
    ("NAÏVE naïve Naïve", 3),
    ("of OF Of", 0),                        # entry "OF" is upper case: never matches
    ("STRASSE straße STRAßE", 2),           # "STRASSE" lowercases to "strasse", not "straße"
    ("I think the naïve über-plan is OK", 3),  # "I", "naïve", "über" (UAX#29 splits at '-')
    ("nothing here at all", 0),
]


@pytest.fixture(scope="module")
def cfg(tmp_path_factory):
    p = tmp_path_factory.mktemp("cfg") / "stop.yaml"
    p.write_text(CFG, encoding="utf-8")
    return load_pipeline_config(str(p))


def test_stop_word_counts_follow_reference_rule(cfg):
    texts = [t for t, _ in CASES]
    data, off = synth.pack(texts)
    cpu = Engine(cfg, backend="cpu", segmentation="icu", nthreads=1, keep_reasons=True).process(data, off)
    found = []
    for i in range(len(texts)):
        r = cpu.reasons.get(i)
        m = re.search(r"gopher_too_few_stop_words \(found (\d+), required 100\)", r or "")
        assert m, r
        found.append(int(m.group(1)))
    assert found == [n for _, n in CASES]


def test_stop_word_fast_and_slow_paths_equal_cpu(cfg):
    texts = [t for t, _ in CASES] + synth.make_corpus(200, 400, seed=3)
    data, off = synth.pack(texts)
    a = Engine(cfg, backend="emulate", nthreads=2, keep_reasons=True).process(data, off)
    b = Engine(cfg, backend="cpu", segmentation="icu", nthreads=2, keep_reasons=True).process(data, off)
    assert a.reasons == b.reasons
