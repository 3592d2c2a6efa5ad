"""Documents for the C4 byte scan and stop-word tests: the texts of tools/c4_scan_selftest.cpp (the
program writes them to a file when given a path), and whole documents built around them.

A text stays at the start of its document (what follows it is appended), so its phrases keep
their distance to the document's start: the positions that straddle a lane's 16 bytes, a wave's
1024 and a workgroup's stride stay where the self-test put them. Texts that are not valid UTF-8
(a phrase cut inside a Kelvin sign) stay with the stand-alone program: the engines take Arrow
strings."""
import functools
import os
import struct
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# GopherQuality lets nearly everything through except a document with fewer than two stop words,
# so its record carries the stop-word count and C4 sees the documents built by wrap()
_GQ = """  - type: GopherQualityFilter
    min_doc_words: 1
    max_doc_words: 100000
    min_avg_word_length: 0.01
    max_avg_word_length: 100.0
    max_symbol_word_ratio: 100.0
    max_bullet_lines_ratio: 1.0
    max_ellipsis_lines_ratio: 1.0
    max_non_alpha_words_ratio: 0.01
    min_stop_words: 2
"""
_C4 = """  - type: C4QualityFilter
    split_paragraph: true
    remove_citations: true
    filter_no_terminal_punct: true
    min_num_sentences: 1
    min_words_per_line: 3
    max_word_length: 1000
    filter_lorem_ipsum: true
    filter_javascript: true
    filter_curly_bracket: true
    filter_policy: true
"""
_FW = """  - type: FineWebQualityFilter
    line_punct_thr: 0.12
    line_punct_exclude_zero: false
    short_line_thr: 0.67
    short_line_length: 30
    char_duplicates_ratio: 0.01
    new_line_ratio: 0.3
"""
CFG_GQ_C4 = "pipeline:\n" + _GQ + _C4 + _FW
# C4 in front: every text reaches it as it is, and no stage kernel has exported its lines, so C4
# pass A takes its general path (the phrase search over the processed lines)
CFG_C4_FIRST = "pipeline:\n" + _C4 + _FW

TAIL = ".\nThe cat and the dog sat with that tree of theirs.\nIt was there because they should be with it."
# stop-word candidates at the first and at the last bytes of a document, cased
STOP_EDGES = ["the", "The", "THE", "of", "OF", "a", "A", "with", "WITH", "should", "Should", "because", "BECAUSE",
              "becauses", "thé", "étheir", "their", "k", "K", "and", "AND", "xyz"]


@functools.lru_cache(maxsize=1)
def selftest_texts():
    """Every text of the self-test, as bytes."""
    with tempfile.TemporaryDirectory() as d:
        exe, out = os.path.join(d, "c4_scan_selftest"), os.path.join(d, "texts.bin")
        subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(REPO, "tools", "c4_scan_selftest.cpp"), "-o", exe],
                       check=True, capture_output=True, timeout=300)
        r = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        with open(out, "rb") as f:
            raw = f.read()
    texts, p = [], 0
    while p < len(raw):
        (n,) = struct.unpack_from("<I", raw, p)
        texts.append(raw[p + 4:p + 4 + n])
        p += 4 + n
    return texts


def valid_texts():
    out = []
    for t in selftest_texts():
        try:
            out.append(t.decode("utf-8"))
        except UnicodeDecodeError:
            pass
    return out


def wrap(text):
    """A document that starts with ``text`` and passes GopherQuality."""
    return text + TAIL


def wrap_long(text, at_least=5120):
    """wrap(), with more lines appended until the document has ``at_least`` bytes."""
    doc, k = wrap(text), 0
    while len(doc.encode()) < at_least:
        doc += f"\nThen line {k} of the story went on with the cat and the dog and that tree."
        k += 1
    return doc


def stop_edge_documents():
    docs = []
    for first in STOP_EDGES:
        for last in STOP_EDGES[::3]:
            docs.append(f"{first} cat and that dog sat near some tree.\nIt was there for a day, as they {last}")
    return docs


def documents(small_every=1, wrapped_every=1, big=None):
    """Raw texts and wrapped ones. Texts over 2,100 bytes (the ones that straddle a workgroup's
    stride) are wrapped only and brought to 5 KB at least, ``big`` of them at most, spread evenly."""
    texts = valid_texts()
    small = [t for t in texts if len(t.encode()) <= 2100]
    large = [t for t in texts if len(t.encode()) > 2100]
    if big is not None and len(large) > big:
        large = [large[(i * len(large)) // big] for i in range(big)]
    docs = small[::small_every] + [wrap(t) for t in small[::wrapped_every]] + [wrap_long(t) for t in large]
    return docs + stop_edge_documents()
