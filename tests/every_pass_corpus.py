"""The corpus of the every-pass tests (test_every_pass_corpus.py on the CPU, test_gpu_every_pass.py
on the device): adversarial text for every device pass and every routing class, to be run with the
step gates off so that no kernel is spared the documents an earlier step would have filtered.

Three groups, name -> text:

* ``adv*`` / ``edge*``: adversarial_corpus() as it is (the UAX#29 fuzz pool and the constructs across
  the 64-item chunk edges of the wave primitives, all one-wave documents) and the EDGE list of
  test_gpu_kernels.py;
* ``join_*``: slices of the adversarial corpus joined with "\\n", " " and "\\n\\n" (many lines, one
  long line, many paragraphs), cut or padded to the byte on both sides of every threshold the
  runner routes on (ngram_big_bytes, long_doc_bytes, 8192, MID_DOC_BYTES, split_doc_bytes,
  pre_doc_bytes), plus the two routes that depend on the word count (blk_part, slot64) and the
  one-wave documents of more than 1024 words (rest);
* ``wg_*`` / ``tile_*``: the MOTIFS of adversarial.py placed across code point and byte index
  255/256, 511/512 and 1023/1024 (the 256- and 512-thread passes of the workgroup kernels) and
  across the 16 KB tile edges of the pre-pass, with ASCII padding (code point index == byte index)
  and 2-byte padding (the two fall apart), as boundary_docs() does for 63/64.

Two documents of EDGE hold a dictionary script; where the routing rule sends them to the CPU path
by design, expected_flags() says so and the tests pin exactly that flag. Nothing else may be flagged.

``runner`` is anything with the routing attributes (a DeviceRunner, or a DeviceTuning on a machine
without a GPU). No GPU import."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adversarial import MOTIFS, adversarial_corpus  # noqa: E402
from collision_corpus import SLOT64_WORDS, route_of  # noqa: E402

from textblaster_amd.ops.kernels import PRE_TILE  # noqa: E402
from textblaster_amd.pipeline.device import MID_DOC_BYTES  # noqa: E402

EDGE = ["", "   ", "\n\n", "a", "a\r\nb\r\n", "Hello.\n\n\nHello.\n\nHello.", "x [1] y [2, 3]. z",
        "ΣΑΣ ΣΑΣ.", "İstanbul THE the", "cooKie policy is here.", "lorem IPSUM dolor", "{ curly }",
        "日本語のテキストです。", "mixed 日本 text. Another sentence here.", "- bullet\n- bullet\n• x...",
        "a b a b a b a b a b a b a b", "ab c a bc ab c a bc"]

ROUTES = ("ng256", "ng512", "ng1024", "rest", "blk", "blk_part", "split", "slot64", "pre")
SEPS = {"nl": "\n", "sp": " ", "para": "\n\n"}
WG_EDGES = (256, 512, 1024)
ASCII_PAD = "ab cd ef gh "
TWO_BYTE_PAD = "æø "


def route(runner, text):
    """collision_corpus.route_of, which wants at least one word; documents without one are
    one-wave documents of the smallest n-gram class."""
    return route_of(runner, text) if text.split() else "ng256"


def nbytes(text):
    return len(text.encode())


DOC_NEEDS_CPU = 1  # doc_ctx.h


def expected_flags(h, texts, dict_marks, segments=True):
    """The flag every document must come back with, from the routing rule alone (h: the host
    module). A document with a dictionary script (CJK, Thai, ...) that reaches a pass which segments
    words without host ICU marks goes to the CPU path by design: the host marks none when no stage
    over the original text segments words (device.dict_marks_wanted: a pipeline of C4 steps only)
    and none for a document that is mostly dictionary script (text.cpp dict_word_marks: the
    language gate is expected to filter it; with the gates off it is analysed). Language ID flags
    nothing (``segments`` false). Everything else is 0: two documents of EDGE are not."""
    out = []
    for t in texts:
        cpu = segments and h.has_dict_script(t)
        if cpu and dict_marks:
            cpu = 2 * sum(1 for c in t if h.has_dict_script(c)) > len(t)
        out.append(DOC_NEEDS_CPU if cpu else 0)
    return out


def fit(text, n, pad=ASCII_PAD):
    """``text`` cut at a code point (or padded with short words) to exactly ``n`` UTF-8 bytes."""
    cut = text.encode()[:n].decode("utf-8", errors="ignore")
    k = 0
    while nbytes(cut) < n:
        cut += pad[k % len(pad)] if nbytes(cut) + nbytes(pad[k % len(pad)]) <= n else "x"
        k += 1
    assert nbytes(cut) == n
    return cut


def joined(adv, sep, n, start):
    """Adversarial documents from ``start`` on (cyclically), joined with ``sep``, exactly ``n`` bytes."""
    parts, size, k = [], 0, start
    while size < n:
        parts.append(adv[k % len(adv)])
        size += nbytes(parts[-1]) + len(sep)
        k += 1
    return fit(sep.join(parts), n)


class _Builder:
    """Text under construction with its code point and byte counts."""

    def __init__(self, unit):
        self.parts, self.cp, self.by, self.unit, self.k = [], 0, 0, unit, 0

    def add(self, s):
        self.parts.append(s)
        self.cp += len(s)
        self.by += nbytes(s)

    def pad_to(self, target, by_bytes):
        """Padding up to exactly ``target`` code points (or bytes)."""
        while True:
            ch = self.unit[self.k % len(self.unit)]
            if (self.by + nbytes(ch) if by_bytes else self.cp + 1) > target:
                break
            self.add(ch)
            self.k += 1
        while (self.by if by_bytes else self.cp) < target:
            self.add("x")

    def text(self):
        return "".join(self.parts)


def straddling(motifs, unit, edges, size):
    """``motifs[k]`` across ``edges[k]`` = (index, by_bytes): its first code point (or byte) is the
    last item before the index or, for every other edge, only its last one lies past it. Padded
    with ``unit`` to at least ``size`` bytes."""
    b = _Builder(unit)
    per_cp = nbytes(unit) / len(unit)  # (the order of the edges in the text)
    for k, (motif, (edge, by_bytes)) in enumerate(zip(motifs, sorted(edges, key=lambda e: e[0] * (1 if e[1] else per_cp)))):
        n = nbytes(motif) if by_bytes else len(motif)
        lead = 1 if k % 2 == 0 or n < 2 else n - 1
        assert (b.by if by_bytes else b.cp) <= edge - lead, (motif, edge)
        b.pad_to(edge - lead, by_bytes)
        b.add(motif)
        assert (b.by if by_bytes else b.cp) > edge or n < 2
        b.add(" ")
    b.pad_to(max(size, b.by), True)
    b.add(" tail words here. End.")
    return b.text()


def straddles(text, motifs, edge, by_bytes):
    """Does an occurrence of one of ``motifs`` begin before code point (or byte) index ``edge`` and
    end after it? (A motif of one item cannot.)"""
    hay = text.encode() if by_bytes else text
    for m in motifs:
        needle = m.encode() if by_bytes else m
        if len(needle) >= 2 and hay.find(needle, edge - len(needle) + 1, edge + len(needle) - 1) >= 0:
            return True
    return False


def workgroup_boundary_docs(runner):
    """Per motif: all three workgroup edges by byte index with ASCII padding (the code point index
    too, until a motif that is not ASCII), and by code point index and by byte index in one
    document with 2-byte padding."""
    size = runner.long_doc_bytes + 64
    docs = {}
    for m, motif in enumerate(MOTIFS):
        docs[f"wg_ascii_{m:02d}"] = straddling([motif] * 3, ASCII_PAD, [(e, True) for e in WG_EDGES], size)
        both = [(e, True) for e in WG_EDGES] + [(e, False) for e in WG_EDGES]
        docs[f"wg_2byte_{m:02d}"] = straddling([motif] * 6, TWO_BYTE_PAD, both, size)
    return docs


def tile_boundary_docs(runner):
    """Pre-pass documents (>= pre_doc_bytes) with a motif across every 16 KB tile edge: byte index
    with ASCII padding; byte index and code point index with 2-byte padding."""
    size = runner.pre_doc_bytes
    docs = {}
    # (ASCII: one tile more, so that four documents hold every motif)
    byte_edges = [(e, True) for e in range(PRE_TILE, size + PRE_TILE + 1, PRE_TILE)]
    # (2-byte padding: 3 code points in 5 bytes)
    cp_edges = [(e, False) for e in range(PRE_TILE, size * 3 // 5, PRE_TILE)]
    for unit, tag, edges in ((ASCII_PAD, "ascii", byte_edges), (TWO_BYTE_PAD, "2byte", byte_edges[:-1] + cp_edges)):
        for d, k in enumerate(range(0, len(MOTIFS), len(edges))):
            ms = (MOTIFS[k:] + MOTIFS)[:len(edges)]
            docs[f"tile_{tag}_{d}"] = straddling(ms, unit, edges, max(size, edges[-1][0] + 64))
    return docs


def routing_docs(runner, adv):
    """Joins of the adversarial corpus on both sides of every routing threshold."""
    assert runner.pre_doc_bytes > runner.split_doc_bytes >= MID_DOC_BYTES > 8192 > runner.long_doc_bytes \
        > runner.ngram_big_bytes > 0
    docs = {}
    # (documents of more than T bytes take the longer route; of at least pre_doc_bytes the pre-pass)
    sizes = sorted({t + d for t in (runner.ngram_big_bytes, runner.long_doc_bytes, 8192, MID_DOC_BYTES,
                                    runner.split_doc_bytes) for d in (0, 1)}
                   | {runner.pre_doc_bytes - 1, runner.pre_doc_bytes})
    start = 0
    for tag, sep in SEPS.items():
        for n in sizes:
            if n >= runner.pre_doc_bytes - 1 and tag == "para":
                continue  # (the paragraph join of this class is the longest document below)
            docs[f"join_{tag}_{n}"] = joined(adv, sep, n, start)
            start += 97
    docs["join_para_longest"] = joined(adv, SEPS["para"], runner.pre_doc_bytes + 4500, start)
    # one-wave documents of more than 1024 words; workgroup documents whose word table exceeds
    # the LDS slice; documents with 64-bit table slots (at least SLOT64_WORDS words)
    part_words = runner.lds_bytes_blk // 6 + 16
    for k, sep in enumerate((" ", "\n")):
        short = [w for d in adv[k::2] for w in d.split() if nbytes(w) <= 4]
        docs[f"join_rest_{k}"] = fit(sep.join(w for w in short if nbytes(w) <= 2), runner.long_doc_bytes - k)
        # (more than 512 and at most 1024 words: the 1024-word n-gram class)
        docs[f"join_ng1024_{k}"] = fit(sep.join(short), 3000 + k)
        body = joined(adv, sep, 4000, 400 + 31 * k)
        docs[f"join_blk_part_{k}"] = body + sep + sep.join(["a", "bc"][i % 2] for i in range(part_words))
        docs[f"join_slot64_{k}"] = body + sep + sep.join("ab"[i % 2] for i in range(SLOT64_WORDS))
    return docs


def every_pass_corpus(runner):
    adv = adversarial_corpus()
    docs = {f"adv{i:03d}": t for i, t in enumerate(adv)}
    docs.update({f"edge{i:02d}": t for i, t in enumerate(EDGE)})
    docs.update(routing_docs(runner, adv))
    docs.update(workgroup_boundary_docs(runner))
    docs.update(tile_boundary_docs(runner))
    return docs
