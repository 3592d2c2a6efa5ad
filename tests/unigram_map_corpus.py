"""What the tests of the mapped Unigram counter share (tests/test_unigram_map.py on the host
emulation, tests/test_gpu_unigram_map.py on k_uni_count_map): the per-document rule with the
normalizer's replacements applied by the counter, written against the `tokenizers` library and not
read from the spec's table, and the smallest documents at which the replacements can go wrong."""
import base64
import json
import unicodedata

import unigram_corpus as uc

MAX_MAP_BYTES = 32  # the cap of a replacement (models/tokenizer.py UNI_MAX_MAP_BYTES)


def to_host(path, variant):
    """text -> bool. A document goes to the host when it holds an added token's or the unk piece's
    text, a grapheme joiner, a kept U+2581, kept white space in layout C, or a code point whose
    replacement is over the cap, holds U+2581 or (layout C) white space other than U+0020. The unk
    piece's text counts in the normalised text too: replacements can spell it where the raw text has
    none, the library then gives the characters to the model, and the counter does not follow it
    there (csrc/common/unigram.h). And a joiner that on its own becomes a space is one more case of
    "a joiner" where it directly follows a replaced or dropped code point: the normalizer looks a
    grapheme under 6 bytes up as a whole and the replaced code point swallows it (U+200C behind
    nmt_nfkc)."""
    from tokenizers import normalizers

    with open(path, encoding="utf-8") as f:
        tj = json.load(f)
    seq = tj["normalizer"]["normalizers"]
    unk = tj["model"]["vocab"][tj["model"]["unk_id"]][0]
    pre = None
    if seq[0]["type"] == "Precompiled":
        pre = normalizers.Precompiled(base64.b64decode(seq[0]["precompiled_charsmap"]))
    layout_c = uc.VARIANTS[variant]["layout"] == "C"
    memo = {}

    def joiner(c):
        return uc.JOINER.match(c) is not None or unicodedata.category(c) in ("Mn", "Me", "Mc", "Cn")

    def host_char(c):
        if c not in memo:
            out = pre.normalize_str(c) if pre else c
            if c == " " or out == " ":
                memo[c] = False
            elif out == c:
                if c == "\u2581":
                    memo[c] = True
                elif ord(c) in uc.WHITE:
                    memo[c] = layout_c
                else:
                    memo[c] = pre is not None and joiner(c)
            else:
                memo[c] = (joiner(c) or len(out.encode("utf-8")) > MAX_MAP_BYTES or "\u2581" in out
                           or (layout_c and any(ord(x) in uc.WHITE and x != " " for x in out)))
        return memo[c]

    def replaced(c):
        return pre is not None and c != " " and pre.normalize_str(c) not in (" ", c)

    def joining_space(c):
        return pre is not None and c != " " and pre.normalize_str(c) == " " and joiner(c)

    def rule(t):
        if any(a in t for a in uc.ADDED) or any(host_char(c) for c in set(t)):
            return True
        if any(joining_space(b) and replaced(a) for a, b in zip(t, t[1:])):
            return True
        return pre is not None and unk in pre.normalize_str(t)

    return rule


def full_width(word):
    """``word`` in full-width forms (U+FF01..FF5E), which nmt_nfkc folds back; None when a
    character has none."""
    if not all(0x21 <= ord(c) <= 0x7E for c in word):
        return None
    return "".join(chr(ord(c) + 0xFEE0) for c in word)


def constructed(word):
    """``word``: unigram_corpus.longest_word of the tokenizer under test."""
    docs = [full_width("the"), "x " + full_width("the") + " y"]
    if full_width(word) is not None:
        docs += [full_width(word), "x" + full_width(word) + "s"]
    docs += ["a\u00a8b", "\u00a8", "a\u00a8", "ab \u00a8",  # a word starts inside an output
             "a\x01b", "a" + "\x01" * 40 + "b", "\x01\x01\x01", "a \x01\x01 b", "\x01a", "a\x01",
             "\u2026a", "a\u2026", "a\u2026\u2026b", "\u2026", "wait\u2026 what",
             "\u00bd", "a\u00bdb", "\u2122", "the\u2122 the",
             "\ufdfa", "a \ufdfa",
             "a\uff1c\uff55\uff4e\uff4b\uff1eb", "\uff1cunk>", "a\uff1c\uff0f\uff53\uff1eb", "\uff1c/s>",
             "\ufb01ne", "\uff21\uff22 \u0958",
             # U+200C: a space of its own, swallowed by a replaced code point of one or two bytes in front of it
             "a\u200cb", "a\u00a8\u200cb", "\u00bd\u200c\u200cb", "\u2026\u200cb", "a\x01\u200cb", "\u200c\u00a8", "\u00a8 \u200cb"]
    return docs


def lane_edge_docs(word):
    """The documents at which a lane edge (16 bytes up to 1 KB, then 1/64 of the document) meets a
    replacement."""
    docs = ["a" * lead + "\u2026b" for lead in range(13, 18)]  # a 3-byte map code point straddles the edge
    docs += ["a" * lead + "\u00a8b" for lead in range(14, 18)]  # a word starts inside an output at the edge
    docs += ["a" * 15 + "\x01" * k + "b" for k in (1, 17, 40)]  # the look-back goes through lanes of drops
    fw = full_width(word)
    if fw is not None:
        docs += [("a" * (lead - 1) + " ")[:lead] + fw + " b" for lead in range(17)]  # lead bytes in front
    docs.append("\u2026" * 700)  # over 2 KB: every lane begins inside or beside a map code point
    return docs
