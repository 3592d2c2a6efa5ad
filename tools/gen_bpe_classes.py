"""Generates csrc/common/bpe_classes.inc: the character classes of the byte-level BPE
pre-tokenizer regex (GPT-2's ``'s|'t|'re|'ve|'m|'ll|'d| ?\\p{L}+| ?\\p{N}+| ?[^\\s\\p{L}\\p{N}]+|\\s+(?!\\S)|\\s+``)
for every code point, read off the ``tokenizers`` library itself (the TokenCounter oracle,
reference src/pipeline/token/token_counter.rs) rather than from ICU: its regex engine carries a
newer Unicode version than this box's ICU (9,392 code points differ), and the device token
counter must split exactly as it does.

Class per code point (2 bits): 0 other, 1 letter (\\p{L}), 2 number (\\p{N}), 3 whitespace (\\s).
Probe: ``X`` is a letter iff "a"+X pre-tokenizes to one piece, a number iff "1"+X does, other
iff "!"+X does, whitespace iff "\\t"+X does (exactly one holds for every scalar value).

Run: python tools/gen_bpe_classes.py > csrc/common/bpe_classes.inc  (about a minute on 8 CPUs)

``--check-split`` probes instead the Split pre-tokenizer of the Llama-3 / cl100k_base pattern
(csrc/common/bpe_split.h, pattern A) over every scalar value and compares the classes with the
compiled table (the two regexes run in one engine, so they must agree; this verifies it):
``X`` is a letter iff "a"+X is one piece, a number iff "1"+X is, other iff "!"+X+"!" is (a letter
or a newline after "!" would join it), whitespace iff "\\t"+X+"\\t" is (\\r and \\n end their piece:
"\\t"+X is one). Prints the number of differences; exit status 1 if there are any.

``--case`` writes csrc/common/bpe_case_classes.inc instead: the seven classes of the case-aware
patterns (csrc/common/bpe_case.h; 4 bits per code point: 0 other, 1 U = Lu / Lt, 2 l = Ll, 3 B =
Lm / Lo, 4 M = marks, 5 number, 6 whitespace), read off the library's Split with pattern C
(o200k_base). With a, A, n, w, o, x = "is one piece" of "a"+X, "A"+X, "1"+X, "\\t"+X+"\\t", "!!"+X+"!"
and X+"Aa": a number iff n, whitespace iff w, U iff A and not a (a lower-case letter does not
continue into it), l iff a and not x (no run goes on from it into an upper-case letter), B iff a
and x and not o, M iff a and x and o (a mark also joins a run of punctuation that has begun; after a
single "!" it would start a letter run with the "!" as leading code point), other iff o and not A. ``--check-case`` probes again and compares with the committed table, and with bpe_classes.inc
(letters = U, l, B; others = M, O); it prints the number of violations, exit status 1 if any.

Run: python tools/gen_bpe_classes.py --case > csrc/common/bpe_case_classes.inc
     python tools/gen_bpe_classes.py --check-case > profiles/bpe_case_nfc/class_probe_case.txt
"""
import os
import sys
from multiprocessing import Pool

N = 0x110000
BS = 128


def _probe(rng):
    from tokenizers import pre_tokenizers

    bl = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    out = bytearray(rng[1] - rng[0])
    for cp in range(*rng):
        if 0xD800 <= cp < 0xE000:
            continue  # not a scalar value: never produced by the UTF-8 decoder (U+FFFD instead)
        c = chr(cp)
        got = [k for k, pre in ((1, "a"), (2, "1"), (0, "!"), (3, "\t")) if len(bl.pre_tokenize_str(pre + c)) == 1]
        if len(got) != 1:
            raise SystemExit(f"U+{cp:04X}: ambiguous class {got}")
        out[cp - rng[0]] = got[0]
    return bytes(out)


def probe_split(cps, pattern=None):
    """Classes (bytes, one per code point of ``cps``, surrogates 0) read off the library's Split
    pre-tokenizer with ``pattern`` (default: pattern A)."""
    from tokenizers import Regex, pre_tokenizers

    if pattern is None:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from textblaster_amd.models.tokenizer import SPLIT_PATTERN_A as pattern
    sp = pre_tokenizers.Split(Regex(pattern), behavior="isolated", invert=False)
    one = lambda t: len(sp.pre_tokenize_str(t)) == 1  # noqa: E731
    out = bytearray(len(cps))
    for i, cp in enumerate(cps):
        if 0xD800 <= cp < 0xE000:
            continue
        c = chr(cp)
        if c in "\r\n":
            got = [3] if one("\t" + c) and not one("\t" + c + "\t") else []
        else:
            got = [k for k, t in ((1, "a" + c), (2, "1" + c), (0, "!" + c + "!"), (3, "\t" + c + "\t")) if one(t)]
        if len(got) != 1:
            raise SystemExit(f"U+{cp:04X}: ambiguous class {got}")
        out[i] = got[0]
    return bytes(out)


def _probe_split_range(rng):
    return probe_split(range(*rng))


def check_split():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from textblaster_amd import native

    c1, c2 = native.host().bpe_classes()
    step = N // 64
    with Pool(8) as p:
        cls = b"".join(p.map(_probe_split_range, [(i, min(i + step, N)) for i in range(0, N, step)]))
    diff = [cp for cp in range(N) if not 0xD800 <= cp < 0xE000
            and cls[cp] != (int(c2[int(c1[cp >> 7]) * 8 + ((cp & 127) >> 4)]) >> (2 * (cp & 15))) & 3]
    import tokenizers

    print(f"tokenizers {tokenizers.__version__}: Split(pattern A) classes of {N - 0x800} scalar values, "
          f"{len(diff)} differ from bpe_classes.inc" + "".join(f" U+{cp:04X}" for cp in diff[:20]))
    return 1 if diff else 0


def probe_case(cps):
    """The case-aware classes (bytes, one per code point of ``cps``, surrogates 0) read off the
    library's Split with pattern C."""
    from tokenizers import Regex, pre_tokenizers

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from textblaster_amd.models.tokenizer import SPLIT_PATTERN_C

    sp = pre_tokenizers.Split(Regex(SPLIT_PATTERN_C), behavior="isolated", invert=False)
    one = lambda t: len(sp.pre_tokenize_str(t)) == 1  # noqa: E731
    out = bytearray(len(cps))
    for i, cp in enumerate(cps):
        if 0xD800 <= cp < 0xE000:
            continue
        c = chr(cp)
        if c in "\r\n":
            got = [6] if one("\t" + c) and not one("\t" + c + "\t") else []
        else:
            a, up, n, w, o, x = (one(t) for t in ("a" + c, "A" + c, "1" + c, "\t" + c + "\t", "!!" + c + "!", c + "Aa"))
            got = [k for k, hit in ((5, n), (6, w), (1, up and not a), (2, a and not x), (3, a and x and not o),
                                    (4, a and x and o), (0, o and not up)) if hit]
        if len(got) != 1:
            raise SystemExit(f"U+{cp:04X}: ambiguous class {got}")
        out[i] = got[0]
    return bytes(out)


def _probe_case_range(rng):
    return probe_case(range(*rng))


def _probe_case_all():
    step = N // 64
    with Pool(8) as p:
        return b"".join(p.map(_probe_case_range, [(i, min(i + step, N)) for i in range(0, N, step)]))


def write_case():
    import tokenizers

    cls = _probe_case_all()
    blocks, order, stage1 = {}, [], []
    for b in range(N // BS):
        blk = cls[b * BS:(b + 1) * BS]
        if blk not in blocks:
            blocks[blk] = len(order)
            order.append(blk)
        stage1.append(blocks[blk])
    w = sys.stdout.write
    w(f"// GENERATED by tools/gen_bpe_classes.py --case from tokenizers {tokenizers.__version__}. Do not edit.\n")
    w("#pragma once\n#include <cstdint>\n")
    w(f"static const uint16_t TB_BPE_CASE_STAGE1[{len(stage1)}] = {{")
    w(",".join(("\n" if i % 32 == 0 else "") + str(v) for i, v in enumerate(stage1)) + "};\n")
    w(f"#define TB_BPE_CASE_NBLOCKS {len(order)}\n")
    # 4 bits per code point: 128 code points per 64-byte block, as 16 u32 words
    words = []
    for blk in order:
        for k in range(0, BS, 8):
            v = 0
            for j in range(8):
                v |= blk[k + j] << (4 * j)
            words.append(v)
    w(f"static const uint32_t TB_BPE_CASE_STAGE2[{len(words)}] = {{")
    w(",".join(("\n" if i % 8 == 0 else "") + f"0x{v:08x}u" for i, v in enumerate(words)) + "};\n")


def check_case():
    import tokenizers

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from textblaster_amd import native

    h = native.host()
    (c1, c2), (k1, k2) = h.bpe_classes(), h.bpe_case_classes()
    cls = _probe_case_all()
    scalar = [cp for cp in range(N) if not 0xD800 <= cp < 0xE000]
    table = {cp: (int(k2[int(k1[cp >> 7]) * 16 + ((cp & 127) >> 3)]) >> (4 * (cp & 7))) & 15 for cp in scalar}
    coarse = {cp: (int(c2[int(c1[cp >> 7]) * 8 + ((cp & 127) >> 4)]) >> (2 * (cp & 15))) & 3 for cp in scalar}
    diff = [cp for cp in scalar if cls[cp] != table[cp]]
    to_coarse = {0: 0, 1: 1, 2: 1, 3: 1, 4: 0, 5: 2, 6: 3}
    odd = [cp for cp in scalar if to_coarse[cls[cp]] != coarse[cp]]
    names = ["other", "U", "l", "B", "M", "number", "whitespace"]
    print(f"tokenizers {tokenizers.__version__}: Split(pattern C) classes of {len(scalar)} scalar values; table: stage 1 "
          f"{len(k1) * 2} bytes, stage 2 {len(k2) * 4} bytes")
    print("code points per class: " + ", ".join(f"{nm} {sum(1 for cp in scalar if cls[cp] == k)}"
                                                for k, nm in enumerate(names)))
    print(f"differ from bpe_case_classes.inc: {len(diff)}" + "".join(f" U+{cp:04X}" for cp in diff[:20]))
    print(f"differ from bpe_classes.inc (letters = U, l, B; others = M, other): {len(odd)}"
          + "".join(f" U+{cp:04X}" for cp in odd[:20]))
    print(f"violations: {len(diff) + len(odd)}")
    return 1 if diff or odd else 0


def main():
    if "--check-split" in sys.argv[1:]:
        raise SystemExit(check_split())
    if "--check-case" in sys.argv[1:]:
        raise SystemExit(check_case())
    if "--case" in sys.argv[1:]:
        return write_case()
    step = N // 64
    with Pool(8) as p:
        cls = b"".join(p.map(_probe, [(i, min(i + step, N)) for i in range(0, N, step)]))
    import tokenizers

    blocks, order, stage1 = {}, [], []
    for b in range(N // BS):
        blk = cls[b * BS:(b + 1) * BS]
        if blk not in blocks:
            blocks[blk] = len(order)
            order.append(blk)
        stage1.append(blocks[blk])
    w = sys.stdout.write
    w(f"// GENERATED by tools/gen_bpe_classes.py from tokenizers {tokenizers.__version__}. Do not edit.\n")
    w("#pragma once\n#include <cstdint>\n")
    w(f"static const uint16_t TB_BPE_CLS_STAGE1[{len(stage1)}] = {{")
    w(",".join(("\n" if i % 32 == 0 else "") + str(v) for i, v in enumerate(stage1)) + "};\n")
    w(f"#define TB_BPE_CLS_NBLOCKS {len(order)}\n")
    # 2 bits per code point: 128 code points per 32-byte block, as 8 u32 words
    words = []
    for blk in order:
        for k in range(0, BS, 16):
            v = 0
            for j in range(16):
                v |= blk[k + j] << (2 * j)
            words.append(v)
    w(f"static const uint32_t TB_BPE_CLS_STAGE2[{len(words)}] = {{")
    w(",".join(("\n" if i % 8 == 0 else "") + f"0x{v:08x}u" for i, v in enumerate(words)) + "};\n")


if __name__ == "__main__":
    main()
