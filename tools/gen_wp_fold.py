"""Generates csrc/common/wp_fold.inc: what BertNormalizer's ``lowercase`` and ``strip_accents`` of
the ``tokenizers`` library turn every code point >= U+0080 into (the folding WordPiece counter,
csrc/common/wordpiece.h). Like wp_classes.inc the table is read off the library itself.

Three modes: 0 ``lowercase`` alone, 1 ``strip_accents`` alone, 2 both. Per mode a stage-1 array
(one uint16 per 128 code points) selects a block of 128 uint16 entries in the shared stage 2:
  0       the code point normalises to itself (its class is wp_classes.inc's)
  0xFFFF  host: its place depends on context (NFD reorders code points with a non-zero combining
          class; one that survives the stripping, or an output that holds one - probed on the
          library next to two marks of known class, not taken from Python's tables), or its output is
          something a record cannot express (over 3 code points / 12 bytes, mixed word classes,
          several isolated code points, kept bytes that differ between the clean_text settings)
  0xFFFE  a Hangul syllable, decomposed by arithmetic into 2 or 3 jamo (kept)
  else    1 + the offset of a record in the byte pool: a header byte (bits 0-3 output bytes,
          bits 4-5 class of the output with ``clean_text: true``, bits 6-7 with ``false``; classes
          as in wp_classes.inc, an empty output is a drop) and the output as UTF-8
The class is read from the output (U+2260 is kept, its output ``=`` is isolated punctuation).

A string's normalisation is the concatenation of its code points' outputs as long as it holds no
"host" code point; ``--check`` verifies that on random strings and re-probes every scalar value
against the committed table.

Run: python tools/gen_wp_fold.py > csrc/common/wp_fold.inc
     python tools/gen_wp_fold.py --check > profiles/wordpiece_fold/fold_probe.txt
"""
import os
import random
import re
import sys
import unicodedata
from multiprocessing import Pool

N = 0x110000
BS = 128
KEEP, DROP, SPACE, ISOLATE = 0, 1, 2, 3
HOST, HANGUL = 0xFFFF, 0xFFFE
MODES = ((True, False), (False, True), (True, True))  # (lowercase, strip_accents) of mode 0, 1, 2
MAX_CPS, MAX_BYTES = 3, 12
INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "common", "wp_fold.inc")

_NORM = {}


def normalizer(clean, lower, strip):
    from tokenizers import normalizers

    key = (clean, lower, strip)
    if key not in _NORM:
        _NORM[key] = normalizers.BertNormalizer(clean_text=clean, handle_chinese_chars=True, strip_accents=strip,
                                                lowercase=lower)
    return _NORM[key]


def _class_of(s, pre):
    """Word class of a normalised output, None when it is not uniform (or several isolates)."""
    if s == "":
        return DROP
    pieces = [p for p, _ in pre.pre_tokenize_str("a" + s + "b")]
    if len(pieces) == 1:
        return KEEP
    if len(pieces) == 2 and pieces == ["a", "b"]:
        return SPACE
    if len(pieces) == 3 and pieces[0] == "a" and pieces[2] == "b" and len(pieces[1]) == 1:
        return ISOLATE
    return None


_MOVES = {}


def _moves(x):
    """Does NFD reorder the code point ``x`` (one that survived strip_accents) against a
    neighbour, i.e. has it a non-zero combining class in the library's tables? Probed with two
    spacing marks that survive the stripping: U+302F (class 224) before it, U+1B44 (class 9) after."""
    if x not in _MOVES:
        nz = normalizer(False, False, True).normalize_str
        _MOVES[x] = (nz("\u302f" + x) != nz("\u302f") + nz(x) or nz(x + "\u1b44") != nz(x) + nz("\u1b44"))
    return _MOVES[x]


def probe_range(rng):
    return probe(range(*rng))


def probe(cps):
    """Per code point a 3-tuple (mode 0, 1, 2) of None (identity), "host", or (output bytes, class
    with clean_text, class without)."""
    from tokenizers import pre_tokenizers

    pre = pre_tokenizers.BertPreTokenizer()
    out = []
    for cp in cps:
        if cp < 0x80 or 0xD800 <= cp < 0xE000:
            out.append((None, None, None))
            continue
        c = chr(cp)
        plain_t = normalizer(True, False, False).normalize_str(c)
        plain_f = normalizer(False, False, False).normalize_str(c)
        row = []
        for lower, strip in MODES:
            fold_t = normalizer(True, lower, strip).normalize_str(c)
            fold_f = normalizer(False, lower, strip).normalize_str(c)
            if strip and any(_moves(x) for x in set(fold_t + fold_f)):
                row.append("host")
                continue
            if fold_t == plain_t and fold_f == plain_f:
                row.append(None)
                continue
            kt, kf = _class_of(fold_t, pre), _class_of(fold_f, pre)
            raw = fold_f.encode("utf-8")
            if (kt is None or kf is None or len(fold_f) > MAX_CPS or len(raw) > MAX_BYTES
                    or (kt == KEEP and fold_t != fold_f) or (kf != KEEP and kt == KEEP)):
                row.append("host")
                continue
            row.append((raw, kt, kf))
        out.append(tuple(row))
    return out


def hangul(cp):
    """NFD of a Hangul syllable by arithmetic, as UTF-8."""
    s = cp - 0xAC00
    lead, vowel, tail = 0x1100 + s // 588, 0x1161 + (s % 588) // 28, 0x11A7 + s % 28
    return "".join(chr(x) for x in ((lead, vowel, tail) if s % 28 else (lead, vowel))).encode("utf-8")


def probe_all():
    step = N // 64
    with Pool(8) as p:
        parts = p.map(probe_range, [(i, min(i + step, N)) for i in range(0, N, step)])
    return [e for part in parts for e in part]


def build(rows):
    """(stage1 [3][N / 128], stage2 blocks, pool) of the probed rows."""
    pool, recs = bytearray(), {}

    def entry(cp, e):
        if e is None:
            return 0
        if e == "host":
            return HOST
        raw, kt, kf = e
        if 0xAC00 <= cp < 0xAC00 + 11172 and (kt, kf) == (KEEP, KEEP) and raw == hangul(cp):
            return HANGUL
        rec = bytes([len(raw) | kt << 4 | kf << 6]) + raw
        if rec not in recs:
            recs[rec] = len(pool)
            pool.extend(rec)
        if recs[rec] + 1 >= HANGUL:
            raise SystemExit("record pool over 16-bit offsets")
        return recs[rec] + 1

    blocks, order, stage1 = {}, [], [[], [], []]
    for m in range(3):
        for b in range(N // BS):
            blk = tuple(entry(cp, rows[cp][m]) for cp in range(b * BS, (b + 1) * BS))
            if blk not in blocks:
                blocks[blk] = len(order)
                order.append(blk)
            stage1[m].append(blocks[blk])
    return stage1, order, bytes(pool)


def write_inc(stage1, order, pool, w):
    import tokenizers

    def arr(vals):
        return ",".join(("\n" if i % 32 == 0 else "") + str(v) for i, v in enumerate(vals))

    w(f"// GENERATED by tools/gen_wp_fold.py from tokenizers {tokenizers.__version__}. Do not edit.\n")
    w("#pragma once\n#include <cstdint>\n")
    w(f"#define TB_WP_FOLD_NSTAGE1 {N // BS}\n")
    w(f"static const uint16_t TB_WP_FOLD_STAGE1[3 * TB_WP_FOLD_NSTAGE1] = {{")
    w(arr([v for m in range(3) for v in stage1[m]]) + "};\n")
    w(f"#define TB_WP_FOLD_NBLOCKS {len(order)}\n")
    w(f"static const uint16_t TB_WP_FOLD_STAGE2[{len(order) * BS}] = {{")
    w(arr([v for blk in order for v in blk]) + "};\n")
    w(f"static const uint8_t TB_WP_FOLD_POOL[{len(pool)}] = {{")
    w(arr(pool) + "};\n")


_ARR = re.compile(r"static const uint\d+_t (\w+)\[[^\]]*\] = \{([^}]*)\};")


def read_inc(path=INC):
    """(stage1 flat, stage2 flat, pool) of a generated file."""
    with open(path, encoding="utf-8") as f:
        found = {name: [int(x) for x in body.split(",")] for name, body in _ARR.findall(f.read())}
    return found["TB_WP_FOLD_STAGE1"], found["TB_WP_FOLD_STAGE2"], bytes(found["TB_WP_FOLD_POOL"])


def lookup(tables, mode, cp):
    """The table's entry for a code point, in probe()'s form."""
    stage1, stage2, pool = tables
    if cp < 0x80:
        return None
    e = int(stage2[int(stage1[mode * (N // BS) + (cp >> 7)]) * BS + (cp & 127)])
    if e == 0:
        return None
    if e == HOST:
        return "host"
    if e == HANGUL:
        return (hangul(cp), KEEP, KEEP)
    h = pool[e - 1]
    return (bytes(pool[e:e + (h & 15)]), (h >> 4) & 3, (h >> 6) & 3)


def string_pool(rows_of, rng, n_changed=4000):
    """Code points to draw random strings from: changed ones, marks, the context-dependent ones and
    ASCII. ``rows_of(cp)`` gives the probe row."""
    marks = [cp for cp in range(0x300, 0x370)] + [0x0483, 0x05B0, 0x0651, 0x093C, 0x0E31, 0x0E48, 0x3099, 0x20D0]
    ctx = [cp for cp in range(0x80, N) if not 0xD800 <= cp < 0xE000 and unicodedata.combining(chr(cp))
           and unicodedata.category(chr(cp)) != "Mn"]
    # marks of Python's tables that the library's older tables neither strip nor reorder
    ctx += [cp for cp in range(0x80, N) if not 0xD800 <= cp < 0xE000 and unicodedata.combining(chr(cp))
            and unicodedata.category(chr(cp)) == "Mn" and rows_of(cp)[1] is None]
    changed = []
    while len(changed) < n_changed:
        cp = rng.randrange(0x80, 0x30000)
        if 0xAC00 <= cp < 0xD7A4 and rng.random() < 0.9:
            continue  # most changed code points are Hangul syllables: keep them a minority
        if not 0xD800 <= cp < 0xE000 and any(e is not None for e in rows_of(cp)):
            changed.append(cp)
    return changed + marks + ctx + [0x1D15E, 0x1D160, 0xAC00, 0xAC01, 0xD7A3, 0x130, 0x212B, 0x37E, 0x2260, 0x1FEF] \
        + list(range(0x20, 0x7F)), ctx


def concat_differences(entry_of, n, seed):
    """Random strings whose library normalisation is not the concatenation of the per-code-point
    outputs ``entry_of(mode, cp)`` (strings with a "host" code point are skipped): (differing,
    compared)."""
    rng = random.Random(seed)
    memo = {}

    def rows_of(cp):
        if cp not in memo:
            memo[cp] = tuple(entry_of(m, cp) for m in range(3))
        return memo[cp]

    pool, _ = string_pool(rows_of, rng)
    differing = compared = 0
    for _ in range(n):
        s = [rng.choice(pool) for _ in range(rng.randint(1, 6))]
        text = "".join(chr(c) for c in s)
        for m, (lower, strip) in enumerate(MODES):
            es = [rows_of(c)[m] for c in s]
            if "host" in es:
                continue
            for clean in (False, True):
                ident = normalizer(clean, False, False)
                fold = normalizer(clean, lower, strip)
                parts = []
                for c, e in zip(s, es):
                    if c < 0x80:
                        parts.append(fold.normalize_str(chr(c)))  # ASCII is folded in code, not by the table
                    elif e is None:
                        parts.append(ident.normalize_str(chr(c)))
                    elif clean and e[1] in (DROP, SPACE):
                        # the record's bytes are the output without clean_text, which maps white
                        # space to U+0020 and removes controls; only the class is used for these
                        parts.append(fold.normalize_str(chr(c)))
                    else:
                        parts.append(e[0].decode("utf-8"))
                compared += 1
                differing += fold.normalize_str(text) != "".join(parts)
    return differing, compared


def check():
    import tokenizers

    tables = read_inc()
    rows = probe_all()
    w = sys.stdout.write
    w(f"tokenizers {tokenizers.__version__}; table: stage 1 {len(tables[0]) * 2} bytes, stage 2 "
      f"{len(tables[1]) * 2} bytes, record pool {len(tables[2])} bytes\n")
    bad = 0
    for m, (lower, strip) in enumerate(MODES):
        changed = empty = host = cls_diff = hang = 0
        most_cp = most_b = 0
        for cp in range(0x80, N):
            e = rows[cp][m]
            if lookup(tables, m, cp) != e:
                bad += 1
            if e is None:
                continue
            if e == "host":
                host += 1
                continue
            changed += 1
            hang += 0xAC00 <= cp < 0xAC00 + 11172
            empty += e[0] == b""
            most_cp, most_b = max(most_cp, len(e[0].decode("utf-8"))), max(most_b, len(e[0]))
        w(f"mode {m} (lowercase={lower}, strip_accents={strip}): {changed} code points >= U+0080 change "
          f"({hang} Hangul syllables), {empty} become empty, at most {most_cp} code points / {most_b} bytes, "
          f"{host} host\n")
    w(f"scalar values whose probe differs from the committed table: {bad}\n")
    differing, compared = concat_differences(lambda m, cp: lookup(tables, m, cp), 20000, 1)
    w(f"random strings compared with the concatenation of the table's outputs: {compared}, differing: {differing}\n")
    w(f"differences: {bad + differing}\n")
    return 1 if bad + differing else 0


def main():
    if "--check" in sys.argv[1:]:
        sys.exit(check())
    write_inc(*build(probe_all()), sys.stdout.write)


if __name__ == "__main__":
    main()
