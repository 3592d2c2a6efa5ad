"""Synthetic record matrices for the device metadata formatter (csrc/common/metafmt.h): every
branch of decide_t (csrc/host/filters.cpp) per step kind, the rounding ties of {:.2} / {:.4}, and
the language confidences, shared by tests/test_device_meta.py (host emulation) and
tests/test_gpu_device_meta.py (kernels). The step parameters are those of
config/pipeline_config.yaml."""
import struct

import numpy as np

from textblaster_amd import native
from textblaster_amd.config import load_pipeline_config

T40 = 1 << 40


def _bits(x: float) -> int:
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _conf_values():
    out = []
    for v in (1.0, 0.5, 0.25, 0.2, 1.0 / 3.0, 0.9999999999999999):
        out += [v, float(np.nextafter(v, 0.0)), float(np.nextafter(v, 2.0))]
    return out


# passing record of each kind (default thresholds)
PASS = {
    "LanguageDetectionFilter": [1, _bits(1.0)],
    "GopherRepetitionFilter": [1000, 5, 0, 0, 10, 0, 0] + [0] * 9,
    "GopherQualityFilter": [100, 500, 0, 0, 10, 0, 0, 100, 10],
    "C4QualityFilter": [0, 0, 0, 0, 0, 10, 100],
    "FineWebQualityFilter": [10, 5, 2, 0, 1000, 9, 200],
}


def _gq():
    p = PASS["GopherQualityFilter"]

    def r(**kw):
        names = ["n", "sum", "hash", "ell", "lines", "bullet", "ell_lines", "alpha", "stop"]
        v = list(p)
        for k, x in kw.items():
            v[names.index(k)] = x
        return v

    rows = [p, r(n=10, sum=50, alpha=10), r(n=200000, sum=1000000, alpha=200000), r(sum=241), r(sum=1500),
            r(hash=20), r(ell=20), r(hash=11, ell=12), r(bullet=10), r(ell_lines=5), r(alpha=50), r(stop=1),
            # eight reasons at once, then the two a long document adds
            [10, 20, 5, 5, 10, 10, 5, 2, 0], [200000, 2200000, 0, 0, 10, 0, 0, 200000, 10],
            # no words at all: the " - 0 non-symbol words" suffix
            [0, 0, 0, 0, 1, 0, 0, 0, 0], [0, 0, 3, 2, 0, 0, 0, 0, 0],
            # exact binary ties of {:.2}: 1/8, 3/8, 5/8, 7/8 (average length), 25/8 (hash ratio)
            r(n=8, sum=1, alpha=8), r(n=8, sum=3, alpha=8), r(n=8, sum=5, alpha=8), r(n=8, sum=7, alpha=8),
            r(n=8, sum=40, hash=25, alpha=8), r(n=8, sum=40, ell=25, alpha=8),
            # near ties
            r(n=200, sum=1, alpha=200), r(n=200, sum=3, alpha=200), r(n=3, sum=1, alpha=3), r(n=3, sum=2, alpha=1),
            # large quotients and counts
            r(n=1, sum=2000000, alpha=1), r(n=7, sum=7 * 12345678 + 3, alpha=7), r(n=60, sum=700, alpha=60),
            r(n=T40 + 3, sum=5 * T40, alpha=T40), r(n=100, sum=T40 + 1), r(n=100, sum=500, hash=T40 - 1, ell=T40 + 7),
            r(lines=3, bullet=T40), r(stop=0), r(n=49, sum=49 * 3, alpha=49, stop=2), r(n=50, sum=150, alpha=40)]
    return rows


def _gr():
    p = PASS["GopherRepetitionFilter"]

    def r(chars=1000, para=5, pd=0, pb=0, lines=10, ld=0, lb=0, top=(0, 0, 0), dup=(0,) * 6):
        return [chars, para, pd, pb, lines, ld, lb, *top, *dup]

    rows = [p, r(chars=-1), [-5] + [7] * 15, r(pd=2), r(pb=300), r(ld=4), r(lb=300), r(top=(250, 0, 0)),
            r(top=(0, 190, 0)), r(top=(0, 0, 170)), r(dup=(160, 0, 0, 0, 0, 0)), r(dup=(0, 150, 0, 0, 0, 0)),
            r(dup=(0, 0, 140, 0, 0, 0)), r(dup=(0, 0, 0, 130, 0, 0)), r(dup=(0, 0, 0, 0, 120, 0)),
            r(dup=(0, 0, 0, 0, 0, 101)),
            # every fraction and every top and duplicated order at once
            r(pd=5, pb=900, ld=9, lb=800, top=(500, 400, 300), dup=(900, 800, 700, 600, 500, 400)),
            # ties over 8 characters: 1/8 (only past the 0.10 / 0.11 / 0.12 orders), 3/8, 5/8, 7/8, 25/8
            r(chars=8, dup=(0, 0, 0, 1, 1, 1)), r(chars=8, top=(3, 3, 3)), r(chars=8, top=(5, 0, 5)),
            r(chars=8, top=(7, 7, 0), dup=(7, 0, 0, 0, 0, 0)), r(chars=8, top=(25, 0, 0), pb=25, lb=25),
            # near ties
            r(chars=200, dup=(0, 0, 0, 0, 0, 21)), r(chars=3, top=(1, 1, 1)), r(chars=200, top=(43, 0, 0)),
            # large quotients, counts near 2^40, empty documents' guards (zero paragraphs / lines)
            r(chars=1, top=(2000000, 0, 0)), r(chars=T40, top=(T40 - 1, 0, 0), pb=T40 // 2),
            r(chars=0, para=0, lines=0, pd=1, ld=1), r(chars=3, top=(T40, 0, 0)), r(pd=1, ld=3), r(pb=200, lb=200)]
    return rows


def _c4():
    p = PASS["C4QualityFilter"]
    rows = [p, [0, 0, 3, 2, 1, 10, 100], [1, 0, 0, 0, 0, 0, 10], [0, 1, 0, 0, 0, 0, 10], [1, 1, 5, 5, 5, 0, 10],
            [0, 0, 0, 0, 0, 5, 10], [0, 0, 0, 0, 0, 4, 10]]
    for a in (0, 3):
        for b in (0, 17):
            for c in (0, T40 + 1):
                rows.append([0, 0, a, b, c, 2, 50])
    rows.append([0, 0, T40, T40 - 1, 1, 0, 0])
    return rows


def _fw():
    p = PASS["FineWebQualityFilter"]

    def r(lines=10, stop=5, short=2, dup=0, chars=1000, nl=9, words=200):
        return [lines, stop, short, dup, chars, nl, words]

    rows = [p, r(lines=0), r(lines=0, nl=4, words=0), r(stop=1), r(stop=0), r(short=9), r(short=7), r(dup=11),
            r(dup=10), r(chars=0, dup=5), r(chars=0), r(nl=3, words=0), r(nl=0, words=0), r(nl=100), r(nl=60),
            # exact binary ties of {:.4}: 1/32, 3/32 (line punctuation), 5/32 (duplicated characters)
            r(lines=32, stop=1), r(lines=32, stop=3), r(dup=5, chars=32), r(lines=32, stop=5, short=23),
            # near ties
            r(lines=200, stop=1), r(lines=200, stop=3), r(nl=1, words=3), r(lines=3, stop=1, short=3),
            # quotients >= 10 and >= 10^6, counts near 2^40
            r(nl=10000000, words=1), r(nl=25, words=2), r(dup=T40, chars=7), r(lines=T40 + 1, stop=T40 // 9),
            r(lines=T40, stop=T40, short=T40 - 1)]
    return rows


def _ld():
    rows = [[-1, 0], [-1, _bits(0.9)]]
    for lang in range(5):
        rows.append([lang, _bits(1.0)])
    for v in _conf_values():
        rows += [[1, _bits(v)], [0, _bits(v)]]
    return rows


MATRIX = {"LanguageDetectionFilter": _ld, "GopherRepetitionFilter": _gr, "GopherQualityFilter": _gq,
          "C4QualityFilter": _c4, "FineWebQualityFilter": _fw}
TOKENS = [0, 1, 5, 1023, 2 ** 31 - 1]


def default_cfg():
    return load_pipeline_config("config/pipeline_config.yaml")


class Case:
    """One pipeline and its record matrix: steps, per non-trailing step a record array [n, width],
    token counts per document for the trailing TokenCounter steps."""

    def __init__(self, cfg, recs, tokens=None):
        h = native.host()
        self.cfg = cfg
        self.steps = [h.make_step(s.native_dict()) for s in cfg.pipeline]
        self.types = [s.type for s in cfg.pipeline]
        self.n_tok = 0
        while self.n_tok < len(self.types) and self.types[len(self.types) - 1 - self.n_tok] == "TokenCounter":
            self.n_tok += 1
        self.n_dev = len(self.types) - self.n_tok
        self.recs = [np.ascontiguousarray(np.array(r, dtype=np.int64).reshape(-1)) for r in recs]
        self.n = len(recs[0])
        self.tokens = np.asarray(tokens if tokens is not None else np.zeros(self.n), dtype=np.int64)
        self.data, self.off = np.zeros(16, np.uint8), np.zeros(self.n + 1, np.int64)
        self.resolve = h.build_resolve(self.steps, [(i, i, 0) for i in range(self.n_dev)], [-1] * self.n_dev)

    def tiled(self, n):
        """The same case with the rows repeated up to n documents."""
        reps = -(-n // self.n)
        recs = [np.tile(r.reshape(self.n, -1), (reps, 1))[:n] for r in self.recs]
        return Case(self.cfg, recs, np.tile(self.tokens, reps)[:n])

    def plan(self, row_cap=0):
        return native.host().build_meta_plan(self.steps, self.resolve, self.n_tok, row_cap)

    def host_resolve(self):
        h = native.host()
        fail, st, _, _, rows = h.resolve_host(self.resolve, self.recs, self.n, np.zeros(self.n, np.uint32),
                                              [self.data], [self.off])
        nk, nx = int(np.count_nonzero(st == 0)), int(np.count_nonzero(st == 1))
        return fail, st, rows, nk, nx

    def kept_tokens(self, rows, nk):
        return [np.ascontiguousarray(self.tokens[rows[:nk]], dtype=np.int32) for _ in range(self.n_tok)]

    def emulate(self, row_cap=0):
        fail, st, rows, nk, nx = self.host_resolve()
        return native.host().meta_format_host(self.resolve, self.plan(row_cap), self.recs, self.n, fail, rows, nk, nx,
                                              self.kept_tokens(rows, nk))

    def expected(self):
        """BatchState.apply_records over the same records, then assemble(rows, False): the column
        of the kept rows followed by the excluded rows."""
        h = native.host()
        bs = h.BatchState(self.data[:0], self.off, None, None, None, 2)
        for i in range(self.n_dev):
            bs.apply_records(self.steps[i], i, self.recs[i], -1)
        for i in range(self.n_dev, len(self.steps)):
            rec = np.full(self.n, -1, dtype=np.int64)
            alive = bs.alive_indices()
            rec[alive] = self.tokens[alive]
            bs.apply_records(self.steps[i], i, rec, -1)
        st = bs.status()
        parts = [bs.assemble(np.nonzero(st == k)[0].astype(np.int64), False)[2:] for k in (0, 1)]
        md = bytes(parts[0][0]) + bytes(parts[1][0])
        off = np.concatenate([parts[0][1], parts[1][1][1:] + parts[0][1][-1]])
        return md, off, np.concatenate([parts[0][2], parts[1][2]]), bs


def single_kind_case(kind, flip_exclude_zero=False):
    cfg = default_cfg()
    cfg.pipeline = [s for s in cfg.pipeline if s.type == kind]
    if flip_exclude_zero:
        cfg.pipeline[0].params.line_punct_exclude_zero = not cfg.pipeline[0].params.line_punct_exclude_zero
    return Case(cfg, [MATRIX[kind]()])


def default_case(with_tokens=True):
    """The default pipeline: for every step each row of its matrix with passing records in the
    other steps (so every branch is reached as the failing step and the steps before it emit their
    passed members), then kept rows with the token counts."""
    cfg = default_cfg()
    if not with_tokens:
        cfg.pipeline = [s for s in cfg.pipeline if s.type != "TokenCounter"]
    kinds = [s.type for s in cfg.pipeline if s.type != "TokenCounter"]
    cols = {k: [] for k in kinds}
    for k in kinds:
        for row in MATRIX[k]():
            for j in kinds:
                cols[j].append(row if j == k else PASS[j])
    tokens = [7] * len(cols[kinds[0]])
    for t in TOKENS:
        for j in kinds:
            cols[j].append(PASS[j])
        tokens.append(t)
    return Case(cfg, [cols[k] for k in kinds], tokens)


def token_only_case():
    cfg = default_cfg()
    cfg.pipeline = [s for s in cfg.pipeline if s.type in ("FineWebQualityFilter", "TokenCounter")]
    n = len(TOKENS)
    return Case(cfg, [[PASS["FineWebQualityFilter"]] * n], TOKENS)


def all_cases():
    out = {k: single_kind_case(k) for k in MATRIX}
    out["FineWeb_exclude_zero_flipped"] = single_kind_case("FineWebQualityFilter", True)
    out["default"] = default_case()
    out["default_no_tokens"] = default_case(False)
    out["fineweb_tokens"] = token_only_case()
    return out
