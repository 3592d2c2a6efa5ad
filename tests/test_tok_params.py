"""The token counters' parameter blocks (csrc/host/tok_params.h through the host module): the one
validator (bpe_spec_error / wp_spec_error) accepts the specs of every family and refuses malformed
ones in both executions (bpe_count / wp_count: the host emulation; bpe_params / wp_params: the
kernels' block), and the one filler writes every field from the spec and the addresses given."""
import dataclasses
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bpe_sp_corpus as sc  # noqa: E402

from textblaster_amd import native  # noqa: E402
from textblaster_amd.models import tokenizer as tk  # noqa: E402
from textblaster_amd.utils import synth  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = native.host()
R = dataclasses.replace
FREE = np.uint64(2 ** 64 - 1)  # a free slot of vslots (its value word) and of sp_cp

BPE_ARRAYS = ["byte_id", "keys", "vals", "added", "aoff", "vslots", "vpool", "sp_ascii", "sp_cp", "cls1", "cls2",
              "ccls1", "ccls2", "nfc1", "nfc2"]
WP_ARRAYS = ["slots", "pool", "added", "cls1", "cls2", "fold1", "fold2", "foldp"]
BPE_PTRS = {name: 0x1000 * (i + 1) for i, name in enumerate(BPE_ARRAYS)}  # never dereferenced
WP_PTRS = {name: 0x1000 * (i + 1) for i, name in enumerate(WP_ARRAYS)}


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """One tokenizer per family: the committed gpt2-format file and 4,000-entry trained ones."""
    d = tmp_path_factory.mktemp("tok")
    files = {
        "gpt2": os.path.join(REPO, "tests", "fixtures", "tokenizers", "gpt2", "tokenizer.json"),
        "split": tk.train_synthetic_split_bpe(str(d / "split4k_A1.json"), vocab_size=4000, pattern="A",
                                              ignore_merges=True, n_docs=1500, seed=2),
        "case": tk.train_synthetic_split_bpe(str(d / "case4k_C0.json"), vocab_size=4000, pattern="C",
                                             ignore_merges=False, n_docs=1500, seed=2),
        "sp": sc.tokenizer(d, "L-prepend"),
        "wp": tk.train_synthetic_wordpiece(str(d / "wp4k.json"), vocab_size=4000, n_docs=1500, seed=2),
        "wp_uncased": tk.train_synthetic_wordpiece(str(d / "wp4k_uncased.json"), vocab_size=4000, n_docs=1500, seed=2,
                                                   lowercase=True),
    }
    return {name: tk.TokenCounterModel(path) for name, path in files.items()}


@pytest.fixture(scope="module")
def specs(models):
    out = {name: m.device_spec() for name, m in models.items()}
    assert out["gpt2"].kind == tk.BPE_GPT2 and out["split"].kind == tk.BPE_SPLIT_A and out["split"].ignore_merges
    assert out["case"].kind == tk.BPE_CASE_C and out["sp"].kind == tk.BPE_SP
    assert out["wp"].fold == 0 and out["wp_uncased"].fold == 3  # lowercase, and strip_accents follows it
    return out


CORPUS = synth.make_corpus(10, 600, seed=31)


def is_wp(spec):
    return isinstance(spec, tk.WordPieceSpec)


def count(spec):
    data, off = synth.pack(CORPUS)
    return (H.wp_count if is_wp(spec) else H.bpe_count)(data, off, spec, 2)


def params(spec, ptrs=None):
    if is_wp(spec):
        return H.wp_params(spec, WP_PTRS if ptrs is None else ptrs)
    return H.bpe_params(spec, BPE_PTRS if ptrs is None else ptrs)


def field(block, spec, name, fmt):
    offsets = H.DEV_WP_OFFSETS if is_wp(spec) else H.DEV_BPE_OFFSETS
    v = struct.unpack_from("<" + fmt, block, offsets[name])
    return v[0] if len(v) == 1 else list(v)


@pytest.mark.parametrize("name", ["gpt2", "split", "case", "sp", "wp", "wp_uncased"])
def test_valid_specs_are_accepted_and_count_as_the_library(models, specs, name):
    raw = count(specs[name])
    assert raw.dtype == np.int32 and len(raw) == len(CORPUS)
    assert raw.tolist() == models[name].count(CORPUS)
    assert len(params(specs[name])) == (H.SIZEOF_DEV_WP if is_wp(specs[name]) else H.SIZEOF_DEV_BPE)
    assert params(specs[name]) == params(specs[name])  # byte for byte


def with_added(spec, n):
    """``n`` one-byte added tokens."""
    return R(spec, added=np.full(n, ord("#"), dtype=np.uint8), added_off=list(range(n + 1)))


def bpe_variants(s):
    g, sp, cs, spm = s["gpt2"], s["split"], s["case"], s["sp"]
    assert len(sp.added_off) >= 3
    off = list(sp.added_off)
    past_pool = sp.vslots.copy()
    used = np.nonzero(past_pool[1::2] != FREE)[0][0]
    past_pool[2 * used + 1] = np.uint64((len(sp.vpool) << 32) | 1)
    return {
        "byte_id of 255 entries": R(g, byte_id=g.byte_id[:255]),
        "keys shorter than mask + 1": R(g, keys=g.keys[:-1]),
        "vals shorter than keys": R(g, vals=g.vals[:-1]),
        "added_off not starting at 0": R(sp, added_off=[1] + off[1:]),
        "added_off unsorted": R(sp, added_off=[off[0], off[2], off[1]] + off[3:]),
        "added_off ending past added": R(sp, added_off=off[:-1] + [len(sp.added) + 1]),
        "nine added tokens on GPT-2": with_added(g, tk.MAX_ADDED + 1),
        "1,025 added tokens on a split spec": with_added(sp, tk.SPLIT_MAX_ADDED + 1),
        "ignore_merges on GPT-2": R(g, ignore_merges=True, vslots=sp.vslots, vmask=sp.vmask, vpool=sp.vpool,
                                    vlongest=sp.vlongest),
        "nfc on GPT-2": R(g, nfc=True),
        "nfc on SP": R(spm, nfc=True),
        "ignore_merges on SP": R(spm, ignore_merges=True, vslots=sp.vslots, vmask=sp.vmask, vpool=sp.vpool,
                                 vlongest=sp.vlongest),
        "vslots of the wrong length": R(sp, vslots=sp.vslots[:-2]),
        "vslots absent": R(sp, vslots=None),
        "vlongest 0 with ignore_merges": R(sp, vlongest=0),
        "a vslots entry past vpool": R(sp, vslots=past_pool),
        "sp_ascii of 127 entries": R(spm, sp_ascii=spm.sp_ascii[:127]),
        "sp_cp without a free slot": R(spm, sp_cp=np.where(spm.sp_cp == FREE, np.uint64(0x2581 << 32), spm.sp_cp)),
        "sp_cp shorter than sp_mask + 1": R(spm, sp_cp=spm.sp_cp[:-1]),
        "sp_flags with an unknown bit": R(spm, sp_prepend=8),
        "sp_flags with both prepend rules": R(spm, sp_prepend=3),
        "sp_flags prepend-always + split": R(spm, sp_prepend=tk.SP_PREPEND_ALWAYS, sp_split=True),
        "kind 6": R(cs, kind=6),
        "kind -1": R(g, kind=-1),
        "keys of another type": R(g, keys=g.keys.astype(np.float64)),
    }


def wp_variants(s):
    w, u = s["wp"], s["wp_uncased"]
    return {
        "slots of the wrong length": R(w, slots=w.slots[:-2]),
        "longest 0": R(w, longest=0),
        "max_chars -1": R(w, max_chars=-1),
        "cls_shift 1": R(w, cls_shift=1),
        "fold 4": R(u, fold=4),
        "fold -1": R(u, fold=-1),
        "ten added tokens": with_added(w, tk.MAX_ADDED + 2),
        "added_off ending past added": R(w, added_off=[0, len(w.added) + 1]),
    }


def test_malformed_specs_are_refused_by_both_executions(specs):
    variants = {**bpe_variants(specs), **wp_variants(specs)}
    assert len(variants) >= 26
    for what, bad in variants.items():
        for run in (count, params):
            with pytest.raises(ValueError):
                run(bad)
                pytest.fail(f"{what}: accepted by {run.__name__}")


def test_the_largest_added_token_lists_are_accepted(specs):
    """The bounds are kBpeMaxAdded / kBpeSplitMaxAdded themselves, not one below."""
    for spec, n in ((specs["gpt2"], tk.MAX_ADDED), (specs["split"], tk.SPLIT_MAX_ADDED), (specs["wp"], tk.MAX_ADDED)):
        ok = with_added(spec, n)
        assert len(count(ok)) == len(CORPUS)
        assert field(params(ok), ok, "n_added", "i") == n


def added_mask(spec):
    m = [0, 0, 0, 0]
    for a, b in zip(spec.added_off, spec.added_off[1:]):
        if b > a:
            m[int(spec.added[a]) >> 6] |= 1 << (int(spec.added[a]) & 63)
    return m


BPE_POINTER_FIELDS = {"aoff": "aoff", **{n: n for n in BPE_ARRAYS if n != "aoff"}}


@pytest.mark.parametrize("name", ["gpt2", "split", "case", "sp"])
def test_bpe_params_hold_the_spec_and_the_addresses(specs, name):
    sp = specs[name]
    blk = params(sp)
    mem = sp.kind != tk.BPE_GPT2  # the added tokens' offsets in memory behind the first-byte mask
    for fld, arr in BPE_POINTER_FIELDS.items():
        want = BPE_PTRS[arr] if (mem or fld != "aoff") else 0
        assert field(blk, sp, fld, "Q") == want, fld
    n_added = max(len(sp.added_off) - 1, 0)
    assert field(blk, sp, "mask", "I") == sp.mask and field(blk, sp, "n_added", "i") == n_added
    assert field(blk, sp, "post_add", "i") == sp.post_add and field(blk, sp, "kind", "i") == sp.kind
    assert field(blk, sp, "ignore_merges", "i") == int(sp.ignore_merges) and field(blk, sp, "nfc", "i") == int(sp.nfc)
    assert field(blk, sp, "vmask", "I") == sp.vmask and field(blk, sp, "vlongest", "i") == sp.vlongest
    assert field(blk, sp, "sp_mask", "I") == sp.sp_mask and field(blk, sp, "sp_id", "I") == sp.sp_id
    assert field(blk, sp, "sp_flags", "i") == sp.sp_flags
    inline = list(sp.added_off) + [0] * (tk.MAX_ADDED + 1 - len(sp.added_off))
    assert field(blk, sp, "added_off", f"{tk.MAX_ADDED + 1}i") == ([0] * (tk.MAX_ADDED + 1) if mem else inline)
    assert field(blk, sp, "amask", "4Q") == (added_mask(sp) if mem else [0] * 4)
    if name == "split":
        assert n_added > tk.MAX_ADDED and any(added_mask(sp))


def test_nfc_block_and_its_tables(specs):
    nfc = R(specs["split"], nfc=True)
    assert field(params(nfc), nfc, "nfc", "i") == 1 and field(params(nfc), nfc, "nfc1", "Q") == BPE_PTRS["nfc1"]


@pytest.mark.parametrize("name", ["wp", "wp_uncased"])
def test_wp_params_hold_the_spec_and_the_addresses(specs, name):
    sp = specs[name]
    blk = params(sp)
    for fld in ("slots", "pool", "added", "cls1", "cls2"):
        assert field(blk, sp, fld, "Q") == WP_PTRS[fld], fld
    f1, f2, fp = H.wp_fold_tables()
    stage1 = WP_PTRS["fold1"] + (sp.fold - 1) * f1.shape[1] * f1.itemsize  # the mode's part of the three
    assert [field(blk, sp, f, "Q") for f in ("fold1", "fold2", "foldp")] == (
        [stage1, WP_PTRS["fold2"], WP_PTRS["foldp"]] if sp.fold else [0, 0, 0])
    for fld, fmt in (("mask", "I"), ("flags", "I"), ("cls_shift", "I"), ("self_bit", "I"), ("max_chars", "i"),
                     ("longest", "i"), ("post_add", "i")):
        assert field(blk, sp, fld, fmt) == getattr(sp, fld), fld
    assert field(blk, sp, "n_added", "i") == len(sp.added_off) - 1 > 0
    assert field(blk, sp, "added_off", f"{tk.MAX_ADDED + 1}i")[:len(sp.added_off)] == list(sp.added_off)
    assert [field(blk, sp, f"asc{i}", "Q") for i in range(4)] == H.wp_ascii(sp.cls_shift).tolist()
    other = R(sp, cls_shift=2)
    assert [field(params(other), other, f"asc{i}", "Q") for i in range(4)] == H.wp_ascii(2).tolist()


def test_a_missing_address_of_a_needed_array_is_refused(specs):
    cases = [(specs["split"], "vslots"), (specs["split"], "vpool"), (specs["split"], "aoff"), (specs["case"], "ccls1"),
             (specs["case"], "ccls2"), (R(specs["split"], nfc=True), "nfc1"), (R(specs["case"], nfc=True), "nfc2"),
             (specs["sp"], "sp_cp"), (specs["sp"], "sp_ascii"), (specs["sp"], "byte_id"),
             (specs["wp_uncased"], "fold1"), (specs["wp_uncased"], "fold2"), (specs["wp_uncased"], "foldp")]
    for sp, name in cases:
        full = dict(WP_PTRS if is_wp(sp) else BPE_PTRS)
        params(sp, full)
        for ptrs in ({**full, name: 0}, {k: v for k, v in full.items() if k != name}):
            with pytest.raises(ValueError):
                params(sp, ptrs)
                pytest.fail(f"{name} = 0 accepted")
    # ... and an array the family does not read may stay away
    g = specs["gpt2"]
    lean = {k: v for k, v in BPE_PTRS.items() if k in ("byte_id", "keys", "vals", "added", "cls1", "cls2")}
    assert field(params(g, lean), g, "ccls1", "Q") == 0
    w = specs["wp"]
    assert field(params(w, {k: v for k, v in WP_PTRS.items() if not k.startswith("fold")}), w, "fold1", "Q") == 0


def test_python_constants_equal_the_headers():
    for name, value in H.TOK_CONSTANTS.items():
        assert getattr(tk, name) == value, name
    assert len(H.TOK_CONSTANTS) == 15


def test_merge_table_keeps_the_last_rank_of_a_repeated_pair():
    u32 = lambda v: np.array(v, dtype=np.uint32)  # noqa: E731
    keys, vals, mask = H.bpe_build_table(u32([1, 2, 1]), u32([2, 3, 2]), u32([0, 1, 2]), u32([7, 8, 9]))
    assert len(keys) == len(vals) == mask + 1 and (keys != FREE).sum() == 2
    assert int(vals[keys == np.uint64((1 << 32) | 2)][0]) == (2 << 32) | 9
    with pytest.raises(ValueError):
        H.bpe_build_table(u32([2 ** 32 - 1]), u32([2 ** 32 - 1]), u32([0]), u32([1]))
