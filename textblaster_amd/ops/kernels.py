"""ctypes bindings for libtbhip.so (the kernel units of csrc/hip/, html.hip, runtime.hip) and thin launch
helpers.

Device memory comes from the native runtime layer (ops/hiprt.py: caching HBM allocator,
``DevArray`` views); kernels are launched on the calling thread's current hiprt stream. Every
launch checks the returned hipError_t and raises — there is no silent fallback on a GPU box.

The argument groups the document kernels share travel as structs (``LAUNCH_STRUCTS``: each the one
mirror of its C struct in csrc/hip/kernel_common.h or its family's unit, sizes checked when
``Kernels`` is created): ``Tables`` per batch, ``Docs`` and ``Work`` per launch, ``DictIn`` /
``DictLines`` per content version / C4 step. ``_SIGS`` types them as ``POINTER(Struct)``, so a
struct in the wrong place raises in Python. The token counters' parameter blocks (DevBpe, DevWp) have
no mirror here: the host module fills them (csrc/host/tok_params.h) and returns them as bytes, as it
does the device plan, and ``BpeTables`` / ``WpTables`` only upload the arrays and keep the block.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from ..errors import DeviceError

_P = ctypes.c_void_p
_I32 = ctypes.c_int32
_U32 = ctypes.c_uint32
_I64 = ctypes.c_int64
_SZ = ctypes.c_size_t

# Bumped with every change of an entry point's signature or of a launch struct's layout: a stale
# libtbhip.so with an older argument list would otherwise be called with the wrong arguments.
ABI_VERSION = 27


def _ptr(t) -> Optional[int]:
    return None if t is None else t.data_ptr()


class Tables(ctypes.Structure):
    """TbTables: the Unicode property tables and the hash powers B^k / B^-k (``Kernels.tables``)."""
    _fields_ = [("s1", _P), ("s2", _P), ("l1", _P), ("l2", _P), ("pw", _P), ("pw_n", _U32)]


class Docs(ctypes.Structure):
    """TbDocs: a content version (bytes, off), the launch positions perm[0 .. n_launch) and the
    batch's dead marks; ``ndocs``: documents in the batch (the record stride)."""
    _fields_ = [("bytes", _P), ("off", _P), ("perm", _P), ("dead", _P), ("n_launch", _I32), ("ndocs", _I32)]

    @classmethod
    def of(cls, bytes_, off, perm, n_launch, ndocs, dead=None):
        if perm is not None and perm.numel() < n_launch:
            raise DeviceError("launch: the permutation is shorter than the launch")
        return cls(_ptr(bytes_), _ptr(off), _ptr(perm), _ptr(dead), int(n_launch), int(ndocs))


class Work(ctypes.Structure):
    """TbWork: what a document kernel writes (scratch slices by launch position, records, flags,
    phase counters) and its dynamic LDS slice."""
    _fields_ = [("scratch", _P), ("scratch_off", _P), ("rec", _P), ("flags", _P), ("prof", _P), ("lds_bytes", _U32)]

    @classmethod
    def of(cls, scratch, scratch_off, rec, flags, lds_bytes=0, prof=None):
        return cls(_ptr(scratch), _ptr(scratch_off), _ptr(rec), _ptr(flags), _ptr(prof), int(lds_bytes))


class DictIn(ctypes.Structure):
    """devplan.h DictIn: the word sources of a content version's dictionary-script documents."""
    _fields_ = [("moff", _P), ("bits", _P), ("words", _P)]


class DictLines(ctypes.Structure):
    """devplan.h DictLines (offsets int64, data uint32): host ICU line statistics of a C4 step's
    dictionary-script documents."""
    _fields_ = [("off", _P), ("data", _P)]


class BadWords(ctypes.Structure):
    """TbBadWords: the inputs of one C4BadWords step (``Kernels.badwords_match``)."""
    _fields_ = [("root", _P), ("cjk", _P), ("table", _P), ("f1", _P), ("f2", _P), ("seg_doc", _P), ("seg_idx", _P),
                ("root0", _I32), ("cjk0", _I32), ("dead_max", _U32), ("table_mask", _U32), ("seg_bytes", _U32)]


class ResolveOut(ctypes.Structure):
    """TbResolveOut: outputs and scratch of tb_resolve (``cap``: bytes of ``out``)."""
    _fields_ = [("fail", _P), ("status", _P), ("fver", _P), ("lanes", _P), ("sc", _P), ("out", _P), ("cap", _I64),
                ("out_off", _P), ("rows", _P), ("err", _P)]


class MetaOut(ctypes.Structure):
    """TbMetaOut: outputs and scratch of tb_meta_format (``cap``: bytes of ``out``)."""
    _fields_ = [("lens", _P), ("off", _P), ("valid", _P), ("out", _P), ("cap", _I64), ("err", _P)]


LAUNCH_STRUCTS = {Tables: "tb_sizeof_tables", Docs: "tb_sizeof_docs", Work: "tb_sizeof_work",
                  DictIn: "tb_sizeof_dict_in", DictLines: "tb_sizeof_dict_lines", BadWords: "tb_sizeof_badwords",
                  ResolveOut: "tb_sizeof_resolve_out", MetaOut: "tb_sizeof_meta_out"}

_TAB, _DOCS, _WORK = ctypes.POINTER(Tables), ctypes.POINTER(Docs), ctypes.POINTER(Work)

_SIGS = {
    # stream, plan, stage, docs, work, tables, line_stats, gr_export, dict_in
    "tb_stage_analyze": [_P, _P, _P, _DOCS, _WORK, _TAB, _P, _P, ctypes.POINTER(DictIn)],
    # stream, plan, stage, docs, work, tables, gr_export, n_split, split_bytes, line_stats, pre, dict_in
    "tb_stage_analyze_blk": [_P, _P, _P, _DOCS, _WORK, _TAB, _P, _I32, _U32, _P, _P, ctypes.POINTER(DictIn)],
    # (the same without pre)
    "tb_stage_analyze_blk_mid": [_P, _P, _P, _DOCS, _WORK, _TAB, _P, _I32, _U32, _P, ctypes.POINTER(DictIn)],
    # stream, stage, gr_step, docs, n_tasks, gr_export, work, tables, (block, n_big | cursor)
    "tb_gr_split_wave": [_P, _P, _I32, _DOCS, _I32, _P, _WORK, _TAB, _I32, _I32],
    "tb_gr_dup_split": [_P, _P, _I32, _DOCS, _I32, _P, _WORK, _TAB, _P],
    # stream, docs, pre, (tiles_max, cnt, tables | chunks_max, tables, flags)
    "tb_pre_decode": [_P, _DOCS, _P, _U32, _P, _TAB],
    "tb_pre_wcanon": [_P, _DOCS, _P, _U32, _TAB, _P],
    # stream, c4, docs, work, tables, src, line_stats, c4_words, dict_lines
    "tb_c4_pass_a": [_P, _P, _DOCS, _WORK, _TAB, _P, _P, _P, ctypes.POINTER(DictLines)],
    "tb_c4_pass_a_blk": [_P, _P, _DOCS, _WORK, _TAB, _P, _P, _P, ctypes.POINTER(DictLines)],
    "tb_c4_pass_b": [_P, _P, _P, _I32, _P, _P, _P, _P, _P],
    # stream, docs, tables, step inputs, matched
    "tb_badwords_match": [_P, _DOCS, _TAB, ctypes.POINTER(BadWords), _P],
    # stream, docs, tables, E, aux, WT, w_scale, bias, rec, width, prof
    "tb_langid_mfma": [_P, _DOCS, _TAB, _P, _P, _P, ctypes.c_double, _P, _P, _I32, _P],
    "tb_langid_prepare": [_P, _P, _P],
    "tb_langid_aux_bytes": [],
    "tb_gate": [_P, _P, _P, _I32, _I32, _P, _P, _I32],
    # stream, rp, recs, nrecs, ndocs, flags, vb, vo, nver, outputs
    "tb_resolve": [_P, _P, _P, _I32, _I32, _P, _P, _P, _I32, ctypes.POINTER(ResolveOut)],
    # stream, rp, mp, recs, nrecs, ndocs, fail, rows, sc, toks, ntoks, outputs
    "tb_meta_format": [_P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _I32, ctypes.POINTER(MetaOut)],
    "tb_sizeof_meta_plan": [],
    "tb_pow_table": [_P, _P, _U32],
    "tb_html_sizes": [_P, _P, _P, _I32, _P, _P, _P, _P, _I32, _P, _U32, _P],
    "tb_html_scatter": [_P, _P, _P, _I32, _P, _P, _P, _P, _I32, _P, _U32, _P, _P],
    "tb_bpe_count": [_P, _P, _P, _P, _P, _I32, _P],
    "tb_wp_count": [_P, _P, _P, _P, _P, _I32, _P],
    "tb_sizeof_wp": [],
    "tb_uni_count": [_P, _P, _P, _P, _P, _I32, _P],
    "tb_sizeof_uni": [],
    "tb_abi_version": [], "tb_block_threads": [], "tb_phase_slots": [], "tb_stage_waves": [],
    "tb_sizeof_pre_doc": [], "tb_sizeof_gr_export": [], "tb_sizeof_gate": [], "tb_sizeof_resolve": [],
    "tb_sizeof_bpe": [], "tb_sizeof_plan": [], "tb_sizeof_stage": [], "tb_sizeof_c4": [],
    **{name: [] for name in LAUNCH_STRUCTS.values()},
    # native runtime layer (csrc/hip/runtime.hip)
    "tbrt_device_count": [_P], "tbrt_set_device": [_I32], "tbrt_get_device": [_P], "tbrt_device_sync": [],
    "tbrt_mem_info": [_P, _P], "tbrt_malloc": [_P, _SZ], "tbrt_free": [_P], "tbrt_host_alloc": [_P, _SZ],
    "tbrt_host_free": [_P], "tbrt_empty_cache": [], "tbrt_cache_stats": [_P], "tbrt_stream_create": [_P, _I32],
    "tbrt_stream_destroy": [_P], "tbrt_stream_sync": [_P], "tbrt_stream_priority_range": [_P, _P],
    "tbrt_event_create": [_P, _I32], "tbrt_event_destroy": [_P], "tbrt_event_record": [_P, _P],
    "tbrt_event_sync": [_P], "tbrt_event_query": [_P], "tbrt_event_elapsed": [_P, _P, _P],
    "tbrt_stream_wait_event": [_P, _P], "tbrt_memcpy_h2d": [_P, _P, _SZ, _P], "tbrt_memcpy_d2h": [_P, _P, _SZ, _P],
    "tbrt_memcpy_d2d": [_P, _P, _SZ, _P], "tbrt_memset": [_P, _I32, _SZ, _P],
    "tb_scan_strided_i64": [_P, _P, _I64, _I64, _P],
}


# doc_ctx.h PreDoc (checked against tb_sizeof_pre_doc)
PRE_DOC = np.dtype([("off", "<u8"), ("prop", "<u8"), ("wbm", "<u8"), ("nl_pos", "<u8"), ("nl_len", "<u8"),
                    ("n", "<u4"), ("C", "<u4"), ("dict", "<u4"), ("NL", "<u4"), ("tcs", "<u4"), ("tce", "<u4"),
                    ("nl_a", "<u4"), ("nl_e", "<u4"), ("wtmp", "<u8"), ("wcs", "<u8"), ("wce", "<u8"),
                    ("wbs", "<u8"), ("wbe", "<u8"), ("wal", "<u8"), ("W", "<u4"), ("pad", "<u4"),
                    ("wh", "<u8"), ("wtab", "<u8"), ("wk", "<u8"), ("wpb", "<u8"), ("wcsum", "<u8"),
                    ("wslot", "<u8"), ("wid", "<u8"), ("wl", "<u8"), ("wready", "<u4"), ("pad2", "<u4")])
PRE_WCHUNK = 2048  # prepass.hip kPreWChunk
PRE_TILE = 16384  # prepass.hip kPreTile


class _TokTables:
    """A token counter's tables in HBM and the kernel's parameter block pointing at them. The block
    is built by the host module (csrc/host/tok_params.h: the code that fills it for the host
    emulation too) from the spec and the addresses of ``arrays`` (name -> host array, None = the
    spec has none); a spec it refuses raises DeviceError."""

    def __init__(self, params, spec, arrays):
        from . import hiprt

        self.arrays = {name: hiprt.to_device(a) for name, a in arrays.items() if a is not None}
        try:
            self.block = params(spec, {name: a.data_ptr() for name, a in self.arrays.items()})
        except ValueError as e:
            raise DeviceError(str(e)) from e


class BpeTables(_TokTables):
    """csrc/common/bpe.h DevBpe of a models/tokenizer.py BpeSpec; ``static``: the class / NFC tables
    of its family by DevBpe field name."""

    def __init__(self, h, spec, static):
        super().__init__(h.bpe_params, spec, {
            "byte_id": spec.byte_id, "keys": spec.keys, "vals": spec.vals, "added": spec.added,
            "aoff": np.array(spec.added_off or [0], dtype=np.int32), "vslots": spec.vslots, "vpool": spec.vpool,
            "sp_ascii": spec.sp_ascii, "sp_cp": spec.sp_cp, **static})


class WpTables(_TokTables):
    """csrc/common/wordpiece.h DevWp of a models/tokenizer.py WordPieceSpec; ``static``: the class
    table and, for a folding spec, wp_fold.inc (stage 1 of all three modes: the block names the
    mode's, and tb_wp_count then launches k_wp_count_fold)."""

    def __init__(self, h, spec, static):
        super().__init__(h.wp_params, spec, {"slots": spec.slots, "pool": spec.pool, "added": spec.added, **static})


class UniTables(_TokTables):
    """csrc/common/unigram.h DevUni of a models/tokenizer.py UnigramSpec: the spec carries every
    table, the class table of its own normalizer included, and with a map (spec.mapped) that
    normalizer's replacements: tb_uni_count then launches k_uni_count_map."""

    def __init__(self, h, spec):
        maps = {"map1": spec.map1, "map2": spec.map2, "map_rec": spec.map_rec, "map_pool": spec.map_pool}
        super().__init__(h.uni_params, spec, {
            "slots": spec.slots, "pool": spec.pool, "added": spec.added, "cls1": spec.cls1, "cls2": spec.cls2,
            "aoff": np.array(spec.added_off or [0], dtype=np.int32), **(maps if spec.mapped else {})})


def declare(lib: ctypes.CDLL) -> None:
    for name, args in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = ctypes.c_size_t if name.startswith("tb_sizeof") else ctypes.c_int


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise DeviceError(f"{what} failed with hipError_t {rc}")


def _ptr_array8(arrays):
    """Up to 8 device arrays as a void*[8] (null-padded)."""
    return (ctypes.c_void_p * 8)(*([a.data_ptr() for a in arrays] + [None] * (8 - len(arrays))))


class Kernels:
    """Launch helpers bound to one device (holds the Unicode tables in HBM)."""

    def __init__(self, device: int):
        from .. import native
        from . import hiprt

        self.device = device
        self.lib = native.hip()
        h = native.host()
        if self.lib.tb_abi_version() != ABI_VERSION:
            raise DeviceError(f"libtbhip.so ABI {self.lib.tb_abi_version()} != {ABI_VERSION}; rebuild")
        if (self.lib.tb_sizeof_plan() != h.SIZEOF_DEV_PLAN or self.lib.tb_sizeof_stage() != h.SIZEOF_DEV_STAGE
                or self.lib.tb_sizeof_gate() != h.SIZEOF_DEV_GATE
                or self.lib.tb_sizeof_resolve() != h.SIZEOF_DEV_RESOLVE
                or self.lib.tb_sizeof_meta_plan() != h.SIZEOF_DEV_META_PLAN
                or self.lib.tb_sizeof_bpe() != h.SIZEOF_DEV_BPE or self.lib.tb_sizeof_wp() != h.SIZEOF_DEV_WP):
            raise DeviceError("libtbhip.so and _tbhost disagree on the device plan or token counter layout; rebuild")
        self.sizeof_gr_export = int(self.lib.tb_sizeof_gr_export())
        if int(self.lib.tb_sizeof_pre_doc()) != PRE_DOC.itemsize:
            raise DeviceError("libtbhip.so and ops/kernels.py disagree on PreDoc; rebuild")
        for st, sizeof in LAUNCH_STRUCTS.items():
            if int(getattr(self.lib, sizeof)()) != ctypes.sizeof(st):
                raise DeviceError(f"libtbhip.so and ops/kernels.py disagree on {st.__name__}; rebuild")
        s1, s2, l1, l2 = h.ucd_tables()
        self.tabs = [hiprt.to_device(a) for a in (s1, s2, l1, l2)]
        self._pw = None
        self._pw_n = 0

    @staticmethod
    def stream() -> int:
        from . import hiprt

        return hiprt.current_stream().handle

    def pow_table(self, n: int):
        if n > self._pw_n:
            from . import hiprt

            cap = max(n, 1 << 16)
            cap = 1 << (cap - 1).bit_length()
            # B^0..B^cap followed by B^-0..B^-cap (k_pow_table)
            self._pw = hiprt.empty(2 * cap + 2, np.int64)
            _check(self.lib.tb_pow_table(self.stream(), self._pw.data_ptr(), cap), "tb_pow_table")
            # other slots' streams read the table right away with no event ordering them after
            # the kernel that fills it: growth is rare (documents over ~2 MB), so wait for it here
            hiprt.current_stream().synchronize()
            self._pw_n = cap
        return self._pw, self._pw_n

    def tables(self, pw, pw_n) -> Tables:
        """The tables struct of a batch: this device's Unicode tables + the batch's ``pow_table``."""
        return Tables(*[t.data_ptr() for t in self.tabs], pw.data_ptr(), pw_n)

    def stage_analyze(self, plan, stage, docs: Docs, work: Work, tables: Tables, line_stats=None, gr_export=None,
                      dict_in: Optional[DictIn] = None):
        """k_stage_analyze_wave over launch positions [0, docs.n_launch) (0: all); ``line_stats``
        (uint32, >= 4 * (total bytes / 8 + 16 ndocs) + 16): the C4 line export (stage_analyze.h
        StageOut::line_stats), document d at 4 * (off[d] / 8 + 16 d). ``gr_export`` (zeroed, >=
        n_launch descriptors): split mode, every launched document exports its word arrays and
        gr_split_wave finishes its n-gram orders (the launcher then runs k_stage_analyze_wave_ex,
        the build without the in-stage n-gram code: the stage must have exactly one
        GopherRepetition step with n-gram orders, or its documents go to the CPU path)."""
        if gr_export is not None and gr_export.nbytes < max(docs.n_launch, 0) * self.sizeof_gr_export:
            raise DeviceError("stage_analyze: export buffer too small")
        rc = self.lib.tb_stage_analyze(self.stream(), plan.data_ptr(), stage.data_ptr(), docs, work, tables,
                                       _ptr(line_stats), _ptr(gr_export), dict_in)
        _check(rc, "tb_stage_analyze")

    def gr_export_wave_bytes(self, n_docs: int) -> int:
        """Bytes of a zeroed wave export buffer: n_docs descriptors, then the k_gr_ngrams kernels'
        two lists of the documents their LDS arrays cannot hold (NgRest: 32-byte header + two u32
        per document)."""
        return n_docs * self.sizeof_gr_export + 32 + 8 * n_docs

    def gr_split_wave(self, stage, gr_step, docs: Docs, n_tasks, gr_export, work: Work, tables: Tables, block=True,
                      n_big=0):
        """The n-gram orders of the wave documents stage_analyze exported (n_tasks = the
        GopherRepetition step's duplicated + top orders). With ``block`` one workgroup per
        document builds the word arrays on chip (k_gr_ngrams: launch positions [0, n_big) with
        512-word arrays, the rest with 256-word ones, what they leave with 1024-word ones);
        without it the generic code, one wave per (document, order) (k_gr_words, k_gr_split_wave)."""
        if not 0 <= n_big <= docs.n_launch:
            raise DeviceError("gr_split_wave: n_big out of range")
        if gr_export.nbytes < self.gr_export_wave_bytes(docs.n_launch):
            raise DeviceError("gr_split_wave: operand shapes")
        rc = self.lib.tb_gr_split_wave(self.stream(), stage.data_ptr(), gr_step, docs, n_tasks, gr_export.data_ptr(),
                                       work, tables, 1 if block else 0, int(n_big))
        _check(rc, "tb_gr_split_wave")

    def stage_analyze_blk(self, plan, stage, docs: Docs, work: Work, tables: Tables, gr_export=None, n_split=0,
                          split_bytes=0, line_stats=None, pre=None, dict_in: Optional[DictIn] = None, mid=False):
        """k_stage_analyze_blk; ``gr_export`` (zeroed, >= n_split descriptors): the first n_split
        launch positions longer than ``split_bytes`` export their word arrays (split mode);
        ``pre``: the pre-pass descriptors of every launched document. ``mid``: the 256-thread
        build for mid-sized documents (k_stage_analyze_blk_mid; it has no pre-pass variant)."""
        if gr_export is not None and gr_export.nbytes < n_split * self.sizeof_gr_export:
            raise DeviceError("stage_analyze_blk: export buffer too small")
        if not 0 <= n_split <= docs.n_launch:
            raise DeviceError("stage_analyze_blk: n_split out of range")
        ns = n_split if gr_export is not None else 0
        if mid:
            if pre is not None:
                raise DeviceError("stage_analyze_blk: the mid-size kernel takes no pre-pass documents")
            rc = self.lib.tb_stage_analyze_blk_mid(self.stream(), plan.data_ptr(), stage.data_ptr(), docs, work,
                                                   tables, _ptr(gr_export), ns, split_bytes, _ptr(line_stats),
                                                   dict_in)
        else:
            rc = self.lib.tb_stage_analyze_blk(self.stream(), plan.data_ptr(), stage.data_ptr(), docs, work, tables,
                                               _ptr(gr_export), ns, split_bytes, _ptr(line_stats), _ptr(pre), dict_in)
        _check(rc, "tb_stage_analyze_blk_mid" if mid else "tb_stage_analyze_blk")

    def pre_decode(self, docs: Docs, pre, tiles_max, cnt, tables: Tables):
        """k_pre_count / k_pre_decode / k_pre_wb: code points and word-break marks of
        the first ``docs.n_launch`` long documents over many workgroups; ``pre``: PRE_DOC
        descriptors (device), ``cnt``: int64 [n_launch * tiles_max]."""
        npre = docs.n_launch
        if cnt.numel() < npre * tiles_max or pre.nbytes < npre * PRE_DOC.itemsize:
            raise DeviceError("pre_decode: operand shapes")
        rc = self.lib.tb_pre_decode(self.stream(), docs, pre.data_ptr(), int(tiles_max), cnt.data_ptr(), tables)
        _check(rc, "tb_pre_decode")

    def pre_wcanon(self, docs: Docs, pre, chunks_max, tables: Tables, flags):
        """k_pre_wcanon / k_pre_wsum: GopherRepetition's word hashes, canonical word ids
        and concatenation-hash arrays of the pre-pass documents over many workgroups (after
        pre_decode; ``chunks_max`` >= ceil(max words / PRE_WCHUNK))."""
        if pre.nbytes < docs.n_launch * PRE_DOC.itemsize or chunks_max <= 0:
            raise DeviceError("pre_wcanon: operand shapes")
        rc = self.lib.tb_pre_wcanon(self.stream(), docs, pre.data_ptr(), int(chunks_max), tables, flags.data_ptr())
        _check(rc, "tb_pre_wcanon")

    def gr_dup_split(self, stage, gr_step, docs: Docs, n_tasks, gr_export, work: Work, tables: Tables, cursor):
        """k_gr_dup_split: persistent workgroups take (split document, task) pairs from an atomic
        cursor (``cursor``: a uint32 device word of this launch, reset by the call; keep it alive
        until the kernel completes); n_tasks = the GopherRepetition step's duplicated + top n-gram
        orders + duplicated lines + paragraphs."""
        if gr_export.nbytes < docs.n_launch * self.sizeof_gr_export or cursor.nbytes < 4:
            raise DeviceError("gr_dup_split: operand shapes")
        rc = self.lib.tb_gr_dup_split(self.stream(), stage.data_ptr(), gr_step, docs, n_tasks, gr_export.data_ptr(),
                                      work, tables, cursor.data_ptr())
        _check(rc, "tb_gr_dup_split")

    def badwords_match(self, tables: Tables, bytes_, off, ndocs, table, fold, matched, root=None, cjk=None, root0=-1,
                       cjk0=0, dead=None, dead_max=0, seg_bytes=2048, seg_doc=None, seg_idx=None):
        """k_badwords_match over documents [0, ndocs) of (bytes_, off): ``table`` is the hashed trie
        table (uint32 [4 * slots], csrc/common/badwords.h); per document root/cjk arrays, or one
        root0/cjk0 for all; documents with 0 < dead <= dead_max are skipped (matched -1). The first
        launch covers the first ``seg_bytes`` of every document; ``seg_doc`` / ``seg_idx`` (int32,
        the documents' further segments) add a second launch over those segments."""
        slots = table.numel() // 4
        if slots < 1 or slots & (slots - 1) or matched.numel() < ndocs or off.numel() < ndocs + 1:
            raise DeviceError("badwords_match: operand shapes")
        for a in (root, cjk, dead):
            if a is not None and a.numel() < ndocs:
                raise DeviceError("badwords_match: per-document array shorter than the batch")
        if (seg_doc is None) != (seg_idx is None) or (seg_doc is not None and seg_doc.numel() != seg_idx.numel()):
            raise DeviceError("badwords_match: segment lists")
        for sd, si in ((None, None), (seg_doc, seg_idx)):
            nitems = ndocs if sd is None else sd.numel()
            if sd is not None and nitems == 0:
                continue
            bw = BadWords(_ptr(root), _ptr(cjk), table.data_ptr(), fold[0].data_ptr(), fold[1].data_ptr(), _ptr(sd),
                          _ptr(si), int(root0), int(cjk0), int(dead_max), slots - 1, int(seg_bytes))
            rc = self.lib.tb_badwords_match(self.stream(), Docs.of(bytes_, off, None, nitems, ndocs, dead), tables,
                                            bw, matched.data_ptr())
            _check(rc, "tb_badwords_match")

    def langid_prepare(self, E):
        """The pair table of k_langid_mfma (orders 1 + 2 of every position over a 32-letter alphabet,
        + a zero row) built on the device from the embedding table ``E`` (E + 128, uint8); once per
        model. Returns the device buffer to pass as ``aux``."""
        from .. import native
        from . import hiprt

        h = native.host()
        if E.numel() != h.LID_BUCKETS * h.LID_ROW_DIM:
            raise DeviceError("langid_prepare: operand shapes")
        aux = hiprt.empty(int(self.lib.tb_langid_aux_bytes()), np.uint8)
        _check(self.lib.tb_langid_prepare(self.stream(), E.data_ptr(), aux.data_ptr()), "tb_langid_prepare")
        hiprt.current_stream().synchronize()
        return aux

    def langid_mfma(self, docs: Docs, tables: Tables, E, aux, WT, w_scale, bias, rec, width, prof=None):
        """k_langid_mfma (v3 model): fastText int8 embedding bag + bf16 MFMA head, 16 documents per
        tile; the language record of every launched document into ``rec`` (document d at
        rec[d * width]). ``E``: the embedding table as E + 128, uint8 [buckets * 16], ``aux``: its
        pair table (langid_prepare), ``WT``: bf16 bits [16 * 32] (head transposed), ``bias``:
        float32 [8] (csrc/common/langid.h)."""
        from .. import native

        h = native.host()
        if (E.numel() != h.LID_BUCKETS * h.LID_ROW_DIM or WT.numel() != 16 * h.LID_DIM or bias.numel() != h.LID_ROW
                or width < 2 or rec.numel() < docs.n_launch * width or not w_scale > 0
                or aux.numel() != int(self.lib.tb_langid_aux_bytes())):
            raise DeviceError("langid_mfma: operand shapes")
        rc = self.lib.tb_langid_mfma(self.stream(), docs, tables, E.data_ptr(), aux.data_ptr(), WT.data_ptr(),
                                     float(w_scale), bias.data_ptr(), rec.data_ptr(), width, _ptr(prof))
        _check(rc, "tb_langid_mfma")

    def c4_pass_a(self, c4, docs: Docs, work: Work, tables: Tables, src, line_stats=None, c4_words=None,
                  dict_lines: Optional[DictLines] = None, blk=False):
        """k_c4_pass_a (``blk``: k_c4_pass_a_blk, one workgroup per document); ``line_stats``: the
        line export of a stage over the same content version (trimmed spans, word counts and
        longest words of the Rust lines: documents without a citation skip decode, lines and words
        when split_paragraph is set). ``c4_words`` (uint32 per document, preset to 0xFFFFFFFF):
        the rewrite's word count on the export path."""
        name = "tb_c4_pass_a_blk" if blk else "tb_c4_pass_a"
        rc = getattr(self.lib, name)(self.stream(), c4.data_ptr(), docs, work, tables, src.data_ptr(),
                                     _ptr(line_stats), _ptr(c4_words), dict_lines)
        _check(rc, name)

    def c4_pass_b(self, bytes_, off, ndocs, scratch, scratch_off, src, new_off, out):
        rc = self.lib.tb_c4_pass_b(self.stream(), bytes_.data_ptr(), off.data_ptr(), ndocs, scratch.data_ptr(),
                                   scratch_off.data_ptr(), src.data_ptr(), new_off.data_ptr(), out.data_ptr())
        _check(rc, "tb_c4_pass_b")

    def gate(self, gate, recs, ndocs, flags, dead, code, max_slot, need):
        """k_gate: mark documents that a step of the finished pass filtered (dead[doc] = code).
        ``need``: int64 fields per document the gate's steps read from each record buffer (the
        kernel trusts the blob's prefix/width, so the buffers are checked here)."""
        if not 0 < code <= 255:
            raise DeviceError("gate code out of range")
        if max_slot >= len(recs) or len(recs) > 8 or dead.numel() < ndocs or flags.numel() < ndocs:
            raise DeviceError("gate: operand shapes")
        if any(r.numel() < need * ndocs for r in recs):
            raise DeviceError("gate: a record buffer is smaller than the gate's steps read")
        rc = self.lib.tb_gate(self.stream(), gate.data_ptr(), ctypes.cast(_ptr_array8(recs), ctypes.c_void_p),
                              len(recs), ndocs, flags.data_ptr(), dead.data_ptr(), code)
        _check(rc, "tb_gate")

    def bpe_tables(self, spec) -> BpeTables:
        from .. import native
        from ..models.tokenizer import BPE_CASE_C, BPE_CASE_D

        h = native.host()
        static = dict(zip(("cls1", "cls2"), h.bpe_classes()))
        if spec.kind in (BPE_CASE_C, BPE_CASE_D):  # csrc/common/bpe_case_classes.inc
            static.update(zip(("ccls1", "ccls2"), h.bpe_case_classes()))
        if spec.nfc:  # the NFC gate's table (csrc/common/nfc_qc.inc)
            static.update(zip(("nfc1", "nfc2"), h.nfc_qc()))
        return BpeTables(h, spec, static)

    def bpe_count(self, tabs: BpeTables, text, off, n_dev, n_max: int, counts):
        """k_bpe_count + k_bpe_long, or for a split-regex spec k_bpe_split_count + k_bpe_split_long,
        for a SentencePiece-style spec k_bpe_sp_count + k_bpe_sp_long
        (k_bpe_case_count + k_bpe_case_long for the case-aware patterns; the _nfc count kernels behind
        the NFC gate):
        token counts of documents k < min(n_dev[0], n_max) (csrc/hip/bpe.hip); ``n_dev``: optional
        one-element int64 device array (the kept count of K16)."""
        if off.numel() < n_max + 1 or counts.numel() < n_max or off.dtype != np.int64 or counts.dtype != np.int32:
            raise DeviceError("bpe_count: operand shapes")
        rc = self.lib.tb_bpe_count(self.stream(), tabs.block, text.data_ptr(), off.data_ptr(),
                                   _ptr(n_dev), n_max, counts.data_ptr())
        _check(rc, "tb_bpe_count")

    def wp_tables(self, spec) -> WpTables:
        from .. import native

        h = native.host()
        static = dict(zip(("cls1", "cls2"), h.wp_classes()))
        if spec.fold:
            static.update(zip(("fold1", "fold2", "foldp"), h.wp_fold_tables()))
        return WpTables(h, spec, static)

    def wp_count(self, tabs: WpTables, text, off, n_dev, n_max: int, counts):
        """k_wp_count: WordPiece token counts under bpe_count's contract (csrc/hip/wordpiece.hip)."""
        if off.numel() < n_max + 1 or counts.numel() < n_max or off.dtype != np.int64 or counts.dtype != np.int32:
            raise DeviceError("wp_count: operand shapes")
        rc = self.lib.tb_wp_count(self.stream(), tabs.block, text.data_ptr(), off.data_ptr(),
                                  _ptr(n_dev), n_max, counts.data_ptr())
        _check(rc, "tb_wp_count")

    def uni_tables(self, spec) -> UniTables:
        from .. import native

        return UniTables(native.host(), spec)

    def uni_count(self, tabs: UniTables, text, off, n_dev, n_max: int, counts):
        """k_uni_count, or k_uni_count_map for tables with a map: Unigram token counts under
        bpe_count's contract (csrc/hip/unigram.hip)."""
        if off.numel() < n_max + 1 or counts.numel() < n_max or off.dtype != np.int64 or counts.dtype != np.int32:
            raise DeviceError("uni_count: operand shapes")
        rc = self.lib.tb_uni_count(self.stream(), tabs.block, text.data_ptr(), off.data_ptr(),
                                   _ptr(n_dev), n_max, counts.data_ptr())
        _check(rc, "tb_uni_count")

    def token_tables(self, spec):
        """The device tables of a token counter spec of any kind."""
        from ..models.tokenizer import UnigramSpec, WordPieceSpec

        if isinstance(spec, UnigramSpec):
            return self.uni_tables(spec)
        return self.wp_tables(spec) if isinstance(spec, WordPieceSpec) else self.bpe_tables(spec)

    def token_count(self, tabs, text, off, n_dev, n_max: int, counts):
        """k_wp_count, k_uni_count, k_bpe_count or k_bpe_split_count, by the kind of ``tabs``."""
        fn = self.wp_count if isinstance(tabs, WpTables) else (
            self.uni_count if isinstance(tabs, UniTables) else self.bpe_count)
        fn(tabs, text, off, n_dev, n_max, counts)

    def resolve(self, rp, recs, ndocs, flags, versions, fail, status, fver, lanes, sc, out, out_off, rows, err):
        """K16: k_resolve + four scans + k_compact (see tb_resolve). ``recs``: record buffers by
        slot; ``versions``: [(bytes, offsets)] by content version; the rest are outputs/scratch."""
        if len(recs) > 8 or not 1 <= len(versions) <= 8:
            raise DeviceError("resolve: too many record buffers or versions")
        if (flags.numel() < ndocs or fail.numel() < ndocs or status.numel() < ndocs or fver.numel() < ndocs
                or lanes.numel() < 4 * ndocs or sc.numel() < 4 * ndocs or out_off.numel() < ndocs + 1
                or rows.numel() < ndocs or err.numel() < 1 or any(vo.numel() != ndocs + 1 for _, vo in versions)):
            raise DeviceError("resolve: operand shapes")
        ra, vb, vo = (ctypes.cast(_ptr_array8(x), ctypes.c_void_p)
                      for x in (recs, [b for b, _ in versions], [o for _, o in versions]))
        bufs = ResolveOut(fail.data_ptr(), status.data_ptr(), fver.data_ptr(), lanes.data_ptr(), sc.data_ptr(),
                          out.data_ptr(), out.numel(), out_off.data_ptr(), rows.data_ptr(), err.data_ptr())
        rc = self.lib.tb_resolve(self.stream(), rp.data_ptr(), ra, len(recs), ndocs, flags.data_ptr(), vb, vo,
                                 len(versions), bufs)
        _check(rc, "tb_resolve")

    def meta_format(self, rp, mp, recs, ndocs, fail, rows, sc, toks, lens, off, valid, out, err):
        """K18: k_meta_size + scan + k_meta_write (see tb_meta_format) over tb_resolve's ``fail`` /
        ``rows`` / ``sc``. ``toks``: the k_bpe_count result arrays of the plan's trailing
        TokenCounter steps; ``lens`` [ndocs] scratch, ``off`` [ndocs + 1], ``valid`` [ndocs],
        ``out`` the column bytes, ``err`` one zeroed int32 are the outputs."""
        if len(recs) > 8 or len(toks) > 4:
            raise DeviceError("meta_format: too many record buffers or token arrays")
        if (fail.numel() < ndocs or rows.numel() < ndocs or sc.numel() < 4 * ndocs or lens.numel() < ndocs
                or off.numel() < ndocs + 1 or valid.numel() < ndocs or err.numel() < 1
                or any(t.numel() < ndocs for t in toks) or lens.dtype != np.int64 or off.dtype != np.int64
                or fail.dtype != np.int32 or rows.dtype != np.int32 or sc.dtype != np.int64):
            raise DeviceError("meta_format: operand shapes")
        ra, ta = (ctypes.cast(_ptr_array8(x), ctypes.c_void_p) for x in (recs, toks))
        bufs = MetaOut(lens.data_ptr(), off.data_ptr(), valid.data_ptr(), out.data_ptr(), out.numel(), err.data_ptr())
        rc = self.lib.tb_meta_format(self.stream(), rp.data_ptr(), mp.data_ptr(), ra, len(recs), ndocs,
                                     fail.data_ptr(), rows.data_ptr(), sc.data_ptr(), ta, len(toks), bufs)
        _check(rc, "tb_meta_format")
