"""TokenCounter tokenizer (reference src/pipeline/token/token_counter.rs:8-43).

The reference calls ``Tokenizer::from_pretrained(name)`` (a Hugging Face Hub download). There is
no network here, so the name is resolved locally, in order:
  1. ``name`` is a path to a ``tokenizer.json`` file or to a directory containing one;
  2. ``<tokenizer_dir>/<name>/tokenizer.json`` (CLI ``--tokenizer-dir``, env ``TB_TOKENIZER_DIR``);
  3. the Hugging Face cache (``$HF_HOME`` / ``~/.cache/huggingface/hub/models--<name>/snapshots/*``).
Load failure raises ``Unexpected("Error in loading tokenizer")`` like the reference.

Counting = ``len(encode(text, add_special_tokens=True).tokens)``, batched through the Rust
tokenizers library's parallel ``encode_batch``. GPT-2-style byte-level BPE tokenizers also get a
:class:`BpeSpec` (:meth:`TokenCounterModel.bpe_spec`): the merge table as an open-addressed hash
table plus the byte ids, which the device pipeline counts with (csrc/common/bpe.h, k_bpe_count)
and ``count_native`` runs on the host (same algorithm; documents it cannot count exactly are
counted by ``tokenizers``). So do the byte-level BPE tokenizers serialised as
Split(regex) + ByteLevel(use_regex=false) with the Llama-3 / cl100k_base pattern or Qwen2's
(csrc/common/bpe_split.h, k_bpe_split_count), or with the case-aware pattern of o200k_base or of
Mistral's Tekken (csrc/common/bpe_case.h, k_bpe_case_count): their spec also carries the vocabulary's raw bytes
for ``ignore_merges`` and up to 1024 added tokens. Real Qwen2 files carry an NFC normalizer: their
spec has ``nfc`` set, and the counter (k_bpe_split_count_nfc) counts the documents that the Unicode
quick check proves NFC leaves unchanged and returns -2 for the rest. WordPiece tokenizers (BertNormalizer +
BertPreTokenizer, the BERT family) get a :class:`WordPieceSpec` instead (:meth:`TokenCounterModel.wordpiece_spec`): the vocabulary as an
open-addressed hash table over a byte pool (csrc/common/wordpiece.h, k_wp_count). With ``lowercase``
or ``strip_accents`` the device path counts with :meth:`TokenCounterModel.wordpiece_fold_spec`, which
names the fold tables of the tokenizer's mode (csrc/common/wp_fold.inc, k_wp_count_fold).
The SentencePiece-converted character-level BPE files with ``byte_fallback`` (Llama-2, Mistral, Gemma:
normalizer Prepend + Replace(" ", "▁") and no pre-tokenizer, or a Metaspace pre-tokenizer) get a
:class:`BpeSpec` of kind ``BPE_SP`` (csrc/common/bpe_sp.h, k_bpe_sp_count): the ids of the
single-character entries, of the 256 ``<0xNN>`` tokens and of ``▁``, and the prepend and split rules.
Unigram files (T5, mT5, XLM-R: a Precompiled normalizer, white-space splitting and Metaspace in one
of two layouts) get a :class:`UnigramSpec` (:meth:`TokenCounterModel.unigram_spec`; csrc/common/unigram.h,
k_uni_count): the pieces with their scores in a hash table over a byte pool, and a class table probed
from the file's own normalizer that says which code points it keeps, turns into a space, or changes
(documents with one of those are counted by ``tokenizers``). The mapped spec
(:meth:`TokenCounterModel.unigram_map_spec`, k_uni_count_map, ``TB_TUNE=uni_map=1``) also carries what
the normalizer changes those code points into, for the counter to apply itself.

A spec is data only. The host module reads it as it stands (``bpe_count`` / ``wp_count`` for the host
emulation (``uni_count`` for Unigram), ``bpe_params`` / ``wp_params`` / ``uni_params`` for the kernels' parameter block), and one validator and
one filler there (csrc/host/tok_params.h) decide whether it is usable and write the block for both.
"""
from __future__ import annotations

import glob
import os
import dataclasses
import json
from typing import List, Optional

import numpy as np

from ..errors import Unexpected


def resolve_tokenizer_file(name: str, tokenizer_dir: Optional[str] = None) -> Optional[str]:
    cands = []
    if os.path.isfile(name):
        cands.append(name)
    if os.path.isdir(name):
        cands.append(os.path.join(name, "tokenizer.json"))
    for d in (tokenizer_dir, os.environ.get("TB_TOKENIZER_DIR")):
        if d:
            cands.append(os.path.join(d, name, "tokenizer.json"))
            cands.append(os.path.join(d, name.replace("/", "--"), "tokenizer.json"))
    hf = os.environ.get("HF_HOME", os.path.join(os.path.expanduser("~"), ".cache", "huggingface"))
    cands += sorted(glob.glob(os.path.join(hf, "hub", "models--" + name.replace("/", "--"), "snapshots", "*",
                                           "tokenizer.json")))
    for c in cands:
        if os.path.isfile(c):
            return c
    return None


def bytes_to_unicode() -> List[str]:
    """GPT-2's byte -> printable character map of the ByteLevel pre-tokenizer."""
    bs = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    m = dict(zip(bs, cs))
    return [chr(m[b]) for b in range(256)]


MAX_ADDED = 8  # csrc/common/bpe.h kBpeMaxAdded (this and the constants below: pinned to the headers' values by
# tests/test_tok_params.py through the host module's TOK_CONSTANTS)


def _u32(v) -> np.ndarray:
    return np.array(v, dtype=np.uint32)


def _pack_added(contents: List[str]):
    """The added tokens' contents as the specs carry them: their UTF-8 bytes concatenated (one zero
    byte when there are none) and the n + 1 offsets ([] when there are none)."""
    added = [c.encode("utf-8") for c in contents]
    off = [0]
    for t in added:
        off.append(off[-1] + len(t))
    return np.frombuffer(b"".join(added) or b"\0", dtype=np.uint8).copy(), off if added else []


def _save_atomically(path: str, write) -> str:
    """``write(tmp)`` then rename onto ``path``: a concurrent reader never sees a partial file."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    tmp = f"{path}.{os.getpid()}.tmp"
    write(tmp)
    os.replace(tmp, path)
    return path


@dataclasses.dataclass
class BpeSpec:
    """Device tables of a byte-level, or SentencePiece-style character-level, BPE tokenizer
    (csrc/common/bpe.h DevBpe)."""
    byte_id: np.ndarray    # uint32 [256]
    keys: np.ndarray       # uint64 [mask + 1]
    vals: np.ndarray       # uint64 [mask + 1]
    mask: int
    added: np.ndarray      # uint8: added-token contents, concatenated
    added_off: List[int]   # [n_added + 1]
    post_add: int          # tokens the post-processor adds
    # the split-regex family (csrc/common/bpe_split.h); GPT-2 keeps the defaults
    kind: int = 0                          # BPE_GPT2 / BPE_SPLIT_A / BPE_SPLIT_B / BPE_CASE_C / BPE_CASE_D / BPE_SP
    ignore_merges: bool = False
    vslots: Optional[np.ndarray] = None    # uint64 [2 * (vmask + 1)]: the vocabulary's raw bytes, WpSlot pairs
    vmask: int = 0
    vpool: Optional[np.ndarray] = None     # uint8: the entries' raw bytes
    vlongest: int = 0                      # bytes of the longest entry
    nfc: bool = False                      # the normalizer is NFC: documents it may change come back -2
    # the SentencePiece-style family (kind BPE_SP, csrc/common/bpe_sp.h): byte_id holds the ids of <0xNN>
    sp_prepend: int = 0                    # SP_PREPEND_*: a U+2581 in front of the text
    sp_split: bool = False                 # a chunk starts at every space (Metaspace split), not only after a word
    sp_ascii: Optional[np.ndarray] = None  # uint32 [128]: id of each ASCII character, 0xFFFFFFFF = no entry
    sp_cp: Optional[np.ndarray] = None     # uint64 [sp_mask + 1]: (code point << 32 | id) of the other characters
    sp_mask: int = 0
    sp_id: int = 0                         # id of U+2581

    @property
    def sp_flags(self) -> int:
        return self.sp_prepend | (SP_SPLIT if self.sp_split else 0)


BPE_GPT2, BPE_SPLIT_A, BPE_SPLIT_B, BPE_CASE_C, BPE_CASE_D = 0, 1, 2, 3, 4  # csrc/common/bpe.h BpeKind
BPE_SP = 5  # SentencePiece-style character-level BPE with byte_fallback (csrc/common/bpe_sp.h)
SP_SPACE = "▁"  # "▁": what these tokenizers write for U+0020
SP_PREPEND_NONE, SP_PREPEND_ALWAYS, SP_PREPEND_UNLESS_SPACE, SP_SPLIT = 0, 1, 2, 4  # bpe.h BpeSpFlags
SPLIT_MAX_ADDED, SPLIT_MAX_ADDED_BYTES = 1024, 65536  # kBpeSplitMaxAdded, kBpeSplitMaxAddedBytes
# the Split patterns counted on the device: Llama-3 / cl100k_base, and the Qwen2 family
SPLIT_PATTERN_A = (r"(?i:'s|'t|'re|'ve|'m|'ll|'d)|[^\r\n\p{L}\p{N}]?\p{L}+|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n]*"
                   r"|\s*[\r\n]+|\s+(?!\S)|\s+")
SPLIT_PATTERN_B = SPLIT_PATTERN_A.replace(r"\p{N}{1,3}", r"\p{N}")
# the case-aware patterns (csrc/common/bpe_case.h): o200k_base, and Mistral's Tekken
SPLIT_PATTERN_C = (r"[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]*[\p{Ll}\p{Lm}\p{Lo}\p{M}]+(?i:'s|'t|'re|'ve|'m|'ll|'d)?"
                   r"|[^\r\n\p{L}\p{N}]?[\p{Lu}\p{Lt}\p{Lm}\p{Lo}\p{M}]+[\p{Ll}\p{Lm}\p{Lo}\p{M}]*(?i:'s|'t|'re|'ve|'m|'ll|'d)?"
                   r"|\p{N}{1,3}| ?[^\s\p{L}\p{N}]+[\r\n/]*|\s*[\r\n]+|\s+(?!\S)|\s+")
SPLIT_PATTERN_D = SPLIT_PATTERN_C.replace(r"(?i:'s|'t|'re|'ve|'m|'ll|'d)?", "").replace(r"\p{N}{1,3}", r"\p{N}")
SPLIT_PATTERNS = {"A": SPLIT_PATTERN_A, "B": SPLIT_PATTERN_B, "C": SPLIT_PATTERN_C, "D": SPLIT_PATTERN_D}


def _split_kind(pt) -> Optional[int]:
    """BPE_SPLIT_A / _B / BPE_CASE_C / _D when the pre-tokenizer is exactly Sequence[Split(Regex(A, B,
    C or D), Isolated), ByteLevel(add_prefix_space=false, use_regex=false)], else None."""
    if not isinstance(pt, dict) or pt.get("type") != "Sequence":
        return None
    pts = pt.get("pretokenizers") or []
    if len(pts) != 2 or any(not isinstance(q, dict) for q in pts):
        return None
    sp, bl = pts
    if sp.get("type") != "Split" or sp.get("behavior") != "Isolated" or sp.get("invert") is not False:
        return None
    if bl.get("type") != "ByteLevel" or bl.get("add_prefix_space") is not False or bl.get("use_regex") is not False:
        return None
    pat = sp.get("pattern")
    if not isinstance(pat, dict) or set(pat) != {"Regex"}:
        return None
    return {SPLIT_PATTERN_A: BPE_SPLIT_A, SPLIT_PATTERN_B: BPE_SPLIT_B, SPLIT_PATTERN_C: BPE_CASE_C,
            SPLIT_PATTERN_D: BPE_CASE_D}.get(pat["Regex"])


def _post_add(pp) -> Optional[int]:
    """Special tokens the post-processor adds to a single sequence, None if not known."""
    if pp is None:
        return 0
    t = pp.get("type")
    if t == "ByteLevel":
        return 0
    if t in ("RobertaProcessing", "BertProcessing"):
        return 2
    if t == "TemplateProcessing":
        n = 0
        for piece in pp.get("single", []):
            if "SpecialToken" in piece:
                sp = pp.get("special_tokens", {}).get(piece["SpecialToken"]["id"])
                if sp is None:
                    return None
                n += len(sp.get("ids", []))
            elif "Sequence" not in piece:
                return None
        return n
    if t == "Sequence":
        tot = 0
        for q in pp.get("processors", []):
            k = _post_add(q)
            if k is None:
                return None
            tot += k
        return tot
    return None


def _sp_layout(tj: dict):
    """(SP_PREPEND_*, split) when normalizer and pre-tokenizer are one of the two layouts of the
    SentencePiece-style family, else None: L = no pre-tokenizer behind Replace(" ", "▁") or
    Sequence[Prepend("▁"), Replace(" ", "▁")]; M = no normalizer, Metaspace("▁", prepend_scheme, split)."""
    nz, pt = tj.get("normalizer"), tj.get("pre_tokenizer")
    replace = {"type": "Replace", "pattern": {"String": " "}, "content": SP_SPACE}
    if pt is None:
        if nz == replace:
            return SP_PREPEND_NONE, False
        if nz == {"type": "Sequence", "normalizers": [{"type": "Prepend", "prepend": SP_SPACE}, replace]}:
            return SP_PREPEND_ALWAYS, False
        return None
    if nz is not None or not isinstance(pt, dict) or set(pt) != {"type", "replacement", "prepend_scheme", "split"}:
        return None
    if pt["type"] != "Metaspace" or pt["replacement"] != SP_SPACE or not isinstance(pt["split"], bool):
        return None
    # "first" is "always" here: a document with an added token's text, the only kind the library
    # cuts into sections, goes to the host
    prepend = {"always": SP_PREPEND_UNLESS_SPACE, "first": SP_PREPEND_UNLESS_SPACE,
               "never": SP_PREPEND_NONE}.get(pt["prepend_scheme"])
    return None if prepend is None else (prepend, pt["split"])


def _merge_pairs(m: dict, vocab: dict):
    """The merges as (left id, right id, rank, merged id) lists and their string pairs, None when an
    entry is malformed or names a string that is not in the vocabulary."""
    a, b, rank, nid, pairs = [], [], [], [], []
    for i, mg in enumerate(m.get("merges") or []):
        parts = mg.split(" ") if isinstance(mg, str) else mg
        if len(parts) != 2:
            return None
        x, y = parts
        if x not in vocab or y not in vocab or (x + y) not in vocab:
            return None
        a.append(vocab[x])
        b.append(vocab[y])
        rank.append(i)
        nid.append(vocab[x + y])
        pairs.append((x, y))
    return a, b, rank, nid, pairs


def _build_sp_spec(tj: dict, prepend: int, split: bool) -> Optional[BpeSpec]:
    """BpeSpec of kind BPE_SP for a character-level BPE with byte_fallback in layout L or M (see
    :func:`_sp_layout`), None when the device counter would not reproduce it: all 256 ``<0xNN>``
    tokens and ``▁`` must be in the vocabulary (``unk`` can then never appear), no ignore_merges,
    and without Metaspace's split no merge may join a piece that ends in another character than
    ``▁`` to one that starts with ``▁`` (then the merges of the whole text are those of its
    chunks ``▁* [^▁]*``, which is what the counter merges)."""
    from .. import native

    m = tj["model"]
    vocab = m.get("vocab") or {}
    if m.get("ignore_merges") or not isinstance(vocab, dict) or SP_SPACE not in vocab:
        return None
    byte_tokens = [f"<0x{b:02X}>" for b in range(256)]
    if any(t not in vocab for t in byte_tokens):
        return None
    post = _post_add(tj.get("post_processor"))
    mg = _merge_pairs(m, vocab)
    if post is None or mg is None:
        return None
    a, b, rank, nid, pairs = mg
    if not split and any(x and y and x[-1] != SP_SPACE and y[0] == SP_SPACE for x, y in pairs):
        return None
    toks = [t for t in tj.get("added_tokens") or [] if t.get("content")]
    # matched on normalised text: the same statement about the raw text only without a space in it
    if any(t.get("normalized") and (" " in t["content"] or SP_SPACE in t["content"]) for t in toks):
        return None
    added, off = _pack_added([t["content"] for t in toks])
    if len(toks) > SPLIT_MAX_ADDED or len(added) > SPLIT_MAX_ADDED_BYTES:
        return None
    h = native.host()
    keys, vals, mask = h.bpe_build_table(_u32(a), _u32(b), _u32(rank), _u32(nid))
    sp_ascii = np.full(128, 0xFFFFFFFF, dtype=np.uint32)
    cps, ids = [], []
    for s, i in vocab.items():
        if len(s) == 1:
            if ord(s) < 128:
                sp_ascii[ord(s)] = i
            else:
                cps.append(ord(s))
                ids.append(i)
    sp_cp, sp_mask = h.bpe_sp_build_table(_u32(cps), _u32(ids))
    spec = BpeSpec(_u32([vocab[t] for t in byte_tokens]), keys, vals, int(mask), added, off, post)
    spec.kind = BPE_SP
    spec.sp_prepend, spec.sp_split = prepend, split
    spec.sp_ascii, spec.sp_cp, spec.sp_mask, spec.sp_id = sp_ascii, sp_cp, int(sp_mask), int(vocab[SP_SPACE])
    return spec


def build_bpe_spec(tj: dict, nfc: bool = False) -> Optional[BpeSpec]:
    """BpeSpec of a parsed tokenizer.json, or None when the tokenizer is not a byte-level BPE the
    device counter reproduces exactly: plain BPE merges, no truncation / padding, a known
    post-processor, and as pre-tokenizer either GPT-2's ByteLevel regex without prefix space (no
    normalizer, at most MAX_ADDED added tokens, no ignore_merges) or Split(pattern A / B / C / D) +
    ByteLevel without regex (Llama-3, cl100k_base, Qwen2, o200k_base, Tekken: ignore_merges allowed, no byte_fallback, at most
    SPLIT_MAX_ADDED added tokens of SPLIT_MAX_ADDED_BYTES bytes together).

    A tokenizer with a normalizer has no spec, unless ``nfc`` is set (as :meth:`TokenCounterModel.bpe_spec`
    does): then a split-regex tokenizer whose normalizer is exactly ``{"type": "NFC"}`` and that has
    no added token matched on normalised text gets a spec with ``nfc`` on, whose counter returns -2
    for every document it cannot prove NFC leaves unchanged.

    A character-level BPE with ``byte_fallback`` in one of the SentencePiece-style layouts (Llama-2,
    Mistral, Gemma: :func:`_sp_layout`) gets a spec of kind BPE_SP under the conditions of
    :func:`_build_sp_spec`."""
    from .. import native

    m = tj.get("model") or {}
    if m.get("type") != "BPE" or m.get("dropout") not in (None, 0, 0.0) or m.get("continuing_subword_prefix") \
            or m.get("end_of_word_suffix"):
        return None
    if tj.get("truncation") is not None or tj.get("padding") is not None:
        return None
    if m.get("byte_fallback"):
        layout = _sp_layout(tj)
        if layout is not None:
            return _build_sp_spec(tj, *layout)
    pt = tj.get("pre_tokenizer")
    kind = _split_kind(pt)
    nz = tj.get("normalizer")
    if nz is not None and (not nfc or nz != {"type": "NFC"} or kind is None
                           or any(t.get("normalized") for t in tj.get("added_tokens") or [] if t.get("content"))):
        return None
    nfc = nz is not None
    if kind is None:
        kind = BPE_GPT2
        if m.get("ignore_merges"):
            return None
        if pt is not None and pt.get("type") == "Sequence" and len(pt.get("pretokenizers", [])) == 1:
            pt = pt["pretokenizers"][0]
        if pt is None or pt.get("type") != "ByteLevel" or pt.get("add_prefix_space") or not pt.get("use_regex", True):
            return None
    elif m.get("byte_fallback"):
        return None
    post = _post_add(tj.get("post_processor"))
    if post is None:
        return None
    vocab = m.get("vocab") or {}
    b2u = bytes_to_unicode()
    if any(ch not in vocab for ch in b2u):
        return None
    byte_id = np.array([vocab[ch] for ch in b2u], dtype=np.uint32)
    mg = _merge_pairs(m, vocab)
    if mg is None:
        return None
    a, b, rank, nid, _ = mg
    keys, vals, mask = native.host().bpe_build_table(_u32(a), _u32(b), _u32(rank), _u32(nid))
    contents = [t["content"] for t in tj.get("added_tokens") or [] if t.get("content")]
    if len(contents) > (MAX_ADDED if kind == BPE_GPT2 else SPLIT_MAX_ADDED):
        return None
    added, off = _pack_added(contents)
    spec = BpeSpec(byte_id, keys, vals, int(mask), added, off, post)
    if kind == BPE_GPT2:
        return spec
    if len(added) > SPLIT_MAX_ADDED_BYTES:
        return None
    spec.kind = kind
    spec.nfc = nfc
    spec.ignore_merges = bool(m.get("ignore_merges"))
    if spec.ignore_merges:
        # the vocabulary as raw bytes (entries with a character outside the byte-level alphabet
        # can never equal a pre-token)
        u2b = {ch: i for i, ch in enumerate(b2u)}
        entries = [bytes(u2b[ch] for ch in w) for w in vocab if w and all(ch in u2b for ch in w)]
        voff = np.zeros(len(entries) + 1, dtype=np.int64)
        np.cumsum([len(e) for e in entries], out=voff[1:])
        spec.vpool = np.frombuffer(b"".join(entries), dtype=np.uint8).copy()
        spec.vslots, vmask, longest = native.host().wp_build_table(spec.vpool, voff,
                                                                   np.zeros(len(entries), dtype=np.uint8))
        spec.vmask, spec.vlongest = int(vmask), int(longest)
    return spec


@dataclasses.dataclass
class WordPieceSpec:
    """Device tables of a WordPiece tokenizer (csrc/common/wordpiece.h DevWp)."""
    slots: np.ndarray      # uint64 [2 * (mask + 1)]: (key, value) pairs
    mask: int
    pool: np.ndarray       # uint8: piece bytes
    flags: int             # WP_LOWER | WP_CHINESE
    cls_shift: int         # class bits of wp_classes.inc: 0 clean_text, 2 not
    self_bit: int          # "normalises to itself" bit non-ASCII code points must carry, 0 = cased
    max_chars: int         # max_input_chars_per_word
    longest: int           # bytes of the longest piece
    added: np.ndarray      # uint8: added-token contents, concatenated
    added_off: List[int]   # [n_added + 1]
    post_add: int          # tokens the post-processor adds
    fold: int = 0          # fold tables of wp_fold.inc: 0 none, 1 lowercase, 2 strip_accents, 3 both


WP_LOWER, WP_CHINESE = 1, 2  # csrc/common/wordpiece.h kWpLower, kWpChinese


def build_wordpiece_spec(tj: dict, fold: bool = False) -> Optional[WordPieceSpec]:
    """WordPieceSpec of a parsed tokenizer.json, or None when the tokenizer is not a WordPiece model
    behind BertNormalizer + BertPreTokenizer that the device counter reproduces exactly (no
    truncation / padding, the unknown token in the vocabulary, a known post-processor, at most
    MAX_ADDED added tokens, none of them matched on normalised text).

    The identity spec (``fold`` false) leaves every document with a non-ASCII code point that
    ``lowercase`` / ``strip_accents`` change to the host. With ``fold`` the spec of a tokenizer that
    has either on names its mode's fold tables instead (k_wp_count_fold), and only the documents
    with a code point NFD may move go to the host; a cased tokenizer's spec is the same either way."""
    from .. import native

    m = tj.get("model") or {}
    nz, pt = tj.get("normalizer") or {}, tj.get("pre_tokenizer") or {}
    if m.get("type") != "WordPiece" or nz.get("type") != "BertNormalizer" or pt.get("type") != "BertPreTokenizer":
        return None
    if tj.get("truncation") is not None or tj.get("padding") is not None:
        return None
    vocab = m.get("vocab") or {}
    if not isinstance(vocab, dict) or m.get("unk_token") not in vocab:
        return None
    post = _post_add(tj.get("post_processor"))
    if post is None:
        return None
    toks = [t for t in tj.get("added_tokens") or [] if t.get("content")]
    if len(toks) > MAX_ADDED or any(t.get("normalized") for t in toks):
        return None
    max_chars = m.get("max_input_chars_per_word", 100)
    prefix = m.get("continuing_subword_prefix", "##")
    if not isinstance(max_chars, int) or not 0 <= max_chars < 2 ** 31 or not isinstance(prefix, str):
        return None
    lower = bool(nz.get("lowercase", True))
    strip = lower if nz.get("strip_accents") is None else bool(nz.get("strip_accents"))
    # pieces: every entry as a word-initial piece, and behind the prefix as a continuation
    pieces, cont = [], []
    for s in vocab:
        if s:
            pieces.append(s.encode("utf-8"))
            cont.append(0)
        if s.startswith(prefix) and len(s) > len(prefix):
            pieces.append(s[len(prefix):].encode("utf-8"))
            cont.append(1)
    if not pieces:
        return None
    off = np.zeros(len(pieces) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in pieces], out=off[1:])
    pool = np.frombuffer(b"".join(pieces), dtype=np.uint8).copy()
    slots, mask, longest = native.host().wp_build_table(pool, off, np.array(cont, dtype=np.uint8))
    added, aoff = _pack_added([t["content"] for t in toks])
    mode = (1 if lower else 0) | (2 if strip else 0) if fold else 0
    return WordPieceSpec(slots, int(mask), pool, (WP_LOWER if lower else 0) | (WP_CHINESE if nz.get(
        "handle_chinese_chars", True) else 0), 0 if nz.get("clean_text", True) else 2,
        0 if mode else {(False, False): 0, (True, False): 1 << 4, (False, True): 1 << 5,
                        (True, True): 1 << 6}[(lower, strip)],
        max_chars, int(longest), added, aoff, post, mode)


@dataclasses.dataclass
class UnigramSpec:
    """Device tables of a Unigram tokenizer (csrc/common/unigram.h DevUni)."""
    slots: np.ndarray      # uint64 [3 * (mask + 1)]: (key, value, f64 score bits) triples
    mask: int
    pool: np.ndarray       # uint8: piece bytes
    cls1: np.ndarray       # uint16 [0x110000 >> 7]: class table of this file's normalizer, stage 1
    cls2: np.ndarray       # uint8: stage 2, 32 bytes per block of 128 code points, 2 bits each
    sp: np.ndarray         # uint8: UTF-8 of the replacement character
    flags: int             # UNI_BYTE_FALLBACK
    unk_score: float       # min(score) - 10
    longest_cp: int        # code points of the longest piece
    longest: int           # bytes of the longest piece
    added: np.ndarray      # uint8: added-token contents and the unk piece's text, concatenated
    added_off: List[int]   # [n_added + 1]
    post_add: int          # tokens the post-processor adds
    layout: str = "H"      # "H" (hub files) or "C" (converted files): see build_unigram_spec
    # the replacements of the normalizer (build_unigram_spec(mapped=True)); empty: a spec without a map
    map1: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.uint16))     # uint16 [0x110000 >> 7]: block of map2
    map2: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.uint16))     # uint16, 128 per block: record or UNI_MAP_NONE
    map_rec: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.uint32))  # uint32: offset in map_pool << 8 | UNI_REC_JOIN | bytes
    map_pool: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.uint8))  # uint8: the outputs, white space as 0x20

    @property
    def mapped(self) -> bool:
        return len(self.map1) > 0


# csrc/common/unigram.h (pinned to the header's values by tests/test_unigram.py through UNI_CONSTANTS)
UNI_KEEP, UNI_SPACE, UNI_HOST, UNI_MAP = 0, 1, 2, 3
UNI_BYTE_FALLBACK = 1
UNI_MAX_PIECE_CP, UNI_MAX_PIECE_BYTES = 32, 128
UNI_MAX_MAP_BYTES = 32   # a replacement with more bytes leaves its code point to the host (nmt_nfkc: U+FDFA, 33)
UNI_MAP_NONE = 0xFFFF    # map2: the code point has no record
UNI_REC_LEN, UNI_REC_JOIN = 0x7F, 0x80  # map_rec: the length's bits; a space code point that joins the grapheme before it
# Rust's char::is_whitespace (White_Space): what WhitespaceSplit separates on and Strip removes
RUST_WHITESPACE = frozenset([*range(9, 14), 0x20, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F,
                             0x205F, 0x3000])
_UNI_SQUEEZE = {"Regex": " {2,}"}
_UNI_JOINERS = r"[\p{GCB=Extend}\p{GCB=ZWJ}\p{GCB=SpacingMark}\p{GCB=Prepend}\p{GCB=L}\p{GCB=V}\p{GCB=T}]"


def _metaspace(pt, schemes) -> bool:
    """Is ``pt`` Metaspace("▁", a prepend scheme of ``schemes``, split true), in today's or the older
    serialisation (add_prefix_space)?"""
    if not isinstance(pt, dict) or pt.get("type") != "Metaspace" or pt.get("replacement") != SP_SPACE:
        return False
    if set(pt) - {"type", "replacement", "prepend_scheme", "split", "add_prefix_space", "str_rep"}:
        return False
    if pt.get("str_rep", SP_SPACE) != SP_SPACE or pt.get("add_prefix_space", True) is not True:
        return False
    return pt.get("prepend_scheme", "always") in schemes and pt.get("split", True) is True


def _unigram_layout(tj: dict):
    """(layout, charsmap as base64 or None) when normalizer and pre-tokenizer are one of the two
    layouts of :func:`build_unigram_spec`, else None."""
    nz, pt = tj.get("normalizer"), tj.get("pre_tokenizer")
    if not isinstance(nz, dict) or nz.get("type") != "Sequence" or not isinstance(pt, dict):
        return None
    seq = list(nz.get("normalizers") or [])
    charsmap = None
    if seq and isinstance(seq[0], dict) and seq[0].get("type") == "Precompiled":
        charsmap = seq.pop(0).get("precompiled_charsmap")
        if not isinstance(charsmap, str) or not charsmap:
            return None
    if seq == [{"type": "Replace", "pattern": _UNI_SQUEEZE, "content": " "}]:
        pts = pt.get("pretokenizers") or []
        if (pt.get("type") == "Sequence" and len(pts) == 2 and pts[0] == {"type": "WhitespaceSplit"}
                and _metaspace(pts[1], ("always",))):
            return "H", charsmap
        return None
    if seq == [{"type": "Strip", "strip_left": False, "strip_right": True},
               {"type": "Replace", "pattern": _UNI_SQUEEZE, "content": SP_SPACE}]:
        # "first" is "always" here: a document with an added token's text, the only kind the library
        # cuts into sections, goes to the host
        return ("C", charsmap) if _metaspace(pt, ("always", "first")) else None
    return None


def _two_stage_2bit(cls: np.ndarray):
    """A class per code point (uint8 [0x110000], values 0..3) as DevUni's two-stage table."""
    packed = cls.reshape(-1, 4)
    packed = (packed[:, 0] | (packed[:, 1] << 2) | (packed[:, 2] << 4) | (packed[:, 3] << 6)).astype(np.uint8)
    blocks, inverse = np.unique(packed.reshape(-1, 32), axis=0, return_inverse=True)
    return inverse.reshape(-1).astype(np.uint16), np.ascontiguousarray(blocks.reshape(-1))


def unigram_probe(charsmap: Optional[str]) -> List[Optional[str]]:
    """What the file's Precompiled normalizer makes of every scalar value on its own (None for the
    surrogates); without a charsmap every code point normalises to itself."""
    if charsmap is None:
        return [None if 0xD800 <= c < 0xE000 else chr(c) for c in range(0x110000)]
    import base64

    from tokenizers import normalizers

    f = normalizers.Precompiled(base64.b64decode(charsmap)).normalize_str
    return [None if 0xD800 <= c < 0xE000 else f(chr(c)) for c in range(0x110000)]


def unigram_classes(charsmap: Optional[str], layout: str) -> np.ndarray:
    """UNI_KEEP / UNI_SPACE / UNI_HOST of every code point for a normalizer and a layout (about 1 s).

    keep: the normalizer leaves the code point as it is. space: it becomes exactly U+0020, it is
    U+0020, or (layout H) it is kept white space, which WhitespaceSplit separates on. host: the
    rest - dropped or replaced code points, kept white space in layout C (Strip and embedded white
    space are no spaces there), a kept U+2581, and behind Precompiled every code point that can
    share a grapheme with a neighbour (Grapheme_Cluster_Break Extend, ZWJ, SpacingMark, Prepend, L,
    V, T; the combining marks and unassigned code points of Python's own Unicode data): Precompiled looks a whole grapheme
    under 6 bytes up and replaces all of it by the shortest matching prefix's output."""
    out = unigram_probe(charsmap)
    cls = np.full(0x110000, UNI_HOST, dtype=np.uint8)
    for c, o in enumerate(out):
        if o == " " or c == 0x20:
            cls[c] = UNI_SPACE
        elif o is not None and o == chr(c) and c != 0x2581:
            if c in RUST_WHITESPACE:
                cls[c] = UNI_SPACE if layout == "H" else UNI_HOST
            else:
                cls[c] = UNI_KEEP
    if charsmap is not None:
        cls[_unigram_joiners() & (cls == UNI_KEEP)] = UNI_HOST
    return cls


def _unigram_joiners() -> np.ndarray:
    """bool [0x110000]: the code points that can share a grapheme with a neighbour. The library's
    segmentation may know a newer Unicode than any one source here: the union of ICU's property,
    Python's combining marks and unassigned code points, and the regex module's property where it
    is installed."""
    import unicodedata

    from .. import native

    joiner = native.host().uni_grapheme_joiners().astype(bool)
    for c in range(0x80, 0x110000):
        if unicodedata.category(chr(c)) in ("Mn", "Me", "Mc", "Cn"):
            joiner[c] = True
    try:
        import regex
    except ImportError:
        regex = None
    if regex is not None:
        text = "".join(chr(c) for c in range(0x110000) if not 0xD800 <= c < 0xE000)
        for hit in regex.finditer(_UNI_JOINERS, text):
            joiner[ord(hit.group())] = True
    return joiner


def unigram_map(charsmap: Optional[str], layout: str):
    """(cls, outputs, joins): :func:`unigram_classes` with UNI_MAP for the host code points whose
    replacement the device counter applies itself, code point -> the replacement's bytes as the
    counter reads them (white space as 0x20; empty: the code point is dropped), and the space code
    points that are grapheme joiners (U+200C behind nmt_nfkc). Precompiled looks a whole grapheme
    under 6 bytes up and replaces all of it by its first code point's output, so a map code point
    swallows such a joiner: the counter hands a document with that pair to the host.

    A host code point becomes UNI_MAP when it is no surrogate and no grapheme joiner, its output on
    its own differs from it, has at most UNI_MAX_MAP_BYTES bytes and no U+2581, every white-space
    code point of the output separates words in the layout (H: any, C: U+0020 only, as for kept
    white space), and between two letters the normalizer gives the same output: the code point is a
    grapheme of its own. The output's code points are not classified again: the library neither
    segments nor normalises them a second time, so they are word text, or 0x20."""
    cls = unigram_classes(charsmap, layout)
    outputs = {}
    if charsmap is None:
        return cls, outputs, []
    import base64

    from tokenizers import normalizers

    f = normalizers.Precompiled(base64.b64decode(charsmap)).normalize_str
    joiner = _unigram_joiners()
    for c in np.nonzero((cls == UNI_HOST) & ~joiner)[0].tolist():
        if 0xD800 <= c < 0xE000:
            continue
        o = f(chr(c))
        if o == chr(c) or SP_SPACE in o or len(o.encode("utf-8")) > UNI_MAX_MAP_BYTES:
            continue
        white = [x for x in o if ord(x) in RUST_WHITESPACE]
        if layout != "H" and any(x != " " for x in white):
            continue
        if f("a" + chr(c) + "b") != "a" + o + "b":
            continue
        cls[c] = UNI_MAP
        outputs[c] = "".join(" " if ord(x) in RUST_WHITESPACE else x for x in o).encode("utf-8")
    return cls, outputs, np.nonzero((cls == UNI_SPACE) & joiner)[0].tolist()


def _two_stage_map(outputs: dict, joins=()):
    """code point -> bytes as UnigramSpec's map1, map2, map_rec, map_pool; equal outputs share a
    record, and the code points of ``joins`` one that is UNI_REC_JOIN. Both of the last two hold
    one entry at least, so that every table has an address."""
    recs, pool, index = [], bytearray(), np.full(0x110000, UNI_MAP_NONE, dtype=np.uint16)
    seen = {}
    if len(joins):
        recs.append(UNI_REC_JOIN)
        index[np.asarray(joins, dtype=np.int64)] = 0
    for c in sorted(outputs):
        o = outputs[c]
        if o not in seen:
            if len(recs) >= UNI_MAP_NONE:
                raise ValueError("unigram map: more replacements than map2 can name")
            seen[o] = len(recs)
            recs.append((len(pool) << 8) | len(o))
            pool += o
        index[c] = seen[o]
    blocks, inverse = np.unique(index.reshape(-1, 128), axis=0, return_inverse=True)
    # block 0 of np.unique is not the empty one in general; any order serves the lookup
    return (inverse.reshape(-1).astype(np.uint16), np.ascontiguousarray(blocks.reshape(-1)),
            np.array(recs or [0], dtype=np.uint32), np.frombuffer(bytes(pool) or b"\0", dtype=np.uint8).copy())


def _unigram_map_table(charsmap: Optional[str], layout: str, cache_dir: Optional[str]):
    """(cls1, cls2, map1, map2, map_rec, map_pool) of a mapped spec, from the cache file next to
    the tokenizer when there is one (a file of its own: unigram_classes.*.npz stays as it is)."""
    import hashlib

    names = ("cls1", "cls2", "map1", "map2", "map_rec", "map_pool")
    kinds = (np.uint16, np.uint8, np.uint16, np.uint16, np.uint32, np.uint8)
    key = hashlib.sha256(f"m2:{UNI_MAX_MAP_BYTES}:{layout}:{charsmap or ''}".encode("utf-8")).hexdigest()[:16]
    path = os.path.join(cache_dir, f"unigram_map.{key}.npz") if cache_dir else None
    if path and os.path.isfile(path):
        try:
            with np.load(path) as z:
                t = tuple(z[n].astype(k) for n, k in zip(names, kinds))
            if (t[0].shape == t[2].shape == (0x110000 >> 7,) and (int(t[0].max()) + 1) * 32 <= len(t[1])
                    and (int(t[2].max()) + 1) * 128 <= len(t[3]) and len(t[4]) and len(t[5])):
                return t  # the parameter block's validator checks the records
        except (OSError, ValueError, KeyError):
            pass
    cls, outputs, joins = unigram_map(charsmap, layout)
    t = _two_stage_2bit(cls) + _two_stage_map(outputs, joins)
    if path:
        def write(tmp):
            with open(tmp, "wb") as f:
                np.savez_compressed(f, **dict(zip(names, t)))

        try:
            _save_atomically(path, write)
        except OSError:
            pass  # a read-only tokenizer directory: probed again next time
    return t


def _unigram_class_table(charsmap: Optional[str], layout: str, cache_dir: Optional[str]):
    """The two-stage class table, from the cache file next to the tokenizer when there is one."""
    import hashlib

    key = hashlib.sha256(f"v2:{layout}:{charsmap or ''}".encode("utf-8")).hexdigest()[:16]
    path = os.path.join(cache_dir, f"unigram_classes.{key}.npz") if cache_dir else None
    if path and os.path.isfile(path):
        try:
            with np.load(path) as z:
                c1, c2 = z["cls1"].astype(np.uint16), z["cls2"].astype(np.uint8)
            if c1.shape == (0x110000 >> 7,) and c2.ndim == 1 and (int(c1.max()) + 1) * 32 <= len(c2):
                return c1, c2
        except (OSError, ValueError, KeyError):
            pass
    c1, c2 = _two_stage_2bit(unigram_classes(charsmap, layout))
    if path:
        def write(tmp):
            with open(tmp, "wb") as f:
                np.savez_compressed(f, cls1=c1, cls2=c2)

        try:
            _save_atomically(path, write)
        except OSError:
            pass  # a read-only tokenizer directory: probed again next time
    return c1, c2


def build_unigram_spec(tj: dict, cache_dir: Optional[str] = None, mapped: bool = False) -> Optional[UnigramSpec]:
    """UnigramSpec of a parsed tokenizer.json, or None when the tokenizer is not a Unigram model the
    device counter reproduces exactly: ``unk_id`` set, no duplicate pieces, finite scores, with
    ``byte_fallback`` all 256 ``<0xNN>`` pieces, no truncation / padding, a known post-processor, at
    most SPLIT_MAX_ADDED added tokens of SPLIT_MAX_ADDED_BYTES bytes in all, none matched on
    normalised text, no piece over UNI_MAX_PIECE_CP code points / UNI_MAX_PIECE_BYTES bytes, and
    normalizer and pre-tokenizer in one of two layouts:

    * H (the hub files of T5 / mT5 / XLM-R): normalizer Sequence[Precompiled?, Replace(Regex " {2,}" -> " ")],
      pre-tokenizer Sequence[WhitespaceSplit, Metaspace("▁", prepend always)];
    * C (what transformers' SpmConverter writes): normalizer Sequence[Precompiled?, Strip(right),
      Replace(Regex " {2,}" -> "▁")], pre-tokenizer Metaspace("▁", prepend always or first, split).

    In both the count of a document is the sum over its words, each encoded as "▁" + word. The
    class table comes from probing the file's own Precompiled normalizer (:func:`unigram_classes`)
    and is cached in ``cache_dir``.

    ``mapped``: the spec also carries the normalizer's replacements (:func:`unigram_map`; class
    UNI_MAP in the table, ``map1`` / ``map2`` / ``map_rec`` / ``map_pool``), and the counter applies
    them instead of handing the document to the host (k_uni_count_map)."""
    import math

    from .. import native

    m = tj.get("model") or {}
    if m.get("type") != "Unigram" or tj.get("truncation") is not None or tj.get("padding") is not None:
        return None
    lay = _unigram_layout(tj)
    post = _post_add(tj.get("post_processor"))
    vocab, unk_id = m.get("vocab"), m.get("unk_id")
    if lay is None or post is None or not isinstance(vocab, list) or not vocab:
        return None
    if not isinstance(unk_id, int) or isinstance(unk_id, bool) or not 0 <= unk_id < len(vocab):
        return None
    try:
        pieces = [p.encode("utf-8") for p, _ in vocab]
        scores = np.array([float(s) for _, s in vocab], dtype=np.float64)
    except (TypeError, ValueError, AttributeError, UnicodeEncodeError):
        return None
    if len(set(pieces)) != len(pieces) or b"" in pieces or not np.isfinite(scores).all():
        return None
    unk_score = float(scores.min()) - 10.0
    # a run of unknowns must lose against any piece that spells it (else byte_fallback would see a
    # known string): k (min - 10) < min for every k >= 2
    if not unk_score < 0.0:
        return None
    byte_fallback = bool(m.get("byte_fallback", False))
    if byte_fallback and not {f"<0x{b:02X}>".encode() for b in range(256)} <= set(pieces):
        return None
    longest = max(len(p) for p in pieces)
    longest_cp = max(len(p) for p, _ in vocab)
    if longest_cp > UNI_MAX_PIECE_CP or longest > UNI_MAX_PIECE_BYTES:
        return None
    toks = [t for t in tj.get("added_tokens") or [] if t.get("content")]
    if any(t.get("normalized") for t in toks):
        return None
    contents = [t["content"] for t in toks]
    if vocab[unk_id][0] not in contents:  # the unk piece's own text: one more added-token string
        contents.append(vocab[unk_id][0])
    added, aoff = _pack_added(contents)
    if len(contents) > SPLIT_MAX_ADDED or len(added) > SPLIT_MAX_ADDED_BYTES:
        return None
    layout, charsmap = lay
    maps = ()
    try:
        if mapped:
            cls1, cls2, *maps = _unigram_map_table(charsmap, layout, cache_dir)
        else:
            cls1, cls2 = _unigram_class_table(charsmap, layout, cache_dir)
    except Exception:  # noqa: BLE001 - a charsmap the library does not read
        return None
    off = np.zeros(len(pieces) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in pieces], out=off[1:])
    pool = np.frombuffer(b"".join(pieces), dtype=np.uint8).copy()
    slots, mask = native.host().uni_build_table(pool, off, scores, unk_id)
    assert math.isfinite(unk_score)
    return UnigramSpec(slots, int(mask), pool, cls1, cls2, np.frombuffer(SP_SPACE.encode("utf-8"), dtype=np.uint8).copy(),
                       UNI_BYTE_FALLBACK if byte_fallback else 0, unk_score, longest_cp, longest, added, aoff, post,
                       layout, *maps)


class TokenCounterModel:
    def __init__(self, path: str):
        from tokenizers import Tokenizer

        self.path = path
        self.tok = Tokenizer.from_file(path)
        self._spec = False
        self._wp_spec = False
        self._wp_fold_spec = False
        self._uni_spec = False
        self._uni_map_spec = False

    def count(self, texts: List[str]) -> List[int]:
        if not texts:
            return []
        encs = self.tok.encode_batch(texts, add_special_tokens=True)
        return [len(e.tokens) for e in encs]

    def bpe_spec(self) -> Optional[BpeSpec]:
        """Device/native tables when this is a byte-level BPE tokenizer (else None; behind an NFC
        normalizer the spec of the NFC gate); built once."""
        if self._spec is False:
            with open(self.path, encoding="utf-8") as f:
                self._spec = build_bpe_spec(json.load(f), nfc=True)
        return self._spec

    def wordpiece_spec(self) -> Optional[WordPieceSpec]:
        """Device/native tables when this is a BERT-style WordPiece tokenizer (else None); built once."""
        if self._wp_spec is False:
            with open(self.path, encoding="utf-8") as f:
                self._wp_spec = build_wordpiece_spec(json.load(f))
        return self._wp_spec

    def wordpiece_fold_spec(self) -> Optional[WordPieceSpec]:
        """:meth:`wordpiece_spec` with the fold tables of the tokenizer's ``lowercase`` /
        ``strip_accents`` mode (the same spec for a cased tokenizer); built once."""
        if self._wp_fold_spec is False:
            ident = self.wordpiece_spec()
            if ident is None or ident.self_bit == 0:
                self._wp_fold_spec = ident
            else:
                with open(self.path, encoding="utf-8") as f:
                    self._wp_fold_spec = build_wordpiece_spec(json.load(f), fold=True)
        return self._wp_fold_spec

    def unigram_spec(self) -> Optional[UnigramSpec]:
        """Device/native tables when this is a Unigram tokenizer in one of the counted layouts (else
        None); built once, its class table cached next to the tokenizer file."""
        if self._uni_spec is False:
            with open(self.path, encoding="utf-8") as f:
                self._uni_spec = build_unigram_spec(json.load(f), os.path.dirname(os.path.abspath(self.path)))
        return self._uni_spec

    def unigram_map_spec(self) -> Optional[UnigramSpec]:
        """:meth:`unigram_spec` with the normalizer's replacements for the counter to apply
        (``build_unigram_spec(mapped=True)``); built once, its tables cached next to the tokenizer
        file."""
        if self._uni_map_spec is False:
            with open(self.path, encoding="utf-8") as f:
                self._uni_map_spec = build_unigram_spec(json.load(f), os.path.dirname(os.path.abspath(self.path)),
                                                        mapped=True)
        return self._uni_map_spec

    def device_spec(self, uni_map: bool = False):
        """The spec the device path counts with: :class:`BpeSpec`, :class:`WordPieceSpec` (folding
        when the tokenizer lowercases or strips accents), :class:`UnigramSpec` (``uni_map``: the one
        with the normalizer's replacements, DeviceTuning.uni_map) or None."""
        sp = self.bpe_spec() or self.wordpiece_fold_spec()
        if sp is None and uni_map:
            return self.unigram_map_spec()
        return sp or self.unigram_spec()

    def count_native(self, data: np.ndarray, off: np.ndarray, nthreads: int = 8) -> np.ndarray:
        """Token counts of packed UTF-8 documents with the native counter of whichever spec the
        tokenizer has (host emulation of k_bpe_count / k_wp_count / k_uni_count); documents it returns -2 for
        (added-token text, invalid UTF-8, BPE pre-tokens or SentencePiece-style chunks over 2048 bytes, text that an NFC normalizer
        may change, WordPiece text with a code point whose place NFD may change under strip_accents, Unigram text
        with a code point its normalizer changes or the unk piece's own text) are counted by ``tokenizers``."""
        from .. import native

        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, np.int64)
        sp = self.device_spec()
        if sp is None:
            raise Unexpected("count_native needs a byte-level BPE, a WordPiece or a Unigram tokenizer")
        out = count_spec(sp, data, off, nthreads).astype(np.int64)
        bad = np.nonzero(out < 0)[0]
        if len(bad):
            out[bad] = self.count([bytes(data[off[k]:off[k + 1]]).decode("utf-8", "replace") for k in bad.tolist()])
        return out


def count_spec(sp, data: np.ndarray, off: np.ndarray, nthreads: int = 8, chunk: int = 0) -> np.ndarray:
    """The native counter's raw result (int32 counts, -2 = count on the host) for any kind of
    spec; ``chunk`` > 0 counts each chunk-byte range on its own, as the kernels' lanes do."""
    from .. import native

    h = native.host()
    fn = h.wp_count if isinstance(sp, WordPieceSpec) else (h.uni_count if isinstance(sp, UnigramSpec) else h.bpe_count)
    return fn(data, off, sp, nthreads, chunk)


def train_synthetic_wordpiece(path: str, vocab_size: int = 30522, n_docs: int = 20000, seed: int = 1,
                              lowercase: bool = False, strip_accents: Optional[bool] = None) -> str:
    """Train a BERT-format WordPiece tokenizer (BertNormalizer, BertPreTokenizer, ``[CLS] $A [SEP]``
    template, the five BERT special tokens, ``vocab_size`` entries) on the synthetic Zipf corpus
    and save it as ``path`` (kept if it already exists): the stand-in for bert-base-cased /
    -uncased, which cannot be downloaded here."""
    if os.path.isfile(path):
        return path
    from tokenizers import Tokenizer, decoders, models, normalizers, pre_tokenizers, processors, trainers

    from ..utils import synth

    texts = synth.make_corpus(n_docs, 1024, seed=seed, vocab="zipf")
    tok = Tokenizer(models.WordPiece(unk_token="[UNK]"))
    tok.normalizer = normalizers.BertNormalizer(clean_text=True, handle_chinese_chars=True, strip_accents=strip_accents,
                                                lowercase=lowercase)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    tok.decoder = decoders.WordPiece(prefix="##")
    special = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    tr = trainers.WordPieceTrainer(vocab_size=vocab_size, special_tokens=special, show_progress=False)
    tok.train_from_iterator(texts, tr)
    tok.post_processor = processors.TemplateProcessing(
        single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] $B:1 [SEP]:1",
        special_tokens=[("[CLS]", tok.token_to_id("[CLS]")), ("[SEP]", tok.token_to_id("[SEP]"))])
    return _save_atomically(path, tok.save)


def train_synthetic_bpe(path: str, vocab_size: int = 50257, n_docs: int = 20000, seed: int = 1) -> str:
    """Train a GPT-2-format byte-level BPE tokenizer (ByteLevel pre-tokenizer and post-processor,
    ``<|endoftext|>`` special token, ``vocab_size`` entries) on the synthetic Zipf corpus and save
    it as ``path`` (kept if it already exists). There is no network for the real gpt2 files: this
    stands in for them with the same model type, pre-tokenizer and vocabulary size; the token
    counts differ from real GPT-2, the work per byte is of the same kind."""
    if os.path.isfile(path):
        return path
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers

    from ..utils import synth

    texts = synth.make_corpus(n_docs, 1024, seed=seed, vocab="zipf")
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    tok.post_processor = processors.ByteLevel(trim_offsets=False)
    tr = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=["<|endoftext|>"], show_progress=False,
                             initial_alphabet=pre_tokenizers.ByteLevel.alphabet())
    tok.train_from_iterator(texts, tr)
    return _save_atomically(path, tok.save)


def train_synthetic_split_bpe(path: str, vocab_size: int = 32000, pattern: str = "A", ignore_merges: bool = True,
                              n_added: int = 256, n_docs: int = 20000, seed: int = 1, nfc: bool = False) -> str:
    """Train a Llama-3-format byte-level BPE tokenizer on the synthetic Zipf corpus and save it as
    ``path`` (kept if it already exists): pre-tokenizer Sequence[Split(pattern A, B, C or D, Isolated),
    ByteLevel(use_regex=false)], post-processor Sequence[ByteLevel, TemplateProcessing] that puts
    ``<|begin_of_text|>`` in front, ``ignore_merges`` as given, and ``n_added`` added tokens
    (``<|begin_of_text|>``, ``<|end_of_text|>`` and reserved specials) after the ``vocab_size``
    model entries, as Llama-3 lays them out; ``nfc`` adds the NFC normalizer of the Qwen2 files. The stand-in for Llama-3 / cl100k_base / Qwen2, which
    cannot be downloaded here; the counts differ from theirs, the work per byte is of the same kind."""
    if os.path.isfile(path):
        return path
    from tokenizers import Regex, Tokenizer, decoders, models, normalizers, pre_tokenizers, processors, trainers

    from ..utils import synth

    pat = SPLIT_PATTERNS[pattern]
    texts = synth.make_corpus(n_docs, 1024, seed=seed, vocab="zipf")
    tok = Tokenizer(models.BPE(ignore_merges=ignore_merges))
    if nfc:
        tok.normalizer = normalizers.NFC()
    tok.pre_tokenizer = pre_tokenizers.Sequence([
        pre_tokenizers.Split(Regex(pat), behavior="isolated", invert=False),
        pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)])
    tok.decoder = decoders.ByteLevel()
    tr = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=[], show_progress=False,
                             initial_alphabet=pre_tokenizers.ByteLevel.alphabet())
    tok.train_from_iterator(texts, tr)
    special = ["<|begin_of_text|>", "<|end_of_text|>"][:n_added]
    special += [f"<|reserved_special_token_{i}|>" for i in range(n_added - len(special))]
    tok.add_special_tokens(special)
    procs = [processors.ByteLevel(trim_offsets=False)]
    if special:
        procs.append(processors.TemplateProcessing(
            single="<|begin_of_text|> $A", pair="<|begin_of_text|> $A <|begin_of_text|>:1 $B:1",
            special_tokens=[("<|begin_of_text|>", tok.token_to_id("<|begin_of_text|>"))]))
    tok.post_processor = processors.Sequence(procs)
    return _save_atomically(path, tok.save)


_SP_SPECIAL = ["<unk>", "<s>", "</s>"]
_sp_trained: dict = {}  # (vocab_size, n_docs, seed) -> serialised tokenizer: the layouts share one training run


def _train_sp_base(vocab_size: int, n_docs: int, seed: int) -> dict:
    key = (vocab_size, n_docs, seed)
    if key not in _sp_trained:
        from tokenizers import Tokenizer, models, pre_tokenizers, trainers

        from ..utils import synth

        texts = synth.make_corpus(n_docs, 1024, seed=seed, vocab="zipf")
        tok = Tokenizer(models.BPE(unk_token="<unk>"))
        tok.pre_tokenizer = pre_tokenizers.Metaspace(replacement=SP_SPACE, prepend_scheme="always", split=True)
        tr = trainers.BpeTrainer(vocab_size=vocab_size, show_progress=False,
                                 special_tokens=_SP_SPECIAL + [f"<0x{b:02X}>" for b in range(256)])
        tok.train_from_iterator(texts, tr)
        _sp_trained[key] = tok.to_str()
    return json.loads(_sp_trained[key])


def train_synthetic_sp_bpe(path: str, vocab_size: int = 32000, layout: str = "L", prepend: bool = True,
                           prepend_scheme: str = "first", split: bool = True, n_docs: int = 20000,
                           seed: int = 1) -> str:
    """Train a SentencePiece-style character-level BPE tokenizer on the synthetic Zipf corpus and
    save it as ``path`` (kept if it already exists): trained behind Metaspace(split=true) with
    ``<unk>``, ``<s>``, ``</s>`` and the 256 ``<0xNN>`` byte tokens in front of the vocabulary, then
    written with ``byte_fallback`` and ``fuse_unk`` on, a template that puts ``<s>`` in front, and

    * ``layout="L"`` (Llama-2, Mistral, Gemma): normalizer Sequence[Prepend("▁"), Replace(" ", "▁")]
      (``prepend`` false: the Replace alone), no pre-tokenizer;
    * ``layout="M"``: no normalizer, pre-tokenizer Metaspace("▁", ``prepend_scheme``, ``split``).

    The stand-in for the files of those models, which cannot be downloaded here; the counts differ
    from theirs, the work per byte is of the same kind."""
    if os.path.isfile(path):
        return path
    if layout not in ("L", "M") or prepend_scheme not in ("always", "first", "never"):
        raise ValueError("train_synthetic_sp_bpe: layout is L or M, prepend_scheme always, first or never")
    from tokenizers import Tokenizer

    tj = _train_sp_base(vocab_size, n_docs, seed)
    # the byte tokens are plain vocabulary entries, as the SentencePiece conversions have them
    tj["added_tokens"] = [t for t in tj["added_tokens"] if t["content"] in _SP_SPECIAL]
    tj["model"].update(byte_fallback=True, fuse_unk=True, unk_token="<unk>", ignore_merges=False)
    replace = {"type": "Replace", "pattern": {"String": " "}, "content": SP_SPACE}
    if layout == "L":
        tj["normalizer"] = ({"type": "Sequence", "normalizers": [{"type": "Prepend", "prepend": SP_SPACE}, replace]}
                            if prepend else replace)
        tj["pre_tokenizer"] = None
    else:
        tj["normalizer"] = None
        tj["pre_tokenizer"] = {"type": "Metaspace", "replacement": SP_SPACE, "prepend_scheme": prepend_scheme,
                               "split": split}
    bos = tj["model"]["vocab"]["<s>"]
    tj["post_processor"] = {
        "type": "TemplateProcessing",
        "single": [{"SpecialToken": {"id": "<s>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}}],
        "pair": [{"SpecialToken": {"id": "<s>", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}},
                 {"SpecialToken": {"id": "<s>", "type_id": 1}}, {"Sequence": {"id": "B", "type_id": 1}}],
        "special_tokens": {"<s>": {"id": "<s>", "ids": [bos], "tokens": ["<s>"]}}}
    tj["decoder"] = {"type": "Sequence", "decoders": [
        {"type": "Replace", "pattern": {"String": SP_SPACE}, "content": " "}, {"type": "ByteFallback"},
        {"type": "Fuse"}]}
    Tokenizer.from_str(json.dumps(tj))  # the library reads what was written
    def write(tmp):
        with open(tmp, "w", encoding="utf-8") as f:
            json.dump(tj, f, ensure_ascii=False)

    return _save_atomically(path, write)


_UNI_SPECIAL = ["<pad>", "</s>", "<unk>"]  # ids 0, 1, 2, as T5 has them
_uni_trained: dict = {}  # (vocab_size, rule, byte_fallback, n_docs, seed) -> (pieces, charsmap): layouts share a run


def _train_unigram_base(vocab_size: int, rule: str, byte_fallback: bool, n_docs: int, seed: int):
    key = (vocab_size, rule, byte_fallback, n_docs, seed)
    if key not in _uni_trained:
        import io

        import sentencepiece as spm
        from sentencepiece import sentencepiece_model_pb2 as pb

        from ..utils import synth

        texts = synth.make_corpus(n_docs, 1024, seed=seed, vocab="zipf")
        lines = [ln for t in texts for ln in t.split("\n") if ln.strip()]
        buf = io.BytesIO()
        spm.SentencePieceTrainer.train(
            sentence_iterator=iter(lines), model_writer=buf, vocab_size=vocab_size, model_type="unigram",
            normalization_rule_name=rule, byte_fallback=byte_fallback, hard_vocab_limit=False, pad_id=0, eos_id=1,
            unk_id=2, bos_id=-1, pad_piece="<pad>", eos_piece="</s>", unk_piece="<unk>", num_threads=4,
            max_sentence_length=1 << 20, minloglevel=2)
        mp = pb.ModelProto()
        mp.ParseFromString(buf.getvalue())
        _uni_trained[key] = ([(p.piece, float(p.score)) for p in mp.pieces],
                             bytes(mp.normalizer_spec.precompiled_charsmap))
    return _uni_trained[key]


def train_synthetic_unigram(path: str, vocab_size: int = 32000, layout: str = "H", rule: str = "nmt_nfkc",
                            byte_fallback: bool = False, prepend_scheme: str = "always", n_docs: int = 20000,
                            seed: int = 1) -> str:
    """Train a Unigram tokenizer with ``sentencepiece`` on the synthetic Zipf corpus and save it as
    ``path`` (kept if it already exists), written as the T5 / mT5 / XLM-R files are: ``<pad>``,
    ``</s>``, ``<unk>`` in front of the vocabulary and registered as added tokens, a template that
    puts ``</s>`` behind the text, the trained model's ``precompiled_charsmap`` of normalisation
    rule ``rule`` (``nmt_nfkc``, ``nfkc``; ``identity`` has none) in a Precompiled normalizer, and

    * ``layout="H"`` (the hub files): normalizer Sequence[Precompiled, Replace(Regex " {2,}" -> " ")],
      pre-tokenizer Sequence[WhitespaceSplit, Metaspace("▁", always)];
    * ``layout="C"`` (transformers' SpmConverter): normalizer Sequence[Precompiled, Strip(right),
      Replace(Regex " {2,}" -> "▁")], pre-tokenizer Metaspace("▁", ``prepend_scheme``, split).

    The stand-in for the files of those models, which cannot be downloaded here; the counts differ
    from theirs, the work per byte is of the same kind."""
    if os.path.isfile(path):
        return path
    if layout not in ("H", "C") or rule not in ("nmt_nfkc", "nfkc", "identity") or prepend_scheme not in ("always", "first"):
        raise ValueError("train_synthetic_unigram: layout is H or C, rule nmt_nfkc, nfkc or identity, "
                         "prepend_scheme always or first")
    import base64

    from tokenizers import Tokenizer

    pieces, charsmap = _train_unigram_base(vocab_size, rule, byte_fallback, n_docs, seed)
    ids = {p: i for i, (p, _) in enumerate(pieces)}
    seq = [{"type": "Precompiled", "precompiled_charsmap": base64.b64encode(charsmap).decode("ascii")}] if charsmap else []
    meta = {"type": "Metaspace", "replacement": SP_SPACE, "prepend_scheme": prepend_scheme if layout == "C" else "always",
            "split": True}
    if layout == "H":
        seq.append({"type": "Replace", "pattern": {"Regex": " {2,}"}, "content": " "})
        pre = {"type": "Sequence", "pretokenizers": [{"type": "WhitespaceSplit"}, meta]}
    else:
        seq += [{"type": "Strip", "strip_left": False, "strip_right": True},
                {"type": "Replace", "pattern": {"Regex": " {2,}"}, "content": SP_SPACE}]
        pre = meta
    eos = ids["</s>"]
    tj = {
        "version": "1.0", "truncation": None, "padding": None,
        "added_tokens": [{"id": ids[t], "content": t, "single_word": False, "lstrip": False, "rstrip": False,
                          "normalized": False, "special": True} for t in _UNI_SPECIAL],
        "normalizer": {"type": "Sequence", "normalizers": seq},
        "pre_tokenizer": pre,
        "post_processor": {
            "type": "TemplateProcessing",
            "single": [{"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "</s>", "type_id": 0}}],
            "pair": [{"Sequence": {"id": "A", "type_id": 0}}, {"SpecialToken": {"id": "</s>", "type_id": 0}},
                     {"Sequence": {"id": "B", "type_id": 0}}, {"SpecialToken": {"id": "</s>", "type_id": 0}}],
            "special_tokens": {"</s>": {"id": "</s>", "ids": [eos], "tokens": ["</s>"]}}},
        "decoder": dict(meta),
        "model": {"type": "Unigram", "unk_id": ids["<unk>"], "vocab": [[p, s] for p, s in pieces],
                  "byte_fallback": byte_fallback}}
    Tokenizer.from_str(json.dumps(tj))  # the library reads what was written

    def write(tmp):
        with open(tmp, "w", encoding="utf-8") as f:
            json.dump(tj, f, ensure_ascii=False)

    return _save_atomically(path, write)


def load_tokenizer(name: str, tokenizer_dir: Optional[str] = None) -> TokenCounterModel:
    path = resolve_tokenizer_file(name, tokenizer_dir)
    if path is None:
        raise Unexpected("Error in loading tokenizer")
    try:
        return TokenCounterModel(path)
    except Exception as e:  # noqa: BLE001 - any load failure maps to the reference's error
        raise Unexpected("Error in loading tokenizer") from e
