"""The C launch ABI of libtbhip.so (the extern "C" blocks of the csrc/hip/*.hip kernel units) against its ctypes
mirror (ops/kernels.py): struct sizes, and the launchers' argument checks, which all return before
any HIP call, so these run without a GPU."""
import ctypes

import pytest

from textblaster_amd import native
from textblaster_amd.ops import kernels as K

P = ctypes.c_void_p(16)  # a non-null pointer no launcher dereferences on the paths below
KB = 1024


@pytest.fixture(scope="module")
def lib():
    lib = native.hip()
    K.declare(lib)
    return lib


def tables():
    return K.Tables(s1=16, s2=16, l1=16, l2=16, pw=16, pw_n=0)


def docs(n_launch=1, ndocs=1):
    return K.Docs(bytes=16, off=16, perm=16, dead=16, n_launch=n_launch, ndocs=ndocs)


def work(lds_bytes=0):
    return K.Work(scratch=16, scratch_off=16, rec=16, flags=16, prof=16, lds_bytes=lds_bytes)


def badwords(table_mask=3, seg_bytes=2048):
    return K.BadWords(root=16, cjk=16, table=16, f1=16, f2=16, seg_doc=16, seg_idx=16, root0=0, cjk0=0, dead_max=0,
                      table_mask=table_mask, seg_bytes=seg_bytes)


def resolve_out():
    return K.ResolveOut(fail=16, status=16, fver=16, lanes=16, sc=16, out=16, cap=64, out_off=16, rows=16, err=16)


DICT_IN = K.DictIn(16, 16, 16)
DICT_LINES = K.DictLines(16, 16)
PTRS8 = (ctypes.c_void_p * 8)(*[16] * 8)
PP = ctypes.cast(PTRS8, ctypes.c_void_p)


def test_launch_struct_sizes_match_the_library(lib):
    assert K.ABI_VERSION == lib.tb_abi_version()
    for st, sizeof in K.LAUNCH_STRUCTS.items():
        assert ctypes.sizeof(st) == getattr(lib, sizeof)(), st.__name__
    # the token counters' blocks have no mirror: the host module builds them as bytes
    assert lib.tb_sizeof_bpe() == native.host().SIZEOF_DEV_BPE
    assert lib.tb_sizeof_wp() == native.host().SIZEOF_DEV_WP


def test_struct_arguments_are_typed(lib):
    structs = {ctypes.POINTER(st) for st in K.LAUNCH_STRUCTS}
    for name, args in K._SIGS.items():
        if structs & set(args):
            assert len(args) <= 12, name
    with pytest.raises(ctypes.ArgumentError):
        lib.tb_c4_pass_a(None, P, work(), docs(), tables(), P, None, None, None)  # docs and work swapped
    with pytest.raises(ctypes.ArgumentError):
        lib.tb_stage_analyze(None, P, P, docs(0, 0), work(), tables(), None, None, DICT_LINES)


def test_empty_launches_return_success(lib):
    """Count 0 in the field (or argument) each launcher takes its count from, everything else a
    dummy pointer: 0 before anything is read."""
    t, w = tables(), work()
    wave0, launch0 = docs(n_launch=1, ndocs=0), docs(n_launch=0, ndocs=1)
    assert lib.tb_stage_analyze(None, P, P, wave0, w, t, P, P, DICT_IN) == 0
    assert lib.tb_stage_analyze_blk(None, P, P, launch0, w, t, P, 0, 0, P, P, DICT_IN) == 0
    assert lib.tb_gr_split_wave(None, P, 0, launch0, 1, P, w, t, 1, 0) == 0
    assert lib.tb_gr_dup_split(None, P, 0, launch0, 1, P, w, t, P) == 0
    assert lib.tb_pre_decode(None, launch0, P, 1, P, t) == 0
    assert lib.tb_pre_wcanon(None, launch0, P, 1, t, P) == 0
    assert lib.tb_c4_pass_a(None, P, wave0, w, t, P, P, P, DICT_LINES) == 0
    assert lib.tb_c4_pass_a_blk(None, P, launch0, w, t, P, P, P, DICT_LINES) == 0
    assert lib.tb_c4_pass_b(None, P, P, 0, P, P, P, P, P) == 0
    assert lib.tb_badwords_match(None, launch0, t, badwords(), P) == 0
    assert lib.tb_langid_mfma(None, launch0, t, P, P, P, 1.0, P, P, 2, P) == 0
    assert lib.tb_gate(None, P, PP, 1, 0, P, P, 1) == 0
    assert lib.tb_resolve(None, P, PP, 1, 0, P, PP, PP, 1, resolve_out()) == 0


def test_bad_arguments_are_refused(lib):
    """One case per argument check that returns before any HIP call."""
    t, w, d = tables(), work(), docs()
    assert lib.tb_gr_split_wave(None, P, 0, d, 1, P, w, t, 1, 2) != 0  # n_big > n_docs
    assert lib.tb_gr_dup_split(None, P, 0, d, 1, P, w, t, None) != 0  # null cursor
    assert lib.tb_badwords_match(None, d, t, badwords(table_mask=2), P) != 0  # not 2^k - 1
    assert lib.tb_badwords_match(None, d, t, badwords(seg_bytes=100), P) != 0
    assert lib.tb_pre_decode(None, docs(n_launch=65536, ndocs=65536), P, 1, P, t) != 0
    assert lib.tb_gate(None, P, PP, 1, 1, P, P, 0) != 0  # code 0
    assert lib.tb_resolve(None, P, PP, 1, 1, P, PP, PP, 0, resolve_out()) != 0  # no content version
    big = work(lds_bytes=160 * KB + 256)
    assert lib.tb_stage_analyze(None, P, P, d, big, t, None, None, None) != 0
    assert lib.tb_c4_pass_a(None, P, d, big, t, P, None, None, None) != 0
