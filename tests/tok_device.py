"""What the token counters' GPU tests share (test_gpu_bpe_*.py, test_gpu_wordpiece*.py, test_bpe.py):
a launch of the counting kernels on packed documents compared with the host emulation's result, and
Engine(cuda) with a trailing TokenCounter against Engine(cpu) with the host / device document
counters read around it."""
import struct

import numpy as np


def assert_kernels_equal(sp, data, off, raw, runs=1, tables="token_tables", count="token_count"):
    """The kernels of ``sp`` directly on the packed documents (16 bytes of padding behind the text,
    no K16 count pointer), ``runs`` times on one input: every result equals ``raw``, the host
    emulation's. Returns the device tables."""
    from textblaster_amd.ops import hiprt
    from textblaster_amd.ops.kernels import Kernels

    k = Kernels(0)
    tabs = getattr(k, tables)(sp)
    d_text = hiprt.to_device(np.concatenate([data, np.zeros(16, np.uint8)]))
    d_off = hiprt.to_device(off)
    n = len(off) - 1
    for _ in range(runs):
        out = hiprt.zeros(n, np.int32)
        getattr(k, count)(tabs, d_text, d_off, None, n, out)
        np.testing.assert_array_equal(out.to_host(), raw)
    return tabs


def block_pointer(block, offsets, name):
    """The pointer field ``name`` of a parameter block (offsets: the host module's DEV_*_OFFSETS)."""
    return struct.unpack_from("<Q", block, offsets[name])[0]


def device_and_cpu(make_cfg, tok, data, off, backend="cuda"):
    """Engine(backend) over ``make_cfg()`` with the resolve and the token counter on the device, and Engine(cpu), on one
    input: statuses and outputs are equal. Returns the device result, its outputs, and how many
    kept documents the host tokenizer / the kernels counted."""
    from test_emulated_device_path import outputs

    from textblaster_amd.ops import hiprt
    from textblaster_amd.pipeline.engine import Engine
    from textblaster_amd.utils import metrics

    assert hiprt.device_count() > 0
    eng = Engine(make_cfg(), backend=backend, keep_reasons=True, tokenizer_file=tok)
    assert eng.device_runner.resolve_t is not None and eng.device_runner.bpe
    h0, d0 = metrics.BPE_HOST_DOCS_TOTAL._value.get(), metrics.BPE_DEVICE_DOCS_TOTAL._value.get()
    a = eng.process(data, off)
    nh = metrics.BPE_HOST_DOCS_TOTAL._value.get() - h0
    nd = metrics.BPE_DEVICE_DOCS_TOTAL._value.get() - d0
    b = Engine(make_cfg(), backend="cpu", nthreads=8, keep_reasons=True, tokenizer_file=tok,
               segmentation="icu").process(data, off)
    np.testing.assert_array_equal(a.status, b.status)
    oa = outputs(a)
    assert oa == outputs(b)
    return a, oa, nh, nd
