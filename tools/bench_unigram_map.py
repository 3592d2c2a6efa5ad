"""Times k_uni_count_map against k_uni_count on one GPU: the same packed documents, with the code
points that only the mapped kernel counts (U+2026 in the synthetic corpus) removed, so that both
kernels count every document and give equal results. One stream, one launch at a time, timed with
HIP events; prints the median and the band of ``--reps`` launches per kernel, and their ratio: the
price of walking the text through the replacement records where there is nothing to replace.

    python tools/bench_unigram_map.py TOKENIZER.json [--docs 19000] [--mean-bytes 1024] [--reps 9]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tokenizer")
    ap.add_argument("--docs", type=int, default=19000, help="about the kept documents of a 262,144-document step")
    ap.add_argument("--mean-bytes", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    from textblaster_amd.models.tokenizer import TokenCounterModel, count_spec
    from textblaster_amd.ops import hiprt
    from textblaster_amd.ops.kernels import Kernels
    from textblaster_amd.utils import synth

    m = TokenCounterModel(a.tokenizer)
    texts = [t.replace("\u2026", "") for t in synth.make_corpus(a.docs, a.mean_bytes, seed=7, vocab="zipf")]
    data, off = synth.pack(texts)
    want = count_spec(m.unigram_spec(), data, off, 16)
    assert (want >= 0).all() and (count_spec(m.unigram_map_spec(), data, off, 16) == want).all()
    k = Kernels(0)
    d_text = hiprt.to_device(np.concatenate([data, np.zeros(16, np.uint8)]))
    d_off = hiprt.to_device(off)
    n = len(texts)
    out = {"docs": n, "bytes": int(len(data)), "tokenizer": os.path.basename(a.tokenizer), "reps": a.reps}
    for name, spec in (("k_uni_count", m.unigram_spec()), ("k_uni_count_map", m.unigram_map_spec())):
        tabs = k.uni_tables(spec)
        counts = hiprt.zeros(n, np.int32)
        ms = []
        for rep in range(a.reps + 2):  # two warm-up launches
            t0 = hiprt.Event(timing=True).record()
            k.uni_count(tabs, d_text, d_off, None, n, counts)
            t1 = hiprt.Event(timing=True).record()
            t1.synchronize()
            if rep >= 2:
                ms.append(t0.elapsed_time(t1))
        assert (counts.to_host() == want).all(), name
        out[name] = {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}
    out["ratio"] = round(out["k_uni_count_map"]["median_ms"] / out["k_uni_count"]["median_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
