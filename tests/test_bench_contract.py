"""bench.py output contract (one JSON line from rank 0 with the driver's keys) on the CPU backend:
one process, and two gloo ranks under torch.distributed.run (global batch = per-rank batch x
world, counters summed over ranks, value = global docs / max-over-ranks seconds); --full and
--dump-outputs (reproducible .npy dump of the last timed step's result)."""
import json
import os
import socket
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--backend", "cpu", "--segmentation", "rules", "--docs-per-step", "128", "--pool", "64",
        "--mean-bytes", "512", "--threads", "2"]
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd, env_extra=None):
    env = dict(os.environ)
    env.update(env_extra or {})
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def _check(line, steps, warmup, world):
    assert KEYS <= set(line)
    assert line["metric"] == "documents/sec through full C4+Gopher+langID pipeline at 1/2/4/8 MI355X"
    assert line["unit"] == "docs/s" and line["higher_is_better"] is True and line["scaling"] == "weak"
    assert line["steps"] == steps and line["warmup"] == warmup
    # dtype = the language-id head that ran: the default v3 model's bf16 MFMA head
    assert line["dtype"] == "bf16" and "bf16 MFMA head" in line["config"]["model"]
    assert line["config"]["global_batch"] == 128 * world
    assert line["config"]["parallelism"] == f"dp{world}"
    # every timed step's documents are counted once: kept + excluded + errors = steps x global batch
    assert line["kept"] + line["excluded"] + line["errors"] == steps * 128 * world
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value = global docs / timed seconds = global batch / step time
    assert abs(line["value"] * line["ms_per_step"] / 1000.0 - 128 * world) / (128 * world) < 0.01
    assert {"finish", "total"} <= set(line["mean_step_timings"])


def test_bench_single_process_contract():
    line = _run([sys.executable, "bench.py", "--steps", "2", "--warmup", "1"] + ARGS)
    _check(line, 2, 1, 1)


def test_bench_full_option_keeps_the_contract():
    """--full (where measurements with runs of their own go) prints the same single line."""
    line = _run([sys.executable, "bench.py", "--steps", "3", "--warmup", "0", "--full"] + ARGS)
    _check(line, 3, 0, 1)


def test_bench_dump_outputs_is_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's result as float .npy arrays that agree with the
    line's counters and are identical from run to run (seeded inputs)."""
    import numpy as np

    dumps = []
    for d in ("a", "b"):
        line = _run([sys.executable, "bench.py", "--steps", "1", "--warmup", "1",
                     "--dump-outputs", str(tmp_path / d)] + ARGS)
        _check(line, 1, 1, 1)
        dumps.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = dumps
    assert set(a) == set(b) >= {"rows", "status", "fail_step", "text_len", "text_crc32", "meta_len", "meta_crc32",
                                "sample_rows", "sample_text", "sample_text_off", "sample_meta", "sample_meta_off"}
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    assert sum(v.nbytes for v in a.values()) <= 64_000_000
    # one timed step: the dumped per-document columns are that step's counters
    assert np.array_equal(a["rows"], np.arange(128))
    assert int((a["status"] == 0).sum()) == line["kept"] and int((a["status"] == 1).sum()) == line["excluded"]
    assert np.array_equal(a["fail_step"] < 0, a["status"] == 0)
    assert (a["text_len"][a["status"] < 2] >= 0).all()
    # the sampled bytes are the documents the per-document columns describe
    off = a["sample_text_off"].astype(np.int64)
    rows = a["sample_rows"].astype(np.int64)[:len(off) - 1]
    assert np.array_equal(np.diff(off), a["text_len"][rows]) and off[-1] == len(a["sample_text"])
    r0 = int(rows[0])
    assert zlib.crc32(a["sample_text"][off[0]:off[1]].astype(np.uint8).tobytes()) == a["text_crc32"][r0]


def test_bench_two_ranks_contract():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "2",
           "--steps", "2", "--warmup", "1"] + ARGS
    line = _run(cmd, {"MASTER_ADDR": "127.0.0.1"})
    _check(line, 2, 1, 2)


def test_bench_spawns_ranks_itself():
    """``bench.py --gpus N`` without an outer launcher starts N ranks (gloo here) as a child
    torch.distributed.run and reports the whole job."""
    line = _run([sys.executable, "bench.py", "--gpus", "3", "--steps", "2", "--warmup", "1"] + ARGS,
                {"TB_MASTER_PORT": str(_free_port())})
    _check(line, 2, 1, 3)
    assert line["n_gpus"] == 3


def test_bench_refuses_missing_gpus():
    """More GPUs than visible fails loudly instead of silently running one rank."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="0")
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "1"], cwd=ROOT, capture_output=True,
                       text=True, timeout=300, env=env)
    assert p.returncode != 0 and "--gpus 2" in p.stderr


def test_bench_world_mismatch_fails():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "1"] + ARGS, cwd=ROOT,
                       capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode != 0 and "WORLD_SIZE=1" in p.stderr


def test_bench_rejects_zero_steps():
    p = subprocess.run([sys.executable, "bench.py", "--steps", "0"] + ARGS, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert p.returncode != 0 and "--steps" in p.stderr
