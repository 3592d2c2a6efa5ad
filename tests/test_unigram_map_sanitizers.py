"""The mapped Unigram counter's host code under sanitizers: tools/unigram_map_selftest.cpp
(csrc/common/unigram.h unim_* over adversarial words in exactly sized buffers, against a std::string
Viterbi on the materialised normalised text and against its own lane split, and the validator's
refusals) built with AddressSanitizer + UBSan as a stand-alone program. Host code only (GPU
sanitizers are not available on the MI355X pool)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = [pytest.mark.slow,
              pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")]


def test_asan_ubsan(tmp_path):
    exe = str(tmp_path / "unigram_map_selftest")
    src = os.path.join(REPO, "tools", "unigram_map_selftest.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=undefined", src, "-o", exe],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout
