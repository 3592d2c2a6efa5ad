"""The folding WordPiece counter's host code under sanitizers: tools/wp_fold_selftest.cpp (csrc/
common/wordpiece.h wpf_* over adversarial documents in exactly sized buffers, in the three fold
modes, against a std::string implementation of the same rules and against its own lane split) built
with AddressSanitizer + UBSan as a stand-alone program. Host code only."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = [pytest.mark.slow,
              pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")]


def test_asan_ubsan(tmp_path):
    exe = str(tmp_path / "wp_fold_selftest")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=undefined", os.path.join(REPO, "tools", "wp_fold_selftest.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, "1500"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout
