"""C4 pass A's byte scan and the stop-word fast path under sanitizers: tools/c4_scan_selftest.cpp
(csrc/common/c4_pass_a.h c4_byte_scan / c4_phrases_at and stage_analyze.h is_stop_word on the
host, over phrases at every alignment, cut by the end of the text and across the scan's item boundaries, in buffers that
end with the text, against ci_contains / ci_starts_with and a std::set of stop words) built with
AddressSanitizer + UBSan as a stand-alone program. Host code only (GPU sanitizers are not
available on the MI355X pool)."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = [pytest.mark.slow,
              pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")]


def test_asan_ubsan(tmp_path):
    exe = str(tmp_path / "c4_scan_selftest")
    src = os.path.join(REPO, "tools", "c4_scan_selftest.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-fno-sanitize-recover=undefined", src, "-o", exe],
                   check=True, capture_output=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout
