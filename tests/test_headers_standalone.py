"""Every header of csrc/common compiles on its own: a family header (doc_ctx.h, doc_text.h, ...,
see docproc.h for the map) includes what it uses and does not lean on the unit that includes it."""
import glob
import os
import shutil
import subprocess

import pytest

COMMON = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "common")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(COMMON, "*.h")))
assert "doc_ctx.h" in HEADERS and "docproc.h" in HEADERS, COMMON


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header):
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-x", "c++", os.path.join(COMMON, header)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
