"""Every microbenchmark under tools/microbench that includes a header of fourq_amd/csrc must still compile against it: these are the programs
DESIGN.md cites for its numbers, and nothing else builds them.  -Werror=undefined-inline turns a device function that a header declares
but only another header defines -- which compiles, then fails to link -- into a compile error.  Needs the ROCm compiler, no GPU."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs the ROCm compiler")

BENCH_DIR = os.path.join(ROOT, "tools", "microbench")
USES_PRODUCT_HEADER = re.compile(r'#include\s+"[^"]*fourq_amd/csrc/|#include\s+"add_entry\.hip\.h"')


def product_benchmarks():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(BENCH_DIR, "*.hip")) if USES_PRODUCT_HEADER.search(open(p).read()))


def test_the_list_is_not_empty():
    assert len(product_benchmarks()) >= 10


@pytest.mark.parametrize("name", product_benchmarks())
def test_microbenchmark_compiles_against_the_product_headers(name):
    cmd = [HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only", "-Werror=undefined-inline", name]
    r = subprocess.run(cmd, cwd=BENCH_DIR, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    errors = [ln for ln in r.stdout.splitlines() if "error" in ln]
    assert r.returncode == 0, "\n".join(errors[:20])
