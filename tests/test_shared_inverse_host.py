"""The slot geometry of a lane and the shared inversion (fourq_amd/csrc/lower.hip.h: LaneSlots, SharedInverse) on the CPU.  Both are plain
C++ behind one qualifier macro, so tests/c/shared_inverse_check.cpp includes the shipped header, compiles for the host and runs them over the
integers modulo 251: K in {1, 2, 4, 8}, every n from 1 to 4 K + 3, every lane and three past the last, nobody / everybody / each single
element / 200 seeded random sets masked.  The program itself checks that every id in [0, n) is produced exactly once, that every slot loads a
row below n, that each unmasked element times its result is 1, that a masked element leaves the other results of its lane as the run without
the mask gave them, and that a lane inverts once.  The elements end their own heap allocation, and the same program runs once more under
AddressSanitizer + UndefinedBehaviorSanitizer (stand-alone, nothing preloaded)."""
import os
import subprocess

import pytest

from conftest import ROOT

KS = (1, 2, 4, 8)
CASES = sum(2 + n + 200 for K in KS for n in range(1, 4 * K + 4))
LANES = sum((2 + n + 200) * ((n + K - 1) // K) for K in KS for n in range(1, 4 * K + 4))


def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "fourq_amd", "csrc")] + extra +
                   [os.path.join(ROOT, "tests", "c", "shared_inverse_check.cpp"), "-o", exe], check=True)
    return exe


def _run(exe):
    proc = subprocess.run([exe], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    assert "runtime error" not in proc.stderr and "Sanitizer" not in proc.stderr, proc.stderr[-4000:]
    assert proc.stdout.split() == ["cases", str(CASES), "lanes", str(LANES)] and CASES > 10000


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("shared_inverse_check")


def test_shipped_geometry_and_shared_inversion_over_a_toy_field(tmp):
    _run(_build(tmp, "shared_inverse_check", []))


def test_shipped_geometry_and_shared_inversion_under_the_sanitizers(tmp):
    _run(_build(tmp, "shared_inverse_check_san", ["-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"]))
