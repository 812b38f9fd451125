"""The generated bodies on the MI355X at the corners of their contracts.  tests/test_asm_bounds.py proves the bodies' bounds in
tools/asmgen/sim.py's semantics; this shows that the hardware agrees with those semantics where it matters: tests/hip/asm_body_probe.hip
runs each body (through the library's ladder_asm.hip.h wrappers) on bounds.corner_vectors' inputs -- limbs at their extremes, max / min
patterns per component, top limbs in [2^23, 2^24) -- with both neg-mask values, and every output register must equal sim.run's."""
import ctypes
import os
import random
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools", "asmgen"))
import bounds as bd                # noqa: E402
import sim                         # noqa: E402

pytestmark = pytest.mark.gpu

BODY_IDS = {"DBL": 0, "DBLT": 1, "ADD": 2, "STEP": 3, "TAU": 4, "UPSILON": 5, "CHI": 6, "TAUDUAL": 7, "R1TOR2": 8, "TABLEADD": 9,
            "MULU<1,1>": 10, "SQRU<1>": 11}     # the probe's switch; MULU / SQRU through fe2_mul_asm<1, 1> / fe2_sqr_asm<1>
WORDS = 128
COUNT = 1000


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from test_asm_probe import build_probe        # compile_unit's register check has passed, or this raises before anything runs
    lib = ctypes.CDLL(build_probe(str(tmp_path_factory.mktemp("probe"))))
    fn = lib.fq_asm_body_probe_run
    fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    fn.restype = ctypes.c_int
    return fn


@pytest.mark.parametrize("name", list(BODY_IDS))
def test_gpu_body_equals_sim_at_the_corners(probe, name):
    lines = [t for _, t in bd.shipped()[bd.body_of(name)]]
    vecs = bd.corner_vectors(name, random.Random(zlib.crc32(name.encode()) + 1), COUNT)
    outs = [(op, base, n) for op, (base, n, _, out) in bd.operands(name).items() if out is not None]
    for neg in bd.neg_values(name):
        rin = np.zeros((len(vecs), WORDS), dtype=np.uint32)
        want = []
        for k, v in enumerate(vecs):
            regs = bd.registers(name, v, neg)
            for r, x in regs.items():
                rin[k, int(r[1:])] = x
            if name == "SQRU<1>":
                rin[k, 40:45] = [t // 2 for t in v["t"]]         # a.re, which the wrapper turns into d, s, t itself
            res = sim.run(lines, regs)
            want.append([res["%%%d" % (base + i)] for _, base, n in outs for i in range(n)])
        rout = np.zeros_like(rin)
        assert probe(BODY_IDS[name], rin.ctypes.data, rout.ctypes.data, len(vecs)) == 0
        for k in range(len(vecs)):
            got = [int(rout[k, base + i]) for _, base, n in outs for i in range(n)]
            assert got == want[k], (name, neg, k, [op for op, _, _ in outs])
