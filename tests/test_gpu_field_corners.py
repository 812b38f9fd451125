"""The field arithmetic hipcc compiles from C++ on the MI355X at the corners of its limb bounds.  tests/test_gpu_asm_corners.py does this
for the generated ladder bodies; here it is fp127.hip.h's plain, chained, signed and generated products, the lazy additions and their
exits, pair.hip.h's two- and four-lane arithmetic, canonical form and the verdicts, and the group law written on them -- every
instantiation the library makes and the frontier of every product's static_asserts (tests/test_field_probe.py keeps that list complete).

tests/hip/field_flavour_probe.hip runs ONE instantiation per launch on raw limbs: all limbs at +-B UNIT, every max / min combination of
the components, random extremes, the shape fe_finish hands on, and for canonical form the redundant zeros k p and K (2^130 - 8).  A vector
passes only if (1) the residue of every output is the operation on the input residues, computed with curve4q_oracle on Python integers,
and (2) every output limb lies within what the result type promises.  tests/field_model.py's model -- shown on the CPU to meet both on
these very vectors -- appears in a failure's message only."""
import ctypes
import time

import numpy as np
import pytest

import field_model as fm

pytestmark = pytest.mark.gpu

TABLE = fm.probe_table()


def _load(tmp_path_factory, chain):
    from test_field_probe import build_field_probe       # compile_unit's register check has passed, or this raises before anything runs
    t0 = time.time()
    lib = ctypes.CDLL(build_field_probe(str(tmp_path_factory.mktemp("field_probe")), chain))
    print("field probe%s: %d entries compiled in %.1f s" % (" (FQ_CHAIN=1)" if chain else "", len(TABLE), time.time() - t0))
    assert lib.fq_field_probe_count() == len(TABLE)       # the table this file read is the table that was compiled
    fn = lib.fq_field_probe_run
    fn.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    fn.restype = ctypes.c_int
    return fn


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return _load(tmp_path_factory, False)


@pytest.fixture(scope="module")
def chain_probe(tmp_path_factory):
    return _load(tmp_path_factory, True)


def run_entry(probe, ident, entry):
    """one launch: every vector of the entry, every output checked; returns the seconds spent in the call"""
    vecs = fm.vectors(entry)
    rin = np.array(fm.pack(entry, vecs), dtype=np.uint32)
    rout = np.zeros_like(rin)
    t0 = time.time()
    assert probe(ident, rin.ctypes.data, rout.ctypes.data, len(rin)) == 0, fm.entry_name(entry)
    spent = time.time() - t0
    reach = 0.0
    for k, ((pattern, v, mask), views) in enumerate(zip(vecs, fm.unpack(entry, rout.tolist()))):
        want = fm.expected(entry, v, mask)
        for pair, out in enumerate(views):                   # the four-lane entries hold every value twice: both pairs are checked
            bad = fm.check_outputs(entry, out, want)
            if bad is not None:
                try:
                    model = fm.model_outputs(entry, v, mask)
                except fm.ModelOverflow as exc:
                    model = "overflows: %s" % exc
                raise AssertionError("id %d %s, vector %d (%s, mask %x), pair %d: %s\n  inputs %r\n  the model gives %r" % (
                    ident, fm.entry_name(entry), k, pattern, mask, pair, bad, v, model))
            reach = max(reach, fm.limb1_reach(entry, out))
    print("id %3d %-22s %4d vectors, %5d lanes, largest |limb 1| of a product %.6f UNIT" % (ident, fm.entry_name(entry), len(vecs), len(rin), reach))
    return spent


@pytest.mark.parametrize("family", sorted(fm.FAMILIES))
def test_gpu_family_meets_its_contract_at_the_corners(probe, family):
    ids = [(i, e) for i, e in enumerate(TABLE) if e[0] == family]
    assert ids, family
    spent = sum(run_entry(probe, ident, entry) for ident, entry in ids)
    print("%s: %d ids, %.3f s in copies and kernels" % (family, len(ids), spent))


def test_gpu_add_table_on_chained_products(chain_probe):
    """add_table's products are the unit's MUL_GROUP: Plain in the probe as the other tests build it, Chain in the FQ_CHAIN=1 units that run
    the comb table's ladder -- the same entry of the same source built as such a unit"""
    entry = ("AddTable", 0, 0)
    run_entry(chain_probe, TABLE.index(entry), entry)
