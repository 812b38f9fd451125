"""Cross-checks the CPU oracle against the REAL reference, through tests/golden/reference.json: the reference's constants, public
names, self-test output and results on the seeded inputs drawn below, recorded by tests/golden/make_golden.py (which loads the
reference in memory with oracle/ref_loader.py).  The inputs are drawn here again with the same seeds, in the same order; bulk
results are compared as digests of the same hex form the generator hashes."""
import hashlib
import json
import random

import pytest

import curve4q_oracle as o
from conftest import load_golden


def hx(v):
    """As tests/golden/make_golden.hx: ints -> hex strings, recursively."""
    if isinstance(v, (bool, str)):
        return v
    if isinstance(v, dict):
        return {k: hx(e) for k, e in v.items()}
    if isinstance(v, int):
        return "%x" % v
    return [hx(e) for e in v]


def digest(values):
    """As tests/golden/make_golden.digest."""
    return hashlib.sha256(json.dumps(hx(values), separators=(",", ":")).encode()).hexdigest()[:16]


@pytest.fixture(scope="module")
def ref():
    return load_golden("reference.json", raw=True)


def test_reference_self_tests_pass(ref):
    """The loader ran the reference faithfully when the fixtures were made: its own self-tests printed only [PASS]."""
    out = ref["self_tests"]
    assert not [ln for ln in out if "[FAIL]" in ln] and sum(ln.startswith("[PASS]") for ln in out) >= 20


def test_constants_identical(ref):
    c = ref["constants"]
    assert hx([o.P127, o.d, o.N, o.Gx, o.Gy, o.Ox, o.Oy]) == [c[k] for k in ("p1271", "d", "N", "Gx", "Gy", "Ox", "Oy")]
    assert hx(o.ctau) == c["ctau"] and hx(o.ctaudual) == c["ctaudual"]
    assert hx(list(o.cphi)) == c["cphi"]
    assert hx([o.cpsi[i] for i in (1, 2, 3, 4)]) == c["cpsi"]
    assert hx([list(b) for b in o.BASIS]) == c["basis"] and hx(list(o.ELL)) == c["ell"]
    assert hx(list(o.OFFSET_C)) == c["c"] and hx(list(o.OFFSET_CP)) == c["cp"]


def test_recoding_random(ref):
    rng = random.Random(11)
    edge = [0, 1, 2, o.N - 1, o.N, o.N + 1, (1 << 256) - 1, 1 << 255, (1 << 64) - 1, 1 << 64]
    assert hx([o.decompose(m) for m in edge]) == ref["decompose_edge"]
    ms = edge + [rng.getrandbits(256) for _ in range(20000)]
    vs = [o.decompose(m) for m in ms]
    assert digest(vs) == ref["decompose"]
    assert all(0 <= x < (1 << 64) for v in vs for x in v)
    ms = edge + [rng.getrandbits(256) for _ in range(1500)]
    rec = [o.recode(o.decompose(m)) for m in ms]
    assert digest([[list(x) for x in r] for r in rec]) == ref["recode"]
    assert all(od[64] <= 7 for _, od in rec)


def test_field_random(ref):
    rng = random.Random(12)
    ops = []
    for _ in range(3000):
        a, b = (rng.getrandbits(127) % o.P127, rng.getrandbits(127) % o.P127), (rng.getrandbits(127) % o.P127, rng.getrandbits(127) % o.P127)
        ops.append([o.f2_mul(a, b), o.f2_sqr(a), o.f2_add(a, b), o.f2_sub(a, b)])
    assert digest(ops) == ref["field"]
    ops = []
    for _ in range(40):
        a = (rng.getrandbits(127) % o.P127, rng.getrandbits(127) % o.P127)
        ops.append([o.f2_inv(a), o.fp_invsqrt(a[0])])
    assert digest(ops) == ref["field_inv"]


def test_scalar_mul_and_dh_random(ref):
    rng = random.Random(13)
    P = o.AffineToR1(o.Gx, o.Gy)
    aff = (o.Gx, o.Gy)
    for i in range(60):
        m = rng.getrandbits(256)
        e = o.MUL_endo(m, P)
        row = [e, o.MUL_windowed(m, P)]
        if i % 6 == 0:
            row += [o.table_endo(P), o.table_windowed(P), o.DH_endo(m, aff), o.DH_windowed(m, aff)]
            aff = o.DH_endo(m, aff)
        assert digest(row) == ref["scalar_mul_and_dh"][i], i
        P = e


def test_wire_random(ref):
    rng = random.Random(14)
    for want in ref["wire"]:
        raw = bytearray(rng.getrandbits(256).to_bytes(32, "little"))
        raw[15] &= 0x7F
        try:
            got = ["ok", hx(o.decode(bytes(raw)))]
        except Exception as exc:
            got = [type(exc).__name__, str(exc)]
        assert got == want
    assert len(ref["wire"]) == 150


def test_mirror_module_has_every_public_name_of_the_reference(ref):
    """A user who swaps `import curve4q` for `from fourq_amd import curve4q` must find every module-level name
    (functions and constants; the reference's own test functions and its `getrandbits` import aside), and every
    constant must hold the same value.  Importing the mirror needs no GPU."""
    from fourq_amd import curve4q as m
    from fourq_amd import fields as mf
    public = ref["public_names"]
    assert public and [n for n in public if not hasattr(m, n)] == []
    for n, v in ref["public_values"].items():
        assert hx(getattr(m, n)) == v, n
    for cls in ("GFp", "GFp2"):
        have = dir(getattr(mf, cls))
        assert [n for n in ref["field_methods"][cls] if n not in have] == [], cls


def test_gfp2_invsqrt_as_written(ref):
    """GFp2.invsqrt (fields.py:202-230) is dead code in the reference; the restatement follows it to the letter."""
    rng = random.Random(15)
    cases = [(rng.getrandbits(127) % o.P127, rng.getrandbits(127) % o.P127) for _ in range(40)]
    cases += [(rng.getrandbits(127) % o.P127, 0) for _ in range(20)] + [(4, 0), (1, 0), (2, 0)]
    assert [a for a, _ in ref["gfp2_invsqrt"]] == hx([list(a) for a in cases])
    for a, (_, want) in zip(cases, ref["gfp2_invsqrt"]):
        assert hx(o.GFp2.invsqrt(a)) == want, a
