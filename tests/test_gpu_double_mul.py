"""[k]B + [l]P on the device and the byte-level signature check on top of it (fourq_double_mul_* / fourq_verify_bytes_*, combine_kernel).

Expected values come from three places, none of them the code under test: the real reference's answers recorded in
tests/golden/double_mul.json, the group law [k]G + [l][t]G = [(k + l t) mod N]G with the point work done by the C oracle, and the
C oracle's two halves joined by the Python oracle's ADD.  tests/test_double_mul_oracle.py pins all three against each other on the CPU.
Every test takes `eng`, so everything runs with table selection by address and with constant-time selection.
"""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import curve4q_oracle as o
import oracle_c as oc
from bench import seeded_scalars
from conftest import ROOT
from fourq_amd import _lib, codec

pytestmark = pytest.mark.gpu

G1 = o.AffineToR1(o.Gx, o.Gy)
G1_WORDS = codec.pack_point(G1)
NEUTRAL_AFFINE = codec.pack_point(((0, 0), (1, 0)))
NEUTRAL_ENC = np.frombuffer(bytes([1] + [0] * 31), dtype=np.uint8)
DECODE_CODE = {"AttributeError": _lib.DECODE_REF_ATTRIBUTE_ERROR, "Exception: Point not on curve": _lib.DECODE_NOT_ON_CURVE,
               "Exception: Malformed point: reserved bit": _lib.DECODE_RESERVED_BIT}

_cache = {}


def g_comb(eng):
    """The comb of G itself (one per session: a table is data, the same from either selection mode)."""
    if "comb" not in _cache:
        _cache["comb"] = eng.comb_table(G1_WORDS)
        _cache["table"] = oc.table(oc.ENDO, G1_WORDS)
    eng.comb_stage(_cache["comb"])                    # calls below may pass comb=None: "the staged table"
    return _cache["comb"]


def identity_batch(eng, n, seed):
    """Seeded k, l, t; P_i = [t_i]G from the existing comb call; expected [(k_i + l_i t_i) mod N]G from the C oracle: the modular
    arithmetic in Python ints, the point work in oracle/fourq_oracle.c.  Cached per (n, seed): both selection modes share it."""
    key = ("identity", n, seed)
    if key not in _cache:
        comb = g_comb(eng)
        k, l, t = seeded_scalars(seed, n), seeded_scalars(seed + 1, n), seeded_scalars(seed + 2, n)
        sums = [(a + b * c) % o.N for a, b, c in zip(codec.unpack_scalars(k), codec.unpack_scalars(l), codec.unpack_scalars(t))]
        want = oc.r1_to_affine(oc.mul(oc.ENDO, codec.pack_scalars(sums), None, _cache["table"]))
        P, st = eng.comb_mul(t, comb)
        assert not st.any()
        # the inputs themselves against the C oracle: P_i = [t_i]G
        assert np.array_equal(P, oc.r1_to_affine(oc.mul(oc.ENDO, t, None, _cache["table"])))
        _cache[key] = (k, l, t, P, want)
    return _cache[key]


def mismatches(got, want):
    return np.flatnonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(torch.device("cuda", 0))


def dev_double_mul(eng, k, l, P, comb=None):
    import torch
    out = torch.empty((len(k), 8), dtype=torch.int64, device=torch.device("cuda", 0))
    eng.double_mul_dev(to_dev(k), to_dev(l), to_dev(P), out, len(k), comb_host=comb)
    eng.sync()
    return out.cpu().numpy().view(np.uint64)


def dev_verify(eng, k, l, keys, expect, comb=None):
    import torch
    dev = torch.device("cuda", 0)
    ok, st = torch.empty(len(k), dtype=torch.uint8, device=dev), torch.empty(len(k), dtype=torch.uint8, device=dev)
    eng.verify_bytes_dev(to_dev(k), to_dev(l), to_dev(keys), to_dev(expect), ok, st, len(k), comb_host=comb)
    eng.sync()
    return ok.cpu().numpy(), st.cpu().numpy()


def hex_rows(values):
    return np.frombuffer(b"".join(bytes.fromhex("%064x" % v) for v in values), dtype=np.uint8).reshape(-1, 32)


# ---- 1. the reference's own answers -------------------------------------------------------------------------------------------
def test_fixture_parity_affine_bytes_and_single_call(eng, golden):
    cases = list(golden("double_mul.json")["cases"])
    comb = g_comb(eng)
    k, l = codec.pack_scalars([c["k"] for c in cases]), codec.pack_scalars([c["l"] for c in cases])
    P = codec.pack_points([c["P"] for c in cases], 2)
    want = codec.pack_points([c["R"] for c in cases], 2)
    got = eng.double_mul(k, l, P, comb)
    assert mismatches(got, want).size == 0, [cases[i]["_label"] for i in mismatches(got, want)]
    assert mismatches(dev_double_mul(eng, k, l, P), want).size == 0
    # 32-byte flavour: where the reference's decode refuses encode(P) (the neutral point's encoding is one such string) the status says so
    out, st = eng.double_mul_bytes(k, l, hex_rows(c["P_enc"] for c in cases), comb)
    want_enc = hex_rows(c["R_enc"] for c in cases).copy()
    want_st = np.zeros(len(cases), dtype=np.uint8)
    for i, c in enumerate(cases):
        if c["_P_decode"] != "ok":
            code = [v for key, v in DECODE_CODE.items() if c["_P_decode"].startswith(key)]
            assert len(code) == 1, c["_P_decode"]
            want_st[i] = _lib.BYTES_DECODE_BASE + code[0]
            want_enc[i] = 0
    assert np.array_equal(st, want_st) and mismatches(out, want_enc).size == 0
    assert (want_st == 0).sum() >= 56
    # the drop-in module's single call (an addition to the reference's names), on the same selection mode
    from fourq_amd import curve4q as c4
    from fourq_amd.engine import default_engine
    before = default_engine().ct_select
    default_engine().ct_select = eng.ct_select
    try:
        for c in cases[:6] + cases[-8:] + [c for c in cases if c["_label"].startswith(("sum neutral", "doubling", "k = l"))]:
            assert c4.MUL_double(c["k"], c["l"], c["P"]) == c["R"], c["_label"]
    finally:
        default_engine().ct_select = before


# ---- 2. group law at scale ----------------------------------------------------------------------------------------------------
def test_group_law_parity_at_scale(eng):
    """n = 2^16 + 777: one fused generation and a two-lane remainder on the variable half; every element compared."""
    n = (1 << 16) + 777
    k, l, t, P, want = identity_batch(eng, n, 9100)
    got = eng.double_mul(k, l, P, g_comb(eng))
    bad = mismatches(got, want)
    assert bad.size == 0, bad[:8]
    assert mismatches(dev_double_mul(eng, k, l, P), want).size == 0


# ---- 3. generic points, the two halves joined by the oracle's own ADD ---------------------------------------------------------------
def test_generic_points_including_ones_outside_the_subgroup(eng, golden):
    cases = list(golden("double_mul.json")["cases"])
    bases = sorted({c["P"] for c in cases if not c["_label"].startswith("random")})
    assert sum(1 for c in cases if c["_label"].startswith("P outside")) >= 6
    n = 4096
    rng = random.Random(9300)
    pts = [bases[rng.randrange(len(bases))] for _ in range(n)]
    k, l = seeded_scalars(9301, n), seeded_scalars(9302, n)
    P = codec.pack_points(pts, 2)
    lifted = np.zeros((n, 20), dtype=np.uint64)
    lifted[:, 0:8] = P
    lifted[:, 8] = 1
    lifted[:, 12:20] = P
    g_comb(eng)
    first = codec.unpack_points(oc.mul(oc.ENDO, k, None, _cache["table"]))
    second = codec.unpack_points(oc.mul(oc.ENDO, l, lifted))
    want = oc.r1_to_affine(codec.pack_points([o.ADD(A, o.R1toR2(B)) for A, B in zip(first, second)], 5))
    got = eng.double_mul(k, l, P, g_comb(eng))
    bad = mismatches(got, want)
    assert bad.size == 0, (bad[:8], [pts[i] for i in bad[:2]])


# ---- 4. every route -----------------------------------------------------------------------------------------------------------
def test_every_route_size(eng):
    """Four and two lanes per element, the fused generation, remainders: sizes around every switch, read from the engine.  The comb half
    runs comb_kernel's deferred flavour at all of them, the variable half whatever MUL_endo takes at that size."""
    lanes = eng.lanes
    sizes = [1, 2, 63, 64, 65, 255, 257, lanes // 4 - 1, lanes // 4, lanes // 4 + 1, lanes // 2 - 1, lanes // 2, lanes // 2 + 1, lanes - 1, lanes, lanes + 1]
    k, l, t, P, want = identity_batch(eng, lanes + 1, 9400)
    comb = g_comb(eng)
    enc_P, enc_want = oc.encode(P), oc.encode(want)
    for n in sizes:
        got = eng.double_mul(k[:n], l[:n], P[:n], comb)
        assert mismatches(got, want[:n]).size == 0, n
        assert mismatches(dev_double_mul(eng, k[:n], l[:n], P[:n]), want[:n]).size == 0, n
        out, st = eng.double_mul_bytes(k[:n], l[:n], enc_P[:n])
        assert not st.any() and mismatches(out, enc_want[:n]).size == 0, n
        ok, st = eng.verify_bytes(k[:n], l[:n], enc_P[:n], enc_want[:n])
        assert ok.all() and not st.any(), n


# ---- 5. the verifier must not say yes too often ---------------------------------------------------------------------------------------
def test_verify_accepts_exactly_the_valid_signatures(eng, golden):
    n = 1 << 16
    k, l, t, P, want = identity_batch(eng, n, 9500)
    comb = g_comb(eng)
    keys, expect = oc.encode(P), oc.encode(want)
    ok, st = eng.verify_bytes(k, l, keys, expect, comb)
    assert ok.dtype == np.uint8 and np.array_equal(ok, np.ones(n, dtype=np.uint8)) and not st.any()
    # undecodable keys: 32-byte strings the reference refuses (reserved bit / y not on the curve), from the wire fixture
    refused = [bytes.fromhex(r[0]) for r in golden("wire.json", raw=True)["strings"] if r[1] != "ok" and "AttributeError" not in r[1]]
    assert len(refused) >= 2
    k2, l2, keys2, expect2 = k.copy(), l.copy(), keys.copy(), expect.copy()
    want_ok, want_bad_key = np.ones(n, dtype=np.uint8), np.zeros(n, dtype=bool)
    rng = random.Random(9501)
    for j, i in enumerate(range(0, n, 7)):
        how = j % 5
        if how == 0:
            expect2[i, rng.randrange(32)] ^= 1 << rng.randrange(8)
        elif how == 1:
            k2[i, rng.randrange(4)] ^= np.uint64(1) << np.uint64(rng.randrange(64))
        elif how == 2:
            l2[i, rng.randrange(4)] ^= np.uint64(1) << np.uint64(rng.randrange(64))
        elif how == 3:
            keys2[i] = keys[(i + 1) % n]                       # another valid key
        else:
            keys2[i] = np.frombuffer(refused[(j // 5) % len(refused)], dtype=np.uint8)
            want_bad_key[i] = True
        want_ok[i] = 0
    ok, st = eng.verify_bytes(k2, l2, keys2, expect2)
    assert np.array_equal(ok, want_ok), np.flatnonzero(ok != want_ok)[:8]
    assert np.array_equal(st != 0, want_bad_key)
    assert set(np.unique(st)) <= {0, _lib.BYTES_DECODE_BASE + _lib.DECODE_RESERVED_BIT, _lib.BYTES_DECODE_BASE + _lib.DECODE_NOT_ON_CURVE}
    ok_dev, st_dev = dev_verify(eng, k2, l2, keys2, expect2)
    assert np.array_equal(ok_dev, want_ok) and np.array_equal(st_dev, st)
    # a reserved-bit encoding of the RIGHT point is a mismatch: expect32 is compared as bytes
    expect3 = expect[:64].copy()
    expect3[:, 15] |= 0x80
    ok, st = eng.verify_bytes(k[:64], l[:64], keys[:64], expect3)
    assert not ok.any() and not st.any()


# ---- 6. a bad element cannot touch the ones that share its inversion ------------------------------------------------------------------
def test_bad_elements_do_not_poison_their_lane(eng, golden):
    """A device-resident batch beyond two generations shares ONE inversion between the two elements of a lane (combine_kernel<2>: lane t
    owns t and t + T, T = ceil(n / 2)).  Undecodable keys (32-byte flavour) and all-zero affine pairs (affine flavour) in both slots of
    a lane, in one slot only, at the head and at the ragged end; every other element against the group-law expectation."""
    import torch
    lanes = eng.lanes
    n = 2 * lanes + 131
    T = (n + 1) // 2
    k, l, t, P, want = identity_batch(eng, n, 9600)
    g_comb(eng)
    rng = random.Random(9601)
    bad_at = sorted(set([0, T, 5, 9 + T, 77, 77 + T, T - 1, n - 1] + rng.sample(range(n), 60)))
    good = np.ones(n, dtype=bool)
    good[bad_at] = False
    P2 = P.copy()
    P2[bad_at] = 0
    got = dev_double_mul(eng, k, l, P2)
    assert mismatches(got[good], want[good]).size == 0
    got = eng.double_mul(k, l, P2)                                # host arrays: chunks of one generation, one element per lane
    assert mismatches(got[good], want[good]).size == 0
    refused = [bytes.fromhex(r[0]) for r in golden("wire.json", raw=True)["strings"] if r[1] != "ok" and "AttributeError" not in r[1]]
    keys, expect = oc.encode(P).copy(), oc.encode(want).copy()
    for j, i in enumerate(bad_at):
        keys[i] = np.frombuffer(refused[j % len(refused)], dtype=np.uint8)
    dev = torch.device("cuda", 0)
    out, st = torch.empty((n, 32), dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    eng.double_mul_bytes_dev(to_dev(k), to_dev(l), to_dev(keys), out, st, n)
    eng.sync()
    out, st = out.cpu().numpy(), st.cpu().numpy()
    assert np.array_equal(st != 0, ~good) and not out[~good].any()
    assert mismatches(out[good], expect[good]).size == 0
    ok, st = dev_verify(eng, k, l, keys, expect)
    assert np.array_equal(ok, good.astype(np.uint8)) and np.array_equal(st != 0, ~good)


# ---- 7. the neutral point is an ordinary result ---------------------------------------------------------------------------------------
def test_neutral_result(eng):
    rng = random.Random(9700)
    rows = [(0, 0, rng.getrandbits(256)), (o.N, 0, 3), (0, o.N, 3), (o.N, o.N, rng.getrandbits(256))]
    for _ in range(4):
        l, t = rng.getrandbits(256), rng.getrandbits(256) % o.N
        rows.append(((-l * t) % o.N, l, t))
    k, l, t = (codec.pack_scalars([r[i] for r in rows]) for i in range(3))
    comb = g_comb(eng)
    P, st = eng.comb_mul(t, comb)
    assert not st.any()
    got = eng.double_mul(k, l, P, comb)
    assert np.array_equal(got, np.repeat(NEUTRAL_AFFINE.reshape(1, 8), len(rows), axis=0))
    out, st = eng.double_mul_bytes(k, l, oc.encode(P))
    assert not st.any() and all(np.array_equal(r, NEUTRAL_ENC) for r in out)
    ok, st = eng.verify_bytes(k, l, oc.encode(P), out)
    assert ok.all() and not st.any()
    # unlike the comb's own call, whose DH semantics report the neutral point and zero the row
    _, st = eng.comb_mul(codec.pack_scalars([0, o.N]), comb)
    assert (st == _lib.DH_NEUTRAL).all()


# ---- 8. host-pointer and device flavours, one device and several ----------------------------------------------------------------------
def test_host_and_device_flavours_agree(eng):
    from fourq_amd import MultiEngine, device_count
    n = (1 << 18) + 5
    k, l, t, P, want = identity_batch(eng, n, 9800)
    comb = g_comb(eng)
    keys, expect = oc.encode(P), oc.encode(want).copy()
    expect[::11, 7] ^= 2
    want_ok = np.ones(n, dtype=np.uint8)
    want_ok[::11] = 0
    # pageable arrays
    got = eng.double_mul(k, l, P, comb)
    assert mismatches(got, want).size == 0
    ok, st = eng.verify_bytes(k, l, keys, expect)
    assert np.array_equal(ok, want_ok) and not st.any()
    # pinned arrays, results into pinned arrays
    pinned = [eng.host_array(a) for a in (k, l, P, keys, expect)]
    out_p, ok_p, st_p = eng.host_empty((n, 8)), eng.host_empty(n, np.uint8), eng.host_empty(n, np.uint8)
    try:
        eng.double_mul(pinned[0], pinned[1], pinned[2], out=out_p)
        assert np.array_equal(out_p, got)
        eng.verify_bytes(pinned[0], pinned[1], pinned[3], pinned[4], ok=ok_p, status=st_p)
        assert np.array_equal(ok_p, want_ok) and not st_p.any()
        assert eng.host_stats()["chunks"] > 1
    finally:
        for a in pinned + [out_p, ok_p, st_p]:
            eng.host_free(a)
    # device-resident: one launch chain over the whole batch
    assert np.array_equal(dev_double_mul(eng, k, l, P), got)
    ok_d, st_d = dev_verify(eng, k, l, keys, expect)
    assert np.array_equal(ok_d, want_ok) and not st_d.any()
    # every device present (a one-GPU box: two contexts on device 0)
    count = device_count()
    with MultiEngine(list(range(count)) if count > 1 else [0, 0]) as multi:
        multi.ct_select = eng.ct_select
        ok_m, st_m = multi.verify_bytes(k, l, keys, expect, comb)
        assert np.array_equal(ok_m, want_ok) and np.array_equal(st_m, st)
        assert np.array_equal(multi.double_mul(k[:70000], l[:70000], P[:70000], comb), got[:70000])


# ---- 9. the C ABI from C ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs a C compiler")
def test_c_host_program_checks_fixture_rows(eng, golden, tmp_path):
    from fourq_amd.build import LIB_PATH
    cases = [c for c in golden("double_mul.json")["cases"] if c["_P_decode"] == "ok"]
    src = os.path.join(ROOT, "tests", "c", "double_mul_check.c")
    exe, libdir = str(tmp_path / "double_mul_check"), os.path.dirname(LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), "-o", exe, src,
                    "-L", libdir, "-lfourq_amd", "-Wl,-rpath," + libdir], check=True)
    n = len(cases)
    path = tmp_path / "vectors.bin"
    with open(path, "wb") as fh:
        fh.write(np.uint64(n).tobytes())
        fh.write(np.uint64(1 if eng.ct_select else 0).tobytes())
        fh.write(np.ascontiguousarray(G1_WORDS, dtype="<u8").tobytes())
        for a in (codec.pack_scalars([c["k"] for c in cases]), codec.pack_scalars([c["l"] for c in cases]),
                  codec.pack_points([c["P"] for c in cases], 2), codec.pack_points([c["R"] for c in cases], 2)):
            fh.write(np.ascontiguousarray(a, dtype="<u8").tobytes())
        fh.write(hex_rows(c["P_enc"] for c in cases).tobytes())
        fh.write(hex_rows(c["R_enc"] for c in cases).tobytes())
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = "/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")     # no PyTorch in a C program: the system HIP runtime
    proc = subprocess.run([exe, str(path)], capture_output=True, text=True, env=env)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "double-scalar rows bit-exact through the C ABI" in proc.stdout

