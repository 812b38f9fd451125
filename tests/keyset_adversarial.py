"""Keys a registrant, not the verifier, chooses, for the key set (fourq_keyset_*, fourq_amd/csrc/keyset.hip.h): three families of 32-byte
strings, the scalar rows that go with the third, and the keyed walk of keyset_comb_kernel in integers modulo N.  Pure Python and the two
oracles; nothing from the library under test.  Shared by the CPU tests (test_keyset_adversarial.py, which proves that every family is what
it is for), the fixture generator (golden/make_keyset_adversarial.py) and the GPU tests (test_gpu_keyset_adversarial.py).

    strings      every member of adversarial_points.all_strings(), duplicates kept: the same bytes in two slots is a case
    shifted      A + T for three honest keys A = [t]G and every T != O of adversarial_points.torsion(), and (-x, -y) of each A: on the curve,
                 of order lcm(N, ord T), so [N] of it is a point of the 392-torsion (or beyond it) and never the neutral point
    structured   [c]G for c in STRUCTURED_C: G and -G, their doubles, 1/2, and the comb's row and plane strides 2^7 and 2^28 (CombShape<9, 4, 7>:
                 e = 7, d = 28).  With a key that is a known multiple of G the accumulator of the two-comb walk is a known scalar, and the
                 rows of structured_rows() steer it into the special cases of the complete addition

walk(k, l, c) follows the kernel's loop with the accumulator as a scalar modulo N and counts those cases.  "add as doubling" needs no
search beyond the rows below: with c = 1 and l = k it is the very first mixed addition (column 6, the key's entry onto G's), and with
c = N - 2 and k = 0 (mod N) the rows reach it in the LAST row of the comb, at column 21 with G's entry (test_keyset_adversarial.py asserts
both places)."""
import hashlib
import random

import adversarial_points as adv
import bucket_ref
import curve4q_oracle as o
import keyset_ref
import sig_ref

N = o.N
G = (o.Gx, o.Gy)
W, V, E, D = 9, 4, 7, 28                                    # CombShape<9, 4, 7>: planes, sub-tables, rows, columns
STRUCTURED_C = (1, N - 1, 2, N - 2, (N + 1) // 2, 1 << 7, 1 << 28, (1 << 7) + 1)
SHIFT_T = (0x5eed0001, 0x5eed0002, 0x5eed0003)              # seeds of the three honest keys of "shifted"
STATES = ("add cancels", "add to neutral", "add as doubling", "dbl of neutral")
_cache = {}


# ---- the C oracle -------------------------------------------------------------------------------------------------------------------
def multiples_of_g(scalars):
    """(n, 32) uint8: encode([s]G) through the C oracle (oracle_c.mul + r1_to_affine + encode), s taken modulo N"""
    import oracle_c as oc
    from fourq_amd import codec
    if "table" not in _cache:
        _cache["table"] = oc.table(oc.ENDO, codec.pack_point(sig_ref.G1))
    words = codec.pack_scalars([s % N for s in scalars])
    return oc.encode(oc.r1_to_affine(oc.mul(oc.ENDO, words, None, _cache["table"])))


# ---- the families: lists of (label, 32 bytes) -----------------------------------------------------------------------------------------
def strings():
    if "strings" not in _cache:
        _cache["strings"] = [("%s: %s" % (fam, label), b) for fam, label, b in adv.all_strings()]
    return _cache["strings"]


def shift_keys():
    """the three honest keys of "shifted": (t, affine [t]G)"""
    if "shift_keys" not in _cache:
        ts = [random.Random(seed).getrandbits(256) % N for seed in SHIFT_T]
        _cache["shift_keys"] = [(t, o.R1toAffine(o.MUL_endo(t, sig_ref.G1))) for t in ts]
    return _cache["shift_keys"]


def shift_points():
    """(label, label of T or None, point): A + T for every honest key and every T != O, then (-x, -y) of every honest key"""
    if "shift_points" not in _cache:
        out = []
        for j, (_, A) in enumerate(shift_keys()):
            for label, T in adv.torsion():
                if T != adv.NEUTRAL:
                    out.append(("key %d + %s" % (j, label), label, adv.point_add(A, T)))
        for j, (_, A) in enumerate(shift_keys()):
            out.append(("key %d as (-x, -y)" % j, None, (o.f2_neg(A[0]), o.f2_neg(A[1]))))
        _cache["shift_points"] = out
    return _cache["shift_points"]


def shifted():
    return [(label, adv.encode(pt)) for label, _, pt in shift_points()]


def honest_shift_strings():
    return [adv.encode(A) for _, A in shift_keys()]


def c_name(c):
    for base, name in ((N, "N"), ((N + 1) // 2, "(N+1)/2")):
        if abs(c - base) <= 2:
            return name + ("" if c == base else "%+d" % (c - base))
    return adv.word_name(c)


def structured():
    if "structured" not in _cache:
        enc = multiples_of_g(STRUCTURED_C)
        _cache["structured"] = [("[%s]G" % c_name(c), enc[i].tobytes()) for i, c in enumerate(STRUCTURED_C)]
    return _cache["structured"]


def families():
    return {"strings": strings(), "shifted": shifted(), "structured": structured()}


def all_keys():
    """(family, label, 32 bytes) of every key, in the fixture's order"""
    return [(name, label, b) for name, fam in families().items() for label, b in fam]


def keys_sha256():
    return hashlib.sha256(b"".join(b for _, _, b in all_keys())).hexdigest()


def key_statuses(keys):
    """keyset_ref.key_status of every string, equal strings computed once"""
    memo = _cache.setdefault("status", {})
    out = []
    for b in keys:
        b = bytes(b)
        if b not in memo:
            memo[b] = keyset_ref.key_status(b)
        out.append(memo[b])
    return out


# ---- the scalar rows of the structured keys ---------------------------------------------------------------------------------------------
def structured_rows():
    """(key index, k, l, how): per key, k over the edge scalars and four seeded 256-bit values (two with an odd and two with an even residue
    modulo N) with l = k, l = N - (k mod N), l = -k / c (the result is the neutral point), l = 0 and the pair (0, k); and one seeded pair"""
    if "rows" in _cache:
        return _cache["rows"]
    rows = []
    for j, c in enumerate(STRUCTURED_C):
        rng = random.Random(7700 + j)
        seeded = []
        while len(seeded) < 4:
            k = rng.getrandbits(256)
            if (k % N) % 2 == (len(seeded) < 2):
                seeded.append(k)
        for k in list(bucket_ref.EDGE_SCALARS) + seeded:
            rows += [(j, k, k, "l = k"), (j, k, N - k % N, "l = N - k"), (j, k, -k * pow(c, -1, N) % N, "l = -k / c"), (j, k, 0, "l = 0"),
                     (j, 0, k, "k = 0")]
        rows.append((j, rng.getrandbits(256), rng.getrandbits(256), "seeded pair"))
    _cache["rows"] = rows
    return rows


def parities(k, l):
    return (k % N) % 2, (l % N) % 2


# ---- the walk of keyset_comb_kernel in integers modulo N --------------------------------------------------------------------------------
def columns(m):
    """per column 0 .. 27 of the recoding of m: (sign with the even-scalar negation folded in, table index u as its eight bits' value)"""
    from test_adversarial_scalars import comb_model
    negated, _, planes, _, carry = comb_model(m, W, D)
    assert carry == 0
    flip = -1 if negated else 1
    return [(flip * (1 if (planes[0] >> col) & 1 else -1), sum(((planes[r] >> col) & 1) << (r - 1) for r in range(1, W))) for col in range(D)]


def entry_scalar(j, u):
    """the scalar of entry u of sub-table j: 2^(7 j) (1 + sum_r u_r 2^(28 (r + 1)))"""
    return (1 << (E * j)) * (1 + sum(((u >> r) & 1) << (D * (r + 1)) for r in range(W - 1)))


def walk(k, l, c, trace=None):
    """[k]G + [l]A for A = [c]G as keyset_comb_kernel walks it: rows i = 6 .. 0, sub-tables j = 0 .. 3, column 7 j + i; one doubling at
    j = 0 except in the first row; G's entry first (the very first one starts the accumulator), then c times the key's.  Returns (the final
    value modulo N, {state: count}); trace, a list, receives (state, column, "G" or "A") for every special case."""
    cg, ca = columns(k), columns(l)
    counts = dict.fromkeys(STATES, 0)

    def note(state, col, which):
        counts[state] += 1
        if trace is not None:
            trace.append((state, col, which))

    acc = None
    for i in range(E - 1, -1, -1):
        for j in range(V):
            col = E * j + i
            if j == 0 and acc is not None:
                if acc == 0:
                    note("dbl of neutral", col, "")
                acc = 2 * acc % N
            for which, (sign, u), times in (("G", cg[col], 1), ("A", ca[col], c)):
                e = sign * entry_scalar(j, u) * times % N
                if acc is None:
                    acc = e                                 # affine_table_start: the accumulator IS the first entry
                    continue
                if acc == 0:
                    note("add to neutral", col, which)
                elif (acc + e) % N == 0:
                    note("add cancels", col, which)
                elif acc == e:
                    note("add as doubling", col, which)
                acc = (acc + e) % N
    return acc, counts


# ---- expectations -------------------------------------------------------------------------------------------------------------------------
def group_law_bytes(ks, ls, ts):
    """(n, 32) uint8: encode([k + l t]G) for keys [t]G, the sum in Python integers and the point from the C oracle"""
    out = multiples_of_g([k + l * t for k, l, t in zip(ks, ls, ts)])
    for i, (k, l, t) in enumerate(zip(ks, ls, ts)):
        if (k + l * t) % N == 0:
            assert out[i].tobytes() == keyset_ref.NEUTRAL_BYTES
    return out


def sign_with_logarithm(c, pk, msg, r):
    """a signature under the key [c]G from its logarithm: R = [r]G, s = r - c h mod N"""
    R = multiples_of_g([r])[0].tobytes()
    h = sig_ref.challenge(R, pk, msg)
    return R + ((r - c * h) % N).to_bytes(32, "little")
