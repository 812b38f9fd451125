"""Sequences of calls on ONE context with no synchronisation between them, and the state a context carries from one call to the next
(fourq_amd/csrc/fourq_amd.hip, struct fourq_ctx): the staged fixed-base table and comb with their host shadows, the work buffer that
eighteen layouts carve differently (work_layout.h and the later families' *_layout.h and msm_shape.h: Keyset, Commit, Bucket, MsmRagged, Dleq,
Vrf and Shamir, whose own regions start behind an inner_extent and nest up to three deep) and that grows by free + allocate, the objects
that synchronous setters replace -- the key set, the commitment bases, the ragged shape --, the projective planes, scratch and the staging
buffer, the selection mode read at enqueue, and the chunk plans a multi-chunk host call leaves for the next one.

The shape of every test: every step's inputs are uploaded and its outputs allocated -- separate device tensors pre-filled with 0xA5 --
before the first call; then all steps are enqueued with nothing in between (no .cpu(), no torch.cuda.synchronize, no host-array call
unless the test is about one); then ONE eng.sync(); then every step's bytes are compared with the oracle's, and a failure names the step's
index and kind.  The steps and their expectations are built by tests/call_sequences.py; nothing expected comes from the library.
Every test makes its own Engine(0), in both selection modes.

Sections 1 to 7 are the first families'; sections 8 to 13 put the later families into sequences: behind dirt that a predecessor left in
the bytes they carve (the regions they read or merge into before their own kernels write them depend on one memset each), with the selection
mode flipped, on a growing buffer, around host-array calls, and with the objects replaced while calls over the old ones are in flight.
tests/test_call_sequence_table.py checks on the CPU that the table is complete and that the dirt lies where those layouts carve."""
import re
import random

import numpy as np
import pytest

import call_sequences as cs
from call_sequences import KINDS, STATE_KINDS, State, run
from fourq_amd import _lib

pytestmark = pytest.mark.gpu

MODES = {"select-by-address": False, "constant-time": True}


def new_engine(ct):
    from fourq_amd import Engine
    e = Engine(0)
    e.ct_select = ct
    assert e.ct_select == ct
    cs.data(e.lanes // 2 + 1)                        # the pool every step slices, once per process: as long as the largest batch of this module
    return e


@pytest.fixture(params=list(MODES.values()), ids=list(MODES))
def fresh(request):
    """a new context per test: no call before the test's first, no reserve, nothing staged"""
    e = new_engine(request.param)
    yield e
    e.close()


@pytest.fixture(params=list(MODES.values()), ids=list(MODES))
def fresh_deferring(request, monkeypatch):
    """... on which every variable-base DH batch that runs on the one-lane kernels defers its normalisation into the projective planes
    (FOURQ_NORM_K=2, a routing hook read at context creation), as only batches of two generations do otherwise"""
    monkeypatch.setenv("FOURQ_NORM_K", "2")
    e = new_engine(request.param)
    yield e
    e.close()


class Steps:
    """builds a test's steps in order, so that the State (which comb NULL means) follows the calls"""

    def __init__(self, seed):
        self.st, self.rng, self.plans = State(), random.Random(seed), []

    def add(self, name, n=0, **kw):
        self.plans.append(cs.build(name, min(n, KINDS[name].cap or n), self.st, self.rng, **kw))      # restatement-backed kinds stay at 257 rows
        return self


# ---- 1. tables and combs that change between unsynchronised calls ----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 257, 4099])
def test_tables_and_combs_change_between_unsynchronised_calls(fresh, n):
    """Every step's output is that of the table given in THAT call: the memcmp against the shadow, the one shadow_read event both shadows
    share, comb == NULL = whatever is staged.  fourq_comb_table / fourq_table_* for a third point run kernels over scratch, comb_packed and
    table_packed in the middle; what is staged stays staged (include/fourq_amd.h says so), and the returned tables are the oracle's."""
    s = Steps(100 + n)
    s.add("fixed", n, algo="endo", base="G").add("fixed", n, algo="windowed", base="P2").add("fixed", n, algo="endo", base="P2").add("fixed", n, algo="endo", base="G")
    s.add("dh", n, algo="endo", table392="G").add("dh", n, algo="endo", table392=None).add("exchange", n, base="P2", with_table=True)
    s.add("comb_mul", n, comb="G").add("comb_mul", n, comb="P2").add("comb_mul", n, comb=None)
    s.add("fixed", n, algo="endo", base="P2")
    s.add("tables_of_p3")
    s.add("comb_mul", n, comb=None)                              # still P2's
    s.add("fixed", n, algo="endo", base="P2")                    # the same 1 KiB as before the table calls: not staged again, and still P2's
    s.add("comb_stage", comb="G").add("sig_keygen", n, comb=None)
    s.add("double_mul_bytes", n, comb="P2").add("verify_bytes", n, comb=None)
    s.add("mixed", n, base="G").add("mixed", n, base="P2")
    s.add("exchange_comb", n, comb="G392").add("comb_mul", n, comb=None).add("sig_sign", n, comb="G").add("sig_verify", n, comb=None)
    assert s.plans[12].note == "comb=None (P2)"
    run(fresh, s.plans)


# ---- 2. set_stream ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 4099])
def test_set_stream_between_unsynchronised_runs(fresh, n):
    """sync, switch to a torch stream, go on there -- comb == NULL (staged again from the shadow by the context itself), the same and a
    changed fixed-base table -- with a producer on that stream (add_ on the scalars) directly in front of a _dev call; sync, switch back
    with set_stream(None), go on."""
    s = Steps(200 + n)
    s.add("fixed", n, algo="endo", base="G").add("comb_mul", n, comb="G").add("dh", n, algo="endo", table392="G")
    s.add("set_stream", side=True)
    s.add("comb_mul", n, comb=None).add("fixed", n, algo="endo", base="G").add("fixed", n, algo="endo", base="P2")
    s.add("mul_r1", n, algo="endo", producer=True).add("comb_mul", n, comb=None, producer=True)
    s.add("double_mul", n, comb="P2").add("dh", n, algo="endo", table392="P2").add("mul_bytes", n, algo="endo")
    s.add("set_stream", side=False)
    s.add("comb_mul", n, comb=None).add("fixed", n, algo="endo", base="P2").add("fixed", n, algo="windowed", base="G")
    s.add("verify_bytes", n, comb=None).add("mixed", n, base="G").add("sig_keygen", n, comb="G")
    run(fresh, s.plans)


# ---- 3. regions of the work buffer that different layouts share ------------------------------------------------------------------------
SUCCESSORS = [("oprf_blind", {}), ("hash_to_curve", {"mode": "ro", "affine": False}), ("msm_bytes", {}), ("dh_bytes", {"algo": "endo"}), ("sig_verify", {"comb": "G"}),
              ("oprf_finalize", {}), ("oprf_eval", {})]
REJECTING = [("dh_bytes", {"algo": "endo"}), ("msm_bytes", {"groups": 1}), ("msm_bytes", {}), ("sig_verify", {"comb": "G"}), ("oprf_finalize", {}), ("oprf_evaluate", {})]


@pytest.mark.parametrize("before,after", [(1, 1), (257, 257), (257, 256)])
def test_a_successor_finds_the_predecessors_bytes_where_it_expects_its_own(fresh, before, after):
    """mul_bytes_dev with every point undecodable leaves the decode codes 1, 2, 3 in MulRows::st_decode (from byte 384 n) and non-zero rows
    below it; each successor carves the same bytes its own way directly behind it, at the same n and at a smaller one.  Its statuses and
    outputs are the restatement's, 0 for every valid row."""
    s = Steps(300 + before + after)
    for name, kw in SUCCESSORS:
        s.add("mul_bytes", before, algo="endo", bad=True).add(name, after, **kw)
    run(fresh, s.plans)


@pytest.mark.parametrize("n", [1, 257])
def test_mul_bytes_behind_a_call_that_rejected_rows(fresh, n):
    s = Steps(350 + n)
    for name, kw in REJECTING:
        s.add(name, n, bad=True, **kw).add("mul_bytes", n, algo="endo").add("mul_bytes", n, algo="windowed")
    run(fresh, s.plans)


# ---- 4. growth and shrinkage ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reserve", [False, True], ids=["grown on demand", "reserved first"])
def test_buffers_grow_under_calls_in_flight(fresh_deferring, reserve):
    """work and proj are grown by synchronise + free + allocate inside the call that needs more (257 -> lanes / 4 + 1 -> lanes / 2 + 1: the
    four-lane, two-lane and one-lane routes), while the previous calls are still in flight; the staging buffer grows under FP2_MUL calls of
    64, 5 000 and 70 000 rows in the same run.  The outputs of the earlier, smaller calls are intact at the end."""
    eng = fresh_deferring
    quarter, half = eng.lanes // 4 + 1, eng.lanes // 2 + 1
    s = Steps(400)
    if reserve:
        s.add("reserve", half)
    trio = lambda n, comb: s.add("mul_affine", n, algo="endo").add("dh", n, algo="endo", table392=None).add("double_mul", n, comb=comb)
    trio(257, "G")
    s.add("mul_affine", quarter, algo="endo").add("prim", 64).add("dh", quarter, algo="endo", table392=None).add("double_mul", quarter, comb=None)
    trio(257, None)
    s.add("mul_affine", half, algo="endo").add("dh", half, algo="endo", table392=None).add("prim", 5000).add("double_mul", half, comb=None)
    s.add("mul_affine", 1, algo="endo").add("prim", 70000).add("dh", 1, algo="endo", table392=None).add("double_mul", 1, comb=None)
    run(eng, s.plans)


# ---- 5. the selection mode toggled between unsynchronised calls ------------------------------------------------------------------------
def test_selection_mode_flips_before_every_call(fresh):
    """fourq_ctx::ct is read at enqueue and selects another translation unit's kernels over the same scratch, tables and planes"""
    s = Steps(500)
    for n in (4099, 257, 1):
        s.add("ct_flip").add("mul_r1", n, algo="endo").add("ct_flip").add("comb_mul", n, comb="G" if n == 4099 else None)
        s.add("ct_flip").add("dh", n, algo="endo", table392=None).add("ct_flip").add("mixed", n, base="P2")
        s.add("ct_flip").add("fixed", n, algo="endo", base="P2").add("ct_flip").add("dh", n, algo="endo", table392="G").add("ct_flip")
    run(fresh, s.plans)


# ---- 6. host-array calls in between -------------------------------------------------------------------------------------------------------
def test_host_array_calls_between_dev_calls_in_flight(fresh):
    """_dev calls in flight, directly followed by a host-array call on the same context -- the zero-copy size 7, the one-chunk size 2 978,
    the multi-chunk size 2 x lanes + 77 (three times: planned from the first-call guesses, then twice from its own measurements; identical
    bytes each time) -- then more _dev calls whose inputs were on the device before the host call."""
    eng = fresh
    s = Steps(600)
    s.add("mul_r1", 4099, algo="endo").add("dh", 4099, algo="endo", table392=None).add("double_mul", 257, comb="G")
    s.add("host_mul", 7)
    s.add("comb_mul", 4099, comb=None).add("mul_affine", 4099, algo="endo")
    s.add("host_dh_bytes", 7)
    s.add("mixed", 4099, base="G").add("oprf_blind", 257)
    s.add("host_mul", 2978)
    s.add("dh_bytes", 257, algo="endo").add("fixed", 4099, algo="endo", base="G")
    s.add("host_dh_bytes", 2978)
    s.add("exchange_comb", 257, comb="G392").add("mul_bytes", 4099, algo="endo")
    for _ in range(3):
        s.add("host_mul", 2 * eng.lanes + 77)
    s.add("mul_r1", 4099, algo="windowed").add("comb_mul", 257, comb=None).add("fixed", 4099, algo="endo", base="G")
    rt = cs.Runtime()
    live = run(eng, s.plans, rt)
    stats = rt.host_stats                            # of each host call, read right behind it
    assert [st["chunks"] > 1 for st in stats] == [False] * 4 + [True] * 3, [st["chunks"] for st in stats]
    assert [st["planned_from_measurement"] for st in stats[4:]] == [0, 1, 1]
    big = [x.host[0] for x in live if x.plan.kind == "host_mul" and x.plan.n > 2978]
    assert len(big) == 3 and np.array_equal(big[0], big[1]) and np.array_equal(big[0], big[2])


# ---- 7. seeded sequences over every _dev family and every change of state ----------------------------------------------------------------
def test_the_step_table_names_every_dev_entry_point():
    named = {e for k in KINDS.values() for e in k.entries}
    declared = {name for name in _lib.PROTOTYPES if name.endswith("_batch_dev")}
    assert declared and named >= declared, sorted(declared - named)
    declared = {name for name in _lib.PROTOTYPES if name.endswith("_dev")}            # ... and the later families' names, which end in _dev alone
    assert named == declared, (sorted(declared - named), sorted(named - declared))
    assert set(STATE_KINDS) == {name for name, k in KINDS.items() if not k.entries}
    cs.check_entry_points()
    cs.check_state_calls()


SEEDS = [20261019, 20261020, 20261021]
LATER_SEEDS = [20261101, 20261102, 20261109]            # drawn from the whole table, LATER_STEPS steps each
LATER_STEPS = 60


@pytest.fixture(scope="module")
def restated():
    """the later families' restated expectations: seconds of CPU time once per process, spent here and not inside whichever test asks first"""
    return cs.restated()


@pytest.fixture
def later(fresh, restated):
    """a fresh context for the later families' tests"""
    return fresh


def test_the_three_seeds_reach_every_kind_of_step(restated):
    first = {p.kind for seed in SEEDS for p in cs.seeded_sequence(seed)}
    assert first == set(cs.FIRST_KINDS)                                                  # as ever: the first three reach the table they were chosen for
    assert first | {p.kind for seed in LATER_SEEDS for p in cs.seeded_sequence(seed, LATER_STEPS, True)} == set(KINDS)


@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_sequences_unsynchronised_and_synchronised(fresh, seed):
    """40 steps drawn from the table, n from {1, 7, 257, 4099}: once with no sync until the end, once -- on another fresh context -- with a
    sync behind every step.  Both equal the expectations, and therefore each other."""
    plans = cs.seeded_sequence(seed)
    assert len(plans) == 40
    ct = fresh.ct_select
    run(fresh, plans)
    again = new_engine(ct)
    try:
        run(again, plans, sync_each=True)
    finally:
        again.close()


@pytest.mark.parametrize("seed", LATER_SEEDS)
def test_seeded_sequences_over_the_whole_table(later, seed):
    """LATER_STEPS steps drawn from every kind, the later families' and their objects included, a state kind every third step: once with
    no sync until the end, once -- on another fresh context -- with a sync behind every step."""
    plans = cs.seeded_sequence(seed, LATER_STEPS, True)
    assert len(plans) == LATER_STEPS
    ct = later.ct_select
    run(later, plans)
    again = new_engine(ct)
    try:
        run(again, plans, sync_each=True)
    finally:
        again.close()


# ---- 8. the object a call was enqueued with is the object it uses ------------------------------------------------------------------------
def installed_nowhere_but_in_state_steps(plans):
    return not [p.note for p in plans if "installed here" in p.note]


def test_the_object_a_call_was_enqueued_with_is_the_object_it_uses(later):
    """Keyed calls over set A in flight, fourq_keyset_set(B) with no sync by the test, keyed calls over B; the same for two sets of
    commitment bases and two ragged shapes.  The setters are synchronous and free the old arrays: every output is the restatement's for
    the object installed at its enqueue.  The generator's staged comb and the staged fixed-base table serve comb == NULL and table calls
    afterwards: the setters leave them alone (include/fourq_amd.h)."""
    s = Steps(800)
    s.add("comb_stage", comb="G").add("fixed", 257, algo="endo", base="P2")
    s.add("keyset_set", keyset="A").add("keyed_verify", 257, comb=None).add("keyed_double_mul", 257, comb=None).add("vrf_verify_keyed", 257, comb=None)
    s.add("keyset_set", keyset="B").add("keyed_verify", 257, comb=None).add("keyed_double_mul", 257, comb=None).add("vrf_verify_keyed", 257, comb=None)
    s.add("keyset_set", keyset="A").add("keyed_verify", 257, comb=None)
    s.add("commit_bases", bases="A").add("commit", 257, size=7, route=1, flavour="affine").add("commit", 257, size=1, route=2, flavour="bytes")
    s.add("commit_bases", bases="B").add("commit", 257, size=65, route=0, flavour="affine").add("commit", 257, size=7, route=1, flavour="bytes")
    s.add("msm_shape", shape="mid").add("ragged", 257, flavour="affine").add("ragged", 257, flavour="bytes", bad=True)
    s.add("msm_shape", shape="seven").add("ragged", 257, flavour="bytes").add("ragged", 257, flavour="affine")
    s.add("comb_mul", 257, comb=None).add("fixed", 257, algo="endo", base="P2").add("sig_keygen", 257, comb=None).add("keyed_verify", 257, comb=None)
    assert installed_nowhere_but_in_state_steps(s.plans) and [p.n for p in s.plans if p.kind == "ragged"] == [257, 257, 7, 7]
    assert [p.n for p in s.plans if p.kind == "keyed_verify"] == [65, 257, 65, 65]
    run(later, s.plans)


# ---- 9. the later layouts behind dirt -------------------------------------------------------------------------------------------------
def add_with_its_object_first(s, name, n, kw):
    """the successor's key set, bases or shape installed by a state step of its own, in FRONT of the predecessor: nothing runs between the two"""
    for key, state_kind, have in (("keyset", "keyset_set", s.st.keyset), ("bases", "commit_bases", s.st.bases), ("shape", "msm_shape", s.st.shape)):
        if key in kw and kw[key] != have:
            s.add(state_kind, **{key: kw[key]})
    return s


@pytest.mark.parametrize("rows,bad", [(cs.DIRT_ROWS, False), (257, True), (cs.DIRT_ROWS, True)], ids=["valid 4099", "undecodable 257", "undecodable 4099"])
def test_the_later_layouts_behind_dirt(later, rows, bad):
    """The counterpart of test_a_successor_finds_the_predecessors_bytes_where_it_expects_its_own for the seven later layouts.  A valid
    mul_bytes_dev at 4 099 rows leaves full R1 rows in bytes [0, 320 x 4099) of the work buffer -- all of every successor's layout
    (tests/test_call_sequence_table.py checks that on the CPU) --, an all-undecodable one the codes 1, 2, 3 from byte 384 n.  The
    successors' flags, counts, group codes, merged statuses and pre-statuses start from those bytes unless their call zeroes them."""
    s = Steps(810 + rows + bad)
    s.add("comb_stage", comb="G")
    for name, kw, _ in cs.DIRT_SUCCESSORS:
        add_with_its_object_first(s, name, 257, kw).add("mul_bytes", rows, algo="endo", bad=bad).add(name, 257, **kw)
    assert installed_nowhere_but_in_state_steps(s.plans)
    run(later, s.plans)


def test_mul_bytes_and_every_other_later_family_behind_one_that_rejected_rows(later):
    """the reverse pair: each later family with refused, spoiled or undecodable rows, directly followed by mul_bytes (endo and windowed)
    and -- every ordered pair once -- by each other later family"""
    s = Steps(820)
    s.add("comb_stage", comb="G").add("keyset_set", keyset="B").add("commit_bases", bases="A").add("msm_shape", shape="mid")
    for name, kw in cs.DIRT_REJECTING:
        s.add(name, 257, **kw).add("mul_bytes", 257, algo="endo").add("mul_bytes", 257, algo="windowed")
    for name, kw in cs.DIRT_REJECTING:
        for after, kw_after in cs.DIRT_REJECTING:
            if after != name:
                s.add(name, 257, **kw).add(after, 257, **kw_after)
    assert installed_nowhere_but_in_state_steps(s.plans)
    run(later, s.plans)


# ---- 10. the selection mode flipped before every call over the later families ------------------------------------------------------------
FLIPPED = [("keyed_verify", {"keyset": "B"}), ("commit", {"size": 7, "route": 1}), ("bucket", {"size": 65, "window": 4}), ("ragged", {"shape": "mid"}),
           ("vrf_verify_keyed", {"keyset": "B"}), ("shamir_verify", {"t": 3}), ("keyed_double_mul", {"keyset": "B"}), ("commit", {"size": 65, "route": 2, "bases": "B"}),
           ("bucket", {"size": 7, "window": 5, "flavour": "bytes", "bad": True})]


def test_selection_mode_flips_before_every_call_over_the_later_families(later):
    """The key set's and the bases' combs serve both modes; the keyed calls switch between the comb route and the gathered unkeyed route
    (the VRF's keyed verify nests three deep there), the bucket route falls back to the ladders under constant-time selection."""
    s = Steps(830)
    for n in (257, 7):
        for name, kw in FLIPPED:
            s.add("ct_flip").add(name, n if n > 7 or "size" not in kw else kw["size"], **kw)
    s.add("ct_flip")
    run(later, s.plans)


# ---- 11. growth under the later families --------------------------------------------------------------------------------------------------
def test_the_later_families_grow_the_buffer_under_calls_in_flight(later):
    """a fresh, unreserved context at 1, then 33, then 257 rows with no sync: commit, bucket, ragged and the threshold calls each grow
    the work buffer by synchronise + free + allocate with the earlier ones in flight, dh and double_mul the planes; compared with the
    restatements, not with a second context"""
    s = Steps(840)
    for n, size, shape, t in ((1, 1, "one", 1), (33, 7, "small", 3), (257, 65, "mid", 5)):
        s.add("commit", n, size=size, route=1, flavour="bytes", bases="B").add("dh", n, algo="endo", table392=None)
        s.add("bucket", n, size=size, window=4, flavour="affine").add("ragged", n, shape=shape, flavour="affine")
        s.add("double_mul", n, comb="G" if n == 1 else None).add("shamir_verify", n, t=t).add("shamir_combine_points", n, t=t).add("shamir_shares", n, t=t, m=5)
    assert [p.n for p in s.plans if p.kind == "ragged"] == [1, 33, 257]
    run(later, s.plans)


# ---- 12. host-array calls of the later families between their _dev calls ----------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 257])
def test_host_array_calls_of_the_later_families_between_their_dev_calls(later, n):
    """one host-array call each of commit_bytes, msm_ragged_bytes, sig_verify_keyed and shamir_combine_points directly behind _dev calls
    of their families in flight, at the zero-copy size 7 and at 257, then more _dev calls whose inputs were on the device before"""
    s = Steps(850 + n)
    s.add("comb_stage", comb="G").add("keyset_set", keyset="B").add("commit_bases", bases="B").add("msm_shape", shape="mid")
    s.add("commit", 257, size=65, route=0).add("keyed_verify", 257)
    s.add("host_keyed", n, which="commit_bytes", size=7, bases="A")
    s.add("commit", 257, size=7, route=2).add("ragged", 257, flavour="bytes")
    s.add("host_keyed", n, which="msm_ragged_bytes")
    s.add("ragged", 257, flavour="affine").add("vrf_verify_keyed", 257)
    s.add("host_keyed", n, which="sig_verify_keyed", keyset="B")
    s.add("keyed_double_mul", 257).add("shamir_verify", 257, t=3)
    s.add("host_keyed", n, which="shamir_combine_points", t=3)
    s.add("shamir_combine_points", 257, t=5).add("keyed_verify", 257).add("commit", 257, size=1, route=1)
    rt = cs.Runtime()
    run(later, s.plans, rt)
    assert len(rt.host_stats) == 4


# ---- 13. the harness can fail --------------------------------------------------------------------------------------------------------
def test_one_flipped_expected_byte_names_its_step_and_no_other(later):
    s = Steps(860)
    s.add("commit", 7, size=7, route=1, flavour="bytes", bases="A").add("keyed_verify", 7, keyset="B", comb="G").add("shamir_lagrange", 7, t=3).add("ragged", 7, shape="seven")
    plans = list(s.plans)
    p = plans[2]
    label, want = p.wants[0]
    wrong = want.copy()
    wrong.view(np.uint8).reshape(-1)[9] ^= 1
    plans[2] = cs.Plan(p.kind, p.n, p.ins, [(label, wrong)] + list(p.wants[1:]), p.call, p.host_wants, p.note)
    with pytest.raises(AssertionError) as caught:
        run(later, plans)
    message = str(caught.value)
    assert "step 2 shamir_lagrange" in message and re.findall(r"step (\d+)", message) == ["2"] and label + " differs in 1 rows" in message
    run(later, s.plans)                              # ... and with the expectation as built, the same steps pass
