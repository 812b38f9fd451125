"""Sequences of calls on ONE context with no synchronisation between them, and the state a context carries from one call to the next
(fourq_amd/csrc/fourq_amd.hip, struct fourq_ctx): the staged fixed-base table and comb with their host shadows, the work buffer that
eleven layouts carve differently (work_layout.h) and that grows by free + allocate, the projective planes, scratch and the staging
buffer, the selection mode read at enqueue, and the chunk plans a multi-chunk host call leaves for the next one.

The shape of every test: every step's inputs are uploaded and its outputs allocated -- separate device tensors pre-filled with 0xA5 --
before the first call; then all steps are enqueued with nothing in between (no .cpu(), no torch.cuda.synchronize, no host-array call
unless the test is about one); then ONE eng.sync(); then every step's bytes are compared with the oracle's, and a failure names the step's
index and kind.  The steps and their expectations are built by tests/call_sequences.py; nothing expected comes from the library.
Every test makes its own Engine(0), in both selection modes."""
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
    assert declared and named == declared, (sorted(declared - named), sorted(named - declared))
    assert set(STATE_KINDS) == {name for name, k in KINDS.items() if not k.entries}


SEEDS = [20261019, 20261020, 20261021]


def test_the_three_seeds_reach_every_kind_of_step():
    assert {p.kind for seed in SEEDS for p in cs.seeded_sequence(seed)} == set(KINDS)


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
