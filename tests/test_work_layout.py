"""The work-buffer layouts of the protocol-level calls (fourq_amd/csrc/work_layout.h, plain C++): compiled with g++ and checked on the CPU.
Every region starts 16-byte aligned, the regions of a layout are disjoint and end within bytes(n), and bytes(n) is the formula the library has
always allocated by, restated here as literals -- the size at which the context's work buffer is reallocated is behaviour.  What each region
must hold is restated here too, from the kernels that write it: 8 words per affine point, 20 per R1 row, 32 bytes per string or scalar,
one status byte per element."""
import os
import subprocess

import pytest

from conftest import ROOT

SIZES = [1, 2, 255, 256, 257, 4095, 65537, 0xffffff00]


def a(n):
    return (n + 255) // 256 * 256


# bytes each region's users read or write for n elements
NEED = {
    "dh_bytes": {"pts": lambda n: n * 64, "shared": lambda n: n * 64, "st_decode": lambda n: n, "st_dh": lambda n: n},
    "exchange": {"base_pts": lambda n: n * 64, "mid": lambda n: n * 64, "st_first": lambda n: n},
    "mul_rows": {"rows_in": lambda n: n * 160, "rows_out": lambda n: n * 160, "unused": lambda n: n * 64, "st_decode": lambda n: n},
    "double_mul": {"rows_in": lambda n: n * 160, "rows_out": lambda n: n * 160, "st_decode": lambda n: n, "st_comb": lambda n: n,
                   "tail": lambda n: 3 * n * 32 + a(n)},
    "sig_verify": {"rows_in": lambda n: n * 160, "rows_out": lambda n: n * 160, "st_decode": lambda n: n, "st_comb": lambda n: n,
                   "sig.s": lambda n: n * 32, "sig.h": lambda n: n * 32, "sig.r32": lambda n: n * 32, "sig.pre": lambda n: n},
    "sig": {"a": lambda n: n * 32, "r": lambda n: n * 32, "r32": lambda n: n * 32, "affine": lambda n: n * 64, "st_comb": lambda n: n},
    "h2c": {"u": lambda n: 2 * n * 32},
}
# the totals the library allocated by before the layouts had a header of their own
BYTES = {
    "dh_bytes": lambda n: 2 * n * 64 + 2 * a(n),
    "exchange": lambda n: 2 * n * 64 + a(n),
    "mul_rows": lambda n: 2 * n * 160 + n * 64 + a(n),
    "double_mul": lambda n: 2 * n * 160 + 2 * a(n) + 3 * n * 32 + a(n),
    "sig_verify": lambda n: 2 * n * 160 + 2 * a(n) + 3 * n * 32 + a(n),
    "sig": lambda n: 3 * n * 32 + n * 64 + a(n),
    "h2c": lambda n: 2 * n * 32,
}


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("work_layout") / "work_layout_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "fourq_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "work_layout_dump.cpp"), "-o", exe], check=True)
    cache, shared = {}, {}

    def run(n):
        if n not in cache:
            regions, totals, listed = {}, {}, {}
            shared[n] = {"extent": {}, "lent": {}}
            for line in subprocess.run([exe, str(n)], check=True, capture_output=True, text=True).stdout.splitlines():
                layout, name, value = line.split()
                if layout in ("extent", "lent"):      # how the layout shares the buffer with the calls its call makes: layout -> bytes
                    shared[n][layout][name] = int(value)
                elif layout == "list":                # the header's list of all layouts: struct name -> total, and "max_bytes"
                    listed[name] = int(value)
                elif name == "bytes":
                    totals[layout] = int(value)
                else:
                    regions.setdefault(layout, {})[name] = int(value)
            cache[n] = (regions, totals, listed)
        return cache[n]
    run.shared = lambda n: (run(n), shared[n])[1]
    return run


@pytest.mark.parametrize("n", SIZES)
def test_regions_are_aligned_disjoint_and_inside_the_total(layouts, n):
    regions, totals, _ = layouts(n)
    assert set(regions) == set(NEED) == set(totals)
    for layout, offs in regions.items():
        assert set(offs) == set(NEED[layout]), layout
        spans = sorted((off, off + NEED[layout][name](n), name) for name, off in offs.items())
        for off, end, name in spans:
            assert off % 16 == 0, (layout, name, off)
            assert end <= totals[layout], (layout, name, end, totals[layout])
        for (_, end, name), (off, _, nxt) in zip(spans, spans[1:]):
            assert end <= off, (layout, name, nxt)


@pytest.mark.parametrize("n", SIZES)
def test_totals_are_the_formulas_the_library_allocated_by(layouts, n):
    regions, totals, _ = layouts(n)
    for layout, formula in BYTES.items():
        assert totals[layout] == formula(n), layout
    # the signature check is the double multiplication plus a tail: same total (double_mul_dev, called with the buffer already sized by
    # fourq_sig_verify_batch_dev, does not move it), the same four regions, and the tail begins where they end
    dm, sv = regions["double_mul"], regions["sig_verify"]
    assert totals["sig_verify"] == totals["double_mul"]
    assert all(sv[name] == dm[name] for name in ("rows_in", "rows_out", "st_decode", "st_comb"))
    assert sv["sig.s"] == dm["tail"] == dm["st_comb"] + a(n) == 2 * n * 160 + 2 * a(n)
    # two offsets the kernels' callers have always used
    assert regions["mul_rows"]["st_decode"] == 2 * n * 160 + n * 64
    assert regions["sig"]["affine"] == 3 * n * 32


# who calls whom with a work layout of its own, restated from fourq_amd.hip: composite -> [(inner layout, the size it is called with)]
CALLS = {"sig_verify": [("double_mul", lambda n: n)]}


@pytest.mark.parametrize("n", SIZES)
def test_the_inner_extent_is_the_first_own_region_and_holds_every_inner_call(layouts, n):
    """The bytes from the buffer's start that a layout admits for the calls its call makes (work_layout.h, the rule): nothing for a layout
    whose call makes none, the offset of the first own region for a composite -- here the signature check, whose own regions are the tail
    -- and at least what every inner call carves at the size it is called with.  The double multiplication's total includes that very tail,
    which it lends to the signature check and never touches: nested, it has to fit without it, and that is exactly the extent."""
    regions, totals, _ = layouts(n)
    extent, lent = layouts.shared(n)["extent"], layouts.shared(n)["lent"]
    assert set(extent) == set(lent) == set(NEED)
    for layout in NEED:
        assert extent[layout] == (regions["sig_verify"]["sig.s"] if layout == "sig_verify" else 0), layout
        assert lent[layout] == (3 * n * 32 + a(n) if layout == "double_mul" else 0), layout
    assert lent["double_mul"] == totals["double_mul"] - regions["double_mul"]["tail"] == NEED["double_mul"]["tail"](n)
    for outer, inner_calls in CALLS.items():
        for inner, size in inner_calls:
            m = size(n)
            inner_regions, inner_totals, _ = layouts(m)
            assert extent[outer] >= inner_totals[inner] - layouts.shared(m)["lent"][inner], (outer, inner)
            # ... and nothing the inner call reads or writes lies outside it
            assert all(off + NEED[inner][name](m) <= extent[outer] for name, off in inner_regions[inner].items() if name != "tail"), (outer, inner)


@pytest.mark.parametrize("n", SIZES)
def test_the_list_of_all_layouts_gives_the_largest_total(layouts, n):
    """fourq_ctx_reserve sizes the work buffer by the list's max_bytes(n): it is the largest of the members' totals, and the members'
    totals are the ones pinned above."""
    _, totals, listed = layouts(n)
    listed = dict(listed)
    most = listed.pop("max_bytes")
    assert most == max(listed.values()) == BYTES["sig_verify"](n)              # the signature check's, as it has been since it came
    for struct, label in (("DhBytes", "dh_bytes"), ("Exchange", "exchange"), ("MulRows", "mul_rows"), ("DoubleMul", "double_mul"), ("Sig", "sig"), ("H2c", "h2c")):
        assert listed[struct] == totals[label] == BYTES[label](n), struct


def test_the_list_names_every_layout_struct_of_the_header(layouts):
    """A layout left out of the list would not be counted by fourq_ctx_reserve, and the first large _dev call that uses it would synchronise
    and reallocate.  The structs of work_layout.h that carve the buffer are those with a bytes( member of their own.  Two are special: SigTail
    is carved INSIDE DoubleMul's tail (DoubleMul's total includes it) and sizes nothing itself, so it is the one struct with a total that
    the list leaves out; SigVerify has no bytes( of its own -- it inherits DoubleMul's total, which the list has."""
    import re
    text = open(os.path.join(ROOT, "fourq_amd", "csrc", "work_layout.h")).read()
    structs = {m.group(1) for m in re.finditer(r"^struct (\w+)[^\n]*\{(.*?)^\};", text, re.M | re.S) if "bytes(" in m.group(2)} - {"Carver"}
    listed = set(layouts(1)[2]) - {"max_bytes"}
    assert len(listed) == 11 and structs == listed | {"SigTail"}, sorted(structs ^ listed)
    assert re.search(r"^struct SigVerify : DoubleMul \{", text, re.M) and "SigVerify" not in structs
