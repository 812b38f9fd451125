"""The probe of tests/test_gpu_asm_corners.py (tests/hip/asm_body_probe.hip), on the CPU: it compiles through fourq_amd/build.py's
compile_unit, the library units' own path (hipcc's device listing, check_register_ranges, the placement pass, the bundle), and its kernel
owns every register the generated bodies clobber.  The GPU test launches only what build_probe produced, and build_probe produces nothing
when the register check fails (compile_unit raises RegisterOwnershipError before any object exists)."""
import os
import re
import subprocess

from conftest import ROOT

PROBE_SRC = os.path.join(ROOT, "tests", "hip", "asm_body_probe.hip")


def build_probe(out_dir, src=PROBE_SRC, name="asm_body_probe", extra_flags=()):
    """compile a probe like a library unit (plus `extra_flags`) and link it into a shared object; returns its path"""
    from fourq_amd import build as fb
    obj = os.path.join(out_dir, name + ".o")
    fb.compile_unit(src, obj, fb.HIPCC_FLAGS + ["-I" + fb.SRC_DIR] + list(extra_flags))
    so = os.path.join(out_dir, "lib%s.so" % name)
    proc = subprocess.run([fb._hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so, obj], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    return so


def test_probe_owns_the_bodies_registers_and_builds(tmp_path):
    from fourq_amd import build as fb
    listing = str(tmp_path / "asm_body_probe.s")
    flags = [f for f in fb.HIPCC_FLAGS if not f.startswith("-Rpass")] + ["-I" + fb.SRC_DIR]
    subprocess.run([fb._hipcc()] + flags + ["--cuda-device-only", "-S", "-o", listing, PROBE_SRC], check=True, capture_output=True)
    fb.check_register_ranges(listing)                             # raises RegisterOwnershipError if the kernel does not own v255
    text = open(listing).read()
    assert re.search(r"\bv255\b", text)                           # the bodies' temporaries are in the kernel
    alloc = [int(x) for x in re.findall(r"\.amdhsa_next_free_vgpr\s+(\d+)", text)]
    assert len(alloc) == 1 and alloc[0] >= 256, alloc
    so = build_probe(str(tmp_path))
    assert os.path.getsize(so) > 0
