"""The one filler of every hashed string (fourq_amd/csrc/sha512.hip.h: sha512_fill, ShaTail and its builder, sha512_hash_rows) on the CPU.
They are plain C++ behind one qualifier macro, so tests/c/sha_string_check.cpp includes the shipped header, compiles for the host and hashes
the cases built below; every digest is held against hashlib.sha512 of the byte string this file assembles itself, and the tail builder's
words against the bytes built here.  Shapes: padding only with 0, 4 and 8 prefix words; a tail behind 128 hashed bytes; 4 words and a tail;
both; the rows hasher with 1 row, 3 rows and a counter, and 5 rows.  Every row length 0..300, every load mode at every alignment that
allows it, DSTs of 1, 16 and 255 bytes and the two per shape that put prefix + tail + 17 on a multiple of 128 and one past it.  Every row
sits at the end of its own exact-size heap allocation, and the same program runs once more under AddressSanitizer +
UndefinedBehaviorSanitizer (stand-alone, nothing preloaded): "no byte at or past a row's length is read" fails there, not in a comment."""
import hashlib
import os
import random
import struct
import subprocess

import pytest

from conftest import ROOT

BYTES, LOAD_8, LOAD_16 = 0, 1, 2
# (alignment of the row's first byte modulo 16, load mode): each mode wherever the alignment allows it
ALIGN_MODES = [(0, LOAD_16), (0, LOAD_8), (0, BYTES), (8, LOAD_8), (8, BYTES), (1, BYTES)]
TAIL_WORDS = 35
# shape: (prefix words, has a tail, bytes hashed in front, head)
STRINGS = {0: (0, False, 0, b""), 1: (4, False, 0, b""), 2: (8, False, 0, b""),
           3: (0, True, 128, b"\x00\x80\x00"), 4: (4, True, 0, b"Finalize"), 5: (4, True, 128, b"\x00\x80\x00")}
# shape: (rows, has a counter, head)
ROWS = {6: (1, False, b"VrfOutput"), 7: (3, True, b"Composite"), 8: (5, False, b"Challenge")}
SHAPE_TAIL = 9
COUNTERS = (0, 1, 0x01020304, 0xFFFFFFFF)


def dst_lengths(prefix, head):
    """1, 16, 255 and the two that put prefix + tail + 17 on 128 k and 128 k + 1 (tail = head || DST || one length byte)"""
    d0 = -(prefix + len(head) + 1 + 17) % 128 or 128
    return [1, 16, 255, d0, d0 + 1]


def build_cases():
    rng = random.Random(512)
    heads = sorted({s[3] for s in STRINGS.values()} | {r[2] for r in ROWS.values()})
    pool = bytearray(rng.randbytes(2048))
    head_off = {}
    for h in heads:
        head_off[h] = len(pool)
        pool += h
    cases, want = [], []

    def tail_bytes(head, dst_off, dst_len):
        return head + bytes(pool[dst_off:dst_off + dst_len]) + bytes([dst_len])

    def add(shape, align, mode, length, row_off, head, dst_len, dst_off, counter, pre_off, expect):
        cases.append(struct.pack("<12I", shape, align, mode, length, row_off, len(head), head_off.get(head, 0), dst_len, dst_off, counter, pre_off, 0))
        want.append(expect)

    for shape, (pw, has_tail, before, head) in STRINGS.items():
        for dst_len in (dst_lengths(8 * pw, head) if has_tail else [0]):
            for align, mode in ALIGN_MODES:
                for length in range(301):
                    row_off, dst_off, pre_off = rng.randrange(1024), rng.randrange(1024), rng.randrange(1024)
                    s = bytes(before) + bytes(pool[pre_off:pre_off + 8 * pw]) + bytes(pool[row_off:row_off + length])
                    if has_tail:
                        s += tail_bytes(head, dst_off, dst_len)
                    add(shape, align, mode, length, row_off, head, dst_len, dst_off, 0, pre_off, hashlib.sha512(s).digest())
    for shape, (rows, has_counter, head) in ROWS.items():
        for dst_len in dst_lengths(32 * rows + (4 if has_counter else 0), head):
            for counter in (COUNTERS if has_counter else (0,)):
                dst_off, pre_off = rng.randrange(1024), rng.randrange(1024)
                s = bytes(pool[pre_off:pre_off + 32 * rows]) + (struct.pack(">I", counter) if has_counter else b"") + tail_bytes(head, dst_off, dst_len)
                add(shape, 0, BYTES, 0, 0, head, dst_len, dst_off, counter, pre_off, hashlib.sha512(s).digest())
    for head in heads[1:] + [b"\x01"]:
        if head not in head_off:
            head_off[head] = len(pool)
            pool += head
        for dst_len in (1, 2, 7, 8, 16, 254, 255):
            dst_off = rng.randrange(1024)
            t = tail_bytes(head, dst_off, dst_len)
            words = t + b"\x80" + bytes(8 * TAIL_WORDS - len(t) - 1)
            assert len(t) + 1 <= 8 * (TAIL_WORDS - 1)          # the marker lies in front of the last word, which stays zero
            add(SHAPE_TAIL, 0, BYTES, 0, 0, head, dst_len, dst_off, 0, 0, words + struct.pack("<I", len(t)))
    return bytes(pool), cases, want


def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "fourq_amd", "csrc")] + extra +
                   [os.path.join(ROOT, "tests", "c", "sha_string_check.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sha_string_check")
    pool, rows, want = build_cases()
    path = tmp / "cases.bin"
    path.write_bytes(struct.pack("<I", len(pool)) + pool + b"".join(rows))
    return tmp, str(path), rows, want


def _run_and_compare(exe, path, out, rows, want):
    proc = subprocess.run([exe, path, out], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    assert "runtime error" not in proc.stderr and "Sanitizer" not in proc.stderr, proc.stderr[-4000:]
    n_hashes = sum(len(w) == 64 for w in want)
    assert proc.stdout.split() == ["cases", str(len(rows)), "hashes", str(n_hashes)] and n_hashes > 30000
    got = open(out, "rb").read()
    assert len(got) == sum(len(w) for w in want)
    at = 0
    for row, w in zip(rows, want):
        assert got[at:at + len(w)] == w, struct.unpack("<12I", row)
        at += len(w)


def test_shipped_filler_tail_and_rows_hasher_equal_hashlib(cases):
    tmp, path, rows, want = cases
    _run_and_compare(_build(tmp, "sha_string_check", []), path, str(tmp / "out.bin"), rows, want)


def test_shipped_filler_under_the_sanitizers(cases):
    tmp, path, rows, want = cases
    exe = _build(tmp, "sha_string_check_san", ["-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=undefined"])
    _run_and_compare(exe, path, str(tmp / "out_san.bin"), rows, want)

