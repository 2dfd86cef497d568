"""csrc/fold.h — the operand load, the wrapping add and the result store the
device fold kernels are built from — on a CPU box: scripts/test_fold_host.cpp
includes the header, is built with g++ -fsanitize=address,undefined as its
own program, and is checked against a plain Python model. Every operand ends
where its heap block ends, so a read past its length aborts the driver."""
import ctypes as C
import os
import random
import subprocess

import pytest

import rocksplicator_amd.ffi as ffi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "build", "test_fold_host")
MASK = (1 << 64) - 1
LENS = (0, 1, 3, 7, 8, 9, 16)


@pytest.fixture(scope="module")
def driver():
    os.makedirs(os.path.join(REPO, "build"), exist_ok=True)
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "scripts/test_fold_host.cpp", "-o", BIN], cwd=REPO, check=True)
    return BIN


def run(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n",
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.splitlines()


def u64le(b):
    """The model: first min(8, len) bytes, little-endian, zero-extended."""
    return int.from_bytes(b[:8], "little")


def hx(b):
    return b.hex() if b else "-"


def test_operand_load_every_length_and_misalignment(driver):
    out = run(driver, ["loads"])
    assert len(out) == 13 * 16
    seen = set()
    for line in out:
        tag, ln, mis, val = line.split()
        ln, mis = int(ln), int(mis)
        b = bytes((0xA1 + 17 * i + mis) & 0xFF for i in range(ln))
        assert tag == "load" and int(val, 16) == u64le(b), line
        seen.add((ln, mis))
    assert seen == {(ln, m) for ln in range(13) for m in range(16)}


def test_wrapping_add(driver):
    rng = random.Random(1)
    pairs = [(0, 0), (MASK, 1), (MASK, MASK), (1 << 63, 1 << 63),
             (MASK - 1, 1), (0x0123456789ABCDEF, 0xFEDCBA9876543211)]
    pairs += [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(50)]
    out = run(driver, [f"add {a:x} {b:x}" for a, b in pairs])
    assert [int(x.split()[1], 16) for x in out] == \
        [(a + b) & MASK for a, b in pairs]


def test_random_chains_fold_like_the_model(driver):
    rng = random.Random(2)
    cases = []
    for i in range(300):
        base = None if rng.random() < 0.4 else rng.randbytes(rng.choice(LENS))
        nops = rng.choice((1, 2, 3, 17, 64, 65, 200))
        ops = [rng.randbytes(rng.choice(LENS)) for _ in range(nops)]
        if i % 7 == 0:  # the sum wraps
            ops[rng.randrange(nops)] = b"\xff" * 8
            ops.append(b"\xff" * 9)
        cases.append((rng.randrange(16), base, ops))
    out = run(driver, ["fold %d %s %s" % (mis, "*" if b is None else hx(b),
                                          " ".join(hx(o) for o in ops))
                       for mis, b, ops in cases])
    assert len(out) == len(cases)
    wrapped = 0
    for line, (mis, base, ops) in zip(out, cases):
        tag, val, clen = line.split()
        total = (u64le(base) if base is not None else 0) + sum(map(u64le, ops))
        wrapped += total > MASK
        assert tag == "fold"
        assert bytes.fromhex(val) == (total & MASK).to_bytes(8, "little"), \
            (mis, base, ops)
        concat = b",".join(([base] if base is not None else []) + ops)
        assert int(clen) == len(concat)
    assert wrapped > 20


def test_engine_opts_layout_matches_the_header(driver):
    tag, size, off = run(driver, ["sizeof"])[0].split()
    assert tag == "sizeof"
    assert int(size) == C.sizeof(ffi.GraEngineOpts)
    assert int(off) == ffi.GraEngineOpts.fold_on_device.offset
    # the new field is the struct's last
    assert ffi.GraEngineOpts._fields_[-1][0] == "fold_on_device"
