"""The windowed byte source of wb_format.h (wb::WinSrc under wb::walk_src,
what k_decode parses through) against the plain walk_f and the oracle, on a
CPU box: scripts/test_decode_window_host.cpp is built with
g++ -fsanitize=address,undefined as its own program and driven over stdin.

For every blob the driver walks windows of {0, 1, 11, 12, 13, 14, 31, 32, 33,
48, 64, 128, len-1, len, len+1} bytes, each window and each blob copy in a
heap buffer of exactly its size, and counts the windows whose WalkTotals or
(Rec, index) sequence is not bit-equal to plain walk_f's. The accept/reject
decision, record count and header fields are then checked against the
oracle decoder here."""
import json
import os
import random
import subprocess

import pytest

import oracle_ffi
from pywb import PyBatch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "build", "test_decode_window_host")
GOLDEN = os.path.join(REPO, "tests", "golden", "writebatch_vectors.json")


@pytest.fixture(scope="module")
def driver():
    os.makedirs(os.path.join(REPO, "build"), exist_ok=True)
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "scripts/test_decode_window_host.cpp", "-o", BIN],
        cwd=REPO, check=True)
    return BIN


@pytest.fixture(scope="module")
def olib():
    return oracle_ffi.load()


def drive(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n",
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stderr == "", r.stderr[-3000:]  # the sanitizers report nothing
    return r.stdout.splitlines()


def _val(n, salt):
    return bytes((i * 131 + salt * 17) & 0xFF for i in range(n))


def built_blobs():
    """PyBatch batches whose tags and length varints land on every window
    edge: key lengths that push the value varint across 31..33, 48, 64 and
    128, multi-record batches, cf prefixes, non-consuming records first."""
    out = []
    for kl in list(range(0, 40)) + [44, 45, 46, 47, 48, 60, 61, 62, 63, 64,
                                    110, 111, 112, 113, 114, 127, 128, 129, 140]:
        for vl in (0, 1, 200):
            out.append(PyBatch(seq=kl).put(b"k" * kl, _val(vl, kl)).data())
    out.append(PyBatch().put(b"big", _val(16384 + 5, 1)).data())  # 3-B varint
    for n in (2, 3, 5, 40):
        b = PyBatch(seq=1000 + n)
        for j in range(n):
            b.put(b"key%03d" % j, _val(10 + (j * 7) % 21, j))
        out.append(b.data())
    out.append(PyBatch().cf_put(5, b"cfk", _val(100, 2)).cf_delete(5, b"d")
               .cf_merge(1 << 28, b"m", b"12345678")
               .cf_delete_range(300, b"a", b"zz")
               .cf_single_delete(70000, b"sd").data())
    out.append(PyBatch().log_data(b"x" * 40).noop().put(b"after", b"v")
               .begin_prepare().commit_xid(b"xid").delete(b"after").data())
    out.append(PyBatch().data())  # 12-byte empty batch
    out.append(PyBatch().merge(b"ctr", b"\x01" * 8).delete_range(b"a", b"b")
               .single_delete(b"s").data())
    return out


def all_blobs():
    rng = random.Random(20240611)
    with open(GOLDEN) as f:
        base = [bytes.fromhex(v["hex"]) for v in json.load(f)]
    base += built_blobs()
    blobs = list(base)
    for b in base:
        # truncations: every header edge, then a spread over the body
        cuts = set(range(0, min(len(b), 15)))
        cuts.update(rng.randrange(len(b)) for _ in range(6))
        cuts.add(len(b) - 1)
        blobs += [b[:c] for c in sorted(cuts) if 0 <= c < len(b)]
        # byte mutations: count field, tag, length varints, anywhere
        for _ in range(8):
            m = bytearray(b)
            pos = rng.choice([8, 12, 13, rng.randrange(len(m)),
                              rng.randrange(len(m))])
            if pos < len(m):
                m[pos] = rng.choice([0x00, 0x7F, 0x80, 0xFF, m[pos] ^ 0x01,
                                     rng.randrange(256)])
                blobs.append(bytes(m))
    return blobs


def test_windowed_walk_matches_plain_walk_and_oracle(driver, olib):
    blobs = all_blobs()
    assert len(blobs) > 1500
    out = drive(driver, ["blob " + (b.hex() or "-") for b in blobs])
    assert len(out) == len(blobs)
    n_ok = 0
    for b, line in zip(blobs, out):
        f = line.split()
        assert f[0] == "blob", line
        ok, nrec, _payload, _p16, hdr_count, hdr_seq, emitted, nwin, differ = \
            (int(x) for x in f[1:])
        assert nwin == (15 if len(b) else 14), line
        assert differ == 0, (b.hex(), line)
        try:
            seq, cnt, recs = oracle_ffi.decode(olib, b)
            want_ok = True
        except ValueError:
            want_ok = False
        assert bool(ok) == want_ok, (b.hex(), line)
        if want_ok:
            n_ok += 1
            consuming = [r for r in recs if r.consumes_seq]
            assert (hdr_seq, hdr_count) == (seq, cnt), b.hex()
            assert nrec == emitted == len(consuming), b.hex()
    assert 300 < n_ok < len(blobs) - 300  # both decisions well represented


def test_chunk_helper(driver):
    assert drive(driver, ["chunks"]) == ["chunks 0"]
