"""The packed one-record form of wb_format.h (wb::EmitRec, what k_decode
hands k_emit) against the plain walk_f and the oracle, on a CPU box:
scripts/test_emit_record_host.cpp is built with
g++ -fsanitize=address,undefined as its own program and driven over stdin.

For every blob the driver walks with walk_f, packs (WalkTotals, first Rec)
and, where the kind is 1, unpacks again. Checked here: the kind is 0, 1 or 2
by exactly the rule (0: rejected or no record; 1: one record with
key_off <= 255 and key_len <= 65535; 2: everything else), a kind-1 record
unpacks bit-equal to the walk's first Rec, and the walk's decision and first
record agree with the oracle decoder."""
import os
import struct
import subprocess

import pytest

import oracle_ffi
from pywb import PyBatch, varint32
from test_decode_window_host import all_blobs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "build", "test_emit_record_host")

KIND_NONE, KIND_ONE, KIND_WALK = 0, 1, 2


@pytest.fixture(scope="module")
def driver():
    os.makedirs(os.path.join(REPO, "build"), exist_ok=True)
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "scripts/test_emit_record_host.cpp", "-o", BIN],
        cwd=REPO, check=True)
    return BIN


@pytest.fixture(scope="module")
def olib():
    return oracle_ffi.load()


class Row:
    def __init__(self, line):
        f = line.split()
        assert f[0] == "blob" and len(f) == 19, line
        v = [int(x) for x in f[1:]]
        (self.ok, self.nrec, self.emitted, self.key_off, self.key_len,
         self.val_off, self.val_len, self.tag, self.cf_id) = v[:9]
        (self.kind, self.p_key_off, self.p_key_len, self.p_val_gap,
         self.p_val_len, self.p_tag, self.p_cf_id, self.p_pad, self.equal) = v[9:]


def drive(driver, blobs):
    text = "".join("blob %s\n" % (b.hex() or "-") for b in blobs)
    r = subprocess.run([driver], input=text, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stderr == "", r.stderr[-3000:]  # the sanitizers report nothing
    out = r.stdout.splitlines()
    assert len(out) == len(blobs)
    return [Row(line) for line in out]


def want_kind(row):
    if not row.ok or row.nrec == 0:
        return KIND_NONE
    if row.nrec == 1 and row.key_off <= 255 and row.key_len <= 65535:
        return KIND_ONE
    return KIND_WALK


def check_row(row, blob, olib):
    """The rule, the round trip and the oracle's view of one blob."""
    assert row.kind == want_kind(row), (blob[:64].hex(), vars(row))
    try:
        _seq, _cnt, recs = oracle_ffi.decode(olib, blob)
        consuming = [r for r in recs if r.consumes_seq]
    except ValueError:
        consuming = None
    assert bool(row.ok) == (consuming is not None), blob[:64].hex()
    if consuming is not None:
        assert row.nrec == row.emitted == len(consuming), blob[:64].hex()
    if row.kind == KIND_ONE:
        assert row.equal == 1, (blob[:64].hex(), vars(row))
        assert row.p_pad == 0
        # the packed fields, spelled out
        assert (row.p_key_off, row.p_key_len, row.p_val_len, row.p_tag,
                row.p_cf_id) == (row.key_off, row.key_len, row.val_len,
                                 row.tag, row.cf_id)
        if row.val_off:
            assert 1 <= row.p_val_gap <= 5  # the value's length varint
            assert row.key_off + row.key_len + row.p_val_gap == row.val_off
        else:
            assert row.p_val_gap == 0 and row.val_len == 0
        o = consuming[0]
        assert (o.type, o.cf_id, o.key_len, o.val_len) == \
            (row.tag, row.cf_id, row.key_len, row.val_len)
        assert blob[o.key_off:o.key_off + o.key_len] == \
            blob[row.key_off:row.key_off + row.key_len]
        if row.val_off:
            assert blob[o.val_off:o.val_off + o.val_len] == \
                blob[row.val_off:row.val_off + row.val_len]
    else:
        assert row.equal == -1
        # nothing of a record leaks into a kind-0 or kind-2 EmitRec
        assert (row.p_key_off, row.p_key_len, row.p_val_gap, row.p_val_len,
                row.p_tag, row.p_cf_id, row.p_pad) == (0,) * 7


def test_corpus_kinds_and_round_trip(driver, olib):
    blobs = all_blobs()
    assert len(blobs) > 1500
    rows = drive(driver, blobs)
    kinds = [0, 0, 0]
    n_ok = 0
    for b, row in zip(blobs, rows):
        check_row(row, b, olib)
        kinds[row.kind] += 1
        n_ok += row.ok
    assert 300 < n_ok < len(blobs) - 300  # both decisions well represented
    assert kinds[KIND_ONE] > 200 and kinds[KIND_WALK] > 20, kinds


def _val(n, salt):
    return bytes((i * 131 + salt * 17) & 0xFF for i in range(n))


def _put_at(pos, key=b"KEY-at-edge"):
    """One Put behind a LogData record sized so the key starts at `pos`."""
    # 12 header + tag + varint(n) + n log bytes + tag + klen varint
    for n in range(0, 400):
        blob = PyBatch().log_data(b"\xAA" * n).put(key, b"value").data()
        if blob.index(key) == pos:
            return blob
    raise AssertionError(pos)


def test_pack_limits(driver, olib):
    cases = []  # (blob, kind, first-record expectations or None)

    def case(blob, kind, **first):
        cases.append((blob, kind, first))

    key = b"KEY-at-edge"
    for pos in (254, 255, 256, 257):
        blob = _put_at(pos, key)
        assert blob.index(key) == pos
        case(blob, KIND_ONE if pos <= 255 else KIND_WALK, key_off=pos,
             key_len=len(key), val_len=5, tag=0x01)
    for kl in (65535, 65536):
        k = bytes((i * 7 + 3) & 0xFF for i in range(kl))
        blob = PyBatch().put(k, b"v").data()
        assert blob.index(k) == 12 + 1 + 3  # tag + 3-byte key varint
        case(blob, KIND_ONE if kl == 65535 else KIND_WALK, key_off=16,
             key_len=kl, val_off=16 + kl + 1, val_len=1)
    case(PyBatch().delete(b"gone").data(), KIND_ONE, key_off=14, key_len=4,
         val_off=0, val_len=0, tag=0x00)
    case(PyBatch().single_delete(b"").data(), KIND_ONE, key_off=14, key_len=0,
         val_off=0, val_len=0, tag=0x07)
    case(PyBatch().cf_delete_range(300, b"a", b"zz").data(), KIND_ONE,
         key_off=16, key_len=1, val_off=18, val_len=2, tag=0x0E, cf_id=300)
    blob = PyBatch().cf_put(0xFFFFFFFF, b"maxcf", b"v").data()
    assert blob[13:18] == varint32(0xFFFFFFFF) == b"\xff\xff\xff\xff\x0f"
    case(blob, KIND_ONE, key_off=19, key_len=5, val_len=1, tag=0x05,
         cf_id=0xFFFFFFFF)
    big = _val(16384 + 5, 1)
    blob = PyBatch().put(b"big", big).data()
    assert blob.index(big) == 12 + 1 + 1 + 3 + 3  # 3-byte value varint
    case(blob, KIND_ONE, key_off=14, key_len=3, val_off=20, val_len=16389)
    # an empty value still has a value slice: gap 1, not the key-only code
    case(PyBatch().put(b"k", b"").data(), KIND_ONE, key_off=14, key_len=1,
         val_off=16, val_len=0)
    # kinds 0 and 2 at their simplest
    case(PyBatch().data(), KIND_NONE)
    case(PyBatch().log_data(b"only").noop().data(), KIND_NONE)
    case(struct.pack("<QI", 0, 2) + PyBatch().put(b"k", b"v").body, KIND_NONE)
    case(PyBatch().put(b"a", b"1").put(b"b", b"2").data(), KIND_WALK)

    rows = drive(driver, [c[0] for c in cases])
    for (blob, kind, first), row in zip(cases, rows):
        check_row(row, blob, olib)
        assert row.kind == kind, (blob[:64].hex(), vars(row))
        for name, want in first.items():
            assert getattr(row, name) == want, (name, blob[:64].hex(), vars(row))
