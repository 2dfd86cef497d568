"""Shapes at which the partition copy (k_copy, part_copy.h) and the one-pass
block-sum scan (k_scan2) can go wrong, checked against the CPU oracle.

Every case applies the same update blobs three ways: to a retaining engine
through the replay path (upload + tick + sync), to a second engine through
handle_replicate_response + flush, and to the oracle. The per-shard store
checksum covers every stored byte, so a wrong lane mapping, a lost head or
tail byte or a clobbered cf prefix shows there; latest_seq and a sample of
gets are compared as well.

The copy kernel picks its lanes-per-record shape (8, 16, 32 or 64) from the
tick's average update size, so the cases are run once per shape: filler
updates pull the average into the wanted band without changing the records
under test.
"""
import ctypes as C
import os
import struct
import subprocess
import sys

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)

import oracle_ffi  # noqa: E402
import rocksplicator_amd as ra  # noqa: E402
from pywb import PyBatch  # noqa: E402
from rocksplicator_amd.ffi import GraUpdateDesc  # noqa: E402

pytestmark = pytest.mark.gpu

STORE = 256 << 20

# average update bytes that select each lanes-per-record shape (engine.hip:
# < 192 -> 8, < 384 -> 16, < 768 -> 32, else 64); one target inside each band
SHAPES = {"g8": 100, "g16": 288, "g32": 576, "g64": 1500}


@pytest.fixture(scope="module")
def olib():
    return oracle_ffi.load()


def _val(n, salt):
    """n distinct-ish bytes, so a shifted or swapped chunk changes the sum."""
    return bytes((i * 131 + salt * 17 + (i >> 8)) & 0xFF for i in range(n))


def _key(i, klen=16):
    return (b"k%07d" % i + b"abcdefghijklmnopqrstuvwxyz" * 10)[:klen]


def _fill_to_shape(tick, shape, shard_of):
    """Append filler puts so the tick's average update size lands in the band
    of `shape`. Fillers are ordinary records and are checked like the rest."""
    target = SHAPES[shape]
    lo = {"g8": 0, "g16": 192, "g32": 384, "g64": 768}[shape]
    hi = {"g8": 192, "g16": 384, "g32": 768, "g64": 1 << 30}[shape]
    tick = list(tick)
    i = 0
    while True:
        total = sum(len(b) for _, b in tick)
        avg = total // len(tick)
        if lo <= avg < hi:
            return tick
        # move the average toward the target with small or large fillers
        vlen = 8 if avg > target else 4 * target
        blob = PyBatch().put(b"fill%04d" % i, _val(vlen, i)).data()
        tick.append((shard_of(i), blob))
        i += 1
        assert i < 20000, "filler did not converge"


def _apply_all(olib, nshards, ticks, merge_op=0, probes=(), **eng_kw):
    """ticks: list of [(shard, blob), ...]. Applies through replay, through
    the streaming entry and to the oracle, and compares all three."""
    ticks = [sorted(t, key=lambda sb: sb[0]) for t in ticks]  # shard-grouped
    ost = oracle_ffi.Store(olib, nshards, merge_op=merge_op)
    nupd = sum(len(t) for t in ticks)
    descs = (GraUpdateDesc * nupd)()
    parts, off, i = [], 0, 0
    for t in ticks:
        for s, blob in t:
            assert ost.apply(s, blob, 7)
            d = descs[i]
            d.shard, d.len, d.off, d.ts = s, len(blob), off, 7
            parts.append(blob)
            off += len(blob)
            i += 1
    raw = b"".join(parts)
    arena = (C.c_uint8 * (len(raw) + 16)).from_buffer_copy(raw + bytes(16))
    want_sum = [olib.orc_shard_checksum(ost.h, s) for s in range(nshards)]
    want_seq = [ost.latest_seq(s) for s in range(nshards)]
    nrec = sum(want_seq)

    def check(e, how):
        for s in range(nshards):
            db = e.open(s)
            assert db.latest_seq() == want_seq[s], (how, s)
            assert db.checksum() == want_sum[s], (how, s)
            for k in probes:
                assert db.get(k) == ost.get(s, k), (how, s, k)
            db.close()
        st = e.stats()
        assert st.updates == nupd and st.records == nrec, how

    e = ra.Engine(nshards=nshards, merge_op=merge_op, store_bytes=STORE, **eng_kw)
    try:
        rep = e.upload(C.cast(arena, C.POINTER(C.c_uint8)), len(raw), descs, nupd)
        first = 0
        for t in ticks:
            rep.tick(first, len(t))
            first += len(t)
        rep.sync()
        check(e, "replay")
    finally:
        e.close()
    e = ra.Engine(nshards=nshards, merge_op=merge_op, store_bytes=STORE, **eng_kw)
    try:
        dbs = [e.open(s) for s in range(nshards)]
        for t in ticks:
            for s, blob in t:
                assert dbs[s].handle_replicate_response(blob, ts=7)
            e.flush()
        check(e, "stream")
    finally:
        e.close()
    return ost


VAL_LENS = [0, 1, 15, 16, 17, 31, 255, 256, 1008, 1023, 1024, 1025, 1039,
            1040, 2047, 2048, 2049, 4101, 65536]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_value_lengths(olib, shape):
    """Either side of one and two 64-lane x 16 B steps, plus long slices."""
    tick = [(i % 3, PyBatch().put(_key(i), _val(n, i)).data())
            for i, n in enumerate(VAL_LENS)]
    tick = _fill_to_shape(tick, shape, lambda i: i % 3)
    _apply_all(olib, 3, [tick], probes=[_key(i) for i in range(len(VAL_LENS))])


KEY_LENS = [0, 1, 3, 15, 16, 17, 33, 250]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_key_lengths(olib, shape):
    """Every residue of the value destination, and varint widths that shift
    the source alignment (key >= 128 B, value >= 128 B and >= 16384 B)."""
    tick, probes = [], []
    i = 0
    for kl in KEY_LENS:
        for vl in (100, 1024, 16384 + kl):
            k = _key(i, kl)
            tick.append((i % 2, PyBatch().put(k, _val(vl, i)).data()))
            probes.append(k)
            i += 1
    # odd key lengths 1..15 step the destination residue one byte at a time
    for kl in range(1, 16):
        k = _key(i, kl)
        tick.append((i % 2, PyBatch().put(k, _val(100 + kl, i)).data()))
        probes.append(k)
        i += 1
    tick = _fill_to_shape(tick, shape, lambda j: j % 2)
    _apply_all(olib, 2, [tick], probes=probes)


def _kinds_updates():
    """Updates of 1, 2, 3 and 9 records over every record kind; 1 and 2 take
    k_emit's record cache, 3 and 9 its second blob walk."""
    v = lambda n, s: _val(n, s)  # noqa: E731
    one = PyBatch().merge(b"ctr", v(8, 1))
    two = PyBatch().delete(b"gone").log_data(b"between").put(b"kept", v(333, 2))
    three = (PyBatch().cf_put(5, b"cfk", v(1024, 3)).single_delete(b"sd")
             .cf_delete(5, b"cfgone"))
    nine = (PyBatch().put(b"a1", v(17, 4)).cf_delete_range(9, b"b", b"dd")
            .delete_range(b"r0", b"r9zz").merge(b"ctr", v(8, 5))
            .log_data(b"x" * 40).cf_merge(2, b"cm", v(100, 6))
            .cf_single_delete(2, b"csd").put(b"", v(5, 7))
            .cf_put(70000, b"big-cf", v(2049, 8)).delete(b"a1"))
    assert [b.count for b in (one, two, three, nine)] == [1, 2, 3, 9]
    only_log = PyBatch().log_data(b"nothing to apply")
    return [one, two, three, nine, only_log]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_record_kinds(olib, shape):
    ups = _kinds_updates()
    tick = [(i % 3, b.data()) for i, b in enumerate(ups * 3)]
    tick = _fill_to_shape(tick, shape, lambda i: i % 3)
    cf = lambda c, k: struct.pack("<I", c) + k  # noqa: E731
    _apply_all(olib, 3, [tick], probes=[
        b"ctr", b"gone", b"kept", cf(5, b"cfk"), b"sd", cf(5, b"cfgone"),
        b"a1", b"a2", b"", cf(2, b"cm"), cf(70000, b"big-cf"), b"r5"])


def test_record_kinds_u64add(olib):
    tick = [(0, PyBatch().merge(b"ctr", struct.pack("<Q", i)).data())
            for i in range(1, 40)]
    _apply_all(olib, 1, [tick], merge_op=ra.MERGE_U64ADD, probes=[b"ctr"])


COUNTS = [1, 2, 31, 32, 33, 63, 64, 65, 4097]


@pytest.mark.parametrize("nshards", [1, 7])
@pytest.mark.parametrize("vlen", [8, 1024])
def test_records_per_tick(olib, nshards, vlen):
    """Record totals on either side of the 4-, 8-, 16- and 32-record batches,
    one tick each, small-update and large-update launch shapes."""
    ticks, i = [], 0
    for n in COUNTS:
        t = []
        for _ in range(n):
            t.append((i % nshards, PyBatch().put(_key(i, 8), _val(vlen, i)).data()))
            i += 1
        ticks.append(t)
    _apply_all(olib, nshards, ticks, probes=[_key(j, 8) for j in (0, 1, 99, i - 1)])


SCAN_TICKS = [1, 255, 256, 257, 65535, 65536, 65537]


def test_scan_block_counts(olib):
    """One-record updates: 1 and 2 block sums, then 256 and 257, so the scan's
    per-thread chunk goes from 1 to 2 entries."""
    ticks, i = [], 0
    for n in SCAN_TICKS:
        t = []
        for _ in range(n):
            t.append((i % 7, PyBatch().put(_key(i, 8), b"v%07d" % i).data()))
            i += 1
        ticks.append(t)
    _apply_all(olib, 7, ticks, probes=[_key(j, 8) for j in (0, 255, 256, 70000, i - 1)])


def test_scan_skips_corrupt_update(olib):
    """A count-mismatch update adds (0, 0) to the scan: its shard keeps the
    prefix before it, the other shards are untouched."""
    nshards, per = 3, 200  # 600 updates -> 3 block sums
    good = lambda s, j: PyBatch().put(_key(j, 12), _val(40 + j % 9, j)).data()  # noqa: E731
    ost = oracle_ffi.Store(olib, nshards)
    e = ra.Engine(nshards=nshards, store_bytes=STORE)
    try:
        dbs = [e.open(s) for s in range(nshards)]
        for j in range(per):
            for s in range(nshards):
                blob = good(s, j)
                if s == 1 and j == 77:
                    bad = bytearray(blob)
                    bad[8] = 9  # header count != records in the batch
                    blob = bytes(bad)
                assert dbs[s].handle_replicate_response(blob, ts=1)
                if s != 1 or j < 77:
                    assert ost.apply(s, blob, 1)
        e.flush()
        assert ost.latest_seq(1) == 77
        for s in range(nshards):
            assert dbs[s].latest_seq() == ost.latest_seq(s), s
            assert dbs[s].checksum() == olib.orc_shard_checksum(ost.h, s), s
        assert dbs[1].counters()["apply_failures"] == 1
        assert dbs[0].counters()["apply_failures"] == 0
        assert dbs[0].get(_key(199, 12)) == ost.get(0, _key(199, 12))
    finally:
        e.close()


def test_ring_wraps_without_failures():
    """A 4 MiB ring store, ticks of about 1.1 MiB: 12 ticks wrap it twice.
    Ring reads are undefined by contract, so only the counters are checked."""
    nshards, per_tick, nticks = 4, 1000, 12
    e = ra.Engine(nshards=nshards, store_ring=1, store_bytes=4 << 20)
    try:
        dbs = [e.open(s) for s in range(nshards)]
        i = 0
        for _ in range(nticks):
            for _ in range(per_tick):
                blob = PyBatch().put(_key(i), _val(1024, i)).data()
                assert dbs[i % nshards].handle_replicate_response(blob, ts=1)
                i += 1
            e.flush()
        for s in range(nshards):
            c = dbs[s].counters()
            assert c["apply_failures"] == 0, s
            assert dbs[s].latest_seq() == nticks * per_tick // nshards, s
        st = e.stats()
        assert st.records == nticks * per_tick
        assert st.payload_bytes > 2 * (4 << 20)
    finally:
        e.close()


def _grid_child():
    """Runs in a fresh process with GRA_COPY_GRID=1: four waves cover 16 to
    128 records per pass, so every wave strides over the task list many
    times, in both the small-update and the large-update launch shape."""
    olib = oracle_ffi.load()
    ticks, i = [], 0
    for vlen, n in ((8, 3001), (1024, 1203), (300, 777), (600, 555)):
        t = []
        for _ in range(n):
            t.append((i % 5, PyBatch().put(_key(i, 8), _val(vlen, i)).data()))
            i += 1
        ticks.append(t)
    _apply_all(olib, 5, ticks, probes=[_key(j, 8) for j in (0, 3000, 3001, i - 1)])
    print("grid-child OK")


def test_grid_stride_small_grid():
    env = dict(os.environ, GRA_COPY_GRID="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--grid-child"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "grid-child OK" in r.stdout, r.stdout + r.stderr


if __name__ == "__main__" and "--grid-child" in sys.argv:
    _grid_child()
