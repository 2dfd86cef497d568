"""Blobs at which k_decode's LDS-staged window parse can go wrong, checked
against the CPU oracle.

k_decode stages the head of every blob into a per-lane LDS row with 16 B
loads and parses from there, reading on from global memory once the walk
leaves the window. The cases sweep tags, length varints and record starts
across every candidate window edge (48, 64, 128), so they do not depend on
the window size the engine was built with.

Every case applies the same update blobs three ways, as
test_gpu_copy_shapes.py does: to one engine through the replay path (upload
+ tick + sync), to a second through handle_replicate_response + flush, and
to the oracle. latest_seq, apply_failures, the per-shard content checksum
and a sample of gets are compared; all expected values are the oracle's.
A blob the oracle rejects is always the last update of its shard, so the
expected state of that shard is everything before it plus one failure."""
import ctypes as C
import os
import struct
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

STORE = 64 << 20


@pytest.fixture(scope="module")
def olib():
    return oracle_ffi.load()


def _val(n, salt):
    return bytes((i * 131 + salt * 17 + (i >> 8)) & 0xFF for i in range(n))


def _key(i, klen):
    return (b"k%05d" % i + b"abcdefghijklmnopqrstuvwxyz" * 6)[:klen]


def _three_way(olib, nshards, ticks, probes=()):
    """ticks: list of [(shard, blob), ...]. A blob the oracle rejects must be
    its shard's last update. Returns the per-shard failure counts."""
    ticks = [sorted(t, key=lambda sb: sb[0]) for t in ticks]  # shard-grouped
    ost = oracle_ffi.Store(olib, nshards)
    fails = [0] * nshards
    nupd = sum(len(t) for t in ticks)
    descs = (GraUpdateDesc * nupd)()
    parts, off, i = [], 0, 0
    for t in ticks:
        for s, blob in t:
            assert fails[s] == 0, "a rejected blob must end its shard"
            if not ost.apply(s, blob, 7):
                fails[s] = 1
            d = descs[i]
            d.shard, d.len, d.off, d.ts = s, len(blob), off, 7
            parts.append(blob)
            off += len(blob)
            i += 1
    raw = b"".join(parts)
    arena = (C.c_uint8 * (len(raw) + 16)).from_buffer_copy(raw + bytes(16))
    want_sum = [olib.orc_shard_checksum(ost.h, s) for s in range(nshards)]
    want_seq = [ost.latest_seq(s) for s in range(nshards)]

    def check(e, how):
        for s in range(nshards):
            db = e.open(s)
            assert db.latest_seq() == want_seq[s], (how, s)
            assert db.counters()["apply_failures"] == fails[s], (how, s)
            assert db.checksum() == want_sum[s], (how, s)
            for k in probes:
                assert db.get(k) == ost.get(s, k), (how, s, k)
            db.close()
        st = e.stats()
        assert st.updates == nupd and st.records == sum(want_seq), how

    e = ra.Engine(nshards=nshards, store_bytes=STORE)
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
    e = ra.Engine(nshards=nshards, store_bytes=STORE)
    try:
        dbs = [e.open(s) for s in range(nshards)]
        for t in ticks:
            for s, blob in t:
                assert dbs[s].handle_replicate_response(blob, ts=7)
            e.flush()
        check(e, "stream")
    finally:
        e.close()
    return fails


def _sweep_blob(kl, vl, i):
    return PyBatch().put(_key(i, kl), _val(vl, i)).data()


def test_key_length_sweep(olib):
    """One Put per blob, key_len 0..140 x value of 0, 1 and 200 bytes: the
    tag, the key varint and the one- or two-byte value varint cross every
    window edge. One value of 16 KiB + 5 has a 3-byte varint."""
    tick, probes, i = [], [], 0
    for kl in range(0, 141):
        for vl in (0, 1, 200):
            tick.append((i % 5, _sweep_blob(kl, vl, i)))
            if kl in (0, 5, 31, 33, 46, 47, 48, 62, 63, 64, 126, 127, 128, 140):
                probes.append(_key(i, kl))
            i += 1
    tick.append((2, PyBatch().put(b"three-byte-varint", _val(16384 + 5, 9)).data()))
    probes.append(b"three-byte-varint")
    fails = _three_way(olib, 5, [tick], probes=probes)
    assert fails == [0] * 5


def _small_records(n, salt):
    b = PyBatch()
    for j in range(n):
        # a record is tag + 2 length bytes + key + value = 10..30 bytes
        b.put(b"m%02d%02d" % (salt, j), _val(2 + (j * 5 + salt) % 21, j))
    return b


def test_multi_record_batches(olib):
    """3, 5 and 40 records per batch exceed the decode record cache, so
    k_emit walks the blob again and the decode walk runs out of the window.
    The padded family puts the second record's tag on the last byte inside
    and the first byte outside a 48-, 64- and 128-byte window."""
    tick, i = [], 0
    for n in (3, 5, 40, 3, 5, 40):
        tick.append((i % 3, _small_records(n, i).data()))
        i += 1
    for edge in (48, 64, 128):
        for tag_pos in (edge - 1, edge):
            # first record: 12 header + tag + klen + 8 key + vlen + value
            vl = tag_pos - 15 - 8
            b = (PyBatch().put(b"pad%05d" % tag_pos, _val(vl, edge))
                 .delete(b"pad%05d" % 0).put(b"after%03d" % tag_pos, _val(33, 1)))
            blob = b.data()
            assert blob[tag_pos] == 0x00 and blob[tag_pos - 1] == _val(vl, edge)[-1]
            tick.append((i % 3, blob))
            i += 1
    probes = [b"m0000", b"m0239", b"m0504", b"pad00047", b"pad00000",
              b"after048", b"after127", b"after128"]
    fails = _three_way(olib, 3, [tick], probes=probes)
    assert fails == [0] * 3


def test_tags(olib):
    """cf-prefixed Put, Delete, Merge and range-delete with a 1-byte and a
    5-byte cf varint; LogData and Noop ahead of the first Put."""
    tick = []
    for s, cf in enumerate((5, 1 << 28)):
        assert len(PyBatch().cf_delete(cf, b"").body) == (3 if cf == 5 else 7)
        tick.append((s, PyBatch().cf_put(cf, b"cfk", _val(100, 1)).data()))
        tick.append((s, PyBatch().cf_put(cf, b"cfgone", _val(60, 2))
                     .cf_delete(cf, b"cfgone").data()))
        tick.append((s, PyBatch().cf_merge(cf, b"cfm", _val(8, 3)).data()))
        tick.append((s, PyBatch().cf_put(cf, b"r5", b"covered")
                     .cf_delete_range(cf, b"r0", b"r9")
                     .cf_put(cf, _key(7, 50), _val(70, 4)).data()))
    tick.append((2, PyBatch().log_data(b"x" * 40).noop().put(b"kept", _val(9, 5))
                 .data()))
    tick.append((2, PyBatch().noop().log_data(b"y" * 130).put(b"kept2", _val(300, 6))
                 .noop().data()))
    tick.append((2, PyBatch().log_data(b"only log data").data()))
    cfk = lambda c, k: struct.pack("<I", c) + k  # noqa: E731
    probes = [b"kept", b"kept2"]
    for cf in (5, 1 << 28):
        probes += [cfk(cf, b"cfk"), cfk(cf, b"cfgone"), cfk(cf, b"cfm"),
                   cfk(cf, b"r5"), cfk(cf, _key(7, 50))]
    fails = _three_way(olib, 3, [tick], probes=probes)
    assert fails == [0] * 3


def test_header_edge_lengths(olib):
    """Blobs of 0..13 bytes, the 12-byte empty batch and a count mismatch.
    Shorter than a header never reaches the device: both entries refuse it."""
    good = PyBatch().put(b"first", b"v").data()
    empty = PyBatch().data()
    assert len(empty) == 12
    noop13 = PyBatch().noop().data()
    put13 = struct.pack("<QI", 0, 1) + b"\x01"  # count 1, a Put tag, no slices
    mismatch = bytearray(PyBatch().put(b"k", b"v").data())
    mismatch[8] = 2
    assert len(noop13) == len(put13) == 13
    tick = [(0, good), (0, empty), (0, noop13), (0, PyBatch().put(b"last", b"w").data()),
            (1, good), (1, put13),
            (2, good), (2, bytes(mismatch)),
            (3, good), (3, struct.pack("<QI", 0, 1))]  # header alone, count 1
    fails = _three_way(olib, 4, [tick], probes=[b"first", b"last", b"k"])
    assert fails == [0, 1, 1, 1]
    e = ra.Engine(nshards=1, store_bytes=STORE)
    try:
        db = e.open(0)
        for n in range(0, 12):
            short = good[:n]
            assert not db.handle_replicate_response(short, ts=1), n
            if n:
                d = (GraUpdateDesc * 1)()
                d[0].shard, d[0].len, d[0].off, d[0].ts = 0, n, 0, 1
                arena = (C.c_uint8 * 32).from_buffer_copy(short + bytes(32 - n))
                with pytest.raises(RuntimeError):
                    e.upload(C.cast(arena, C.POINTER(C.c_uint8)), n, d, 1)
        e.flush()
        assert db.latest_seq() == 0
        assert db.counters()["apply_failures"] == 0
    finally:
        e.close()


def test_truncations(olib):
    """Four of the sweep blobs cut at every length from 12 to 140: each cut
    sits alone on a shard behind one good update."""
    tick, s = [], 0
    for kl, vl in ((20, 200), (60, 200), (130, 200), (100, 1)):
        full = _sweep_blob(kl, vl, kl)
        for cut in range(12, 141):
            if cut >= len(full):
                continue
            tick.append((s, PyBatch().put(b"good", _val(20, s)).data()))
            tick.append((s, full[:cut]))
            s += 1
    assert s > 480
    fails = _three_way(olib, s, [tick])
    assert fails == [1] * s  # a cut one-Put batch is never well-formed


def test_alignment(olib):
    """Odd-sized blobs back to back: 129-byte blobs step the offset through
    every residue mod 128 (and mod 16), a few other odd sizes are mixed in,
    and the arena's last blob is 13 bytes long."""
    tick = []
    for i in range(130):
        blob = PyBatch().put(_key(i, 14), _val(100, i)).data()
        assert len(blob) == 129
        tick.append((0, blob))
    for i, (kl, vl) in enumerate(((3, 17), (50, 12), (9, 130), (61, 1), (1, 1))):
        blob = PyBatch().put(_key(500 + i, kl), _val(vl, i)).data()
        assert len(blob) % 2 == 1
        tick.append((1, blob))
    tick.append((1, PyBatch().noop().data()))  # sorts last: ends the arena
    assert len(tick[-1][1]) == 13
    offs, off = set(), 0
    for _, b in tick:
        offs.add(off % 128)
        off += len(b)
    assert len(offs) == 128
    fails = _three_way(olib, 2, [tick],
                       probes=[_key(0, 14), _key(129, 14), _key(502, 9)])
    assert fails == [0, 0]


def test_block_tails(olib):
    """Ticks of 1, 255, 257 and 513 updates: lanes past the tick's end stage
    nothing and still take part in the block scan."""
    ticks, i = [], 0
    for n in (1, 255, 257, 513):
        t = []
        for _ in range(n):
            t.append((i % 7, PyBatch().put(_key(i, 5 + i % 60), _val(i % 90, i)).data()))
            i += 1
        ticks.append(t)
    fails = _three_way(olib, 7, ticks,
                       probes=[_key(j, 5 + j % 60) for j in (0, 1, 255, 256, 512, i - 1)])
    assert fails == [0] * 7


def test_single_corrupt_update_among_clean(olib):
    """One corrupt update in a tick of clean ones, through replay and through
    handle_replicate_response: the per-update validity is fetched from the
    device only on this path. Its shard keeps the prefix before it; the
    other shards are untouched."""
    tick = []
    for j in range(200):
        for s in range(3):
            if s == 1 and j > 77:
                continue
            blob = PyBatch().put(_key(j, 12), _val(40 + j % 9, j)).data()
            if s == 1 and j == 77:
                bad = bytearray(blob)
                bad[13] = 0x8F  # key length varint now runs past the blob
                blob = bytes(bad)
            tick.append((s, blob))
    fails = _three_way(olib, 3, [tick], probes=[_key(0, 12), _key(76, 12),
                                                 _key(77, 12), _key(199, 12)])
    assert fails == [0, 1, 0]
