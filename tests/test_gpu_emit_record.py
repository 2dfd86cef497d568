"""What k_decode hands k_emit (a 16 B wb::EmitRec per update) and the run
descriptors that ride as the trailing blocks of the k_emit launch, checked
against the CPU oracle.

An update reaches k_emit as one of three kinds: nothing to emit (rejected,
or no seq-consuming record), one record packed by decode, or "walk the blob
again" (two or more records, or a key that starts past byte 255). Each kind
computes its own place in the header, task and payload arrays from the scan,
so the cases mix the kinds inside one block of 256 updates and across
blocks. A group's last_seq comes from the header count of its last blob, so
the group-end cases end shards on blobs whose count is 0, 40, or differs
from the number of tags in the body.

Every case but the overflow one uses the three-way comparison of
test_gpu_decode_window.py: replay path, handle_replicate_response + flush,
and the oracle; all expected values are the oracle's, and a rejected blob is
its shard's last update."""
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
from test_gpu_decode_window import _key, _three_way, _val  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def olib():
    return oracle_ffi.load()


def _cfk(cf, k):
    return struct.pack("<I", cf) + k


def _multi(n, i):
    """n Puts in one batch: kind 2 for every n >= 2."""
    b = PyBatch()
    for j in range(n):
        b.put(b"b%05d.%02d" % (i, j), _val(3 + (i + 5 * j) % 40, i + j))
    return b.data()


# One pass over this pattern puts a kind-1 update on both sides of every
# kind-2 batch and has both flavours of kind 0. 11 is coprime to 256, so the
# block edges of a 513-update tick fall on different kinds.
_PATTERN = ("put", "multi2", "put", "empty", "delete", "multi3", "cfput",
            "logonly", "put", "multi40", "cfput")


def _mixed_update(i):
    """(blob, kind, probe keys) of update i of the mixed stream."""
    what = _PATTERN[i % len(_PATTERN)]
    if what == "put":
        k = _key(i, 5 + i % 29)
        return PyBatch().put(k, _val(1 + i % 70, i)).data(), 1, [k]
    if what == "delete":  # the Put two updates back, when on the same shard
        k = _key(i - 2, 5 + (i - 2) % 29)
        return PyBatch().delete(k).data(), 1, [k]
    if what == "cfput":
        cf = 7 if i % 2 else 1 << 21
        k = b"cf%05d" % i
        return PyBatch().cf_put(cf, k, _val(9 + i % 50, i)).data(), 1, [_cfk(cf, k)]
    if what == "empty":
        return PyBatch().data(), 0, []
    if what == "logonly":
        return PyBatch().log_data(b"L" * (i % 60)).noop().data(), 0, []
    n = int(what[5:])
    return _multi(n, i), 2, [b"b%05d.%02d" % (i, 0), b"b%05d.%02d" % (i, n - 1)]


@pytest.mark.parametrize("nupd", [257, 513])
def test_mixed_kinds_in_and_across_blocks(olib, nupd):
    """Ticks of 257 and 513 updates interleaving all three kinds. Shards are
    contiguous index ranges, so the tick keeps the interleaving. Gets probe
    the records on both sides of, and inside, kind-2 batches spread over the
    tick, the block edges included."""
    nshards = 3
    ups = [_mixed_update(i) for i in range(nupd)]
    tick = [(i * nshards // nupd, ups[i][0]) for i in range(nupd)]
    assert {u[1] for u in ups} == {0, 1, 2}
    twos = [i for i in range(nupd) if ups[i][1] == 2]
    probes = []
    picked = twos[:3] + twos[-3:] + [i for i in twos if 245 <= i <= 268]
    for i in sorted(set(picked)):
        for j in (i - 1, i, i + 1):
            if 0 <= j < nupd:
                probes += ups[j][2]
    fails = _three_way(olib, nshards, [tick], probes=probes)
    assert fails == [0] * nshards


def _put_with_key_at(pos, key, val):
    """LogData ahead of a single Put, sized so the key starts at `pos`."""
    for n in range(0, 400):
        blob = PyBatch().log_data(b"\xAA" * n).put(key, val).data()
        if blob.index(key) == pos:
            return blob
    raise AssertionError(pos)


def test_key_off_edge(olib):
    """key_off 255 packs, 256 walks again; each also ends a shard."""
    k255, k256 = b"starts-at-255", b"starts-at-256"
    b255 = _put_with_key_at(255, k255, _val(77, 1))
    b256 = _put_with_key_at(256, k256, _val(78, 2))
    assert b255.index(k255) == 255 and b256.index(k256) == 256
    good = lambda i: PyBatch().put(_key(i, 9), _val(20, i)).data()  # noqa: E731
    tick = [(0, good(0)), (0, b255), (0, b256), (0, good(1)),
            (1, good(2)), (1, b255),
            (2, good(3)), (2, b256)]
    fails = _three_way(olib, 3, [tick],
                       probes=[k255, k256, _key(0, 9), _key(1, 9)])
    assert fails == [0] * 3


def _group_end_ticks():
    """Two ticks over five shards whose groups end on a count of 0, on 40, on
    a batch whose LogData and Noop records take no count, on a one-record cf
    range delete, and a group that is one empty batch."""
    put = lambda i: PyBatch().put(_key(i, 8), _val(30, i)).data()  # noqa: E731
    padded = (PyBatch().log_data(b"x" * 20).put(b"p1", b"v1").noop()
              .log_data(b"").put(b"p2", b"v2").noop().noop().data())
    assert struct.unpack_from("<I", padded, 8)[0] == 2  # 7 tags, count 2
    ticks = []
    for t in range(2):
        ticks.append([
            (0, put(10 * t)), (0, put(10 * t + 1)), (0, PyBatch().data()),
            (1, put(10 * t + 2)), (1, _multi(40, 900 + t)),
            (2, put(10 * t + 3)), (2, padded),
            (3, put(10 * t + 4)),
            (3, PyBatch().cf_delete_range(9, b"a", b"z").data()),
            (4, PyBatch().data()),  # a group of one empty batch
        ])
    return ticks


def test_group_ends(olib):
    """The content of shards whose groups end on those shapes, three ways.
    Two ticks, so the second starts from the first's seqs. (What the device
    reports as a group's last_seq is checked by the next test: on clean
    ticks latest_seq comes from the host's own count.)"""
    fails = _three_way(olib, 5, _group_end_ticks(),
                       probes=[b"p1", b"p2", _key(0, 8), _key(14, 8),
                               b"b00900.39", b"b00901.00"])
    assert fails == [0] * 5


@pytest.mark.parametrize("how", ["replay", "stream"])
def test_group_ends_set_the_durable_boundary(olib, how):
    """last_seq = last update's base_seq + its header count - 1, the count
    read by the descriptor blocks from bytes 8..11 of the group's last blob.
    The host keeps the largest last_seq of a shard's clean groups as its
    durable boundary and shows it only when the shard fails. So the
    group-end ticks go into a 1 MiB non-ring store and a tick that overflows
    it follows: every shard rolls back to its boundary, which must be the
    oracle's latest_seq from before that tick, 0 for the shard of empty
    batches. A count taken from the wrong place moves the boundary. After
    the fail-once every shard takes a small update again."""
    nshards = 5
    ticks = _group_end_ticks()
    big = [(s, PyBatch().put(b"big%d" % s, bytes(300 * 1024)).data())
           for s in range(nshards)]  # 1.5 MB into a 1 MiB store
    ost = oracle_ffi.Store(olib, nshards)
    for t in ticks:
        for s, blob in t:
            assert ost.apply(s, blob, 7)
    want_seq = [ost.latest_seq(s) for s in range(nshards)]
    assert want_seq == [4, 82, 6, 4, 0]
    want_sum = [olib.orc_shard_checksum(ost.h, s) for s in range(nshards)]
    e = ra.Engine(nshards=nshards, store_bytes=1 << 20, store_ring=0)
    try:
        dbs = [e.open(s) for s in range(nshards)]
        if how == "replay":
            ups = [sb for t in ticks for sb in sorted(t, key=lambda x: x[0])] + big
            descs = (GraUpdateDesc * len(ups))()
            off = 0
            for d, (s, blob) in zip(descs, ups):
                d.shard, d.len, d.off, d.ts = s, len(blob), off, 7
                off += len(blob)
            raw = b"".join(b for _, b in ups)
            arena = (C.c_uint8 * (off + 16)).from_buffer_copy(raw + bytes(16))
            rep = e.upload(C.cast(arena, C.POINTER(C.c_uint8)), off, descs, len(ups))
            first = 0
            for n in [len(t) for t in ticks] + [len(big)]:
                rep.tick(first, n)
                first += n
            rep.sync()
        else:
            for t in ticks:
                for s, blob in t:
                    assert dbs[s].handle_replicate_response(blob, ts=7)
                e.flush()
            assert [db.latest_seq() for db in dbs] == want_seq
            for s, blob in big:
                dbs[s].handle_replicate_response(blob, ts=7)
            e.flush()
        assert [db.counters()["apply_failures"] for db in dbs] == [1] * nshards
        assert [db.latest_seq() for db in dbs] == want_seq  # the boundary
        for s in range(nshards):
            assert dbs[s].checksum() == want_sum[s], s
            assert dbs[s].get(b"big%d" % s) is None
        for s in range(nshards):
            after = PyBatch().put(b"after%d" % s, b"y" * 40).data()
            assert not dbs[s].handle_replicate_response(after, ts=7)  # fail once
            assert dbs[s].handle_replicate_response(after, ts=7)
            assert ost.apply(s, after, 7)
        e.flush()
        for s in range(nshards):
            assert dbs[s].latest_seq() == ost.latest_seq(s) == want_seq[s] + 1
            assert dbs[s].checksum() == olib.orc_shard_checksum(ost.h, s)
            assert dbs[s].get(b"after%d" % s) == b"y" * 40
            assert dbs[s].counters()["apply_failures"] == 1
    finally:
        e.close()


@pytest.mark.parametrize("nshards,per_shard", [(600, 1), (256, 1), (257, 1),
                                               (1, 1), (3, 513)])
def test_run_descriptor_blocks(olib, nshards, per_shard):
    """Shard groups per tick against 256 per descriptor block: 600 groups is
    3 emit blocks + 3 descriptor blocks, 256 and 257 sit on the block edge,
    1 group and 3 long groups are the small end."""
    tick, i = [], 0
    for s in range(nshards):
        for _ in range(per_shard):
            tick.append((s, PyBatch().put(_key(i, 6 + i % 20), _val(i % 50, i)).data()))
            i += 1
    probes = [_key(j, 6 + j % 20) for j in (0, i // 2, i - 1)]
    fails = _three_way(olib, nshards, [tick], probes=probes)
    assert fails == [0] * nshards


def test_store_overflow_tick(olib):
    """One tick larger than a non-ring store: the tick's groups apply
    nothing, their shards count one failure each and poison at the durable
    boundary, a shard outside the tick is untouched, and after the
    fail-once a small tick applies. The descriptor blocks must report the
    overflow (base_seq 0) although the emit blocks return early. The
    expected counters, seqs and contents are the behaviour of the build
    before the descriptors moved into the k_emit launch: this test was run
    against that build too and passes there unchanged (profiles/emitrec)."""
    ost = oracle_ffi.Store(olib, 3)
    e = ra.Engine(nshards=3, store_bytes=1 << 20, store_ring=0)
    try:
        dbs = [e.open(s) for s in range(3)]
        for s in range(3):
            first = PyBatch().put(b"first%d" % s, b"x" * (s + 1)).data()
            assert dbs[s].handle_replicate_response(first, ts=1)
            assert ost.apply(s, first, 1)
        e.flush()
        assert [db.latest_seq() for db in dbs] == [1, 1, 1]
        big = bytes(300 * 1024)
        for i, s in enumerate((0, 0, 0, 1, 1)):  # 1.5 MB into a 1 MiB store
            dbs[s].handle_replicate_response(
                PyBatch().put(b"big%d" % i, big).data(), ts=1)
        e.flush()
        assert [db.counters()["apply_failures"] for db in dbs] == [1, 1, 0]
        assert [db.latest_seq() for db in dbs] == [1, 1, 1]
        assert e.stats().records == 3
        for s in range(3):
            assert dbs[s].get(b"first%d" % s) == b"x" * (s + 1)
        assert dbs[0].get(b"big0") is None and dbs[1].get(b"big3") is None
        # poisoned shards fail once, then take the small tick
        after = [PyBatch().put(b"after%d" % s, b"y" * 40).data() for s in range(3)]
        assert not dbs[0].handle_replicate_response(after[0], ts=1)
        assert not dbs[1].handle_replicate_response(after[1], ts=1)
        for s in range(3):
            assert dbs[s].handle_replicate_response(after[s], ts=1)
            assert ost.apply(s, after[s], 1)
        e.flush()
        for s in range(3):
            assert dbs[s].latest_seq() == ost.latest_seq(s) == 2
            assert dbs[s].counters()["apply_failures"] == (1 if s < 2 else 0)
            assert dbs[s].checksum() == olib.orc_shard_checksum(ost.h, s)
            assert dbs[s].get(b"after%d" % s) == b"y" * 40
        assert e.stats().records == 6
    finally:
        e.close()
