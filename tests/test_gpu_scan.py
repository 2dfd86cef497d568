"""Ordered range scans served from the device store (gra_scan) against the
CPU oracle. Expected results come from the oracle store only — for every
stored key the test ever wrote, in range and found by orc_get — and equality
is exact. `info.candidates` is checked against the test's own count of point
entries in range over all versions."""
import ctypes as C
import random
import struct

import pytest

import oracle_ffi
import rocksplicator_amd as ra
import scan_streams as ss
from pywb import PyBatch

pytestmark = pytest.mark.gpu

BIG = 1 << 22
SMALL_ENGINE = dict(store_bytes=256 << 20, staging_bytes=64 << 20)


@pytest.fixture(scope="module")
def olib():
    return oracle_ffi.load()


@pytest.fixture(scope="module")
def stream():
    return ss.make_stream(seed=21, n_records=4000, n_batches=40)


def apply_all(e, db, ost, reps, flush_every=None, shard=0):
    for i, rep in enumerate(reps):
        assert db.handle_replicate_response(rep)
        assert ost.apply(shard, rep)
        if flush_every and (i + 1) % flush_every == 0:
            e.flush()
    e.flush()
    assert db.latest_seq() == ost.latest_seq(shard)


def one_shot(db, lo=b"", hi=None):
    ents, info = db.scan_page(lo, hi, max_entries=1 << 16, cap=BIG)
    assert info.more == 0 and info.n == len(ents)
    return ents, info


def pages(db, lo, hi, max_entries, cap):
    """Manual paging with the documented resume rule -> [(ents, more)]."""
    out = []
    while True:
        ents, info = db.scan_page(lo, hi, max_entries=max_entries, cap=cap)
        out.append((ents, info.more))
        if not info.more:
            return out
        assert ents
        lo = ents[-1][0] + b"\x00"


# 1 ---------------------------------------------------------------- parity

@pytest.mark.parametrize("merge_op", [0, 1])
def test_scan_parity_small(olib, stream, merge_op):
    reps, universe, points = stream
    e = ra.Engine(nshards=1, merge_op=merge_op, **SMALL_ENGINE)
    db = e.open(0)
    ost = oracle_ffi.Store(olib, 1, merge_op=merge_op)
    apply_all(e, db, ost, reps, flush_every=10)  # 4 flushes
    nonempty = 0
    for lo, hi in ss.scan_set(6, universe):
        ents, info = one_shot(db, lo, hi)
        assert info.served_by == ra.GRA_SCAN_DEVICE, (lo, hi)
        assert ents == ss.expected(ost, 0, universe, lo, hi), (lo, hi)
        assert info.candidates == sum(ss.in_range(k, lo, hi) for k in points)
        nonempty += bool(ents)
    assert nonempty > 25
    # pagination over a mid range: max_entries 1 and 7, and a cap that cuts
    lo, hi = universe[5], universe[-5]
    want = ss.expected(ost, 0, universe, lo, hi)
    assert len(want) > 30
    for mx in (1, 7):
        got = pages(db, lo, hi, mx, BIG)
        assert [x for p, _ in got for x in p] == want
        assert [m for _, m in got] == [1] * (len(got) - 1) + [0]
    # the device path returns keys only for merge heads, so its byte cost
    # is at most key + value: twice the largest entry always makes progress
    cap = 2 * max(len(k) + len(v) for k, v in want) + 3
    got = pages(db, lo, hi, 1 << 16, cap)
    assert len(got) > 3
    assert [x for p, _ in got for x in p] == want
    e.close()


# 2 ------------------------------------------------- sort-size boundaries

def k12(i):
    """Distinct 12-byte keys sharing their first 8 bytes: every comparison
    the sort makes is decided by the full-key path."""
    return b"SAMEPFX8" + struct.pack(">I", i)


def load_k12(e, db, ost, n, seed):
    order = list(range(n))
    random.Random(seed).shuffle(order)
    for first in range(0, n, 1000):
        b = PyBatch()
        for i in order[first:first + 1000]:
            b.put(k12(i), struct.pack("<I", i))
        rep = b.data()
        assert db.handle_replicate_response(rep)
        assert ost.apply(0, rep)
    e.flush()


def test_scan_sort_size_boundaries(olib):
    n = 4200
    e = ra.Engine(nshards=1, **SMALL_ENGINE)
    db = e.open(0)
    ost = oracle_ffi.Store(olib, 1)
    load_k12(e, db, ost, n, seed=3)
    universe = [k12(i) for i in range(n)]
    for c in (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049,
              4097):
        lo, hi = k12(50), k12(50 + c)
        ents, info = one_shot(db, lo, hi)
        assert info.served_by == ra.GRA_SCAN_DEVICE
        assert info.candidates == c
        keys = [k for k, _ in ents]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)
        assert ents == ss.expected(ost, 0, universe, lo, hi, cap=64), c
    e.close()


def test_scan_candidate_regrow_on_first_scan(olib):
    """A fresh engine starts with room for at most 16384 candidates; its
    very first scan collects 20000 and must regrow and re-run."""
    n = 20000
    e = ra.Engine(nshards=1, **SMALL_ENGINE)
    db = e.open(0)
    ost = oracle_ffi.Store(olib, 1)
    load_k12(e, db, ost, n, seed=4)
    universe = [k12(i) for i in range(n)]
    ents, info = one_shot(db)
    assert info.served_by == ra.GRA_SCAN_DEVICE
    assert info.candidates == n
    keys = [k for k, _ in ents]
    assert keys == sorted(keys)
    assert ents == ss.expected(ost, 0, universe, b"", None, cap=64)
    # and a small scan on the grown buffers
    ents, info = one_shot(db, k12(7), k12(10))
    assert info.candidates == 3
    assert ents == ss.expected(ost, 0, universe, k12(7), k12(10))
    e.close()


# 3 ---------------------------------------------------------------- hot key

@pytest.mark.parametrize("ending", ["put", "delete", "merge"])
def test_scan_hot_key_newest_version_decides(olib, ending):
    rng = random.Random(11)
    hot = b"hot-key-0123"
    others = [b"hot-key-%04d" % i for i in range(25)] + \
             [b"hos-key-%04d" % i for i in range(25)]
    e = ra.Engine(nshards=1, **SMALL_ENGINE)
    db = e.open(0)
    ost = oracle_ffi.Store(olib, 1)
    b = PyBatch()
    for k in others:
        b.put(k, b"o" + k[-4:])
    reps = [b.data()]
    for run in range(3):  # 3000 versions over 3 runs
        b = PyBatch()
        for i in range(1000):
            x = rng.random()
            v = b"%d.%d" % (run, i)
            if x < 0.5:
                b.put(hot, v)
            elif x < 0.8:
                b.merge(hot, v)
            elif x < 0.9:
                b.delete(hot)
            else:
                b.single_delete(hot)
        reps.append(b.data())
    last = PyBatch()
    {"put": lambda: last.put(hot, b"final"),
     "delete": lambda: last.delete(hot),
     "merge": lambda: last.merge(hot, b"final")}[ending]()
    reps.append(last.data())
    apply_all(e, db, ost, reps, flush_every=1)
    universe = sorted(others + [hot])
    ents, info = one_shot(db)
    assert info.served_by == ra.GRA_SCAN_DEVICE
    assert info.candidates == 3001 + len(others)
    assert ents == ss.expected(ost, 0, universe, b"", None)
    assert (hot in dict(ents)) == (ending != "delete")
    if ending == "put":
        assert dict(ents)[hot] == b"final"
    e.close()


# 4 -------------------------------------------------------- range tombstones

def test_scan_range_tombstones(olib):
    cf = ss.CF
    reps = [
        PyBatch().put(b"a", b"1").put(b"b", b"2").put(b"c", b"3")
        .put(b"d", b"4").put(b"e", b"5").data(),
        PyBatch().delete_range(b"b", b"d").data(),   # newer than the Puts
        PyBatch().delete_range(b"f", b"h").data(),   # older than the Puts
        PyBatch().put(b"f", b"6").put(b"g", b"7").data(),
        PyBatch().merge(b"m", b"m1").data(),
        PyBatch().delete_range(b"m", b"n").data(),   # covers a Merge head
        PyBatch().put(b"c", b"again").data(),        # re-Put inside the tomb
        PyBatch().merge(b"p", b"p1").merge(b"p", b"p2").data(),  # live merge
        PyBatch().cf_put(cf, b"a", b"ca").cf_put(cf, b"b", b"cb")
        .cf_put(cf, b"c", b"cc").data(),
        PyBatch().cf_delete_range(cf, b"a", b"c").data(),  # cf-prefixed tomb
        PyBatch().cf_put(cf, b"b", b"cb2").data(),
    ]
    universe = sorted([b"a", b"b", b"c", b"d", b"e", b"f", b"g", b"m", b"p"] +
                      [ss.cfkey(cf, k) for k in (b"a", b"b", b"c")])
    e = ra.Engine(nshards=1, **SMALL_ENGINE)
    db = e.open(0)
    ost = oracle_ffi.Store(olib, 1)
    apply_all(e, db, ost, reps, flush_every=3)
    ranges = [(b"", None), (b"a", b"z"),
              (b"c", b"g"),      # tomb [b, d) only partly inside
              (b"a", b"c"), (b"m", b"n"), (b"l", b"q"),
              (ss.cfkey(cf, b""), ss.cfkey(cf + 1, b"")),
              (ss.cfkey(cf, b"b"), None)]
    for lo, hi in ranges:
        ents, info = one_shot(db, lo, hi)
        assert info.served_by == ra.GRA_SCAN_DEVICE
        assert ents == ss.expected(ost, 0, universe, lo, hi), (lo, hi)
    full = dict(one_shot(db)[0])
    assert b"b" not in full and b"m" not in full      # tombstoned
    assert full[b"c"] == b"again" and full[b"f"] == b"6"
    assert full[b"p"] == b"p1,p2"
    assert ss.cfkey(cf, b"a") not in full
    assert full[ss.cfkey(cf, b"b")] == b"cb2"
    # 4100 overlapping tombstones that meet the scanned range overflow the
    # device tombstone list (4096): the host path answers, same result
    reps2 = []
    for first in range(0, 4100, 1000):
        b = PyBatch()
        for i in range(first, min(first + 1000, 4100)):
            b.delete_range(b"q%04d" % i, b"q~")
        reps2.append(b.data())
    reps2.append(PyBatch().put(b"q5000", b"alive").put(b"q0001", b"x").data())
    apply_all(e, db, ost, reps2)
    universe = sorted(universe + [b"q5000", b"q0001"])
    for lo, hi in [(b"", None), (b"p", b"r")]:
        ents, info = one_shot(db, lo, hi)
        assert info.served_by == ra.GRA_SCAN_HOST
        assert info.candidates == 0
        assert ents == ss.expected(ost, 0, universe, lo, hi)
    assert dict(one_shot(db)[0])[b"q5000"] == b"alive"
    # a range none of them meets is still served on the device
    ents, info = one_shot(db, b"a", b"h")
    assert info.served_by == ra.GRA_SCAN_DEVICE
    assert ents == ss.expected(ost, 0, universe, b"a", b"h")
    e.close()


# 5 -------------------------------------------------------------- pagination

def test_scan_pagination_and_value_lengths(olib):
    e = ra.Engine(nshards=1, **SMALL_ENGINE)
    db = e.open(0)
    ost = oracle_ffi.Store(olib, 1)
    rng = random.Random(9)
    b = PyBatch()
    universe = []
    for i in range(60):  # values of 0, 1, 3 and 17 bytes
        k = b"p%03d" % i
        b.put(k, rng.randbytes((0, 1, 3, 17)[i % 4]))
        universe.append(k)
    for i in range(12):  # and 1001 bytes among them
        k = b"q%03d" % i
        b.put(k, rng.randbytes((1001, 0, 3)[i % 3]))
        universe.append(k)
    b.put(b"", b"")  # the empty key with an empty value costs 0 bytes
    universe = sorted(universe + [b""])
    apply_all(e, db, ost, [b.data()])
    want = ss.expected(ost, 0, universe, b"", None)
    assert len(want) == 73
    assert one_shot(db)[0] == want
    assert {len(v) for _, v in want} == {0, 1, 3, 17, 1001}
    for mx in (1, 7):
        assert list(db.scan(max_entries=mx, cap=BIG)) == want
        got = pages(db, b"", None, mx, BIG)
        assert [m for _, m in got] == [1] * (len(got) - 1) + [0]
        assert all(len(p) == mx for p, _ in got[:-1])
    assert list(db.scan(limit=10, max_entries=4)) == want[:10]
    # a 300-byte cap over the p-range (largest entry: 4 + 17 bytes)
    want_p = ss.expected(ost, 0, universe, b"p", b"q")
    assert list(db.scan(b"p", b"q", cap=300)) == want_p
    got = pages(db, b"p", b"q", 1 << 16, 300)
    assert len(got) > 1
    assert [x for p, _ in got for x in p] == want_p
    assert [m for _, m in got] == [1] * (len(got) - 1) + [0]
    assert all(sum(len(k) + len(v) for k, v in p) <= 300 for p, _ in got)
    # the first entry of the q-range needs 4 + 1001 bytes
    with pytest.raises(BufferError):
        db.scan_page(b"q", None, cap=300)
    with pytest.raises(BufferError):
        db.scan_page(b"q", None, cap=1004)
    ents, info = db.scan_page(b"q", None, cap=1005)
    assert ents == [want[61 + 0]] and info.more == 1 and info.buf_used == 1005
    e.close()


# 6 ------------------------------------------------------------- mixed shard

def test_scan_mixed_shard_takes_host_path(olib, stream):
    reps, universe, _ = stream
    e = ra.Engine(nshards=1, merge_op=1, **SMALL_ENGINE)
    db = e.open(0)
    ost = oracle_ffi.Store(olib, 1, merge_op=1)
    apply_all(e, db, ost, reps[:10], flush_every=5)
    lead = PyBatch().put(b"leader-key", b"lv").merge(b"abc", b"\x05").data()
    db.write_leader(lead)
    assert ost.apply(0, lead)
    universe = sorted(set(universe) | {b"leader-key", b"abc"})
    for lo, hi in [(b"", None), (b"a", b"m"), (universe[3], universe[40])]:
        ents, info = one_shot(db, lo, hi)
        assert info.served_by == ra.GRA_SCAN_HOST
        assert ents == ss.expected(ost, 0, universe, lo, hi)
    assert dict(one_shot(db)[0])[b"leader-key"] == b"lv"
    e.close()


# 7 ------------------------------------------------------------ replay path

def test_scan_replay_path(olib):
    nshards, nupd = 16, 30000
    arena, used, descs = ra.gen_stream(nshards=nshards, n_updates=nupd,
                                       key_len=16, val_len=32, kind=2,
                                       key_space=1 << 12, seed=77)
    raw = bytes(arena)[:used]
    ost = oracle_ffi.Store(olib, nshards, merge_op=1)
    points = {s: [] for s in range(nshards)}
    for i in range(nupd):  # the universe: every key the stream decodes to
        d = descs[i]
        blob = raw[d.off:d.off + d.len]
        assert ost.apply(d.shard, blob, d.ts)
        for r in oracle_ffi.decode(olib, blob)[2]:
            if r.consumes_seq and r.type != 0x0F:
                k = blob[r.key_off:r.key_off + r.key_len]
                points[d.shard].append(ss.cfkey(r.cf_id, k) if r.cf_id else k)
    e = ra.Engine(nshards=nshards + 1, merge_op=1, **SMALL_ENGINE)
    rep = e.upload(C.cast(arena, C.POINTER(C.c_uint8)), used, descs, nupd)
    for first in range(0, nupd, 5000):
        rep.tick(first, min(5000, nupd - first))
    rep.sync()
    rng = random.Random(5)
    for s in (0, 5, 10, 15):
        db = e.open(s)
        universe = sorted(set(points[s]))
        assert len(universe) > 100
        ranges = [(b"", None)]
        for _ in range(5):
            a, b = rng.choice(universe), rng.choice(universe)
            ranges.append((min(a, b), max(a, b)))
        for lo, hi in ranges:
            ents, info = one_shot(db, lo, hi)
            assert info.served_by == ra.GRA_SCAN_DEVICE
            assert info.candidates == sum(ss.in_range(k, lo, hi)
                                          for k in points[s])
            assert ents == ss.expected(ost, s, universe, lo, hi), (s, lo, hi)
        db.close()
    empty = e.open(nshards)  # a shard nothing was written to
    ents, info = empty.scan_page()
    assert ents == [] and info.n == 0 and info.more == 0
    e.close()
