"""gra_compact — a shard's device runs replaced by one key-sorted run — and
the indexed scan that enters it, against the CPU oracle and the Python shard
model (tests/fold_model.py). Expected values never come from the code under
test: reads are compared with orc_get, the store's content with a checksum
this file computes itself from the model."""
import random
import struct

import pytest

import fold_model as fm
import oracle_ffi
import rocksplicator_amd as ra
import scan_streams as ss
from pywb import PyBatch

pytestmark = pytest.mark.gpu

BIG = 1 << 22
SMALL_ENGINE = dict(store_bytes=256 << 20, staging_bytes=64 << 20)
MASK = (1 << 64) - 1
PUT = 1


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


def raw_scan(db, lo=b"", hi=None, max_entries=1 << 16, cap=BIG):
    """One page as the C ABI wrote it; every entry must be FOUND."""
    ents, info = db.scan_page_raw(lo, hi, max_entries, cap)
    assert all(st == ra.ffi.GRA_GET_FOUND for _, _, st in ents)
    return [(k, v) for k, v, _ in ents], info


def one_shot(db, lo=b"", hi=None):
    ents, info = raw_scan(db, lo, hi)
    assert info.more == 0 and info.n == len(ents)
    return ents, info


def pages(db, lo, hi, max_entries, cap):
    out = []
    while True:
        ents, info = raw_scan(db, lo, hi, max_entries, cap)
        out.append((ents, info.more))
        if not info.more:
            return out
        assert ents
        lo = ents[-1][0] + b"\x00"


def absent_keys(universe):
    out = [b"no-such-key-%02d" % i for i in range(20)]
    out += [ss.cfkey(ss.CF, b"nokey%d" % i) for i in range(5)]
    assert not set(out) & set(universe)
    return out


def check_point_reads(db, ost, keys, shard=0, raw=True):
    """multiget (as the C ABI answered when raw: FOUND or MISS, never
    NEEDS_HOST) and get against the oracle."""
    want = [ost.get(shard, k) for k in keys]
    if raw:
        got = db.multiget_raw(keys)
        for k, (st, vlen, val), w in zip(keys, got, want):
            if w is None:
                assert st == ra.ffi.GRA_GET_MISS, k
            else:
                assert st == ra.ffi.GRA_GET_FOUND and val == w, k
    else:
        assert db.multiget(keys) == want
    for k, w in zip(keys, want):
        assert db.get(k) == w, k
    return want


def rec_hash(seq, typ, key, val):
    """rec_hash_cs: FNV-1a 64 over seq LE8 | type | key_len LE4 | val_len
    LE4 | key | value."""
    h = 1469598103934665603
    for b in (struct.pack("<QBII", seq, typ, len(key), len(val)) + key + val):
        h = ((h ^ b) * 1099511628211) & MASK
    return h


def model_checksum(model, merge_op):
    """What gra_shard_checksum must report for a fully compacted shard: per
    live key one Put carrying its newest entry's seq and the folded value.
    -> (sum, live keys)"""
    total = n = 0
    for k in model.keys():
        v = model.value(k, merge_op)
        if v is not None:
            total = (total + rec_hash(model.ver[k][-1][0], PUT, k, v)) & MASK
            n += 1
    return total, n


# 1 ---------------------------------------------------------------- parity

@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("merge_op", [0, 1])
def test_compact_parity(olib, stream, merge_op, fold):
    reps, universe, _ = stream
    e = ra.Engine(nshards=1, merge_op=merge_op, fold_on_device=fold,
                  **SMALL_ENGINE)
    db = e.open(0)
    ost = oracle_ffi.Store(olib, 1, merge_op=merge_op)
    apply_all(e, db, ost, reps, flush_every=10)  # 4 runs
    live = [k for k in universe if ost.get(0, k) is not None]
    info = db.compact()
    assert info.status == ra.GRA_COMPACT_DONE
    assert info.runs_in == 4 and info.runs_after == 1
    assert info.entries_in == sum(len(fm.parse_rep(r)) for r in reps)
    assert info.entries_out == len(live) and len(live) > 50
    assert info.bytes_out < info.bytes_in
    nonempty = 0
    for lo, hi in ss.scan_set(6, universe):
        ents, sinfo = one_shot(db, lo, hi)
        assert sinfo.served_by == ra.GRA_SCAN_DEVICE_INDEXED, (lo, hi)
        assert ents == ss.expected(ost, 0, universe, lo, hi), (lo, hi)
        assert sinfo.candidates == len(ents)  # one entry per key is left
        nonempty += bool(ents)
    assert nonempty > 25
    # nothing is left to fold: FOUND or MISS with fold_on_device = 0 too
    check_point_reads(db, ost, universe + absent_keys(universe))
    lo, hi = universe[5], universe[-5]
    want = ss.expected(ost, 0, universe, lo, hi)
    assert len(want) > 30
    for mx in (1, 7):
        got = pages(db, lo, hi, mx, BIG)
        assert [x for p, _ in got for x in p] == want
        assert [m for _, m in got] == [1] * (len(got) - 1) + [0]
    cap = 2 * max(len(k) + len(v) for k, v in want) + 3
    got = pages(db, lo, hi, 1 << 16, cap)
    assert len(got) > 3
    assert [x for p, _ in got for x in p] == want
    e.close()


# 2 ------------------------------------------------------- content is pinned

@pytest.mark.parametrize("merge_op", [0, 1])
@pytest.mark.parametrize("kind", ["scan_stream", "counter_stream"])
def test_compact_content_checksum(olib, stream, merge_op, kind):
    """The store's content after compaction, record for record: head seq,
    Put tag, key and folded value of every live key, and nothing else."""
    reps = stream[0] if kind == "scan_stream" else fm.counter_stream(23)
    model = fm.Model(reps)  # assigns the seqs: consecutive per record
    e = ra.Engine(nshards=1, merge_op=merge_op, **SMALL_ENGINE)
    db = e.open(0)
    ost = oracle_ffi.Store(olib, 1, merge_op=merge_op)
    apply_all(e, db, ost, reps, flush_every=7)
    assert db.checksum() == olib.orc_shard_checksum(ost.h, 0)
    want, nlive = model_checksum(model, merge_op)
    for k in model.keys():  # the model's values are the oracle's
        assert model.value(k, merge_op) == ost.get(0, k), k
    info = db.compact()
    assert info.status == ra.GRA_COMPACT_DONE and info.entries_out == nlive
    assert db.checksum() == want
    e.close()


# 3 ---------------------------------------------------- newer runs on top

@pytest.mark.parametrize("merge_op", [0, 1])
def test_compact_then_newer_runs(olib, merge_op):
    reps = fm.counter_stream(31)
    half = fm.Model(reps[:20])
    live = [k for k in half.keys() if half.value(k, merge_op) is not None]
    chains = [k for k in live if half.live_chain(k) and not k.startswith(
        struct.pack("<I", ss.CF))]
    assert len(live) > 60 and len(chains) > 10
    # the second half also hits keys that live in the sorted run: a range
    # tombstone over some, a Delete of one, Merges over folded chains
    lo_i = len(live) // 3
    tomb_lo, tomb_hi = live[lo_i], live[lo_i + 6]
    victim = live[-3]
    chains = [k for k in chains
              if k != victim and not tomb_lo <= k < tomb_hi]
    merged = chains[:4] + chains[-4:]
    extra = PyBatch().delete_range(tomb_lo, tomb_hi).delete(victim)
    for i, k in enumerate(merged):
        extra.merge(k, struct.pack("<Q", 1000 + i))
    second = [extra.data()] + reps[20:]
    universe = fm.Model(reps).keys()

    e = ra.Engine(nshards=1, merge_op=merge_op, fold_on_device=1,
                  **SMALL_ENGINE)
    db = e.open(0)
    ost = oracle_ffi.Store(olib, 1, merge_op=merge_op)
    apply_all(e, db, ost, reps[:20], flush_every=5)
    info = db.compact()
    assert (info.status, info.runs_in, info.runs_after) == \
        (ra.GRA_COMPACT_DONE, 4, 1)
    assert db.checksum() == model_checksum(half, merge_op)[0]
    apply_all(e, db, ost, second[:1])
    assert ost.get(0, victim) is None and ost.get(0, tomb_lo) is None
    assert all(ost.get(0, k) is not None for k in merged)
    apply_all(e, db, ost, second[1:], flush_every=5)

    def check(indexed):
        for lo, hi in [(b"", None), (tomb_lo, tomb_hi), (live[3], live[-3]),
                       (universe[10], universe[40])]:
            ents, sinfo = one_shot(db, lo, hi)
            assert sinfo.served_by == indexed
            assert ents == ss.expected(ost, 0, universe, lo, hi), (lo, hi)
        # concat chains over the sorted run are not folded by multiget
        check_point_reads(db, ost, universe + absent_keys(universe),
                          raw=merge_op == 1)

    check(ra.GRA_SCAN_DEVICE_INDEXED)
    info = db.compact()  # the sorted run plus the 1 + 4 runs on top of it
    assert (info.status, info.runs_in, info.runs_after) == \
        (ra.GRA_COMPACT_DONE, 6, 1)
    check(ra.GRA_SCAN_DEVICE_INDEXED)
    full = fm.Model(reps[:20] + second)
    assert db.checksum() == model_checksum(full, merge_op)[0]
    e.close()


# 4 ------------------------------------------------------- size boundaries

def k12(i):
    """12-byte keys sharing their first 8 bytes (test_gpu_scan.load_k12)."""
    return b"SAMEPFX8" + struct.pack(">I", i)


SIZES = (1, 255, 256, 257, 1023, 1024, 1025, 2049, 4200)


def test_compact_size_boundaries(olib):
    e = ra.Engine(nshards=len(SIZES), **SMALL_ENGINE)
    ost = oracle_ffi.Store(olib, len(SIZES))
    dbs = [e.open(s) for s in range(len(SIZES))]
    for s, n in enumerate(SIZES):  # keys 2, 4, ..., 2n, shuffled, 500 a run
        order = list(range(1, n + 1))
        random.Random(n).shuffle(order)
        for first in range(0, n, 500):
            b = PyBatch()
            for i in order[first:first + 500]:
                b.put(k12(2 * i), struct.pack("<I", i))
            assert dbs[s].handle_replicate_response(b.data())
            assert ost.apply(s, b.data())
            e.flush()
    for s, n in enumerate(SIZES):
        db = dbs[s]
        info = db.compact()
        assert info.status == ra.GRA_COMPACT_DONE
        assert info.runs_in == (n + 499) // 500 and info.entries_out == n
        ents, sinfo = one_shot(db)
        assert sinfo.served_by == ra.GRA_SCAN_DEVICE_INDEXED
        assert sinfo.candidates == n
        assert ents == [(k12(2 * i), struct.pack("<I", i))
                        for i in range(1, n + 1)]
    db, n, s = dbs[-1], SIZES[-1], len(SIZES) - 1
    universe = [k12(2 * i) for i in range(1, n + 1)]
    ranges = [(k12(100), k12(100 + 2 * c))
              for c in (1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2048,
                        2049, 4097)]
    ranges += [
        (b"", k12(2)), (b"A", k12(3)), (b"SAMEPFX", k12(2) + b"\x00"),
        (k12(2 * n), None), (k12(2 * n + 1), None), (k12(2 * n - 1), b"T"),
        (k12(2 * n) + b"\x00", None), (b"T", None),         # past the last
        (b"", b"SAMEPFX8"), (b"A", b"B"),                   # before the first
        (k12(101), k12(103)), (k12(101), k12(102)), (k12(1001), k12(2001)),
        (k12(100), k12(100) + b"\x00"), (k12(100), k12(101)),
        (k12(100) + b"\x00", k12(102)), (k12(99), k12(100)),
        (k12(2), k12(2 * n)), (k12(2), k12(2 * n) + b"\x00"),
    ]
    for lo, hi in ranges:
        ents, sinfo = one_shot(db, lo, hi)
        want = ss.expected(ost, s, universe, lo, hi, cap=64)
        assert sinfo.served_by == ra.GRA_SCAN_DEVICE_INDEXED
        assert sinfo.candidates == len(want), (lo, hi)
        assert ents == want, (lo, hi)
    assert len(one_shot(db, *ranges[12])[0]) == 4097
    e.close()


@pytest.mark.parametrize("fold", [0, 1])
def test_scan_and_compact_share_staging(olib, fold):
    """gra_compact grows the staging buffers it shares with gra_scan past the
    capacity the scan sizes its launches by, between two scans; multiget
    batches grow, then shrink, on the same engine."""
    n = 20000
    e = ra.Engine(nshards=2, fold_on_device=fold, **SMALL_ENGINE)
    ost = oracle_ffi.Store(olib, 2)
    small, big = e.open(0), e.open(1)
    few = [k12(2 * i) for i in (1, 2, 3)]
    b = PyBatch()
    for i, k in enumerate(few):
        b.put(k, struct.pack("<I", i))
    apply_all(e, small, ost, [b.data()], shard=0)

    def scan_small():
        ents, sinfo = one_shot(small)
        assert sinfo.served_by == ra.GRA_SCAN_DEVICE
        assert len(ents) == 3 and ents == ss.expected(ost, 0, few, b"", None)

    scan_small()  # the scan's candidate capacity is now its first: 16384
    order = list(range(1, n + 1))
    random.Random(n).shuffle(order)
    reps = []
    for first in range(0, n, 1000):
        b = PyBatch()
        for i in order[first:first + 1000]:
            b.put(k12(2 * i), struct.pack("<I", i))
        reps.append(b.data())
    apply_all(e, big, ost, reps, flush_every=5, shard=1)  # 4 runs
    universe = [k12(2 * i) for i in range(1, n + 1)]
    info = big.compact()  # sized for 32768 candidates
    assert info.status == ra.GRA_COMPACT_DONE
    assert info.runs_in == 4 and info.entries_out == n
    scan_small()
    ents, sinfo = one_shot(big)  # 20000 > 16384: the scan's own regrow pass
    assert sinfo.candidates == n
    assert sinfo.served_by == ra.GRA_SCAN_DEVICE_INDEXED
    assert [k for k, _ in ents] == sorted(k for k, _ in ents)
    assert ents == ss.expected(ost, 1, universe, b"", None)
    lo, hi = k12(2 * 7001), k12(2 * 7004)
    ents, sinfo = one_shot(big, lo, hi)
    assert len(ents) == 3 and ents == ss.expected(ost, 1, universe, lo, hi)
    for s, db in enumerate((small, big)):
        assert db.checksum() == olib.orc_shard_checksum(ost.h, s)
    for first, count in ((9000, 4096), (123, 7)):  # stored and absent keys
        keys = [k12(j) for j in range(first, first + count)]
        for k, (st, _, val) in zip(keys, big.multiget_raw(keys)):
            want = ost.get(1, k)
            if want is None:
                assert st == ra.ffi.GRA_GET_MISS, k
            else:
                assert st == ra.ffi.GRA_GET_FOUND and val == want, k
    e.close()


# 5 ------------------------------------------------------------------ chains

U64_CHAINS = (1, 63, 64, 65, 320, 4000)
CONCAT_CHAINS = (1, 64, 256, 257, 300)
SHAPES = ("over_put", "over_nothing", "tomb_inside")


def chain_reps(rng, shape, nops):
    """A chain of nops operands on b"chain-key" (values of 0..12 bytes),
    800 records a batch, between two neighbours."""
    recs = [("put", b"chain-kex", b"left"), ("put", b"chain-kez", b"right")]
    if shape == "over_put":
        recs.append(("put", b"chain-key", rng.randbytes(rng.randrange(13))))
    for i in range(nops):
        if shape == "tomb_inside" and i == nops // 2:
            recs.append(("tomb", b"chain-key", b"chain-key\x00"))
        recs.append(("merge", b"chain-key", rng.randbytes(rng.randrange(13))))
    reps = []
    for first in range(0, len(recs), 800):
        b = PyBatch()
        for op, k, v in recs[first:first + 800]:
            {"put": b.put, "merge": b.merge, "tomb": b.delete_range}[op](k, v)
        reps.append(b.data())
    return reps


@pytest.mark.parametrize("merge_op,lengths", [(1, U64_CHAINS),
                                              (0, CONCAT_CHAINS)])
def test_compact_chains(olib, merge_op, lengths):
    rng = random.Random(41 + merge_op)
    cases = [(n, shape) for n in lengths for shape in SHAPES]
    e = ra.Engine(nshards=len(cases), merge_op=merge_op, **SMALL_ENGINE)
    ost = oracle_ffi.Store(olib, len(cases), merge_op=merge_op)
    models = []
    for s, (n, shape) in enumerate(cases):
        reps = chain_reps(rng, shape, n)
        models.append(fm.Model(reps))
        apply_all(e, e.open(s), ost, reps, flush_every=1, shard=s)
    keys = [b"chain-kex", b"chain-key", b"chain-kez", b"chain-kf"]
    for s, (n, shape) in enumerate(cases):
        db, model = e.open(s), models[s]
        look = model.look(b"chain-key")
        assert len(look["ops"]) == (n - n // 2 if shape == "tomb_inside"
                                    else n)
        assert (look["base"] is not None) == (shape == "over_put")
        want = model.value(b"chain-key", merge_op)
        assert want == ost.get(s, b"chain-key", 1 << 20)
        info = db.compact()
        assert info.status == ra.GRA_COMPACT_DONE, (n, shape)
        assert info.entries_out == 3 and info.runs_after == 1
        assert db.checksum() == model_checksum(model, merge_op)[0], (n, shape)
        ents, sinfo = one_shot(db)
        assert sinfo.served_by == ra.GRA_SCAN_DEVICE_INDEXED
        assert ents == [(b"chain-kex", b"left"), (b"chain-key", want),
                        (b"chain-kez", b"right")], (n, shape)
        check_point_reads(db, ost, keys, shard=s)
    e.close()


# 6 ------------------------------------------------------ mixed and refused

def stored_bytes(reps_per_tick):
    """Arena bytes the apply path takes for ticks of these reps: per tick a
    header array padded to 16 B, per record its key and value padded to
    16 B."""
    total = 0
    for reps in reps_per_tick:
        recs = [r for rep in reps for r in fm.parse_rep(rep)]
        total += (24 * len(recs) + 15) & ~15
        total += sum((len(k) + len(v) + 15) & ~15 for _, k, v in recs)
    return total


def test_compact_mixed_shard_takes_the_device_prefix(olib, stream):
    reps, universe, _ = stream
    e = ra.Engine(nshards=3, merge_op=1, **SMALL_ENGINE)
    db = e.open(0)
    ost = oracle_ffi.Store(olib, 3, merge_op=1)
    apply_all(e, db, ost, reps[:10], flush_every=5)
    lead = PyBatch().put(b"leader-key", b"lv").merge(b"abc", b"\x05").data()
    db.write_leader(lead)
    assert ost.apply(0, lead)
    universe = sorted(set(universe) | {b"leader-key", b"abc"})
    info = db.compact()
    assert (info.status, info.runs_in, info.runs_after) == \
        (ra.GRA_COMPACT_DONE, 2, 2)
    for lo, hi in [(b"", None), (b"a", b"m"), (universe[3], universe[40])]:
        ents, sinfo = one_shot(db, lo, hi)
        assert sinfo.served_by == ra.GRA_SCAN_HOST
        assert ents == ss.expected(ost, 0, universe, lo, hi)
    check_point_reads(db, ost, universe, raw=False)
    # an already-compacted prefix, a leader-only shard, an empty shard
    before = db.checksum()
    lead_only = e.open(1)
    lead_only.write_leader(lead)
    for d, runs in ((db, 2), (lead_only, 1), (e.open(2), 0)):
        info = d.compact()
        assert info.status == ra.GRA_COMPACT_NOTHING
        assert info.runs_in == 0 and info.runs_after == runs
        assert info.entries_out == 0 and info.bytes_out == 0
    assert db.checksum() == before
    assert lead_only.get(b"leader-key") == b"lv"
    e.close()


def test_compact_refused_on_a_ring_store():
    e = ra.Engine(nshards=1, store_ring=1, **SMALL_ENGINE)
    db = e.open(0)
    assert db.handle_replicate_response(PyBatch().put(b"k", b"v").data())
    e.flush()
    with pytest.raises(RuntimeError, match="store_ring"):
        db.compact()
    e.close()


def test_compact_arena_full(olib, stream):
    reps, universe, _ = stream
    reps = reps[:20]
    ticks = [reps[i:i + 5] for i in range(0, 20, 5)]
    used = stored_bytes(ticks)
    ost = oracle_ffi.Store(olib, 1, merge_op=0)
    for rep in reps:
        assert ost.apply(0, rep)
    live = [(k, ost.get(0, k)) for k in universe]
    live = [(k, v) for k, v in live if v is not None]
    out_bytes = ((24 * len(live) + 15) & ~15) + \
        sum((len(k) + len(v) + 15) & ~15 for k, v in live)
    slack = 1024  # the arena holds the input and 1 KiB more
    assert out_bytes > 2 * slack
    e = ra.Engine(nshards=1, merge_op=0, store_bytes=used + slack,
                  staging_bytes=64 << 20)
    db = e.open(0)
    for t in ticks:
        for rep in t:
            assert db.handle_replicate_response(rep)
        e.flush()
    assert db.latest_seq() == ost.latest_seq(0)
    before = db.checksum()
    assert before == olib.orc_shard_checksum(ost.h, 0)
    with pytest.raises(ra.StoreFullError):
        db.compact()
    assert db.checksum() == before  # untouched: the shard answers as before
    ents, sinfo = one_shot_any(db)
    assert sinfo.served_by == ra.GRA_SCAN_DEVICE and ents == live
    e.close()
    # the same shard with room for the output compacts
    e = ra.Engine(nshards=1, merge_op=0, store_bytes=used + out_bytes,
                  staging_bytes=64 << 20)
    db = e.open(0)
    for t in ticks:
        for rep in t:
            assert db.handle_replicate_response(rep)
        e.flush()
    info = db.compact()
    assert info.status == ra.GRA_COMPACT_DONE
    assert info.bytes_in == sum(
        24 + ((len(k) + len(v) + 15) & ~15)
        for rep in reps for _, k, v in fm.parse_rep(rep))
    assert info.bytes_out == sum(
        24 + ((len(k) + len(v) + 15) & ~15) for k, v in live)
    assert one_shot(db)[0] == live
    e.close()


def one_shot_any(db, lo=b"", hi=None):
    """One page with the host fold for keys the device left alone."""
    ents, info = db.scan_page(lo, hi, max_entries=1 << 16, cap=BIG)
    assert info.more == 0 and info.n == len(ents)
    return ents, info


def test_compact_too_many_range_tombstones(olib):
    e = ra.Engine(nshards=1, **SMALL_ENGINE)
    db = e.open(0)
    ost = oracle_ffi.Store(olib, 1)
    reps = [PyBatch().put(b"q0001", b"x").put(b"a", b"1").data()]
    for first in range(0, 4100, 1000):
        b = PyBatch()
        for i in range(first, min(first + 1000, 4100)):
            b.delete_range(b"q%04d" % i, b"q~")
        reps.append(b.data())
    reps.append(PyBatch().put(b"q5000", b"alive").data())
    apply_all(e, db, ost, reps, flush_every=2)
    before = db.checksum()
    info = db.compact()
    assert info.status == ra.GRA_COMPACT_UNSUPPORTED
    assert info.runs_in == 0 and info.runs_after == 4
    assert info.entries_in == 4103 and info.entries_out == 0
    assert db.checksum() == before == olib.orc_shard_checksum(ost.h, 0)
    universe = [b"a", b"q0001", b"q5000"]
    ents, sinfo = one_shot_any(db)
    assert sinfo.served_by == ra.GRA_SCAN_HOST  # as before the call
    assert ents == [(b"a", b"1"), (b"q5000", b"alive")]
    assert ents == ss.expected(ost, 0, universe, b"", None)
    check_point_reads(db, ost, universe, raw=False)
    e.close()


# 7 ---------------------------------------------------------- default unchanged

def test_never_compacted_shard_scans_as_before(olib, stream):
    reps, universe, points = stream
    e = ra.Engine(nshards=1, **SMALL_ENGINE)
    db = e.open(0)
    ost = oracle_ffi.Store(olib, 1)
    apply_all(e, db, ost, reps[:12], flush_every=4)
    pts = [k for rep in reps[:12] for t, k, _ in fm.parse_rep(rep)
           if t != fm.RANGE_DELETE]
    for lo, hi in ss.scan_set(6, universe)[:12]:
        ents, sinfo = one_shot_any(db, lo, hi)
        assert sinfo.served_by == ra.GRA_SCAN_DEVICE
        assert sinfo.candidates == sum(ss.in_range(k, lo, hi) for k in pts)
        assert ents == ss.expected(ost, 0, universe, lo, hi), (lo, hi)
    e.close()
