"""The device Snappy stage (k_snappy -> snp::decompress, device build)
against the oracle, element by element.

The device build of snp::decompress moves literals and copies in 16- and
8-byte chunks, overshoots an element's end into the slot slack, and reads
its stream out of an LDS stage when it is at most 508 bytes long; none of
that runs in a host test. The streams come from snappy_cases.py, whose
claims test_snappy_cases_host.py checks on the CPU.

Expected state comes from the oracle and the transport metadata only
(snappy_cases.Expected): updates in tick order; an update of a poisoned
shard is skipped; an update is good when the oracle decompresses it within
ulen_meta bytes, to exactly ulen_meta bytes, and the oracle store applies
the result; an update that is not good poisons its shard. Every comparison
is exact: latest_seq, the full-store checksum and a get of every key of the
case, per shard, and the engine's update and record totals where no shard
is poisoned.
"""
import ctypes as C

import pytest

import pysnappy as ps
import rocksplicator_amd as ra
import snappy_cases as sc
from pywb import PyBatch
from rocksplicator_amd.ffi import GraUpdateDesc

pytestmark = pytest.mark.gpu

STORE = 64 << 20
TS = 7
GET_CAP = 1 << 17  # the longest value of the table is about 70 KB


def _flat(table):
    """Case table -> [(shard, comp, ulen, count)], one shard per case."""
    return [(s, comp, ulen, count)
            for s, (_, ups) in enumerate(table) for comp, ulen, count in ups]


def _keys(table):
    return {s: sc.INFO[name]["keys"] for s, (name, _) in enumerate(table)}


def _upload(e, ticks):
    ups = [u for t in ticks for u in t]
    descs = (GraUpdateDesc * len(ups))()
    off = 0
    for d, (shard, comp, _, _) in zip(descs, ups):
        d.shard, d.len, d.off, d.ts = shard, len(comp), off, TS
        off += len(comp)
    raw = b"".join(u[1] for u in ups)
    arena = (C.c_uint8 * (len(raw) + 16)).from_buffer_copy(raw + bytes(16))
    return e.upload_snappy(C.cast(arena, C.POINTER(C.c_uint8)), len(raw), descs,
                           len(ups), [u[2] for u in ups], [u[3] for u in ups])


def _check(e, exp, nshards, keys, names=None):
    for s in range(nshards):
        who = (s, names[s] if names else None)
        db = e.open(s)
        assert db.latest_seq() == exp.seq(s), who
        assert db.checksum() == exp.checksum(s), who
        for k in keys.get(s, ()):
            assert db.get(k, GET_CAP) == exp.get(s, k), (who, k)
        db.close()
    if not exp.poisoned:
        st = e.stats()
        assert st.updates == exp.applied
        assert st.records == sum(exp.seq(s) for s in range(nshards))


def _run(nshards, ticks, keys, names=None, poisoned=None):
    """One engine, one upload, one tick per window; then compare every
    shard with the expected state. Returns (engine, expected): the caller
    closes the engine."""
    exp = sc.Expected(nshards)
    for t in ticks:
        for shard, comp, ulen, _ in t:
            exp.feed(shard, comp, ulen, TS)
    if poisoned is not None:
        assert exp.poisoned == poisoned
    e = ra.Engine(nshards=nshards, store_bytes=STORE)
    try:
        rep = _upload(e, ticks)
        first = 0
        for t in ticks:
            rep.tick(first, len(t))
            first += len(t)
        rep.sync()
        _check(e, exp, nshards, keys, names)
    except BaseException:
        e.close()
        raise
    return e, exp


def _windows(ups, w):
    return [ups[i:i + w] for i in range(0, len(ups), w)] if w else [ups]


@pytest.mark.parametrize("window", [None, 1, 255, 256, 257])
def test_valid_elements(window):
    """Every valid case, one shard each: all in one tick, then in ticks of
    1, 255, 256 and 257 updates (a full block of 256 lanes, one lane less,
    one more, and a ragged last tick)."""
    table = sc.valid_cases()
    ups = _flat(table)
    assert len(ups) > 257
    e, exp = _run(len(table), _windows(ups, window), _keys(table),
                  names=[n for n, _ in table], poisoned=set())
    e.close()
    assert exp.applied == len(ups)


@pytest.mark.parametrize("order", ["short_first", "long_first", "interleaved"])
def test_stage_boundary_mixed_window(order):
    """300 streams of 380..639 compressed bytes in one tick: the length
    sort puts staged (<= 508) and global-memory streams into the same block
    of 256. The arena holds the two kinds in either order, or interleaved."""
    mix = list(sc.mixed_window())
    if order != "interleaved":
        mix.sort(key=lambda m: (len(m[1]) > 508) == (order == "short_first"))
    assert (len(mix[0][1]) <= 508) == (order != "long_first")
    ups = [m[:4] for m in mix]
    keys = {}
    for shard, _, _, _, _, key in mix:
        keys.setdefault(shard, []).append(key)
    e, exp = _run(4, [ups], keys, poisoned=set())
    e.close()
    assert exp.applied == 300


def test_multi_record_counts():
    """Batches of 2, 7 and 64 records: the base seqs of what follows them
    in the shard come from the host-supplied counts, so each multi-record
    update is followed by a single Put on the same shard."""
    table = [(n, u) for n, u in sc.valid_cases() if "multi_" in n]
    counts = [u[0][2] for _, u in table]
    assert sorted(counts) == sorted([2, 7, 64] * 3)  # built, gra:, orc:
    keys = _keys(table)
    ups = []
    for s, comp, ulen, count in _flat(table):
        ups.append((s, comp, ulen, count))
        tail = PyBatch().put(b"after-%d" % s, sc.val(33, s)).data()
        ups.append((s, ps.encode_with(tail, ps.Policy("copy2")), len(tail), 1))
        keys[s] = keys[s] + [b"after-%d" % s]
    e, exp = _run(len(table), [ups], keys, names=[n for n, _ in table],
                  poisoned=set())
    e.close()
    assert [exp.seq(s) for s in range(len(table))] == [c + 1 for c in counts]


# ------------------------------------------------------------- malformed

def _good(shard, tick):
    key = b"t%d-s%03d" % (tick, shard)
    blob = PyBatch().put(key, sc.val(90 + shard, tick * 50 + shard)).data()
    return (shard, ps.encode_with(blob, ps.Policy("copy2")), len(blob), 1), key, blob


def _malformed_plan():
    """Shard 2i holds malformed case i, shard 2i + 1 a valid case, so every
    bad slot has good neighbours on both sides in arena order (the first
    has one after it and the tick-1 slots before it).
    -> (nshards, per-shard middle update, keys, names, bad shards)"""
    bad = sc.malformed_cases()
    small = [(n, u) for n, u in sc.valid_cases() if len(u[0][0]) < 600]
    valid = small[::len(small) // len(bad)][:len(bad)]
    assert len(valid) == len(bad)
    middle, keys, names = [], {}, []
    for i, (b, v) in enumerate(zip(bad, valid)):
        for s, (name, ups) in ((2 * i, b), (2 * i + 1, v)):
            comp, ulen, count = ups[0]
            middle.append((s, comp, ulen, count))
            keys[s] = list(sc.INFO[name]["keys"])
            names.append(name)
    return 2 * len(bad), middle, keys, names, set(range(0, 2 * len(bad), 2))


def test_malformed_isolated():
    """Tick 1: a good update per shard. Tick 2: malformed and valid cases
    alternating. Tick 3: another good update per shard, which is stale for
    a shard that tick 2 poisoned. Shards with a bad case keep exactly
    tick 1; all others hold all three. Then the reference cadence on one
    poisoned shard: the next response fails once, the re-pull applies."""
    nshards, middle, keys, names, bad = _malformed_plan()
    t1, t3 = [], []
    for s in range(nshards):
        for tick, into in ((1, t1), (3, t3)):
            up, key, _ = _good(s, tick)
            into.append(up)
            keys[s].append(key)
    e, exp = _run(nshards, [t1, middle, t3], keys, names, poisoned=bad)
    try:
        for s in range(nshards):
            assert exp.seq(s) == (1 if s in bad else 3), names[s]
        s = sorted(bad)[3]
        db = e.open(s)
        _, key, blob = _good(s, 3)
        assert db.get(key) is None
        assert not db.handle_replicate_response(blob, ts=TS)  # fail once
        assert db.handle_replicate_response(blob, ts=TS)      # the re-pull
        e.flush()
        assert exp.ost.apply(s, blob, TS)
        assert db.latest_seq() == exp.seq(s) == 2
        assert db.checksum() == exp.checksum(s)
        assert db.get(key) == exp.get(s, key) != None  # noqa: E711
        db.close()
    finally:
        e.close()


def test_malformed_same_tick():
    """The same content as one shard-grouped tick: good, case, good per
    shard. A bad case cuts its shard after the first update."""
    nshards, middle, keys, names, bad = _malformed_plan()
    tick = []
    for up in middle:
        s = up[0]
        first, k1, _ = _good(s, 1)
        last, k3, _ = _good(s, 3)
        tick += [first, up, last]
        keys[s] += [k1, k3]
    e, exp = _run(nshards, [tick], keys, names, poisoned=bad)
    e.close()
    for s in range(nshards):
        assert exp.seq(s) == (1 if s in bad else 3), names[s]


def test_mutants_match_oracle():
    """300 seeded single-byte mutations and truncations of valid streams,
    one shard each, in three ticks. The oracle accepts and applies 128 of
    them and rejects 172 (test_snappy_cases_host.py asserts the counts);
    the device must poison exactly the shards of the rejected ones and
    hold the oracle's bytes in all others."""
    table = sc.mutants()
    ups = _flat(table)
    e, exp = _run(len(table), _windows(ups, 100), _keys(table),
                  names=[n for n, _ in table])
    e.close()
    assert exp.applied >= 30 and len(exp.poisoned) >= 30
    assert exp.applied + len(exp.poisoned) == 300


def test_upload_rejects_ulen_below_header():
    """ulen metadata below the 12-byte batch header: upload_snappy raises
    and no shard's seq moves."""
    e = ra.Engine(nshards=2, store_bytes=STORE)
    try:
        dbs = [e.open(s) for s in range(2)]
        for s in range(2):
            assert dbs[s].handle_replicate_response(_good(s, 1)[2], ts=TS)
        e.flush()
        ups = [_good(0, 3)[0], (1, ps.stream(11, [ps.literal(b"x" * 11)]), 11, 1),
               _good(1, 3)[0]]
        with pytest.raises(RuntimeError, match="bad desc"):
            _upload(e, [ups])
        assert [db.latest_seq() for db in dbs] == [1, 1]
    finally:
        e.close()
