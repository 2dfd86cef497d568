"""gra_export / gra_import — a shard captured as one self-checking image and
installed in an empty shard so that replication resumes behind it — against
the CPU oracle, the Python shard model (tests/fold_model.py) and the tests'
own byte-level statement of the format (tests/pyimage.py). Expected images,
verdicts and values never come from the code under test. The hostile table
is the one tests/test_image_host.py runs on the host under the sanitizer."""
import struct

import pytest

import fold_model as fm
import oracle_ffi
import pyimage
import rocksplicator_amd as ra
import scan_streams as ss
from pywb import PyBatch
from rocksplicator_amd import replicator as rp

pytestmark = pytest.mark.gpu

BIG = 1 << 22
SMALL_ENGINE = dict(store_bytes=256 << 20, staging_bytes=64 << 20)
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def olib():
    return oracle_ffi.load()


@pytest.fixture(scope="module")
def stream():
    return ss.make_stream(seed=27, n_records=4000, n_batches=40)


@pytest.fixture(scope="module")
def more():
    """10 more batches, over another draw of the key pool."""
    return ss.make_stream(seed=28, n_records=1000, n_batches=10)


@pytest.fixture(scope="module")
def hostile():
    return pyimage.hostile_table(600)


def apply_all(e, db, ost, reps, flush_every=None, shard=0, oshard=0):
    for i, rep in enumerate(reps):
        assert db.handle_replicate_response(rep)
        if ost is not None:
            assert ost.apply(oshard, rep)
        if flush_every and (i + 1) % flush_every == 0:
            e.flush()
    e.flush()


def full_scan(db):
    """Every page of the whole range, host fold where the device left a
    chain alone -> ([(key, value)], served_by of the first page)."""
    out, lo, served = [], b"", None
    while True:
        ents, info = db.scan_page(lo, None, max_entries=1 << 16, cap=BIG)
        served = info.served_by if served is None else served
        out += ents
        if not info.more:
            return out, served
        lo = ents[-1][0] + b"\x00"


def absent_keys(universe):
    out = [b"no-such-key-%02d" % i for i in range(20)]
    out += [ss.cfkey(ss.CF, b"nokey%d" % i) for i in range(5)]
    assert not set(out) & set(universe)
    return out


def check_reads(db, ost, universe, raw, oshard=0):
    """get, multiget (as the C ABI answered when raw) and the full scan
    against the oracle; absent keys and cf keys included."""
    keys = universe + absent_keys(universe)
    assert any(k.startswith(struct.pack("<I", ss.CF)) for k in universe)
    want = [ost.get(oshard, k) for k in keys]
    if raw:
        for k, (st, _, val), w in zip(keys, db.multiget_raw(keys), want):
            if w is None:
                assert st == ra.ffi.GRA_GET_MISS, k
            else:
                assert st == ra.ffi.GRA_GET_FOUND and val == w, k
    else:
        assert db.multiget(keys) == want
    for k, w in zip(keys, want):
        assert db.get(k) == w, k
    ents, served = full_scan(db)
    assert ents == [(k, w) for k, w in zip(keys, want) if w is not None]
    return served


def model_checksum(items):
    return sum(pyimage.rec_hash(s, pyimage.PUT, k, v)
               for k, v, s in items) & MASK


# 1 ------------------------------------------------------ export is the model

@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("merge_op", [0, 1])
def test_export_is_the_model(olib, stream, merge_op, fold):
    reps, universe, _ = stream
    e = ra.Engine(nshards=2, merge_op=merge_op, fold_on_device=fold,
                  **SMALL_ENGINE)
    db = e.open(0)
    img, info = e.open(1).export_image(with_info=True)  # the empty shard
    assert img == pyimage.pack([], 0, merge_op) and len(img) == 64
    assert info.n_entries == 0 and info.image_bytes == 64
    ost = oracle_ffi.Store(olib, 1, merge_op=merge_op)
    apply_all(e, db, ost, reps, flush_every=10)  # 4 runs
    model = fm.Model(reps)
    S = model.t
    assert db.latest_seq() == S == ost.latest_seq(0)
    items = pyimage.items_from_model(model, merge_op)
    assert len(items) > 50
    for k, v, _ in items:  # the model's values are the oracle's
        assert v == ost.get(0, k), k
    want = pyimage.pack(items, S, merge_op)
    used = e.store_usage().used
    cs = db.checksum()
    assert cs == olib.orc_shard_checksum(ost.h, 0)
    img, info = db.export_image(with_info=True)
    assert info.served_by == 0
    assert (info.n_entries, info.last_seq, info.image_bytes) == \
        (len(items), S, len(want))
    assert img == want
    assert pyimage.verdict(img) == (pyimage.OK, pyimage.NO_INDEX)
    # the store is untouched
    assert e.store_usage().used == used
    assert db.checksum() == cs
    assert db.latest_seq() == S
    assert check_reads(db, ost, universe, raw=False) == ra.GRA_SCAN_DEVICE
    assert db.export_image(cap=len(want)) == want  # and again, the same
    assert e.store_usage().used == used
    cinfo = db.compact()  # the list still held the four runs
    assert (cinfo.status, cinfo.runs_in) == (ra.GRA_COMPACT_DONE, 4)
    assert db.export_image() == want  # one sorted run exports the same bytes
    e.close()


# 2 ------------------------------------------------------ two paths, one image

@pytest.mark.parametrize("merge_op", [0, 1])
def test_host_path_and_device_chain_write_the_same_bytes(olib, stream,
                                                         merge_op):
    reps = stream[0]
    model = fm.Model(reps)
    want = pyimage.pack(pyimage.items_from_model(model, merge_op), model.t,
                        merge_op)
    e = ra.Engine(nshards=3, merge_op=merge_op, **SMALL_ENGINE)
    follower, leader, mixed = e.open(0), e.open(1), e.open(2)
    apply_all(e, follower, None, reps, flush_every=10)
    for rep in reps:
        leader.write_leader(rep)
    apply_all(e, mixed, None, reps[:20], flush_every=10)
    for rep in reps[20:]:
        mixed.write_leader(rep)
    used = e.store_usage().used
    f_img, f_info = follower.export_image(with_info=True)
    l_img, l_info = leader.export_image(with_info=True)
    m_img, m_info = mixed.export_image(with_info=True)
    assert (f_info.served_by, l_info.served_by, m_info.served_by) == (0, 1, 1)
    assert f_img == want
    assert l_img == f_img and m_img == f_img
    assert l_info.content_sum == f_info.content_sum == \
        pyimage.fields(want)["content_sum"]
    assert e.store_usage().used == used
    e.close()


# 3 ------------------------------------------------------ round trip and resume

@pytest.mark.parametrize("merge_op", [0, 1])
def test_round_trip_and_resume(olib, stream, more, merge_op):
    reps, universe, _ = stream
    src_e = ra.Engine(nshards=1, merge_op=merge_op, **SMALL_ENGINE)
    dst_e = ra.Engine(nshards=1, merge_op=merge_op, fold_on_device=1,
                      **SMALL_ENGINE)
    src, dst = src_e.open(0), dst_e.open(0)
    ost = oracle_ffi.Store(olib, 1, merge_op=merge_op)
    apply_all(src_e, src, ost, reps, flush_every=10)
    model = fm.Model(reps)
    S = model.t
    img = src.export_image()
    info = dst.import_image(img)
    assert (info.reason, info.n_entries, info.last_seq) == \
        (ra.GRA_IMG_OK, pyimage.fields(img)["n"], S)
    assert dst.latest_seq() == S
    assert dst.counters()["latest_seq"] == S
    # every key is one Put now: FOUND or MISS from the device, nothing to fold
    assert check_reads(dst, ost, universe, raw=True) == \
        ra.GRA_SCAN_DEVICE_INDEXED
    lo, hi = universe[5], universe[-5]
    want = ss.expected(ost, 0, universe, lo, hi)
    got, page_lo = [], lo
    while True:  # paged
        ents, sinfo = dst.scan_page_raw(page_lo, hi, 7, BIG)
        assert sinfo.served_by == ra.GRA_SCAN_DEVICE_INDEXED
        got += [(k, v) for k, v, st in ents if st == ra.ffi.GRA_GET_FOUND]
        if not sinfo.more:
            break
        page_lo = ents[-1][0] + b"\x00"
    assert got == want and len(want) > 30
    assert dst.checksum() == model_checksum(
        pyimage.items_from_model(model, merge_op))
    # replication resumes behind the image: the same batches on both sides
    reps2, universe2, _ = more
    apply_all(src_e, src, ost, reps2, flush_every=5)
    apply_all(dst_e, dst, None, reps2, flush_every=5)
    assert dst.latest_seq() == src.latest_seq() == ost.latest_seq(0)
    both = sorted(set(universe) | set(universe2))
    for db in (src, dst):
        check_reads(db, ost, both, raw=False)
    cinfo = dst.compact()
    assert (cinfo.status, cinfo.runs_in, cinfo.runs_after) == \
        (ra.GRA_COMPACT_DONE, 3, 1)
    check_reads(dst, ost, both, raw=True)
    rinfo = dst_e.reclaim()
    assert rinfo.status == ra.GRA_RECLAIM_DONE
    assert check_reads(dst, ost, both, raw=True) == ra.GRA_SCAN_DEVICE_INDEXED
    # both sides hold the same shard: their images are the same bytes
    assert dst.export_image() == src.export_image()
    src_e.close()
    dst_e.close()


# 4 ------------------------------------------- sizes that can break the kernel

SIZES = (1, 255, 256, 257, 1025)


def sized_items(n):
    """n ascending keys: the empty key, then keys sharing a 200-byte prefix,
    every seventh followed by its own extension (a key that is a prefix of
    the next); values of 0 bytes, values that make the record exactly 16 k
    and 16 k + 1 bytes, and 5-byte values."""
    keys = [b""]
    i = 0
    while len(keys) < n:
        base = b"p" * 200 + struct.pack(">I", i)
        keys.append(base)
        if i % 7 == 0 and len(keys) < n:
            keys.append(base + b"\x00")
        i += 1
    assert keys == sorted(set(keys)) and len(keys) == n
    items = []
    for j, k in enumerate(keys):
        fill = -len(k) % 16 or 16
        vlen = (5, 0, fill, fill + 1)[j % 4] if n > 1 else 16
        items.append((k, bytes((j + b) & 0xFF for b in range(vlen)), j + 1))
    return items


def test_import_size_boundaries():
    e = ra.Engine(nshards=len(SIZES), **SMALL_ENGINE)
    for s, n in enumerate(SIZES):
        items = sized_items(n)
        img = pyimage.pack(items, n + 5, 0)
        assert pyimage.verdict(img) == (pyimage.OK, pyimage.NO_INDEX)
        db = e.open(s)
        info = db.import_image(img)
        assert info.reason == ra.GRA_IMG_OK and info.n_entries == n
        assert db.latest_seq() == n + 5
        ents, served = full_scan(db)
        assert served == ra.GRA_SCAN_DEVICE_INDEXED
        assert ents == [(k, v) for k, v, _ in items], n
        assert db.checksum() == model_checksum(items)
        out, oinfo = db.export_image(with_info=True)
        assert oinfo.served_by == 0
        assert out == img, n
    e.close()


# 5 ------------------------------------------------ the hostile table, on device

def test_hostile_images_are_rejected_on_the_device(hostile):
    good, cases = hostile
    e = ra.Engine(nshards=1, **SMALL_ENGINE)
    db = e.open(0)
    assert e.store_usage().used == 0
    seen = set()
    for name, img, header_level in cases:
        want = pyimage.verdict(img)
        assert want[0] != pyimage.OK
        assert header_level == (want[0] in (pyimage.BAD_HEADER,
                                            pyimage.BAD_SIZE)), name
        with pytest.raises(ra.ImageRejected) as exc:
            db.import_image(img)
        got = exc.value.info
        assert (got.reason, got.bad_index) == want, name
        seen.add(want[0])
        # the engine is untouched
        assert e.store_usage().used == 0, name
        assert db.latest_seq() == 0, name
        ents, info = db.scan_page_raw()
        assert ents == [] and info.n == 0, name
    assert seen == {1, 2, 3, 4, 5, 6}
    info = db.import_image(good)  # the same shard takes a good image
    assert info.reason == ra.GRA_IMG_OK
    _, items = pyimage.unpack(good)
    assert db.latest_seq() == pyimage.fields(good)["last_seq"]
    assert full_scan(db)[0] == [(k, v) for k, v, _ in items]
    assert db.get(items[300][0]) == items[300][1]
    assert db.checksum() == model_checksum(items)
    e.close()


# 6 ------------------------------------------------------------------- refusals

def test_refusals_leave_the_store_untouched(hostile):
    good = hostile[0]
    one = PyBatch().put(b"k", b"v").data()
    # import into a non-empty shard
    e = ra.Engine(nshards=2, **SMALL_ENGINE)
    db = e.open(0)
    assert db.handle_replicate_response(one)
    e.flush()
    used, cs = e.store_usage().used, db.checksum()
    with pytest.raises(RuntimeError, match="pristine"):
        db.import_image(good)
    assert (e.store_usage().used, db.checksum(), db.latest_seq()) == \
        (used, cs, 1)
    assert db.get(b"k") == b"v"
    # a merge operator the engine does not run
    u64 = pyimage.pack(pyimage.unpack(good)[1], 2400, 1)
    with pytest.raises(RuntimeError, match="merge operator"):
        e.open(1).import_image(u64)
    assert e.store_usage().used == used and e.open(1).latest_seq() == 0
    # export with no room for the bytes: the exact size comes back
    want = pyimage.pack([(b"k", b"v", 1)], 1, 0)
    rc, img, info = db.export_image_raw(0)
    assert (rc, img, info.image_bytes) == \
        (ra.ffi.GRA_BUF_TOO_SMALL, None, len(want))
    rc, img, info = db.export_image_raw(len(want) - 1)
    assert (rc, info.image_bytes) == (ra.ffi.GRA_BUF_TOO_SMALL, len(want))
    assert e.store_usage().used == used
    assert db.export_image(cap=0) == want  # the retry
    assert e.store_usage().used == used
    e.close()
    # a store_ring engine keeps no runs
    e = ra.Engine(nshards=1, store_ring=1, **SMALL_ENGINE)
    db = e.open(0)
    with pytest.raises(RuntimeError, match="store_ring"):
        db.import_image(good)
    assert db.latest_seq() == 0
    with pytest.raises(RuntimeError, match="store_ring"):
        db.export_image()
    e.close()
    # a 1 MiB arena and an image of more
    fat = [(b"fat%04d" % i, bytes([i & 0xFF]) * 2048, i + 1)
           for i in range(600)]
    e = ra.Engine(nshards=1, store_bytes=1 << 20, staging_bytes=64 << 20)
    db = e.open(0)
    with pytest.raises(ra.StoreFullError):
        db.import_image(pyimage.pack(fat, 600, 0))
    assert e.store_usage().used == 0 and db.latest_seq() == 0
    assert db.scan_page_raw()[0] == []
    db.import_image(pyimage.pack(fat[:100], 600, 0))  # this much fits
    assert db.latest_seq() == 600
    assert full_scan(db)[0] == [(k, v) for k, v, _ in fat[:100]]
    e.close()


# 7 ------------------------------------------------------------ the hole, closed

def test_follower_bootstraps_past_a_truncated_log(olib, stream):
    reps, universe, _ = stream
    ost = oracle_ffi.Store(olib, 1, merge_op=1)
    lead_e = ra.Engine(nshards=1, merge_op=1, retain_log=1,
                       log_bytes=32 << 10, **SMALL_ENGINE)
    fol_e = ra.Engine(nshards=2, merge_op=1, **SMALL_ENGINE)
    leader, follower = rp.Replicator(lead_e), rp.Replicator(fol_e)
    try:
        ldb = leader.add_db("db", rp.LEADER).db
        for rep in reps:  # ~200 KiB of history through a 32 KiB log
            leader.write("db", rep)
            assert ost.apply(0, rep)
        S = ldb.latest_seq()
        assert S == ost.latest_seq(0) > 3000
        # today's only way: replay from seq 0 — the log no longer has it
        probe = follower.add_db("probe", rp.FOLLOWER).db
        with pytest.raises(RuntimeError, match="truncated"):
            rp.pull_once(ldb, probe)
        assert probe.latest_seq() == 0
        # the image carries the follower past the hole; pulling resumes at S
        fdb = follower.restore_db("db", leader.backup_db("db"), rp.FOLLOWER,
                                  ldb).db
        assert fdb.latest_seq() >= S
        last = S
        for i in range(5):
            b = PyBatch().put(b"after-%d" % i, b"v%d" % i) \
                .merge(universe[10 + i], struct.pack("<Q", 7 + i)) \
                .delete(universe[40 + i])
            last = leader.write("db", b.data())
            assert ost.apply(0, b.data())
        assert last == ost.latest_seq(0) == S + 15
        # the follower's pull request with seq_no = last is the confirmed ack
        assert ldb.wait_ack(last, confirmed=True, timeout_ms=20000)
        follower.change_role("db", rp.FOLLOWER, None)  # stop pulling
        fol_e.flush()
        assert fdb.latest_seq() == last
        keys = universe + [b"after-%d" % i for i in range(5)]
        for k in keys + absent_keys(keys):
            assert fdb.get(k) == ost.get(0, k), k
        assert full_scan(fdb)[0] == ss.expected(ost, 0, sorted(keys), b"",
                                                None)
    finally:
        follower.close()
        leader.close()
        fol_e.close()
        lead_e.close()
