"""gra_multiget, element by element, on both device paths: the hash join
(k_kpref, k_mg_scan, k_mg_resolve1/2, k_mg_tombs, k_mg_emit) and the per-query
scan kernel it falls back to (k_multiget), plus the host-side merge of a mixed
shard. The cases, their expectations and the predictor of the path a batch
takes are in tests/multiget_cases.py; tests/test_multiget_cases_host.py checks
them on the CPU. Values are the oracle's, statuses the model's, every
comparison is exact, and every device assertion goes through
Db.multiget_raw: Db.multiget answers NEEDS_HOST with get() and would hide a
wrong verdict. Each case also checks Db.multiget against the oracle.

A "both" plan runs twice: as it is (a join batch) and with the ballast key
appended, whose 4*nq + 1025 Put versions overflow the candidate cap and send
the whole batch to k_multiget. The two answer lists must be identical to each
other and to the expectation.

Out of scope: more than 65,535 runs in one shard (the only other way into the
fallback; it costs 65,536 flushes), and seqs at or above 2^56 (term_pack
shifts seq left by 8; RocksDB seqs are 56-bit and the engine numbers records
itself)."""
import pytest

import multiget_cases as mc
import oracle_ffi
import rocksplicator_amd as ra
from rocksplicator_amd.ffi import (GRA_GET_FOUND, GRA_GET_MISS,
                                   GRA_GET_NEEDS_HOST)

pytestmark = pytest.mark.gpu

ENGINE = dict(store_bytes=256 << 20, staging_bytes=64 << 20)


@pytest.fixture(scope="module")
def olib():
    return oracle_ffi.load()


def test_status_codes():
    assert (mc.FOUND, mc.MISS, mc.NEEDS_HOST) == \
        (GRA_GET_FOUND, GRA_GET_MISS, GRA_GET_NEEDS_HOST)


class Rig:
    """One engine and one oracle store fed the same steps."""

    def __init__(self, olib, case, fold=0):
        self.case = case
        self.e = ra.Engine(nshards=case.nshards, merge_op=case.merge_op,
                           fold_on_device=fold, **ENGINE)
        self.dbs = [self.e.open(s) for s in range(case.nshards)]
        self.ost = oracle_ffi.Store(olib, case.nshards,
                                    merge_op=case.merge_op)
        self.at = 0

    def play(self, upto=None):
        upto = len(self.case.steps) if upto is None else upto
        for st in self.case.steps[self.at:upto]:
            if st[0] == "flush":
                self.e.flush()
            elif st[0] == "dev":
                assert self.dbs[st[1]].handle_replicate_response(st[2])
                assert self.ost.apply(st[1], st[2])
            else:
                self.dbs[st[1]].write_leader(st[2])
                assert self.ost.apply(st[1], st[2])
        self.at = upto
        for s, db in enumerate(self.dbs):
            assert db.latest_seq() == self.ost.latest_seq(s)
        return self

    def want(self, plan, keys):
        return mc.expect(self.case.models(self.at)[0][plan.shard], self.ost,
                         plan.shard, keys, plan.stride)

    def ask(self, plan, keys, path, may_decline=()):
        """One raw batch on the path it names -> the answers, checked."""
        dev = self.case.models(self.at)[1][plan.shard]
        assert mc.predict(dev, keys) == path, (self.case.name, path)
        got = self.dbs[plan.shard].multiget_raw(keys, plan.stride)
        want = self.want(plan, keys)
        assert len(got) == len(keys)
        for k, g, w in zip(keys, got, want):
            if k in may_decline and g[0] == GRA_GET_NEEDS_HOST:
                continue
            assert g == w, (self.case.name, path, plan.stride, k)
        return got

    def run(self, plan, may_decline=()):
        answers = [self.ask(plan, keys, path, may_decline)
                   for keys, path in mc.batches(plan)]
        if plan.path == "both":  # the fallback batch ends in the ballast
            assert answers[1][:-1] == answers[0], self.case.name
        db = self.dbs[plan.shard]
        assert db.multiget(plan.keys) == \
            [self.ost.get(plan.shard, k) for k in plan.keys]

    def close(self):
        self.e.close()


def run_whole(olib, case, fold=0):
    mc.check_paths(case)
    rig = Rig(olib, case, fold).play()
    for plan in case.plans:
        rig.run(plan)
    rig.close()


# ------------------------------------------------------------- collisions

@pytest.mark.parametrize("rot", range(4))
def test_fingerprint_collisions(olib, rot):
    """Colliding pairs of equal and of different length: both stored, one
    stored and the other queried, Put beside Delete, one under a range
    tombstone. Only the memcmp tells them apart."""
    run_whole(olib, mc.collisions(rot))


def test_shared_slots_and_duplicates(olib):
    """The probe wraps from slot 63 to slot 0 and displaces residents; one
    key 1, 2 and 5 times in a batch, each copy with its own row."""
    case = mc.slots()
    run_whole(olib, case)


def test_query_count_boundaries(olib):
    """nq on both sides of the qtab doublings and of the 256-thread blocks
    of k_mg_tombs and the resolve kernels."""
    run_whole(olib, mc.query_counts())


# -------------------------------------------------------------- exact caps

def test_candidate_cap_exact(olib):
    """ncand == cand_cap is a join batch, cand_cap + 1 a fallback batch; the
    newest of the 1028..1037 versions wins both times."""
    run_whole(olib, mc.cand_caps())


@pytest.mark.parametrize("ntombs", [mc.TOMB_CAP, mc.TOMB_CAP + 1])
def test_tombstone_cap_exact(olib, ntombs):
    run_whole(olib, mc.tomb_caps(ntombs))


# --------------------------------------------------- range-tombstone bounds

@pytest.mark.parametrize("order", ["older", "newer"])
def test_range_tombstone_bounds(olib, order):
    """begin <= key < end at every prefix relation of key and bounds, in the
    default column family and in CF, by k_mg_tombs (join) and by k_multiget
    (fallback); a failure names the path."""
    case = mc.bounds(order)
    mc.check_paths(case)
    rig = Rig(olib, case).play()
    plan = case.plans[0]
    for keys, path in mc.batches(plan):
        got = rig.ask(plan, keys, path)
        assert [st for st, _, _ in got[:len(plan.keys)]] == \
            case.claims["status"], path
    rig.run(plan)
    rig.close()


# ----------------------------------------------- newest decides, across runs

def test_newest_decides_across_runs(olib):
    """Histories ending in Put, Delete, SingleDelete, Put-after-Delete and
    Delete-after-Put with the winner in each of four runs, and winners at
    entries 0, 255, 256 and n-1 of each run."""
    run_whole(olib, mc.newest())


# --------------------------------------------------- key and value lengths

def test_value_stride_table(olib):
    """FOUND, vlen the true length and the first min(vlen, stride) bytes,
    for every key length, value length and stride, on both paths."""
    case = mc.lengths()
    mc.check_paths(case)
    rig = Rig(olib, case).play()
    for plan in case.plans:
        for keys, path in mc.batches(plan):
            got = rig.ask(plan, keys, path)
            for k, (st, vlen, val) in zip(plan.keys[:-1], got):
                assert (st, vlen, len(val)) == \
                    (GRA_GET_FOUND, case.claims["vlens"][k],
                     min(vlen, plan.stride)), (path, plan.stride, k)
        rig.run(plan)
    rig.close()


# ---------------------------------------------------------------- long runs

@pytest.mark.parametrize("boundary", [65536, 262144])
def test_long_run(olib, boundary):
    """One run longer than the clamped grid of k_kpref (256 blocks: 65,536
    entries) resp. k_mg_scan (1024 blocks: 262,144 entries); the first
    multiget on it builds the index. One tick holds the run under these
    engine options."""
    case = mc.long_run(boundary)
    mc.check_paths(case)
    rig = Rig(olib, case)
    ticks = rig.e.stats().ticks
    rig.play(case.marks["ballast"])
    assert rig.e.stats().ticks == ticks + 1  # one group, hence one run
    plan = case.plans[0]
    first = rig.ask(plan, plan.keys, "join")
    assert [st for st, _, _ in first] == \
        [GRA_GET_FOUND] * (len(plan.keys) - 5) + [GRA_GET_MISS] * 5
    rig.play()
    rig.run(plan)
    rig.close()


# ------------------------------------------------------------ index lifetime

def test_index_lifetime(olib):
    """The lazy index across calls: new runs beside indexed ones, then the
    same shard compacted, reclaimed, and imported into another engine."""
    case = mc.lifetime()
    plan = case.plans[0]
    rig = Rig(olib, case).play(case.marks["first"])
    rig.ask(plan, plan.keys, "join")
    rig.play()  # two more runs, and the ballast run
    mc.check_paths(case)
    rig.run(plan)
    want = rig.want(plan, plan.keys)
    db = rig.dbs[0]
    assert db.compact().status == ra.GRA_COMPACT_DONE
    assert db.compact().status == ra.GRA_COMPACT_NOTHING
    assert db.multiget_raw(plan.keys, plan.stride) == want
    rig.e.reclaim()
    assert db.multiget_raw(plan.keys, plan.stride) == want
    image = db.export_image()
    assert db.multiget_raw(plan.keys, plan.stride) == want
    e2 = ra.Engine(nshards=1, merge_op=case.merge_op, **ENGINE)
    db2 = e2.open(0)
    db2.import_image(image)
    assert db2.multiget_raw(plan.keys, plan.stride) == want
    assert db2.multiget(plan.keys) == [rig.ost.get(0, k) for k in plan.keys]
    e2.close()
    rig.close()


def test_first_call_is_a_fallback(olib):
    """A fresh engine whose first multiget goes straight to k_multiget: the
    index is built by a call that the join does not serve."""
    case = mc.collisions(0)
    rig = Rig(olib, case).play()
    plan = case.plans[0]
    fb = rig.ask(plan, plan.keys + [mc.BALLAST], "fallback")
    assert rig.ask(plan, plan.keys, "join") == fb[:-1]
    rig.close()


# ------------------------------------------------------- mixed shard matrix

@pytest.mark.parametrize("fold", [0, 1])
def test_mixed_shard_matrix(olib, fold):
    """Device half x host half x which is newer. The statuses are the
    model's over the union; only the keys mixed_deviants names may read
    NEEDS_HOST instead. fold_on_device changes nothing on a mixed shard."""
    case = mc.mixed()
    mc.check_paths(case)
    deviants = mc.mixed_deviants(case)
    assert len(deviants) == 3
    rig = Rig(olib, case, fold).play()
    rig.run(case.plans[0], may_decline=set(deviants))
    rig.close()


# ----------------------------------------------------------- shard isolation

def test_shard_isolation(olib):
    """The same keys in four shards: each shard's multiget sees its own
    values and tombstones only."""
    run_whole(olib, mc.shards())
