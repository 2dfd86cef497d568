"""CPU checks of tests/multiget_cases.py: the collision sets collide, and for
every stream tests/test_gpu_multiget.py plays the model and the oracle agree
on each probed key, every shape the GPU test claims to contain occurs, and
every query batch takes the device path it names. A builder mistake is caught
here, without a GPU."""
import collections

import pytest

import multiget_cases as mc
import oracle_ffi


@pytest.fixture(scope="module")
def olib():
    return oracle_ffi.load()


def statuses(case, olib, plan=0):
    p = case.plans[plan]
    ost = case.oracle(olib)
    return [st for st, _, _ in mc.expect(case.models()[0][p.shard], ost,
                                         p.shard, p.keys, p.stride)]


# ------------------------------------------------------------- fingerprints

def test_fnv1a32_vectors():
    # the published FNV-1a 32-bit test vectors
    assert mc.fnv1a32(b"") == 0x811C9DC5
    assert mc.fnv1a32(b"a") == 0xE40C292C
    assert mc.fnv1a32(b"foobar") == 0xBF9CF968


def test_collision_sets_collide():
    assert len(mc.SAME_LEN_PAIRS) >= 4
    for a, b in mc.SAME_LEN_PAIRS + [mc.WORD_SAME_PAIR]:
        assert a != b and len(a) == len(b)
        assert mc.fnv1a32(a) == mc.fnv1a32(b)
    for a, b in mc.DIFF_LEN_PAIRS:
        assert a != b and len(a) != len(b)
        assert mc.fnv1a32(a) == mc.fnv1a32(b)
    assert len(mc.collision_pairs()) == 7
    assert len(set(k for p in mc.collision_pairs() for k in p)) == 14


def test_slot_sets():
    assert len(mc.SLOT63) >= 10
    assert all(mc.fnv1a32(k) & 63 == 63 for k in mc.SLOT63)
    for s in (0, 1, 2):
        assert len(mc.SLOT_LOW[s]) == 3
        assert all(mc.fnv1a32(k) & 63 == s for k in mc.SLOT_LOW[s])


# ------------------------------------------------------------ every stream

@pytest.mark.parametrize("case", mc.all_cases(), ids=lambda c: c.name)
def test_model_oracle_and_paths(olib, case):
    ost = case.oracle(olib)
    allm, _ = case.models()
    for p in case.plans:
        assert p.keys
        for k in set(p.keys) | {mc.BALLAST}:
            assert allm[p.shard].value(k, case.merge_op) == \
                ost.get(p.shard, k), (case.name, k)
        assert len(mc.expect(allm[p.shard], ost, p.shard, p.keys,
                             p.stride)) == len(p.keys)
        if p.path == "both":  # the ballast is alive, its newest value on top
            n = len(allm[p.shard].ver[mc.BALLAST])
            assert n >= mc.cand_cap(len(p.keys) + 1) + 1
            assert ost.get(p.shard, mc.BALLAST) == b"ballast-%06d" % (n - 1)
    mc.check_paths(case)
    assert {path for p in case.plans for _, path in mc.batches(p)} >= \
        ({"fallback"} if case.name == "tomb-caps-4097"
         else {"join", "fallback"})


# ------------------------------------------------------ the claimed shapes

@pytest.mark.parametrize("rot", range(4))
def test_collision_roles(olib, rot):
    case = mc.collisions(rot)
    got = dict(zip(case.plans[0].keys, statuses(case, olib)))
    roles = case.claims["roles"]
    assert collections.Counter(roles.values()) == \
        {r: (2 if (mc.ROLES.index(r) - rot) % 4 < 3 else 1)
         for r in mc.ROLES}
    want = {"both_put": (mc.FOUND, mc.FOUND), "one_stored": (mc.FOUND, mc.MISS),
            "put_delete": (mc.FOUND, mc.MISS), "tomb": (mc.MISS, mc.FOUND)}
    for (a, b), role in roles.items():
        assert (got[a], got[b]) == want[role], (a, b, role)
    dev = case.models()[1][0]
    for (a, b), role in roles.items():  # what the device runs hold
        assert bool(dev.ver.get(b)) == (role != "one_stored")
        assert dev.ver[a]


def test_every_pair_takes_every_role():
    seen = collections.defaultdict(set)
    for rot in range(4):
        for (a, b), role in mc.collisions(rot).claims["roles"].items():
            seen[frozenset((a, b))].add(role)
    assert len(seen) == 7
    assert all(v == set(mc.ROLES) for v in seen.values())


def test_slot_batches():
    case = mc.slots()
    assert case.claims["slot63"] >= 5 and case.claims["low"] == 9
    wrap = case.plans[0].keys
    assert len(wrap) + 1 <= 32  # qtab_size 64, with the ballast query too
    # the host-built table of this batch: a slot-63 key lands in slot 0..,
    # and a resident of slots 0..2 is then pushed along
    for keys in (case.plans[0].keys, case.plans[1].keys):
        tab, moved = {}, 0
        for k in keys:
            s = home = mc.fnv1a32(k) & 63
            wrapped = False
            while s in tab:
                wrapped |= s == 63
                s = (s + 1) & 63
            tab[s] = k
            moved += (home == 63 and wrapped) or (home < 3 and s != home)
        assert moved >= 8, moved
    x, p = mc.SAME_LEN_PAIRS[0]
    counts = sorted(pl.keys.count(x) for pl in case.plans[3:6])
    assert counts == [1, 2, 5]
    assert all(p in pl.keys for pl in case.plans[3:])


def test_query_count_batches(olib):
    case = mc.query_counts()
    assert tuple(len(p.keys) for p in case.plans) == mc.NQ_SIZES
    model = case.models()[0][0]
    assert 1900 <= len(model.keys()) <= 2000
    seen = collections.Counter()
    for i, p in enumerate(case.plans):
        absent = sum(k not in model.ver for k in p.keys)
        assert absent == len(p.keys) // 2
        seen.update(statuses(case, olib, i))
    assert seen[mc.FOUND] > 1000 and seen[mc.MISS] > 1000
    assert seen[mc.NEEDS_HOST] > 20


def test_cap_cases(olib):
    case = mc.cand_caps()
    assert case.claims["versions"] == {
        b"cap-1-at": 1028, b"cap-1-over": 1029,
        b"cap-3-at": 1036, b"cap-3-over": 1037}
    dev = case.models()[1][0]
    ost = case.oracle(olib)
    for k, n in case.claims["versions"].items():
        assert len(dev.ver[k]) == n
        assert ost.get(0, k) == b"%s-%05d" % (k, n - 1)  # the newest wins
    assert sum(st[0] == "flush" for st in case.steps) == 3
    for n in (mc.TOMB_CAP, mc.TOMB_CAP + 1):
        case = mc.tomb_caps(n)
        dev = case.models()[1][0]
        assert len(dev.tombs) == n == case.claims["tombs"]
        assert statuses(case, olib) == case.claims["status"]
        covering = [t for t in dev.tombs
                    if any(t[1] <= k < t[2] for k in mc.TOMB_PROBES)]
        assert len(covering) == 6
        assert mc.tomb_caps(n).plans[0].keys == mc.TOMB_PROBES


@pytest.mark.parametrize("order", ["older", "newer"])
def test_bounds_table(olib, order):
    table = mc.bounds_table()
    assert len(table) == 32
    for name, b, e, k, cf, cov in table:
        assert cov == (b <= k < e), name
    names = {n for n, *_ in table}
    assert len(names) == 16
    by = {n: (b, e, k) for n, b, e, k, cf, _ in table if cf == 0}
    b, e, k = by["key<begin:prefix"]
    assert b.startswith(k) and b != k
    b, e, k = by["begin<key:prefix"]
    assert k.startswith(b) and b != k
    b, e, k = by["key<end:prefix"]
    assert e.startswith(k) and e != k
    b, e, k = by["end<key:prefix"]
    assert k.startswith(e) and e != k
    assert by["key=begin+00"][2] == by["key=begin+00"][0] + b"\x00"
    assert by["key=begin=empty"] == (b"", b"\x00\x01", b"")
    case = mc.bounds(order)
    got = statuses(case, olib)
    assert got == case.claims["status"]
    assert got.count(mc.MISS) == (14 if order == "newer" else 0)
    # in stored-key space too: every probe is covered by exactly the
    # tombstone of its own row, or by none
    dev = case.models()[1][0]
    for (name, b, e, k, cf, cov), probe in zip(table, case.plans[0].keys):
        hits = [t for t in dev.tombs if t[1] <= probe < t[2]]
        assert len(hits) == (1 if cov else 0), name


def test_newest_shapes(olib):
    case = mc.newest()
    assert statuses(case, olib)[:-2] == case.claims["status"]
    assert sum(st[0] == "flush" for st in case.steps) == 4 + 1  # + ballast
    dev = case.models()[1][0]
    where = case.claims["where"]
    # the claimed entry is the key's newest version: seq = run * RUN_LEN + pos
    for k, (run, pos) in where.items():
        assert dev.ver[k][-1][0] == run * mc.RUN_LEN + pos + 1, k
    for r in range(4):
        for pos in mc.POSITIONS:
            assert where[b"pos-%d-%03d" % (r, pos)] == (r, pos)
        for name, ops in mc.ENDINGS.items():
            k = b"end-%d-" % r + name.encode()
            assert where[k][0] == r
            kinds = [{mc.fm.PUT: "put", mc.fm.DELETE: "del",
                      mc.fm.SINGLE_DELETE: "sdel"}[t] for _, t, _ in dev.ver[k]]
            assert kinds == ops
    spread = [k for k in where if k.startswith(b"end-3") and
              len({(t - 1) // mc.RUN_LEN for t, _, _ in dev.ver[k]}) > 1]
    assert len(spread) >= 2  # histories that cross runs


def test_length_shapes(olib):
    case = mc.lengths()
    vlens = case.claims["vlens"]
    assert sorted({len(k) for k in vlens}) == list(mc.KEY_LENS)
    assert sorted(set(vlens.values())) == list(mc.VAL_LENS)
    assert tuple(p.stride for p in case.plans) == mc.STRIDES
    ost = case.oracle(olib)
    for k, vl in vlens.items():
        assert len(ost.get(0, k)) == vl
    for i, p in enumerate(case.plans):
        want = mc.expect(case.models()[0][0], ost, 0, p.keys, p.stride)
        for k, (st, vlen, val) in zip(p.keys[:-1], want[:-1]):
            assert (st, vlen, len(val)) == \
                (mc.FOUND, vlens[k], min(vlens[k], p.stride))
        assert want[-1] == (mc.MISS, 0, b"")
    truncated = sum(vl > p.stride for p in case.plans for vl in vlens.values())
    assert truncated > 150


@pytest.mark.parametrize("boundary", [65536, 262144])
def test_long_run_shapes(boundary):
    case = mc.long_run(boundary)
    n = case.claims["entries"]
    assert n == boundary + 301
    idx = case.claims["idx"]
    assert idx[:5] == [0, n - 1, boundary - 2, boundary - 1, boundary]
    dev = case.models(case.marks["ballast"])[1][0]
    assert len(dev.ver) == n and dev.t == n  # distinct keys, one version
    flushes = [i for i, st in enumerate(case.steps) if st[0] == "flush"]
    assert flushes[0] == case.marks["ballast"] - 1  # one flush: one run
    for i, k in zip(idx, case.plans[0].keys):
        assert dev.ver[k][0][0] == i + 1  # entry i of the run
    assert max(len(k) for k in dev.ver) <= 11


def test_lifetime_shapes(olib):
    case = mc.lifetime()
    first = case.marks["first"]
    flushes = [i for i, st in enumerate(case.steps) if st[0] == "flush"]
    assert sum(i < first for i in flushes) == 2
    assert sum(first < i < case.marks["ballast"] for i in flushes) == 2
    early, late = case.models(first)[0][0], case.models()[0][0]
    assert not any(v[1] == mc.fm.MERGE for vs in late.ver.values()
                   for v in vs)
    p = case.plans[0]
    a = mc.expect(early, case.oracle(olib, first), 0, p.keys, p.stride)
    b = mc.expect(late, case.oracle(olib), 0, p.keys, p.stride)
    assert sum(x != y for x, y in zip(a, b)) > 20  # the new runs matter
    seen = collections.Counter(st for st, _, _ in b)
    assert seen[mc.FOUND] > 40 and seen[mc.MISS] > 40
    assert late.tombs and any(k[:4] == mc.ss.cfkey(mc.CF, b"") for k in p.keys)


def test_mixed_matrix(olib):
    case = mc.mixed()
    combo = case.claims["combo"]
    assert len(combo) == 50
    assert collections.Counter(combo.values()) == \
        {(d, h, n): 1 for d in mc.HALVES for h in mc.HALVES
         for n in ("host", "dev")}
    allm, devm = case.models()
    for k, (d, h, newer) in combo.items():
        dv = [(t, typ) for t, typ, _ in devm[0].ver.get(k, [])] + \
            [(t, mc.fm.RANGE_DELETE) for t, b, e in devm[0].tombs if b == k]
        al = [(t, typ) for t, typ, _ in allm[0].ver.get(k, [])] + \
            [(t, mc.fm.RANGE_DELETE) for t, b, e in allm[0].tombs if b == k]
        hv = sorted(set(al) - set(dv))
        assert len(dv) == (d != "nothing") and len(hv) == (h != "nothing")
        if dv and hv:
            assert (hv[0][0] > dv[0][0]) == (newer == "host"), k
    dev = mc.mixed_deviants(case)
    assert sorted(combo[k] for k in dev) == [
        ("merge", "delete", "host"), ("merge", "put", "host"),
        ("merge", "tomb", "host")]
    seen = collections.Counter(statuses(case, olib))
    assert min(seen[mc.FOUND], seen[mc.MISS], seen[mc.NEEDS_HOST]) >= 8


def test_shard_shapes(olib):
    case = mc.shards()
    ost = case.oracle(olib)
    keys = case.plans[0].keys
    assert all(p.keys == keys for p in case.plans)
    per = [[ost.get(s, k) for k in keys] for s in range(4)]
    assert len({tuple(v) for v in per}) == 4
    for s in range(4):
        assert ost.get(s, b"only-in-%d" % s) == b"mine"
        assert all(ost.get(t, b"only-in-%d" % s) is None
                   for t in range(4) if t != s)
        assert 12 <= sum(v is None for v in per[s]) <= 16
        assert len(case.models()[1][s].tombs) == 1
