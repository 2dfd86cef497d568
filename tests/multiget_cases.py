"""Case builders and expectations for the gra_multiget suite
(tests/test_multiget_cases_host.py checks them on the CPU,
tests/test_gpu_multiget.py runs them on the device). TEST INFRASTRUCTURE ONLY.

A Case is a list of steps (device batches, leader-side host batches, flushes)
and a list of plans (the query batches, each with the device path it means to
hit). Expected values always come from the oracle store; expected statuses
come from fold_model.Model by the rule in include/rocksplicator_gpu.h: with
floor = max(T, RD), a Merge above the floor is NEEDS_HOST (FOUND with the 8
folded bytes under fold_on_device=1 + u64add); otherwise FOUND iff T is a Put
above RD; otherwise MISS. predict() restates which of the two device paths
gra_multiget takes, so no "fallback" case can be vacuous.
"""
import functools
import random
import struct

import fold_model as fm
import oracle_ffi
import scan_streams as ss
from pywb import PyBatch

FOUND, MISS, NEEDS_HOST = 0, 1, 2  # GRA_GET_* (include/rocksplicator_gpu.h)
TOMB_CAP = 4096                    # tomb_cap in gra_multiget
MAX_WB = 1000                      # records a rep (the engine takes 1024)
BALLAST = b"~ballast"
CF = ss.CF


def cand_cap(nq):
    return 4 * nq + 1024


# ------------------------------------------------------------- fingerprints

def fnv1a32(key):
    """wb::key_fnv_fold from kFnvBasis32: the fingerprint k_kpref stores."""
    h = 2166136261
    for b in key:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def _search_same_length(draws=300000, seed=1):
    rng = random.Random(seed)
    seen, pairs = {}, []
    for _ in range(draws):
        k = rng.randbytes(8)
        h = fnv1a32(k)
        o = seen.setdefault(h, k)
        if o != k:
            pairs.append((o, k))
    return pairs


SAME_LEN_PAIRS = _search_same_length()
DIFF_LEN_PAIRS = [(b"costarring", b"liquid"), (b"altarage", b"zinke")]
WORD_SAME_PAIR = (b"declinate", b"macallums")  # 9 bytes each
SLOT63 = [k for k in (b"wr%04d" % i for i in range(2000))
          if fnv1a32(k) & 63 == 63]
SLOT_LOW = {s: [k for k in (b"lo%04d" % i for i in range(2000))
                if fnv1a32(k) & 63 == s][:3] for s in (0, 1, 2)}


# ------------------------------------------------------------------- cases

def put(k, v, cf=0):
    return ("put", k, v, cf)


def delete(k, cf=0):
    return ("del", k, b"", cf)


def sdel(k, cf=0):
    return ("sdel", k, b"", cf)


def merge(k, v, cf=0):
    return ("merge", k, v, cf)


def rdel(b, e, cf=0):
    return ("rdel", b, e, cf)


def stored(rec):
    """Stored key of a point record."""
    return ss.cfkey(rec[3], rec[1]) if rec[3] else rec[1]


def encode(recs):
    b = PyBatch()
    for op, k, v, cf in recs:
        if op == "put":
            b.cf_put(cf, k, v) if cf else b.put(k, v)
        elif op == "del":
            b.cf_delete(cf, k) if cf else b.delete(k)
        elif op == "sdel":
            b.cf_single_delete(cf, k) if cf else b.single_delete(k)
        elif op == "merge":
            b.cf_merge(cf, k, v) if cf else b.merge(k, v)
        else:
            b.cf_delete_range(cf, k, v) if cf else b.delete_range(k, v)
    return b.data()


class Plan:
    """One query batch. path: "join", "fallback", or "both" = the keys as a
    join batch and the keys plus BALLAST as a fallback batch."""

    def __init__(self, keys, path, stride, shard):
        self.keys, self.path, self.stride, self.shard = \
            list(keys), path, stride, shard


class Case:
    def __init__(self, name, nshards=1, merge_op=0):
        self.name, self.nshards, self.merge_op = name, nshards, merge_op
        self.steps = []   # ("dev"|"host", shard, rep) | ("flush",)
        self.marks = {}   # name -> index into steps
        self.plans = []
        self.claims = {}  # what the builder says the stream holds
        self._models = {}

    def dev(self, recs, shard=0, flush=True):
        """Records for the device path, one rep per MAX_WB, then a flush
        (one flush = one tick = one run of the shard)."""
        for i in range(0, len(recs), MAX_WB):
            self.steps.append(("dev", shard, encode(recs[i:i + MAX_WB])))
        if flush:
            self.flush()

    def host(self, recs, shard=0):
        """Records written on the leader side: a host-origin run."""
        self.steps.append(("host", shard, encode(recs)))

    def flush(self):
        self.steps.append(("flush",))

    def mark(self, name):
        self.marks[name] = len(self.steps)

    def plan(self, keys, path="both", stride=64, shard=0):
        self.plans.append(Plan(keys, path, stride, shard))

    def add_ballast(self):
        """BALLAST Put 4*nq + 1025 times, nq the largest fallback batch of a
        "both" plan: queried once, it alone overflows the candidate cap."""
        self.mark("ballast")
        for s in range(self.nshards):
            nq = max([len(p.keys) + 1 for p in self.plans
                      if p.path == "both" and p.shard == s], default=0)
            if nq:
                self.dev([put(BALLAST, b"ballast-%06d" % i)
                          for i in range(cand_cap(nq) + 1)], shard=s)
        return self

    def models(self, upto=None):
        """-> (per-shard Model of everything, per-shard Model of the device
        runs alone) after steps[:upto]."""
        upto = len(self.steps) if upto is None else upto
        if upto not in self._models:
            allm = [fm.Model() for _ in range(self.nshards)]
            devm = [fm.Model() for _ in range(self.nshards)]
            for st in self.steps[:upto]:
                if st[0] == "flush":
                    continue
                allm[st[1]].apply(st[2])
                if st[0] == "dev":
                    # the device half, with the seqs it has in the shard
                    devm[st[1]].t = allm[st[1]].t - \
                        struct.unpack_from("<I", st[2], 8)[0]
                    devm[st[1]].apply(st[2])
            self._models[upto] = (allm, devm)
        return self._models[upto]

    def oracle(self, olib, upto=None):
        ost = oracle_ffi.Store(olib, self.nshards, merge_op=self.merge_op)
        for st in self.steps[:upto]:
            if st[0] != "flush":
                assert ost.apply(st[1], st[2])
        return ost


def expect(model, ost, shard, keys, stride, fold_u64=False):
    """[(status, vlen, bytes)] as Db.multiget_raw reports them."""
    out = []
    for k in keys:
        s = model.look(k)
        if s["ops"] and not fold_u64:
            out.append((NEEDS_HOST, 0, b""))
        elif s["ops"] or s["base"] is not None:
            v = ost.get(shard, k)
            assert v is not None, k
            out.append((FOUND, len(v), v[:stride]))
        else:
            out.append((MISS, 0, b""))
    return out


def predict(dev_model, keys):
    """The path gra_multiget serves this batch by, restated from its rule:
    cands = stored non-range entries whose key equals a query's, summed over
    the queries; tombs = range deletions in the shard's device runs."""
    cands = sum(len(dev_model.ver.get(k, ())) for k in keys)
    tombs = len(dev_model.tombs)
    return "join" if cands <= cand_cap(len(keys)) and tombs <= TOMB_CAP \
        else "fallback"


def batches(plan):
    """-> [(keys, intended path)] of one plan."""
    if plan.path == "both":
        return [(plan.keys, "join"), (plan.keys + [BALLAST], "fallback")]
    return [(plan.keys, plan.path)]


def check_paths(case, upto=None):
    """Every plan takes the path it names."""
    _, devm = case.models(upto)
    for p in case.plans:
        for keys, path in batches(p):
            assert predict(devm[p.shard], keys) == path, (case.name, path)


# ------------------------------------------------------------- collisions

ROLES = ("both_put", "one_stored", "put_delete", "tomb")


def collision_pairs():
    return SAME_LEN_PAIRS[:4] + DIFF_LEN_PAIRS + [WORD_SAME_PAIR]


@functools.lru_cache(None)
def collisions(rot):
    """Every colliding pair in one of four roles, rotated by `rot` so that
    the four cases give every pair every role. Two flushes."""
    c = Case("collisions-%d" % rot)
    old, new, probes = [], [], []
    roles = {}
    for i, (a, b) in enumerate(collision_pairs()):
        if (i + rot) % 2:
            a, b = b, a
        role = ROLES[(i + rot) % 4]
        roles[(a, b)] = role
        va, vb = b"A-%d-" % i + a, b"B-%d-" % i + b
        if role == "both_put":
            old += [put(a, b"stale"), put(b, b"stale-too")]
            new += [put(b, vb), put(a, va)]
        elif role == "one_stored":
            old += [put(a, b"stale")]
            new += [put(a, va)]
        elif role == "put_delete":
            old += [put(b, vb), put(a, va)]
            new += [delete(b)]
        else:  # a under a newer range tombstone, b outside it
            old += [put(a, va), put(b, vb)]
            new += [rdel(a, a + b"\x00")]
        probes += [a, b]
    c.dev(old)
    c.dev(new)
    c.claims = {"roles": roles}
    c.plan(probes)
    c.plan(probes[::-1])
    return c.add_ballast()


@functools.lru_cache(None)
def slots():
    """Queries that share table slots: the slot-63 keys wrap the linear probe
    to slot 0 and displace the residents of slots 0..2 (qtab_size 64 for at
    most 32 queries); one key 1, 2 and 5 times next to its collision
    partner."""
    c = Case("slots")
    low = [k for s in (0, 1, 2) for k in SLOT_LOW[s]]
    hi_stored, hi_absent = SLOT63[:6], SLOT63[6:10]
    x, p = SAME_LEN_PAIRS[0]
    recs = [put(k, b"v-" + k) for k in low + hi_stored] + \
        [put(x, b"old-x"), put(p, b"partner"), delete(hi_stored[1])]
    c.dev(recs)
    c.dev([put(x, b"the-x"), put(low[0], b"newer")])
    wrap = low + hi_stored + hi_absent
    assert len(wrap) + 1 <= 32
    c.plan(wrap)                      # residents first, then the wrappers
    c.plan(hi_absent + hi_stored + low)   # wrappers first: they take 0..
    c.plan(hi_stored[:5] + [hi_stored[0]] * 3 + low[:3])
    for n in (1, 2, 5):
        c.plan([x] * (n // 2) + [p] + [x] * (n - n // 2))
    c.plan([x] * 5 + [p] * 2 + [b"absent"] * 3)
    c.claims = {"slot63": len(hi_stored) + len(hi_absent), "low": len(low)}
    return c.add_ballast()


# --------------------------------------------------- query-count boundaries

NQ_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


@functools.lru_cache(None)
def query_counts():
    """A 2,000-key shard in two runs (Puts, some Deletes, SingleDeletes,
    Merges and narrow range tombstones); per nq a batch with half of the
    queries absent."""
    rng = random.Random(41)
    c = Case("query-counts")
    keys = [b"k%05d" % i for i in range(2000)]
    pointed = set()
    for half in (keys[:1200], keys[800:]):
        recs = []
        for k in half:
            x = rng.random()
            if x < 0.80:
                recs.append(put(k, rng.randbytes(rng.randrange(0, 41))))
            elif x < 0.90:
                recs.append(delete(k))
            elif x < 0.94:
                recs.append(sdel(k))
            elif x < 0.98:
                recs.append(merge(k, rng.randbytes(5)))
            else:
                i = int(k[1:])
                recs.append(rdel(k, b"k%05d" % (i + 3)))
            if recs[-1][0] != "rdel":
                pointed.add(k)
        c.dev(recs)
    for nq in NQ_SIZES:
        present = rng.sample(sorted(pointed), nq - nq // 2)
        absent = [b"x%05d" % i for i in rng.sample(range(100000), nq // 2)]
        batch = present + absent
        rng.shuffle(batch)
        c.plan(batch)
    return c.add_ballast()


# -------------------------------------------------------------- exact caps

@functools.lru_cache(None)
def cand_caps():
    """Per nq in (1, 3): a key with exactly cand_cap(nq) Put versions and one
    with cand_cap(nq) + 1, over three runs; the batch at the cap is a join
    batch, the one past it a fallback batch."""
    c = Case("cand-caps")
    recs, rng = [], random.Random(43)
    hist = {}
    for nq in (1, 3):
        for tag, n in ((b"at", cand_cap(nq)), (b"over", cand_cap(nq) + 1)):
            k = b"cap-%d-" % nq + tag
            hist[k] = n
            recs += [put(k, b"%s-%05d" % (k, i)) for i in range(n)]
    # interleave the keys, keep each key's order
    order = sorted(range(len(recs)), key=lambda i: (int(recs[i][2][-5:]), i))
    recs = [recs[i] for i in order]
    third = len(recs) // 3
    for part in (recs[:third], recs[third:2 * third], recs[2 * third:]):
        c.dev(part)
    c.claims = {"versions": hist}
    pad = [b"cap-absent-1", b"cap-absent-2"]
    c.plan([b"cap-1-at"], "join")
    c.plan([b"cap-1-over"], "fallback")
    c.plan([b"cap-3-at"] + pad, "join")
    c.plan([b"cap-3-over"] + pad, "fallback")
    c.plan([pad[0], b"cap-3-at", pad[1]], "join")
    c.plan([pad[0], pad[1], b"cap-3-over"], "fallback")
    return c


TOMB_PROBES = [b"tp-%d" % i for i in range(6)] + [b"tp-absent"]


@functools.lru_cache(None)
def tomb_caps(ntombs):
    """ntombs range deletions in the device runs: all but six cover a key
    region nothing probed lies in; the six sit below, between and above the
    probes' Puts in seq. The same probes at every count."""
    c = Case("tomb-caps-%d" % ntombs)
    p = TOMB_PROBES
    one = lambda k: rdel(k, k + b"\x00")
    filler = [rdel(b"t%05d" % i, b"t%05d\x00" % i) for i in range(ntombs - 6)]
    run1 = [one(p[0]), rdel(p[1], p[1] + b"zz")] + filler[:1500] + \
        [put(k, b"v1-" + k) for k in p[:6]] + [one(p[2])] + filler[1500:3000]
    run2 = [put(p[2], b"v2-tp-2"), one(p[4]), one(p[5])] + filler[3000:] + \
        [put(p[5], b"v3-tp-5"), rdel(b"tp-5", b"tp-6")]
    c.dev(run1)
    c.dev(run2)
    c.claims = {"tombs": ntombs,
                "status": [FOUND, FOUND, FOUND, FOUND, MISS, MISS, MISS]}
    c.plan(p, "both" if ntombs <= TOMB_CAP else "fallback")
    return c.add_ballast()


# --------------------------------------------------- range-tombstone bounds

def bounds_table():
    """[(name, begin, end, key, cf, covered)] in user-key space; covered is
    begin <= key < end, written out by hand. Namespaced by entry so that no
    tombstone meets another entry's key; the empty begin ends below every
    namespaced key."""
    rows = [
        ("key==begin", b"b", b"d", b"b", True),
        ("key==end", b"b", b"d", b"d", False),
        ("key=begin+00", b"b", b"d", b"b\x00", True),
        ("key<begin:prefix", b"bb", b"d", b"b", False),
        ("begin<key:prefix", b"b", b"d", b"bzz", True),
        ("key<end:prefix", b"b", b"dd", b"d", True),
        ("end<key:prefix", b"b", b"d", b"dd", False),
        ("key=end-00", b"b", b"c\x00", b"c", True),
        ("key<begin", b"b", b"d", b"a", False),
        ("key>end", b"b", b"d", b"e", False),
        ("begin==end", b"b", b"b", b"b", False),
        ("begin>end", b"d", b"b", b"c", False),
        ("begin>end:key==begin", b"d", b"b", b"d", False),
    ]
    out = []
    for cf in (0, CF):
        for i, (name, b, e, k, cov) in enumerate(rows):
            ns = b"E%02d:" % i
            out.append((name, ns + b, ns + e, ns + k, cf, cov))
        out.append(("begin=empty", b"", b"\x00\x01", b"\x00", cf, True))
        out.append(("key=begin=empty", b"", b"\x00\x01", b"", cf, True))
        out.append(("begin=empty:key==end", b"", b"\x00\x01", b"\x00\x01",
                    cf, False))
    return out


@functools.lru_cache(None)
def bounds(order):
    """The bounds table with every tombstone older ("older") or newer
    ("newer") than its key's Put, in two runs."""
    c = Case("bounds-" + order)
    tombs, puts, probes, want = [], [], [], []
    seen = set()
    for name, b, e, k, cf, cov in bounds_table():
        if (b, e, cf) not in seen:
            seen.add((b, e, cf))
            tombs.append(rdel(b, e, cf))
        r = put(k, b"val:" + k, cf)
        puts.append(r)
        probes.append(stored(r))
        want.append(MISS if cov and order == "newer" else FOUND)
    first, second = (tombs, puts) if order == "older" else (puts, tombs)
    c.dev(first[:len(first) // 2])
    c.dev(first[len(first) // 2:] + second)
    c.claims = {"status": want}
    c.plan(probes)
    return c.add_ballast()


# ----------------------------------------------- newest decides, across runs

ENDINGS = {
    "put": ["put"],
    "delete": ["put", "del"],
    "sdel": ["put", "sdel"],
    "put_after_delete": ["put", "del", "put"],
    "delete_after_put": ["del", "put", "del"],
}
RUN_LEN = 600
POSITIONS = (0, 255, 256, RUN_LEN - 1)


@functools.lru_cache(None)
def newest():
    """Four runs of RUN_LEN entries. Per ending and per run r, a key whose
    history ends in run r (older versions in earlier runs, or earlier in run
    0): the winner lives in the newest, a middle or the oldest run. Per run
    and position in POSITIONS a key whose newest Put is that entry of the run
    (thread 255 and thread 0's second turn in k_multiget's 256-wide stride),
    with an older version in the run before."""
    rng = random.Random(47)
    c = Case("newest")
    runs = [dict() for _ in range(4)]  # position -> record
    free = [[i for i in range(RUN_LEN) if i not in POSITIONS]
            for _ in range(4)]
    probes, want, where = [], [], {}

    def mk(op, k, tag):
        return put(k, tag + b"=" + k) if op == "put" else \
            delete(k) if op == "del" else sdel(k)

    for r in range(4):
        for pos in POSITIONS:
            k = b"pos-%d-%03d" % (r, pos)
            runs[r][pos] = put(k, b"winner=" + k)
            if r:
                runs[r - 1][free[r - 1].pop(rng.randrange(len(free[r - 1])))] \
                    = put(k, b"loser=" + k)
            probes.append(k)
            want.append(FOUND)
            where[k] = (r, pos)
        for name, ops in ENDINGS.items():
            k = b"end-%d-" % r + name.encode()
            # the last op in run r, the ones before it in runs <= r, in order
            at = sorted(rng.randrange(0, r + 1) for _ in ops[:-1]) + [r]
            slots_ = []
            for run in sorted(set(at)):
                n = at.count(run)
                take = sorted(free[run].pop(rng.randrange(len(free[run])))
                              for _ in range(n))
                slots_ += [(run, t) for t in take]
            for j, (op, (run, t)) in enumerate(zip(ops, slots_)):
                runs[run][t] = mk(op, k, b"%d" % j)
            probes.append(k)
            want.append(FOUND if ops[-1] == "put" else MISS)
            where[k] = slots_[-1]
    fill = 0
    for r in range(4):
        recs = []
        for i in range(RUN_LEN):
            if i not in runs[r]:
                runs[r][i] = put(b"fill%05d" % fill, b"f")
                fill += 1
            recs.append(runs[r][i])
        c.dev(recs)
    c.claims = {"status": want, "where": where}
    c.plan(probes + [b"fill00007", b"end-absent"])
    return c.add_ballast()


# --------------------------------------------------- key and value lengths

KEY_LENS = (0, 1, 3, 4, 5, 8, 16, 17, 255, 256, 1000)
VAL_LENS = (0, 1, 7, 8, 9, 255, 256, 257, 4096)
STRIDES = (0, 1, 8, 256, 257, 4096)


@functools.lru_cache(None)
def lengths():
    """Per key length up to nine keys, one per value length (the empty key
    has one value), each over an older version of another length; every
    stride asks for all of them."""
    rng = random.Random(53)
    c = Case("lengths")
    old, new, probes, vlens = [], [], [], {}
    for kl in KEY_LENS:
        stem = rng.randbytes(kl)
        for j, vl in enumerate(VAL_LENS if kl else VAL_LENS[5:6]):
            k = stem[:-1] + bytes([(stem[-1] + j) & 0xFF]) if kl else b""
            old.append(put(k, rng.randbytes(VAL_LENS[(j + 4) % 9])))
            new.append(put(k, rng.randbytes(vl)))
            probes.append(k)
            vlens[k] = vl
    assert len(set(probes)) == len(probes)
    c.dev(old)
    c.dev(new)
    c.claims = {"vlens": vlens}
    for stride in STRIDES:
        c.plan(probes + [b"no-such-length"], stride=stride)
    return c.add_ballast()


# ---------------------------------------------------------------- long runs

def long_key(i):
    return b"%06x" % (i * 2654435761 & 0xFFFFFF) + b"%x" % i


@functools.lru_cache(None)
def long_run(boundary):
    """One run of boundary + 1 + 300 entries: distinct small keys, 4-byte
    values, one flush. Probes: the first and last entries, the three around
    the boundary (where the clamped grid of k_kpref — 65,536 threads — or of
    k_mg_scan — 262,144 — takes its second turn), 200 seeded others and a
    few absent keys."""
    n = boundary + 1 + 300
    c = Case("long-run-%d" % boundary)
    c.dev([put(long_key(i), struct.pack("<I", i)) for i in range(n)])
    rng = random.Random(boundary)
    idx = [0, n - 1, boundary - 2, boundary - 1, boundary] + \
        rng.sample(range(n), 200)
    if boundary > 65536:
        idx += [65534, 65535, 65536]
    probes = [long_key(i) for i in idx] + \
        [long_key(n + i) for i in range(5)]
    c.claims = {"entries": n, "idx": idx}
    c.plan(probes, stride=8)
    return c.add_ballast()


# ------------------------------------------------------------ index lifetime

def plain_stream(seed, n_records, n_batches):
    """Puts, Deletes, SingleDeletes and range deletions (no Merge, so that
    compaction changes no raw answer) over the scan tests' key pool, a
    quarter of them in column family CF. -> [records per batch]"""
    rng = random.Random(seed)
    pool = ss.key_pool(rng)
    out = []
    for _ in range(n_batches):
        recs = []
        for _ in range(n_records // n_batches):
            cf = CF if rng.random() < 0.25 else 0
            k = rng.choice(pool)
            x = rng.random()
            if x < 0.04:
                i = rng.randrange(len(pool))
                recs.append(rdel(pool[i], pool[min(len(pool) - 1,
                                                   i + rng.randrange(0, 4))],
                                 cf))
            elif x < 0.70:
                recs.append(put(k, rng.randbytes(rng.randrange(0, 41)), cf))
            elif x < 0.90:
                recs.append(delete(k, cf))
            else:
                recs.append(sdel(k, cf))
        out.append(recs)
    return out


@functools.lru_cache(None)
def lifetime():
    """Two runs, a mark, two more runs; the probes are every stored key and
    some absent ones."""
    c = Case("lifetime")
    bs = plain_stream(61, 1200, 30)
    for i in range(0, 20, 10):
        c.dev([r for b in bs[i:i + 10] for r in b])
    c.mark("first")
    for i in range(20, 30, 5):
        c.dev([r for b in bs[i:i + 5] for r in b])
    universe = c.models()[0][0].keys()
    c.plan(universe + [b"no-such-key-%02d" % i for i in range(20)] +
           [ss.cfkey(CF, b"nokey%d" % i) for i in range(5)])
    return c.add_ballast()


# ------------------------------------------------------- mixed shard matrix

HALVES = ("nothing", "put", "delete", "merge", "tomb")


def _half(kind, k, tag):
    if kind == "put":
        return [put(k, struct.pack("<Q", 1000 + len(tag)))]
    if kind == "delete":
        return [delete(k)]
    if kind == "merge":
        return [merge(k, struct.pack("<Q", 7))]
    if kind == "tomb":
        return [rdel(k, k + b"\x00")]
    return []


@functools.lru_cache(None)
def mixed():
    """Every (device half, host half) in HALVES x HALVES, once with the host
    half newer and once with the device half newer: device run, leader
    batch, device run. u64add, so that fold_on_device has something to be
    switched off for."""
    c = Case("mixed", merge_op=1)
    d_old, h_mid, d_new, probes = [], [], [], []
    combo = {}
    for d in HALVES:
        for h in HALVES:
            for newer in ("host", "dev"):
                k = b"mx-%s-%s-%s" % (d.encode(), h.encode(), newer.encode())
                (d_old if newer == "host" else d_new).extend(
                    _half(d, k, b"dev"))
                h_mid.extend(_half(h, k, b"host"))
                probes.append(k)
                combo[k] = (d, h, newer)
    c.dev(d_old)
    c.host(h_mid)
    c.dev(d_new)
    c.claims = {"combo": combo}
    c.plan(probes)
    return c.add_ballast()


def mixed_deviants(case):
    """The one shape that may read NEEDS_HOST instead of the exact status:
    the device half alone looks live-merge while the union does not (the
    host half holds a newer terminator or tombstone)."""
    allm, devm = case.models()
    return [k for k in case.plans[0].keys
            if devm[0].look(k)["ops"] and not allm[0].look(k)["ops"]]


# ----------------------------------------------------------- shard isolation

@functools.lru_cache(None)
def shards():
    """Four shards holding the same keys with their own values, Deletes and
    range tombstones, and one key each that only that shard has."""
    c = Case("shards", nshards=4)
    keys = [b"sh%03d" % i for i in range(40)]
    for s in range(4):
        recs = [put(k, b"shard%d:" % s + k) for k in keys]
        recs += [delete(k) for i, k in enumerate(keys) if i % 4 == s]
        recs += [rdel(keys[20 + 4 * s], keys[23 + 4 * s]),
                 put(b"only-in-%d" % s, b"mine")]
        c.dev(recs[:30], shard=s, flush=False)
        c.dev(recs[30:], shard=s, flush=False)
    c.flush()
    for s in range(4):
        c.plan(keys + [b"only-in-%d" % t for t in range(4)], shard=s)
    return c.add_ballast()


def small_cases():
    """Every case that one engine plays whole and whose plans then run as
    they are."""
    return [collisions(0), collisions(1), collisions(2), collisions(3),
            slots(), query_counts(), cand_caps(), tomb_caps(TOMB_CAP),
            tomb_caps(TOMB_CAP + 1), bounds("older"), bounds("newer"),
            newest(), lengths(), shards()]


def all_cases():
    return small_cases() + [lifetime(), mixed(), long_run(65536),
                            long_run(262144)]
