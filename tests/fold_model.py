"""A plain Python model of one shard, for tests/test_gpu_fold.py: it replays
WriteBatch reps record by record and answers, per stored key, what the merge
fold has to work on — the newest terminator T, the newest covering range
tombstone RD, the operands above max(T, RD) and the base — so the tests can
assert which shapes a stream really holds. Values come from the same walk.
TEST INFRASTRUCTURE ONLY; the expected values of the GPU tests are the
oracle's, the model says which keys are which.
"""
import random
import struct

import scan_streams as ss
from pywb import PyBatch

PUT, DELETE, MERGE, SINGLE_DELETE, RANGE_DELETE = 1, 0, 2, 7, 0x0F
_BASE = {0x00: DELETE, 0x01: PUT, 0x02: MERGE, 0x07: SINGLE_DELETE,
         0x0F: RANGE_DELETE, 0x04: DELETE, 0x05: PUT, 0x06: MERGE,
         0x08: SINGLE_DELETE, 0x0E: RANGE_DELETE}
_CF_TAGS = {0x04, 0x05, 0x06, 0x08, 0x0E}
MASK = (1 << 64) - 1
LENS = (0, 1, 3, 7, 8, 9, 16)


def _varint(rep, p):
    v = shift = 0
    while True:
        b = rep[p]
        p += 1
        v |= (b & 0x7F) << shift
        if b < 0x80:
            return v, p
        shift += 7


def _slice(rep, p):
    n, p = _varint(rep, p)
    return rep[p:p + n], p + n


def parse_rep(rep):
    """-> [(type, stored_key, value)]; for a range deletion the pair is
    (begin, end), both in the stored ([cf LE4 | key]) key space."""
    out, p = [], 12
    while p < len(rep):
        tag = rep[p]
        p += 1
        cf = 0
        if tag in _CF_TAGS:
            cf, p = _varint(rep, p)
        t = _BASE[tag]
        k, p = _slice(rep, p)
        v = b""
        if t in (PUT, MERGE, RANGE_DELETE):
            v, p = _slice(rep, p)
        if cf:
            k = ss.cfkey(cf, k)
            if t == RANGE_DELETE:
                v = ss.cfkey(cf, v)
        out.append((t, k, v))
    assert len(out) == struct.unpack_from("<I", rep, 8)[0]
    return out


class Model:
    def __init__(self, reps=()):
        self.t = 0
        self.ver = {}    # stored key -> [(t, type, value)], oldest first
        self.tombs = []  # (t, begin, end)
        for rep in reps:
            self.apply(rep)

    def apply(self, rep):
        for typ, k, v in parse_rep(rep):
            self.t += 1
            if typ == RANGE_DELETE:
                self.tombs.append((self.t, k, v))
            else:
                self.ver.setdefault(k, []).append((self.t, typ, v))

    def keys(self):
        return sorted(self.ver)

    def look(self, key):
        """-> dict(rd, term, ops (oldest first), base, shape)."""
        vs = self.ver.get(key, [])
        rd = max([t for t, b, e in self.tombs if b <= key < e], default=0)
        term = next(((t, typ, v) for t, typ, v in reversed(vs)
                     if typ != MERGE), None)
        tt = term[0] if term else 0
        floor = max(tt, rd)
        ops = [v for t, typ, v in vs if typ == MERGE and t > floor]
        base = term[2] if term and term[1] == PUT and tt > rd else None
        shape = None
        if ops:
            if base is not None:
                shape = "over_put"
            elif tt > rd:
                shape = "over_delete"
            elif any(typ == MERGE and tt < t < rd for t, typ, v in vs):
                shape = "cut_by_tomb"
            else:
                shape = "over_nothing"
        elif vs and vs[-1][1] == MERGE:
            shape = "dead"  # a chain at the top, wholly below a tombstone
        return dict(rd=rd, term=term, ops=ops, base=base, shape=shape)

    def live_chain(self, key):
        return bool(self.look(key)["ops"])

    def value(self, key, merge_op):
        s = self.look(key)
        if not s["ops"]:
            return s["base"]
        if merge_op == 1:
            acc = sum(int.from_bytes(v[:8], "little")
                      for v in s["ops"] + ([s["base"]] if s["base"] is not None
                                           else []))
            return (acc & MASK).to_bytes(8, "little")
        return b",".join(([s["base"]] if s["base"] is not None else []) +
                         s["ops"])


def counter_stream(seed, n_records=4000, n_batches=40):
    """A merge-heavy stream over ~200 stored keys: the scan tests' key pool
    (cf keys, families sharing 8- and 16-byte prefixes, the empty key), all
    five record types, value lengths from LENS. -> reps"""
    rng = random.Random(seed)
    pool = ss.key_pool(rng)
    users = pool  # holds b""
    cf_users = rng.sample(users, 50)
    per = [n_records // n_batches] * n_batches
    for i in range(n_records - sum(per)):
        per[i] += 1
    reps = []
    for nb in per:
        b = PyBatch()
        for _ in range(nb):
            cf = ss.CF if rng.random() < 0.25 else 0
            k = rng.choice(cf_users if cf else users)
            v = rng.randbytes(rng.choice(LENS))
            if rng.random() < 0.05:
                v = b"\xff" * rng.choice((8, 9, 16))
            x = rng.random()
            if x < 0.03:
                i = rng.randrange(len(pool))
                bk, ek = pool[i], pool[min(len(pool) - 1,
                                           i + rng.randrange(0, 4))]
                b.cf_delete_range(cf, bk, ek) if cf else b.delete_range(bk, ek)
            elif x < 0.18:
                b.cf_put(cf, k, v) if cf else b.put(k, v)
            elif x < 0.26:
                b.cf_delete(cf, k) if cf else b.delete(k)
            elif x < 0.30:
                b.cf_single_delete(cf, k) if cf else b.single_delete(k)
            else:
                b.cf_merge(cf, k, v) if cf else b.merge(k, v)
        reps.append(b.data())
    return reps
