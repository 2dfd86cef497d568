"""Shared inputs for the range-scan tests (tests/test_scan_host.py and
tests/test_gpu_scan.py): a seeded WriteBatch stream over a key pool built to
stress the scan comparator, the scan set both tests run, and the oracle-side
expectation. TEST INFRASTRUCTURE ONLY.

Expected results always come from the oracle store: a scan of [lo, hi) must
return exactly the stored keys in that range for which orc_get finds a
value, ascending, with that value.
"""
import random
import struct

from pywb import PyBatch

CF = 3


def cfkey(cf, k):
    """Stored form of a column-family key: [cf LE4 | key]."""
    return struct.pack("<I", cf) + k


def key_pool(rng):
    """~170 user keys, lengths 0..40: short keys, keys that are prefixes of
    each other (zero-byte extensions included), and two families sharing
    8- and 16-byte prefixes so ordering is decided past the first 8 bytes."""
    pool = {b"", b"a", b"ab", b"abc", b"abcd", b"abcd\x00", b"abcd\x00\x00",
            b"abcdefgh", b"abcdefgh\x00", b"abcdefghi", b"\x00", b"\x00\x00",
            b"\xff", b"\xff\xff\xff\xff\xff\xff\xff\xff\xff"}
    for _ in range(30):
        pool.add(bytes(rng.choice(b"abxyz\x00\xff")
                       for _ in range(rng.randrange(1, 8))))
    p8 = b"PREFIX8_"
    pool.add(p8)
    for _ in range(50):
        pool.add(p8 + bytes(rng.choice(b"01\x00\xfe")
                            for _ in range(rng.randrange(0, 9))))
    p16 = b"sixteen-byte-pfx"
    pool.add(p16)
    for _ in range(50):
        pool.add(p16 + bytes(rng.choice(b"pq\x00")
                             for _ in range(rng.randrange(0, 25))))
    assert max(len(k) for k in pool) <= 40
    return sorted(pool)


def make_stream(seed, n_records, n_batches):
    """-> (reps, universe, points): reps = one WriteBatch rep per batch;
    universe = every stored key a point record wrote; points = the stored
    key of every point record, one element per version."""
    rng = random.Random(seed)
    pool = key_pool(rng)
    per = [n_records // n_batches] * n_batches
    for i in range(n_records - sum(per)):
        per[i] += 1
    reps, points = [], []
    for nb in per:
        b = PyBatch()
        for _ in range(nb):
            cf = CF if rng.random() < 0.25 else 0
            k = rng.choice(pool)
            v = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 41)))
            x = rng.random()
            if x < 0.04:
                i = rng.randrange(len(pool))
                j = i + rng.randrange(-1, 5)  # mostly narrow, some empty
                bk, ek = pool[i], pool[max(0, min(len(pool) - 1, j))]
                if cf:
                    b.cf_delete_range(cf, bk, ek)
                else:
                    b.delete_range(bk, ek)
                continue
            if x < 0.54:
                b.cf_put(cf, k, v) if cf else b.put(k, v)
            elif x < 0.66:
                b.cf_delete(cf, k) if cf else b.delete(k)
            elif x < 0.74:
                b.cf_single_delete(cf, k) if cf else b.single_delete(k)
            else:
                b.cf_merge(cf, k, v) if cf else b.merge(k, v)
            points.append(cfkey(cf, k) if cf else k)
        reps.append(b.data())
    return reps, sorted(set(points)), points


def in_range(k, lo, hi):
    return lo <= k and (hi is None or k < hi)


def scan_set(seed, universe):
    """[(lo, hi)] with hi None = unbounded: the full range, ~50 random
    ranges, lo == hi, lo > hi, and bounds equal to existing keys."""
    rng = random.Random(seed)
    u = universe
    out = [(b"", None), (b"", b""), (u[0], u[-1]), (u[0], u[-1] + b"\x00")]
    for _ in range(50):
        a, b = rng.choice(u), rng.choice(u)
        if rng.random() < 0.3:  # bounds that are not stored keys
            a = a[:rng.randrange(len(a) + 1)] + bytes([rng.randrange(256)])
        if rng.random() < 0.3:
            b = b[:rng.randrange(len(b) + 1)] + bytes([rng.randrange(256)])
        lo, hi = min(a, b), max(a, b)
        out.append((lo, hi if rng.random() < 0.9 else None))
    k = u[len(u) // 2]
    out += [(k, k), (u[-1], u[0]), (k + b"\x00", k),       # lo == hi, lo > hi
            (k, k + b"\x00"), (u[3], u[10]), (u[10], u[11]),  # existing keys
            (cfkey(CF, b""), cfkey(CF + 1, b"")),          # exactly cf 3
            (cfkey(CF, b"PREFIX8_"), cfkey(CF, b"PREFIX8`"))]
    return out


def expected(ost, shard, universe, lo, hi, cap=1 << 20):
    """Oracle-side answer for a scan of [lo, hi); cap bounds one value."""
    out = []
    for k in universe:
        if in_range(k, lo, hi):
            v = ost.get(shard, k, cap)
            if v is not None:
                out.append((k, v))
    return out
