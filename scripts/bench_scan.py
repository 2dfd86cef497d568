"""Range-scan cost over the device store: one shard, 100K entries (16 B keys,
128 B values), gra_scan at ~0.1 %, 1 %, 10 % and 100 % selectivity. Run on a
GPU box; a measurement tool, not a test.

Prints ms per scan and live keys/s for the device path and, in the same run,
for the host path: a second engine holding the same store plus one leader
write (a host-origin run routes the whole call to gra::run_scan), timed
after a first call so its runs are already fetched to the host.

Work per call is O(entries in the shard) on both paths — runs are unsorted
by key — so the small selectivities show the fixed cost of a scan.
"""
import ctypes as C
import os
import random
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import rocksplicator_amd as ra  # noqa: E402

N_ENTRIES = 100_000
VAL_LEN = 128
SELECTIVITY = (0.001, 0.01, 0.1, 1.0)
MIN_WINDOW_S = 0.5  # timed window per figure

lib = ra.load()
rng = random.Random(7)
keys = [f"user{i:012d}".encode() for i in range(N_ENTRIES)]  # 16 B, sorted
order = list(range(N_ENTRIES))
rng.shuffle(order)  # arrival order is not key order

arena = bytearray()
descs = []
for first in range(0, N_ENTRIES, 50):  # 50-record batches
    b = ra.Batch()
    for i in order[first:first + 50]:
        b.put(keys[i], rng.randbytes(VAL_LEN))
    rep = b.data()
    descs.append((0, len(rep), len(arena)))
    arena += rep
buf = (C.c_uint8 * (len(arena) + 64)).from_buffer_copy(bytes(arena) + b"\0" * 64)
ds = (ra.ffi.GraUpdateDesc * len(descs))()
for j, (s, ln, of) in enumerate(descs):
    ds[j].shard, ds[j].len, ds[j].off, ds[j].ts = s, ln, of, 0


def load_engine():
    e = ra.Engine(nshards=1, store_bytes=1 << 30)
    r = e.upload(C.cast(buf, C.POINTER(C.c_uint8)), len(arena), ds, len(descs))
    r.tick(0, len(descs))
    r.sync()
    return e, e.open(0), r


dev_e, dev_db, dev_r = load_engine()
host_e, host_db, host_r = load_engine()
host_db.write_leader(ra.Batch().put(b"zzzz-leader-key", b"x").data())
print(f"loaded 2 x {N_ENTRIES} entries ({len(keys[0])} B keys, {VAL_LEN} B "
      f"values), latest_seq={dev_db.latest_seq()}")

ents = (ra.ffi.GraScanEntry * (N_ENTRIES + 8))()
cap = N_ENTRIES * (len(keys[0]) + VAL_LEN) + 4096
out = C.create_string_buffer(cap)
info = ra.ffi.GraScanInfo()


def scan(db, lo, hi):
    rc = lib.gra_scan(db.h, lo, len(lo), hi, len(hi), N_ENTRIES + 8, ents,
                      out, cap, C.byref(info))
    assert rc == 0, rc
    return info.n


def bench(label, db, served_by, lo, hi, want):
    assert scan(db, lo, hi) == want  # warm: staging grown, host runs fetched
    assert info.served_by == served_by and info.more == 0
    t0 = time.perf_counter()
    scan(db, lo, hi)  # every call ends in a stream sync or is host work
    rounds = max(5, min(2000, int(MIN_WINDOW_S / (time.perf_counter() - t0))))
    t0 = time.perf_counter()
    for _ in range(rounds):
        scan(db, lo, hi)
    dt = (time.perf_counter() - t0) / rounds
    print(f"  {label}: {dt * 1e3:9.3f} ms/scan  {want / dt / 1e6:8.3f} M live keys/s"
          f"  ({rounds} scans timed)")
    return dt


for sel in SELECTIVITY:
    n = max(1, int(N_ENTRIES * sel))
    a = 0 if n == N_ENTRIES else N_ENTRIES // 3
    lo, hi = keys[a], (keys[a + n] if a + n < N_ENTRIES else b"user~")
    print(f"selectivity {sel * 100:g} % ({n} keys)")
    d = bench("device", dev_db, ra.GRA_SCAN_DEVICE, lo, hi, n)
    h = bench("host  ", host_db, ra.GRA_SCAN_HOST, lo, hi, n)
    print(f"  device/host time ratio: {d / h:.2f}"
          + ("  (device path SLOWER than host)" if d > h else ""))

# spot check: both paths return the same page
a = dev_db.scan_page(keys[500], keys[520])[0]
b = host_db.scan_page(keys[500], keys[520])[0]
assert a == b and [k for k, _ in a] == keys[500:520]
dev_e.close()
host_e.close()
