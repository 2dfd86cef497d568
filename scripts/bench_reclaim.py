"""What gra_reclaim costs: 1024 shards filled with a few ticks of the headline
shape (bench.py's: 16 B keys, 1 KiB values, Zipf, 819200 updates a tick, 50
updates a run), every other shard compacted, then Engine.reclaim() timed. Run
on a GPU box; a measurement tool, not a test.

The timed span is a host clock around reclaim(), which ends in a stream sync.
One warm-up engine, then --engines identical engines: the figure is their
median, the spread (max - min) / median. GRA_RECLAIM_TIMING=1 makes the
library print the call's phases (collect, plan, copies, rewrite) on stderr,
which tells the copy kernel's share from the host's. The sweep runs one engine
per "piece:bounce" pair (bytes) after that, and --first-only one engine per
pair in which only shard 0 is compacted: a small gap in front of the whole
store, the layout the batch rule likes least. The yardstick is one
hipMemcpyAsync device-to-device copy of bytes_moved bytes on the same box,
median of five after a warm-up: not the code under test.

A sample of shards is checksummed before and after every reclaim and must
not change.
"""
import argparse
import ctypes as C
import mmap
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ.setdefault("GRA_RECLAIM_TIMING", "1")

import rocksplicator_amd as ra  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument("--nshards", type=int, default=1024)
p.add_argument("--tick-updates", type=int, default=819200)
p.add_argument("--ticks", type=int, default=3)
p.add_argument("--key-len", type=int, default=16)
p.add_argument("--val-len", type=int, default=1024)
p.add_argument("--engines", type=int, default=3)
p.add_argument("--sweep", default="16384:67108864,65536:67108864,"
               "262144:67108864,1048576:67108864,4194304:67108864,"
               "65536:4194304,16777216:67108864",
               help="comma-separated piece:bounce byte pairs, '' for none")
p.add_argument("--first-only", default="65536:67108864,1048576:67108864,"
               "4194304:67108864,16777216:67108864",
               help="pairs for the layout with only shard 0 compacted")
args = p.parse_args()
lib = ra.load()

n_upd = args.tick_updates * args.ticks
worst = n_upd * (23 + args.key_len + args.val_len + 16) + 4096
arena = (C.c_uint8 * worst).from_buffer(mmap.mmap(-1, worst))
arena_p = C.cast(arena, C.POINTER(C.c_uint8))
descs = (ra.ffi.GraUpdateDesc * n_upd)()
g = ra.ffi.GraGenOpts(args.nshards, args.key_len, args.val_len, 1, 1 << 24,
                      0.99, 0xB0CC5EED, 0, 0)
used = C.c_size_t()
rc = lib.gra_gen_stream(C.byref(g), n_upd, arena_p, worst, C.byref(used),
                        descs, 0)
assert rc == 0, rc
used = used.value
print(f"stream: {n_upd} updates, {used / 1e9:.3f} GB, {args.ticks} ticks of "
      f"{args.tick_updates} over {args.nshards} shards", flush=True)
SAMPLE = sorted({0, 1, 2, 3, args.nshards // 2, args.nshards // 2 + 1,
                 args.nshards - 2, args.nshards - 1} & set(range(args.nshards)))


def one_engine(label, piece=None, bounce=None, step=2):
    for name, v in (("GRA_RECLAIM_PIECE", piece), ("GRA_RECLAIM_BOUNCE", bounce)):
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)
    e = ra.Engine(nshards=args.nshards, store_bytes=int(used * 2.2) + (1 << 28),
                  staging_bytes=64 << 20)
    r = e.upload(arena_p, used, descs, n_upd)
    for t in range(args.ticks):
        r.tick(t * args.tick_updates, args.tick_updates)
    r.sync()
    dbs = [e.open(s) for s in range(args.nshards)]
    t0 = time.perf_counter()
    victims = range(0, args.nshards, step)
    for s in victims:
        info = dbs[s].compact()
        assert info.status == ra.GRA_COMPACT_DONE, (s, info.status)
    t_compact = time.perf_counter() - t0
    before = e.store_usage()
    sums = [dbs[s].checksum() for s in SAMPLE]
    t0 = time.perf_counter()
    info = e.reclaim()
    wall = time.perf_counter() - t0
    assert info.status == ra.GRA_RECLAIM_DONE
    assert [dbs[s].checksum() for s in SAMPLE] == sums, "content changed"
    after = e.store_usage()
    assert after.used == info.used_after and after.live == before.live
    assert e.reclaim().status == ra.GRA_RECLAIM_NOTHING
    print(f"{label}: reclaim {wall * 1e3:9.3f} ms  moved {info.bytes_moved} B "
          f"({info.bytes_moved / wall / 1e9:7.1f} GB/s of moved bytes)  "
          f"bounced {info.bytes_bounced} B "
          f"({info.bytes_bounced / max(1, info.bytes_moved):.2%})  "
          f"batches {info.batches}  runs moved {info.runs_moved}  used "
          f"{info.used_before} -> {info.used_after} (live {before.live})  "
          f"[{len(victims)} compactions took {t_compact:.2f} s]",
          flush=True)
    del r
    e.close()
    return wall, info


one_engine("warm-up ")
runs = [one_engine(f"default {i}") for i in range(args.engines)]
walls = sorted(w for w, _ in runs)
mid = walls[len(walls) // 2]
moved = runs[0][1].bytes_moved
print(f"== reclaim(), default sizes: median {mid * 1e3:.3f} ms, spread "
      f"{(walls[-1] - walls[0]) / mid:.1%}, {moved / mid / 1e9:.1f} GB/s of "
      f"{moved} moved bytes ==", flush=True)
for pair in filter(None, args.sweep.split(",")):
    piece, bounce = (int(x) for x in pair.split(":"))
    one_engine(f"piece {piece:>9} bounce {bounce:>9}", piece, bounce)

for pair in filter(None, args.first_only.split(",")):
    piece, bounce = (int(x) for x in pair.split(":"))
    one_engine(f"shard 0 only, piece {piece:>9} bounce {bounce:>9}", piece,
               bounce, step=args.nshards)

# the yardstick, through the HIP runtime the library has loaded
path = next(line.split()[-1] for line in open("/proc/self/maps")
            if "libamdhip64" in line)
hip = C.CDLL(path)
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                               C.c_void_p]
hip.hipFree.argtypes = [C.c_void_p]
D2D = 3  # hipMemcpyDeviceToDevice
a, b = C.c_void_p(), C.c_void_p()
assert hip.hipMalloc(C.byref(a), moved) == 0
assert hip.hipMalloc(C.byref(b), moved) == 0
assert hip.hipMemset(b, 1, moved) == 0 and hip.hipDeviceSynchronize() == 0
ts = []
for i in range(6):
    t0 = time.perf_counter()
    assert hip.hipMemcpyAsync(a, b, moved, D2D, None) == 0
    assert hip.hipDeviceSynchronize() == 0
    ts.append(time.perf_counter() - t0)
hip.hipFree(a)
hip.hipFree(b)
ts = sorted(ts[1:])  # the first is the warm-up
ymid = ts[len(ts) // 2]
print(f"== yardstick: one hipMemcpyAsync device-to-device copy of {moved} B: "
      f"median {ymid * 1e3:.3f} ms, spread {(ts[-1] - ts[0]) / ymid:.1%}, "
      f"{moved / ymid / 1e9:.1f} GB/s ==")
print(f"== reclaim() wall / yardstick = {mid / ymid:.2f} ==")
