"""What a shard image costs, and what it saves: gra_export and gra_import
timed against the two things they stand beside. Run on a GPU box; a
measurement tool, not a test. No figure here is held to a threshold.

Workloads, as scripts/bench_compact.py: the README's 100K-entry shard (100K
Puts, 16 B keys, 128 B values) and the Zipf counter shard (100,777 records
over 8192 counters, GRA_MERGE_U64ADD).

Per workload, in one run:
  export   Db.export_image_raw with an exact-size buffer on a follower whose
           history arrived in ticks of 400 batches (the device chain; the
           store is untouched, so the call repeats)
  import   Db.import_image into a fresh shard each time; wall time of the
           call, and the library's own split of it (GRA_IMAGE_TIMING=1:
           device events around the H2D copy, check + reserve, place)
  replay   an empty follower brought to the same state the parent's only
           way: every batch of the history through handle_replicate_response,
           then flush (a fresh shard each time)
  d2d      one device-to-device hipMemcpyAsync of the image's bytes, synced

Every timed call ends in a device sync. One warm-up call per figure, then
REPEATS calls; a figure is their median, its spread (max - min) / median.
"""
import ctypes as C
import os
import random
import re
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
os.environ["GRA_IMAGE_TIMING"] = "1"  # read once, at the first import call

import rocksplicator_amd as ra  # noqa: E402

REPEATS = 7
TICK_BATCHES = 400
ENGINE = dict(store_bytes=1 << 30, staging_bytes=256 << 20)


def median(ts):
    return sorted(ts)[len(ts) // 2]


def show(label, ts, extra=""):
    m = median(ts)
    print(f"  {label:34s} {m * 1e3:9.3f} ms  spread "
          f"{(max(ts) - min(ts)) / m:6.1%}  calls ["
          + ", ".join(f"{t * 1e3:.3f}" for t in ts) + f"] ms{extra}")
    return m


def once(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


class StderrCapture:
    """The library's stderr lines (fd 2) while the block runs."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        sys.stderr.flush()
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            lib = C.CDLL(name)
            break
        except OSError:
            continue
    else:
        raise RuntimeError("libamdhip64.so not found: no d2d figure without it")
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    lib.hipFree.argtypes = [C.c_void_p]
    lib.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    lib.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t,
                                   C.c_int, C.c_void_p]
    return lib


def d2d_figure(nbytes):
    lib = hip()
    a, b = C.c_void_p(), C.c_void_p()
    assert lib.hipMalloc(C.byref(a), nbytes) == 0
    assert lib.hipMalloc(C.byref(b), nbytes) == 0
    assert lib.hipMemset(a, 1, nbytes) == 0

    def copy():
        assert lib.hipMemcpyAsync(b, a, nbytes, 3, None) == 0  # D2D
        assert lib.hipDeviceSynchronize() == 0

    copy()
    ts = [once(copy) for _ in range(REPEATS)]
    lib.hipFree(a)
    lib.hipFree(b)
    return ts


def apply_history(e, db, reps):
    for i, rep in enumerate(reps):
        assert db.handle_replicate_response(rep)
        if (i + 1) % TICK_BATCHES == 0:
            e.flush()
    e.flush()


def workload(name, reps, merge_op):
    n_targets = REPEATS + 1
    src_e = ra.Engine(nshards=1, merge_op=merge_op, **ENGINE)
    src = src_e.open(0)
    apply_history(src_e, src, reps)
    S = src.latest_seq()
    _, img, info = src.export_image_raw(1 << 28)
    assert img is not None and info.served_by == 0
    nbytes = len(img)
    print(f"== {name}: {sum(len(r) for r in reps)} bytes of history in "
          f"{len(reps)} batches, last seq {S}; image {nbytes} bytes, "
          f"{info.n_entries} entries ==")
    used = src_e.store_usage().used
    ts = [once(lambda: src.export_image_raw(nbytes)) for _ in range(REPEATS)]
    assert src_e.store_usage().used == used
    t_export = show("export (device chain + D2H)", ts)

    dst_e = ra.Engine(nshards=n_targets, merge_op=merge_op, **ENGINE)
    walls, splits = [], []
    for s in range(n_targets):
        db = dst_e.open(s)
        with StderrCapture() as cap:
            walls.append(once(lambda: db.import_image(img)))
        m = re.search(r"h2d ([\d.]+) ms, check\+reserve ([\d.]+) ms, "
                      r"place ([\d.]+) ms", cap.text)
        assert m, cap.text
        splits.append(tuple(float(x) / 1e3 for x in m.groups()))
        assert db.latest_seq() == S
    assert dst_e.open(1).checksum() == info.content_sum
    t_import = show("import (wall, fresh shard)", walls[1:])
    for i, part in enumerate(("h2d", "check + reserve", "place")):
        show(f"  of it, {part} (device events)", [s[i] for s in splits[1:]])
    dst_e.close()

    rep_e = ra.Engine(nshards=n_targets, merge_op=merge_op, **ENGINE)
    ts = []
    for s in range(n_targets):
        db = rep_e.open(s)
        ts.append(once(lambda: apply_history(rep_e, db, reps)))
        assert db.latest_seq() == S
    t_replay = show("replay the history (fresh shard)", ts[1:])
    rep_e.close()
    src_e.close()

    t_d2d = show("d2d hipMemcpyAsync of the image", d2d_figure(nbytes))
    print(f"  import / replay {t_import / t_replay:.3f}, import / d2d "
          f"{t_import / t_d2d:.1f}, export / d2d {t_export / t_d2d:.1f}")


def put_shard():
    rng = random.Random(7)
    keys = [f"user{i:012d}".encode() for i in range(100_000)]
    order = list(range(len(keys)))
    rng.shuffle(order)
    reps = []
    for first in range(0, len(keys), 50):
        b = ra.Batch()
        for i in order[first:first + 50]:
            b.put(keys[i], rng.randbytes(128))
        reps.append(b.data())
    return reps


def counter_shard():
    n_keys, n_records = 8192, 100_000
    rng = random.Random(7)
    keys = [f"ctr{i:013d}".encode() for i in range(n_keys)]
    weights = [1.0 / (r + 1) ** 0.99 for r in range(n_keys)]
    rank = list(range(n_keys))
    rng.shuffle(rank)
    picks = rng.choices(range(n_keys), weights=weights, k=n_records)
    records = [(rank[r], r != 0 and rng.random() < 0.01,
                rng.getrandbits(20).to_bytes(8, "little")) for r in picks]
    seen = {i for i, _, _ in records}
    records += [(i, False, (1).to_bytes(8, "little"))
                for i in range(n_keys) if i not in seen]
    rng.shuffle(records)
    reps = []
    for first in range(0, len(records), 50):
        b = ra.Batch()
        for i, is_set, v in records[first:first + 50]:
            (b.put if is_set else b.merge)(keys[i], v)
        reps.append(b.data())
    return reps


if __name__ == "__main__":
    workload("100K-entry shard (Puts, 16 B keys, 128 B values)", put_shard(),
             ra.MERGE_CONCAT)
    workload("Zipf counter shard (8192 counters, u64add)", counter_shard(),
             ra.MERGE_U64ADD)
