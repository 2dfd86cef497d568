"""Host run compaction (gra::run_compact, the plain-C++ restatement of
gra_compact) against the oracle, on a CPU box: scripts/test_compact_host.cpp
is built with g++ -fsanitize=address,undefined as its own program and driven
over stdin. Expected values come from the oracle store and from
tests/fold_model.py, never from the code under test; equality is exact."""
import os
import subprocess

import pytest

import fold_model as fm
import oracle_ffi
import scan_streams as ss
from pywb import PyBatch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "build", "test_compact_host")
NO_CAP = 1 << 30
NO_MAX = 1 << 30
PUT = 1


@pytest.fixture(scope="module")
def driver():
    os.makedirs(os.path.join(REPO, "build"), exist_ok=True)
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "scripts/test_compact_host.cpp",
         "rocksplicator_amd/csrc/host_store.cpp", "-o", BIN],
        cwd=REPO, check=True)
    return BIN


@pytest.fixture(scope="module")
def stream():
    return ss.make_stream(seed=22, n_records=2000, n_batches=40)


def hx(b):
    return b.hex() if b else "-"


def unhx(s):
    return b"" if s == "-" else bytes.fromhex(s)


def fnv32(b):
    h = 2166136261
    for x in b:
        h = ((h ^ x) * 16777619) & 0xFFFFFFFF
    return h


def drive(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n",
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return iter(r.stdout.splitlines())


def read_compact(it):
    f = next(it).split()
    assert f[0] == "compact"
    return dict(rc=int(f[1]), n=int(f[2]), payload=int(f[3]), base=int(f[4]),
                last=int(f[5]), sorted=int(f[6]))


def read_dump(it):
    recs = []
    for line in it:
        if line == "end":
            return recs
        f = line.split()
        assert f[0] == "rec", line
        recs.append(dict(seq=int(f[1]), type=int(f[2]), flags=int(f[3]),
                         kv_off=int(f[4]), kpref=int(f[5]), key=unhx(f[6]),
                         val=unhx(f[7])))
    raise AssertionError("dump without end")


def read_get(it):
    f = next(it).split()
    assert f[0] == "get"
    return unhx(f[2]) if f[1] == "0" else None


def read_scan(it):
    f = next(it).split()
    assert f[0] == "rc", f
    rc, n, more = int(f[1]), int(f[3]), int(f[5])
    ents = []
    for e in it:
        if e == "end":
            break
        k, v = e.split()
        ents.append((unhx(k), unhx(v)))
    assert len(ents) == n
    return rc, more, ents


def oracle_for(reps, merge_op):
    ost = oracle_ffi.Store(oracle_ffi.load(), 1, merge_op=merge_op)
    for rep in reps:
        assert ost.apply(0, rep)
    return ost


def absent_keys(universe):
    out = [b"no-such-key-%02d" % i for i in range(40)]
    out += [ss.cfkey(ss.CF, b"nokey%d" % i) for i in range(10)]
    assert not set(out) & set(universe)
    return out


def check_run_shape(recs, info):
    """Sorted, Put-only, laid out as the apply path lays a run out."""
    assert info["rc"] == 0 and info["sorted"] == 1 and info["n"] == len(recs)
    keys = [r["key"] for r in recs]
    assert all(a < b for a, b in zip(keys, keys[1:]))  # strictly ascending
    off = 0
    for r in recs:
        assert r["type"] == PUT and r["flags"] == 0
        assert r["kv_off"] % 16 == 0 and r["kv_off"] == off
        assert r["kpref"] == fnv32(r["key"])
        off += (len(r["key"]) + len(r["val"]) + 15) & ~15
    assert off == info["payload"]


@pytest.mark.parametrize("merge_op", [0, 1])
@pytest.mark.parametrize("cut", [0, 10, 20, 30])
def test_compacted_runs_read_like_the_oracle(driver, stream, merge_op, cut):
    """cut 0 compacts all 40 runs; the others every proper prefix, with the
    rest left as runs on top."""
    reps, universe, _ = stream
    ost = oracle_for(reps, merge_op)
    keys = universe + absent_keys(universe)
    ranges = ss.scan_set(6, universe)
    lines = ["run " + r.hex() for r in reps]
    lines += [f"compact {cut} {merge_op}", "dump 0"]
    lines += [f"get {hx(k)} {merge_op}" for k in keys]
    lines += [f"scan {hx(lo)} {'*' if hi is None else hx(hi)} "
              f"{NO_MAX} {NO_CAP} {merge_op}" for lo, hi in ranges]
    it = drive(driver, lines)
    info = read_compact(it)
    recs = read_dump(it)
    check_run_shape(recs, info)
    # the run holds exactly what the oracle finds in the compacted prefix
    n_pre = cut or len(reps)
    pre = oracle_for(reps[:n_pre], merge_op)
    model = fm.Model(reps[:n_pre])
    want = [(k, pre.get(0, k)) for k in universe]
    want = [(k, v) for k, v in want if v is not None]
    assert [(r["key"], r["val"]) for r in recs] == want
    assert len(want) > 30
    for r in recs:  # a key carries its newest entry's seq
        assert r["seq"] == model.ver[r["key"]][-1][0]
    assert info["base"] == 1 and info["last"] == model.t
    # reads over [compacted + rest] are the oracle's over the whole stream
    vals = {k: ost.get(0, k) for k in keys}  # the reference, computed once
    found = 0
    for k in keys:
        got = read_get(it)
        assert got == vals[k], k
        found += got is not None
    assert found > 30 and found < len(universe)
    nonempty = 0
    for lo, hi in ranges:
        rc, more, ents = read_scan(it)
        assert rc == 0 and more == 0
        assert ents == [(k, vals[k]) for k in universe
                        if ss.in_range(k, lo, hi) and vals[k] is not None], \
            (lo, hi)
        nonempty += bool(ents)
    assert nonempty > 25


def chain_reps(shape, nops=300):
    """One concat/u64add chain of `nops` operands on b"chain", over three
    runs, with neighbours on both sides."""
    ops = [b"%03d" % i + b"x" * (i % 13) for i in range(nops)]
    first = PyBatch().put(b"before", b"b").put(b"later", b"l")
    if shape == "over_put":
        first.put(b"chain", b"base-value")
    elif shape == "over_delete":
        first.put(b"chain", b"gone").delete(b"chain")
    reps = [first.data()]
    for lo in range(0, nops, 100):
        b = PyBatch()
        for i in range(lo, min(lo + 100, nops)):
            if shape == "cut_by_tomb" and i == 150:
                b.delete_range(b"c", b"d")
            b.merge(b"chain", ops[i])
        reps.append(b.data())
    return reps


@pytest.mark.parametrize("merge_op", [0, 1])
@pytest.mark.parametrize("shape", ["over_put", "over_delete", "cut_by_tomb"])
def test_long_chains_fold_to_the_model(driver, shape, merge_op):
    reps = chain_reps(shape)
    model = fm.Model(reps)
    look = model.look(b"chain")
    assert look["shape"] == shape
    assert len(look["ops"]) == (150 if shape == "cut_by_tomb" else 300)
    want = model.value(b"chain", merge_op)
    assert want == oracle_for(reps, merge_op).get(0, b"chain")
    it = drive(driver, ["run " + r.hex() for r in reps] +
               [f"compact 0 {merge_op}", "dump 0", f"get {hx(b'chain')} {merge_op}"])
    info = read_compact(it)
    recs = read_dump(it)
    check_run_shape(recs, info)
    assert [r["key"] for r in recs] == [b"before", b"chain", b"later"]
    assert recs[1]["val"] == want
    assert recs[1]["seq"] == model.t  # the newest operand is the last record
    assert read_get(it) == want
