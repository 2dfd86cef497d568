"""Host range scan (gra::run_scan, the host side of gra_scan) against the
oracle, on a CPU box: scripts/test_host_scan.cpp is built with plain g++
against host_store.cpp and driven over stdin. Expected results come from the
oracle store only; equality is exact."""
import os
import subprocess

import pytest

import oracle_ffi
import scan_streams as ss

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "build", "test_host_scan")
NO_CAP = 1 << 30
NO_MAX = 1 << 30


@pytest.fixture(scope="module")
def driver():
    os.makedirs(os.path.join(REPO, "build"), exist_ok=True)
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra",
         "scripts/test_host_scan.cpp", "rocksplicator_amd/csrc/host_store.cpp",
         "-o", BIN], cwd=REPO, check=True)
    return BIN


@pytest.fixture(scope="module")
def stream():
    return ss.make_stream(seed=20, n_records=2000, n_batches=40)


def hx(b):
    return b.hex() if b else "-"


def unhx(s):
    return b"" if s == "-" else bytes.fromhex(s)


def run_scans(driver, reps, scans, merge_op):
    """scans: [(lo, hi, max_entries, cap)] -> [(rc, more, [(key, value)])],
    all in one driver process."""
    lines = ["run " + r.hex() for r in reps]
    for lo, hi, mx, cap in scans:
        lines.append(f"scan {hx(lo)} {'*' if hi is None else hx(hi)} "
                     f"{mx} {cap} {merge_op}")
    r = subprocess.run([driver], input="\n".join(lines) + "\n",
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out, it = [], iter(r.stdout.splitlines())
    for line in it:
        f = line.split()
        assert f[0] == "rc", line
        rc, n, more = int(f[1]), int(f[3]), int(f[5])
        ents = []
        for e in it:
            if e == "end":
                break
            k, v = e.split()
            ents.append((unhx(k), unhx(v)))
        assert len(ents) == n
        out.append((rc, more, ents))
    assert len(out) == len(scans)
    return out


def oracle_for(reps, merge_op):
    olib = oracle_ffi.load()
    ost = oracle_ffi.Store(olib, 1, merge_op=merge_op)
    for rep in reps:
        assert ost.apply(0, rep)
    return ost


@pytest.mark.parametrize("merge_op", [0, 1])
def test_scan_ranges_match_oracle(driver, stream, merge_op):
    reps, universe, _ = stream
    ost = oracle_for(reps, merge_op)
    ranges = ss.scan_set(5, universe)
    got = run_scans(driver, reps,
                    [(lo, hi, NO_MAX, NO_CAP) for lo, hi in ranges], merge_op)
    nonempty = 0
    for (lo, hi), (rc, more, ents) in zip(ranges, got):
        assert rc == 0 and more == 0, (lo, hi)
        assert ents == ss.expected(ost, 0, universe, lo, hi), (lo, hi)
        nonempty += bool(ents)
    full = got[0][2]
    assert len(full) > 50          # the stream leaves plenty alive ...
    assert len(full) < len(universe)  # ... and plenty dead
    assert nonempty > 25


def paged(driver, reps, lo, hi, mx, cap, merge_op):
    """Page with the documented resume rule, one driver process per page."""
    pages, cur = [], lo
    while True:
        (rc, more, ents), = run_scans(driver, reps, [(cur, hi, mx, cap)],
                                      merge_op)
        assert rc == 0
        pages.append((more, ents))
        if not more:
            return pages
        assert ents  # a page that reports more always made progress
        cur = ents[-1][0] + b"\x00"


@pytest.mark.parametrize("merge_op", [0, 1])
def test_scan_pagination(driver, stream, merge_op):
    reps, universe, _ = stream
    ost = oracle_for(reps, merge_op)
    lo, hi = universe[5], universe[-5]
    want = ss.expected(ost, 0, universe, lo, hi)
    assert len(want) > 30
    for mx in (1, 7):
        # one driver process per page: single-entry pages over a prefix
        phi, pwant = (want[20][0], want[:20]) if mx == 1 else (hi, want)
        pages = paged(driver, reps, lo, phi, mx, NO_CAP, merge_op)
        assert [e for _, p in pages for e in p] == pwant
        assert all(len(p) == mx for _, p in pages[:-1])
        assert [m for m, _ in pages] == [1] * (len(pages) - 1) + [0]
    # a cap that cuts mid-range: every page fits, the pages concatenate to
    # the one-shot scan
    cap = 2 * max(len(k) + len(v) for k, v in want) + 3
    pages = paged(driver, reps, lo, hi, NO_MAX, cap, merge_op)
    assert len(pages) > 3
    assert [e for _, p in pages for e in p] == want
    assert all(sum(len(k) + len(v) for k, v in p) <= cap for _, p in pages)
    # a cap below the first entry reports too-small (GRA_BUF_TOO_SMALL = 2)
    k0, v0 = want[0]
    (rc, more, ents), = run_scans(
        driver, reps, [(lo, hi, NO_MAX, len(k0) + len(v0) - 1)], merge_op)
    assert rc == 2 and ents == []
    (rc, more, ents), = run_scans(
        driver, reps, [(lo, hi, NO_MAX, len(k0) + len(v0))], merge_op)
    assert rc == 0 and ents == [want[0]] and more == 1


def test_scan_agrees_with_point_gets_semantics(driver):
    """Hand-written cases for the per-key rule: only the newest entry and
    the covering tombstones decide."""
    from pywb import PyBatch
    reps = [
        PyBatch().put(b"a", b"1").put(b"b", b"2").put(b"c", b"3").data(),
        PyBatch().delete_range(b"a", b"c").data(),       # kills a, b
        PyBatch().merge(b"b", b"m").put(b"d", b"").data(),  # merge over tomb
        PyBatch().delete(b"c").merge(b"e", b"x").merge(b"e", b"y").data(),
    ]
    ost = oracle_for(reps, 0)
    universe = [b"a", b"b", b"c", b"d", b"e"]
    (rc, more, ents), = run_scans(driver, reps, [(b"", None, 10, 100)], 0)
    assert rc == 0 and more == 0
    assert ents == [(b"b", b"m"), (b"d", b""), (b"e", b"x,y")]
    assert ents == ss.expected(ost, 0, universe, b"", None)
