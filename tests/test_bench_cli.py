"""bench.py command line: a plain run prints only the headline line, --full
adds the side legs, and --dump-outputs writes the timed path's results —
checked here against the CPU oracle applied to the same seeded window."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_ffi
import rocksplicator_amd as ra

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")

# smallest shape that still has several shards, two 50-update groups per
# shard per tick, and a last step that lands on a non-first resident window
NSHARDS, TICK, KEY, VAL, STEPS, WARMUP = 8, 800, 16, 64, 3, 2
SHAPE = ["--nshards", str(NSHARDS), "--tick-updates", str(TICK),
         "--key-len", str(KEY), "--val-len", str(VAL)]


def test_cli_has_full_and_dump_options():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True,
                         text=True, check=True).stdout
    assert "--full" in out and "--dump-outputs" in out


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("dump"))
    r = subprocess.run(
        [sys.executable, BENCH, "--gpus", "1", "--steps", str(STEPS),
         "--warmup", str(WARMUP), "--dump-outputs", d, *SHAPE],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), d


@pytest.mark.gpu
def test_plain_run_is_headline_only(plain_run):
    res, _ = plain_run
    for k in ("metric", "value", "unit", "higher_is_better", "dtype",
              "ms_per_step"):
        assert k in res
    assert res["steps"] == STEPS and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(TICK / (res["ms_per_step"] * 1e-3))
    for k in ("h2d_staged", "drain_host", "cpu_baseline", "gpu_vs_cpu"):
        assert k not in res


@pytest.mark.gpu
def test_dump_outputs_match_oracle(plain_run):
    _, d = plain_run
    arrs = {n[:-4]: np.load(os.path.join(d, n)) for n in os.listdir(d)}
    assert set(arrs) == {"shard_latest_seq", "shard_apply_failures",
                         "apply_stats", "last_step_checksum"}
    assert all(a.dtype == np.float64 for a in arrs.values())
    n_ticks = min(STEPS + WARMUP, 6)
    assert arrs["shard_latest_seq"].tolist() == [n_ticks * TICK // NSHARDS] * NSHARDS
    assert not arrs["shard_apply_failures"].any()
    ticks, updates, records = arrs["apply_stats"][:3]
    assert (ticks, updates, records) == (STEPS, STEPS * TICK, STEPS * TICK)

    # the same seeded stream bench.py generates (rank 0), last step's window
    arena, used, descs = ra.gen_stream(
        nshards=NSHARDS, n_updates=n_ticks * TICK, key_len=KEY, val_len=VAL,
        kind=1, key_space=1 << 24, zipf_s=0.99, seed=0xB0CC5EED)
    raw = bytes(arena)[:used]
    olib = oracle_ffi.load()
    ost = oracle_ffi.Store(olib, NSHARDS)
    first = ((WARMUP + STEPS - 1) % n_ticks) * TICK
    for i in range(first, first + TICK):
        dsc = descs[i]
        assert ost.apply(dsc.shard, raw[dsc.off:dsc.off + dsc.len], dsc.ts)
    want = [olib.orc_shard_checksum(ost.h, s) for s in range(NSHARDS)]
    got = [(int(hi) << 32) | int(lo) for hi, lo in arrs["last_step_checksum"]]
    assert got == want


@pytest.mark.gpu
def test_full_run_adds_side_legs():
    # the drain leg sizes its ring store from the tick's bytes and the engine
    # wants that >= 10x the 256 MiB staging default, so a tick must carry
    # >= ~112 MB: 128000 updates x 1 KB values is the smallest round shape
    r = subprocess.run(
        [sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1",
         "--full", "--cpu-sample-seconds", "0.05", "--nshards", "64",
         "--tick-updates", "128000", "--key-len", "16", "--val-len", "1024"],
        capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("h2d_staged", "drain_host", "cpu_baseline", "gpu_vs_cpu"):
        assert k in res
