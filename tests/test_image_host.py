"""The host side of shard images (gra::run_compact -> gra::image_from_run ->
gra::check_image) on a CPU box: scripts/test_image_host.cpp is built with
g++ -fsanitize=address,undefined as its own program and driven over stdin.
Expected images come from tests/pyimage.py packing what tests/fold_model.py
says the shard holds (its values checked against the oracle), expected
verdicts from pyimage.verdict — never from the code under test. Runs before
tests/test_gpu_image.py sends the same hostile table to a GPU."""
import os
import subprocess

import pytest

import fold_model as fm
import oracle_ffi
import pyimage
import scan_streams as ss

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "build", "test_image_host")


@pytest.fixture(scope="module")
def driver():
    os.makedirs(os.path.join(REPO, "build"), exist_ok=True)
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "scripts/test_image_host.cpp",
         "rocksplicator_amd/csrc/host_store.cpp", "-o", BIN],
        cwd=REPO, check=True)
    return BIN


def drive(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n",
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return iter(r.stdout.splitlines())


def unhx(s):
    return b"" if s == "-" else bytes.fromhex(s)


def read_image(it):
    f = next(it).split()
    assert f[0] == "image"
    return int(f[1]), unhx(f[2])


def read_check(it):
    f = next(it).split()
    assert f[0] == "check"
    idx = int(f[2])
    return dict(reason=int(f[1]),
                bad_index=pyimage.NO_INDEX if idx < 0 else idx,
                n=int(f[3]), payload_bytes=int(f[4]), image_bytes=int(f[5]),
                last_seq=int(f[6]), content_sum=int(f[7]))


STREAMS = {
    "scan_stream": lambda: ss.make_stream(seed=24, n_records=2000,
                                          n_batches=40)[0],
    "counter_stream": lambda: fm.counter_stream(25, n_records=2000),
    "short": lambda: ss.make_stream(seed=26, n_records=30, n_batches=3)[0],
}


@pytest.mark.parametrize("merge_op", [0, 1])
@pytest.mark.parametrize("kind", sorted(STREAMS))
def test_round_trip_is_the_model(driver, kind, merge_op):
    reps = STREAMS[kind]()
    model = fm.Model(reps)
    ost = oracle_ffi.Store(oracle_ffi.load(), 1, merge_op=merge_op)
    for rep in reps:
        assert ost.apply(0, rep)
    items = pyimage.items_from_model(model, merge_op)
    for k in model.keys():  # the model's values are the oracle's
        assert model.value(k, merge_op) == ost.get(0, k), k
    assert kind == "short" or len(items) > 30
    want = pyimage.pack(items, model.t, merge_op)
    it = drive(driver, ["run " + r.hex() for r in reps] +
               [f"image {merge_op}", "check " + want.hex()])
    rc, img = read_image(it)
    assert rc == 0
    assert img == want
    chk = read_check(it)
    assert (chk["reason"], chk["bad_index"]) == (pyimage.OK, pyimage.NO_INDEX)
    f = pyimage.fields(want)
    assert (chk["n"], chk["payload_bytes"], chk["image_bytes"],
            chk["last_seq"], chk["content_sum"]) == \
        (len(items), f["payload_bytes"], len(want), model.t, f["content_sum"])


def test_empty_shard_and_all_dead(driver):
    from pywb import PyBatch
    dead = PyBatch().put(b"a", b"1").put(b"b", b"2").delete(b"a") \
        .delete_range(b"b", b"c").data()
    it = drive(driver, ["image 0", "run " + dead.hex(), "image 1"])
    assert read_image(it) == (0, pyimage.pack([], 0, 0))
    assert read_image(it) == (0, pyimage.pack([], 4, 1))


def test_hostile_images_get_pyimages_verdict(driver):
    good, cases = pyimage.hostile_table(600)
    it = drive(driver, ["check " + good.hex()] +
               ["check " + (img.hex() or "-") for _, img, _ in cases] +
               ["check -", "check " + good[:63].hex()])
    chk = read_check(it)
    assert (chk["reason"], chk["n"]) == (pyimage.OK, 600)
    seen = set()
    for name, img, _ in cases:
        want = pyimage.verdict(img)
        chk = read_check(it)
        assert (chk["reason"], chk["bad_index"]) == want, name
        seen.add(want)
    # the table says what it claims to
    assert {r for r, _ in seen} == {1, 2, 3, 4, 5, 6}
    assert (pyimage.BAD_RECORD, 37) in seen      # two faults: the lower
    assert (pyimage.BAD_ORDER, 64) in seen and (pyimage.BAD_ORDER, 256) in seen
    assert (pyimage.BAD_ORDER, 257) in seen
    assert (pyimage.BAD_LAYOUT, 599) in seen     # key_len past the payload
    for _ in range(2):  # no bytes at all, a cut header
        chk = read_check(it)
        assert chk["reason"] == pyimage.BAD_HEADER
