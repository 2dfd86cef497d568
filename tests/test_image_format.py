"""The shard-image format on a CPU box: rocksplicator_amd/image.py against the
tests' own byte-level statement (tests/pyimage.py), both against field-by-field
vectors (tests/golden/image_vectors.json), and gra_image_check — the host
verdict rule behind gra_export and in front of gra_import — through ctypes on
the vectors and on the hostile table. Expected verdicts never come from the
code under test."""
import json
import os
import random

import pytest

import pyimage
import rocksplicator_amd as ra
from rocksplicator_amd import image as rimage

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(HERE, "golden", "image_vectors.json")) as f:
        return json.load(f)["vectors"]


def vec_items(v):
    return [(bytes.fromhex(i["key"]), bytes.fromhex(i["value"]), i["seq"])
            for i in v["items"]]


def want_index(v):
    return pyimage.NO_INDEX if v["bad_index"] is None else v["bad_index"]


def test_vectors_are_what_both_packers_write(vectors):
    good = [v for v in vectors if v["reason"] == 0 and "kpref" not in v["name"]]
    assert len(good) >= 3
    for v in good:
        img = bytes.fromhex(v["image"])
        args = (vec_items(v), v["last_seq"], v["merge_op"])
        assert pyimage.pack(*args) == img, v["name"]
        assert rimage.pack_image(*args) == img, v["name"]
        assert len(img) == 64 + ((24 * len(v["items"]) + 15) & ~15) + sum(
            (len(k) + len(val) + 15) & ~15 for k, val, _ in args[0])


def test_vectors_unpack_and_judge(vectors):
    seen = set()
    for v in vectors:
        img = bytes.fromhex(v["image"])
        assert pyimage.verdict(img) == (v["reason"], want_index(v)), v["name"]
        seen.add(v["reason"])
        if v["reason"] == 0:
            f, items = pyimage.unpack(img)
            assert items == vec_items(v)
            got = rimage.unpack_image(img)
            assert got["items"] == vec_items(v)
            assert (got["last_seq"], got["merge_op"]) == \
                (v["last_seq"], v["merge_op"]) == (f["last_seq"], f["merge_op"])
    assert {0, 1, 2, 5, 6} <= seen


def test_gra_image_check_on_the_vectors(vectors):
    for v in vectors:
        img = bytes.fromhex(v["image"])
        info = ra.image_check(img)
        assert (info.reason, info.bad_index) == (v["reason"], want_index(v)), \
            v["name"]
        if v["reason"] == 0:
            assert info.n_entries == len(v["items"])
            assert info.last_seq == v["last_seq"]
            assert info.image_bytes == len(img)
            assert info.version == 1 and info.merge_op == v["merge_op"]


def test_packers_agree_on_random_items():
    rng = random.Random(77)
    for n in (0, 1, 2, 15, 16, 17, 300):
        keys = sorted({rng.randbytes(rng.randrange(0, 30)) for _ in range(n)})
        items = [(k, rng.randbytes(rng.choice((0, 1, 15, 16, 17, 100))),
                  rng.randrange(1, 1000)) for k in keys]
        for merge_op in (0, 1):
            img = pyimage.pack(items, 1000, merge_op)
            assert rimage.pack_image(items, 1000, merge_op) == img
            assert pyimage.verdict(img) == (pyimage.OK, pyimage.NO_INDEX)
            assert rimage.unpack_image(img)["items"] == items
            info = ra.image_check(img)
            assert info.reason == ra.GRA_IMG_OK
            assert info.n_entries == len(items)
    # pairs take last_seq
    img = rimage.pack_image([(b"a", b"1"), (b"b", b"2")], 44, 1)
    assert pyimage.unpack(img)[1] == [(b"a", b"1", 44), (b"b", b"2", 44)]


@pytest.mark.parametrize("items,last_seq,merge_op", [
    ([(b"b", b"", 1), (b"a", b"", 1)], 5, 0),    # descending
    ([(b"a", b"", 1), (b"a", b"", 2)], 5, 0),    # equal
    ([(b"a", b"", 0)], 5, 0),                    # seq 0
    ([(b"a", b"", 6)], 5, 0),                    # seq past last_seq
    ([(b"k" * 70000, b"", 1)], 5, 0),            # key_len is 16 bits
    ([(b"a", b"", 1)], 5, 2),                    # no such merge operator
])
def test_pack_image_refuses_what_the_importer_would(items, last_seq, merge_op):
    with pytest.raises(ValueError):
        rimage.pack_image(items, last_seq, merge_op)


def test_gra_image_check_on_the_hostile_table():
    good, cases = pyimage.hostile_table()
    assert pyimage.verdict(good) == (pyimage.OK, pyimage.NO_INDEX)
    assert ra.image_check(good).reason == ra.GRA_IMG_OK
    reasons = set()
    for name, img, header_level in cases:
        want = pyimage.verdict(img)
        assert want[0] != pyimage.OK, name
        assert header_level == (want[0] in (pyimage.BAD_HEADER,
                                            pyimage.BAD_SIZE)), name
        info = ra.image_check(img)
        assert (info.reason, info.bad_index) == want, name
        reasons.add(want[0])
    assert reasons == {1, 2, 3, 4, 5, 6}
    assert len(cases) == 22
