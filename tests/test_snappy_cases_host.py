"""The Snappy case table (snappy_cases.py) checked on a CPU box: the three
decoders agree on every stream, the valid cases apply, the table holds what
its names claim, the mutants exercise both verdicts, the stream compressor
keeps its contract, and snp::decompress stays inside its slot under ASan.

The product decoder runs here as its host build (byte loops); the device's
chunked copies are covered by test_gpu_snappy.py on the same table.
"""
import ctypes as C
import os
import subprocess

import pytest

import oracle_ffi
import pysnappy as ps
import rocksplicator_amd as ra
import snappy_cases as sc
from rocksplicator_amd.ffi import GRA_FULL, GRA_OK, GraUpdateDesc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "build", "test_snappy_bounds")


def all_tables():
    return (("valid", sc.valid_cases()), ("malformed", sc.malformed_cases()),
            ("mutant", sc.mutants()))


def streams(table):
    for name, ups in table:
        for comp, ulen, count in ups:
            yield name, comp, ulen, count


# ------------------------------------------------------- pysnappy itself

def test_pysnappy_known_vectors():
    """The decoder against streams written out by hand from the format
    description, so it does not only ever see its own encoder's output."""
    assert ps.decode(b"\x00", 0) == b""
    assert ps.decode(b"\x05\x10hello", 5) == b"hello"
    # "ab" + copy1(off 2, len 4) -> ababab ; tag 01, len-4 = 0, off 2
    assert ps.decode(b"\x06\x04ab\x01\x02", 6) == b"ababab"
    # copy2: tag = (len-1) << 2 | 2, len 5, off 1 -> run of 'x'
    assert ps.decode(b"\x06\x00x\x12\x01\x00", 6) == b"xxxxxx"
    # copy4, off 3 len 3
    assert ps.decode(b"\x06\x08abc\x0b\x03\x00\x00\x00", 6) == b"abcabc"
    # literal with one length byte: tag 60 << 2, len-1 = 2
    assert ps.decode(b"\x03\xf0\x02abc", 3) == b"abc"
    # rejects: cap, offset 0, offset past start, short, long, cut operand
    assert ps.decode(b"\x05\x10hello", 4) is None
    assert ps.decode(b"\x06\x04ab\x01\x00", 6) is None
    assert ps.decode(b"\x06\x04ab\x01\x03", 6) is None
    assert ps.decode(b"\x06\x10hello", 6) is None
    assert ps.decode(b"\x04\x10hello", 4) is None
    assert ps.decode(b"\x06\x04ab\x12\x01", 6) is None
    assert ps.decode(b"\x80", 9) is None and ps.decode(b"", 9) is None
    # the encoder's elements read back as written
    s = ps.stream(20, [ps.literal(b"abcde", 4), ps.copy1(5, 4),
                       ps.copy2(9, 10), ps.copy4(1, 1)])
    assert [(e.kind, e.off, e.len, e.ext) for e in ps.elements(s)] == [
        ("lit", 0, 5, 4), ("copy1", 5, 4, 0), ("copy2", 9, 10, 0),
        ("copy4", 1, 1, 0)]
    assert ps.decode(s, 20) == b"abcde" + b"abcd" + b"abcdeabcda" + b"a"


def test_encode_with_roundtrips_and_obeys_policy():
    sc.valid_cases()
    blob = sc.INFO["policy_copy1"]["plain"][0]
    seen = set()
    for name, ups in sc.valid_cases():
        if not name.startswith("policy_"):
            continue
        comp = ups[0][0]
        assert ps.decode(comp, len(blob)) == blob, name
        seen.add(comp)
    assert len(seen) == 8  # eight policies, eight distinct streams
    by = {n: list(ps.elements(u[0][0])) for n, u in sc.valid_cases()
          if n.startswith("policy_")}
    kinds = lambda n: {e.kind for e in by[n]}  # noqa: E731
    assert "copy1" in kinds("policy_copy1")
    assert kinds("policy_copy4") == {"lit", "copy4"}
    assert kinds("policy_lit1_ext4") == {"lit"}
    assert all(e.len == 1 and e.ext == 4 for e in by["policy_lit1_ext4"])
    assert all(e.len <= 16 for e in by["policy_lit16"])
    assert all(e.len <= 5 for e in by["policy_copy2_len5"] if e.kind != "lit")
    for n, lo, hi in (("policy_dist_1_7", 1, 7), ("policy_dist_8_15", 8, 15),
                      ("policy_dist_64_up", 64, 65535)):
        offs = [e.off for e in by[n] if e.kind != "lit"]
        assert offs and all(lo <= o <= hi for o in offs), n


# ------------------------------------------------------ three-way agreement

@pytest.mark.parametrize("which", ["valid", "malformed", "mutant"])
def test_three_decoders_agree(which):
    """pysnappy.decode arbitrates; the oracle's and the product's host
    decoder must give its verdict and its bytes for every stream."""
    table = dict(all_tables())[which]
    n = 0
    for name, comp, ulen, _ in streams(table):
        want = ps.decode(comp, ulen)
        assert sc.orc_decompress(comp, ulen) == want, ("oracle", name)
        assert sc.gra_decompress(comp, ulen) == want, ("product", name)
        n += 1
    assert n >= 25


def test_valid_cases_decode_and_apply():
    olib, _ = sc.libs()
    table = sc.valid_cases()
    ost = oracle_ffi.Store(olib, len(table))
    for shard, (name, ups) in enumerate(table):
        for (comp, ulen, count), plain in zip(ups, sc.INFO[name]["plain"]):
            assert len(plain) == ulen, name
            assert ps.decode(comp, ulen) == plain, name
            _, cnt, _ = oracle_ffi.decode(olib, plain)
            assert cnt == count, name
            assert ost.apply(shard, plain, 0), name
        assert ost.latest_seq(shard) == sum(c for _, _, c in ups), name


def test_malformed_cases_are_not_good():
    """Every malformed case fails the rule that the GPU test expects by:
    the oracle rejects it, or it decodes to another size than claimed."""
    table = sc.malformed_cases()
    exp = sc.Expected(len(table))
    for shard, (name, comp, ulen, _) in enumerate(streams(table)):
        assert not exp.good(shard, comp, ulen), name
        assert exp.seq(shard) == 0, name
    only_size = [n for n, c, u, _ in streams(table) if ps.decode(c, u) is not None]
    assert only_size == ["varint_minus1"]


# ------------------------------------------------- the table says what it claims

def test_stage_boundary_lengths():
    got = {}
    for name, comp, ulen, _ in streams(sc.valid_cases()):
        want = sc.INFO[name]["comp_len"]
        if want is not None:
            assert len(comp) == want, name
            assert name.endswith(str(want))
            got.setdefault(name.rsplit("_", 1)[0], []).append(want)
    assert got == {"stage_lit": sc.STAGE_LENS, "stage_copy": sc.STAGE_LENS}
    lens = sorted(len(c) for _, c, _, _, _, _ in sc.mixed_window())
    assert len(lens) == 300
    # after the length sort the first block of 256 holds both kinds
    assert lens[0] <= 508 < lens[255] and lens[-1] > 508
    assert 100 < sum(n <= 508 for n in lens) < 200


def test_geometry_cases_contain_their_elements():
    """Parse every built stream back: the elements after the head literal
    are exactly the claimed ones, and the cross of offsets, lengths and tag
    kinds that the table promises is all there."""
    seen = set()
    for name, comp, ulen, _ in streams(sc.valid_cases()):
        claims = sc.INFO[name]["claims"]
        if not claims:
            continue
        els = list(ps.elements(comp))[1:]
        assert len(els) == len(claims), name
        for e, (kind, off, n) in zip(els, claims):
            if kind == "lit":
                assert (e.kind, e.len) == ("lit", n), name
                assert off is None or e.ext == off, name  # forced form
            else:
                assert (e.kind, e.off, e.len) == (kind, off, n), name
                seen.add((kind, off, n))
    for kind in ("copy1", "copy2", "copy4"):
        for off in sc.OFFS:
            for n in sc.kind_lens(kind):
                if sc.kind_holds(kind, off):
                    assert (kind, off, n) in seen, (kind, off, n)
    rel = {(o < n) - (o > n) for _, o, n in seen}
    assert rel == {-1, 0, 1}  # off > len, off == len, off < len
    assert any(k == "copy4" and o > 65535 for k, o, _ in seen)
    lits = {(e.len, e.ext) for _, c, _, _ in streams(sc.valid_cases())
            for e in ps.elements(c) if e.kind == "lit"}
    canon = lambda n: 0 if n <= 60 else ((n - 1).bit_length() + 7) // 8  # noqa: E731
    for n in sc.LIT_LENS:
        assert (n, canon(n)) in lits, n
    assert {(5, 3), (5, 4), (1, 3), (1, 4), (17, 3), (17, 4)} <= lits
    # a copy as the last element, and one that reads from byte 0
    for name in ("copy_last_off20_len37", "copy_last_off9_len13",
                 "copy_last_off3_len64", "copy_last_copy1"):
        comp = dict(sc.valid_cases())[name][0][0]
        assert list(ps.elements(comp))[-1].kind != "lit", name
    for name in ("copy_from0_len16", "copy_from0_len64"):
        head, cp = list(ps.elements(dict(sc.valid_cases())[name][0][0]))[:2]
        assert cp.off == head.len, name


def test_real_compressor_baseline_is_narrow():
    """What the issue is about: both real compressors emit only literals
    and 2-byte-offset copies, so the baseline cases cover no other tag."""
    kinds = {e.kind for n, c, _, _ in streams(sc.valid_cases())
             if n.startswith(("gra:", "orc:")) for e in ps.elements(c)}
    assert kinds == {"lit", "copy2"}


def test_mutant_verdict_counts():
    """By the oracle's verdict alone: 128 mutants accepted and applied,
    172 rejected (seed 5); both must stay at 30 or more."""
    table = sc.mutants()
    assert len(table) == sc.N_MUTANTS == 300
    exp = sc.Expected(len(table))
    ok = sum(exp.feed(s, comp, ulen)
             for s, (_, comp, ulen, _) in enumerate(streams(table)))
    bad = len(table) - ok
    print(f"mutants: accepted-and-applied {ok}, rejected {bad}")
    assert ok >= 30 and bad >= 30


# ------------------------------------------------ gra_snappy_compress_stream

@pytest.mark.parametrize("nthreads", [1, 3, 16])
def test_compress_stream(nthreads):
    _, glib = sc.libs()
    n = 2000
    arena, used, descs = ra.gen_stream(nshards=7, n_updates=n, key_len=16,
                                       val_len=256, kind=2, seed=9, ts=41,
                                       compressible=1)
    raw = bytes(arena)[:used]
    cap = sum(32 + d.len + d.len // 6 for d in descs)
    out = (C.c_uint8 * cap)()
    out_descs = (GraUpdateDesc * n)()
    ulens = (C.c_uint32 * n)()
    out_used = C.c_size_t()
    src = C.cast(arena, C.POINTER(C.c_uint8))
    rc = glib.gra_snappy_compress_stream(src, descs, n, out, cap,
                                         C.byref(out_used), out_descs, ulens,
                                         nthreads)
    assert rc == GRA_OK
    assert 0 < out_used.value <= cap
    comp = bytes(out)
    total = 0
    for i in range(n):
        d, o = descs[i], out_descs[i]
        assert o.len > 0 and o.off + o.len <= out_used.value, i
        assert ulens[i] == d.len, i
        assert (o.shard, o.ts) == (d.shard, d.ts), i
        assert d.ts == 41
        plain = sc.orc_decompress(comp[o.off:o.off + o.len], d.len)
        assert plain == raw[d.off:d.off + d.len], i
        total += o.len
    assert total < used  # the stream is compressible and was compressed
    # slots do not overlap
    spans = sorted((o.off, o.off + o.len) for o in out_descs)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    # one byte too little for the worst-case layout: GRA_FULL, nothing else
    rc = glib.gra_snappy_compress_stream(src, descs, n, out, cap - 1,
                                         C.byref(out_used), out_descs, ulens,
                                         nthreads)
    assert rc == GRA_FULL


# --------------------------------------------------------------- sanitizer

@pytest.fixture(scope="module")
def driver():
    os.makedirs(os.path.join(REPO, "build"), exist_ok=True)
    subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
         "scripts/test_snappy_bounds.cpp", "-o", BIN], cwd=REPO, check=True)
    return BIN


def test_decompress_stays_in_slot_under_asan(driver):
    """snp::decompress, host build, under ASan + UBSan in a stand-alone
    program: every stream of the table sits in a heap buffer of its exact
    size and decodes into one of exactly ulen_meta + 16 bytes, so a bounds
    check that lets a malformed stream read past its end or write past its
    slot is a sanitizer report. Verdicts and bytes must match
    pysnappy.decode.

    This covers the bounds checks that the host and the device share. It
    does not run the device-only branches (16- and 8-byte chunk copies,
    their overshoot into the slack, the LDS stage): those run only on the
    GPU, in test_gpu_snappy.py."""
    rows = [r for _, t in all_tables() for r in streams(t)]
    text = "".join(f"{ulen} {comp.hex() or '-'}\n" for _, comp, ulen, _ in rows)
    r = subprocess.run([driver], input=text, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(rows)
    for (name, comp, ulen, _), line in zip(rows, lines):
        want = ps.decode(comp, ulen)
        if want is None:
            assert line == "bad", name
        else:
            f = line.split()
            assert f[0] == "ok" and int(f[1]) == len(want), name
            assert (b"" if f[2] == "-" else bytes.fromhex(f[2])) == want, name
