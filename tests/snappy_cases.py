"""Case table for the device Snappy stage (k_snappy -> snp::decompress).

A case is (name, shard-local list of (comp_bytes, ulen_meta, count)): the
compressed stream, the uncompressed length that the transport metadata
claims, and the batch's record count. The payload of every valid case is a
real WriteBatch blob, so an accepted stream also applies; values follow a
position-dependent pattern, so a shifted or duplicated chunk changes bytes.

INFO[name] holds what a test needs besides the stream: the plain blobs, the
keys to probe, the (kind, offset, length) elements that the case claims to
contain, and the exact compressed length where the case is about one.

TEST INFRASTRUCTURE ONLY. Used by test_snappy_cases_host.py (CPU) and
test_gpu_snappy.py (GPU).
"""
import ctypes as C
import functools
import random
import struct

import oracle_ffi
import pysnappy as ps
from pywb import PyBatch, lps, varint32

INFO = {}

OFFS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 63, 64, 2047, 2048, 65535]
LENS = [1, 4, 11, 15, 16, 17, 63, 64]
EXTRA_OFFS = [4, 5, 6, 10, 12, 14]  # tag 10 only: the other residues below
                                    # the 8- and 16-byte chunk thresholds
FAR_OFF = 65535          # offsets from here up live in the one 70 KB value
LIT_LENS = [1, 15, 16, 17, 60, 61, 255, 256, 257, 65536, 65537]
STAGE_LENS = [496, 507, 508, 509, 512, 1024]
REAL_MAX = 8192          # payloads up to this size also go through the
                         # two real compressors
MUTANT_SEED = 5
N_MUTANTS = 300


def pat(i, salt):
    return (i * 131 + salt * 17 + (i >> 8)) & 0xFF


def val(n, salt):
    return bytes(pat(i, salt) for i in range(n))


def kind_lens(kind):
    return [n for n in LENS if 4 <= n <= 11] if kind == "copy1" else LENS


def kind_holds(kind, off):
    return off < {"copy1": 2048, "copy2": 1 << 16, "copy4": 1 << 32}[kind]


# ------------------------------------------------------------ blob builder

def _head(key, vlen):
    return struct.pack("<QI", 0, 1) + b"\x01" + lps(key) + varint32(vlen)


def _oplen(op):
    return op[1] if op[0] == "lit" else op[3]


def build(key, ops, salt=0):
    """One-Put blob whose value is whatever `ops` produce, and the element
    list that produces the blob: the head (batch header, tag, key, value
    length) as one literal, then one element per op.
    ops: ('lit', n[, ext]) appends n pattern bytes as one literal;
    ('copy', kind, off, n) appends what that copy yields; off == 'op' means
    the current write position (the source starts at byte 0)."""
    head = _head(key, sum(_oplen(op) for op in ops))
    out = bytearray(head)
    els, claims = [ps.literal(head)], []
    for op in ops:
        if op[0] == "lit":
            start = len(out)
            out += bytes(pat(i, salt) for i in range(start, start + op[1]))
            els.append(ps.literal(out[start:], op[2] if len(op) > 2 else None))
            claims.append(("lit", op[2] if len(op) > 2 else None, op[1]))
        else:
            _, kind, off, n = op
            off = len(out) if off == "op" else off
            assert 0 < off <= len(out)
            for _ in range(n):
                out.append(out[-off])
            els.append(ps.COPY[kind](off, n))
            claims.append((kind, off, n))
    blob = bytes(out)
    assert blob == PyBatch().put(key, blob[len(head):]).data()
    return blob, els, claims


def comp_len_of(key, ops):
    """Compressed length of build(key, ops)'s stream, by arithmetic: varint
    + tag bytes + payload."""
    vlen = sum(_oplen(op) for op in ops)
    head = len(_head(key, vlen))
    total = len(ps.varint(head + vlen)) + 1 + head
    for op in ops:
        if op[0] == "lit":
            ext = op[2] if len(op) > 2 else None
            total += len(ps.literal_header(op[1], ext)) + op[1]
        else:
            total += {"copy1": 2, "copy2": 3, "copy4": 5}[op[1]]
    return total


def _built(table, name, key, ops, salt, comp_len=None):
    blob, els, claims = build(key, ops, salt)
    comp = ps.stream(len(blob), els)
    if comp_len is not None:
        assert len(comp) == comp_len == comp_len_of(key, ops)
    table.append((name, [(comp, len(blob), 1)]))
    INFO[name] = dict(plain=[blob], keys=[key], claims=claims,
                      comp_len=comp_len)


def _encoded(table, name, batch, keys, policy):
    blob = batch.data()
    table.append((name, [(ps.encode_with(blob, policy), len(blob), batch.count)]))
    INFO[name] = dict(plain=[blob], keys=keys, claims=[], comp_len=None)


def _fit(key, ops_of, want):
    """The literal length n at which ops_of(n) compresses to `want` bytes."""
    for n in range(1, want):
        if comp_len_of(key, ops_of(n)) == want:
            return n
    raise AssertionError(("no literal length gives", want))


# -------------------------------------------------------------- valid cases

def _geometry(table):
    """off x len x tag kind. One case per (kind, offset) holds every length,
    with 5-byte literals between the copies so that each copy starts at
    another residue; offsets >= FAR_OFF share the one 70 KB value."""
    salt = 1
    for kind in ("copy1", "copy2", "copy4"):
        for off in OFFS + (EXTRA_OFFS if kind == "copy2" else []):
            if off >= FAR_OFF or not kind_holds(kind, off):
                continue
            ops = [("lit", off + 3)]
            for n in kind_lens(kind):
                ops += [("copy", kind, off, n), ("lit", 5)]
            _built(table, f"{kind}_off{off}", b"geo-%s-%d" % (kind.encode(), off),
                   ops, salt)
            salt += 1
    # the literal of 65537 bytes, every length at offset 65535 in both tag
    # forms that hold it, then 4-byte offsets past 65535
    ops = [("lit", 65537)]
    for kind in ("copy2", "copy4"):
        for n in LENS:
            ops += [("copy", kind, FAR_OFF, n), ("lit", 5)]
    ops.append(("lit", 70000 - sum(_oplen(op) for op in ops)))
    for off, n in ((65536, 1), (65537, 16), (69000, 17), (69999, 64), (66000, 63)):
        ops += [("copy", "copy4", off, n), ("lit", 3)]
    _built(table, "far_lit65537", b"geo-far", ops, salt)


def _positions(table):
    # a copy as the last element: its chunk overshoot lands in the slot slack
    _built(table, "copy_last_off20_len37", b"pos-a",
           [("lit", 40), ("copy", "copy2", 20, 37)], 60)
    _built(table, "copy_last_off9_len13", b"pos-b",
           [("lit", 21), ("copy", "copy2", 9, 13)], 61)
    _built(table, "copy_last_off3_len64", b"pos-c",
           [("lit", 9), ("copy", "copy4", 3, 64)], 62)
    _built(table, "copy_last_copy1", b"pos-d",
           [("lit", 33), ("copy", "copy1", 17, 11)], 63)
    # a copy whose source starts at byte 0 of the slot (off == op), shorter
    # and longer than the head it copies
    _built(table, "copy_from0_len16", b"pos-e",
           [("copy", "copy2", "op", 16), ("lit", 7)], 64)
    _built(table, "copy_from0_len64", b"pos-f",
           [("copy", "copy2", "op", 64), ("lit", 7)], 65)


def _literals(table):
    for i, n in enumerate(LIT_LENS):
        if n == 65537:
            continue  # in far_lit65537
        ops = ([("lit", n), ("lit", 9)] if n > 1000 else
               [("lit", 3), ("lit", n), ("lit", 6), ("lit", n)])
        _built(table, f"lit_{n}", b"lit-%d" % n, ops, 70 + i)
    _built(table, "lit_ext3_small", b"lit-x3",
           [("lit", 5, 3), ("lit", 17, 3), ("lit", 1, 3)], 90)
    _built(table, "lit_ext4_small", b"lit-x4",
           [("lit", 5, 4), ("lit", 17, 4), ("lit", 1, 4)], 91)
    _built(table, "lit_noncanonical", b"lit-nc",
           [("lit", 1, 1), ("lit", 60, 1), ("lit", 61, 2), ("lit", 60, 0),
            ("lit", 255, 2), ("lit", 16, 1)], 92)


def _stage(table):
    """comp_len on both sides of the LDS stage (508): one long literal, and
    one long literal followed by a copy whose operand ends the stream."""
    for i, want in enumerate(STAGE_LENS):
        key = b"stage-lit-%d" % want
        n = _fit(key, lambda n: [("lit", n)], want)
        _built(table, f"stage_lit_{want}", key, [("lit", n)], 100 + i, want)
        key = b"stage-copy-%d" % want
        tail = lambda n: [("lit", n), ("copy", "copy2", 33, 20)]  # noqa: E731
        n = _fit(key, tail, want)
        _built(table, f"stage_copy_{want}", key, tail(n), 110 + i, want)


def multi_batch(nrec, salt):
    """nrec records, Put / Delete / Merge / DeleteRange in turn."""
    b, keys = PyBatch(), []
    for j in range(nrec):
        k = b"mr%02d-%03d" % (salt, j)
        keys.append(k)
        if j % 4 == 0:
            b.put(k, val(20 + 7 * j % 190, salt + j))
        elif j % 4 == 1:
            b.delete(b"mr%02d-%03d" % (salt, j - 1) if j % 8 == 1 else k)
        elif j % 4 == 2:
            b.merge(b"mr%02d-ctr" % salt, val(8 + j % 5, j))
        else:
            b.delete_range(b"mr%02d-%03d" % (salt, j - 3), k)
    keys.append(b"mr%02d-ctr" % salt)
    assert b.count == nrec
    return b, keys


def _multi(table):
    for nrec, policy in ((2, ps.Policy("copy1")),
                         (7, ps.Policy("copy2", lit_split=16)),
                         (64, ps.Policy("copy4", max_copy_len=17))):
        b, keys = multi_batch(nrec, nrec)
        _encoded(table, f"multi_{nrec}", b, keys, policy)


def _policies(table):
    """One compressible blob (64-byte blocks that recur, as the generator
    makes them) through policies that give distinct streams."""
    blocks = [val(64, s) for s in range(4)]
    value = b"".join(blocks[(i * 7 + i // 3) % 4][:64 - (i % 3)] for i in range(24))
    # short periods (1, 2, 7, 9, 15), for the policies that bound the distance
    value += (b"x" * 40 + b"ab" * 20 + b"1234567" * 9 + b"abcdefghi" * 6
              + b"0123456789ABCDE" * 5)
    batch = PyBatch().put(b"policy", value)
    for tag, p in (("copy1", ps.Policy("copy1")),
                   ("copy2_len5", ps.Policy("copy2", max_copy_len=5)),
                   ("copy4", ps.Policy("copy4")),
                   ("lit1_ext4", ps.Policy(None, lit_split=1, lit_ext=4)),
                   ("lit16", ps.Policy(None, lit_split=16)),
                   ("dist_1_7", ps.Policy("copy2", min_dist=1, max_dist=7)),
                   ("dist_8_15", ps.Policy("copy2", min_dist=8, max_dist=15)),
                   ("dist_64_up", ps.Policy("copy2", min_dist=64))):
        _encoded(table, f"policy_{tag}", batch, [b"policy"], p)


@functools.lru_cache(maxsize=None)
def libs():
    import rocksplicator_amd as ra
    olib = oracle_ffi.load()
    olib.orc_snappy_compress.restype = C.c_size_t
    olib.orc_snappy_compress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p,
                                         C.c_size_t]
    olib.orc_snappy_decompress.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p,
                                           C.c_size_t, C.POINTER(C.c_size_t)]
    return olib, ra.load()


def orc_decompress(comp, cap):
    """The oracle's verdict: uncompressed bytes, or None."""
    olib, _ = libs()
    dst = C.create_string_buffer(cap + 16)
    dlen = C.c_size_t()
    if olib.orc_snappy_decompress(comp, len(comp), dst, cap, C.byref(dlen)):
        return None
    return dst.raw[:dlen.value]


def gra_decompress(comp, cap):
    """snp::decompress on the host (byte loops): bytes, or None."""
    _, glib = libs()
    dst = C.create_string_buffer(cap + 16)
    r = glib.gra_snappy_decompress(comp, len(comp), dst, cap)
    return None if r == 0xFFFFFFFF else dst.raw[:r]


def _real(table):
    olib, glib = libs()
    for name, ups in list(table):
        info = INFO[name]
        blob = info["plain"][0]
        if len(blob) > REAL_MAX:
            continue
        cap = len(blob) + len(blob) // 6 + 64
        buf = C.create_string_buffer(cap)
        for tag, fn in (("gra", glib.gra_snappy_compress),
                        ("orc", olib.orc_snappy_compress)):
            clen = fn(blob, len(blob), buf, cap)
            assert clen > 0
            table.append((f"{tag}:{name}", [(buf.raw[:clen], len(blob), ups[0][2])]))
            INFO[f"{tag}:{name}"] = dict(info, claims=[], comp_len=None)


@functools.lru_cache(maxsize=None)
def valid_cases():
    table = []
    _geometry(table)
    _positions(table)
    _literals(table)
    _stage(table)
    _multi(table)
    _policies(table)
    _real(table)
    assert len({name for name, _ in table}) == len(table)
    return table


# ----------------------------------------------------------- mixed window

@functools.lru_cache(maxsize=None)
def mixed_window(nshards=4, n=300):
    """About 300 streams whose comp_len runs over 380..639, so roughly half
    stage into LDS and half parse from global memory.
    -> [(shard, comp, ulen_meta, count, plain, key)] in generation order."""
    out = []
    for i in range(n):
        want = 380 + (i * 37) % 260
        key = b"mix%04d" % i
        ops_of = lambda n: [("lit", n), ("copy", "copy2", 16 + i % 50, 1 + i % 64)]  # noqa: E731
        ops = ops_of(_fit(key, ops_of, want))
        blob, els, _ = build(key, ops, i)
        comp = ps.stream(len(blob), els)
        assert len(comp) == want
        out.append((i % nshards, comp, len(blob), 1, blob, key))
    return out


# ---------------------------------------------------------- malformed cases

@functools.lru_cache(maxsize=None)
def malformed_cases():
    """Streams that every decoder must reject (or, for varint_minus1, that
    disagree with the metadata). Each is rejected by a bounds check that
    runs before the write it guards, so the partial output stays inside
    the slot of ulen_meta bytes plus its slack."""
    table = []

    def add(name, comp, ulen):
        table.append((name, [(bytes(comp), ulen, 1)]))
        INFO[name] = dict(plain=[], keys=[b"mal"], claims=[], comp_len=None)

    mid = [("lit", 40), ("copy", "copy2", 30, 20), ("lit", 40)]
    blob, els, _ = build(b"mal", mid, 200)
    U, good = len(blob), ps.stream(len(blob), els)
    head = len(blob) - 100
    assert ps.decode(good, U) == blob

    # truncations
    add("trunc_end", good[:-1], U)
    for kind, cut in (("copy1", 1), ("copy2", 1), ("copy2", 2), ("copy4", 3)):
        b2, e2, _ = build(b"mal", [("lit", 40), ("copy", kind, 30, 8)], 201)
        add(f"trunc_{kind}_operand_{cut}", ps.stream(len(b2), e2)[:-cut], len(b2))
    b2, e2, _ = build(b"mal", [("lit", 40), ("lit", 300)], 202)
    for keep in (1, 2):  # tag only, tag + one of the two length bytes
        add(f"trunc_ext_len_{keep}",
            ps.stream(len(b2), e2[:2]) + e2[2][:keep], len(b2))

    # offsets that reach nowhere
    for kind in ("copy1", "copy2", "copy4"):
        add(f"off0_{kind}",
            ps.stream(U, [els[0], els[1], ps.COPY[kind](0, 8, check=False),
                          ps.literal(blob[head + 48:])]), U)
    add("off_op_plus1",
        ps.stream(U, [els[0], els[1], ps.copy2(head + 41, 20), els[3]]), U)
    add("copy_first_off1", ps.stream(U, [ps.copy2(1, 20), ps.literal(blob[20:])]), U)
    add("copy_first_off0",
        ps.stream(U, [ps.copy2(0, 20, check=False), ps.literal(blob[20:])]), U)

    # one byte too many, one too few
    add("over_by_literal", ps.stream(U, els[:3] + [ps.literal(blob[-40:] + b"!")]), U)
    b2, e2, _ = build(b"mal", [("lit", 40), ("copy", "copy2", 30, 20)], 203)
    add("over_by_copy", ps.stream(len(b2), e2[:2] + [ps.copy2(30, 21)]), len(b2))
    add("over_by_copy1",
        ps.stream(len(b2) - 10, e2[:2] + [ps.copy1(30, 11)]), len(b2) - 10)
    add("ends_short", ps.stream(U, els[:3] + [ps.literal(blob[-40:-1])]), U)
    add("ends_short_after_copy", ps.stream(U, els[:3]), U)

    # the stream's own length field
    add("varint_unterminated", b"\x80" * 5 + good[len(ps.varint(U)):], U)
    add("varint_cut", b"\xe4\x80", U)
    add("varint_plus1",
        ps.stream(U + 1, els[:3] + [ps.literal(blob[-40:] + b"\x00")]), U)
    add("varint_minus1",
        ps.stream(U - 1, els[:3] + [ps.literal(blob[-40:-1])]), U)
    assert ps.decode(table[-1][1][0][0], U) == blob[:-1]  # decodes, wrong size

    # bytes after a complete stream
    add("garbage_literal_after", good + ps.literal(b"Z"), U)
    add("garbage_byte_after", good + b"\xff", U)

    # extended literal lengths near 2^32 (4 length bytes): len 0xFFFFFFFF
    # wraps a 32-bit ip + len, and len 2^32 wraps a 32-bit len itself to 0,
    # after which the rest of this stream is consistent
    lit4 = lambda raw: (ps.stream(U, [ps.literal(blob[:30])])  # noqa: E731
                        + bytes([63 << 2]) + raw)
    add("r02_lit4_len_ffffffff", lit4(b"\xfe\xff\xff\xff") + blob[30:], U)
    add("lit4_len_2p32", lit4(b"\xff\xff\xff\xff") + ps.literal(blob[30:]), U)
    return table


# ------------------------------------------------------------------ mutants

@functools.lru_cache(maxsize=None)
def mutants():
    """N_MUTANTS single-byte mutations (60 %) or truncations (40 %) of the
    valid streams below 600 bytes, drawn with MUTANT_SEED. With seed 5 the
    oracle accepts and applies 128 of them and rejects 172.
    -> case table; INFO[name]['keys'] are the source case's keys."""
    rng = random.Random(MUTANT_SEED)
    pool = [(name, ups[0]) for name, ups in valid_cases()
            if len(ups[0][0]) < 600]
    table = []
    for i in range(N_MUTANTS):
        src, (comp, ulen, count) = pool[rng.randrange(len(pool))]
        comp = bytearray(comp)
        if rng.random() < 0.6:
            at = rng.randrange(len(comp))
            comp[at] ^= rng.randrange(1, 256)
            name = f"mut{i:03d}:{src}@{at}"
        else:
            del comp[rng.randrange(1, len(comp)):]
            name = f"mut{i:03d}:{src}[:{len(comp)}]"
        table.append((name, [(bytes(comp), ulen, count)]))
        INFO[name] = dict(plain=[], keys=INFO[src]["keys"], claims=[],
                          comp_len=None)
    return table


# ----------------------------------------------------------- expected state

class Expected:
    """What the oracle and the metadata alone say the shards must hold.
    Updates go in one by one, in tick order; an update of a poisoned shard
    is skipped, and an update that is not good poisons its shard."""

    def __init__(self, nshards, merge_op=0):
        self.olib, _ = libs()
        self.ost = oracle_ffi.Store(self.olib, nshards, merge_op=merge_op)
        self.poisoned = set()
        self.applied = 0

    def good(self, shard, comp, ulen_meta, ts=0):
        plain = orc_decompress(comp, ulen_meta)
        return (plain is not None and len(plain) == ulen_meta
                and self.ost.apply(shard, plain, ts))

    def feed(self, shard, comp, ulen_meta, ts=0):
        if shard in self.poisoned:
            return False
        if not self.good(shard, comp, ulen_meta, ts):
            self.poisoned.add(shard)
            return False
        self.applied += 1
        return True

    def seq(self, shard):
        return self.ost.latest_seq(shard)

    def checksum(self, shard):
        return self.olib.orc_shard_checksum(self.ost.h, shard)

    def get(self, shard, key):
        return self.ost.get(shard, key)
