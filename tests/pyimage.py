"""An independent byte-level statement of the shard-image format (version 1)
for the tests: packer, unpacker and the verdict rule, written from the
format's description and sharing no code with rocksplicator_amd/image.py or
the C++ checkers — those are checked AGAINST this file. TEST INFRASTRUCTURE
ONLY.

Layout: 64-byte header | n x 24-byte record header, zero-padded to 16 |
payload (key|value per record, each zero-padded to 16).
"""
OK, BAD_HEADER, BAD_SIZE, BAD_RECORD, BAD_LAYOUT, BAD_ORDER, BAD_SUM = range(7)
NO_INDEX = (1 << 64) - 1
M64 = (1 << 64) - 1
PUT = 1


def le(v, nbytes):
    return int(v).to_bytes(nbytes, "little")


def rd(buf, off, nbytes):
    return int.from_bytes(buf[off:off + nbytes], "little")


def fnv1a64(data):
    """FNV-1a-64 with the basis the store's record hash has always used
    (1469598103934665603, as orc_shard_checksum), for both sums."""
    h = 1469598103934665603
    for b in data:
        h ^= b
        h = (h * 0x100000001B3) & M64
    return h


def fnv1a32(data):
    h = 0x811C9DC5
    for b in data:
        h ^= b
        h = (h * 0x01000193) & 0xFFFFFFFF
    return h


def pad16(n):
    return -n % 16


def rec_hash(seq, typ, key, val):
    return fnv1a64(le(seq, 8) + le(typ, 1) + le(len(key), 4) +
                   le(len(val), 4) + key + val)


def header(merge_op, last_seq, n, payload_bytes, content_sum, version=1,
           magic=b"GRASHIMG", reserved=0):
    h = (magic + le(version, 4) + le(merge_op, 4) + le(last_seq, 8) +
         le(n, 8) + le(payload_bytes, 8) + le(content_sum, 8) +
         le(reserved, 8))
    assert len(h) == 56
    return h + le(fnv1a64(h), 8)


def rec_header(seq, kv_off, val_len, key_len, typ=PUT, flags=0, kpref=0):
    return (le(seq, 8) + le(kv_off, 4) + le(val_len, 4) + le(key_len, 2) +
            le(typ, 1) + le(flags, 1) + le(kpref, 4))


def pack(items, last_seq, merge_op):
    """items: [(stored_key, value, seq)] in ascending key order -> bytes."""
    heads = b""
    payload = b""
    total = 0
    for key, val, seq in items:
        heads += rec_header(seq, len(payload), len(val), len(key),
                            kpref=fnv1a32(key))
        payload += key + val + b"\x00" * pad16(len(key) + len(val))
        total = (total + rec_hash(seq, PUT, key, val)) & M64
    heads += b"\x00" * pad16(len(heads))
    return header(merge_op, last_seq, len(items), len(payload), total) + \
        heads + payload


def fields(img):
    """The header's fields, unchecked."""
    return dict(magic=img[:8], version=rd(img, 8, 4), merge_op=rd(img, 12, 4),
                last_seq=rd(img, 16, 8), n=rd(img, 24, 8),
                payload_bytes=rd(img, 32, 8), content_sum=rd(img, 40, 8),
                reserved=rd(img, 48, 8), header_sum=rd(img, 56, 8))


def entry(img, i):
    """Record header i, unchecked -> dict."""
    o = 64 + 24 * i
    return dict(seq=rd(img, o, 8), kv_off=rd(img, o + 8, 4),
                val_len=rd(img, o + 12, 4), key_len=rd(img, o + 16, 2),
                type=img[o + 18], flags=img[o + 19], kpref=rd(img, o + 20, 4))


def unpack(img):
    """A well-formed image -> (fields, [(key, value, seq)])."""
    f = fields(img)
    base = 64 + 24 * f["n"] + pad16(24 * f["n"])
    out = []
    for i in range(f["n"]):
        e = entry(img, i)
        k0 = base + e["kv_off"]
        v0 = k0 + e["key_len"]
        out.append((img[k0:v0], img[v0:v0 + e["val_len"]], e["seq"]))
    return f, out


def with_header_sum(img):
    """img with its header_sum recomputed (after a header field changed)."""
    return img[:56] + le(fnv1a64(img[:56]), 8) + img[64:]


def patch(img, off, data, fix_header=False):
    out = img[:off] + data + img[off + len(data):]
    return with_header_sum(out) if fix_header else out


def verdict(img):
    """The verdict rule -> (reason, bad_index)."""
    if len(img) < 64:
        return BAD_HEADER, NO_INDEX
    f = fields(img)
    if (f["magic"] != b"GRASHIMG" or f["version"] != 1 or
            f["header_sum"] != fnv1a64(img[:56]) or f["reserved"] != 0 or
            f["merge_op"] not in (0, 1)):
        return BAD_HEADER, NO_INDEX
    n, pb = f["n"], f["payload_bytes"]
    if n > 1 << 30 or pb % 16 or pb >= 1 << 32 or (n == 0 and pb):
        return BAD_SIZE, NO_INDEX
    base = 64 + 24 * n + pad16(24 * n)
    if len(img) != base + pb:
        return BAD_SIZE, NO_INDEX
    total = 0
    ents = [entry(img, i) for i in range(n)]

    def span(e):
        return e["key_len"] + e["val_len"]

    def inside(e):
        return e["kv_off"] + span(e) <= pb

    def key(e):
        return img[base + e["kv_off"]:base + e["kv_off"] + e["key_len"]]

    for i, e in enumerate(ents):
        if (e["type"] != PUT or e["flags"] != 0 or
                not 1 <= e["seq"] <= f["last_seq"] or
                e["val_len"] >= 0xFFFF0000):
            return BAD_RECORD, i
        want = 0
        if i:
            p = ents[i - 1]
            want = p["kv_off"] + span(p) + pad16(span(p))
        if (e["kv_off"] % 16 or e["kv_off"] != want or not inside(e) or
                (i == n - 1 and
                 e["kv_off"] + span(e) + pad16(span(e)) != pb)):
            return BAD_LAYOUT, i
        if i and inside(ents[i - 1]) and not key(ents[i - 1]) < key(e):
            return BAD_ORDER, i
        k = key(e)
        v0 = base + e["kv_off"] + e["key_len"]
        total = (total + rec_hash(e["seq"], PUT, k,
                                  img[v0:v0 + e["val_len"]])) & M64
    if total != f["content_sum"]:
        return BAD_SUM, NO_INDEX
    return OK, NO_INDEX


def items_from_model(model, merge_op):
    """What an image of a shard holds, from a fold_model.Model of its
    history: per live key, ascending, the folded value and the seq of the
    key's newest entry. -> [(key, value, seq)]"""
    out = []
    for k in model.keys():
        v = model.value(k, merge_op)
        if v is not None:
            out.append((k, v, model.ver[k][-1][0]))
    return out


# ---- the hostile table: one mutation each of a good image ----

def good_items(n, seed=5, seq0=1):
    """n entries, ascending 12-byte keys sharing 8 bytes, values of 0..40
    bytes, seqs a permutation-like spread within [seq0, seq0 + 3n)."""
    import random
    rng = random.Random(seed)
    out = []
    for i in range(n):
        key = b"IMGKEY__" + (2 * i + 2).to_bytes(4, "big")
        val = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 41)))
        out.append((key, val, seq0 + rng.randrange(3 * n)))
    return out


def set_entry(img, i, **kw):
    e = entry(img, i)
    e.update(kw)
    return patch(img, 64 + 24 * i,
                 rec_header(e["seq"], e["kv_off"], e["val_len"], e["key_len"],
                            e["type"], e["flags"], e["kpref"]))


def swap_keys(img, i):
    """Exchange the (equal-length) keys of entries i and i+1, content sum and
    header sum corrected: the only fault left is the order."""
    f, items = unpack(img)
    a, b = items[i], items[i + 1]
    assert len(a[0]) == len(b[0])
    items[i], items[i + 1] = (b[0], a[1], a[2]), (a[0], b[1], b[2])
    return pack(items, f["last_seq"], f["merge_op"])


def hostile_table(n=600):
    """-> (good image, [(name, image, header_level)]). Expected verdicts come
    from verdict(); header_level cases must be refused before any launch."""
    items = good_items(n)
    last_seq = 4 * n
    good = pack(items, last_seq, 0)
    f = fields(good)
    pb = f["payload_bytes"]
    base = 64 + 24 * n + pad16(24 * n)
    mid = n // 2
    cases = []

    def add(name, img, header_level=False):
        cases.append((name, img, header_level))

    add("wrong magic", patch(good, 0, b"GRASHIMX", True), True)
    add("wrong header_sum", patch(good, 56, le(f["header_sum"] ^ 1, 8)), True)
    add("one byte short", good[:-1], True)
    add("one byte long", good + b"\x00", True)
    add("n_entries inflated", patch(good, 24, le(n + 1, 8), True), True)
    add("kv_off = 0xFFFFFFF0", set_entry(good, mid, kv_off=0xFFFFFFF0))
    add("kv_off off by 8",
        set_entry(good, mid, kv_off=entry(good, mid)["kv_off"] + 8))
    add("key_len past the payload", set_entry(good, n - 1, key_len=0xFFFF))
    add("val_len = 0xFFFFFFFF", set_entry(good, mid, val_len=0xFFFFFFFF))
    # a gap: 16 zero bytes in front of record mid, later offsets shifted
    gap = good[:base + entry(good, mid)["kv_off"]] + b"\x00" * 16 + \
        good[base + entry(good, mid)["kv_off"]:]
    for i in range(mid, n):
        gap = set_entry(gap, i, kv_off=entry(gap, i)["kv_off"] + 16)
    add("gap in the dense layout", patch(gap, 32, le(pb + 16, 8), True))
    add("type = Delete", set_entry(good, mid, type=0))
    add("flags = 1", set_entry(good, mid, flags=1))
    add("seq 0", set_entry(good, mid, seq=0))
    add("seq = last_seq + 1", set_entry(good, mid, seq=last_seq + 1))
    # two equal adjacent keys: entry mid+1 takes entry mid's key
    _, its = unpack(good)
    its[mid + 1] = (its[mid][0], its[mid + 1][1], its[mid + 1][2])
    add("equal adjacent keys", pack(its, last_seq, 0))
    for i in (63, 255, 256):
        add(f"descending pair {i}/{i + 1}", swap_keys(good, i))
    # a proper prefix of its predecessor
    _, its = unpack(good)
    its[mid] = (its[mid - 1][0][:-2], its[mid][1], its[mid][2])
    add("key a prefix of its predecessor", pack(its, last_seq, 0))
    # one flipped value byte (entry 0 may have an empty value: find one)
    j = next(i for i in range(n) if entry(good, i)["val_len"])
    e = entry(good, j)
    at = base + e["kv_off"] + e["key_len"]
    add("one flipped value byte", patch(good, at, bytes([good[at] ^ 0x40])))
    add("content_sum + 1",
        patch(good, 40, le((f["content_sum"] + 1) & M64, 8), True))
    # order at 101, record at 37 and at 400: entry 37 decides
    two = set_entry(set_entry(swap_keys(good, 100), 400, flags=1), 37, seq=0)
    add("two faults, the lower index wins", two)
    return good, cases
