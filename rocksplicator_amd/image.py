"""Shard images in pure Python: the offline writer behind the bulk-load case
(≅ building SST files offline for addS3SstFilesToDB, admin_handler.cpp:1635)
and a reader for tools. No GPU and no libgra.so needed.

The format (version 1) is documented in include/rocksplicator_gpu.h: a
64-byte header, n 24-byte record headers padded to 16 B, then the records —
key then value, each padded with zeros to 16 B — one Put per key, strictly
ascending by stored key ([cf LE4 | key] for a column family). An image
written here is installed with Db.import_image like an exported one.
"""
import struct

MAGIC = b"GRASHIMG"
VERSION = 1
HEADER_BYTES = 64
MAX_ENTRIES = 1 << 30
_MASK64 = (1 << 64) - 1
_PUT = 1
_HDR = struct.Struct("<8sIIQQQQQ")  # bytes 0..55; header_sum follows
_REC = struct.Struct("<QIIHBBI")    # wb::RecHdr, 24 B


def _fnv64(data, h=1469598103934665603):
    for b in data:
        h = ((h ^ b) * 1099511628211) & _MASK64
    return h


def _fnv32(data):
    h = 2166136261
    for b in data:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def _align16(n):
    return (n + 15) & ~15


def pack_image(sorted_items, last_seq, merge_op):
    """-> bytes. sorted_items: (stored_key, value, seq) triples, or
    (stored_key, value) pairs that all get seq = last_seq, strictly
    ascending by key; values are final (nothing is left to fold), merge_op
    names the operator the target engine runs. Raises ValueError on
    anything the importer would reject."""
    if merge_op not in (0, 1):
        raise ValueError("merge_op must be 0 (concat) or 1 (u64add)")
    hdrs, pay = bytearray(), bytearray()
    total, prev, n = 0, None, 0
    for item in sorted_items:
        key, val = bytes(item[0]), bytes(item[1])
        seq = item[2] if len(item) > 2 else last_seq
        if prev is not None and not prev < key:
            raise ValueError(f"keys must be strictly ascending at entry {n}")
        if not 1 <= seq <= last_seq:
            raise ValueError(f"seq out of [1, last_seq] at entry {n}")
        if len(key) > 0xFFFF or len(val) >= 0xFFFF0000:
            raise ValueError(f"key or value too long at entry {n}")
        hdrs += _REC.pack(seq, len(pay), len(val), len(key), _PUT, 0,
                          _fnv32(key))
        rec = key + val
        total = (total + _fnv64(
            struct.pack("<QBII", seq, _PUT, len(key), len(val)) + rec)) & _MASK64
        pay += rec + bytes(_align16(len(rec)) - len(rec))
        prev = key
        n += 1
    if n > MAX_ENTRIES or len(pay) >= 1 << 32:
        raise ValueError("image too large (2^30 entries, 4 GiB of records)")
    hdrs += bytes(_align16(len(hdrs)) - len(hdrs))
    head = _HDR.pack(MAGIC, VERSION, merge_op, last_seq, n, len(pay), total, 0)
    return head + struct.pack("<Q", _fnv64(head)) + bytes(hdrs) + bytes(pay)


def unpack_image(image):
    """-> dict(version, merge_op, last_seq, content_sum, items) with items =
    [(stored_key, value, seq)]. Reads a well-formed image (run
    rocksplicator_amd.image_check on untrusted bytes first); raises
    ValueError when the header or the sizes are off."""
    image = bytes(image)
    if len(image) < HEADER_BYTES or image[:8] != MAGIC:
        raise ValueError("not a shard image")
    (_, version, merge_op, last_seq, n, payload_bytes, content_sum,
     reserved) = _HDR.unpack_from(image)
    (header_sum,) = struct.unpack_from("<Q", image, 56)
    if version != VERSION or reserved or header_sum != _fnv64(image[:56]):
        raise ValueError("bad image header")
    pay0 = HEADER_BYTES + _align16(24 * n)
    if n > MAX_ENTRIES or len(image) != pay0 + payload_bytes:
        raise ValueError("image size does not match its header")
    items = []
    for i in range(n):
        seq, kv_off, vlen, klen, _, _, _ = _REC.unpack_from(
            image, HEADER_BYTES + 24 * i)
        if kv_off + klen + vlen > payload_bytes:
            raise ValueError(f"entry {i} leaves the payload")
        k0 = pay0 + kv_off
        items.append((image[k0:k0 + klen], image[k0 + klen:k0 + klen + vlen],
                      seq))
    return dict(version=version, merge_op=merge_op, last_seq=last_seq,
                content_sum=content_sum, items=items)
