"""Pure-Python Snappy raw-block tools: an element-level encoder, an element
iterator and an independent decoder, written from the public format
description (format_description.txt of the Snappy project). TEST
INFRASTRUCTURE ONLY.

Format: varint32 uncompressed length, then elements tagged by the low two
bits of their first byte:
  00 literal: len-1 in bits 2..7 when < 60; 60..63 there mean that len-1
     follows in 1..4 little-endian bytes
  01 copy, len-4 in bits 2..4 (len 4..11), offset = bits 5..7 << 8 | next byte
  10 copy, len-1 in bits 2..7 (len 1..64), 2-byte little-endian offset
  11 copy, len-1 in bits 2..7 (len 1..64), 4-byte little-endian offset
A copy reads `len` bytes starting `offset` bytes behind the write position,
byte by byte, so offset < len repeats a pattern.

The encoder builds a stream from an explicit element list, so a test picks
every tag. `check=False` lets a test write operands the format forbids.
The decoder works in Python integers: nothing can wrap.
"""
from collections import namedtuple


def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


# ---------------------------------------------------------------- encoder

def literal_header(n, ext=None):
    """Tag (+ length bytes) of a literal of n bytes. ext=None picks the
    canonical form; ext=0 forces the inline form, 1..4 that many length
    bytes (non-canonical forms are legal)."""
    assert n >= 1
    if ext is None:
        ext = 0 if n <= 60 else (n - 1).bit_length() + 7 >> 3
    if ext == 0:
        assert n <= 60
        return bytes([(n - 1) << 2])
    assert 1 <= ext <= 4 and n - 1 < 1 << (8 * ext)
    return bytes([(59 + ext) << 2]) + (n - 1).to_bytes(ext, "little")


def literal(data, ext=None):
    return literal_header(len(data), ext) + bytes(data)


def copy1(off, n, check=True):
    if check:
        assert 4 <= n <= 11 and 0 < off < 2048
    return bytes([1 | ((n - 4) & 7) << 2 | (off >> 8 & 7) << 5, off & 0xFF])


def copy2(off, n, check=True):
    if check:
        assert 1 <= n <= 64 and 0 < off < 1 << 16
    return bytes([2 | ((n - 1) & 63) << 2]) + (off & 0xFFFF).to_bytes(2, "little")


def copy4(off, n, check=True):
    if check:
        assert 1 <= n <= 64 and 0 < off < 1 << 32
    return bytes([3 | ((n - 1) & 63) << 2]) + (off & 0xFFFFFFFF).to_bytes(4, "little")


COPY = {"copy1": copy1, "copy2": copy2, "copy4": copy4}


def stream(ulen, elements):
    return varint(ulen) + b"".join(elements)


# ------------------------------------------------------- parser / decoder

Element = namedtuple("Element", "kind off len ext pos")
"""kind: 'lit', 'copy1', 'copy2', 'copy4'; off: copy offset (0 for a
literal); len: bytes produced; ext: a literal's extra length bytes (0 for a
copy); pos: index of the tag byte in the stream."""


def read_varint32(buf, pos=0):
    """-> (value, next pos) or None. At most 5 bytes, value below 2^32."""
    v = 0
    for i in range(5):
        if pos + i >= len(buf):
            return None
        b = buf[pos + i]
        v |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            return (v, pos + i + 1) if v < 1 << 32 else None
    return None


def _walk(buf, cap):
    """Shared by elements() and decode(): yields ('hdr', ulen), then one
    (Element, payload position) per element, then ('end', ok)."""
    hdr = read_varint32(buf)
    if hdr is None or hdr[0] > cap:
        yield "end", False
        return
    ulen, ip = hdr
    yield "hdr", ulen
    op = 0
    while ip < len(buf):
        pos = ip
        tag = buf[ip]
        ip += 1
        kind = tag & 3
        if kind == 0:
            n, ext = (tag >> 2) + 1, 0
            if n > 60:
                ext = n - 60
                if ip + ext > len(buf):
                    yield "end", False
                    return
                n = int.from_bytes(buf[ip:ip + ext], "little") + 1
                ip += ext
            if ip + n > len(buf) or op + n > ulen:
                yield "end", False
                return
            yield Element("lit", 0, n, ext, pos), ip
            ip += n
        else:
            if kind == 1:
                n, width = (tag >> 2 & 7) + 4, 1
            else:
                n, width = (tag >> 2) + 1, 2 if kind == 2 else 4
            if ip + width > len(buf):
                yield "end", False
                return
            off = int.from_bytes(buf[ip:ip + width], "little")
            if kind == 1:
                off |= (tag >> 5) << 8
            ip += width
            if off == 0 or off > op or op + n > ulen:
                yield "end", False
                return
            yield Element(("copy1", "copy2", "copy4")[kind - 1], off, n, 0, pos), ip
        op += n
    yield "end", op == ulen


def elements(buf, cap=1 << 32):
    """The well-formed elements of a stream, in order; stops without an
    error at the first one that a decoder would reject."""
    for item, where in _walk(bytes(buf), cap):
        if isinstance(item, Element):
            yield item


def decode(buf, cap):
    """Uncompressed bytes, or None where the format (or cap) rejects."""
    buf = bytes(buf)
    out = bytearray()
    for item, where in _walk(buf, cap):
        if item == "end":
            return bytes(out) if where else None
        if item == "hdr":
            continue
        if item.kind == "lit":
            out += buf[where:where + item.len]
        else:
            for _ in range(item.len):  # byte by byte: overlap repeats
                out.append(out[-item.off])
    return None


# ------------------------------------------------------- greedy re-encoder

class Policy:
    """Knobs of encode_with. copy_kind is the preferred copy element
    ('copy1', 'copy2', 'copy4', or None for literals only); a match that the
    preferred kind cannot hold falls back to the next wider one."""

    def __init__(self, copy_kind="copy2", max_copy_len=64, lit_split=None,
                 min_dist=1, max_dist=65535, lit_ext=None):
        self.copy_kind = copy_kind
        self.max_copy_len = max_copy_len
        self.lit_split = lit_split
        self.min_dist = min_dist
        self.max_dist = max_dist
        self.lit_ext = lit_ext


def _emit_copy(kind, off, n):
    if kind == "copy1" and (off >= 2048 or not 4 <= n <= 11):
        kind = "copy2"
    if kind == "copy2" and off >= 1 << 16:
        kind = "copy4"
    return COPY[kind](off, n)


def encode_with(data, policy):
    """Re-express `data` as a valid stream under `policy` (greedy: at each
    position the longest match among earlier positions with the same four
    bytes, nearest first on ties)."""
    data = bytes(data)
    els, seen, lit_from, pos = [], {}, 0, 0
    p = policy
    max_len = min(p.max_copy_len, 11 if p.copy_kind == "copy1" else 64)

    def flush(upto):
        i = lit_from
        while i < upto:
            n = min(upto - i, p.lit_split or upto - i)
            ext = p.lit_ext
            if ext == 0 and n > 60 or ext and n - 1 >= 1 << (8 * ext):
                ext = None  # the forced form cannot hold this length
            els.append(literal(data[i:i + n], ext))
            i += n

    while pos < len(data):
        best_n, best_off = 0, 0
        key = data[pos:pos + 4]
        if p.copy_kind and len(key) == 4:
            for cand in reversed(seen.get(key, ())):
                off = pos - cand
                if off > p.max_dist:
                    break
                if off < p.min_dist:
                    continue
                n = 4
                while (n < max_len and pos + n < len(data)
                       and data[cand + n] == data[pos + n]):
                    n += 1
                if n > best_n and n <= max_len:
                    best_n, best_off = n, off
        if best_n >= 4:
            flush(pos)
            els.append(_emit_copy(p.copy_kind, best_off, best_n))
            step = best_n
        else:
            step = 1
        for q in range(pos, pos + step):
            if q + 4 <= len(data):
                seen.setdefault(data[q:q + 4], []).append(q)
        pos += step
        if best_n >= 4:
            lit_from = pos
    flush(len(data))
    return stream(len(data), els)
