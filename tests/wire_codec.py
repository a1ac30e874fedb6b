"""numpy restatement of the compressed wire (raymarching_amd/csrc/rm_wire_tile.h,
rm_wire.hip): the byte-exact message layout the GPU encoders write (rows
encoder and render epilogue), and its decoder.  Test helper for
tests/test_wire.py (the codec is this build's own format; the reference sends
no frames between processes).

A part of n packed RGBA8 rows of W pixels in 8x8 tiles (TX = ceil(W/8) across,
TY = ceil(n/8) down, tile t = ty TX + tx; pixels outside the part are the word
0).  Per tile and channel: differences to the left neighbour, to the one above
in the first column, mod 256 as int8, zig-zagged; the width b of the largest;
the header word (lane 0's RGB, b_R << 24, b_G << 28, b_B << 32) and b bit planes
per channel (bit l = lane (l & 7, l >> 3)).  Message: int64 bytes, uint32 per
tile (word offset << 5 | word count), padded to 8 B, then the tiles' words in
order."""
import numpy as np

TILE_WORDS = 25


def _zigzag(d):
    s = ((d & 255).astype(np.int16) ^ 128) - 128  # int8 wrap
    return np.where(s >= 0, 2 * s, -2 * s - 1).astype(np.uint32)


def header_bytes(T):
    return 8 + ((4 * T + 7) & ~7)


def _tiles(rows):
    n, W = rows.shape
    TX, TY = (W + 7) // 8, (n + 7) // 8
    pad = np.zeros((TY * 8, TX * 8), np.uint32)
    pad[:n, :W] = rows
    return pad.reshape(TY, 8, TX, 8).transpose(0, 2, 1, 3).reshape(TY * TX, 64), TX, TY


def tile_words(p):
    """The words of one tile: p = uint32 [64] RGBA8, lane l = (col l & 7, row l >> 3)."""
    planes, bs = [], []
    for c in range(3):
        v = ((p >> (8 * c)) & 255).astype(np.int32).reshape(8, 8)
        ref = np.empty_like(v)
        ref[:, 1:] = v[:, :-1]
        ref[1:, 0] = v[:-1, 0]
        ref[0, 0] = v[0, 0]
        z = _zigzag((v - ref).ravel())
        z[0] = 0
        b = int(z.max()).bit_length()
        bs.append(b)
        for i in range(b):
            bits = ((z >> i) & 1).astype(np.uint64)
            planes.append(int(np.sum(bits << np.arange(64, dtype=np.uint64))))
    hdr = (int(p[0]) & 0xFFFFFF) | (bs[0] << 24) | (bs[1] << 28) | (bs[2] << 32)
    return [hdr] + planes


def encode(rows):
    """rows: uint32 [n, W] RGBA8 words -> message bytes (uint8 array)."""
    rows = np.ascontiguousarray(rows, np.uint32)
    tiles, TX, TY = _tiles(rows)
    T = TX * TY
    words = [tile_words(tiles[t]) for t in range(T)]
    counts = np.array([len(w) for w in words], np.int64)
    offs = (np.concatenate([[0], np.cumsum(counts)[:-1]]) if T else np.zeros(0)).astype(np.int64)
    table = ((offs << 5) | counts).astype(np.uint32)
    hb = header_bytes(T)
    total = int(counts.sum())
    out = np.zeros(hb + 8 * total, np.uint8)
    out[:8] = np.frombuffer(np.array([hb + 8 * total], np.int64).tobytes(), np.uint8)
    out[8:8 + 4 * T] = np.frombuffer(table.tobytes(), np.uint8)
    flat = np.array([x for w in words for x in w], np.uint64)
    out[hb:] = np.frombuffer(flat.tobytes(), np.uint8)
    return out


_BIT_LENGTH = np.array([int(v).bit_length() for v in range(256)], np.int64)


def encode_fast(rows):
    """encode(rows), byte for byte, in whole-array numpy: `encode` above is the
    specification, this is the same format fast enough for parts of 10^5 tiles
    (tests/test_wire.py pins the two together)."""
    rows = np.ascontiguousarray(rows, np.uint32)
    tiles, TX, TY = _tiles(rows)
    T = TX * TY
    bs, planes = [], []  # per channel: the widths [T]; per (channel, bit): the plane words [T]
    for c in range(3):
        v = ((tiles >> np.uint32(8 * c)) & np.uint32(255)).astype(np.int16).reshape(T, 8, 8)
        ref = np.empty_like(v)
        ref[:, :, 1:] = v[:, :, :-1]
        ref[:, 1:, 0] = v[:, :-1, 0]
        ref[:, 0, 0] = v[:, 0, 0]
        s = (((v - ref) & 255) ^ 128) - 128  # int8 wrap
        z = np.where(s >= 0, 2 * s, -2 * s - 1).astype(np.uint8).reshape(T, 64)
        z[:, 0] = 0
        bs.append(_BIT_LENGTH[z.max(axis=1)] if T else np.zeros(0, np.int64))
        # bit i of the 64 lanes as one little-endian word: lane l is bit l
        planes.append([np.packbits((z >> i) & 1, axis=1, bitorder="little").view("<u8").reshape(T)
                       for i in range(8)])
    counts = 1 + bs[0] + bs[1] + bs[2]
    offs = np.cumsum(counts) - counts
    total = int(counts.sum())
    flat = np.zeros(total, np.uint64)
    flat[offs] = ((tiles[:, 0] & np.uint32(0xFFFFFF)).astype(np.uint64) | (bs[0].astype(np.uint64) << np.uint64(24)) |
                  (bs[1].astype(np.uint64) << np.uint64(28)) | (bs[2].astype(np.uint64) << np.uint64(32)))
    first = offs + 1  # the channel's first plane word
    for c in range(3):
        for i in range(8):
            has = bs[c] > i
            flat[first[has] + i] = planes[c][i][has]
        first = first + bs[c]
    hb = header_bytes(T)
    out = np.zeros(hb + 8 * total, np.uint8)
    out[:8] = np.frombuffer(np.array([hb + 8 * total], np.int64).tobytes(), np.uint8)
    out[8:8 + 4 * T] = np.frombuffer(((offs << 5) | counts).astype(np.uint32).tobytes(), np.uint8)
    out[hb:] = np.frombuffer(flat.astype("<u8").tobytes(), np.uint8)
    return out


def first_difference(got, ref, T):
    """Where two messages of a T-tile part first differ, in a line (None when
    equal): the size word, the first differing table entry, or the first
    differing payload word and the tile of `ref` that owns it."""
    got, ref = np.asarray(got, np.uint8), np.asarray(ref, np.uint8)
    if got.size == ref.size and np.array_equal(got, ref):
        return None
    hb = header_bytes(T)
    if min(got.size, ref.size) < hb:
        return f"sizes {got.size} != {ref.size}: shorter than the {hb}-byte header of {T} tiles"
    size = [int(np.frombuffer(m[:8].tobytes(), np.int64)[0]) for m in (got, ref)]
    tab = [np.frombuffer(m[8:8 + 4 * T].tobytes(), np.uint32) for m in (got, ref)]
    at = np.flatnonzero(tab[0] != tab[1])
    if at.size:
        t = int(at[0])
        return (f"table: tile {t} of {T} is offset {int(tab[0][t]) >> 5} count {int(tab[0][t]) & 31}, expected offset "
                f"{int(tab[1][t]) >> 5} count {int(tab[1][t]) & 31} ({at.size} entries differ; size words {size[0]}, "
                f"expected {size[1]})")
    k = (min(got.size, ref.size) - hb) & ~7
    pay = [np.frombuffer(m[hb:hb + k].tobytes(), np.uint64) for m in (got, ref)]
    at = np.flatnonzero(pay[0] != pay[1])
    if at.size:
        w = int(at[0])
        t = int(np.searchsorted(tab[1] >> 5, w, side="right")) - 1
        return (f"payload: word {w} (tile {t} of {T}, its word {w - (int(tab[1][t]) >> 5)}) is {int(pay[0][w]):#018x}, "
                f"expected {int(pay[1][w]):#018x} ({at.size} words differ)")
    return f"sizes {got.size} != {ref.size} (size words {size[0]}, expected {size[1]}); equal up to the shorter"


def decode(msg, n, W):
    """message -> uint32 [n, W] RGBA8 words (alpha 255)."""
    msg = np.asarray(msg, np.uint8)
    TX, TY = (W + 7) // 8, (n + 7) // 8
    T = TX * TY
    hb = header_bytes(T)
    offs = np.frombuffer(msg[8:8 + 4 * T].tobytes(), np.uint32) >> 5
    payload = np.frombuffer(msg[hb:].tobytes(), np.uint64)
    out = np.zeros((TY * 8, TX * 8), np.uint32)
    lanes = np.arange(64, dtype=np.uint64)
    for t in range(T):
        w = payload[int(offs[t]):]
        h = int(w[0])
        bs = [(h >> 24) & 15, (h >> 28) & 15, (h >> 32) & 15]
        q = 1
        px = np.zeros(64, np.uint32)
        for c in range(3):
            z = np.zeros(64, np.uint32)
            for i in range(bs[c]):
                z |= (((np.uint64(w[q]) >> lanes) & np.uint64(1)).astype(np.uint32)) << np.uint32(i)
                q += 1
            d = ((z >> 1).astype(np.int64) ^ -(z & 1).astype(np.int64)).reshape(8, 8)
            d[0, 0] = (h >> (8 * c)) & 255
            v = np.cumsum(d, axis=1) + (np.cumsum(d[:, 0]) - d[:, 0])[:, None]
            px |= ((v.ravel() & 255).astype(np.uint32)) << np.uint32(8 * c)
        ty, tx = divmod(t, TX)
        out[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8] = (px | np.uint32(0xFF000000)).reshape(8, 8)
    return out[:n, :W]
