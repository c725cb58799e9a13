"""The PNG encoder of csrc/png_encode.hip restated in Python: encode_ref defines the format byte for byte (filter choice, bands,
Huffman tables, header bits, Adler-32), and the case list feeds tests/test_png_encode_cases_cpu.py (which pins encode_ref to zlib,
flow_io.read_png and PIL) and tests/test_gpu_png_encode.py (device bytes == encode_ref).  Written from RFC 1950 / 1951 and the PNG
specification, section 9 and 12.8 (the minimum-sum-of-absolute-differences heuristic); integers only.

A stream is `78 01`, one dynamic-Huffman block per band of BAND_ROWS scanlines (literals and end-of-block only), the Adler-32.
Tables of one block, from the band's byte histogram (plus one end-of-block):
  1. the used symbols sorted by (frequency, symbol);
  2. Huffman's algorithm on two queues (sorted leaves, created nodes in creation order); a leaf is taken when its weight is <= the
     front node's;
  3. the number of leaves per depth, depths above the limit counted at the limit; while the Kraft sum exceeds 1: one code leaves
     the limit and one code of the deepest shorter length becomes two codes one bit longer (each step lowers the sum by 2^-limit);
  4. the lengths handed out along the sorted order, longest first;  5. canonical codes.
If the literal table would cost more than the fixed table FALLBACK (8 bits for 0 .. 254, 9 for 255 and end-of-block) it is replaced
by it: hence at most 9 N + 9 bits for a band of N bytes.  The block header always carries 19 code-length code lengths, 257 literal
lengths and two distance lengths of 1, each length sent as its own code-length symbol (no repeat codes 16 .. 18)."""
import zlib

import numpy as np

from tests.png_cases import header_constant

BAND_ROWS = 32
BPPS = (1, 2, 3, 4, 6, 8)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FALLBACK = [8] * 255 + [9, 9]
HEADER_BITS_MAX = 17 + 19 * 3 + 259 * 7           # fixed fields, code-length code lengths, 259 lengths of at most 7 bits


def memory_bytes(img):
    """[h, w, c] uint8 / uint16 -> (uint8 [h, w * bpp] as the array lies in memory (host order), bpp, swap16)."""
    a = np.ascontiguousarray(img)
    assert a.ndim == 3 and a.dtype in (np.uint8, np.uint16)
    return a.view(np.uint8).reshape(a.shape[0], -1), a.shape[2] * a.dtype.itemsize, a.dtype == np.uint16


def candidates(rows, bpp):
    """The five filtered versions [5, h, stride] of rows [h, stride] (file byte order)."""
    cur = rows.astype(np.int32)
    h, stride = cur.shape
    b = np.zeros_like(cur)
    b[1:] = cur[:-1]
    a, c = np.zeros_like(cur), np.zeros_like(cur)
    if stride > bpp:
        a[:, bpp:] = cur[:, :-bpp]
        c[:, bpp:] = b[:, :-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([(cur - pred) & 255 for pred in (0, a, b, (a + b) >> 1, paeth)]).astype(np.uint8)


def scanlines(mem, bpp, swap16):
    """Memory bytes [h, w * bpp] -> uint8 [h, 1 + w * bpp]: each row behind the filter type with the smallest sum of min(v, 256 - v)
    over its filtered bytes; ties go to the lowest type (np.argmin returns the first minimum)."""
    rows = mem.reshape(mem.shape[0], -1, 2)[:, :, ::-1].reshape(mem.shape) if swap16 else mem
    cand = candidates(rows, bpp)
    cost = np.minimum(cand.astype(np.int64), 256 - cand.astype(np.int64)).sum(axis=2)          # [5, h]
    ft = np.argmin(cost, axis=0)
    chosen = cand[ft, np.arange(rows.shape[0])]
    return np.concatenate([ft.astype(np.uint8)[:, None], chosen], axis=1)


def huffman_lengths(freq, limit):
    """freq[s] >= 0 -> (lengths[s] (0: unused), the deepest leaf before the limit was applied).  At least two symbols are used."""
    order = sorted((f, s) for s, f in enumerate(freq) if f > 0)
    n = len(order)
    assert n >= 2
    w = [f for f, _ in order] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    i, j = 0, n
    for k in range(n, 2 * n - 1):
        for _ in range(2):
            if i < n and (j >= k or w[i] <= w[j]):
                parent[i], i = k, i + 1
                w[k] += w[i - 1]
            else:
                parent[j], j = k, j + 1
                w[k] += w[j - 1]
    depth = [0] * (2 * n - 1)
    for m in range(2 * n - 3, -1, -1):
        depth[m] = depth[parent[m]] + 1
    count = [0] * (limit + 1)
    for m in range(n):
        count[min(depth[m], limit)] += 1
    total = sum(count[l] << (limit - l) for l in range(1, limit + 1))
    while total > (1 << limit):
        count[limit] -= 1
        l = limit - 1
        while count[l] == 0:
            l -= 1
        count[l] -= 1
        count[l + 1] += 2
        total -= 1
    assert total == 1 << limit
    lengths = [0] * len(freq)
    r = 0
    for l in range(limit, 0, -1):
        for _ in range(count[l]):
            lengths[order[r][1]] = l
            r += 1
    return lengths, max(depth[:n])


def canonical_codes(lengths):
    """RFC 1951 3.2.2, bit-reversed: the codes as they enter the LSB-first bit stream."""
    top = max(lengths)
    count = [0] * (top + 2)
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * (top + 2), 0
    for l in range(1, top + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        c = 0
        if l:
            c = int(format(nxt[l], "0%db" % l)[::-1], 2)
            nxt[l] += 1
        out.append(c)
    return out


def band_tables(hist):
    """hist [256] of a band's bytes -> (literal lengths [257], code-length code lengths [19], deepest literal leaf, fallback?)."""
    freq = [int(x) for x in hist] + [1]
    lit, deepest = huffman_lengths(freq, 15)
    fallback = sum(f * l for f, l in zip(freq, lit)) > sum(f * l for f, l in zip(freq, FALLBACK))
    if fallback:
        lit = list(FALLBACK)
    clfreq = [0] * 19
    for l in lit + [1, 1]:
        clfreq[l] += 1
    cl, _ = huffman_lengths(clfreq, 7)
    return lit, cl, deepest, fallback


def band_items(band, final):
    """-> (codes, lengths) of every item of one block in stream order: uint32 arrays."""
    flat = band.reshape(-1)
    lit, cl, _, _ = band_tables(np.bincount(flat, minlength=256))
    litc, clc = canonical_codes(lit), canonical_codes(cl)
    codes = [(1 if final else 0) | (2 << 1) | (0 << 3) | (1 << 8) | (15 << 13)] + [cl[s] for s in CL_ORDER]
    lens = [17] + [3] * 19
    for l in lit + [1, 1]:
        codes.append(clc[l])
        lens.append(cl[l])
    litc, lit = np.asarray(litc, np.uint32), np.asarray(lit, np.uint32)
    return (np.concatenate([np.asarray(codes, np.uint32), litc[flat], litc[256:]]),
            np.concatenate([np.asarray(lens, np.uint32), lit[flat], lit[256:]]))


def deflate_ref(scan):
    """Scanlines uint8 [h, line] -> the zlib stream."""
    h = scan.shape[0]
    parts = [band_items(scan[y:y + BAND_ROWS], y + BAND_ROWS >= h) for y in range(0, h, BAND_ROWS)]
    codes, lens = np.concatenate([p[0] for p in parts]).astype(np.int64), np.concatenate([p[1] for p in parts]).astype(np.int64)
    start = np.cumsum(lens) - lens
    nbits = int(lens.sum())
    bits = np.zeros(-(-nbits // 8) * 8, np.uint8)
    for k in range(17):
        on = (lens > k) & ((codes >> k) & 1 == 1)
        bits[start[on] + k] = 1
    body = np.packbits(bits, bitorder="little").tobytes()
    return b"\x78\x01" + body + (zlib.adler32(scan.tobytes()) & 0xFFFFFFFF).to_bytes(4, "big")


def encode_ref(img, swap16=None):
    """[h, w, c] uint8 / uint16 (swap16 defaults to: 16-bit samples), or uint8 memory bytes [h, w, bpp] with an explicit swap16 ->
    the zlib stream sf_png_encode must produce."""
    mem, bpp, s16 = memory_bytes(img)
    return deflate_ref(scanlines(mem, bpp, s16 if swap16 is None else swap16))


def bound(h, w, bpp):
    """sf_png_encode_bound: 2 + the blocks + 4, rounded up to 4; a block of N bytes has at most HEADER_BITS_MAX + 9 N + 9 bits."""
    nb = -(-h // BAND_ROWS)
    bits = nb * (HEADER_BITS_MAX + 9) + 9 * h * (1 + w * bpp)
    return (2 + -(-bits // 8) + 4 + 3) // 4 * 4


def kitti16_ref(flow):
    """[2, h, w] float32 -> uint16 [h, w, 3] as sf_flow_to_kitti16 states it (NaN and values below 0 -> 0, above 65535 -> 65535)."""
    f = np.asarray(flow, np.float32)
    v = (np.float32(64.0) * f).astype(np.float32) + np.float32(32768.0)
    v = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(0), np.float32(65535)))
    out = np.ones(f.shape[1:] + (3,), np.uint16)
    out[:, :, 0], out[:, :, 1] = v[0].astype(np.uint16), v[1].astype(np.uint16)
    return out


# ---- images ---------------------------------------------------------------------------------------------------------------------
def smooth_field(h, w, seed):
    """A smooth flow field [2, h, w] float32: low-frequency waves plus a little noise (what the measurements of DESIGN.md 9.7 use)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u = 9 * np.sin(x / 97.0 + 0.3) * np.cos(y / 61.0) + 4 * np.sin((x + y) / 29.0) + x / 200.0
    v = 7 * np.cos(x / 83.0) * np.sin(y / 71.0 + 0.9) - 3 * np.cos((x - 2 * y) / 37.0) + y / 150.0
    return (np.stack([u, v]) + rng.normal(0, 0.02, size=(2, h, w))).astype(np.float32)


def wheel_rgb(flow):
    """A host-side stand-in for the colour wheel (smooth in the flow, 8-bit RGB): angle -> hue, radius -> saturation."""
    u, v = flow[0].astype(np.float64), flow[1].astype(np.float64)
    rad = np.sqrt(u * u + v * v)
    rad = rad / max(rad.max(), 1e-9)
    ang = np.arctan2(-v, -u)
    rgb = np.stack([0.5 + 0.5 * np.cos(ang + k * 2 * np.pi / 3) for k in range(3)], axis=-1)
    return np.floor(255 * (1 - rad[..., None] * (1 - rgb))).astype(np.uint8)


def fibonacci_band(seed=0):
    """uint8 [32, 150, 1]: byte frequencies 1, 2, 3, 5, ... 1597 (with the end-of-block's 1 a Fibonacci sequence of 17 terms, sum
    4180) on values of small magnitude, the remaining 620 bytes on value 0, shuffled: rows of noise, which filter type 0 encodes
    cheapest, so the band's histogram is this one and the unlimited Huffman tree is 16 deep."""
    fib = [1, 2]
    while len(fib) < 16:
        fib.append(fib[-1] + fib[-2])
    values = [8, 249, 7, 250, 6, 251, 5, 252, 4, 253, 3, 254, 2, 255, 1, 0]
    data = np.concatenate([np.full(f, v, np.uint8) for f, v in zip(fib, values)] + [np.zeros(32 * 150 - sum(fib), np.uint8)])
    np.random.default_rng(seed).shuffle(data)
    return data.reshape(32, 150, 1)


def make(kind, h, w, bpp, seed):
    """Memory bytes uint8 [h, w, bpp]."""
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return np.zeros((h, w, bpp), np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w, bpp), dtype=np.uint8)
    if kind == "fib":
        assert (h, w, bpp) == (32, 150, 1)
        return fibonacci_band(seed)
    assert kind == "smooth"                      # gradients with a little noise: every filter type wins some rows
    y, x, k = np.mgrid[0:h, 0:w, 0:bpp]
    a = 3 * x + 5 * y * (y % 3) + 40 * k + (x * y) // 7 + rng.integers(0, 3, size=(h, w, bpp))
    a[h // 2:] = a[h // 2:] // 2 + rng.integers(0, 2, size=a[h // 2:].shape) * 8
    return (a & 255).astype(np.uint8)


# (kind, h, w, bpp, swap16, seed): band edges (h 1, 31, 32, 33, 65) against row lengths w * bpp around 1, 64, 256 and 1025, every bpp,
# swap16, the single-symbol block, the length limit, noise
CASES = [("smooth", 1, 1, 1, 0, 1), ("smooth", 31, 63, 1, 0, 2), ("smooth", 32, 64, 1, 0, 3), ("smooth", 33, 65, 1, 0, 4),
         ("smooth", 65, 255, 1, 0, 5), ("smooth", 1, 256, 1, 0, 6), ("smooth", 31, 257, 1, 0, 7), ("smooth", 33, 1025, 1, 0, 8),
         ("smooth", 32, 32, 2, 0, 9), ("smooth", 33, 32, 2, 1, 10), ("smooth", 65, 21, 3, 0, 11), ("smooth", 31, 85, 3, 0, 12),
         ("smooth", 33, 342, 3, 0, 13), ("smooth", 32, 64, 4, 0, 14), ("smooth", 65, 16, 4, 1, 15), ("smooth", 33, 43, 6, 0, 16),
         ("smooth", 31, 171, 6, 1, 17), ("smooth", 65, 8, 8, 0, 18), ("smooth", 33, 32, 8, 1, 19), ("smooth", 1, 129, 8, 1, 20),
         ("zeros", 33, 40, 3, 0, 21), ("zeros", 1, 1, 1, 0, 22), ("fib", 32, 150, 1, 0, 23), ("noise", 65, 100, 3, 0, 24),
         ("noise", 33, 50, 6, 1, 25), ("noise", 32, 1025, 1, 0, 26)]


def case_id(c):
    return "-".join(str(x) for x in c)


def header_band_rows():
    return header_constant("SF_PNG_ENC_BAND_ROWS")
