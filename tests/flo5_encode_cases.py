"""The .flo5 chunk encoder of csrc/flo5_encode.hip restated in Python: chunk_stream_ref defines the format byte for byte, and the case
list feeds tests/test_flo5_encode_cases_cpu.py (which pins it to zlib, flo5.read_flo5 and the real h5py) and
tests/test_gpu_flo5_encode.py (device bytes == chunk_stream_ref).  Integers only; the Huffman-only deflate block is the PNG
encoder's (tests/png_encode_cases.py: huffman_lengths, canonical_codes, band_tables, band_items, imported here).

A field [2, h, w] float32 is cut into ceil(h / rpc) chunks of the HDF5 dataset [h, w, 2]: chunk c holds rows c rpc .. c rpc + rpc - 1,
rows past h as zero bits; its N = rpc w 2 elements in (row, column, channel) order are bit patterns, never values.  The HDF5
shuffle filter puts byte j (little-endian) of element e at j N + e.  A chunk's stream is `78 01`, then for each byte plane j = 0 .. 3 in
turn one block per segment of at most BLOCK_BYTES bytes (no block straddles two planes; BFINAL on the last block of plane 3), then
the big-endian Adler-32 of the 4 N shuffled bytes."""
import zlib

import numpy as np

from tests.png_cases import header_constant
from tests.png_encode_cases import HEADER_BITS_MAX, band_items, band_tables, canonical_codes, huffman_lengths  # noqa: F401

BLOCK_BYTES = 65536
MAX_CHUNKS = 64


def default_rows_per_chunk(h):
    """flo5.write_flo5's rule: at most 32 chunks."""
    return max(1, -(-h // 32))


def chunk_bytes(flow, c, rpc):
    """flow [2, h, w] float32 -> the bytes of HDF5 chunk c of the dataset [h, w, 2]: uint8 [rpc * w * 2 * 4], zero rows past h."""
    f = np.ascontiguousarray(flow, dtype="<f4")
    assert f.ndim == 3 and f.shape[0] == 2
    _, h, w = f.shape
    buf = np.zeros((rpc, w, 2), np.uint32)
    rows = f.view(np.uint32)[:, c * rpc:(c + 1) * rpc].transpose(1, 2, 0)
    buf[:rows.shape[0]] = rows
    return buf.astype("<u4").view(np.uint8).reshape(-1)


def shuffled(flow, c, rpc):
    """The chunk after HDF5's shuffle filter: uint8 [4 N], byte j of element e at j N + e."""
    return np.ascontiguousarray(chunk_bytes(flow, c, rpc).reshape(-1, 4).T).reshape(-1)


def blocks(n_elems, block_bytes=BLOCK_BYTES):
    """(start, stop) of every block in the shuffled chunk, in stream order."""
    return [(j * n_elems + s, j * n_elems + min(s + block_bytes, n_elems)) for j in range(4) for s in range(0, n_elems, block_bytes)]


def pack_items(parts):
    """[(codes, lengths)] per block -> the bytes of the LSB-first bit stream."""
    codes = np.concatenate([p[0] for p in parts]).astype(np.int64)
    lens = np.concatenate([p[1] for p in parts]).astype(np.int64)
    start = np.cumsum(lens) - lens
    nbits = int(lens.sum())
    bits = np.zeros(-(-nbits // 8) * 8, np.uint8)
    for k in range(17):
        on = (lens > k) & ((codes >> k) & 1 == 1)
        bits[start[on] + k] = 1
    return np.packbits(bits, bitorder="little").tobytes()


def chunk_stream_ref(flow, c, rpc, block_bytes=BLOCK_BYTES):
    """The zlib stream sf_flo5_encode must write for chunk c of flow [2, h, w]."""
    data = shuffled(flow, c, rpc)
    cuts = blocks(data.size // 4, block_bytes)
    parts = [band_items(data[a:b], k == len(cuts) - 1) for k, (a, b) in enumerate(cuts)]
    return b"\x78\x01" + pack_items(parts) + (zlib.adler32(data.tobytes()) & 0xFFFFFFFF).to_bytes(4, "big")


def stream_bits(data, block_bytes=BLOCK_BYTES):
    """Bits of the blocks of a shuffled chunk `data` (what the size of a stream is made of), without building the stream."""
    total = 0
    for a, b in blocks(data.size // 4, block_bytes):
        hist = np.bincount(data[a:b], minlength=256)
        lit, cl, _, _ = band_tables(hist)
        total += 17 + 19 * 3 + sum(cl[l] for l in lit + [1, 1]) + int((hist * np.asarray(lit[:256])).sum()) + lit[256]
    return total


def field_streams_ref(flow, rpc=0):
    """Every chunk's stream of one field; rpc = 0: the default rule."""
    rpc = rpc or default_rows_per_chunk(flow.shape[1])
    return [chunk_stream_ref(flow, c, rpc) for c in range(-(-flow.shape[1] // rpc))]


def bound(rpc, w):
    """sf_flo5_chunk_bound: 2 + the blocks + 4, rounded up to 4; a block of B bytes has at most HEADER_BITS_MAX + 9 B + 9 bits."""
    n = rpc * w * 2
    nblk = 4 * -(-n // BLOCK_BYTES)
    bits = nblk * (HEADER_BITS_MAX + 9) + 9 * 4 * n
    return (2 + -(-bits // 8) + 4 + 3) // 4 * 4


# ---- fields -----------------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0x7FC00000, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000,
                     0x00000001, 0x807FFFFF, 0x00400000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00800000], np.uint32)
# quiet NaNs with payloads, a signalling NaN, -0.0, 0.0, +-inf, denormals, the largest finite values, the smallest normal


def make(h, w, seed, special=False):
    """A flow field [2, h, w] float32: smooth waves plus a little noise (sign / exponent bytes with few values, noisy low mantissa
    bytes: what a Spring field looks like to the coder); special=True scatters SPECIALS' bit patterns over it."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u = 9 * np.sin(x / 97.0 + 0.3) * np.cos(y / 61.0) + 4 * np.sin((x + y) / 29.0) + x / 200.0
    v = 7 * np.cos(x / 83.0) * np.sin(y / 71.0 + 0.9) - 3 * np.cos((x - 2 * y) / 37.0) + y / 150.0
    f = (np.stack([u, v]) + rng.normal(0, 0.02, size=(2, h, w))).astype(np.float32)
    if special:
        bits = f.view(np.uint32).reshape(-1)
        where = rng.choice(bits.size, size=min(bits.size, max(len(SPECIALS), bits.size // 7)), replace=False)
        bits[where] = SPECIALS[np.arange(where.size) % len(SPECIALS)]
    return f


def bench_field(h, w, seed):
    """The field of tools/flo5_encode_bench.py: coarse Gaussian noise (one sample per 64 pixels, sigma 12 px) upsampled bilinearly,
    plus 0.01 px of noise.  Synthetic: no Spring frame is involved."""
    rng = np.random.default_rng(seed)
    gh, gw = h // 64 + 2, w // 64 + 2
    coarse = rng.normal(0, 12.0, size=(2, gh, gw))
    yy, xx = np.arange(h) / 64.0, np.arange(w) / 64.0
    y0, x0 = yy.astype(np.int64), xx.astype(np.int64)
    fy, fx = (yy - y0)[None, :, None], (xx - x0)[None, None, :]
    a, b = coarse[:, y0][:, :, x0], coarse[:, y0][:, :, x0 + 1]
    c, d = coarse[:, y0 + 1][:, :, x0], coarse[:, y0 + 1][:, :, x0 + 1]
    smooth = (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy
    return (smooth + rng.normal(0, 0.01, size=(2, h, w))).astype(np.float32)


# (h, w, rpc): N = 2 (one word short of a word); N = 6, the tail behind a word; an edge chunk padded with zero rows; N = 65536, exactly
# one full block per plane; N = 65538, a 2-byte second segment per plane; the default rule (rpc = 0 -> 3 rows, 24 chunks, the last short)
CASES = [(1, 1, 1), (1, 3, 1), (37, 53, 2), (64, 512, 64), (3, 10923, 3), (70, 9, 0)]


def case_id(c):
    return "x".join(str(v) for v in c)


def header_block_bytes():
    return header_constant("SF_FLO5_BLOCK_BYTES")
