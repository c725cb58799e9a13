"""The JPEG encoder of csrc/jpeg_encode.hip restated in Python: encode_ref defines the entropy-coded segment byte for byte (colour
conversion, edge replication, integer DCT, quantisation, the Annex K.3 tables, restart intervals, stuffing), and the case list feeds
tests/test_jpeg_cases_cpu.py (which pins encode_ref to an independent Huffman decoder, a float64 DCT and PIL's libjpeg) and
tests/test_gpu_jpeg_encode.py (device bytes == encode_ref).  Written from ITU-T T.81 and the header comment of sf_jpeg_encode
(include/streamflow_hip.h); decode_scan below shares no code with the encoder half."""
import numpy as np

# ---- the format's constants, as the header states them ----------------------------------------------------------------------------------
DCT_TABLE = np.array([[4096, 4096, 4096, 4096, 4096, 4096, 4096, 4096], [5681, 4816, 3218, 1130, -1130, -3218, -4816, -5681],
                      [5352, 2217, -2217, -5352, -5352, -2217, 2217, 5352], [4816, -1130, -5681, -3218, 3218, 5681, 1130, -4816],
                      [4096, -4096, -4096, 4096, 4096, -4096, -4096, 4096], [3218, -5681, 1130, 4816, -4816, -1130, 5681, -3218],
                      [2217, -5352, 5352, -2217, -2217, 5352, -5352, 2217], [1130, -3218, 4816, -5681, 5681, -4816, 3218, -1130]], np.int64)
DCT_B = 0.3126                                  # |G / 2^18 - exact coefficient| <= DCT_B: dct_bound() is the derivation
PSNR_DEFICIT_DB = 0.114                         # the worst PSNR deficit of encode_ref against libjpeg over CASES (measured on the CPU)
PSNR_MARGIN_DB = PSNR_DEFICIT_DB + 0.05         # + the rounding differences between two correct encoders
BLOCK_BITS_MAX = 22 + 63 * 26                   # DC: 11-bit code + 11 bits; 63 AC levels: 16-bit code + 10 bits

DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
            0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
            0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
            0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
            0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
            0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
            0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
            0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
              0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
              0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
              0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
              0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
              0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
              0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
              0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def zigzag():
    """Scan position k -> natural index 8 v + u, walked along the anti-diagonals (T.81 figure A.6)."""
    order = []
    for d in range(15):
        cells = [(v, d - v) for v in range(8) if 0 <= d - v < 8]
        order += [8 * v + u for v, u in (cells if d % 2 else reversed(cells))]
    return np.array(order)


ZZ = zigzag()


def dct_basis():
    """a[u][x] = c(u) / 2 cos((2 x + 1) u pi / 16), float64: the exact one-dimensional transform."""
    u, x = np.mgrid[0:8, 0:8].astype(np.float64)
    return np.where(u == 0, np.sqrt(0.5), 1.0) / 2 * np.cos((2 * x + 1) * u * np.pi / 16)


def dct_bound():
    """The worst-case distance of G / 2^18 from the exact coefficient, from the table width (13 bits) and the shift (9) alone.  The
    table is 2^13 sqrt 2 a rounded: e = 2^-14 bounds |DCT_TABLE / 2^13 - sqrt 2 a|, |s| <= 128, A = max_u sum_x |sqrt 2 a[u][x]| = 4.
    rows:    |t - sqrt 2 t_exact| <= 8 * 128 * e (table) + 2^-5 (rounding to 4 fraction bits) = d = 0.09375
    columns: |G / 2^17 - 2 F_exact| <= A d (the rows' error through the exact basis) + 8 e (128 A + d) (the table's error on the
    stored t) = 0.375 + 0.25005; half of it, 0.31252, is the bound on the coefficient."""
    e, A = 2.0 ** -14, float(np.abs(np.sqrt(2) * dct_basis()).sum(axis=1).max())
    d = 8 * 128 * e + 2.0 ** -5
    return (A * d + 8 * e * (128 * A + d)) / 2


# ---- the encoder ------------------------------------------------------------------------------------------------------------------------
def components(img):
    """uint8 [h, w, 3] RGB, [h, w, 1] or [h, w] grey -> int64 [nc, h, w] samples 0 .. 255 (JFIF YCbCr for colour)."""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim in (2, 3)
    if a.ndim == 2 or a.shape[2] == 1:
        return a.reshape(a.shape[0], a.shape[1]).astype(np.int64)[None]
    r, g, b = (a[:, :, k].astype(np.int64) for k in range(3))
    return np.stack([(19595 * r + 38470 * g + 7471 * b + 32768) >> 16, (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16,
                     (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16])


def blocks(img):
    """-> int64 [bh, bw, nc, 8, 8]: level-shifted samples, the last row / column replicated up to a multiple of 8."""
    comp = components(img)
    nc, h, w = comp.shape
    bh, bw = -(-h // 8), -(-w // 8)
    comp = np.pad(comp, ((0, 0), (0, 8 * bh - h), (0, 8 * bw - w)), mode="edge") - 128
    return comp.reshape(nc, bh, 8, bw, 8).transpose(1, 3, 0, 2, 4)


def dct_int(s):
    """[..., 8(y), 8(x)] -> G[..., v, u] = 2^18 F: rows to 4 fraction bits (rounded half up), then columns."""
    t = (np.einsum("ux,...yx->...yu", DCT_TABLE, s) + 256) >> 9
    return np.einsum("vy,...yu->...vu", DCT_TABLE, t)


def quantise(F, qtables):
    """F [bh, bw, nc, 8, 8] -> levels [bh, bw, nc, 64] in zigzag order: G / (2^18 q) rounded half away from zero."""
    q = np.asarray(qtables, np.int64).reshape(2, 8, 8)
    nc = F.shape[2]
    qc = np.stack([q[0 if c == 0 else 1] for c in range(nc)])
    mag = (np.abs(F) + (qc << 17)) // (qc << 18)
    lv = np.where(F < 0, -mag, mag)
    return lv.reshape(F.shape[:3] + (64,))[..., ZZ]


def levels(img, qtables):
    return quantise(dct_int(blocks(img)), qtables)


def _codes(spec):
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc, self.n = (self.acc << length) | code, self.n + length

    def value(self, v, cat):
        self.put((v if v >= 0 else v - 1) & ((1 << cat) - 1), cat)

    def padded(self):
        pad = -self.n % 8
        return (((self.acc << pad) | ((1 << pad) - 1)).to_bytes((self.n + pad) // 8, "big"))


def entropy(lv):
    """Levels [bh, bw, nc, 64] -> the segment: one restart interval per block row."""
    bh, bw, nc, _ = lv.shape
    dc = [_codes(DC_LUMA), _codes(DC_CHROMA)]
    ac = [_codes(AC_LUMA), _codes(AC_CHROMA)]
    out = bytearray()
    for row in range(bh):
        bits, pred = _Bits(), [0] * nc
        for bx in range(bw):
            for c in range(nc):
                t = 0 if c == 0 else 1
                z = [int(v) for v in lv[row, bx, c]]
                diff, pred[c] = z[0] - pred[c], z[0]
                cat = abs(diff).bit_length()
                bits.put(*dc[t][cat])
                bits.value(diff, cat)
                run = 0
                for v in z[1:]:
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        bits.put(*ac[t][0xF0])
                        run -= 16
                    cat = abs(v).bit_length()
                    bits.put(*ac[t][run << 4 | cat])
                    bits.value(v, cat)
                    run = 0
                if run:
                    bits.put(*ac[t][0x00])
        out += bits.padded().replace(b"\xff", b"\xff\x00")
        if row < bh - 1:
            out += bytes((0xFF, 0xD0 + row % 8))
    return bytes(out)


def encode_ref(img, qtables):
    """uint8 [h, w, 3] / [h, w, 1] / [h, w] and qtables [2][64] (natural order) -> the segment sf_jpeg_encode must produce."""
    return entropy(levels(img, qtables))


def bound(h, w, channels):
    """sf_jpeg_encode_bound: per block row an interval of at most BLOCK_BITS_MAX bits per block, doubled for stuffing, + its marker."""
    interval = -(-(-(-w // 8) * channels * BLOCK_BITS_MAX) // 8)
    return (-(-h // 8) * (2 * interval + 2) + 3) // 4 * 4


# ---- an independent decoder of the segment ---------------------------------------------------------------------------------------------------
def decode_scan(segment, h, w, channels):
    """The segment -> levels [bh, bw, nc, 64] in zigzag order, by a plain bit-by-bit Huffman decoder: intervals split at the RSTm
    markers (whose numbers are checked), stuffing removed, padding checked to be 1-bits, every interval consumed exactly."""
    def table(spec):
        lookup, code, pos = {}, 0, 0
        for n, count in enumerate(spec[0], start=1):
            for sym in spec[1][pos:pos + count]:
                lookup[(n, code)] = sym
                code += 1
            pos += count
            code *= 2
        return lookup

    dct, act = [table(DC_LUMA), table(DC_CHROMA)], [table(AC_LUMA), table(AC_CHROMA)]
    bh, bw = (h + 7) // 8, (w + 7) // 8
    data, i, chunks, cur = bytes(segment), 0, [], bytearray()
    while i < len(data):
        if data[i] != 0xFF:
            cur.append(data[i])
            i += 1
            continue
        assert i + 1 < len(data), "a lone 0xFF ends the segment"
        if data[i + 1] == 0x00:
            cur.append(0xFF)
        else:
            assert data[i + 1] == 0xD0 + len(chunks) % 8, f"marker {data[i + 1]:#x} behind interval {len(chunks)}"
            chunks.append(bytes(cur))
            cur = bytearray()
        i += 2
    chunks.append(bytes(cur))
    assert len(chunks) == bh, (len(chunks), bh)
    out = np.zeros((bh, bw, channels, 64), np.int64)
    for row, chunk in enumerate(chunks):
        stream = "".join(format(b, "08b") for b in chunk)
        at = 0

        def symbol(lookup):
            nonlocal at
            for n in range(1, 17):
                key = (n, int(stream[at:at + n], 2))
                if len(stream) - at >= n and key in lookup:
                    at += n
                    return lookup[key]
            raise AssertionError(f"no code at bit {at} of interval {row}")

        def receive(cat):
            nonlocal at
            if cat == 0:
                return 0
            raw = int(stream[at:at + cat], 2)
            assert len(stream) - at >= cat
            at += cat
            return raw if raw >> (cat - 1) else raw - (1 << cat) + 1

        last = [0] * channels
        for bx in range(bw):
            for c in range(channels):
                k = 0 if c == 0 else 1
                last[c] += receive(symbol(dct[k]))
                out[row, bx, c, 0] = last[c]
                pos = 1
                while pos < 64:
                    rs = symbol(act[k])
                    if rs == 0:
                        break
                    if rs == 0xF0:
                        pos += 16
                        continue
                    pos += rs >> 4
                    assert pos < 64 and rs & 15, (row, bx, c, rs)
                    out[row, bx, c, pos] = receive(rs & 15)
                    pos += 1
        assert len(stream) - at < 8 and set(stream[at:]) <= {"1"}, f"interval {row}: {len(stream) - at} bits left"
    return out


# ---- images ---------------------------------------------------------------------------------------------------------------------------------
def wheel(h, w, seed):
    """A smooth colour wheel uint8 [h, w, 3]: hue from the angle, saturation from the radius of a smooth flow field."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u = 9 * np.sin(x / 97.0 + 0.3 + seed) * np.cos(y / 61.0) + 4 * np.sin((x + y) / 29.0) + x / 200.0 + rng.normal(0, 0.02, (h, w))
    v = 7 * np.cos(x / 83.0) * np.sin(y / 71.0 + 0.9) - 3 * np.cos((x - 2 * y) / 37.0) + y / 150.0 + rng.normal(0, 0.02, (h, w))
    rad = np.sqrt(u * u + v * v)
    rad = rad / max(rad.max(), 1e-9)
    ang = np.arctan2(-v, -u)
    rgb = np.stack([0.5 + 0.5 * np.cos(ang + k * 2 * np.pi / 3) for k in range(3)], axis=-1)
    return np.floor(255 * (1 - rad[..., None] * (1 - rgb))).astype(np.uint8)


def basis77(amp=100.0):
    """uint8 [8, 8]: 128 + the (7, 7) basis function at amplitude `amp`, rounded.  The rounding leaves a few tenths in the other
    coefficients with odd u and v, so at steps of 1 some of them survive; under the "only63" tables (steps of 255 but for a 1 at
    coefficient 63) a block is its DC difference of 0, three ZRLs, the symbol 0xE? for coefficient 63 and no EOB."""
    a = dct_basis()[7]
    return np.clip(np.rint(128 + amp * 4 * np.outer(a, a)), 0, 255).astype(np.uint8)


def make(kind, h, w, channels, seed):
    """uint8 [h, w, 3] or [h, w]."""
    rng = np.random.default_rng(seed)
    shape = (h, w, 3) if channels == 3 else (h, w)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "const":
        return np.full(shape, seed % 256, np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, size=shape, dtype=np.uint8)
    if kind == "basis77":                       # every block the pattern
        g = np.tile(basis77(), (-(-h // 8), -(-w // 8)))[:h, :w]
    elif kind == "checker":                     # 0 / 255 in cells of `seed` pixels
        g = (((y // seed + x // seed) % 2) * 255).astype(np.uint8)
    elif kind == "blocks":                      # black and white 8 x 8 blocks in turn
        g = (((y // 8 + x // 8) % 2) * 255).astype(np.uint8)
    elif kind == "wheel":
        img = wheel(h, w, seed)
        return img if channels == 3 else img[:, :, 1].copy()
    else:
        assert kind == "mixed"                  # a gradient, an edge and a little noise: short and long runs, both signs
        g = (3 * x + 5 * y + (x * y) // 5 + 90 * (x > w // 2) + rng.integers(0, 12, size=(h, w))) & 255
        g = g.astype(np.uint8)
    if channels == 1:
        return g
    return np.stack([g, np.roll(g, 1, axis=1) if kind == "mixed" else g, 255 - g if kind == "mixed" else g], axis=-1).astype(np.uint8)


# (kind, h, w, channels, quality, seed); quality: the IJG quality of jpeg_gpu.quant_tables, or "only63" (tables())
CASES = [("mixed", h, w, c, 75, 100 + 10 * h + w) for c in (3, 1) for h in (1, 7, 8, 9, 17) for w in (1, 7, 8, 9, 17)]
CASES += [("mixed", 73, 9, 3, 75, 1), ("mixed", 73, 9, 1, 90, 2)]                                  # 10 intervals: RST0 .. RST7, RST0
CASES += [("mixed", 8, w, c, 75, w + c) for c in (3, 1) for w in (680, 688, 2736)]                 # 255, 258, 1026 blocks an interval
CASES += [("const", 17, 19, 3, 75, 0), ("const", 9, 40, 1, 50, 255), ("const", 24, 8, 3, 100, 128), ("const", 8, 8, 1, 90, 77)]
CASES += [("noise", 33, 47, 3, 100, 3), ("noise", 40, 31, 1, 100, 4), ("noise", 19, 23, 3, 50, 5)]
CASES += [("basis77", 8, 8, 1, 100, 0), ("basis77", 16, 24, 3, 100, 0), ("basis77", 8, 8, 1, "only63", 0),
          ("basis77", 16, 24, 3, "only63", 0)]
CASES += [("checker", 16, 24, 1, 100, 1), ("checker", 17, 23, 3, 100, 2), ("checker", 16, 16, 1, 100, 4),
          ("blocks", 16, 40, 1, 100, 0), ("blocks", 24, 24, 3, 100, 0)]
CASES += [("wheel", 64, 96, 3, 50, 1), ("wheel", 64, 96, 3, 75, 2), ("wheel", 61, 90, 3, 90, 3), ("wheel", 40, 50, 1, 75, 4)]


def header_constant(name):
    """An integer #define of include/streamflow_hip.h."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "streamflow_hip.h")
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(path).read()).group(1))


def case_id(c):
    return "-".join(str(x) for x in c)


def tables(quality):
    """uint16 [2, 64], natural order: jpeg_gpu.quant_tables(quality), or for "only63" steps of 255 with a 1 at coefficient 63."""
    if quality == "only63":
        q = np.full((2, 64), 255, np.uint16)
        q[:, 63] = 1
        return q
    from streamflow_amd import jpeg_gpu
    return jpeg_gpu.quant_tables(quality)


def psnr(a, b):
    """PSNR in dB of two uint8 arrays; 99 where they are equal."""
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def pil_file(img, qtables):
    """libjpeg's file of `img` at the same tables, 4:4:4, the typical Huffman tables (PIL takes the tables in natural order)."""
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.asarray(img)).save(buf, "JPEG", qtables=[[int(v) for v in t] for t in np.asarray(qtables).reshape(2, 64)],
                                          subsampling=0, optimize=False)
    return buf.getvalue()


def pil_decode(blob):
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(blob))
    im.load()
    return im
