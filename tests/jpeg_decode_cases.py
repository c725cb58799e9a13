"""The JPEG decoder of csrc/jpeg_decode.hip restated in Python: decode_ref(blob) defines the pixels sf_jpeg_decode must produce, from
its own marker walk, a bit-by-bit Huffman decoder in the style of jpeg_cases.decode_scan, libjpeg's integer inverse DCT ("islow"),
its "fancy" chroma upsampling (and its replication of the samples where a chroma plane is at most 2 samples wide) and the JFIF colour
conversion, in numpy.  Written from ITU-T T.81 and the header comment of sf_jpeg_decode (include/streamflow_hip.h); it shares no code
with streamflow_amd/jpeg_gpu.py (Call, further down, is the one place that uses jpeg_gpu: it builds the arguments of a call).  The
case list names the fixtures of tests/golden/jpeg_decode (made by tests/golden/make_jpeg_decode_golden.py with PIL: the .jpg files
and PIL's pixels in expected.npz) and feeds tests/test_jpeg_decode_cases_cpu.py (decode_ref == PIL == expected.npz; jpeg_gpu.parse against this walk; the overflow
bounds), tests/test_jpeg_decode_core_host_cpu.py (the decoder core under the host sanitizers) and tests/test_gpu_jpeg_decode.py."""
import functools
import os

import numpy as np

from tests import jpeg_cases as jc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg_decode")
COEF_MAX, BLOCK_SUM_MAX = 2048, 18432           # SF_JPEG_COEF_RANGE: |c| and the sum of |c| over a block
(OK, BAD_CODE, BAD_RUN, BAD_CATEGORY, TRUNCATED, NOT_CONSUMED, BAD_DESC, COEF_RANGE, BAD_TABLE, BAD_MARKER) = range(10)
DESC_WORDS, TABLE_SET_BYTES = 6, 1824

# (name, kind, h, w, channels, seed, PIL save options) -- what make_jpeg_decode_golden.py writes with PIL
_SAMPLING = (("444", 3, 0), ("422", 3, 1), ("420", 3, 2), ("grey", 1, None))
_SIZES = ((1, 1), (7, 9), (8, 8), (9, 7), (16, 17), (17, 16), (33, 33), (1, 33), (33, 1), (16, 16), (9, 4), (17, 3))   # w <= 4: no fancy filter
PIL_CASES = []
for _tag, _c, _sub in _SAMPLING:
    for _k, (_h, _w) in enumerate(_SIZES):
        _opt = dict(quality=75, optimize=bool(_k % 2))
        if _sub is not None:
            _opt["subsampling"] = _sub
        PIL_CASES.append((f"{_tag}-{_h}x{_w}" + ("-opt" if _k % 2 else ""), "mixed", _h, _w, _c, 10 * _h + _w, _opt))
PIL_CASES += [
    # restart intervals: every MCU, every third, one per MCU row; ten MCU rows (RST7 is followed by RST0)
    ("420-33x33-rst1", "mixed", 33, 33, 3, 1, dict(quality=75, subsampling=2, restart_marker_blocks=1)),
    ("420-33x33-rst3", "mixed", 33, 33, 3, 2, dict(quality=75, subsampling=2, restart_marker_blocks=3, optimize=True)),
    ("422-17x33-rst3", "mixed", 17, 33, 3, 3, dict(quality=75, subsampling=1, restart_marker_blocks=3)),
    ("444-16x33-rows", "mixed", 16, 33, 3, 4, dict(quality=75, subsampling=0, restart_marker_rows=1)),
    ("grey-33x17-rst1", "mixed", 33, 17, 1, 5, dict(quality=75, restart_marker_blocks=1)),
    ("444-73x9-rows", "mixed", 73, 9, 3, 6, dict(quality=75, subsampling=0, restart_marker_rows=1)),
    ("420-73x9-rows", "mixed", 73, 9, 3, 7, dict(quality=60, subsampling=2, restart_marker_rows=1, optimize=True)),
    # one wide interval
    ("444-8x2736", "wheel", 8, 2736, 3, 8, dict(quality=50, subsampling=0)),
    # quantisation extremes: 16-bit codes, clamping, stuffed FF bytes
    ("420-17x33-q1", "mixed", 17, 33, 3, 9, dict(quality=1, subsampling=2)),
    ("444-16x17-q100-noise", "noise", 16, 17, 3, 10, dict(quality=100, subsampling=0)),
    ("420-17x16-q100-noise", "noise", 17, 16, 3, 11, dict(quality=100, subsampling=2, optimize=True)),
    ("grey-16x24-q100-noise", "noise", 16, 24, 1, 12, dict(quality=100)),
    ("grey-16x24-q100-checker", "checker", 16, 24, 1, 1, dict(quality=100)),
    ("444-17x23-q100-checker", "checker", 17, 23, 3, 1, dict(quality=100, subsampling=0)),
    ("422-16x16-q100-checker", "checker", 16, 16, 3, 2, dict(quality=100, subsampling=1)),
    ("grey-16x40-q100-blocks", "blocks", 16, 40, 1, 0, dict(quality=100)),
    ("420-24x24-q100-blocks", "blocks", 24, 24, 3, 0, dict(quality=100, subsampling=2)),
]
# (name, kind, h, w, channels, quality, seed): files of the project's own encoder (jpeg_cases.encode_ref + jpeg_gpu.jpeg_file)
OWN_CASES = [("own-basis77-only63-16x24", "basis77", 16, 24, 3, "only63", 0), ("own-basis77-only63-8x8-grey", "basis77", 8, 8, 1, "only63", 0),
             ("own-mixed-17x23", "mixed", 17, 23, 3, 75, 3)]
# hand-built framing on top of a PIL file: (name, source case, edit)
EDIT_CASES = [("444-16x17-nodht", "444-16x17", "strip-dht"), ("420-33x33-rst3-fill", "420-33x33-rst3", "fill")]
NAMES = [c[0] for c in PIL_CASES] + [c[0] for c in OWN_CASES] + [c[0] for c in EDIT_CASES]
REFUSED = ("refuse-progressive", "refuse-cmyk", "refuse-411", "refuse-rgb-adobe", "refuse-12bit")


def own_file(case):
    """The file of an OWN_CASES entry: the same bytes wherever it is made."""
    from streamflow_amd import jpeg_gpu
    _, kind, h, w, c, quality, seed = case
    q = jc.tables(quality)
    return jpeg_gpu.jpeg_file(jc.encode_ref(jc.make(kind, h, w, c, seed), q), h, w, c, q)


def segments(blob):
    """[(marker, payload start, payload end)] of the marker segments up to and including SOS."""
    out, pos = [], 2
    while True:
        while blob[pos + 1] == 0xFF:
            pos += 1
        marker, size = blob[pos + 1], int.from_bytes(blob[pos + 2:pos + 4], "big")
        out.append((marker, pos + 4, pos + 2 + size))
        pos += 2 + size
        if marker == 0xDA:
            return out


def edit(blob, how):
    """The hand-built framings: all DHT segments removed; FF fill bytes in front of DQT, SOS, every RSTm and EOI."""
    segs = segments(blob)
    if how == "strip-dht":
        out = blob[:2]
        for marker, lo, hi in segs:
            if marker != 0xC4:
                out += blob[lo - 4:hi]
        return out + blob[segs[-1][2]:]
    assert how == "fill"
    head = blob[:2]
    for marker, lo, hi in segs:
        head += (b"\xff\xff" if marker in (0xDB, 0xDA) else b"") + blob[lo - 4:hi]
    body, out, i = blob[segs[-1][2]:], bytearray(), 0
    while i < len(body):
        if body[i] == 0xFF and body[i + 1] != 0:
            out += b"\xff"                                                  # one fill byte in front of RSTm / EOI
        out.append(body[i])
        if body[i] == 0xFF:
            out.append(body[i + 1])
            i += 1
        i += 1
    return head + bytes(out)


@functools.lru_cache(maxsize=None)
def load(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


@functools.lru_cache(maxsize=None)
def expected():
    with np.load(os.path.join(GOLDEN, "expected.npz")) as z:
        return {k: z[k] for k in z.files}


# ---- the walk ---------------------------------------------------------------------------------------------------------------------------
def walk(blob):
    """dict(h, w, nc, hs, vs, quant [nc][64] natural order, dc / ac [nc] (BITS, HUFFVAL), restart, intervals [(start, end)] into blob):
    a plain sequential walk, byte by byte through the entropy-coded data."""
    assert blob[:2] == b"\xff\xd8"
    quant, huff, restart = {}, {}, 0
    for marker, lo, hi in segments(blob):
        seg = blob[lo:hi]
        if marker == 0xDB:
            while seg:
                assert seg[0] >> 4 == 0
                q = np.zeros(64, np.int64)
                q[jc.ZZ] = list(seg[1:65])
                quant[seg[0] & 15], seg = q, seg[65:]
        elif marker == 0xC4:
            while seg:
                bits = list(seg[1:17])
                huff[(seg[0] >> 4, seg[0] & 15)], seg = (bits, list(seg[17:17 + sum(bits)])), seg[17 + sum(bits):]
        elif marker == 0xDD:
            restart = int.from_bytes(seg, "big")
        elif marker == 0xC0:
            assert seg[0] == 8
            h, w, nc = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"), seg[5]
            comps = [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nc)]
        elif marker == 0xDA:
            assert seg[0] == nc and [seg[1 + 2 * i] for i in range(nc)] == [c[0] for c in comps]
            sel = [(seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(nc)]
            start = hi
    if not huff:                                                            # T.81 Annex K.3, as MJPEG decoders assume
        huff = {(0, 0): jc.DC_LUMA, (1, 0): jc.AC_LUMA, (0, 1): jc.DC_CHROMA, (1, 1): jc.AC_CHROMA}
    hs, vs = (comps[0][1], comps[0][2]) if nc == 3 else (1, 1)
    assert nc == 1 or all(c[1:3] == (1, 1) for c in comps[1:])
    intervals, i, lo = [], start, start
    while True:
        if blob[i] != 0xFF or blob[i + 1] == 0:
            i += 1 + (blob[i] == 0xFF)
            continue
        end = i
        while blob[i + 1] == 0xFF:                                          # fill bytes
            i += 1
        intervals.append((lo, end))
        if blob[i + 1] == 0xD9:
            break
        assert blob[i + 1] == 0xD0 + (len(intervals) - 1) % 8, (len(intervals), blob[i + 1])
        i += 2
        lo = i
    return dict(h=h, w=w, nc=nc, hs=hs, vs=vs, quant=[quant[c[3]] for c in comps], dc=[huff[(0, s[0])] for s in sel],
                ac=[huff[(1, s[1])] for s in sel], restart=restart, intervals=intervals)


def _lookup(spec):
    table, code, pos = {}, 0, 0
    for n, count in enumerate(spec[0], start=1):
        for sym in spec[1][pos:pos + count]:
            table[(n, code)] = sym
            code += 1
        pos += count
        code *= 2
    return table


def coefficients(blob):
    """(walk, [per component int64 [block rows, block columns, 64]]): the dequantised coefficients in natural order, every interval
    decoded bit by bit and consumed exactly (at most 7 padding bits, all 1)."""
    info = walk(blob)
    h, w, nc, hs, vs = (info[k] for k in ("h", "w", "nc", "hs", "vs"))
    mcux, mcuy = -(-w // (8 * hs)), -(-h // (8 * vs))
    shape = [(hs, vs)] + [(1, 1)] * (nc - 1)
    coef = [np.zeros((mcuy * cv, mcux * ch, 64), np.int64) for ch, cv in shape]
    dct, act = [_lookup(s) for s in info["dc"]], [_lookup(s) for s in info["ac"]]
    per = info["restart"] or mcux * mcuy
    assert len(info["intervals"]) == -(-mcux * mcuy // per)
    for n, (lo, end) in enumerate(info["intervals"]):
        stream = "".join(format(b, "08b") for b in blob[lo:end].replace(b"\xff\x00", b"\xff"))
        at = 0

        def symbol(table):
            nonlocal at
            for k in range(1, 17):
                key = (k, int(stream[at:at + k], 2))
                if len(stream) - at >= k and key in table:
                    at += k
                    return table[key]
            raise AssertionError(f"no code at bit {at} of interval {n}")

        def receive(cat):
            nonlocal at
            if cat == 0:
                return 0
            assert len(stream) - at >= cat
            raw = int(stream[at:at + cat], 2)
            at += cat
            return raw if raw >> (cat - 1) else raw - (1 << cat) + 1

        pred = [0] * nc
        for mi in range(n * per, min((n + 1) * per, mcux * mcuy)):
            my, mx = divmod(mi, mcux)
            for c, (ch, cv) in enumerate(shape):
                for j in range(ch * cv):
                    block = coef[c][my * cv + j // ch, mx * ch + j % ch]
                    pred[c] += receive(symbol(dct[c]))
                    block[0] = pred[c]
                    k = 1
                    while k < 64:
                        rs = symbol(act[c])
                        if rs == 0:
                            break
                        if rs == 0xF0:
                            k += 16
                            continue
                        k += rs >> 4
                        assert k < 64 and rs & 15
                        block[jc.ZZ[k]] = receive(rs & 15)
                        k += 1
                    block *= info["quant"][c]
        assert len(stream) - at < 8 and set(stream[at:]) <= {"1"}, f"interval {n}: {len(stream) - at} bits left"
    return info, coef


# ---- the inverse DCT --------------------------------------------------------------------------------------------------------------------
def islow_1d(i):
    """libjpeg's jidctint.c pass on a list of 8 values (anything with +, -, * and <<); the caller descales."""
    z2, z3 = i[2], i[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 - z3 * 15137
    tmp3 = z1 + z2 * 6270
    tmp0 = (i[0] + i[4]) << 13
    tmp1 = (i[0] - i[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069, z4 * -3196
    z3, z4 = z3 + z5, z4 + z5
    t0 = t0 + (z1 + z3)
    t1 = t1 + (z2 + z4)
    t2 = t2 + (z2 + z3)
    t3 = t3 + (z1 + z4)
    return [tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3]


def idct(coef):
    """int64 [..., 64] natural order -> uint8 [..., 8, 8]: columns ((x + 1024) >> 11), rows ((x + 2^17) >> 18), + 128, clamped."""
    f = np.asarray(coef, np.int64).reshape(coef.shape[:-1] + (8, 8))
    cols = np.stack(islow_1d([f[..., v, :] for v in range(8)]), axis=-2)
    ws = (cols + 1024) >> 11
    rows = np.stack(islow_1d([ws[..., :, u] for u in range(8)]), axis=-1)
    return np.clip(((rows + (1 << 17)) >> 18) + 128, 0, 255).astype(np.uint8)


class _Form:
    """A linear form over the 8 inputs of a pass; every one made is logged."""
    log = []

    def __init__(self, w):
        self.w = np.asarray(w, dtype=object)
        _Form.log.append(self.w)

    def __add__(self, o):
        return _Form(self.w + o.w)

    def __sub__(self, o):
        return _Form(self.w - o.w)

    def __mul__(self, c):
        return _Form(self.w * c)

    def __lshift__(self, n):
        return _Form(self.w * (1 << n))


def idct_bounds(coef_max, block_sum_max):
    """(pass 1, pass 2): the largest absolute value any intermediate of islow_1d can take in each pass -- the descale's rounding
    constant included -- over ALL blocks whose coefficients have |c| <= coef_max and sum |c| <= block_sum_max.  A worst-case
    argument on the transform's data flow, not a sample: islow_1d runs on linear forms, which gives every intermediate's weights on
    the pass's 8 inputs (a of pass 2 on ws[y][0 .. 7], b of the outputs of pass 1 on F[0 .. 7][u]).
    Pass 1: |sum_v a_v F_vu| <= coef_max sum |a_v|.
    Pass 2: ws[y][u] = (sum_v b_yv F_vu + 1024) >> 11 is within 1 of sum_v b_yv F_vu / 2^11, so an intermediate is within sum |a_u| of
    sum_uv a_u b_yv F_vu / 2^11; the largest value of sum_uv |a_u b_yv| |F_vu| under the two bounds puts coef_max on the largest
    weights until block_sum_max is used up."""
    _Form.log = []
    outs = islow_1d([_Form(np.eye(8, dtype=object)[k]) for k in range(8)])
    forms = [np.abs(w) for w in _Form.log]
    b = [np.abs(o.w) for o in outs]
    assert len(forms) >= 50 and max(int(f.sum()) for f in forms) >= 8192 * 7
    pass1 = max(coef_max * int(f.sum()) for f in forms) + 1024
    full, rest = divmod(block_sum_max, coef_max)
    pass2 = 0
    for by in b:
        for a in forms:
            wts = sorted((int(x) * int(y) for x in by for y in a), reverse=True)
            total = coef_max * sum(wts[:full]) + (rest * wts[full] if full < 64 else 0)
            pass2 = max(pass2, -(-total // 2048) + int(a.sum()) + (1 << 17))
    return pass1, pass2


# ---- upsampling and colour ----------------------------------------------------------------------------------------------------------------
def upsample_h2v1(c, w):
    """int64 [rows, cw] -> [rows, w]: libjpeg's h2v1_fancy_upsample."""
    left, right = np.concatenate([c[:, :1], c[:, :-1]], axis=1), np.concatenate([c[:, 1:], c[:, -1:]], axis=1)
    even, odd = (3 * c + left + 1) >> 2, (3 * c + right + 2) >> 2
    even[:, 0], odd[:, -1] = c[:, 0], c[:, -1]
    return np.stack([even, odd], axis=-1).reshape(c.shape[0], -1)[:, :w]


def upsample_h2v2(c, h, w):
    """int64 [ch, cw] -> [h, w]: libjpeg's h2v2_fancy_upsample, the first and last chroma rows replicated."""
    up, down = np.concatenate([c[:1], c[:-1]]), np.concatenate([c[1:], c[-1:]])
    t = np.stack([3 * c + up, 3 * c + down], axis=1).reshape(2 * c.shape[0], -1)
    left, right = np.concatenate([t[:, :1], t[:, :-1]], axis=1), np.concatenate([t[:, 1:], t[:, -1:]], axis=1)
    even, odd = (3 * t + left + 8) >> 4, (3 * t + right + 7) >> 4
    even[:, 0], odd[:, -1] = (4 * t[:, 0] + 8) >> 4, (4 * t[:, -1] + 7) >> 4
    return np.stack([even, odd], axis=-1).reshape(t.shape[0], -1)[:h, :w]


def planes(info, coef):
    """The components' sample planes uint8 [8 block rows, 8 block columns], padded to whole blocks."""
    return [idct(c).transpose(0, 2, 1, 3).reshape(8 * c.shape[0], 8 * c.shape[1]) for c in coef]


@functools.lru_cache(maxsize=None)
def decode_ref(blob):
    """A baseline JPEG file -> uint8 [h, w, 3] (a grey file's sample three times): what sf_jpeg_decode must produce, bit for bit."""
    info, coef = coefficients(blob)
    h, w, hs, vs = info["h"], info["w"], info["hs"], info["vs"]
    pl = [p.astype(np.int64) for p in planes(info, coef)]
    y = pl[0][:h, :w]
    if info["nc"] == 1:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    ch, cw = -(-h // vs), -(-w // hs)
    chroma = []
    for p in pl[1:]:
        real = p[:ch, :cw]
        if hs == 2 and cw <= 2:                                             # libjpeg: too narrow for the triangle filter, samples replicated
            real = np.repeat(np.repeat(real, vs, axis=0), hs, axis=1)[:h, :w]
        chroma.append(real if hs == 1 or cw <= 2 else upsample_h2v1(real, w) if vs == 1 else upsample_h2v2(real, h, w))
    cb, cr = chroma[0] - 128, chroma[1] - 128
    rgb = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], axis=-1)
    out = np.clip(rgb, 0, 255).astype(np.uint8)
    out.setflags(write=False)
    return out


def coef_layout(info, coef):
    """The coefficient workspace of one image as sf_jpeg_decode lays it out: int16 [component][block row][block column][64], flat."""
    return np.concatenate([c.reshape(-1) for c in coef]).astype(np.int16)


def pil_pixels(blob):
    """PIL's (libjpeg-turbo's) pixels of a file as uint8 [h, w, 3]."""
    im = jc.pil_decode(blob)
    a = np.asarray(im.convert("RGB") if im.mode != "L" else im)
    return a if a.ndim == 3 else np.repeat(a[:, :, None], 3, axis=2)


# ---- calls: what sf_jpeg_decode (and the host program) take ---------------------------------------------------------------------------------
class Call:
    """The arguments of one sf_jpeg_decode call for the fixtures `names` (one geometry), built by jpeg_gpu.parse / pack."""

    def __init__(self, names):
        from streamflow_amd import jpeg_gpu
        self.names = list(names)
        blobs = [load(n) for n in self.names]
        parsed = [jpeg_gpu.parse(b, n) for b, n in zip(blobs, self.names)]
        assert len({p[:5] for p in parsed}) == 1, "one geometry per call"
        self.h, self.w, self.nc, self.hs, self.vs = parsed[0][:5]
        self.n = len(blobs)
        self.data, self.desc, self.tables = jpeg_gpu.pack(parsed, blobs)
        self.data, self.desc, self.tables = self.data.copy(), self.desc.copy(), self.tables.copy()

    def copy(self):
        c = object.__new__(Call)
        c.__dict__.update(self.__dict__)
        c.data, c.desc, c.tables = self.data.copy(), self.desc.copy(), self.tables.copy()
        return c

    def rows(self, image):
        return [int(r) for r in np.flatnonzero(self.desc[:, 2] == image)]

    def image_blocks(self):
        mcux, mcuy = -(-self.w // (8 * self.hs)), -(-self.h // (8 * self.vs))
        return mcux * mcuy * (self.hs * self.vs + (2 if self.nc == 3 else 0))


MUTATED = ("420-33x33", "420-33x33-rst1", "420-33x33-rst3")       # no DRI, intervals of 1 MCU, of 3 (with tables of its own)


def mutations():
    """[(label, Call)]: deterministic damage to image 1 of the MUTATED batch (images 0 and 2 stay decodable): truncated intervals,
    flipped bits, an interval that runs into the next one's RST marker, all-1 bits with and without stuffing, a lone FF at the end,
    descriptors out of every range, a Huffman specification that is none, steps that push coefficients out of range."""
    base = Call(MUTATED)
    rows = base.rows(1)
    out = []

    def variant(label):
        c = base.copy()
        out.append((label, c))
        return c

    for k, cut in enumerate((1, 2, 10 ** 6)):
        c = variant(f"truncate-{cut}")
        r = rows[2 * k]
        c.desc[r, 1] = max(0, c.desc[r, 1] - cut)
    rng = np.random.default_rng(20261020)
    lo, hi = int(base.desc[rows[0], 0]), int(base.desc[rows[-1], 0] + base.desc[rows[-1], 1])
    for k in range(8):
        c = variant(f"flip-{k}")
        c.data[int(rng.integers(lo, hi))] ^= 1 << int(rng.integers(0, 8))
    c = variant("into-the-next-marker")
    c.desc[rows[1], 1] += 2 + c.desc[rows[2], 1]
    c = variant("all-ones-stuffed")
    r = rows[3]
    n = int(c.desc[r, 1])
    c.data[c.desc[r, 0]:c.desc[r, 0] + n] = np.resize(np.array([0xFF, 0x00], np.uint8), n)
    c = variant("all-ones-unstuffed")
    c.data[c.desc[r, 0]:c.desc[r, 0] + n] = 0xFF
    c = variant("lone-ff-at-the-end")
    c.data[c.desc[r, 0] + n - 1] = 0xFF
    c = variant("all-zero-bits")
    c.data[c.desc[r, 0]:c.desc[r, 0] + n] = 0
    for label, col, value in (("in-off-negative", 0, -1), ("in-off-past-the-data", 0, len(base.data) + 1), ("in-len-past-the-data", 1, len(base.data)),
                              ("in-len-negative", 1, -5), ("in-len-huge", 1, 2 ** 62), ("image-past-the-batch", 2, 3), ("image-negative", 2, -1),
                              ("first-mcu-past-the-image", 3, 9), ("first-mcu-negative", 3, -2), ("n-mcus-past-the-image", 4, 9),
                              ("n-mcus-zero", 4, 0), ("n-mcus-huge", 4, 2 ** 40), ("table-set-past-the-sets", 5, 7), ("table-set-negative", 5, -1)):
        c = variant(label)
        c.desc[rows[1], col] = value
    c = variant("interval-missing")                                         # image 1 loses an interval: its MCUs are not covered
    c.desc = np.delete(c.desc, rows[2], axis=0)
    for label, where, value in (("huffman-bits-all-255", slice(64, 80), 255), ("huffman-oversubscribed", 64 + 272, 3),   # 3 AC codes of one bit
                                ("steps-of-255", slice(0, 64), 255)):
        c = variant(label)                                                  # image 1 gets a table set of its own, then the damage
        c.tables = np.concatenate([c.tables, c.tables[int(base.desc[rows[0], 5])][None]])
        c.desc[rows, 5] = len(c.tables) - 1
        c.tables[-1, where] = value
    return out


def host_program(directory):
    """csrc/host/jpeg_decode_host_main.cpp compiled with the host sanitizers -> the program's path."""
    import shutil
    import subprocess
    from streamflow_amd import build
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(repo, "streamflow_amd", "csrc", "host", "jpeg_decode_host_main.cpp")
    cands = [os.path.join(os.path.dirname(os.path.realpath(build.hipcc())), "..", "lib", "llvm", "bin", "clang++"),
             "/opt/rocm/lib/llvm/bin/clang++"]
    cc = next((c for c in cands if os.path.exists(c)), None) or shutil.which("clang++")
    assert cc, "the ROCm clang++ is needed to build the host program"
    exe = os.path.join(str(directory), "jpeg_decode_host")
    r = subprocess.run([cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", src,
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_host(exe, calls, directory, tag):
    """[Call] -> [(status int32 [n], interval status int32 [n_intervals], coefficients int16 [n, blocks, 64])]; the run must be clean:
    exit code 0, no sanitizer report."""
    import struct
    import subprocess
    fin, fout = os.path.join(str(directory), f"{tag}.in"), os.path.join(str(directory), f"{tag}.out")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(calls)))
        for c in calls:
            f.write(struct.pack("<8iq", c.h, c.w, c.nc, c.hs, c.vs, c.n, len(c.desc), len(c.tables), len(c.data)))
            f.write(c.data.tobytes() + np.ascontiguousarray(c.desc, np.int64).tobytes() + np.ascontiguousarray(c.tables, np.uint8).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-4000:])
    res, at, out = np.fromfile(fout, np.uint8), 0, []
    for c in calls:
        ncoef = c.n * c.image_blocks() * 64
        status = res[at:at + 4 * c.n].view(np.int32)
        ist = res[at + 4 * c.n:at + 4 * (c.n + len(c.desc))].view(np.int32)
        at += 4 * (c.n + len(c.desc))
        out.append((status.copy(), ist.copy(), res[at:at + 2 * ncoef].view(np.int16).reshape(c.n, -1, 64).copy()))
        at += 2 * ncoef
    assert at == len(res)
    return out
