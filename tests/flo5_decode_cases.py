"""The cases of the .flo5 device reader (csrc/inflate_core.h, csrc/flo5_decode.hip, flo5_gpu.read_batch), shared by
tests/test_flo5_decode_cases_cpu.py, tests/test_inflate_core_host_cpu.py, tests/test_gpu_flo5_decode.py and
tools/flo5_decode_bench.py.  No GPU in here.

* inflate_ref: RFC 1950 / 1951 restated in plain Python with sf_inflate's status words, and a report of what a stream contained.
* good_streams(): zlib's output over levels, strategies and flushes, this project's own Huffman-only chunk streams, and two streams
  assembled by hand for what zlib never emits (a distance of exactly 32 768); bad_streams(): a fixed list, each derived from a good one.
* assemble_ref: sf_flo5_assemble in numpy; tiled_file: an HDF5 file around tiled chunks with a multi-level chunk B-tree."""
import struct
import zlib

import numpy as np

from streamflow_amd import flo5

OK, BAD_HEADER, TRUNCATED, BAD_BLOCK_TYPE, BAD_CODE_LENGTHS, BAD_SYMBOL, BAD_DISTANCE, OUTPUT_LONG, OUTPUT_SHORT, BAD_ADLER, \
    BAD_STORED_LEN, PRESET_DICT, BAD_SLOT = range(13)
STATUS_NAMES = ("OK", "BAD_HEADER", "TRUNCATED", "BAD_BLOCK_TYPE", "BAD_CODE_LENGTHS", "BAD_SYMBOL", "BAD_DISTANCE", "OUTPUT_LONG",
                "OUTPUT_SHORT", "BAD_ADLER", "BAD_STORED_LEN", "PRESET_DICT", "BAD_SLOT")
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


class _Stop(Exception):
    def __init__(self, status):
        self.status = status


class _Bits:
    def __init__(self, data, pos):
        self.d, self.pos, self.buf, self.cnt = data, pos, 0, 0

    def take(self, n):
        while self.cnt < n:
            if self.pos >= len(self.d):
                raise _Stop(TRUNCATED)
            self.buf |= self.d[self.pos] << self.cnt
            self.pos += 1
            self.cnt += 8
        v = self.buf & ((1 << n) - 1)
        self.buf >>= n
        self.cnt -= n
        return v

    def unread(self):
        self.cnt -= self.cnt & 7
        self.pos -= self.cnt >> 3
        self.buf = self.cnt = 0


def _construct(lengths):
    """(count per length, symbols in canonical order, left): left 0 complete (or no codes), > 0 incomplete, < 0 over-subscribed."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    if count[0] == len(lengths):
        return count, [], 0
    left = 1
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            return count, [], left
    symbol = [s for l in range(1, 16) for s, sl in enumerate(lengths) if sl == l]
    return count, symbol, left


def _decode(b, count, symbol):
    code = first = index = 0
    for l in range(1, 16):
        code |= b.take(1)
        c = count[l]
        if code - c < first:
            return symbol[index + code - first]
        index += c
        first = (first + c) << 1
        code <<= 1
    raise _Stop(BAD_SYMBOL)


def _huffman_tables(lit_lengths, dist_lengths, check):
    """zlib's rule for a dynamic block (check): over-subscribed is an error, incomplete too unless it is one code of one bit.  The
    fixed distance code is incomplete by definition (30 of 32 codes)."""
    lc, ls, left = _construct(lit_lengths)
    if check and (left < 0 or (left > 0 and lc[0] + lc[1] != len(lit_lengths))):
        raise _Stop(BAD_CODE_LENGTHS)
    dc, ds, left = _construct(dist_lengths)
    if check and (left < 0 or (left > 0 and dc[0] + dc[1] != len(dist_lengths))):
        raise _Stop(BAD_CODE_LENGTHS)
    return lc, ls, dc, ds


def inflate_ref(stream, expect_len, report=None):
    """One zlib stream that must inflate to exactly expect_len bytes -> (bytes, status): sf_inflate's contract and status words
    (include/streamflow_hip.h), decided in the order csrc/inflate_core.h decides them.  On failure the bytes are what was produced
    before.  `report` (a dict) receives what the stream contained: "types" (set of BTYPE), "repeats" (set of 16 / 17 / 18),
    "max_code_len", "max_dist", "overlap" (a match with distance < length), "blocks", "empty_stored" (stored blocks with LEN 0),
    "max_stored_len"."""
    rep = {"types": set(), "repeats": set(), "max_code_len": 0, "max_dist": 0, "overlap": False, "blocks": 0, "empty_stored": 0,
           "max_stored_len": 0}
    d = bytes(stream)
    out = bytearray()
    try:
        if len(d) < 2:
            raise _Stop(TRUNCATED)
        cmf, flg = d[0], d[1]
        if (cmf & 15) != 8 or (cmf >> 4) > 7 or (cmf * 256 + flg) % 31:
            raise _Stop(BAD_HEADER)
        if flg & 0x20:
            raise _Stop(PRESET_DICT)
        b = _Bits(d, 2)
        last = 0
        while not last:
            last, btype = b.take(1), b.take(2)
            if btype == 3:
                raise _Stop(BAD_BLOCK_TYPE)
            rep["blocks"] += 1
            rep["types"].add(btype)
            if btype == 0:
                b.unread()
                if len(d) - b.pos < 4:
                    raise _Stop(TRUNCATED)
                ln, nln = struct.unpack_from("<HH", d, b.pos)
                if ln ^ 0xFFFF != nln:
                    raise _Stop(BAD_STORED_LEN)
                b.pos += 4
                if ln > len(d) - b.pos:
                    raise _Stop(TRUNCATED)
                if ln > expect_len - len(out):
                    raise _Stop(OUTPUT_LONG)
                out += d[b.pos:b.pos + ln]
                b.pos += ln
                rep["empty_stored"] += ln == 0
                rep["max_stored_len"] = max(rep["max_stored_len"], ln)
                continue
            if btype == 1:
                lit_l, dist_l = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 30
            else:
                nlen, ndist, ncode = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                if nlen > 286 or ndist > 30:
                    raise _Stop(BAD_CODE_LENGTHS)
                cl = [0] * 19
                for i in range(ncode):
                    cl[CL_ORDER[i]] = b.take(3)
                cc, cs, left = _construct(cl)
                if left != 0 or cc[0] == 19:
                    raise _Stop(BAD_CODE_LENGTHS)
                lens = []
                while len(lens) < nlen + ndist:
                    sym = _decode(b, cc, cs)
                    if sym < 16:
                        lens.append(sym)
                        continue
                    rep["repeats"].add(sym)
                    if sym == 16:
                        if not lens:
                            raise _Stop(BAD_CODE_LENGTHS)
                        prev, n = lens[-1], 3 + b.take(2)
                    elif sym == 17:
                        prev, n = 0, 3 + b.take(3)
                    else:
                        prev, n = 0, 11 + b.take(7)
                    if len(lens) + n > nlen + ndist:
                        raise _Stop(BAD_CODE_LENGTHS)
                    lens += [prev] * n
                if lens[256] == 0:
                    raise _Stop(BAD_CODE_LENGTHS)
                lit_l, dist_l = lens[:nlen], lens[nlen:]
            lc, ls, dc, ds = _huffman_tables(lit_l, dist_l, btype == 2)
            if btype == 2:
                rep["max_code_len"] = max([rep["max_code_len"]] + lit_l + dist_l)
            while True:
                sym = _decode(b, lc, ls)
                if sym < 256:
                    if len(out) >= expect_len:
                        raise _Stop(OUTPUT_LONG)
                    out.append(sym)
                    continue
                if sym == 256:
                    break
                if sym - 257 >= 29:
                    raise _Stop(BAD_SYMBOL)
                ln = LEN_BASE[sym - 257] + (b.take(LEN_EXTRA[sym - 257]) if LEN_EXTRA[sym - 257] else 0)
                dsym = _decode(b, dc, ds)
                if dsym >= 30:
                    raise _Stop(BAD_SYMBOL)
                dist = DIST_BASE[dsym] + (b.take(DIST_EXTRA[dsym]) if DIST_EXTRA[dsym] else 0)
                if dist > len(out):
                    raise _Stop(BAD_DISTANCE)
                if ln > expect_len - len(out):
                    raise _Stop(OUTPUT_LONG)
                rep["max_dist"] = max(rep["max_dist"], dist)
                rep["overlap"] |= dist < ln
                if dist >= ln:
                    out += out[len(out) - dist:len(out) - dist + ln]
                else:
                    seed = bytes(out[len(out) - dist:])
                    out += (seed * (ln // dist + 1))[:ln]
        if len(out) != expect_len:
            raise _Stop(OUTPUT_SHORT)
        b.unread()
        if len(d) - b.pos < 4:
            raise _Stop(TRUNCATED)
        if int.from_bytes(d[b.pos:b.pos + 4], "big") != zlib.adler32(bytes(out)) & 0xFFFFFFFF:
            raise _Stop(BAD_ADLER)
        status = OK
    except _Stop as e:
        status = e.status
    if report is not None:
        report.update(rep)
    return bytes(out), status


def zlib_ok(stream, expect):
    """zlib itself inflates the stream completely and to exactly `expect` (bytes)."""
    do = zlib.decompressobj()
    try:
        got = do.decompress(bytes(stream))
    except zlib.error:
        return False
    return do.eof and got == expect


# ---- a deflate writer for what zlib never emits -------------------------------------------------------------------------------------
class _BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):                                     # n bits of v, least significant first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):                                    # a Huffman code: most significant bit first
        self.put(int(format(v, f"0{n}b")[::-1], 2), n)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def _fixed_lit(w, sym):
    if sym < 144:
        w.code(0x30 + sym, 8)
    elif sym < 256:
        w.code(0x190 + sym - 144, 9)
    elif sym < 280:
        w.code(sym - 256, 7)
    else:
        w.code(0xC0 + sym - 280, 8)


def fixed_stream(tokens, data):
    """A zlib stream of ONE fixed-Huffman block from tokens -- a byte value, or (length, distance) -- with the Adler-32 of `data`."""
    w = _BitWriter()
    w.put(1, 1)
    w.put(1, 2)
    for t in tokens:
        if isinstance(t, tuple):
            ln, dist = t
            ls = max(i for i in range(29) if LEN_BASE[i] <= ln and (i == 28 or ln < 258))
            _fixed_lit(w, 257 + ls)
            w.put(ln - LEN_BASE[ls], LEN_EXTRA[ls])
            dsym = max(i for i in range(30) if DIST_BASE[i] <= dist)
            w.code(dsym, 5)
            w.put(dist - DIST_BASE[dsym], DIST_EXTRA[dsym])
        else:
            _fixed_lit(w, int(t))
    _fixed_lit(w, 256)
    return b"\x78\x01" + w.done() + (zlib.adler32(bytes(data)) & 0xFFFFFFFF).to_bytes(4, "big")


# ---- good streams -----------------------------------------------------------------------------------------------------------------
def _z(data, level, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=()):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    out, prev = b"", 0
    for cut in flush_at:
        out += co.compress(data[prev:cut]) + co.flush(zlib.Z_FULL_FLUSH)
        prev = cut
    return out + co.compress(data[prev:]) + co.flush()


def float_like(n, seed):
    """n bytes of what a Spring chunk holds: one channel of a smooth float32 field with a little noise and NaN holes."""
    rng = np.random.default_rng(seed)
    k = -(-n // 4)
    v = (7 * np.sin(np.arange(k) / 37.0) + np.arange(k) / 900.0 + rng.normal(0, 0.01, k)).astype("<f4")
    v[rng.random(k) < 0.03] = np.nan
    v[100:400] = np.nan
    return v.tobytes()[:n]


_GOOD = None


def good_streams():
    """[(name, stream, data)], built once."""
    global _GOOD
    if _GOOD is not None:
        return _GOOD
    from tests import flo5_encode_cases as ec
    rng = np.random.default_rng(7)
    strategies = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE}
    text = (b"the quick brown fox jumps over the lazy dog; " * 40 + bytes(rng.integers(0, 256, 700, dtype=np.uint8)) + b"\0" * 300 +
            bytes(rng.integers(97, 105, 900, dtype=np.uint8)))
    out = []
    small = {"empty": b"", "one": b"\x5a", "n64": bytes(range(64)), "n65": bytes(rng.integers(0, 4, 65, dtype=np.uint8)), "text": text}
    for dn, data in small.items():
        for level in (0, 1, 5, 9):
            for sn, st in strategies.items():
                out.append((f"{dn}-l{level}-{sn}", _z(data, level, st), data))
    out.append(("text-flushes", _z(text, 5, flush_at=(0, 100, 100, 1500, len(text))), text))
    chunk = float_like(65280, 1)                                              # a Spring chunk: (68, 240, 1) float32
    for level in (1, 5, 9):
        out.append((f"chunk-l{level}", _z(chunk, level), chunk))
    out.append(("chunk-l5-flushes", _z(chunk, 5, flush_at=(20000, 40000)), chunk))
    noise = bytes(rng.integers(0, 256, 70000, dtype=np.uint8))
    out.append(("noise-l0", _z(noise, 0), noise))                            # stored blocks, as long as zlib's buffers make them
    by_hand = b"\x78\x01" + b"\x00\xff\xff\x00\x00" + noise[:65535] + b"\x00\x00\x00\xff\xff" + \
        b"\x01" + struct.pack("<HH", 70000 - 65535, (70000 - 65535) ^ 0xFFFF) + noise[65535:] + (zlib.adler32(noise) & 0xFFFFFFFF).to_bytes(4, "big")
    out.append(("noise-stored-65535", by_hand, noise))                       # LEN = 65535, an empty block, the rest
    run = b"\x07" * 5000
    out.append(("run-l9", _z(run, 9), run))                                  # distance 1, length 258
    motif = bytes(rng.integers(0, 256, 300, dtype=np.uint8))
    far = motif + bytes(rng.integers(0, 256, 32768 - 300, dtype=np.uint8)) + motif + bytes(rng.integers(0, 256, 40000 - 32768 - 300, dtype=np.uint8))
    out.append(("far-l9", _z(far, 9), far))
    # zlib keeps its matches within 32 768 - 262 bytes; the full distance by hand: 32 768 literals, then a match back to the first
    head = bytes(rng.integers(0, 256, 32768, dtype=np.uint8))
    data = head + head[:258] + head[258:300]
    out.append(("dist-32768-fixed", fixed_stream(list(head) + [(258, 32768), (42, 32768)], data), data))
    counts = [1, 1]
    while len(counts) < 24:
        counts.append(counts[-1] + counts[-2])                                # Fibonacci counts: code lengths past 15 before the limit
    skew = np.repeat(np.arange(len(counts), dtype=np.uint8) * 9 + 3, counts)
    rng.shuffle(skew)
    out.append(("skew-l9-huffman", _z(skew.tobytes(), 9, zlib.Z_HUFFMAN_ONLY), skew.tobytes()))
    # what this project's GPU writer emits (tests/flo5_encode_cases.chunk_stream_ref: shuffled planes, Huffman-only blocks)
    for (h, w, rpc), special in (((37, 53, 2), True), ((64, 512, 64), False)):
        f = ec.make(h, w, 5, special)
        for c in sorted({0, -(-h // rpc) - 1}):
            out.append((f"writer-{h}x{w}-c{c}", ec.chunk_stream_ref(f, c, rpc), ec.shuffled(f, c, rpc).tobytes()))
    _GOOD = out
    return out


def good(name):
    return next((s, d) for n, s, d in good_streams() if n == name)


def features():
    """What the good list contains as a whole, from inflate_ref's reports."""
    tot = {"types": set(), "repeats": set(), "max_code_len": 0, "max_dist": 0, "overlap": False, "blocks": 0, "empty_stored": 0,
           "max_stored_len": 0, "zero_output": False}
    for _, s, d in good_streams():
        rep = {}
        got, st = inflate_ref(s, len(d), rep)
        assert st == OK and got == d
        tot["types"] |= rep["types"]
        tot["repeats"] |= rep["repeats"]
        for k in ("max_code_len", "max_dist", "blocks", "max_stored_len"):
            tot[k] = max(tot[k], rep[k])
        tot["overlap"] |= rep["overlap"]
        tot["empty_stored"] += rep["empty_stored"]
        tot["zero_output"] |= len(d) == 0
    return tot


# ---- bad streams ------------------------------------------------------------------------------------------------------------------
def bad_streams():
    """[(name, stream, expected length, status)]: a fixed list, each entry derived from a good stream."""
    text_s, text = good("text-l5-default")
    fix_s, _ = good("text-l5-fixed")
    st_s, st_d = good("n64-l0-default")
    flip = lambda s, i, m=0xFF: s[:i] + bytes([s[i] ^ m]) + s[i + 1:]
    # 19 code-length codes of one bit each: HLIT = 0, HDIST = 0, HCLEN = 15, then 19 x `001`
    w = _BitWriter()
    w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(15, 4)
    for _ in range(19):
        w.put(1, 3)
    over = text_s[:2] + w.done() + text_s[-8:]
    fdict = bytes([0x78, 0x20 | (31 - (0x78 * 256 + 0x20) % 31)])
    return [
        ("truncated-after-header", text_s[:2], len(text), TRUNCATED),
        ("truncated-mid-block", text_s[:len(text_s) // 2], len(text), TRUNCATED),
        ("truncated-before-trailer", text_s[:-4], len(text), TRUNCATED),
        ("block-type-3", text_s[:2] + b"\x07" + text_s[3:], len(text), BAD_BLOCK_TYPE),
        ("distance-before-start", fixed_stream([65, (3, 2)], b"AAAA"), 4, BAD_DISTANCE),
        ("oversubscribed-code-lengths", over, len(text), BAD_CODE_LENGTHS),
        ("stored-nlen-mismatch", flip(st_s, 5), len(st_d), BAD_STORED_LEN),
        ("expected-one-more", text_s, len(text) + 1, OUTPUT_SHORT),
        ("expected-one-less", fix_s, len(text) - 1, OUTPUT_LONG),
        ("adler-flipped", flip(text_s, len(text_s) - 2, 0x10), len(text), BAD_ADLER),
        ("fdict", fdict + text_s[2:], len(text), PRESET_DICT),
        ("header-check", flip(text_s, 1, 0x01), len(text), BAD_HEADER),
    ]


# ---- sf_flo5_assemble in numpy, and files to feed it ---------------------------------------------------------------------------------
def assemble_ref(shape, chunk_shape, shuffle, chunks):
    """chunks: {(gy, gx, gc): the inflated chunk's bytes} -> uint32 [H, W, 2]: 0 where a chunk is missing, padding dropped."""
    (H, W, _), (ch, cw, cc) = shape, chunk_shape
    out = np.zeros((H, W, 2), np.uint32)
    n = ch * cw * cc
    for (gy, gx, gc), raw in chunks.items():
        b = np.frombuffer(raw, np.uint8)[:4 * n]
        if shuffle:
            b = np.ascontiguousarray(b.reshape(4, n).T)
        tile = b.reshape(-1).view("<u4").reshape(ch, cw, cc)
        y0, x0, c0 = gy * ch, gx * cw, gc * cc
        hh, ww = min(ch, H - y0), min(cw, W - x0)
        out[y0:y0 + hh, x0:x0 + ww, c0:c0 + cc] = tile[:hh, :ww]
    return out


def table_chunks(table):
    """A chunk_table's chunks inflated with zlib: {(gy, gx, gc): bytes}, filter masks honoured (deflate is the last stage)."""
    cs = table["chunk_shape"]
    deflate = len(table["filters"]) - 1
    out = {}
    for offs, addr, nbytes, mask in table["chunks"]:
        raw = table["data"][addr:addr + nbytes]
        out[tuple(o // c for o, c in zip(offs, cs))] = raw if mask >> deflate & 1 else zlib.decompress(raw)
    return out


def tiled_file(array, chunk_shape, level=5, shuffle=False, skip_deflate=(), missing=(), leaf_k=3):
    """The bytes of an HDF5 file with dataset 'flow' = array (float32 [H, W, 2]) in chunks of chunk_shape, h5py's layout in small:
    every chunk a zlib stream at `level` behind a chunk B-tree of at most leaf_k entries per node (so a handful of chunks already
    make a tree of several levels).  skip_deflate: grid positions (gy, gx, gc) stored without the deflate stage (filter mask bit
    set); missing: positions left out of the file (their elements must read 0).  The container is flo5.flo5_file's, field for field
    (the tables are the specification's), with another layout message and chunk index."""
    a = np.ascontiguousarray(array, "<f4")
    H, W, _ = a.shape
    ch, cw, cc = chunk_shape
    U = flo5.UNDEF
    entries = []                                                             # (offsets, mask, stored bytes)
    for gy in range(-(-H // ch)):
        for gx in range(-(-W // cw)):
            for gc in range(2 // cc):
                if (gy, gx, gc) in missing:
                    continue
                buf = np.zeros((ch, cw, cc), "<f4")
                part = a[gy * ch:(gy + 1) * ch, gx * cw:(gx + 1) * cw, gc * cc:(gc + 1) * cc]
                buf[:part.shape[0], :part.shape[1]] = part
                raw = buf.tobytes()
                if shuffle:
                    raw = np.frombuffer(raw, np.uint8).reshape(-1, 4).T.tobytes()
                skip = (gy, gx, gc) in skip_deflate
                mask = (2 if shuffle else 1) if skip else 0
                entries.append(((gy * ch, gx * cw, gc * cc), mask, raw if skip else zlib.compress(raw, level)))
    off_root, off_bt = 96, 96 + 40
    off_heap = off_bt + 544
    off_hd, off_snod = off_heap + 32, off_heap + 64
    off_dset = off_snod + 328
    space = struct.pack("<BBB5x", 1, 3, 0) + struct.pack("<3Q", H, W, 2)
    deflate = struct.pack("<HHHH", 1, 8, 1, 1) + b"deflate\0" + struct.pack("<I4x", int(level))
    if shuffle:
        pipeline = struct.pack("<BB6x", 1, 2) + struct.pack("<HHHH", 2, 8, 1, 1) + b"shuffle\0" + struct.pack("<I4x", 4) + deflate
    else:
        pipeline = struct.pack("<BB6x", 1, 1) + deflate
    msgs = [flo5._message(1, space), flo5._message(3, flo5._float32_datatype(), 1), flo5._message(0xB, pipeline, 1)]
    hdr_size = 16 + sum(len(m) for m in msgs) + 8 + 32
    off_tree = off_dset + hdr_size
    # the nodes of the chunk B-tree, level by level; node size is that of a libhdf5 node with 64 entries
    ksz, node_size = 8 + 8 * 4, 24 + 64 * 8 + 65 * (8 + 8 * 4)
    end_key = ((-(-H // ch)) * ch, 0, 0)
    key = lambda nbytes, mask, offs: struct.pack("<II4Q", nbytes, mask, *offs, 0)
    levels = [[(e[0], e[1], len(e[2])) for e in entries]]                    # levels[L]: (first key offsets, mask, nbytes) of the children of level L
    while True:
        prev = levels[-1]
        levels.append([prev[i] for i in range(0, len(prev), leaf_k)])        # one item per node of this level
        if len(levels[-1]) <= 1:
            break
    # node addresses: level 1 nodes (leaves) first, the root last; chunk data behind all nodes
    n_nodes = [len(l) for l in levels[1:]]
    node_addr, pos = [], off_tree
    for n in n_nodes:
        node_addr.append([pos + i * node_size for i in range(n)])
        pos += n * node_size
    chunk_addr, p = [], pos
    for e in entries:
        chunk_addr.append(p)
        p += len(e[2])
    eof = p
    nodes = b""
    for lv, n in enumerate(n_nodes):
        children, addrs = levels[lv], (chunk_addr if lv == 0 else node_addr[lv - 1])
        for i in range(n):
            kids = list(range(i * leaf_k, min((i + 1) * leaf_k, len(children))))
            nd = struct.pack("<4sBBHQQ", b"TREE", 1, lv, len(kids), U, U)
            for k in kids:
                offs, mask, nbytes = children[k]
                nd += key(nbytes, mask, offs) + struct.pack("<Q", addrs[k])
            nxt = kids[-1] + 1
            nd += key(0, 0, children[nxt][0] if nxt < len(children) else end_key)
            nodes += nd.ljust(node_size, b"\0")
    root_addr = node_addr[-1][0] if entries else U
    layout = struct.pack("<BBB", 3, 2, 4) + struct.pack("<Q", root_addr) + struct.pack("<4I", ch, cw, cc, 4)
    hdr = flo5._object_header(msgs + [flo5._message(8, layout)])
    assert len(hdr) == hdr_size and (not entries or len(levels[-1]) == 1)
    sup = (flo5.SIGNATURE + bytes([0, 0, 0, 0, 0, 8, 8, 0]) + struct.pack("<HHI", 4, 16, 0) + struct.pack("<4Q", 0, U, eof, U) +
           struct.pack("<QQII", 0, off_root, 1, 0) + struct.pack("<QQ", off_bt, off_heap))
    root = flo5._object_header([flo5._message(0x11, struct.pack("<QQ", off_bt, off_heap))])
    gb = (struct.pack("<4sBBHQQ", b"TREE", 0, 0, 1, U, U) + struct.pack("<QQQ", 0, off_snod, 8)).ljust(544, b"\0")
    heap = struct.pack("<4sB3xQQQ", b"HEAP", 0, 32, 16, off_hd)
    hd = b"\0" * 8 + b"flow\0\0\0\0" + struct.pack("<QQ", 1, 16)
    snod = (struct.pack("<4sBxH", b"SNOD", 1, 1) + struct.pack("<QQII16x", 8, off_dset, 0, 0)).ljust(328, b"\0")
    data = sup + root + gb + heap + hd + snod + hdr + nodes + b"".join(e[2] for e in entries)
    assert len(data) == eof
    return data


def smooth_field(h, w, seed, holes=True):
    """float32 [h, w, 2]: smooth waves, a little noise, NaN holes (Spring marks invalid pixels so) with a few payload bit patterns."""
    from tests import flo5_encode_cases as ec
    f = np.ascontiguousarray(ec.make(h, w, seed).transpose(1, 2, 0))
    if holes:
        rng = np.random.default_rng(seed + 1)
        f[rng.random((h, w)) < 0.05] = np.nan
        f[h // 3:h // 3 + max(1, h // 5), w // 4:w // 4 + max(1, w // 3)] = np.nan
        bits = f.view(np.uint32).reshape(-1)
        bits[::97] = ec.SPECIALS[np.arange(bits[::97].size) % len(ec.SPECIALS)]
    return f
