"""Baseline JPEG files <-> device images.

Encoding: the colour conversion, the DCT, the quantisation and the Huffman coding of a whole batch are one sf_jpeg_encode call
(csrc/jpeg_encode.hip); only the entropy-coded segments cross to the host, where `jpeg_file` puts the marker segments around them:
SOI, APP0 (JFIF 1.01), DQT, SOF0 (4:4:4), the four typical Huffman tables of T.81 Annex K.3 as DHT, DRI (one restart interval per MCU
row), SOS, the segment, EOI.  The files are what avi.MjpegWriter takes as frames.

Decoding: `parse` walks a file's marker segments on the host (geometry, tables, where its restart intervals lie); `decode_batch`
uploads the entropy-coded bytes of a batch of files of one geometry as they are and one sf_jpeg_decode call (csrc/jpeg_decode.hip)
makes them uint8 [n, H, W, 3] on the device: Huffman decoding a wave per restart interval, libjpeg's integer inverse DCT, its
"fancy" chroma upsampling and the YCbCr -> RGB conversion -- bit for bit what libjpeg-turbo gives.  Baseline sequential files only
(SOF0, 8 bit, Huffman, one scan; grey or YCbCr at 4:4:4, 4:2:2 or 4:2:0); anything else raises UnsupportedJpeg.

There is no fallback: without a GPU `encode_batch` and `decode_batch` raise.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from .png_gpu import pool_threads

# T.81 Annex K.1: the luminance and chrominance quantisation tables, natural (row-major) order
K1_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
           100, 103, 99)
K1_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) \
    + (99,) * 32

# scan position k -> natural index
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
          57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)

# T.81 Annex K.3: (table class << 4 | destination, BITS, HUFFVAL) in the order the DHT segments are written
_AC_LUMA = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a43444546474849"
    "4a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
    "c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN_TABLES = ((0x00, bytes((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)), bytes(range(12))),
                  (0x10, bytes((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125)), _AC_LUMA),
                  (0x01, bytes((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)), bytes(range(12))),
                  (0x11, bytes((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119)), _AC_CHROMA))


def quant_tables(quality: int) -> np.ndarray:
    """uint16 [2, 64], natural order: the Annex K.1 tables scaled as the IJG library scales them (jpeg_quality_scaling):
    s = 5000 // quality below 50, else 200 - 2 quality; (t s + 50) // 100 clamped to 1 .. 255.  quality: 1 .. 100."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"jpeg quality must be in 1 .. 100, got {quality}")
    s = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([K1_LUMA, K1_CHROMA], np.int64)
    return np.clip((base * s + 50) // 100, 1, 255).astype(np.uint16)


def _check_tables(qtables) -> np.ndarray:
    q = np.ascontiguousarray(np.asarray(qtables)).reshape(-1)
    if q.size != 128 or q.min() < 1 or q.max() > 255:
        raise ValueError("qtables: two tables of 64 steps in 1 .. 255 (natural order)")
    return q.astype(np.uint16).reshape(2, 64)


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes((0xFF, marker)) + (len(payload) + 2).to_bytes(2, "big") + payload


def dht_segments(channels: int = 3) -> List[bytes]:
    """The DHT marker segments of a file: DC and AC luma, and for colour DC and AC chroma; one table per segment."""
    return [_segment(0xC4, bytes((tc,)) + bits + vals) for tc, bits, vals in HUFFMAN_TABLES[:4 if channels == 3 else 2]]


def jpeg_file(segment: bytes, h: int, w: int, channels: int, qtables) -> bytes:
    """The JFIF file around one entropy-coded segment of sf_jpeg_encode (h x w, channels 1 or 3, the qtables it was made with)."""
    if channels not in (1, 3) or not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"jpeg_file: h = {h}, w = {w}, channels = {channels}")
    q = _check_tables(qtables)
    nt = 2 if channels == 3 else 1
    parts = [b"\xff\xd8", _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    parts += [_segment(0xDB, bytes((t,)) + bytes(int(q[t, z]) for z in ZIGZAG)) for t in range(nt)]
    comps = b"".join(bytes((c + 1, 0x11, 1 if c else 0)) for c in range(channels))
    parts.append(_segment(0xC0, b"\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes((channels,)) + comps))
    parts += dht_segments(channels)
    parts.append(_segment(0xDD, ((w + 7) // 8).to_bytes(2, "big")))
    scan = b"".join(bytes((c + 1, 0x11 if c else 0x00)) for c in range(channels))
    parts.append(_segment(0xDA, bytes((channels,)) + scan + b"\x00\x3f\x00"))
    parts += [bytes(segment), b"\xff\xd9"]
    return b"".join(parts)


def encode_batch(images: torch.Tensor, paths: Optional[Sequence[str]] = None, quality: int = 90,
                 threads: Optional[int] = None) -> List[bytes]:
    """Device images uint8 [n, H, W, 3] or [n, H, W] -> n JPEG files as bytes (written to `paths` where given), at the IJG quality
    `quality`.  One ops.jpeg_encode call on the current stream; the n segment lengths are copied first, then only the used bytes of
    every slot (pinned memory); the framing and the file writes run in the thread pool."""
    from . import ops
    if not isinstance(images, torch.Tensor) or images.dim() not in (3, 4) or images.shape[0] == 0:
        raise ValueError(f"jpeg_gpu.encode_batch: images [n, H, W, 3] or [n, H, W] (got {getattr(images, 'shape', type(images).__name__)})")
    if paths is not None:
        paths = list(paths)
        if len(paths) != images.shape[0]:
            raise ValueError(f"jpeg_gpu.encode_batch: {images.shape[0]} images, {len(paths)} paths")
    if not images.is_cuda or not torch.cuda.is_available():
        raise RuntimeError(f"jpeg_gpu encodes on the GPU (device {images.device}, GPU available: {torch.cuda.is_available()}); "
                           "there is no CPU fallback")
    n, h, w = (int(v) for v in images.shape[:3])
    channels = 3 if images.dim() == 4 else 1
    q = quant_tables(quality)
    segments, lengths = ops.jpeg_encode(images, q)
    used = [int(v) for v in lengths.cpu()]
    start = [sum(used[:i]) for i in range(n)]
    host = torch.empty(sum(used), dtype=torch.uint8, pin_memory=True)
    for i in range(n):
        host[start[i]:start[i] + used[i]].copy_(segments[i, :used[i]], non_blocking=True)
    torch.cuda.current_stream(images.device).synchronize()
    data = host.numpy()

    def frame(i: int) -> bytes:
        blob = jpeg_file(data[start[i]:start[i] + used[i]].tobytes(), h, w, channels, q)
        if paths is not None:
            with open(paths[i], "wb") as f:
                f.write(blob)
        return blob

    k = min(pool_threads(threads), n)
    if k == 1:
        return [frame(i) for i in range(n)]
    with ThreadPoolExecutor(max_workers=k) as ex:
        return list(ex.map(frame, range(n)))


# ---- decoding ---------------------------------------------------------------------------------------------------------------------------
class UnsupportedJpeg(ValueError):
    """A well-formed JPEG file outside the subset sf_jpeg_decode takes (progressive, arithmetic, 12 bit, CMYK, RGB, several scans,
    other sampling factors, DNL)."""


DESC_WORDS, TABLE_SET_BYTES, SPEC_BYTES = 6, 1824, 272
DECODE_STATUS = ("ok", "bits that are no Huffman code", "run past coefficient 63", "coefficient category out of range",
                 "truncated restart interval", "restart interval not fully consumed", "descriptor outside the buffers",
                 "coefficient out of range", "bad Huffman table", "marker inside a restart interval")
_SOF_NAMES = {0xC1: "extended sequential", 0xC2: "progressive", 0xC3: "lossless", 0xC5: "differential sequential",
              0xC6: "differential progressive", 0xC7: "differential lossless", 0xC8: "JPG extension", 0xC9: "arithmetic sequential",
              0xCA: "arithmetic progressive", 0xCB: "arithmetic lossless", 0xCC: "arithmetic conditioning (DAC)",
              0xCD: "arithmetic differential sequential", 0xCE: "arithmetic differential progressive", 0xCF: "arithmetic differential lossless"}


class Parsed(NamedTuple):
    """What `parse` finds in a file.  intervals: (offset into the file, length, first MCU, MCUs) per restart interval, the bytes still
    stuffed; table_set: the SF_JPEG_TABLE_SET_BYTES record of its tables (per component 64 steps in natural order, DC and AC
    specification as 16 BITS + 256 HUFFVAL)."""
    h: int
    w: int
    components: int
    hs: int
    vs: int
    table_set: bytes
    intervals: Tuple[Tuple[int, int, int, int], ...]


def _spec(bits: bytes, vals: bytes) -> bytes:
    return bytes(bits) + bytes(vals) + bytes(256 - len(vals))


_DEFAULT_HUFFMAN = {(tc >> 4, tc & 15): _spec(bits, vals) for tc, bits, vals in HUFFMAN_TABLES}
_UNZIGZAG = np.argsort(np.array(ZIGZAG))                                 # natural index -> scan position


def parse(blob: bytes, name: str = "JPEG data") -> Parsed:
    """The marker walk of one file: SOI, APPn, DQT (8-bit tables), SOF0, DHT, DRI, SOS, then the entropy-coded data up to EOI, whose
    RSTm markers are found by one vectorised scan and checked for their numbering.  COM and unknown APPn segments are skipped, FF
    fill bytes in front of a marker and bytes after EOI tolerated.  A frame without DHT (common in AVI files) gets the Annex K.3
    tables.  UnsupportedJpeg for a well-formed file outside the decoder's subset, ValueError (naming `name`) for broken framing."""
    blob = bytes(blob)
    n = len(blob)

    def bad(msg):
        return ValueError(f"{name}: {msg}")

    if n < 4 or blob[:2] != b"\xff\xd8":
        raise bad("not a JPEG file (no SOI)")
    quant, huff, frame, restart, adobe, pos = {}, {}, None, 0, None, 2
    while True:
        if pos + 2 > n:
            raise bad("the file ends before SOS")
        if blob[pos] != 0xFF:
            raise bad(f"byte {blob[pos]:#04x} at {pos} where a marker should start")
        while pos + 1 < n and blob[pos + 1] == 0xFF:                     # fill bytes
            pos += 1
        if pos + 2 > n:
            raise bad("the file ends before SOS")
        marker = blob[pos + 1]
        if marker == 0x01 or marker == 0x00:
            raise bad(f"marker FF {marker:02X} at {pos} outside entropy-coded data")
        if 0xD0 <= marker <= 0xD9:
            raise bad(f"marker FF {marker:02X} at {pos} before SOS")
        if pos + 4 > n:
            raise bad("a marker segment crosses the end of the file")
        size = int.from_bytes(blob[pos + 2:pos + 4], "big")
        if size < 2 or pos + 2 + size > n:
            raise bad(f"segment FF {marker:02X} at {pos}: length {size} crosses the end of the file")
        seg, pos = blob[pos + 4:pos + 2 + size], pos + 2 + size
        if marker in _SOF_NAMES:
            raise UnsupportedJpeg(f"{name}: {_SOF_NAMES[marker]} JPEG (only baseline sequential, SOF0)")
        if marker == 0xDC:
            raise UnsupportedJpeg(f"{name}: DNL marker")
        if marker == 0xDB:
            at = 0
            while at < len(seg):
                pq, tq = seg[at] >> 4, seg[at] & 15
                if pq != 0:
                    raise UnsupportedJpeg(f"{name}: 16-bit quantisation table")
                if tq > 3 or at + 65 > len(seg):
                    raise bad("bad DQT segment")
                quant[tq] = bytes(np.frombuffer(seg[at + 1:at + 65], np.uint8)[_UNZIGZAG])
                at += 65
        elif marker == 0xC4:
            at = 0
            while at < len(seg):
                if at + 17 > len(seg):
                    raise bad("bad DHT segment")
                tc, th, bits = seg[at] >> 4, seg[at] & 15, seg[at + 1:at + 17]
                count = sum(bits)
                if tc > 1 or th > 3 or count > 256 or at + 17 + count > len(seg):
                    raise bad("bad DHT segment")
                code = 0
                for length, k in enumerate(bits, start=1):
                    code += k
                    if code > 1 << length:
                        raise bad("DHT: more codes of a length than the length has patterns")
                    code <<= 1
                huff[(tc, th)] = _spec(bits, seg[at + 17:at + 17 + count])
                at += 17 + count
        elif marker == 0xDD:
            if len(seg) != 2:
                raise bad("bad DRI segment")
            restart = int.from_bytes(seg, "big")
        elif marker == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif marker == 0xC0:
            if frame is not None:
                raise bad("two frame headers")
            if len(seg) < 6 or len(seg) != 6 + 3 * seg[5]:
                raise bad("bad SOF0 segment")
            if seg[0] != 8:
                raise UnsupportedJpeg(f"{name}: {seg[0]}-bit samples")
            h, w, nf = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"), seg[5]
            if h == 0:
                raise UnsupportedJpeg(f"{name}: height 0 (to be set by a DNL marker)")
            if w == 0:
                raise bad("width 0")
            if nf not in (1, 3):
                raise UnsupportedJpeg(f"{name}: {nf} components (1 or 3)")
            frame = (h, w, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)])
        elif marker == 0xDA:
            break
    if frame is None:
        raise bad("SOS before the frame header")
    h, w, comps = frame
    nc = len(comps)
    if len(seg) != 4 + 2 * seg[0] if seg else True:
        raise bad("bad SOS segment")
    if seg[0] != nc:
        raise UnsupportedJpeg(f"{name}: a scan of {seg[0]} of the {nc} components (several scans)")
    if (seg[1 + 2 * nc], seg[2 + 2 * nc], seg[3 + 2 * nc]) != (0, 63, 0):
        raise UnsupportedJpeg(f"{name}: spectral selection / successive approximation in a sequential scan")
    if nc == 3:
        if adobe == 0 or bytes(c[0] for c in comps) == b"RGB":
            raise UnsupportedJpeg(f"{name}: RGB components (Adobe transform 0 or component ids R, G, B)")
        if any((ch, cv) != (1, 1) for _, ch, cv, _ in comps[1:]) or (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)):
            raise UnsupportedJpeg(f"{name}: sampling factors {[(c[1], c[2]) for c in comps]} (4:4:4, 4:2:2 or 4:2:0)")
    hs, vs = (comps[0][1], comps[0][2]) if nc == 3 else (1, 1)           # a scan of one component ignores its sampling factors
    records = []
    for i, (cid, _, _, tq) in enumerate(comps):
        if seg[1 + 2 * i] != cid:
            raise UnsupportedJpeg(f"{name}: the scan's components are not in the frame's order")
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        tabs = huff if huff else _DEFAULT_HUFFMAN
        if tq not in quant or (0, td) not in tabs or (1, ta) not in tabs:
            raise bad(f"component {cid} uses a table the file does not define")
        records.append(quant[tq] + tabs[(0, td)] + tabs[(1, ta)])
    table_set = b"".join(records) + bytes(TABLE_SET_BYTES - len(records) * (TABLE_SET_BYTES // 3))
    # the entropy-coded data: every FF that is followed by neither 00 nor FF starts a marker
    a = np.frombuffer(blob, np.uint8, offset=pos)
    ff = np.flatnonzero(a[:-1] == 0xFF) if len(a) > 1 else np.zeros(0, np.int64)
    follow = a[ff + 1]
    keep = (follow != 0) & (follow != 0xFF)
    at, codes = ff[keep], follow[keep]
    rst = (codes >= 0xD0) & (codes <= 0xD7)
    ends = np.flatnonzero(~rst)
    if len(ends) == 0:
        raise bad("no EOI behind the entropy-coded data")
    last = int(ends[0])
    if codes[last] == 0xDC:
        raise UnsupportedJpeg(f"{name}: DNL marker")
    if codes[last] != 0xD9:
        raise UnsupportedJpeg(f"{name}: marker FF {int(codes[last]):02X} behind the scan (several scans)")
    mcus = -(-w // (8 * hs)) * -(-h // (8 * vs))
    per = restart if restart else mcus
    count = -(-mcus // per)
    if last != count - 1:
        raise bad(f"{last} restart markers where {count - 1} are due (DRI = {restart}, {mcus} MCUs)")
    if last and not np.array_equal(codes[:last], 0xD0 + np.arange(last) % 8):
        k = int(np.argmax(codes[:last] != 0xD0 + np.arange(last) % 8))
        raise bad(f"restart marker {k} is FF {int(codes[k]):02X}, not RST{k % 8}")
    intervals, start = [], 0
    for k in range(count):
        end = int(at[k])
        while end > start and a[end - 1] == 0xFF:                       # fill bytes in front of the marker
            end -= 1
        intervals.append((pos + start, end - start, k * per, min(per, mcus - k * per)))
        start = int(at[k]) + 2
    return Parsed(h, w, nc, hs, vs, table_set, tuple(intervals))


def pack(parsed: Sequence[Parsed], blobs: Sequence[bytes]):
    """The arguments of sf_jpeg_decode for files of one geometry: (data uint8 [B], desc int64 [n_intervals, 6], tables uint8 [n_sets,
    SF_JPEG_TABLE_SET_BYTES]) as numpy arrays: each file's entropy-coded bytes from its first interval to its last, the table sets
    de-duplicated."""
    sets, rows, chunks, base = {}, [], [], 0
    for i, (p, blob) in enumerate(zip(parsed, blobs)):
        lo, hi = p.intervals[0][0], p.intervals[-1][0] + p.intervals[-1][1]
        chunks.append(np.frombuffer(blob, np.uint8, count=hi - lo, offset=lo))
        s = sets.setdefault(p.table_set, len(sets))
        rows += [(base + off - lo, length, i, first, k, s) for off, length, first, k in p.intervals]
        base += hi - lo
    data = np.concatenate(chunks) if base else np.zeros(0, np.uint8)
    tables = np.frombuffer(b"".join(sets), np.uint8).reshape(len(sets), TABLE_SET_BYTES)
    return data, np.array(rows, np.int64).reshape(-1, DESC_WORDS), tables


# decode_batch(split="auto"): a restart interval of at least this many bytes is decoded a thread per segment (sf_jpeg_decode_split),
# a shorter one by one wave.  All of the project's own files (an interval per MCU row) stay below it.
SPLIT_MIN_BYTES = 16384
SPLIT_MODES = ("auto", "never", "always")


def decode_batch(blobs_or_paths: Sequence, device, threads: Optional[int] = None, names: Optional[Sequence[str]] = None,
                 split: str = "auto", segment_bytes: int = 128) -> torch.Tensor:
    """JPEG files (bytes, or paths that are read here) of ONE geometry -> uint8 [n, H, W, 3] on `device`, grey files with their sample
    three times.  split: "never" gives every restart interval one wave (sf_jpeg_decode); "always" decodes every interval a thread
    per segment of segment_bytes unstuffed bytes (sf_jpeg_decode_split: what a file without restart markers needs, since it is ONE
    interval); "auto" does that for the intervals of at least SPLIT_MIN_BYTES bytes.  The pixels are the same either way.  The files are read and parsed in the thread pool; the entropy-coded bytes, the descriptors and the tables go up in
    one copy from pinned memory; one ops.jpeg_decode call on the current stream; one read of the n status words.  ValueError for a
    file of another geometry than the first (naming it), for broken framing, and for an image the device refuses (naming it and the
    status); UnsupportedJpeg (a ValueError) for a file outside the decoder's subset.  RuntimeError without a GPU: there is no host
    decoder in this package."""
    from . import ops
    if split not in SPLIT_MODES:
        raise ValueError(f"jpeg_gpu.decode_batch: split = {split!r} (one of {', '.join(SPLIT_MODES)})")
    items = list(blobs_or_paths)
    if not items:
        raise ValueError("jpeg_gpu.decode_batch: no files")
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(f"jpeg_gpu decodes on the GPU (device {dev}, GPU available: {torch.cuda.is_available()}); there is no CPU fallback")
    names = [it if isinstance(it, str) else f"image {i}" for i, it in enumerate(items)] if names is None else list(names)

    def load(i: int):
        blob = items[i]
        if isinstance(blob, str):
            with open(blob, "rb") as f:
                blob = f.read()
        blob = bytes(blob)
        return blob, parse(blob, names[i])

    k = min(pool_threads(threads), len(items))
    if k == 1:
        got = [load(i) for i in range(len(items))]
    else:
        with ThreadPoolExecutor(max_workers=k) as ex:
            got = list(ex.map(load, range(len(items))))
    blobs, parsed = [g[0] for g in got], [g[1] for g in got]
    geom = parsed[0][:5]
    for i, p in enumerate(parsed):
        if p[:5] != geom:
            raise ValueError(f"{names[i]}: {p.h} x {p.w}, {p.components} components, sampling {p.hs} x {p.vs} differs from "
                             f"{geom[0]} x {geom[1]}, {geom[2]} components, sampling {geom[3]} x {geom[4]} of {names[0]}")
    data, desc, tables = pack(parsed, blobs)
    # one pinned buffer, one copy: the descriptors (8-byte aligned) first, then the tables, then the data
    nd, nt = desc.size * 8, tables.size
    host = torch.empty(nd + nt + max(data.size, 1), dtype=torch.uint8, pin_memory=True)
    view = host.numpy()
    view[:nd] = desc.view(np.uint8).reshape(-1)
    view[nd:nd + nt] = tables.reshape(-1)
    view[nd + nt:nd + nt + data.size] = data
    with torch.cuda.device(dev):
        buf = host.to(dev, non_blocking=True)
        out, status = ops.jpeg_decode(buf[nd + nt:nd + nt + data.size], buf[:nd].view(torch.int64).view(-1, DESC_WORDS),
                                      buf[nd:nd + nt].view(-1, TABLE_SET_BYTES), len(items), *geom,
                                      **({} if split == "never" or (split == "auto" and int(desc[:, 1].max()) < SPLIT_MIN_BYTES) else
                                         dict(segment_bytes=segment_bytes, split_min_bytes=0 if split == "always" else SPLIT_MIN_BYTES)))
        codes = status.cpu().numpy()
    for i in np.flatnonzero(codes):
        code = int(codes[i])
        what = DECODE_STATUS[code] if 0 <= code < len(DECODE_STATUS) else "unknown status"
        raise ValueError(f"{names[i]}: the entropy-coded data does not decode on the GPU: status {code} ({what})")
    return out
