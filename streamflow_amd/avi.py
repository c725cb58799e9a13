"""Motion-JPEG in an AVI container (RIFF, the 1.0 layout with an `idx1` index): every frame is a complete JPEG file, so the frames
jpeg_gpu.encode_batch makes on the GPU go in as they are.  The layout:

    RIFF 'AVI '
      LIST 'hdrl'   avih (main header, AVIF_HASINDEX)
                    LIST 'strl'   strh ('vids' / 'MJPG', dwRate / dwScale = fps)   strf (BITMAPINFOHEADER, 24 bit, 'MJPG')
      LIST 'movi'   '00dc' chunks, one per frame, padded to even length
      idx1          one entry per frame: '00dc', AVIIF_KEYFRAME, offset from the 'movi' tag, size

Frames stream to disk as they come; the sizes and counts are patched on close().  Files stay below 2^31 - 1 bytes (OpenDML
extensions are not written).  MJPEG decoders assume the Annex K.3 Huffman tables and YCbCr; the frames carry their own DHT anyway.

MjpegReader is the way back: it finds the frames of such a file (this writer's or another's: with or without `idx1`, `rec ` lists,
`##db` chunks, empty chunks for repeated frames) and hands their bytes to jpeg_gpu.decode_batch.
"""
from __future__ import annotations

import struct
from fractions import Fraction

AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
MAX_FILE_BYTES = 2 ** 31 - 1
MAX_FPS_DENOMINATOR = 1001                      # 30000 / 1001 and 24000 / 1001 are exact; 23.976 is 2997 / 125


def jpeg_size(data: bytes):
    """(width, height) from the frame header (SOF0 .. SOF2) of a JPEG file; ValueError where there is none."""
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise ValueError("not a JPEG file (no SOI)")
    i = 2
    while i + 4 <= len(data) and data[i] == 0xFF:
        marker, size = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        if marker in (0xC0, 0xC1, 0xC2) and i + 9 <= len(data):
            return int.from_bytes(data[i + 7:i + 9], "big"), int.from_bytes(data[i + 5:i + 7], "big")
        if marker == 0xDA:
            break
        i += 2 + size
    raise ValueError("JPEG file without a frame header")


class MjpegWriter:
    """with MjpegWriter(path, width, height, fps) as v: v.add(jpeg_bytes) ...  Every frame must be a JPEG file of width x height
    (ValueError otherwise, and before the file would pass 2^31 - 1 bytes)."""

    def __init__(self, path: str, width: int, height: int, fps: float):
        if not (1 <= int(width) <= 65535 and 1 <= int(height) <= 65535):
            raise ValueError(f"MjpegWriter: width = {width}, height = {height}")
        if not fps > 0:
            raise ValueError(f"MjpegWriter: fps = {fps}")
        rate = Fraction(fps).limit_denominator(MAX_FPS_DENOMINATOR)
        if rate <= 0:
            raise ValueError(f"MjpegWriter: fps = {fps} is too small")
        self.path, self.width, self.height = path, int(width), int(height)
        self.rate, self.scale = rate.numerator, rate.denominator
        self.index = []                                                 # (offset from the 'movi' tag, size)
        self.largest = 0
        self.f = open(path, "wb")
        self.f.write(self._headers())
        self.movi = self.f.tell() - 4                                   # position of the 'movi' tag
        self.pos = self.f.tell()

    def _headers(self) -> bytes:
        n, w, h = len(self.index), self.width, self.height
        usec = (1000000 * self.scale + self.rate // 2) // self.rate
        data = sum(size for _, size in self.index)
        per_sec = (data * self.rate + n * self.scale - 1) // (n * self.scale) if n else 0
        avih = struct.pack("<14I", usec, min(per_sec, 0xFFFFFFFF), 0, AVIF_HASINDEX, n, 0, 1, self.largest, w, h, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, n, self.largest, 0xFFFFFFFF, 0,
                           0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf)
        hdrl = b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", strl)
        movi_size = 4 + sum(8 + size + (size & 1) for _, size in self.index)
        riff_size = 4 + 8 + len(hdrl) + 8 + movi_size + 8 + 16 * n
        return b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + _chunk(b"LIST", hdrl) + b"LIST" + struct.pack("<I", movi_size) + b"movi"

    def add(self, jpeg: bytes) -> None:
        if self.f is None:
            raise ValueError("MjpegWriter: the file is closed")
        jpeg = bytes(jpeg)
        size = jpeg_size(jpeg)
        if size != (self.width, self.height):
            raise ValueError(f"MjpegWriter: a frame of {size[0]} x {size[1]} in a video of {self.width} x {self.height}")
        n = len(jpeg)
        if self.pos + 8 + n + (n & 1) + 8 + 16 * (len(self.index) + 1) > MAX_FILE_BYTES:
            raise ValueError(f"MjpegWriter: {self.path} would pass {MAX_FILE_BYTES} bytes (OpenDML is not written)")
        self.f.write(b"00dc" + struct.pack("<I", n) + jpeg + b"\x00" * (n & 1))
        self.index.append((self.pos - self.movi, n))
        self.largest = max(self.largest, n)
        self.pos += 8 + n + (n & 1)

    def close(self) -> None:
        if self.f is None:
            return
        idx = b"".join(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, off, size) for off, size in self.index)
        self.f.write(_chunk(b"idx1", idx))
        self.f.seek(0)
        self.f.write(self._headers())
        self.f.close()
        self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _chunk(tag: bytes, payload: bytes) -> bytes:
    return tag + struct.pack("<I", len(payload)) + payload + b"\x00" * (len(payload) & 1)


class MjpegReader:
    """The frames of a Motion-JPEG AVI file as a lazy sequence: `fps` (dwRate / dwScale of the video stream), `hw`, len(),
    `frame_bytes(i)` (the JPEG file of frame i), `device_batch(lo, hi, dev)` (frames lo .. hi - 1 decoded on the GPU by
    jpeg_gpu.decode_batch: uint8 [hi - lo, H, W, 3] where predict_video reads them) and reader[i] (one frame decoded on the GPU,
    returned as a host array).  The frames come from `idx1` where the file has one, else from a walk of `movi` (`rec ` lists
    included); `##dc` and `##db` chunks of the first video stream count, a chunk of length 0 repeats the frame before it.
    ValueError for a file that is no AVI, whose video stream is not MJPG, or that continues in OpenDML `AVIX` segments.  Frames of
    two interlaced fields (`AVI1`) and audio streams are not handled.  `split` is jpeg_gpu.decode_batch's: how frames without restart
    markers -- what most encoders write -- are decoded in parallel."""

    def __init__(self, path: str, split: str = "auto"):
        from .jpeg_gpu import SPLIT_MODES
        if split not in SPLIT_MODES:
            raise ValueError(f"MjpegReader: split = {split!r} (one of {', '.join(SPLIT_MODES)})")
        self.path, self.split = path, split
        self.f = open(path, "rb")
        try:
            self._index()
        except Exception:
            self.f.close()
            raise

    def _bad(self, msg: str) -> ValueError:
        return ValueError(f"{self.path}: {msg}")

    def _chunks(self, start: int, end: int):
        """(tag, payload offset, payload size) of the chunks in [start, end); a chunk that crosses `end` stops the walk."""
        at = start
        while at + 8 <= end:
            self.f.seek(at)
            tag, size = struct.unpack("<4sI", self.f.read(8))
            if at + 8 + size > end:
                raise self._bad(f"chunk {tag!r} at {at}: {size} bytes cross the end of its list at {end}")
            yield tag, at + 8, size
            at += 8 + size + (size & 1)

    def _index(self) -> None:
        self.f.seek(0, 2)
        total = self.f.tell()
        self.f.seek(0)
        head = self.f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
            raise self._bad("not an AVI file (no RIFF 'AVI ' header)")
        end = min(total, 8 + struct.unpack("<I", head[4:8])[0])
        if total >= end + 12:
            self.f.seek(end + (end & 1))
            more = self.f.read(12)
            if more[:4] == b"RIFF" and more[8:12] == b"AVIX":
                raise self._bad("OpenDML file (AVIX segments) -- only AVI 1.0 files are read")
        stream, movi, idx1, streams = None, None, None, 0
        self.fps, self.hw = None, None
        for tag, at, size in self._chunks(12, end):
            if tag == b"LIST":
                self.f.seek(at)
                kind = self.f.read(4)
                if kind == b"hdrl":
                    for t2, a2, s2 in self._chunks(at + 4, at + size):
                        if t2 != b"LIST":
                            continue
                        self.f.seek(a2)
                        if self.f.read(4) != b"strl":
                            continue
                        strh = strf = None
                        for t3, a3, s3 in self._chunks(a2 + 4, a2 + s2):
                            self.f.seek(a3)
                            if t3 == b"strh":
                                strh = self.f.read(s3)
                            elif t3 == b"strf":
                                strf = self.f.read(s3)
                        if strh is not None and len(strh) >= 28 and strh[:4] == b"vids" and stream is None:
                            if strf is None or len(strf) < 20:
                                raise self._bad("video stream without a format chunk")
                            codec = strf[16:20]
                            if codec.upper() != b"MJPG":
                                raise self._bad(f"video stream is {codec!r} / {strh[4:8]!r}, not MJPG")
                            scale, rate = struct.unpack_from("<II", strh, 20)
                            if scale == 0 or rate == 0:
                                raise self._bad(f"video stream with rate {rate} / scale {scale}")
                            w, h = struct.unpack_from("<ii", strf, 4)
                            stream, self.fps, self.hw = streams, rate / scale, (abs(h), abs(w))
                        streams += 1
                elif kind == b"movi":
                    movi = (at, size)
            elif tag == b"idx1":
                idx1 = (at, size)
        if stream is None:
            raise self._bad("no video stream")
        if movi is None:
            raise self._bad("no movi list")
        tags = (b"%02ddc" % stream, b"%02ddb" % stream)
        entries = []                                                    # (payload offset, size), 0 for a repeated frame
        if idx1 is not None and idx1[1] >= 16:
            self.f.seek(idx1[0])
            raw = self.f.read(idx1[1] - idx1[1] % 16)
            rows = [struct.unpack_from("<4sIII", raw, k) for k in range(0, len(raw), 16)]
            rows = [(off, size) for tag, _, off, size in rows if tag in tags]
            if rows:
                # offsets count from the 'movi' tag or from the start of the file: whichever finds the first frame's chunk header
                for base in (movi[0], 0):
                    self.f.seek(base + rows[0][0])
                    if self.f.read(4) in tags:
                        break
                else:
                    raise self._bad("idx1 does not point at the frames")
                entries = [(base + off + 8, size) for off, size in rows]
                if any(at + size > total for at, size in entries):
                    raise self._bad("idx1 points past the end of the file")
        if not entries:
            def walk(start, stop):
                for tag, at, size in self._chunks(start, stop):
                    if tag == b"LIST":
                        self.f.seek(at)
                        if self.f.read(4) == b"rec ":
                            walk(at + 4, at + size)
                    elif tag in tags:
                        entries.append((at, size))
            walk(movi[0] + 4, movi[0] + movi[1])
        self.frames = []
        for at, size in entries:
            if size == 0:
                if not self.frames:
                    raise self._bad("the first frame is empty")
                self.frames.append(self.frames[-1])
            else:
                self.frames.append((at, size))
        if not self.frames:
            raise self._bad("no frames")
        if self.hw[0] == 0 or self.hw[1] == 0:
            w, h = jpeg_size(self.frame_bytes(0))
            self.hw = (h, w)

    def __len__(self) -> int:
        return len(self.frames)

    def frame_bytes(self, i: int) -> bytes:
        at, size = self.frames[i]
        self.f.seek(at)
        data = self.f.read(size)
        if len(data) != size:
            raise self._bad(f"frame {i} crosses the end of the file")
        return data

    def device_batch(self, lo: int, hi: int, dev):
        """The frames lo .. hi - 1 as uint8 [hi - lo, H, W, 3] on `dev`; raises without a GPU (there is no host decoder)."""
        from . import jpeg_gpu
        out = jpeg_gpu.decode_batch([self.frame_bytes(i) for i in range(lo, hi)], dev, names=[f"{self.path}: frame {i}" for i in range(lo, hi)],
                                    split=self.split)
        if tuple(out.shape[1:3]) != self.hw:
            raise self._bad(f"frame {lo} is {tuple(out.shape[1:3])}, the stream header says {self.hw}")
        return out

    def __getitem__(self, i: int):
        if isinstance(i, slice):
            raise TypeError("MjpegReader is indexed by frame number")
        import torch
        i = range(len(self.frames))[i]
        return self.device_batch(i, i + 1, torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu")[0].cpu().numpy()

    def close(self) -> None:
        if self.f is not None:
            self.f.close()
            self.f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
