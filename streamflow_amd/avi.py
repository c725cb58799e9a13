"""Motion-JPEG in an AVI container (RIFF, the 1.0 layout with an `idx1` index): every frame is a complete JPEG file, so the frames
jpeg_gpu.encode_batch makes on the GPU go in as they are.  The layout:

    RIFF 'AVI '
      LIST 'hdrl'   avih (main header, AVIF_HASINDEX)
                    LIST 'strl'   strh ('vids' / 'MJPG', dwRate / dwScale = fps)   strf (BITMAPINFOHEADER, 24 bit, 'MJPG')
      LIST 'movi'   '00dc' chunks, one per frame, padded to even length
      idx1          one entry per frame: '00dc', AVIIF_KEYFRAME, offset from the 'movi' tag, size

Frames stream to disk as they come; the sizes and counts are patched on close().  Files stay below 2^31 - 1 bytes (OpenDML
extensions are not written).  MJPEG decoders assume the Annex K.3 Huffman tables and YCbCr; the frames carry their own DHT anyway.
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
