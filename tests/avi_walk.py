"""A test-side walker of the RIFF AVI files avi.MjpegWriter makes (tests/test_jpeg_cases_cpu.py, tests/test_gpu_jpeg_encode.py).  No
player or demuxer is installed where the tests run, so whether a file plays rests on these field checks: every size field, the even
padding, the headers' counts and rates, and every idx1 entry against the chunk it points at.  Written from the AVI RIFF file
reference (the `avih` / `strh` / `strf` / `idx1` layouts), sharing no code with streamflow_amd/avi.py."""
import struct


def _chunks(data, start, end):
    """(tag, payload start, payload size) of the chunks in data[start:end], which they must fill exactly, each padded to even."""
    out, at = [], start
    while at < end:
        assert at + 8 <= end, f"a chunk header at {at} crosses the end {end}"
        tag, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
        assert at + 8 + size <= end, f"chunk {tag!r} at {at}: {size} bytes cross the end {end}"
        out.append((tag, at + 8, size))
        at += 8 + size + (size & 1)
        if size & 1 and at <= end:
            assert data[at - 1] == 0, f"chunk {tag!r}: the padding byte is {data[at - 1]:#x}"
    assert at == end, (at, end)
    return out


def walk(data):
    """-> dict(width, height, rate, scale, usec, frames: [bytes]); asserts the whole structure."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    riff = struct.unpack_from("<I", data, 4)[0]
    assert riff + 8 == len(data) and len(data) < 2 ** 31, (riff, len(data))
    top = _chunks(data, 12, len(data))
    assert [t for t, _, _ in top] == [b"LIST", b"LIST", b"idx1"], top
    (_, hdrl, hdrl_size), (_, movi, movi_size), (_, idx, idx_size) = top
    assert data[hdrl:hdrl + 4] == b"hdrl" and data[movi:movi + 4] == b"movi"
    inner = _chunks(data, hdrl + 4, hdrl + hdrl_size)
    assert [t for t, _, _ in inner] == [b"avih", b"LIST"] and inner[0][2] == 56
    usec, per_sec, _, flags, total, initial, streams, suggested, width, height = struct.unpack_from("<10I", data, inner[0][1])
    assert flags & 0x10 and streams == 1 and initial == 0
    strl, strl_size = inner[1][1], inner[1][2]
    assert data[strl:strl + 4] == b"strl"
    sub = _chunks(data, strl + 4, strl + strl_size)
    assert [t for t, _, _ in sub] == [b"strh", b"strf"] and sub[0][2] == 56 and sub[1][2] == 40
    fcc, handler, _, _, _, _, scale, rate, start, length, sbuf, _, sample = struct.unpack_from("<4s4sIHHIIIIIIII", data, sub[0][1])
    left, top_, right, bottom = struct.unpack_from("<4H", data, sub[0][1] + 48)
    assert (fcc, handler, start, sample) == (b"vids", b"MJPG", 0, 0) and (left, top_, right, bottom) == (0, 0, width, height)
    size, bw, bh, planes, bits, comp, image = struct.unpack_from("<IiiHH4sI", data, sub[1][1])
    assert (size, bw, bh, planes, bits, comp, image) == (40, width, height, 1, 24, b"MJPG", width * height * 3)
    frames = _chunks(data, movi + 4, movi + movi_size)
    assert all(t == b"00dc" for t, _, _ in frames)
    assert total == length == len(frames) and idx_size == 16 * len(frames)
    biggest = max([s for _, _, s in frames], default=0)
    assert suggested >= biggest and sbuf >= biggest
    assert scale >= 1 and rate >= 1 and abs(usec - 1e6 * scale / rate) <= 0.5
    if frames:
        assert per_sec * len(frames) * scale >= sum(s for _, _, s in frames) * rate > (per_sec - 1) * len(frames) * scale
    for k, (_, at, size) in enumerate(frames):
        tag, fl, off, sz = struct.unpack_from("<4sIII", data, idx + 16 * k)
        assert tag == b"00dc" and fl & 0x10 and sz == size and movi + off == at - 8, (k, tag, fl, off, sz, at)
        assert data[movi + off:movi + off + 4] == b"00dc" and struct.unpack_from("<I", data, movi + off + 4)[0] == sz
    return dict(width=width, height=height, rate=rate, scale=scale, usec=usec, frames=[data[at:at + size] for _, at, size in frames])
