"""CPU: the restatement of the .flo5 chunk encoder (tests/flo5_encode_cases.py) is pinned to what it must be read by -- zlib inflates
every reference stream to the shuffled chunk, flo5.flo5_file frames such streams into files that flo5.read_flo5 and the real h5py
read back bit for bit -- and the parts of the feature that need no device: the bound, the filter message against the one h5py
wrote, write_flo5's bytes unchanged by the factoring, the argument checks of sf_flo5_encode (they return before any launch)."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import flo5_encode_cases as fc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD5 = os.path.join(REPO, "tests", "golden", "flo5")
H5PY_PYTHON = "/opt/conda/bin/python3.9"            # the build container's interpreter that has h5py 3.3.0 / HDF5 1.10.6
SHAPES = ((1, 1), (37, 53), (136, 240))


def nan_field(h, w, seed):
    """[2, h, w] float32 with NaNs (Spring's invalid pixels), a NaN payload, -0.0 and infinities."""
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((2, h, w)) * 9).astype(np.float32)
    if h > 1:
        f[:, rng.random((h, w)) < 0.05] = np.nan
        f.view(np.uint32)[0, 1, :4] = [0x7FC12345, 0x80000000, 0x7F800000, 0xFF800000]
    return f


def gpu_style_file(path, flow, rpc=0, level=1):
    """The file flo5_gpu.write_batch writes for flow [2, h, w], with the reference streams in place of the device's."""
    from streamflow_amd import flo5
    _, h, w = flow.shape
    rpc = rpc or fc.default_rows_per_chunk(h)
    blob = flo5.flo5_file(fc.field_streams_ref(flow, rpc), h, w, rpc, shuffle=True, level=level)
    with open(path, "wb") as f:
        f.write(blob)
    return blob


def test_header_constant_and_case_list():
    assert fc.header_block_bytes() == fc.BLOCK_BYTES == 65536
    assert [2 * (rpc or fc.default_rows_per_chunk(h)) * w for h, w, rpc in fc.CASES] == [2, 6, 212, 65536, 65538, 54]


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_reference_streams_inflate_to_the_shuffled_chunk(case):
    h, w, rpc = case
    rpc = rpc or fc.default_rows_per_chunk(h)
    flow = fc.make(h, w, 3, special=True)
    nchunks = -(-h // rpc)
    for c in sorted({0, nchunks // 2, nchunks - 1}):
        stream = fc.chunk_stream_ref(flow, c, rpc)
        want = fc.shuffled(flow, c, rpc)
        assert stream[:2] == b"\x78\x01" and zlib.decompress(stream) == want.tobytes()
        assert len(stream) <= fc.bound(rpc, w)
        assert len(stream) == 2 + -(-fc.stream_bits(want) // 8) + 4
        # the shuffle is HDF5's: undoing it the way flo5.read_flo5 does gives the chunk, whose rows are the field's (zero past h)
        back = np.frombuffer(want.reshape(4, -1).T.tobytes(), "<u4").reshape(rpc, w, 2)
        rows = flow.view(np.uint32)[:, c * rpc:(c + 1) * rpc].transpose(1, 2, 0)
        assert np.array_equal(back[:rows.shape[0]], rows) and not back[rows.shape[0]:].any()


def test_blocks_never_straddle_planes():
    for n, bb in ((2, 65536), (65536, 65536), (65538, 65536), (100, 16), (96, 16)):
        cuts = fc.blocks(n, bb)
        assert len(cuts) == 4 * -(-n // bb) and cuts[0][0] == 0 and cuts[-1][1] == 4 * n
        assert all(a // n == (b - 1) // n and 0 < b - a <= bb for a, b in cuts)
        assert all(cuts[k][1] == cuts[k + 1][0] for k in range(len(cuts) - 1))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_flo5_file_round_trip_is_bitwise(tmp_path, shape):
    from streamflow_amd import flo5
    h, w = shape
    flow = nan_field(h, w, 5)
    p = str(tmp_path / "f.flo5")
    gpu_style_file(p, flow)
    got = flo5.read_flo5(p)
    assert got.dtype == np.float32 and got.shape == (h, w, 2)
    assert np.array_equal(got.view(np.uint32), flow.transpose(1, 2, 0).view(np.uint32))
    with pytest.raises(ValueError):
        flo5.flo5_file([], h, w, 1, True, 1)                                 # no streams for ceil(h / 1) chunks
    with pytest.raises(ValueError):
        flo5.flo5_file([b""] * 65, 65, 1, 1, True, 1)


@pytest.mark.skipif(not os.path.exists(H5PY_PYTHON), reason="needs the build container's h5py interpreter")
def test_h5py_reads_the_files_back_equal(tmp_path):
    paths = []
    for i, (h, w) in enumerate(SHAPES):
        flow = nan_field(h, w, 6 + i)
        p = str(tmp_path / f"g{i}.flo5")
        gpu_style_file(p, flow)
        np.save(str(tmp_path / f"g{i}.npy"), np.ascontiguousarray(flow.transpose(1, 2, 0)))
        paths.append(p)
    code = ("import sys, h5py, numpy as np\n"
            "for p in sys.argv[1:]:\n"
            "    want = np.load(p[:-5] + '.npy')\n"
            "    with h5py.File(p, 'r') as f:\n"
            "        d = f['flow']; a = d[()]\n"
            "        same = a.dtype == want.dtype and a.shape == want.shape and a.tobytes() == want.tobytes()\n"
            "        print(int(same), d.compression, d.compression_opts, d.shuffle, a.dtype)\n")
    out = subprocess.run([H5PY_PYTHON, "-c", code] + paths, capture_output=True, text=True, timeout=120, env={"PATH": "/usr/bin:/bin"})
    assert out.returncode == 0, out.stderr[-500:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(SHAPES)
    for line in lines:
        assert line.split() == ["1", "gzip", "1", "True", "float32"], line


def test_bound_holds_for_the_worst_chunks():
    """All-0xFF words (one symbol per block: 1-bit codes; and the case the fixed table's 9-bit codes are for), uniform random bytes
    (the fixed-table replacement: at most 9 bits a byte) and an all-zero chunk, at one block per plane and at a short second one."""
    rng = np.random.default_rng(8)
    for rpc, w in ((1, 1), (2, 53), (64, 512), (3, 10923)):
        n = rpc * w * 2
        for kind in ("ff", "noise", "zeros", "high"):
            if kind == "ff":
                bits = np.full((2, rpc, w), 0xFFFFFFFF, np.uint32)
            elif kind == "zeros":
                bits = np.zeros((2, rpc, w), np.uint32)
            elif kind == "high":                             # 255 and 254 only: where a dynamic table could cost more than 9 bits
                bits = rng.integers(254, 256, size=(2, rpc, w, 4), dtype=np.uint8).view(np.uint32)[..., 0]
            else:
                bits = rng.integers(0, 1 << 32, size=(2, rpc, w), dtype=np.uint64).astype(np.uint32)
            flow = bits.view(np.float32)
            data = fc.shuffled(flow, 0, rpc)
            assert data.size == 4 * n
            length = 2 + -(-fc.stream_bits(data) // 8) + 4
            assert length <= fc.bound(rpc, w), (rpc, w, kind, length, fc.bound(rpc, w))
            if n <= 212:
                stream = fc.chunk_stream_ref(flow, 0, rpc)
                assert len(stream) == length and zlib.decompress(stream) == data.tobytes()
    # a block never takes more than its header and 9 bits a byte, whatever its histogram
    for hist in (np.eye(256, dtype=np.int64)[255] * 65536, np.full(256, 256), np.arange(256) ** 3 + 1):
        lit, cl, _, _ = fc.band_tables(hist)
        assert sum(int(f) * l for f, l in zip(hist, lit)) + lit[256] <= 9 * int(hist.sum()) + 9


def _filter_message(path):
    from streamflow_amd import flo5
    with open(path, "rb") as f:
        hf = flo5._File(f.read(), path)
    body = [b for t, b in hf.messages(hf.group_entries(hf.root_header)["flow"]) if t == flo5.MSG_FILTERS]
    assert len(body) == 1
    return body[0]


def test_filter_message_equals_the_one_h5py_wrote(tmp_path):
    """tests/golden/flo5/shuffle_chunks.flo5 was written by h5py with shuffle=True, gzip level 9: flo5_file's message with level 9 is
    that message byte for byte, and differs from it in the level's byte alone otherwise."""
    from streamflow_amd import flo5
    gold = _filter_message(os.path.join(GOLD5, "shuffle_chunks.flo5"))
    flow = fc.make(5, 7, 1)
    for level in (9, 1):
        p = str(tmp_path / f"l{level}.flo5")
        gpu_style_file(p, flow, level=level)
        mine = _filter_message(p)
        assert len(mine) == len(gold) == 8 + 2 * 24
        diff = [i for i in range(len(gold)) if mine[i] != gold[i]]
        assert diff == ([] if level == 9 else [8 + 24 + 16]), (level, diff)
        assert struct.unpack_from("<I", mine, 8 + 24 + 16)[0] == level
    assert struct.unpack_from("<HHHH", gold, 8) == (2, 8, 1, 1) and gold[16:24] == b"shuffle\0" and struct.unpack_from("<I", gold, 24)[0] == 4
    assert flo5._File(open(p, "rb").read(), p)._filters(mine) == [2, 1]


def test_write_flo5_bytes_are_what_they_were(tmp_path):
    """write_flo5 now goes through flo5_file(shuffle=False): the files are its chunks' zlib streams behind the same framing."""
    from streamflow_amd import flo5
    flow = nan_field(37, 53, 9).transpose(1, 2, 0)
    p = str(tmp_path / "w.flo5")
    flo5.write_flo5(p, flow, compression_level=5, rows_per_chunk=4)
    data = open(p, "rb").read()
    chunks = []
    for c in range(10):
        buf = np.zeros((4, 53, 2), "<f4")
        rows = flow[4 * c:4 * c + 4]
        buf[:rows.shape[0]] = rows
        chunks.append(zlib.compress(buf.tobytes(), 5))
    assert data == flo5.flo5_file(chunks, 37, 53, 4, shuffle=False, level=5)
    assert data.endswith(b"".join(chunks)) and _filter_message(p) == (struct.pack("<BB6x", 1, 1) + struct.pack("<HHHH", 1, 8, 1, 1) +
                                                                      b"deflate\0" + struct.pack("<I4x", 5))
    assert np.array_equal(flo5.read_flo5(p).view(np.uint32), np.ascontiguousarray(flow).view(np.uint32))


@pytest.fixture(scope="module")
def lib():
    from streamflow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_bound_and_workspace_functions(lib):
    for rpc, w in ((1, 1), (1, 3), (2, 53), (64, 512), (3, 10923), (34, 1920)):
        assert lib.sf_flo5_chunk_bound(rpc, w) == fc.bound(rpc, w), (rpc, w)
    assert lib.sf_flo5_chunk_bound(0, 4) == -1 and lib.sf_flo5_chunk_bound(4, 0) == -1
    assert lib.sf_flo5_chunk_bound(1 << 14, 1 << 14) == -1                    # 4 N = 2^31
    assert lib.sf_flo5_chunk_bound((1 << 14) - 1, 1 << 14) > 0
    assert lib.sf_flo5_encode_ws_bytes(3, 1080, 1920, 34) >= 3 * 32 * 4 * 34 * 1920 * 2
    for args in ((0, 4, 4, 1), (65536, 4, 4, 1), (1, 0, 4, 1), (1, 4, 0, 1), (1, 4, 4, 0), (1, 65, 4, 1), (1, 4, 1 << 14, 1 << 14)):
        assert lib.sf_flo5_encode_ws_bytes(*args) == -1, args


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Every refusal of the header's list returns SF_ERR_BAD_ARG from the argument checks: no device is needed (the pointers are
    made-up addresses that are never dereferenced)."""
    n, h, w, rpc = 2, 5, 7, 2
    bound, ws_bytes = lib.sf_flo5_chunk_bound(rpc, w), lib.sf_flo5_encode_ws_bytes(n, h, w, rpc)
    assert bound > 0 and ws_bytes > 0
    plane = h * w
    good = dict(flow=1 << 20, fs=2 * plane, cs=plane, rs=w, n=n, h=h, w=w, rpc=rpc, out=2 << 20, ostride=bound, lengths=3 << 20,
                ws=4 << 20, ws_bytes=ws_bytes)
    bad = [dict(flow=None), dict(out=None), dict(lengths=None), dict(ws=None), dict(n=0), dict(n=65536), dict(h=0), dict(w=0),
           dict(rpc=0), dict(rpc=-1), dict(h=65, rpc=1, fs=1 << 20, cs=1 << 10, ws_bytes=1 << 30),          # 65 chunks
           dict(w=1 << 14, rpc=1 << 14, rs=1 << 14, cs=1 << 40, fs=1 << 41, ostride=1 << 40, ws_bytes=1 << 40),     # 4 N = 2^31
           dict(rs=w - 1), dict(cs=plane - 1), dict(fs=2 * plane - 1), dict(flow=(1 << 20) + 2),
           dict(ostride=bound - 4), dict(ostride=bound + 2), dict(out=(2 << 20) + 2), dict(lengths=(3 << 20) + 4),
           dict(ws_bytes=ws_bytes - 1)]
    for change in bad:
        a = dict(good, **change)
        status = lib.sf_flo5_encode(a["flow"], a["fs"], a["cs"], a["rs"], a["n"], a["h"], a["w"], a["rpc"], a["out"], a["ostride"],
                                    a["lengths"], a["ws"], a["ws_bytes"], None)
        assert status == -1, (change, status, lib.sf_last_error())
        assert b"sf_flo5_encode" in lib.sf_last_error()


def test_python_wrappers_refuse_without_a_gpu(tmp_path):
    import torch
    from streamflow_amd import flo5_gpu, ops, submit
    flows = torch.zeros(1, 2, 4, 4)
    with pytest.raises(RuntimeError):
        ops.flo5_encode(flows)
    with pytest.raises(RuntimeError):
        flo5_gpu.write_batch(flows, [str(tmp_path / "a.flo5")])
    with pytest.raises(ValueError):
        flo5_gpu.write_batch(flows, [])
    with pytest.raises(ValueError):
        submit.create_spring_submission_mf(None, None, 1, flo5_encode="device")


def test_block_size_choice_on_a_bench_like_field():
    """DESIGN.md 9.8's comparison at a size a test can afford (one 136 x 1920 strip of the bench field, default chunking at full
    height: 34 rows): 64 KiB blocks are within 1 % of both 16 KiB and 256 KiB, and the shuffled Huffman-only stream is smaller than
    the raw chunk."""
    flow = fc.bench_field(136, 1920, 1)
    data = [fc.shuffled(flow, c, 34) for c in range(4)]
    bits = {bb: sum(fc.stream_bits(d, bb) for d in data) for bb in (16384, 65536, 262144)}
    raw = 8 * sum(d.size for d in data)
    assert bits[65536] < 0.95 * raw
    assert bits[65536] <= 1.01 * min(bits.values()), bits
