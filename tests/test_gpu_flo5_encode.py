"""Spring .flo5 chunks compressed on the GPU: sf_flo5_encode (csrc/flo5_encode.hip) through the C ABI, ops.flo5_encode,
flo5_gpu.write_batch and create_spring_submission_mf(flo5_encode="gpu"), against tests/flo5_encode_cases.py's chunk_stream_ref
(pinned to zlib, flo5.read_flo5 and h5py by tests/test_flo5_encode_cases_cpu.py).

Criterion: every comparison is BITWISE -- the format is integer arithmetic on bit patterns, so there is no tolerance to choose.
Stream lengths and stream bytes must equal chunk_stream_ref's; output slots are prefilled with 0xA5 between guard bands, the bytes
behind a stream up to sf_flo5_chunk_bound are unspecified, everything behind the bound and between slots must come back intact.
Shapes (tests/flo5_encode_cases.CASES): N = 2 and N = 6 (less than a word, a tail behind a word: the float-by-float path), an edge
chunk padded with zero rows, N = 65536 (exactly one full block per plane), N = 65538 (a 2-byte second segment per plane), the
default chunking rule."""
import glob
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import flo5_encode_cases as fc
from tests.guarded import GuardedBytes

pytestmark = pytest.mark.gpu
FILL = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def lib():
    from streamflow_amd import _lib
    return _lib.load()


def encode(dev, fields, rpc, row_gap=0, ch_gap=0, field_gap=0, slot_gap=0, shift=0):
    """sf_flo5_encode through the C ABI on fields [2, h, w] float32 -> (streams [field][chunk], the flat output bytes).  Rows are
    row_gap floats apart beyond w, channels ch_gap and fields field_gap more, the input starts `shift` floats off the allocation's
    alignment; slots are the bound + slot_gap apart.  Asserts on the way: status, guard bands, input unchanged, nothing written
    behind the bound of a slot."""
    n, (_, h, w) = len(fields), fields[0].shape
    rs = w + row_gap
    cs = h * rs + ch_gap
    fs = 2 * cs + field_gap
    floats = (n - 1) * fs + cs + (h - 1) * rs + w
    src = GuardedBytes(dev, 4 * floats, fill=0xEE, shift=4 * shift)
    host = np.full(floats, 0xEEEEEEEE, np.uint32)
    for i, f in enumerate(fields):
        assert f.shape == (2, h, w) and f.dtype == np.float32
        for ch in range(2):
            for y in range(h):
                host[i * fs + ch * cs + y * rs:][:w] = f[ch, y].view(np.uint32)
    src.view().copy_(torch.from_numpy(host.view(np.uint8)))
    nchunks = -(-h // rpc)
    bound, ws_bytes = lib().sf_flo5_chunk_bound(rpc, w), lib().sf_flo5_encode_ws_bytes(n, h, w, rpc)
    assert bound == fc.bound(rpc, w) and ws_bytes > 0
    ostride = bound + slot_gap
    slots = n * nchunks
    out = GuardedBytes(dev, (slots - 1) * ostride + bound, fill=FILL)
    ws = GuardedBytes(dev, ws_bytes, fill=0x3C, shift=4 * shift)
    lengths = torch.full((slots + 2,), -7, dtype=torch.int64, device=dev)
    status = lib().sf_flo5_encode(src.ptr, fs, cs, rs, n, h, w, rpc, out.ptr, ostride, lengths[1:].data_ptr(), ws.ptr, ws_bytes,
                                  torch.cuda.current_stream().cuda_stream)
    assert status == 0, lib().sf_last_error()
    torch.cuda.synchronize()
    assert src.guards_unchanged() and out.guards_unchanged() and ws.guards_unchanged()
    assert np.array_equal(src.view().cpu().numpy(), host.view(np.uint8))
    got = lengths.cpu().numpy()
    assert got[0] == -7 and got[-1] == -7
    flat = out.view().cpu().numpy()
    streams = []
    for k in range(slots):
        assert 6 < got[1 + k] <= bound, got
        streams.append(flat[k * ostride:k * ostride + got[1 + k]].tobytes())
        assert (flat[k * ostride + bound:(k + 1) * ostride] == FILL).all(), "bytes between the slots were written"
    return [streams[i * nchunks:(i + 1) * nchunks] for i in range(n)], flat


def check(dev, fields, rpc, **kw):
    streams, _ = encode(dev, fields, rpc, **kw)
    for i, f in enumerate(fields):
        for c, got in enumerate(streams[i]):
            want = fc.chunk_stream_ref(f, c, rpc)
            assert len(got) == len(want), (i, c, len(got), len(want))
            if got != want:
                a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
                first = int(np.argmax(a != b))
                raise AssertionError(f"field {i} chunk {c}: {int((a != b).sum())} of {len(want)} bytes differ, first at {first}: "
                                     f"{a[first]:#x} != {b[first]:#x}")
    return streams


@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_streams_equal_the_reference(dev, case):
    h, w, rpc = case
    check(dev, [fc.make(h, w, 11 + h, special=h > 1)], rpc or fc.default_rows_per_chunk(h))


def test_batch_of_three_with_strides_and_twice(dev):
    """Three fields in one call, one of them special values only in part: dense (two floats per load where w is even) and with gaps
    between rows, channels, fields and slots, the input 4 bytes off 8-byte alignment (float by float); the streams do not depend on
    the placement, and the same call twice over a 0xA5 prefill gives the same bytes."""
    for h, w, rpc in ((37, 54, 5), (37, 53, 2)):
        fields = [fc.make(h, w, 21), fc.make(h, w, 22, special=True), np.zeros((2, h, w), np.float32)]
        dense = check(dev, fields, rpc)
        gaps = check(dev, fields, rpc, row_gap=3, ch_gap=5, field_gap=7, slot_gap=12, shift=1)
        even = check(dev, fields, rpc, row_gap=2, ch_gap=4, field_gap=6, slot_gap=4)
        assert dense == gaps == even
        again, flat2 = encode(dev, fields, rpc)
        assert again == dense


def test_special_values_pass_as_bit_patterns(dev):
    """NaN payloads, a signalling NaN, -0.0, infinities and denormals: the streams inflate to exactly these bit patterns."""
    import zlib
    h, w, rpc = 4, 14, 2
    bits = np.resize(fc.SPECIALS, 2 * h * w).reshape(2, h, w).copy()
    field = bits.view(np.float32)
    streams = check(dev, [field], rpc)
    for c, s in enumerate(streams[0]):
        raw = np.frombuffer(zlib.decompress(s), np.uint8).reshape(4, -1).T.copy().view("<u4").reshape(rpc, w, 2)
        assert np.array_equal(raw, bits[:, c * rpc:(c + 1) * rpc].transpose(1, 2, 0))


def test_ops_flo5_encode_on_an_unpadded_view(dev):
    """ops.flo5_encode on the unpadded view of a larger padded tensor: row_stride > w and an odd column offset (rows 4-byte but not
    8- or 16-byte aligned), and on a dense batch; refusals."""
    from streamflow_amd import ops
    rng = np.random.default_rng(13)
    big = torch.from_numpy((rng.standard_normal((3, 2, 48, 72)) * 5).astype(np.float32)).to(dev)
    view = big[:, :, 3:40, 5:58]                                             # 37 x 53 at column 5
    assert view.data_ptr() % 8 == 4 and view.stride(2) == 72
    streams, lengths = ops.flo5_encode(view, 2)
    assert streams.dtype == torch.uint8 and lengths.dtype == torch.int64
    assert tuple(streams.shape) == (3, 19, fc.bound(2, 53)) and tuple(lengths.shape) == (3, 19)
    host, used, fields = streams.cpu().numpy(), lengths.cpu().numpy(), view.cpu().numpy()
    for i in range(3):
        for c in range(19):
            assert host[i, c, :used[i, c]].tobytes() == fc.chunk_stream_ref(fields[i], c, 2), (i, c)
    one = big[1:2, :, 1:47, 2:66]                                            # n = 1, even width and offset: two floats per load
    streams, lengths = ops.flo5_encode(one)                                  # the default rule: 46 rows -> 2 rows a chunk
    assert tuple(lengths.shape) == (1, 23)
    host, used = streams.cpu().numpy(), lengths.cpu().numpy()
    for c in (0, 11, 22):
        assert host[0, c, :used[0, c]].tobytes() == fc.chunk_stream_ref(one[0].cpu().numpy(), c, 2), c
    for bad in (big.cpu(), big.double(), big[:, :1], big[0], big.permute(0, 1, 3, 2), big[:, :, :, ::2]):
        with pytest.raises(RuntimeError):
            ops.flo5_encode(bad)
    with pytest.raises(RuntimeError):
        ops.flo5_encode(torch.zeros(1, 2, 65, 4, device=dev), 1)             # 65 chunks


def test_write_batch_files_read_back_bitwise(dev, tmp_path):
    from streamflow_amd import flo5, flo5_gpu
    fields = np.stack([fc.make(70, 90, s, special=s == 2) for s in (1, 2, 3)])
    flows = torch.from_numpy(fields).to(dev)
    paths = [str(tmp_path / f"f{i}.flo5") for i in range(3)]
    sizes = flo5_gpu.write_batch(flows, paths, threads=2)
    for i, p in enumerate(paths):
        assert os.path.getsize(p) == sizes[i]
        got = flo5.read_flo5(p)
        assert got.dtype == np.float32 and got.shape == (70, 90, 2)
        assert np.array_equal(got.view(np.uint32), fields[i].transpose(1, 2, 0).view(np.uint32)), i
        data = open(p, "rb").read()
        assert data == flo5.flo5_file(fc.field_streams_ref(fields[i]), 70, 90, 3, shuffle=True, level=1), i
    one = str(tmp_path / "one.flo5")
    flo5_gpu.write_batch(flows[2:, :, 1:, 1:], [one], rows_per_chunk=23)
    assert np.array_equal(flo5.read_flo5(one).view(np.uint32), fields[2, :, 1:, 1:].transpose(1, 2, 0).view(np.uint32))
    with pytest.raises(ValueError):
        flo5_gpu.write_batch(flows, paths[:2])
    with pytest.raises(RuntimeError):
        flo5_gpu.write_batch(flows.cpu(), paths)


def test_spring_submission_gpu_files_decode_to_the_host_files(dev, tmp_path):
    """create_spring_submission_mf with flo5_encode="gpu" and "host" on a two-scene synthetic tree at 16 x 24: the same file names,
    every pair of files decodes bitwise equal (the file bytes differ: another filter pipeline).  The model is a stub (a field made
    from the frames' tags, NaNs included, inside a padded output): the test is about the writer."""
    from streamflow_amd import flo5, flow_io, submit
    H, W = 16, 24
    rng = np.random.default_rng(15)
    for s, (scene, n) in enumerate({"0003": 4, "0010": 5}.items()):
        for c, cam in enumerate(("left", "right")):
            d = tmp_path / "test" / scene / f"frame_{cam}"
            os.makedirs(d)
            for i in range(n):
                img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
                img[0, 0] = (s, c, i)
                flow_io.write_png(str(d / f"frame_{cam}_{i + 1:04d}.png"), img)

    def model(images, iters=0, test_mode=False):
        tags = [im[0, :, 0, 0].float().round().to(torch.int64).tolist() for im in images]
        out = []
        for (s, c, a), (_, _, b) in zip(tags[:-1], tags[1:]):
            g = torch.Generator().manual_seed(10000 * s + 1000 * c + 10 * a + b)
            f = torch.randn(1, 2, *images[0].shape[-2:], generator=g) * 7
            f[0, 0, 2, 3:6] = float("nan")
            out.append(f.to(images[0].device))
        return out

    runs = {}
    for mode in ("host", "gpu"):
        out = str(tmp_path / mode)
        submit.create_spring_submission_mf(Namespace(spring_root=str(tmp_path)), model, iters=1, output_path=out, nframes=3, device=dev,
                                           flo5_encode=mode)
        files = sorted(glob.glob(os.path.join(out, "*", "*", "*.flo5")))
        runs[mode] = {os.path.relpath(p, out): (flo5.read_flo5(p), open(p, "rb").read()) for p in files}
    assert sorted(runs["host"]) == sorted(runs["gpu"]) and len(runs["host"]) == 2 * 2 * ((4 - 1) + (5 - 1))
    for p, (want, want_bytes) in runs["host"].items():
        got, got_bytes = runs["gpu"][p]
        assert got.shape == (H, W, 2) and got.dtype == want.dtype and np.array_equal(got.view(np.uint32), want.view(np.uint32)), p
        assert np.isnan(got).any() and got_bytes != want_bytes, p
    with pytest.raises(ValueError):
        submit.create_spring_submission_mf(Namespace(spring_root=str(tmp_path)), model, iters=1, output_path=str(tmp_path / "bad"),
                                           nframes=3, device=dev, flo5_encode="device")
