"""GPU: Spring .flo5 files read on the device -- ops.inflate (sf_inflate: a wave per zlib stream), ops.flo5_assemble, flo5_gpu.read_batch
and spring_report(flo5_decode="gpu") -- against zlib, the numpy restatement of tests/flo5_decode_cases.py and flo5.read_flo5, bit for
bit.  The streams are those the sanitized host build of the same decoder core has decoded (tests/test_inflate_core_host_cpu.py: run
the CPU tests first); no mutated stream comes here."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import flo5_decode_cases as dc
from tests import flo5_encode_cases as ec

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
POISON, GUARD = 0xC3, 192


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _run_inflate(dev, cases):
    """cases [(stream, expected length, stored)] -> (status list, the output buffer as numpy, [(slot offset, length)]): streams at
    unaligned input offsets with junk between them, slots separated by poisoned guard bands."""
    from streamflow_amd import ops
    comp, desc, slots = bytearray(b"\xEE" * 3), [], []
    out_at = GUARD + 1
    for k, (s, n, stored) in enumerate(cases):
        desc.append((len(comp), len(s), out_at, n, 1 if stored else 0))
        slots.append((out_at, n))
        comp += bytes(s) + b"\xEE" * (1 + k % 5)                              # odd gaps: every alignment of the input offset
        out_at += n + GUARD + k % 3
    out = torch.full((out_at,), POISON, dtype=torch.uint8, device=dev)
    c = torch.from_numpy(np.frombuffer(bytes(comp), np.uint8).copy()).to(dev)
    status = ops.inflate(c, torch.tensor(desc, dtype=torch.int64, device=dev), out)
    return status.cpu().tolist(), out.cpu().numpy(), slots


def _guards_untouched(buf, slots):
    mask = np.ones(buf.size, bool)
    for at, n in slots:
        mask[at:at + n] = False
    return bool((buf[mask] == POISON).all())


def test_inflate_good_streams(dev):
    good = dc.good_streams()
    cases = [(s, len(d), False) for _, s, d in good]
    status, buf, slots = _run_inflate(dev, cases)
    for (name, _, d), st, (at, n) in zip(good, status, slots):
        assert st == dc.OK, (name, dc.STATUS_NAMES[st])
        assert buf[at:at + n].tobytes() == d, name
    assert _guards_untouched(buf, slots)
    status2, buf2, _ = _run_inflate(dev, cases)
    assert status2 == status and np.array_equal(buf, buf2)


def test_inflate_bad_streams_between_good_ones(dev):
    good, bad = dc.good_streams(), dc.bad_streams()
    pick = [g for g in good if g[0] in ("text-l5-default", "chunk-l5", "run-l9", "n64-l0-fixed", "writer-37x53-c0", "empty-l9-default")]
    raw = bytes(range(256)) * 2
    cases, want = [], []
    for k, (name, s, n, status) in enumerate(bad):
        g = pick[k % len(pick)]
        cases += [(g[1], len(g[2]), False), (s, n, False)]
        want += [(dc.OK, g[2]), (status, None)]
    cases += [(raw, len(raw), True), (raw, len(raw) - 1, True), (raw, len(raw) + 1, True), (b"", 0, True)]
    want += [(dc.OK, raw), (dc.OUTPUT_LONG, None), (dc.OUTPUT_SHORT, None), (dc.OK, b"")]
    status, buf, slots = _run_inflate(dev, cases)
    for k, ((st_want, data), st, (at, n)) in enumerate(zip(want, status, slots)):
        assert st == st_want, (k, dc.STATUS_NAMES[st], dc.STATUS_NAMES[st_want])
        if data is not None:
            assert buf[at:at + n].tobytes() == data, k
    assert _guards_untouched(buf, slots)                                      # a failed stream writes inside its own slot only


def test_inflate_refuses_slots_outside_the_buffers(dev):
    from streamflow_amd import ops
    s, d = dc.good("n64-l5-default")
    comp = torch.from_numpy(np.frombuffer(s, np.uint8).copy()).to(dev)
    out = torch.full((256,), POISON, dtype=torch.uint8, device=dev)
    desc = [(0, len(s), 0, 64, 0), (0, len(s) + 1, 64, 64, 0), (-1, 4, 64, 64, 0), (0, len(s), 200, 64, 0), (0, len(s), 128, -1, 0),
            (1 << 62, 1 << 62, 64, 64, 0), (0, len(s), 1 << 62, 1 << 62, 0)]
    status = ops.inflate(comp, torch.tensor(desc, dtype=torch.int64, device=dev), out).cpu().tolist()
    assert status == [dc.OK] + [dc.BAD_SLOT] * 6
    got = out.cpu().numpy()
    assert got[:64].tobytes() == d and bool((got[64:] == POISON).all())
    with pytest.raises(RuntimeError, match="desc"):
        ops.inflate(comp, torch.zeros(1, 4, dtype=torch.int64, device=dev), out)


ASSEMBLE = [((37, 53), (19, 53, 2), False), ((136, 240), (34, 60, 1), False), ((33, 40), (8, 16, 2), True), ((70, 9), (3, 9, 2), False),
            ((70, 9), (24, 4, 1), True)]


@pytest.mark.parametrize("n", (1, 3))
@pytest.mark.parametrize("case", ASSEMBLE, ids=lambda c: "x".join(map(str, c[0] + c[1])) + ("s" if c[2] else ""))
def test_flo5_assemble(dev, case, n):
    """Raw chunks in shuffled slot order, one chunk of every file missing, a slot index out of range standing for another."""
    from streamflow_amd import ops
    (h, w), (ch, cw, cc), shuffle = case
    gy, gx, gc = -(-h // ch), -(-w // cw), 2 // cc
    size = 4 * ch * cw * cc
    stride = size + 8                                                         # slots need not be packed
    rng = np.random.default_rng(h * 7 + n)
    cells = [(i, y, x, c) for i in range(n) for y in range(gy) for x in range(gx) for c in range(gc)]
    order = rng.permutation(len(cells))
    slots = np.full((len(cells), stride), POISON, np.uint8)
    grid = np.full((n, gy, gx, gc), -1, np.int32)
    want = []
    for i in range(n):
        f = dc.smooth_field(h, w, 10 + i)
        chunks = {}
        for y in range(gy):
            for x in range(gx):
                for c in range(gc):
                    if (y, x, c) == ((i + 1) % gy, i % gx, i % gc):           # missing: stays -1 (file 1), or an index out of range
                        grid[i, y, x, c] = -1 if i != 1 else len(cells) + 5
                        continue
                    buf = np.zeros((ch, cw, cc), "<f4")
                    part = f[y * ch:(y + 1) * ch, x * cw:(x + 1) * cw, c * cc:(c + 1) * cc]
                    buf[:part.shape[0], :part.shape[1]] = part
                    raw = np.frombuffer(buf.tobytes(), np.uint8)
                    if shuffle:
                        raw = np.ascontiguousarray(raw.reshape(-1, 4).T).reshape(-1)
                    s = int(order[cells.index((i, y, x, c))])
                    slots[s, :size] = raw
                    grid[i, y, x, c] = s
                    chunks[(y, x, c)] = raw.tobytes()
        want.append(dc.assemble_ref((h, w, 2), (ch, cw, cc), shuffle, chunks))
    got = ops.flo5_assemble(torch.from_numpy(slots).to(dev), torch.from_numpy(grid).to(dev), h, w, (ch, cw, cc), shuffle)
    assert got.shape == (n, h, w, 2) and got.dtype == torch.float32
    assert np.array_equal(got.cpu().numpy().view(np.uint32), np.stack(want))


@pytest.fixture(scope="module")
def files(tmp_path_factory, dev):
    """Paths: every h5py-written fixture, write_flo5 and write_batch files, tiled_file outputs."""
    from streamflow_amd import flo5, flo5_gpu
    d = tmp_path_factory.mktemp("flo5_decode")
    out = sorted(glob.glob(os.path.join(GOLD, "flo5", "*.flo5"))) + sorted(glob.glob(os.path.join(GOLD, "flo5_decode", "*.flo5")))
    assert len(out) == 9
    for k, (h, w, rpc) in enumerate(((37, 53, 0), (64, 96, 5), (1, 1, 0))):
        p = str(d / f"host_writer_{k}.flo5")
        flo5.write_flo5(p, dc.smooth_field(h, w, 20 + k), rows_per_chunk=rpc)
        out.append(p)
    flows = torch.from_numpy(np.stack([ec.make(70, 96, 30 + k, special=True) for k in range(2)])).to(dev)
    gpu_paths = [str(d / f"gpu_writer_{k}.flo5") for k in range(2)]
    flo5_gpu.write_batch(flows, gpu_paths)
    out += gpu_paths
    tiled = [((136, 240), (34, 60, 1), 5, False, ((1, 2, 0),), ((3, 3, 1),)), ((33, 40), (8, 16, 2), 9, True, ((2, 1, 0),), ()),
             ((136, 240), (34, 60, 1), 1, False, (), ()), ((70, 9), (24, 4, 1), 6, True, (), ((0, 1, 1),))]
    for k, ((h, w), cs, level, shuffle, skip, missing) in enumerate(tiled):
        p = str(d / f"tiled_{k}.flo5")
        with open(p, "wb") as f:
            f.write(dc.tiled_file(dc.smooth_field(h, w, 40 + k), cs, level, shuffle, skip, missing))
        out.append(p)
    return out


@pytest.mark.parametrize("inflate", ("gpu", "host", None))
def test_read_batch_equals_read_flo5(dev, files, inflate):
    from streamflow_amd import flo5, flo5_gpu
    got = flo5_gpu.read_batch(files, dev, inflate=inflate)
    assert len(got) == len(files)
    for p, g in zip(files, got):
        want = flo5.read_flo5(p)
        assert g.device == dev and tuple(g.shape) == want.shape, p
        a = g.cpu().numpy()
        assert a.dtype == want.dtype.newbyteorder("="), p
        bits = np.dtype(f"u{a.dtype.itemsize}")
        assert np.array_equal(a.view(bits), np.ascontiguousarray(want.astype(a.dtype)).view(bits)), p
    f64 = got[[os.path.basename(p) for p in files].index("f64_contiguous.flo5")]
    assert f64.dtype == torch.float64                                         # through the fallback, with its dtype
    assert flo5_gpu.read_batch([], dev) == []


def test_read_batch_routes_large_chunks_to_the_host(dev, files, monkeypatch):
    """Above HOST_INFLATE_CHUNK_BYTES a file's chunks are inflated by the pool; below, by sf_inflate: the same bits either way."""
    from streamflow_amd import flo5, flo5_gpu, ops
    calls = []
    real = ops.inflate
    monkeypatch.setattr(ops, "inflate", lambda c, d, o: (calls.append(int(d.shape[0])), real(c, d, o))[1])
    p = next(f for f in files if f.endswith("host_writer_1.flo5"))            # 13 chunks of 5 x 96 x 2 floats = 3840 bytes
    want = flo5.read_flo5(p).view(np.uint32)
    monkeypatch.setattr(flo5_gpu, "HOST_INFLATE_CHUNK_BYTES", 3840)
    assert np.array_equal(flo5_gpu.read_batch([p], dev, inflate="gpu")[0].cpu().numpy().view(np.uint32), want) and calls == [13]
    monkeypatch.setattr(flo5_gpu, "HOST_INFLATE_CHUNK_BYTES", 3839)
    assert np.array_equal(flo5_gpu.read_batch([p], dev, inflate="gpu")[0].cpu().numpy().view(np.uint32), want) and calls == [13]


@pytest.mark.parametrize("inflate", ("gpu", "host"))
def test_read_batch_raises_on_a_corrupt_chunk(dev, files, tmp_path, inflate):
    from streamflow_amd import flo5, flo5_gpu
    src = os.path.join(GOLD, "flo5_decode", "auto_gzip5.flo5")
    blob = bytearray(open(src, "rb").read())
    offs, addr, nbytes, _ = flo5.chunk_table(bytes(blob))["chunks"][5]
    blob[addr + nbytes - 2] ^= 0x40                                           # the chunk's Adler-32: one flipped bit
    bad = str(tmp_path / "flipped.flo5")
    with open(bad, "wb") as f:
        f.write(bytes(blob))
    with pytest.raises(IOError, match="flipped.flo5") as e:
        flo5_gpu.read_batch([src, bad], dev, inflate=inflate)
    assert str(offs) in str(e.value)
    # strict where the host reader is lax: a chunk that inflates to more than the chunk
    import zlib
    a = dc.smooth_field(16, 16, 1, holes=False)
    good = dc.tiled_file(a, (8, 16, 2), 5)
    t = flo5.chunk_table(good)
    offs, addr, nbytes, _ = t["chunks"][1]
    assert addr + nbytes == len(good)                                         # the last chunk: replace it by a longer one
    longer = zlib.compress(zlib.decompress(good[addr:]) + b"\0" * 4, 5)
    key = good.index(nbytes.to_bytes(4, "little") + b"\0\0\0\0" + (8).to_bytes(8, "little"))
    lax = good[:key] + len(longer).to_bytes(4, "little") + good[key + 4:addr] + longer
    lax = lax[:40] + len(lax).to_bytes(8, "little") + lax[48:]                # the superblock's end-of-file address
    p = str(tmp_path / "long_chunk.flo5")
    with open(p, "wb") as f:
        f.write(lax)
    assert np.array_equal(flo5.read_flo5(p), a)                               # the host reader ignores the extra bytes
    with pytest.raises(IOError, match="long_chunk.flo5"):
        flo5_gpu.read_batch([p], dev, inflate=inflate)


def test_spring_report_with_gpu_decode_equals_host_decode(dev, tmp_path, monkeypatch):
    """A small Spring tree with ground truth at twice the frame size in h5py's tiled layout: flo5_decode="gpu" reads a clip's ground
    truth with one read_batch call and reports exactly what "host" reports, key for key."""
    from streamflow_amd import evaluate, flo5_gpu, flow_io
    from tests import score_cases as sc
    from tests.test_gpu_spring import H, ITERS, T, W, _models, _smooth_frames
    rng = np.random.default_rng(11)
    n = 4
    for cam in ("left", "right"):
        d = tmp_path / "train" / "0041" / f"frame_{cam}"
        os.makedirs(d)
        for i, img in enumerate(_smooth_frames(rng, n, H, W)):
            flow_io.write_png(str(d / f"frame_{cam}_{i + 1:04d}.png"), img)
        for direction in ("FW", "BW"):
            os.makedirs(tmp_path / "train" / "0041" / f"flow_{direction}_{cam}")
            for a in (range(n - 1) if direction == "FW" else range(1, n)):
                gt = sc.random_gt(rng, H, W, 2, 0.1)
                with open(tmp_path / "train" / "0041" / f"flow_{direction}_{cam}" / f"flow_{direction}_{cam}_{a + 1:04d}.flo5", "wb") as f:
                    f.write(dc.tiled_file(gt, (31, 94, 1), 5))
    model, _ = _models(dev, T, "fp32_class")
    host = evaluate.spring_report(model, iters=ITERS, root=str(tmp_path), nframes=T, device=dev)
    calls = []
    real = flo5_gpu.read_batch
    monkeypatch.setattr(flo5_gpu, "read_batch", lambda paths, device, **kw: (calls.append(len(paths)), real(paths, device, **kw))[1])
    gpu = evaluate.spring_report(model, iters=ITERS, root=str(tmp_path), nframes=T, device=dev, flo5_decode="gpu")
    assert calls and sum(calls) == host["pairs"] == gpu["pairs"] > 0
    assert set(gpu) == set(host)
    for k in host:
        assert gpu[k] == host[k] or (np.isnan(gpu[k]) and np.isnan(host[k])), (k, gpu[k], host[k])
