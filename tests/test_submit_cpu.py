"""The leaderboard writers (streamflow_amd/submit.py) on the CPU: small synthetic Sintel / multi-frame KITTI test trees in
tmp_path, a stub model whose output is known in closed form, vis=False (no kernel is launched).  Checked: the exact set of files,
their names (frame%04d.flo numbering, nothing for pairs with frame id -1, the tail clip aligned to the scene's end), their
contents after unpadding, and the warm-start chain."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from streamflow_amd import flow_io, submit

H, W = 44, 60                          # padded to 48 x 64 ('sintel' mode: 2 rows / 2 columns on every side)
HP, WP, TOP, LEFT = 48, 64, 2, 2
SCENES = {"ambush_1": 5, "bamboo_3": 4, "cave_3": 3}


def _frame(rng, scene, idx):
    img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    img[0, 0] = (scene, idx, 9)                                          # the stub reads (scene, frame) back from here
    return img


def _sintel_tree(root):
    rng = np.random.default_rng(0)
    for s, (scene, n) in enumerate(SCENES.items()):
        for d, dstype in enumerate(("clean", "final")):
            os.makedirs(root / "test" / dstype / scene)
            for i in range(n):
                flow_io.write_png(str(root / "test" / dstype / scene / f"frame_{i + 1:04d}.png"), _frame(rng, 10 * d + s, i))


def _stub_flow(tag, idx):
    """Padded flow [1, 2, HP, WP] of the pair that starts at frame `idx` of scene tag `tag`: position dependent, so that a wrong
    unpad shows."""
    yy, xx = torch.meshgrid(torch.arange(HP, dtype=torch.float32), torch.arange(WP, dtype=torch.float32), indexing="ij")
    return torch.stack([xx * 0.25 + tag + 0.5 * idx, yy * -0.125 + idx])[None]


def _want(tag, idx):
    return _stub_flow(tag, idx)[0, :, TOP:TOP + H, LEFT:LEFT + W].permute(1, 2, 0).numpy()


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_sintel_writer_files_and_contents(tmp_path):
    T = 3
    _sintel_tree(tmp_path / "sintel")
    calls = []

    def model(images, iters=0, test_mode=False):
        assert test_mode and iters == 4 and len(images) == T and all(im.shape == (1, 3, HP, WP) for im in images)
        tags = [(int(im[0, 0, TOP, LEFT]), int(im[0, 1, TOP, LEFT])) for im in images]
        calls.append(tags[0])
        return [_stub_flow(t, i) for t, i in tags[:-1]]

    out = tmp_path / "out"
    submit.create_sintel_submission_mf(Namespace(sintel_root=str(tmp_path / "sintel")), model, 4, output_path=str(out), nframes=T,
                                       vis=False)
    want_files = sorted(os.path.join(dstype, scene, "frame%04d.flo" % (i + 1))
                        for dstype in ("clean", "final") for scene, n in SCENES.items() for i in range(n - 1))
    assert _files(out) == want_files                                     # every pair once, no PNG with vis=False
    for d, dstype in enumerate(("clean", "final")):
        for s, (scene, n) in enumerate(SCENES.items()):
            for i in range(n - 1):
                got = flow_io.read_flo(str(out / dstype / scene / ("frame%04d.flo" % (i + 1))))
                assert got.shape == (H, W, 2) and np.array_equal(got, _want(10 * d + s, i)), (dstype, scene, i)
    # 5 frames: clips at 0, 2; 4 frames: clip at 0 and the tail clip at 1 (its first pair has id -1); 3 frames: one clip
    assert calls == [(0, 0), (0, 2), (1, 0), (1, 1), (2, 0), (10, 0), (10, 2), (11, 0), (11, 1), (12, 0)]


def test_sintel_writer_tail_clip_skips_written_pairs(tmp_path):
    """T = 4 on 6 frames: one full clip (pairs 0..2) and a tail clip at frame 2 with ids [-1, 3, 4, 5]: its first pair is NOT
    written again (the stub would write a different value there)."""
    T = 4
    rng = np.random.default_rng(1)
    for dstype in ("clean", "final"):
        os.makedirs(tmp_path / "s" / "test" / dstype / "market_4")
        for i in range(6):
            flow_io.write_png(str(tmp_path / "s" / "test" / dstype / "market_4" / f"frame_{i + 1:04d}.png"), _frame(rng, 7, i))
    clip_no = [0]

    def model(images, iters=0, test_mode=False):
        first = int(images[0][0, 1, TOP, LEFT])
        clip_no[0] += 1
        return [_stub_flow(100 * clip_no[0], first + k) for k in range(T - 1)]

    out = tmp_path / "out"
    submit.create_sintel_submission_mf(Namespace(sintel_root=str(tmp_path / "s")), model, 2, output_path=str(out), nframes=T, vis=False)
    assert _files(out / "clean") == [os.path.join("market_4", "frame%04d.flo" % i) for i in range(1, 6)]
    for i in range(5):
        clip = 1 if i < 3 else 2
        assert np.array_equal(flow_io.read_flo(str(out / "clean" / "market_4" / ("frame%04d.flo" % (i + 1)))), _want(100 * clip, i))


def test_sintel_warmup_writer_chain(tmp_path, monkeypatch):
    """Every clip receives the forward-interpolated low-resolution flows of the previous clip of ITS scene; the chain restarts at a
    scene change.  The writer reuses demo.predict_clips_warm_start, which spells the reference's `flow_init=None` restart as
    zero flows (the same start, and the model then returns the low-resolution fields too): the stub must see zeros there."""
    from streamflow_amd import utils
    T = 3
    _sintel_tree(tmp_path / "sintel")
    monkeypatch.setattr(utils, "forward_interpolate", lambda f: f * 2.0 + 1.0)
    seen = []

    def model(images, iters=0, flow_init=None, test_mode=False):
        assert test_mode and iters == 5 and flow_init is not None and len(flow_init) == T - 1
        assert all(f.shape == (1, 2, HP // 8, WP // 8) for f in flow_init)
        tags = [(int(im[0, 0, TOP, LEFT]), int(im[0, 1, TOP, LEFT])) for im in images]
        seen.append((tags[0], [float(f.mean()) for f in flow_init], [bool((f == f.flatten()[0]).all()) for f in flow_init]))
        low = [torch.full((1, 2, HP // 8, WP // 8), float(100 * t + 10 * i + k)) for k, (t, i) in enumerate(tags[:-1])]
        return [_stub_flow(t, i) for t, i in tags[:-1]], low

    out = tmp_path / "out"
    submit.create_sintel_submission_mf_warmup(Namespace(sintel_root=str(tmp_path / "sintel")), model, 5, output_path=str(out),
                                              nframes=T, vis=False)
    want_files = sorted(os.path.join(dstype, scene, "frame%04d.flo" % (i + 1))
                        for dstype in ("clean", "final") for scene, n in SCENES.items() for i in range(n - 1))
    assert _files(out) == want_files
    for s, (scene, n) in enumerate(SCENES.items()):
        for i in range(n - 1):
            assert np.array_equal(flow_io.read_flo(str(out / "final" / scene / ("frame%04d.flo" % (i + 1)))), _want(10 + s, i))
    assert all(all(c) for _, _, c in seen)
    got = [(tag, init) for tag, init, _ in seen[:5]]                      # the clean pass: scenes 0 (clips 0, 2), 1 (0, tail 1), 2 (0)
    assert got == [((0, 0), [0.0, 0.0]),                                 # scene start: zeros
                   ((0, 2), [2.0 * 0 + 1.0, 2.0 * 11 + 1.0]),             # low = 100 * 0 + 10 * i + k of clip (0, 0): 0, 11
                   ((1, 0), [0.0, 0.0]),                                 # scene change: the chain restarts
                   ((1, 1), [2.0 * 100 + 1.0, 2.0 * 111 + 1.0]),
                   ((2, 0), [0.0, 0.0])]
    assert seen[5][0] == (10, 0) and seen[5][1] == [0.0, 0.0]            # ... and with the render pass


def test_kitti_writer_files_and_contents(tmp_path):
    T = 3
    Hk, Wk = 37, 124                                                     # default padder mode: 40 x 128, top 1, left 2
    rng = np.random.default_rng(2)
    os.makedirs(tmp_path / "kitti" / "testing" / "image_2")
    for s in (0, 3, 17):
        for fr in range(12 - T, 12):
            img = rng.integers(0, 256, size=(Hk, Wk, 3), dtype=np.uint8)
            img[0, 0] = (s, fr, 1)
            flow_io.write_png(str(tmp_path / "kitti" / "testing" / "image_2" / ("%06d_%02d.png" % (s, fr))), img)

    def flow_of(s):
        yy, xx = torch.meshgrid(torch.arange(40, dtype=torch.float32), torch.arange(128, dtype=torch.float32), indexing="ij")
        return torch.stack([xx * 0.5 - 20 + s, yy * 0.25 - s])[None]     # multiples of 1/64: exact through the 16-bit code

    def model(images, iters=0, test_mode=False):
        assert test_mode and iters == 3 and len(images) == T and images[0].shape == (1, 3, 40, 128)
        assert [int(im[0, 1, 1, 2]) for im in images] == [9, 10, 11]
        return [torch.full((1, 2, 40, 128), 1e3)] * (T - 2) + [flow_of(int(images[-2][0, 0, 1, 2]))]

    out = tmp_path / "out"
    submit.create_kitti_submission_mf(Namespace(multi_root=str(tmp_path / "kitti")), model, 3, output_path=str(out), nframes=T)
    assert _files(out) == ["000000_10.png", "000003_10.png", "000017_10.png"]
    assert _files(tmp_path) and not os.path.exists("vis_kitti2")         # nothing lands in the working directory
    for s in (0, 3, 17):
        flow, valid = flow_io.read_flow_kitti(str(out / ("%06d_10.png" % s)))
        want = flow_of(s)[0, :, 1:1 + Hk, 2:2 + Wk].permute(1, 2, 0).numpy()
        assert flow.shape == (Hk, Wk, 2) and np.array_equal(flow, want) and (valid == 1).all()


def test_writers_with_vis_need_the_gpu(tmp_path):
    """vis=True colours on the device: with a CPU model's flows it fails loudly instead of colouring on the host."""
    _sintel_tree(tmp_path / "sintel")

    def model(images, iters=0, test_mode=False):
        return [torch.zeros(1, 2, HP, WP) for _ in images[:-1]]

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        submit.create_sintel_submission_mf(Namespace(sintel_root=str(tmp_path / "sintel")), model, 1, output_path=str(tmp_path / "o"),
                                           nframes=3)
