"""Flow colouring on the GPU: the sf_flow_to_image kernel (csrc/flow_viz.hip) against the reference's recorded images
(tests/golden/flow_viz.npz) and against the numpy restatement of tests/viz_cases.py at the sizes users run; per-field maxima,
fixed scale, BGR, clamp, non-finite pixels, guarded output buffers, graph capture; the submission writers and demo.vis_flow with
the HIP model.

Image criterion (vc.assert_image_close): every operation but the angle is reproduced one for one and the colour is continuous in
the angle, so a different last bit of arctan2 moves a byte by at most one level: max |difference| <= 1 level on every channel and
at most 1e-4 of the pixels of a case differ at all (one pixel for cases under 10 000 pixels)."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import viz_cases as vc

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _nchw(field_hw2):
    return torch.from_numpy(np.ascontiguousarray(field_hw2.transpose(2, 0, 1)))[None]


@pytest.mark.parametrize("name", list(vc.CASES))
def test_golden_cases_vs_reference_images(dev, golden, name):
    from streamflow_amd import flow_viz, ops
    want = golden("flow_viz")[name]
    kw = vc.KWARGS.get(name, {})
    got = ops.flow_to_image(_nchw(vc.field(name)).to(dev), **kw).cpu().numpy()[0]
    vc.assert_image_close(got, want, name)
    got2 = flow_viz.flow_to_image(vc.field(name), **kw)                    # the reference's call: [H, W, 2] numpy in, numpy out
    assert got2.dtype == np.uint8 and np.array_equal(got2, got)
    assert np.array_equal(flow_viz.flow_to_image(_nchw(vc.field(name))[0].to(dev), **kw), got)        # device [2, H, W]


def test_ramp_sign_of_zero(dev, golden):
    """v = +0 and v = -0 at u > 0 are the two sides of the wheel's discontinuity: exactly the reference's colours there."""
    from streamflow_amd import ops
    ramp = vc.field("ramp")
    got = ops.flow_to_image(_nchw(ramp).to(dev)).cpu().numpy()[0]
    zero = (ramp[..., 1] == 0) & (ramp[..., 0] > 0)
    assert zero.sum() >= 256
    diff = np.abs(got[zero].astype(int) - golden("flow_viz")["ramp"][zero].astype(int))
    assert diff.max() <= 1 and (diff.max(axis=1) > 0).sum() <= 1


@pytest.mark.parametrize("H,W", [(436, 1024), (1080, 1920), (375, 1242)])
@pytest.mark.parametrize("N", [1, 3, 7])
def test_batches_vs_restatement(dev, H, W, N):
    """N fields of very different magnitudes in one call: every field on its own scale (no maximum leaks into a neighbour), and
    rad_max_ws bitwise np.max of the fp32 radii."""
    from streamflow_amd import ops
    scales = [3e-3, 40.0, 1.5, 900.0, 0.2, 7.0, 1e-6][:N]
    flows = vc.gaussian_fields(N, H, W, scales, seed=H + N)
    img, ws = ops.flow_to_image(torch.from_numpy(flows).to(dev), return_rad_max=True)
    img, ws = img.cpu().numpy(), ws.cpu().numpy()
    assert img.shape == (N, H, W, 3) and img.dtype == np.uint8
    for i in range(N):
        hw2 = flows[i].transpose(1, 2, 0)
        want_m = vc.rad_max_np(hw2)
        assert ws[i].tobytes() == want_m.tobytes(), (i, ws[i], want_m)
        vc.assert_image_close(img[i], vc.flow_to_image_np(hw2), f"{H}x{W} field {i} of {N} (scale {scales[i]})")


def test_fixed_rad_max_bgr_clip(dev):
    from streamflow_amd import ops
    flows = vc.gaussian_fields(2, 123, 250, [6.0, 2.0], seed=5)            # 30750 pixels: h * w % 4 = 2
    t = torch.from_numpy(flows).to(dev)
    fixed = ops.flow_to_image(t, rad_max=4.0).cpu().numpy()
    assert ops.flow_to_image(t, rad_max=4.0, return_rad_max=True)[1] is None
    for i in range(2):
        hw2 = flows[i].transpose(1, 2, 0)
        vc.assert_image_close(fixed[i], vc.flow_to_image_np(hw2, rad_max=4.0), f"rad_max=4 field {i}")
    rad = np.sqrt((flows[0] ** 2).sum(0))
    over = rad > 4.1
    assert over.sum() > 1000 and fixed[0][over].max() <= 191                # the 0.75 branch: floor(255 * 0.75 col)
    bgr = ops.flow_to_image(t, convert_to_bgr=True).cpu().numpy()
    rgb = ops.flow_to_image(t).cpu().numpy()
    assert np.array_equal(bgr, rgb[..., ::-1])
    clip = ops.flow_to_image(t, clip_flow=3.0, return_rad_max=True)
    for i in range(2):
        hw2 = flows[i].transpose(1, 2, 0)
        assert clip[1][i].item() == vc.rad_max_np(hw2, clip_flow=3.0)
        vc.assert_image_close(clip[0][i].cpu().numpy(), vc.flow_to_image_np(hw2, clip_flow=3.0), f"clip_flow=3 field {i}")
    with pytest.raises(RuntimeError, match=">= 0"):
        ops.flow_to_image(t, rad_max=-1.0)
    with pytest.raises(RuntimeError, match="expected flows"):
        ops.flow_to_image(t[0])


def test_non_finite_pixels_and_zero_field(dev):
    from streamflow_amd import ops
    flows = vc.gaussian_fields(3, 64, 100, [5.0, 5.0, 5.0], seed=9)
    flows[2] = 0.0
    bad = [(0, 0, 3, 7, np.nan), (0, 1, 10, 11, np.inf), (0, 0, 63, 99, -np.inf), (0, 1, 0, 0, np.nan), (1, 0, 20, 20, np.inf)]
    for i, c, y, x, val in bad:
        flows[i, c, y, x] = val
    flows[0, 0, 5, 5], flows[0, 1, 5, 5] = 1e15, 0.0                        # finite: stays in, and IS the maximum
    img, ws = ops.flow_to_image(torch.from_numpy(flows).to(dev), return_rad_max=True)
    img, ws = img.cpu().numpy(), ws.cpu().numpy()
    assert np.isfinite(ws).all() and 0.99e15 < ws[0] < 1.01e15 and ws[2] == 0.0
    for i, c, y, x, val in bad:
        assert tuple(img[i, y, x]) == (0, 0, 0)
    assert (img[2] == 255).all()                                           # all-zero field: white
    for i in range(2):
        hw2 = flows[i].transpose(1, 2, 0)
        assert ws[i].tobytes() == vc.rad_max_np(hw2).tobytes()
        vc.assert_image_close(img[i], vc.flow_to_image_np(hw2), f"non-finite field {i}")
    assert ((img[1] == 0).all(axis=2)).sum() == 1                           # only the painted pixel is black


@pytest.mark.parametrize("H,W,offset", [(64, 96, 64), (64, 96, 61), (37, 61, 64), (37, 61, 63), (3, 5, 6), (1, 1, 1), (1, 3, 2)])
@pytest.mark.parametrize("N", [1, 3])
def test_output_stays_inside_its_buffer(dev, H, W, offset, N):
    """The 12-byte stores and the tails: the images sit at `offset` inside a sentinel-filled byte buffer (aligned and unaligned,
    pixel counts that are and are not multiples of four); everything around them stays intact and the images are right."""
    from streamflow_amd import _lib
    flows = vc.gaussian_fields(N, H, W, [4.0, 0.5, 30.0][:N], seed=offset)
    t = torch.from_numpy(flows).to(dev)
    nbytes = N * H * W * 3
    buf = torch.full((offset + nbytes + 256,), SENTINEL, dtype=torch.uint8, device=dev)
    ws = torch.full((N + 2,), -7.0, device=dev)
    _lib.check(_lib.load().sf_flow_to_image(t.data_ptr(), buf.data_ptr() + offset, ws.data_ptr() + 4, N, H, W, -1.0, -1.0, 0,
                                            _lib.stream()), "sf_flow_to_image")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:offset] == SENTINEL).all() and (host[offset + nbytes:] == SENTINEL).all()
    assert ws[0].item() == -7.0 and ws[N + 1].item() == -7.0
    img = host[offset:offset + nbytes].reshape(N, H, W, 3)
    for i in range(N):
        vc.assert_image_close(img[i], vc.flow_to_image_np(flows[i].transpose(1, 2, 0)), f"{H}x{W}@{offset} field {i}")


def test_inside_graph_capture(dev):
    """Memset + two kernels on the capturing stream, no host synchronisation: captured once, replayed three times with new
    input in the static buffers, equal to the eager call every time."""
    from streamflow_amd import _lib
    N, H, W = 3, 120, 200
    static_in = torch.zeros(N, 2, H, W, device=dev)
    out = torch.zeros(N, H, W, 3, dtype=torch.uint8, device=dev)
    ws = torch.zeros(N, device=dev)

    def call(src, dst, w):
        _lib.check(_lib.load().sf_flow_to_image(src.data_ptr(), dst.data_ptr(), w.data_ptr(), N, H, W, -1.0, -1.0, 0, _lib.stream()),
                   "sf_flow_to_image")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(static_in, out, ws)                                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(static_in, out, ws)
    for r in range(3):
        flows = torch.from_numpy(vc.gaussian_fields(N, H, W, [1.0 + r, 50.0, 0.01 * (r + 1)], seed=20 + r)).to(dev)
        static_in.copy_(flows)
        graph.replay()
        torch.cuda.synchronize()
        eager, eager_ws = torch.empty_like(out), torch.empty_like(ws)
        call(flows, eager, eager_ws)
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(ws, eager_ws), r
        vc.assert_image_close(out[0].cpu().numpy(), vc.flow_to_image_np(flows[0].cpu().numpy().transpose(1, 2, 0)), f"replay {r}")


# ---- the writers with the HIP model ------------------------------------------------------------------------------------
def _model(dev, T):
    from tests.test_gpu_evaluate import _models
    return _models(dev, T, "fp32_class")[0]


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warmup"])
def test_sintel_writers_with_the_hip_model(tmp_path, dev, warm):
    from streamflow_amd import flow_io, flow_viz, submit
    from tests.test_gpu_evaluate import _smooth_frames
    rng = np.random.default_rng(6)
    H, W, T, iters = 124, 188, 3, 3
    scenes = {"ambush_9": 5, "cave_9": 4}
    for scene, n in scenes.items():
        for dstype in ("clean", "final"):
            os.makedirs(tmp_path / "test" / dstype / scene)
            for i, img in enumerate(_smooth_frames(rng, n, H, W)):
                flow_io.write_png(str(tmp_path / "test" / dstype / scene / f"frame_{i + 1:04d}.png"), img)
    out = tmp_path / "out"
    fn = submit.create_sintel_submission_mf_warmup if warm else submit.create_sintel_submission_mf
    fn(Namespace(sintel_root=str(tmp_path)), _model(dev, T), iters, output_path=str(out), nframes=T)
    want = sorted([os.path.join(d, s, "frame%04d.flo" % (i + 1)) for d in ("clean", "final") for s, n in scenes.items() for i in range(n - 1)]
                  + [os.path.join(d, "%s-%d.png" % (s, i + 1)) for d in ("clean", "final") for s, n in scenes.items() for i in range(n - 1)])
    assert _files(out) == want
    for d in ("clean", "final"):
        for s, n in scenes.items():
            for i in range(n - 1):
                flo = flow_io.read_flo(str(out / d / s / ("frame%04d.flo" % (i + 1))))
                png = flow_io.read_png(str(out / d / ("%s-%d.png" % (s, i + 1))))
                assert flo.shape == (H, W, 2) and np.isfinite(flo).all() and np.abs(flo).max() > 0
                assert png.shape == (H, W, 3) and png.dtype == np.uint8
                assert np.array_equal(png, flow_viz.flow_to_image(flo)), (d, s, i)


def test_kitti_writer_and_vis_flow_with_the_hip_model(tmp_path, dev):
    from streamflow_amd import demo, flow_io, flow_viz, submit
    from streamflow_amd.utils import InputPadder
    from tests.test_gpu_evaluate import _smooth_frames
    rng = np.random.default_rng(7)
    H, W, T, iters = 122, 180, 3, 3
    os.makedirs(tmp_path / "testing" / "image_2")
    for s in range(2):
        for i, img in zip(range(12 - T, 12), _smooth_frames(rng, T, H, W)):
            flow_io.write_png(str(tmp_path / "testing" / "image_2" / ("%06d_%02d.png" % (s, i))), img)
    hip_model, produced = _model(dev, T), []

    def model(images, iters, test_mode):                                   # keeps what the model returned, padded
        produced.append(hip_model(images, iters=iters, test_mode=test_mode))
        return produced[-1]

    out, vis = tmp_path / "out", tmp_path / "vis"
    submit.create_kitti_submission_mf(Namespace(multi_root=str(tmp_path)), model, iters, output_path=str(out), nframes=T,
                                      vis_path=str(vis), device=dev)
    assert _files(out) == ["000000_10.png", "000001_10.png"] and _files(vis) == ["flow/000000_10.png", "flow/000001_10.png"]
    fields = []
    for s in range(2):
        flow = InputPadder((H, W)).unpad(produced[s][-1][0]).contiguous()
        fields.append(flow)
        png = flow_io.read_png(str(vis / "flow" / ("%06d_10.png" % s)))
        assert png.shape == (H, W, 3) and np.array_equal(png, flow_viz.flow_to_image(flow))      # coloured before the 16-bit code
        got, valid = flow_io.read_flow_kitti(str(out / ("%06d_10.png" % s)))
        assert got.shape == (H, W, 2) and (valid == 1).all()
        assert np.abs(got - flow.permute(1, 2, 0).cpu().numpy()).max() <= 1.0 / 64
    # demo.vis_flow: one PNG per field (CPU tensors as predict_frames returns them), own scale each; then one fixed scale
    paths = demo.vis_flow([f.cpu() for f in fields] + [fields[0][:, :50, :70].cpu()], str(tmp_path / "seq"))
    assert [os.path.basename(p) for p in paths] == ["frame_0000.png", "frame_0001.png", "frame_0002.png"] and _files(tmp_path / "seq") == [os.path.basename(p) for p in paths]
    for p, f in zip(paths, fields + [fields[0][:, :50, :70]]):
        assert np.array_equal(flow_io.read_png(p), flow_viz.flow_to_image(f.contiguous()))
    paths = demo.vis_flow(fields, str(tmp_path / "seq_fixed"), rad_max=2.0)
    assert np.array_equal(flow_io.read_png(paths[1]), flow_viz.flow_to_image(fields[1].contiguous(), rad_max=2.0))
