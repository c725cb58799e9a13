"""Tiled inference on the GPU: the sf_tile_blend kernel against a CPU restatement of the reference's F.pad accumulation
(evaluate_mf.py:1021-1035), SKFlow_MF8.forward_tiled against per-crop forwards and against the CPU oracle chain, and the tiled
KITTI validators (validate_kitti_mf_tile against the reference's own scores in tests/golden/tile_kitti.npz; both validators with
the HIP model against the oracle model)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import tile_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def ref_blend(flows, weights, plan, n_clips):
    """The reference's loop on the CPU: per crop of the sequence, acc += F.pad(f * w), count += F.pad(w); then acc / count and
    the unpad.  flows [n_clips * n_distinct, P, 2, th, tw] -> [n_clips, P, 2, h, w]."""
    H, W = plan.image_hw
    th, tw = plan.tile_hw
    y0, x0, h, w = plan.crop
    out = []
    for b in range(n_clips):
        acc, count = 0, 0
        for (y, x), d in zip(plan.sequence, plan.index):
            padding = (x, W - x - tw, y, H - y - th)
            acc = acc + F.pad(flows[b * plan.n_distinct + d] * weights, padding)
            count += F.pad(weights, padding)
        out.append((acc / count)[..., y0:y0 + h, x0:x0 + w])
    return torch.stack(out)


# (canvas H, W, tile h, w, min_overlap, pad [left, right, top, bottom], clips, pairs)
BLEND_CASES = [(432, 1242, 432, 960, 20, (0, 0, 0, 57), 2, 3),       # validate_kitti_mf_tile, 375 x 1242 frames
               (432, 1224, 432, 960, 20, (0, 0, 0, 62), 1, 2),
               (376, 1242, 376, 720, 20, (0, 0, 0, 1), 2, 1),        # validate_kitti_tile
               (75, 203, 24, 40, 5, (1, 2, 3, 4), 2, 3),              # small odd shape, 16 crops, an inner output window
               (64, 176, 64, 96, 20, (0, 0, 0, 0), 1, 3)]


@pytest.mark.parametrize("case", BLEND_CASES, ids=lambda c: "x".join(map(str, c[:4])))
def test_tile_blend_bitwise_vs_reference_loop(dev, case):
    """Bitwise equal to the reference's fp32 arithmetic, the image corners included (covered by one crop each, weight ~3e-43:
    out = fl(fl(f * w) / w) there, which FMA contraction or subnormal flushing would change or turn into 0 / 0)."""
    from streamflow_amd import ops, tiling
    H, W, th, tw, mo, pad, B, P = case
    plan = tiling.make_plan((H, W), (th, tw), mo, pad=pad)
    g = torch.Generator().manual_seed(H * W + th)
    flows = torch.randn(B * plan.n_distinct, P, 2, th, tw, generator=g) * 10.0
    wts = tiling.tile_weights((th, tw), tiling.TILE_SIGMA)
    ref = ref_blend(flows, wts, plan, B)
    got = ops.tile_blend(flows.to(dev), tiling.tile_weights((th, tw), tiling.TILE_SIGMA, dev), plan, n_clips=B).cpu()
    assert got.shape == ref.shape == (B, P, 2, plan.crop[2], plan.crop[3])
    corners = (..., [0, 0, -1, -1], [0, -1, 0, -1])
    assert torch.isfinite(got[corners]).all(), got[corners]
    assert torch.equal(got[corners], ref[corners]), (got[corners] - ref[corners]).abs().max()
    diff = (got != ref).sum().item()
    assert diff == 0, (case, diff, (got - ref).abs().max().item())


def test_tile_blend_checks_its_arguments(dev):
    from streamflow_amd import ops, tiling
    plan = tiling.make_plan((64, 176), (64, 96), 20)
    wts = tiling.tile_weights((64, 96), 0.05, dev)
    with pytest.raises(RuntimeError, match="do not match"):
        ops.tile_blend(torch.zeros(plan.n_distinct + 1, 1, 2, 64, 96, device=dev), wts, plan)
    with pytest.raises(RuntimeError, match="weights"):
        ops.tile_blend(torch.zeros(plan.n_distinct, 1, 2, 64, 96, device=dev), wts[:32].contiguous(), plan)


def _model(dev, T, preset, use_graph=False):
    from tests.test_gpu_evaluate import _OracleModel
    from streamflow_amd import synthetic as syn
    from streamflow_amd.model import SKFlow_MF8, default_args
    hot, ef, ec = syn.make_params(31, T), syn.make_twins_params(32), syn.make_twins_params(33)
    sd = dict(hot)
    sd.update({"fnet." + k: v for k, v in ef.items()})
    sd.update({"cnet." + k: v for k, v in ec.items()})
    model = SKFlow_MF8(default_args(T=T, preset=preset, use_graph=use_graph)).to(dev)
    model.load_state_dict(sd, strict=True)
    return model, _OracleModel(hot, ef, ec, T)


def _frames(seed, B, T, H, W):
    from tests.test_gpu_evaluate import _smooth_frames
    rng = np.random.default_rng(seed)
    clips = [_smooth_frames(rng, T, H, W) for _ in range(B)]
    return [torch.stack([torch.from_numpy(c[t]).permute(2, 0, 1).float() for c in clips]) for t in range(T)]


@pytest.mark.parametrize("preset,use_graph", [("fp32_class", False), ("config2_mixed", True)])
def test_forward_tiled_equals_per_crop_forwards(dev, preset, use_graph):
    """One batch of B * n_distinct crops through the encoders and the engine + one blend, against the reference's way: one
    forward per crop of every clip, then the same blend.  The model is NOT batch-invariant: a batch of six crops and six
    single-crop runs differ by up to 4.6e-5 px (fp32_class) and 1.1e-2 px (config2_mixed, whose fp16 activations magnify any
    change of summation order) at single pixels on MI355X.  So the bound is on the EPE: 1e-5 px in the fp32 class; in the
    config-2 class the relative bound of tests/test_gpu_parity.py, 1e-3 of the mean flow magnitude.  Observed values print."""
    from oracle import streamflow_oracle as orc
    from streamflow_amd import ops, tiling
    B, T, H, W, tile, mo, iters = 2, 3, 128, 240, (128, 128), 20, 3
    model, _ = _model(dev, T, preset, use_graph)
    images = [x.to(dev) for x in _frames(7, B, T, H, W)]
    got = model.forward_tiled(images, iters=iters, tile=tile, min_overlap=mo)
    assert len(got) == T - 1 and all(tuple(g.shape) == (B, 2, H, W) for g in got)
    got = torch.stack(got, dim=1)
    plan = tiling.make_plan((H, W), tile, mo)
    per = []
    for b in range(B):
        for (y, x) in plan.distinct:
            flows = model([im[b:b + 1, :, y:y + tile[0], x:x + tile[1]] for im in images], iters=iters, test_mode=True)
            per.append(torch.cat(flows, dim=0))
    ref = ops.tile_blend(torch.stack(per).contiguous(), tiling.tile_weights(tile, 0.05, dev), plan, n_clips=B)
    assert torch.isfinite(got).all()
    got, ref = got.cpu(), ref.cpu()
    epe = max(orc.epe(got[:, i], ref[:, i]) for i in range(T - 1))
    mag = float(ref.norm(dim=2).mean())
    print(f"forward_tiled [{preset}] vs per-crop forwards: EPE {epe:.3e} px, max |diff| {(got - ref).abs().max().item():.3e} px, "
          f"mean |flow| {mag:.2f} px, bitwise equal: {torch.equal(got, ref)}")
    bound = 1e-5 if preset == "fp32_class" else 1e-3 * max(1.0, mag)
    assert epe <= bound, (preset, epe, mag)


@pytest.mark.parametrize("preset", ["fp32_class", "config2_mixed"])
def test_forward_tiled_vs_oracle(dev, preset):
    """forward_tiled against the CPU oracle chain (frames -> Twins_CSC -> hot path per distinct crop, reference blend loop) on a
    128 x 240 frame with six crop entries (three distinct; the engine needs crops of >= 128 px per side).  The project's contract: EPE <= 1e-3 px in the fp32 class, <= 1e-3 of the
    mean flow magnitude in the config-2 presets (tests/test_gpu_parity.py)."""
    from oracle import streamflow_oracle as orc
    from streamflow_amd import tiling
    B, T, H, W, tile, mo, iters = 1, 3, 128, 240, (128, 128), 20, 3
    model, oracle = _model(dev, T, preset)
    images = _frames(8, B, T, H, W)
    got = model.forward_tiled([x.to(dev) for x in images], iters=iters, tile=tile, min_overlap=mo)
    plan = tiling.make_plan((H, W), tile, mo)
    crops = [torch.cat(oracle([im[:, :, y:y + tile[0], x:x + tile[1]] for im in images], iters=iters), dim=0)
             for (y, x) in plan.distinct]
    ref = ref_blend(torch.stack(crops), tiling.tile_weights(tile, 0.05), plan, 1)[0]
    worst = max(orc.epe(g.cpu(), ref[i][None]) for i, g in enumerate(got))
    mag = float(ref.norm(dim=1).mean())
    print(f"forward_tiled [{preset}] vs oracle: EPE {worst:.3e} px, mean |flow| {mag:.2f} px")
    bound = 1e-3 if preset == "fp32_class" else 1e-3 * max(1.0, mag)
    assert worst <= bound, (preset, worst, mag)


def test_validate_kitti_mf_tile_stub_matches_reference(tmp_path, dev, golden):
    """The tiled multi-frame validator over the golden's synthetic tree (375 x 1242 and 370 x 1224: the grid is rebuilt for the
    second width) with the stub model on the GPU and the HIP blend: the reference's own kitti_epe / kitti_f1."""
    from streamflow_amd import evaluate
    gold = golden("tile_kitti")
    tc.write_kitti_mf_tree(str(tmp_path))
    res = evaluate.validate_kitti_mf_tile(tc.StubModel(), iters=tc.ITERS, multi_root=str(tmp_path), nframes=tc.NFRAMES, device=dev)
    assert set(res) == {"kitti_epe", "kitti_f1"}
    assert res["kitti_epe"] == pytest.approx(float(gold["kitti_epe"]), rel=1e-6, abs=0)
    assert res["kitti_f1"] == pytest.approx(float(gold["kitti_f1"]), rel=1e-6, abs=0)


class _Oracle12:
    """The oracle chain with the model's default of 12 iterations (validate_kitti_tile calls the model without iters)."""

    def __init__(self, oracle):
        self.oracle = oracle

    def __call__(self, images, iters=12, test_mode=True):
        return self.oracle(images, iters=iters, test_mode=test_mode)


def _kitti_tree(root, seqs, T, shapes, seed, two_frame=False):
    from streamflow_amd import flow_io
    from tests.test_gpu_evaluate import _smooth_frames
    rng = np.random.default_rng(seed)
    (root / "training" / "image_2").mkdir(parents=True)
    (root / "training" / "flow_occ").mkdir(parents=True)
    for s in range(seqs):
        H, W = shapes[s]
        ids = (10, 11) if two_frame else range(12 - T, 12)
        for i, img in zip(ids, _smooth_frames(rng, len(ids), H, W)):
            flow_io.write_png(str(root / "training" / "image_2" / ("%06d_%02d.png" % (s, i))), img)
        enc = flow_io.kitti_encode(rng.normal(0, 6, size=(H, W, 2)).astype(np.float32))
        enc[..., 2] = rng.random((H, W)) < 0.4
        flow_io.write_png(str(root / "training" / "flow_occ" / ("%06d_10.png" % s)), enc)


def test_validate_kitti_mf_tile_hip_vs_oracle(tmp_path, dev):
    from streamflow_amd import evaluate
    T, iters = 3, 2
    _kitti_tree(tmp_path, 2, T, [(370, 1000), (372, 984)], 11)
    model, oracle = _model(dev, T, "fp32_class")
    got = evaluate.validate_kitti_mf_tile(model, iters=iters, multi_root=str(tmp_path), nframes=T, device=dev)
    ref = evaluate.validate_kitti_mf_tile(oracle, iters=iters, multi_root=str(tmp_path), nframes=T, device=dev)
    assert set(got) == {"kitti_epe", "kitti_f1"}
    assert abs(got["kitti_epe"] - ref["kitti_epe"]) <= 1e-3, (got, ref)
    assert abs(got["kitti_f1"] - ref["kitti_f1"]) <= 0.05, (got, ref)


def test_validate_kitti_tile_hip_vs_oracle(tmp_path, dev):
    """Two-frame layout (image_2/*_10.png, *_11.png), T = 2 model called without iters (12), 376 x 720 crops, hyphenated keys."""
    from streamflow_amd import evaluate
    _kitti_tree(tmp_path, 1, 2, [(370, 736)], 12, two_frame=True)
    model, oracle = _model(dev, 2, "fp32_class")
    got = evaluate.validate_kitti_tile(model, iters=6, root=str(tmp_path), device=dev)
    ref = evaluate.validate_kitti_tile(_Oracle12(oracle), iters=6, root=str(tmp_path), device=dev)
    assert set(got) == {"kitti-epe", "kitti-f1"}
    assert abs(got["kitti-epe"] - ref["kitti-epe"]) <= 1e-3, (got, ref)
    assert abs(got["kitti-f1"] - ref["kitti-f1"]) <= 0.05, (got, ref)


def test_forward_tiled_full_kitti_clip(dev):
    """One 375 x 1242 clip, T = 4, the headline preset: padded to 432 rows, two distinct 432 x 960 crops in one graph."""
    from streamflow_amd import presets
    from streamflow_amd.tiling import FixedHeightPadder
    T = 4
    model, _ = _model(dev, T, presets.BENCH_PRESET, use_graph=True)
    images = [x.to(dev) for x in _frames(9, 1, T, 375, 1242)]
    padder = FixedHeightPadder(images[0].shape, 432)
    flows = model.forward_tiled(padder.pad_list(images), iters=4)
    assert len(flows) == T - 1
    for f in flows:
        f = padder.unpad(f)
        assert tuple(f.shape) == (1, 2, 375, 1242)
        assert torch.isfinite(f).all()
