"""CPU: the host-side plan of tiled inference (streamflow_amd/tiling.py) against the reference's own helpers, recorded in
tests/golden/tile_kitti.npz by tests/golden/make_tile_golden.py (compute_grid_indices, compute_weight, InputPadder2)."""
import numpy as np
import pytest
import torch

from tests import tile_cases as tc


@pytest.fixture(scope="module")
def gold(golden):
    return golden("tile_kitti")


@pytest.mark.parametrize("i", range(len(tc.GRID_CASES)))
def test_tile_grid_matches_reference(gold, i):
    from streamflow_amd import tiling
    H, W, th, tw, mo = tc.GRID_CASES[i]
    got = tiling.tile_grid((H, W), (th, tw), mo)
    assert got == [tuple(int(v) for v in r) for r in gold[f"grid{i}"]]           # duplicates and order included


def test_kitti_grids_repeat_every_crop(gold):
    """At every KITTI shape the reference lists each crop twice (the 'kitti432' example of 432 x 1242: (0,0),(0,282),(0,0),(0,282))."""
    from streamflow_amd import tiling
    assert tiling.tile_grid((432, 1242), (432, 960)) == [(0, 0), (0, 282), (0, 0), (0, 282)]
    for i, (H, W, th, tw, mo) in enumerate(tc.GRID_CASES[:10] + tc.GRID_CASES[-1:]):
        plan = tiling.make_plan((H, W), (th, tw), mo)
        assert len(plan.sequence) == 2 * plan.n_distinct, (H, W)


@pytest.mark.parametrize("i", range(len(tc.GRID_CASES)))
def test_plan_dedup_map(gold, i):
    from streamflow_amd import tiling
    H, W, th, tw, mo = tc.GRID_CASES[i]
    seq = [tuple(int(v) for v in r) for r in gold[f"grid{i}"]]
    if any(y + th > H or x + tw > W for (y, x) in seq):
        with pytest.raises(ValueError, match="leaves the image"):
            tiling.make_plan((H, W), (th, tw), mo)
        return
    plan = tiling.make_plan((H, W), (th, tw), mo)
    assert list(plan.sequence) == seq
    assert len(set(plan.distinct)) == len(plan.distinct) == len(set(seq))
    assert [plan.distinct[d] for d in plan.index] == seq                          # every entry maps to its own crop
    assert plan.crop == (0, 0, H, W)
    x = torch.arange(H * W, dtype=torch.float32).view(1, 1, H, W)
    for (y0, x0), c in zip(plan.distinct, plan.crops(x)):
        assert c.shape[-2:] == (th, tw) and torch.equal(c, x[..., y0:y0 + th, x0:x0 + tw])


@pytest.mark.parametrize("i", range(len(tc.WEIGHT_FULL)))
def test_tile_weights_bitwise_full(gold, i):
    from streamflow_amd import tiling
    th, tw, sigma = tc.WEIGHT_FULL[i]
    w = tiling.tile_weights((th, tw), sigma)
    assert w.dtype == torch.float32 and tuple(w.shape) == (th, tw)
    assert np.array_equal(w.numpy(), gold[f"wfull{i}"])


@pytest.mark.parametrize("i", range(len(tc.WEIGHT_SAMPLED)))
def test_tile_weights_bitwise_kitti_corners(gold, i):
    from streamflow_amd import tiling
    th, tw, sigma = tc.WEIGHT_SAMPLED[i]
    w = tiling.tile_weights((th, tw), sigma).numpy()
    ys, xs = tc.sampled_pixels(th, tw)
    ref = gold[f"wsamp{i}"]
    assert np.array_equal(w[ys, xs], ref)
    corners = ref[:4]
    assert (corners > 0).all() and (corners < np.finfo(np.float32).tiny).all()    # subnormal, not flushed
    assert abs(float(corners[0]) - 3.01e-43) < 0.01e-43 if (th, tw) == (432, 960) else True


def test_tile_weights_cached():
    from streamflow_amd import tiling
    assert tiling.tile_weights((48, 64), 0.05) is tiling.tile_weights((48, 64), 0.05)


@pytest.mark.parametrize("i", range(len(tc.PAD_CASES)))
def test_fixed_height_padder(gold, i):
    from streamflow_amd.tiling import FixedHeightPadder
    mode, h, w = tc.PAD_CASES[i]
    height = int(mode[len("kitti"):])
    p = FixedHeightPadder((1, 3, h, w), height, mode="replicate" if mode == "kitti432" else "zeros")
    assert p._pad == [int(v) for v in gold[f"pad{i}"]]
    x = torch.rand(1, 3, h, w) + 1.0
    (z,) = p.pad(x)
    (r,) = p.pad_list([x])
    assert z.shape[-2:] == r.shape[-2:] == (height, w)
    assert torch.equal(p.unpad(z), x) and torch.equal(p.unpad(r), x)
    assert (z[..., h:, :] == 0).all() and torch.equal(r[..., h:, :], x[..., h - 1:h, :].expand(1, 3, height - h, w))
    assert torch.equal(p.apply([x])[0], r if p.mode == "replicate" else z)


def test_error_cases():
    from streamflow_amd import tiling
    with pytest.raises(ValueError):
        tiling.tile_grid((432, 1242), (432, 960), min_overlap=432)
    with pytest.raises(ValueError):
        tiling.tile_grid((432, 1242), (432, 960), min_overlap=960)
    with pytest.raises(ValueError):
        tiling.tile_grid((375, 1242), (432, 960))                                  # the reference would give negative origins
    with pytest.raises(ValueError):
        tiling.tile_grid((432, 900), (432, 960))
    with pytest.raises(ValueError):
        tiling.FixedHeightPadder((1, 3, 433, 1242), 432)
    with pytest.raises(ValueError):
        tiling.FixedHeightPadder((1, 3, 375, 1242), 432, mode="reflect")
    with pytest.raises(ValueError):
        tiling.make_plan((64, 96), (48, 64), pad=(0, 0, 0, 64))
    with pytest.raises(ValueError):
        tiling.make_plan((2000, 2000), (48, 64))                                   # more crops than the kernel's plan holds


def test_plan_output_crop():
    from streamflow_amd import tiling
    plan = tiling.make_plan((432, 1242), (432, 960), pad=[0, 0, 0, 57])
    assert plan.crop == (0, 0, 375, 1242) and plan.distinct == ((0, 0), (0, 282)) and plan.index == (0, 1, 0, 1)


def test_tile_blend_needs_gpu_tensors():
    from streamflow_amd import ops, tiling
    plan = tiling.make_plan((96, 160), (64, 96), 16)
    flows = torch.zeros(plan.n_distinct, 1, 2, 64, 96)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tile_blend(flows, tiling.tile_weights((64, 96), 0.05), plan)


def test_forward_tiled_rejects_warm_start():
    from streamflow_amd.model import SKFlow_MF8, default_args
    model = SKFlow_MF8(default_args(T=2, Encoder="Twins_CSC"))
    imgs = [torch.zeros(1, 3, 64, 96)] * 2
    with pytest.raises(NotImplementedError):
        model.forward_tiled(imgs, tile=(48, 64), flow_init=[torch.zeros(1, 2, 8, 12)])
