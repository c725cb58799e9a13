"""Spring validation on the GPU (streamflow_amd.evaluate.spring_report, the reference's evaluate_mf.py:50-102): a synthetic Spring
tree (two scenes of 5 and 4 textured 124 x 188 frames, padded to 128 x 192, T = 3 so that tail clips occur; ground truth at
2H x 2W with decoys off the subsampling grid and 10 % NaN pixels) scored with the HIP model -- flows on the device, scored there by
sf_flow_score -- and with the CPU oracle chained the same way, scored on the host by the same loop."""
import os

import numpy as np
import pytest
import torch

from tests import score_cases as sc

pytestmark = pytest.mark.gpu

H, W, T, ITERS = 124, 188, 3, 3
SCENES = (("0041", 5), ("0007", 4))
RATES = ("1px", "3px", "5px", "spring_1px", "spring_1px_s0_10", "spring_1px_s10_40", "spring_1px_s40")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _smooth_frames(rng, n, H, W):
    """A textured image translated by a few pixels per frame (so that consecutive frames are related)."""
    base = rng.integers(0, 256, size=(H + 64, W + 64, 3)).astype(np.float32)
    for _ in range(2):                                                   # cheap blur: correlated texture
        base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (0, 1))) / 4.0
    base = (base - base.min()) / (base.max() - base.min()) * 255.0
    return [base[32 + 2 * i: 32 + 2 * i + H, 32 - 3 * i + 16: 32 - 3 * i + 16 + W].round().astype(np.uint8) for i in range(n)]


class _OracleModel:
    """The CPU oracles behind the reference's test-mode call signature."""
    def __init__(self, hot, ef, ec, T):
        self.hot, self.ef, self.ec, self.T = hot, ef, ec, T

    def __call__(self, images, iters=6, test_mode=True):
        from oracle import streamflow_oracle as orc, twins_oracle as two
        imgs = 2 * (torch.stack([i.cpu().float() for i in images], dim=1) / 255.0) - 1.0
        fmaps = two.twins_csc_forward(imgs, self.ef)
        cnets = two.twins_csc_forward(imgs[:, :-1], self.ec)
        return orc.hotpath_forward(fmaps, cnets, self.hot, iters)[0]


def _models(dev, T, preset):
    from streamflow_amd import synthetic as syn
    from streamflow_amd.model import SKFlow_MF8, default_args
    hot, ef, ec = syn.make_params(31, T), syn.make_twins_params(32), syn.make_twins_params(33)
    sd = dict(hot)
    sd.update({"fnet." + k: v for k, v in ef.items()})
    sd.update({"cnet." + k: v for k, v in ec.items()})
    model = SKFlow_MF8(default_args(T=T, preset=preset)).to(dev)
    model.load_state_dict(sd, strict=True)
    return model, _OracleModel(hot, ef, ec, T)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    from streamflow_amd import flo5, flow_io
    root = tmp_path_factory.mktemp("spring")
    rng = np.random.default_rng(8)
    for scene, n in SCENES:
        for cam in ("left", "right"):
            d = root / "train" / scene / f"frame_{cam}"
            os.makedirs(d)
            for i, img in enumerate(_smooth_frames(rng, n, H, W)):
                flow_io.write_png(str(d / f"frame_{cam}_{i + 1:04d}.png"), img)
            for direction in ("FW", "BW"):
                os.makedirs(root / "train" / scene / f"flow_{direction}_{cam}")
                for a in (range(n - 1) if direction == "FW" else range(1, n)):
                    flo5.write_flo5(str(root / "train" / scene / f"flow_{direction}_{cam}" / f"flow_{direction}_{cam}_{a + 1:04d}.flo5"),
                                    sc.random_gt(rng, H, W, 2, 0.1))
    return str(root)


class _Spy:
    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *a, **kw):
        self.calls += 1
        return self.fn(*a, **kw)


@pytest.fixture(scope="module")
def oracle_report(tree, dev):
    """The oracle's report (host flows), and how often ops.flow_score ran meanwhile."""
    from streamflow_amd import evaluate, ops
    _, oracle = _models(dev, T, "fp32_class")
    spy = _Spy(ops.flow_score)
    mp = pytest.MonkeyPatch()
    mp.setattr(ops, "flow_score", spy)
    try:
        rep = evaluate.spring_report(oracle, iters=ITERS, root=tree, nframes=T, device=torch.device("cpu"), scenes=None)
    finally:
        mp.undo()
    return rep, spy.calls


@pytest.mark.parametrize("preset,tol", [("fp32_class", 1e-3), ("config2_mixed", 2e-2)])
def test_spring_report_hip_vs_oracle(tree, oracle_report, dev, monkeypatch, preset, tol):
    from streamflow_amd import evaluate, ops
    spy = _Spy(ops.flow_score)
    monkeypatch.setattr(ops, "flow_score", spy)
    model, _ = _models(dev, T, preset)
    got = evaluate.spring_report(model, iters=ITERS, root=tree, nframes=T, device=dev, scenes=None)
    assert spy.calls == got["pairs"] == 2 * 2 * (4 + 3)                 # the kernel scored every pair, once
    ref, oracle_calls = oracle_report
    assert oracle_calls == 0                                            # host flows never reach the kernel
    assert ref["pairs"] == got["pairs"] and ref["pixels"] == got["pixels"] and ref["valid_pixels"] == got["valid_pixels"]
    assert np.isnan(got["epe"]) and np.isnan(ref["epe"])
    print(preset, got, ref)
    assert abs(got["epe_valid"] - ref["epe_valid"]) <= tol, (preset, got, ref)
    for r in RATES:
        assert abs(got[r] - ref[r]) <= 5e-3, (preset, r, got, ref)


def test_host_path_equals_kernel_on_identical_flows(tree, dev, monkeypatch):
    """The HIP model's flows scored on the device, then the same model's flows returned as host tensors (the host path): the
    same counts, the means within 1e-8 relative (score_cases.assert_acc_matches gives the bound)."""
    from streamflow_amd import evaluate, ops, scoring
    model, _ = _models(dev, T, "fp32_class")
    spy = _Spy(ops.flow_score)
    monkeypatch.setattr(ops, "flow_score", spy)
    accs, report = [], scoring.report
    monkeypatch.setattr(scoring, "report", lambda acc: (accs.append(np.array(acc, np.float64)), report(acc))[1])
    kern = evaluate.spring_report(model, iters=ITERS, root=tree, nframes=T, device=dev, scenes=None)
    n = spy.calls

    def host_model(images, iters=6, test_mode=True):
        return [f.cpu() for f in model(images, iters=iters, test_mode=test_mode)]

    host = evaluate.spring_report(host_model, iters=ITERS, root=tree, nframes=T, device=dev, scenes=None)
    assert n == kern["pairs"] == 28 and spy.calls == n
    print(kern, host)
    assert len(accs) == 2
    want = {k: float(accs[0][i]) for k, i in sc.ENTRY.items()}
    sc.assert_acc_matches(accs[1], want, "host path vs kernel")
    assert host["pairs"] == kern["pairs"] and host["pixels"] == kern["pixels"] and host["valid_pixels"] == kern["valid_pixels"]
    for r in RATES:                                                     # equal rates over equal denominators: equal counts
        assert sc.close(host[r], kern[r], 0.0), (r, host[r], kern[r])
    for k in ("epe", "epe_valid"):
        assert sc.close(host[k], kern[k], 1e-8), (k, host[k], kern[k])
