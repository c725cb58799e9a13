"""Batched validation on the GPU (streamflow_amd/evaluate.py, clips_per_step > 1): sintel_report / validate_sintel_occ_mf through
video.predict_video and the sf_flow_score_batch kernel, validate_kitti_mf through ops.frames_to_clips and the same kernel, and the
command line -- with a stub model whose flows are a fixed function of the frames (the reports must equal the host twin applied to
predict_video's flows, exactly) and with the HIP model on seeded synthetic weights (against today's one-clip-per-call loops)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import video_cases as vc
from tests.test_gpu_evaluate import _models, _smooth_frames

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class _Stub:
    """vc.stub_model behind both call conventions: the reference's test-mode call (a list of [1, 3, H, W] frames in 0 .. 255,
    normalised with the model's own expression) and predict_video's (a normalised clip batch)."""
    def __call__(self, images, iters=None, test_mode=False):
        if isinstance(images, (list, tuple)):
            images = vc.normalise(torch.stack(list(images), dim=1))
        return vc.stub_model(images)


@pytest.fixture(scope="module")
def stub_tree(tmp_path_factory):
    from streamflow_amd import flow_io
    root = tmp_path_factory.mktemp("sintel_stub")
    rng = np.random.default_rng(11)
    H, W = 44, 60
    for s, (scene, n) in enumerate((("alley_1", 5), ("market_2", 9))):
        frames = vc.random_frames(20 + s, n, H, W).numpy()
        for dstype in ("albedo", "clean", "final"):
            os.makedirs(root / "training" / dstype / scene)
            for i in range(n):
                flow_io.write_png(str(root / "training" / dstype / scene / f"frame_{i + 1:04d}.png"), frames[i])
        os.makedirs(root / "training" / "flow" / scene)
        os.makedirs(root / "training" / "occlusions" / scene)
        for i in range(n - 1):
            flow_io.write_flo(str(root / "training" / "flow" / scene / f"frame_{i + 1:04d}.flo"),
                              rng.normal(0, 2, size=(H, W, 2)).astype(np.float32))
            occ = np.where(rng.random((H, W)) < 0.3, 255, rng.integers(0, 255, size=(H, W))).astype(np.uint8)
            flow_io.write_png(str(root / "training" / "occlusions" / scene / f"frame_{i + 1:04d}.png"), occ)
    return root


@pytest.fixture(scope="module")
def stub_rows(stub_tree, dev):
    """The host twin on predict_video's flows of every scene: rows [12 pairs, EVAL_LEN] with and without the occlusion maps."""
    from streamflow_amd import flow_io, scoring, video
    rows = {False: [], True: []}
    for scene in ("alley_1", "market_2"):
        d = stub_tree / "training" / "clean" / scene
        flows = video.predict_video(_Stub(), video.FrameDir(str(d)), T=4, clips_per_step=8, device=dev).cpu().numpy()
        for i in range(flows.shape[0]):
            gt = flow_io.read_flo(str(stub_tree / "training" / "flow" / scene / f"frame_{i + 1:04d}.flo"))
            occ = flow_io.read_png(str(stub_tree / "training" / "occlusions" / scene / f"frame_{i + 1:04d}.png"))
            for with_occ in (False, True):
                row = np.zeros(scoring.EVAL_LEN)
                scoring.score_host_fields(flows[i], gt, row, "flo", occ if with_occ else None)
                rows[with_occ].append(row)
    return {k: np.stack(v) for k, v in rows.items()}


@pytest.mark.parametrize("clips_per_step", [1, 3, 8])
@pytest.mark.parametrize("occ", [False, True])
def test_sintel_report_batched_vs_host_twin(stub_tree, stub_rows, dev, clips_per_step, occ, capsys):
    from streamflow_amd import evaluate, scoring
    want = scoring.sintel_from(stub_rows[occ])
    assert want["pairs"] == 4 + 8 and 0.05 < want["1px"] < want["3px"] < want["5px"] and want["3px"] < 0.95
    rep = evaluate.sintel_report(_Stub(), iters=3, root=str(stub_tree), nframes=4, dstypes=("clean", "final"), device=dev,
                                 clips_per_step=clips_per_step, occ=occ)
    out = capsys.readouterr().out
    assert set(rep) == {"clean", "final"} and "Validation (final) EPE:" in out and ("Occ epe:" in out) == occ
    for got in rep.values():
        assert got["pairs"] == 4 + 8
        if clips_per_step == 1 and not occ:                            # today's host loop: float32 means of concatenated arrays
            assert abs(got["epe"] - want["epe"]) < 1e-5 and abs(got["3px"] - want["3px"]) < 1e-9
            continue
        assert got["pixels"] == want["pixels"] == 12 * 44 * 60
        for k in ("epe", "1px", "3px", "5px") + (("epe_occ", "epe_noc") if occ else ()):
            assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
        if occ:
            assert got["occ_pixels"] == want["occ_pixels"] > 0
        else:
            assert "epe_occ" not in got
    if occ:
        res = evaluate.validate_sintel_occ_mf(_Stub(), iters=3, root=str(stub_tree), nframes=4, clips_per_step=clips_per_step, device=dev)
        assert set(res) == {"albedo", "clean", "final"} and all(abs(v - want["epe"]) <= 1e-12 for v in res.values())


@pytest.fixture(scope="module")
def hip_model(dev):
    return _models(dev, 3, "fp32_class")[0]


def _sintel_tree(root, rng, H, W):
    from streamflow_amd import flow_io
    for scene, n in (("ambush_9", 5), ("cave_9", 4)):
        for dstype in ("clean", "final"):
            os.makedirs(root / "training" / dstype / scene)
            for i, img in enumerate(_smooth_frames(rng, n, H, W)):
                flow_io.write_png(str(root / "training" / dstype / scene / f"frame_{i + 1:04d}.png"), img)
        os.makedirs(root / "training" / "flow" / scene)
        for i in range(n - 1):
            flow_io.write_flo(str(root / "training" / "flow" / scene / f"frame_{i + 1:04d}.flo"),
                              rng.normal(0, 3, size=(H, W, 2)).astype(np.float32))


def test_sintel_hip_model_batched_vs_per_clip_and_command_line(tmp_path, dev, hip_model):
    """124 x 188, T = 3, iters = 3, scenes of 5 and 4 frames (the second needs the end-aligned tail clip): four clips per call
    against today's loop, within the bounds test_gpu_evaluate.py holds that loop to; then the command line on the same tree with
    the same weights in a checkpoint file prints the function's numbers."""
    from streamflow_amd import evaluate
    H, W, T, iters = 124, 188, 3, 3
    _sintel_tree(tmp_path, np.random.default_rng(3), H, W)
    ref = evaluate.sintel_report(hip_model, iters=iters, root=str(tmp_path), nframes=T, device=dev)
    got = evaluate.sintel_report(hip_model, iters=iters, root=str(tmp_path), nframes=T, device=dev, clips_per_step=4)
    for k in ("clean", "final"):
        print(k, got[k], ref[k])
        assert got[k]["pairs"] == ref[k]["pairs"] == 4 + 3
        assert abs(got[k]["epe"] - ref[k]["epe"]) <= 1e-3, (k, got[k], ref[k])
        for r in ("1px", "3px", "5px"):
            assert abs(got[k][r] - ref[k][r]) <= 5e-3, (k, r, got[k], ref[k])
    res = evaluate.validate_sintel_mf(hip_model, iters=iters, root=str(tmp_path), nframes=T, device=dev, clips_per_step=4)
    assert res == {k: got[k]["epe"] for k in got}
    ckpt = str(tmp_path / "ckpt.pth")
    torch.save({"model": {"module." + k: v.cpu() for k, v in hip_model.state_dict().items()}}, ckpt)
    cmd = [sys.executable, "-m", "streamflow_amd.evaluate", "--dataset", "sintel", "--ckpt", ckpt, "--root", str(tmp_path),
           "--T", str(T), "--iters", str(iters), "--clips-per-step", "4", "--preset", "fp32_class"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for k in ("clean", "final"):
        line = "Validation (%s) EPE: %f, 1px: %f, 3px: %f, 5px: %f" % (k, got[k]["epe"], got[k]["1px"], got[k]["3px"], got[k]["5px"])
        assert line in r.stdout, (line, r.stdout[-2000:])
    assert "clean: %f final: %f" % (res["clean"], res["final"]) in r.stdout


def test_kitti_hip_model_batched_vs_per_clip(tmp_path, dev, hip_model):
    """Four sequences, two of 122 x 180 and two of 122 x 172 (a size change flushes the batch), T = 3, eight clips per call against
    today's loop, within the bounds of test_gpu_evaluate.py."""
    from streamflow_amd import evaluate, flow_io
    rng = np.random.default_rng(4)
    H, T, iters = 122, 3, 3
    os.makedirs(tmp_path / "training" / "image_2")
    os.makedirs(tmp_path / "training" / "flow_occ")
    for s, W in enumerate((180, 180, 172, 172)):
        for i, img in zip(range(12 - T, 12), _smooth_frames(rng, T, H, W)):
            flow_io.write_png(str(tmp_path / "training" / "image_2" / ("%06d_%02d.png" % (s, i))), img)
        enc = flow_io.kitti_encode(rng.normal(0, 6, size=(H, W, 2)).astype(np.float32))
        enc[..., 2] = rng.random((H, W)) < 0.4
        flow_io.write_png(str(tmp_path / "training" / "flow_occ" / ("%06d_10.png" % s)), enc)
    ref = evaluate.validate_kitti_mf(hip_model, iters=iters, multi_root=str(tmp_path), nframes=T, device=dev)
    got = evaluate.validate_kitti_mf(hip_model, iters=iters, multi_root=str(tmp_path), nframes=T, device=dev, clips_per_step=8)
    print(got, ref)
    assert set(got) == {"kitti_epe", "kitti_f1"}
    assert abs(got["kitti_epe"] - ref["kitti_epe"]) <= 1e-3, (got, ref)
    assert abs(got["kitti_f1"] - ref["kitti_f1"]) <= 0.05, (got, ref)
    two = evaluate.validate_kitti_mf(hip_model, iters=iters, multi_root=str(tmp_path), nframes=T, device=dev, clips_per_step=2)
    assert abs(two["kitti_epe"] - got["kitti_epe"]) <= 1e-3 and abs(two["kitti_f1"] - got["kitti_f1"]) <= 0.05
