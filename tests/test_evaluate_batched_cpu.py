"""The Sintel occlusion validator and the `clips_per_step` keyword of streamflow_amd/evaluate.py on the CPU: validate_sintel_occ_mf
over a synthetic tree with the stand-in model of tests/test_evaluate_cpu.py (its error per pair is known in closed form), the
refusal of batched validation without a GPU, the command line's parser, and the new entry point's place in the ABI tables."""
import os
import re

import numpy as np
import pytest
import torch

from streamflow_amd import evaluate, flow_io
from tests.test_evaluate_cpu import _noise, _tag_frame

H, W, T = 44, 60, 4                                                      # not multiples of 8: the padder is exercised
LENGTHS = {"alley_1": 5, "market_2": 9}
PASSES = ("albedo", "clean", "final")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """Sintel layout with three passes, ground truth and occlusion maps (about 30 % occluded; the map of pair (1, 2) all clear)."""
    root = tmp_path_factory.mktemp("sintel_occ")
    rng = np.random.default_rng(0)
    gts, occs = {}, {}
    for s, (scene, n) in enumerate(LENGTHS.items()):
        for dstype in PASSES:
            os.makedirs(root / "training" / dstype / scene)
            for i in range(n):
                flow_io.write_png(str(root / "training" / dstype / scene / f"frame_{i + 1:04d}.png"), _tag_frame(rng, H, W, s, i))
        os.makedirs(root / "training" / "flow" / scene)
        os.makedirs(root / "training" / "occlusions" / scene)
        for i in range(n - 1):
            gts[(s, i)] = rng.normal(0.0, 5.0, size=(H, W, 2)).astype(np.float32)
            flow_io.write_flo(str(root / "training" / "flow" / scene / f"frame_{i + 1:04d}.flo"), gts[(s, i)])
            occ = np.where(rng.random((H, W)) < 0.3, 255, 0).astype(np.uint8)
            if (s, i) == (1, 2):
                occ[:] = 0
            occs[(s, i)] = occ
            flow_io.write_png(str(root / "training" / "occlusions" / scene / f"frame_{i + 1:04d}.png"), occ)
    return root, gts, occs


def _stub(gts):
    def model(images, iters=0, test_mode=False):
        assert test_mode and len(images) == T and all(im.shape == (1, 3, 48, 64) for im in images)
        pad_t, pad_l = (48 - H) // 2, (64 - W) // 2                      # 'sintel' padding: split on both sides
        flows = []
        for im in images[:-1]:
            s, i = int(im[0, 0, pad_t, pad_l]), int(im[0, 1, pad_t, pad_l])
            f = torch.zeros(1, 2, 48, 64)
            f[0, :, pad_t:pad_t + H, pad_l:pad_l + W] = torch.from_numpy(gts[(s, i)]).permute(2, 0, 1) + torch.from_numpy(_noise(s, i, H, W))
            flows.append(f)
        return flows
    return model


def test_validate_sintel_occ_mf_on_a_synthetic_tree(tree, capsys):
    root, gts, occs = tree
    model = _stub(gts)
    pairs = [(s, i) for s, n in enumerate(LENGTHS.values()) for i in range(n - 1)]
    want = np.concatenate([np.sqrt((_noise(s, i, H, W) ** 2).sum(0)).reshape(-1) for s, i in pairs])
    occ = np.concatenate([occs[p].reshape(-1) == 255 for p in pairs])
    assert 0.25 < occ.mean() < 0.35 and not occs[(1, 2)].any()
    res = evaluate.validate_sintel_occ_mf(model, iters=3, root=str(root), nframes=T)
    out = capsys.readouterr().out
    assert set(res) == set(PASSES)
    for p in PASSES:
        assert abs(res[p] - want.mean()) < 1e-5
        assert "Validation (%s) EPE:" % p in out
    lines = re.findall(r"^Occ epe: ([0-9.]+), Noc epe: ([0-9.]+)$", out, flags=re.M)      # the reference's second line per pass
    assert len(lines) == 3
    for o, n in lines:
        assert abs(float(o) - want[occ].mean()) < 1e-5 and abs(float(n) - want[~occ].mean()) < 1e-5
    rep = evaluate.sintel_report(model, iters=3, root=str(root), nframes=T, dstypes=("clean",), occ=True)["clean"]
    assert rep["pairs"] == 4 + 8 and rep["pixels"] == want.size and rep["occ_pixels"] == int(occ.sum())
    assert abs(rep["epe"] - want.mean()) < 1e-5
    assert abs(rep["epe_occ"] - want[occ].mean()) < 1e-5 and abs(rep["epe_noc"] - want[~occ].mean()) < 1e-5
    for k, thr in (("1px", 1), ("3px", 3), ("5px", 5)):
        assert abs(rep[k] - (want < thr).mean()) < 1e-9
    # the scored loop and the reference-style host loop see the same pairs
    plain = evaluate.sintel_report(model, iters=3, root=str(root), nframes=T, dstypes=("clean",))["clean"]
    assert plain["pairs"] == rep["pairs"] and abs(plain["epe"] - rep["epe"]) < 1e-5 and abs(plain["3px"] - rep["3px"]) < 1e-9
    assert "epe_occ" not in plain


def test_bad_occlusion_maps_raise(tree, tmp_path):
    import shutil
    root, gts, _ = tree
    model = _stub(gts)
    bad = tmp_path / "copy"
    shutil.copytree(root, bad)
    victim = bad / "training" / "occlusions" / "alley_1" / "frame_0002.png"
    os.remove(victim)
    with pytest.raises(RuntimeError, match="occlusion"):
        evaluate.validate_sintel_occ_mf(model, iters=3, root=str(bad), nframes=T)
    flow_io.write_png(str(victim), np.zeros((H, W, 3), np.uint8))       # an RGB file where a gray one belongs
    with pytest.raises(RuntimeError, match="8-bit gray"):
        evaluate.validate_sintel_occ_mf(model, iters=3, root=str(bad), nframes=T)
    flow_io.write_png(str(victim), np.zeros((H, W), np.uint16))         # 16-bit gray
    with pytest.raises(RuntimeError, match="8-bit gray"):
        evaluate.sintel_report(model, iters=3, root=str(bad), nframes=T, dstypes=("albedo",), occ=True)


def test_batched_validation_needs_a_gpu(tree):
    root, gts, _ = tree
    model = _stub(gts)                                                   # a host model: no parameters, device cpu
    cpu = torch.device("cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        evaluate.sintel_report(model, iters=3, root=str(root), nframes=T, clips_per_step=8, device=cpu)
    with pytest.raises(RuntimeError, match="GPU"):
        evaluate.validate_sintel_mf(model, iters=3, root=str(root), nframes=T, clips_per_step=8, device=cpu)
    with pytest.raises(RuntimeError, match="GPU"):
        evaluate.validate_sintel_occ_mf(model, iters=3, root=str(root), nframes=T, clips_per_step=8, device=cpu)
    os.makedirs(root / "kitti" / "training" / "flow_occ", exist_ok=True)
    enc = flow_io.kitti_encode(np.zeros((8, 8, 2)))
    flow_io.write_png(str(root / "kitti" / "training" / "flow_occ" / "000000_10.png"), enc)
    with pytest.raises(RuntimeError, match="GPU"):
        evaluate.validate_kitti_mf(model, iters=3, multi_root=str(root / "kitti"), nframes=3, clips_per_step=8, device=cpu)
    with pytest.raises(ValueError):
        evaluate.sintel_report(model, iters=3, root=str(root), nframes=T, clips_per_step=0, device=cpu)


def test_clips_per_step_one_is_the_call_without_it(tree, capsys):
    root, gts, _ = tree
    model = _stub(gts)
    a = evaluate.sintel_report(model, iters=3, root=str(root), nframes=T)
    b = evaluate.sintel_report(model, iters=3, root=str(root), nframes=T, clips_per_step=1)
    assert a == b and set(a) == {"clean", "final"} and set(a["clean"]) == {"epe", "1px", "3px", "5px", "pairs"}
    assert evaluate.validate_sintel_mf(model, iters=3, root=str(root), nframes=T, clips_per_step=1) == \
        evaluate.validate_sintel_mf(model, iters=3, root=str(root), nframes=T)


def test_command_line_parses(capsys):
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    for word in ("--dataset", "sintel_occ", "kitti_tile", "spring", "--ckpt", "--root", "--T", "--iters", "--clips-per-step", "--preset"):
        assert word in out, word
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--dataset", "chairs", "--ckpt", "x", "--root", "y"])
    assert e.value.code != 0


def test_entry_point_is_declared_everywhere():
    import ctypes
    from streamflow_amd import _lib, build, scoring
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(repo, "include", "streamflow_hip.h")).read()
    for name in ("sf_flow_score_batch", "sf_flow_score_batch_ws_bytes"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, hdr)
    assert "flow_score_batch.hip" in build.SOURCES
    assert int(re.search(r"#define SF_SCORE_BATCH_MAX (\d+)", hdr).group(1)) == scoring.SCORE_BATCH_MAX == 32
    assert int(re.search(r"SF_EVAL_LEN = (\d+)", hdr).group(1)) == scoring.EVAL_LEN
    for name in ("PIXELS", "SUM_EPE", "LT1", "LT3", "LT5", "VALID", "SUM_EPE_VALID", "OUTLIER", "OCC", "SUM_EPE_OCC", "NOC", "SUM_EPE_NOC"):
        assert int(re.search(r"SF_EVAL_%s = (\d+)" % name, hdr).group(1)) == getattr(scoring, "EVAL_" + name), name
    assert ctypes.sizeof(_lib.SfScoreFields) == 3 * 32 * ctypes.sizeof(ctypes.c_void_p)
    assert len(_lib.SIGNATURES["sf_flow_score_batch"][1]) == 11
