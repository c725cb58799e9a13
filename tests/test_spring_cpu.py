"""Spring validation and submission on the CPU (streamflow_amd.evaluate.spring_report / validate_spring_mf, submit.
create_spring_submission_mf; reference evaluate_mf.py:25-102, core/mf_datasets.py:47-213): the pairs scored and the files written
against literal restatements of the reference's dataset loops, and the report over synthetic trees against tests/score_cases.py,
with stand-in models that read a tag pixel from each frame (as test_evaluate_cpu.py does) and return host flows (the host path)."""
import glob
import os
import re
from argparse import Namespace

import numpy as np
import torch

from streamflow_amd import datasets, evaluate, flo5, flow_io, scoring, submit
from tests import score_cases as sc


# ---- the reference's loops, restated literally ----------------------------------------------------------------------------------
def _ref_eval_items(images, root, scene, cam, nframes):
    """SpringEval.__init__ (mf_datasets.py:121-165) for one camera: [(image paths, flow paths, frame ids)]."""
    out = []
    len_image = len(images)
    _future_flow_list = []
    for i in range(1, len_image):
        _future_flow_list.append(os.path.join(root, scene, f"flow_FW_{cam}", f"flow_FW_{cam}_{i:04d}.flo5"))
    i = 0
    while True:
        if i + nframes <= len(images):
            imgs = images[i:i + nframes]
            flows = _future_flow_list[i:i + nframes - 1]
            ids = [j for j in range(i, i + nframes)]
        else:
            imgs = images[len(images) - nframes:len(images)]
            flows = _future_flow_list[len(_future_flow_list) - nframes + 1:len(_future_flow_list)]
            ids = [-1 if j < i else j for j in range(len(images) - nframes, len(images))]
        out.append((imgs, flows, ids))
        if i + nframes >= len(images):
            break
        else:
            i += nframes - 1
    images = images[::-1]
    _past_flow_list = []
    for i in range(len_image, 1, -1):
        _past_flow_list.append(os.path.join(root, scene, f"flow_BW_{cam}", f"flow_BW_{cam}_{i:04d}.flo5"))
    i = 0
    while True:
        if i + nframes <= len(images):
            imgs = images[i:i + nframes]
            flows = _past_flow_list[i:i + nframes - 1]
            ids = [j for j in range(i, i + nframes)]
        else:
            imgs = images[len(images) - nframes:len(images)]
            flows = _past_flow_list[len(_past_flow_list) - nframes + 1:len(_past_flow_list)]
            ids = [-1 if j < i else j for j in range(len(images) - nframes, len(images))]
        out.append((imgs, flows, ids))
        if i + nframes >= len(images):
            break
        else:
            i += nframes - 1
    return out


def _ref_submission_items(img_filenames, scene, cam, nframes):
    """SpringSubmission.__init__ (mf_datasets.py:55-88) for one camera: [(image paths, (scene, direction, cam, frame ids))]."""
    out = []
    i = 0
    while True:
        if i + nframes <= len(img_filenames):
            imgs = img_filenames[i:i + nframes]
            info = [scene, 'FW', cam, [j + 1 for j in range(i, i + nframes)]]
        else:
            imgs = img_filenames[len(img_filenames) - nframes:len(img_filenames)]
            ids = [-1 if j < i else j + 1 for j in range(len(img_filenames) - nframes, len(img_filenames))]
            info = [scene, 'FW', cam, ids]
        out.append((imgs, info))
        if i + nframes >= len(img_filenames):
            break
        else:
            i += nframes - 1
    img_filenames = img_filenames[::-1]
    i = 0
    while True:
        if i + nframes <= len(img_filenames):
            imgs = img_filenames[i:i + nframes]
            info = [scene, 'BW', cam, [len(img_filenames) - j for j in range(i, i + nframes)]]
        else:
            imgs = img_filenames[len(img_filenames) - nframes:len(img_filenames)]
            ids = [-1 if j < i else len(img_filenames) - j for j in range(len(img_filenames) - nframes, len(img_filenames))]
            info = [scene, 'BW', cam, ids]
        out.append((imgs, info))
        if i + nframes >= len(img_filenames):
            break
        else:
            i += nframes - 1
    return out


# ---- pair and file mapping ------------------------------------------------------------------------------------------------------
_CAMS = {"left": 0, "right": 1}
_FRAME = re.compile(r"frame_(left|right)_(\d{4})\.png$")


def _tag_image(path):
    """Stand-in for evaluate._image on an empty file: a 4 x 4 frame filled with (camera, frame number, 0)."""
    cam, num = _FRAME.search(path).groups()
    t = torch.zeros(3, 4, 4)
    t[0], t[1] = _CAMS[cam], int(num)
    return t


def _tag_model(images, iters=0, test_mode=False):
    """The flow of pair k names the pair: u = 1000 camera + frame number of image k, v = frame number of image k + 1."""
    assert test_mode
    out = []
    for a, b in zip(images[:-1], images[1:]):
        f = torch.zeros(1, 2, *a.shape[-2:])
        f[0, 0] = 1000 * a[0, 0, 0, 0] + a[0, 1, 0, 0]
        f[0, 1] = b[0, 1, 0, 0]
        out.append(f)
    return out


def _touch_tree(root, scene, n):
    for cam in ("left", "right"):
        d = os.path.join(root, scene, f"frame_{cam}")
        os.makedirs(d, exist_ok=True)
        for i in range(n):
            open(os.path.join(d, f"frame_{cam}_{i + 1:04d}.png"), "wb").close()


def test_pairs_and_files_match_the_reference_loops(tmp_path, monkeypatch):
    """For T = 2..6 and scenes of T..30 frames: the (pair, ground-truth file) set the validator scores equals the reference's, every
    file once; the submission writes exactly the reference's file names, every one once."""
    monkeypatch.setattr(datasets, "read_frame", lambda path: _tag_image(path).permute(1, 2, 0).numpy().astype(np.uint8))
    scored, read, written = [], [], []
    monkeypatch.setattr(flo5, "read_flo5", lambda path: (read.append(path), np.zeros((8, 8, 2), np.float32))[1])
    monkeypatch.setattr(scoring, "score_host",
                        lambda pred, gt, acc, step: scored.append((int(pred[0, 0, 0]), int(pred[1, 0, 0]), read[-1])))
    monkeypatch.setattr(flo5, "write_flo5", lambda path, flow, compression_level=5: written.append((path, compression_level)))
    for T in range(2, 7):
        for n in range(T, 31):
            root = str(tmp_path / f"t{T}_n{n}")
            train, test = os.path.join(root, "train"), os.path.join(root, "test")
            _touch_tree(train, "0041", n)
            _touch_tree(test, "0041", n)
            scored.clear(), read.clear(), written.clear()
            evaluate.spring_report(_tag_model, iters=1, root=root, nframes=T, device=torch.device("cpu"))
            want = []
            for cam in ("left", "right"):
                images = sorted(glob.glob(os.path.join(train, "0041", f"frame_{cam}", "*.png")))
                for imgs, flows, ids in _ref_eval_items(images, train, "0041", cam, T):
                    for i in range(T - 1):
                        if ids[i] != -1:
                            a, b = (int(_FRAME.search(p).group(2)) for p in (imgs[i], imgs[i + 1]))
                            want.append((1000 * _CAMS[cam] + a, b, flows[i]))
            assert sorted(scored) == sorted(want), (T, n)
            assert len(read) == len(set(read)) == 4 * (n - 1), (T, n)             # every ground-truth file once
            out = str(tmp_path / f"sub_t{T}_n{n}")
            submit.create_spring_submission_mf(Namespace(spring_root=root), _tag_model, iters=1, output_path=out, nframes=T,
                                               device=torch.device("cpu"))
            want_files = []
            for cam in ("left", "right"):
                imgs = sorted(glob.glob(os.path.join(test, "0041", f"frame_{cam}", "*.png")))
                for _, (scene, direction, cam_, frame_ids) in _ref_submission_items(imgs, "0041", cam, T):
                    output_dir = os.path.join(out, scene, f"flow_{direction}_{cam_}")
                    for i in range(T - 1):
                        if frame_ids[i] != -1:
                            want_files.append(os.path.join(output_dir, f"flow_{direction}_{cam_}_%04d.flo5" % (frame_ids[i])))
            paths = [p for p, _ in written]
            assert sorted(paths) == sorted(want_files) and len(paths) == len(set(paths)), (T, n)
            assert {lvl for _, lvl in written} == {5}


# ---- report values on a synthetic tree ------------------------------------------------------------------------------------------
H, W, T = 20, 28, 3                                                      # not multiples of 8: the padder is exercised
SCENES = {"0007": 4, "0041": 5}


def _noise(key, h, w):
    s, c, direction, a = key
    g = np.random.default_rng(1000 * s + 100 * c + 50 * (direction == "BW") + a)
    return g.normal(0.0, 1.5, size=(2, h, w)).astype(np.float32)


def _write_tree(root, nan_share, seed):
    """train/<scene>/frame_<cam>/frame_<cam>_NNNN.png with a tag pixel (scene, camera, frame index) and the ground truth of every
    pair (forward and backward) at 2H x 2W, decoys (1e6) at odd rows and columns.  Returns {(scene, cam, dir, source index): gt}."""
    rng = np.random.default_rng(seed)
    gts = {}
    for s, (scene, n) in enumerate(SCENES.items()):
        for c, cam in enumerate(("left", "right")):
            d = os.path.join(root, "train", scene, f"frame_{cam}")
            os.makedirs(d)
            for i in range(n):
                img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
                img[0, 0] = (s, c, i)
                flow_io.write_png(os.path.join(d, f"frame_{cam}_{i + 1:04d}.png"), img)
            for direction in ("FW", "BW"):
                os.makedirs(os.path.join(root, "train", scene, f"flow_{direction}_{cam}"))
                for a in (range(n - 1) if direction == "FW" else range(1, n)):
                    g = sc.random_gt(rng, H, W, 2, nan_share)
                    gts[(s, c, direction, a)] = g
                    flo5.write_flo5(os.path.join(root, "train", scene, f"flow_{direction}_{cam}",
                                                 f"flow_{direction}_{cam}_{a + 1:04d}.flo5"), g)
    return gts


def _stub(gts, calls=None):
    def model(images, iters=0, test_mode=False):
        assert test_mode and len(images) == T and all(im.shape == (1, 3, 24, 32) for im in images)
        pt, pl = (24 - H) // 2, (32 - W) // 2
        tags = [tuple(int(v) for v in im[0, :, pt, pl]) for im in images]
        flows = []
        for (s, c, a), (_, _, b) in zip(tags[:-1], tags[1:]):
            key = (s, c, "FW" if b == a + 1 else "BW", a)
            f = torch.zeros(1, 2, 24, 32)
            f[0, :, pt:pt + H, pl:pl + W] = torch.from_numpy(sc.subsample(gts[key], 2, H, W) + _noise(key, H, W))
            flows.append(f)
        if calls is not None:
            calls.append(tags)
        return flows
    return model


def _expected(gts, scenes):
    pairs = []
    for s, (scene, n) in enumerate(SCENES.items()):
        if scene not in scenes:
            continue
        for c in range(2):
            for key in [(s, c, "FW", a) for a in range(n - 1)] + [(s, c, "BW", a) for a in range(n - 1, 0, -1)]:
                gsub = sc.subsample(gts[key], 2, H, W)
                pairs.append((gsub + _noise(key, H, W), gsub))
    return sc.restate(pairs), len(pairs)


def _check_report(rep, want, npairs):
    assert rep["pairs"] == npairs
    c = want["counts"]
    assert rep["pixels"] == c["pixels"] and rep["valid_pixels"] == c["valid"]
    for k in sc.KEYS:
        print(k, rep[k], want["f64"][k], want["ref32"][k])
        assert sc.close(rep[k], want["f64"][k], 1e-8), (k, rep[k], want["f64"][k])
        # the reference's float32 np.mean: measured 2.6e-7 .. 3.8e-7 from the fp64 mean at 2M .. 16M pixels; 5x margin
        assert sc.close(rep[k], want["ref32"][k], 2e-6), (k, rep[k], want["ref32"][k])


def test_report_on_a_synthetic_tree(tmp_path, capsys):
    gts = _write_tree(str(tmp_path), 0.1, seed=5)
    acc_counts = {}
    for scenes, names in ((("0041",), {"0041"}), (None, set(SCENES))):
        rep = evaluate.spring_report(_stub(gts), iters=2, root=str(tmp_path), nframes=T, device=torch.device("cpu"), scenes=scenes)
        want, npairs = _expected(gts, names)
        c = want["counts"]
        assert np.isnan(rep["epe"]) and np.isfinite(rep["epe_valid"])
        for k in ("s0_10", "s10_40", "s40"):                               # every bucket holds at least a fifth of the valid pixels
            assert c[k] >= c["valid"] / 5, (k, c)
        _check_report(rep, want, npairs)
        acc_counts[scenes] = rep
    assert acc_counts[("0041",)]["pairs"] == 2 * 2 * 4 and acc_counts[None]["pairs"] == 2 * 2 * (4 + 3)
    out = capsys.readouterr().out
    assert "Validation EPE: nan, 1px:" in out and "Spring 1px: " in out and "1px(s0~10): " in out and "1px(s40+): " in out
    calls = []
    epe = evaluate.validate_spring_mf(_stub(gts, calls), iters=2, root=str(tmp_path), nframes=T, device=torch.device("cpu"))
    assert np.isnan(epe) and len(calls) == 2 * 2 * 2                      # only 0041 (5 frames, T = 3: two clips per direction)


def test_report_without_nan(tmp_path):
    gts = _write_tree(str(tmp_path), 0.0, seed=6)
    rep = evaluate.spring_report(_stub(gts), iters=2, root=str(tmp_path), nframes=T, device=torch.device("cpu"), scenes=None)
    want, npairs = _expected(gts, set(SCENES))
    _check_report(rep, want, npairs)
    assert np.isfinite(rep["epe"]) and rep["epe"] == rep["epe_valid"] and rep["valid_pixels"] == rep["pixels"]
    epe = evaluate.validate_spring_mf(_stub(gts), iters=2, root=str(tmp_path), nframes=T, device=torch.device("cpu"), scenes=None)
    assert epe == rep["epe"]


# ---- submission -----------------------------------------------------------------------------------------------------------------
def test_submission_files_hold_the_model_flows(tmp_path):
    rng = np.random.default_rng(7)
    lengths = {"0003": 4, "0010": 5}
    for s, (scene, n) in enumerate(lengths.items()):
        for c, cam in enumerate(("left", "right")):
            d = tmp_path / "test" / scene / f"frame_{cam}"
            os.makedirs(d)
            for i in range(n):
                img = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
                img[0, 0] = (s, c, i)
                flow_io.write_png(str(d / f"frame_{cam}_{i + 1:04d}.png"), img)

    def flow_of(s, c, a, b):
        return np.random.default_rng(10000 * s + 1000 * c + 10 * a + b).normal(0, 7, size=(H, W, 2)).astype(np.float32)

    def model(images, iters=0, test_mode=False):
        pt, pl = (24 - H) // 2, (32 - W) // 2
        tags = [tuple(int(v) for v in im[0, :, pt, pl]) for im in images]
        out = []
        for (s, c, a), (_, _, b) in zip(tags[:-1], tags[1:]):
            f = torch.full((1, 2, 24, 32), 1e6)
            f[0, :, pt:pt + H, pl:pl + W] = torch.from_numpy(flow_of(s, c, a, b)).permute(2, 0, 1)
            out.append(f)
        return out

    out = str(tmp_path / "sub")
    submit.create_spring_submission_mf(Namespace(spring_root=str(tmp_path)), model, iters=2, output_path=out, nframes=3,
                                       device=torch.device("cpu"))
    files = sorted(glob.glob(os.path.join(out, "*", "*", "*.flo5")))
    assert len(files) == 2 * 2 * ((4 - 1) + (5 - 1))
    for s, (scene, n) in enumerate(lengths.items()):
        for c, cam in enumerate(("left", "right")):
            for a in range(n - 1):                                           # forward: source a -> a + 1, file a + 1
                got = flo5.read_flo5(os.path.join(out, scene, f"flow_FW_{cam}", f"flow_FW_{cam}_{a + 1:04d}.flo5"))
                assert got.shape == (H, W, 2) and got.tobytes() == flow_of(s, c, a, a + 1).tobytes()
            for a in range(1, n):                                            # backward: source a -> a - 1, file a + 1
                got = flo5.read_flo5(os.path.join(out, scene, f"flow_BW_{cam}", f"flow_BW_{cam}_{a + 1:04d}.flo5"))
                assert got.shape == (H, W, 2) and got.tobytes() == flow_of(s, c, a, a - 1).tobytes()
