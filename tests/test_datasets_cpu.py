"""The plumbing shared by the dataset loops (streamflow_amd/datasets.py) on the CPU: the three public views of the clip schedule
against the one definition in video.py, and the three public readers of a PNG frame against each other."""
import numpy as np


def test_the_three_schedule_views_agree():
    """T = 2..9, n = T..60: evaluate.sintel_clip_schedule (frame ids), demo.group_clips (keep flags) and video.clip_count /
    clip_start / pair_clip give the same clips, the same kept pairs, and the same owner of every pair."""
    from streamflow_amd import demo, evaluate, video
    cases = 0
    for T in range(2, 10):
        for n in range(T, 61):
            ids = evaluate.sintel_clip_schedule(n, T)
            keep = demo.group_clips(n, T)
            nc = video.clip_count(n, T)
            assert len(ids) == len(keep) == nc, (n, T)
            for c in range(nc):
                first = video.clip_start(c, n, T)
                assert ids[c][0] == keep[c][0] == first, (n, T, c)
                assert len(ids[c][1]) == T and len(keep[c][1]) == T - 1
                assert ids[c][1][T - 1] == first + T - 1                 # the last frame of a clip starts no pair of it: never flagged
                for k in range(T - 1):
                    assert (ids[c][1][k] != -1) == keep[c][1][k], (n, T, c, k)
                    if keep[c][1][k]:
                        assert ids[c][1][k] == first + k and video.pair_clip(first + k, n, T) == (c, k), (n, T, c, k)
            assert sum(sum(k) for _, k in keep) == n - 1, (n, T)         # every pair of the video exactly once
            cases += 1
    assert cases == 444


def test_the_three_frame_readers_agree(tmp_path):
    """5 x 7 PNGs as grey, grey + alpha, RGB and RGBA: video.FrameDir, datasets.read_frame and evaluate._image (back to uint8 HWC)
    give one array -- the grey channel replicated, the colour channels with alpha dropped."""
    from streamflow_amd import datasets, evaluate, flow_io, video
    rng = np.random.default_rng(3)
    grey = rng.integers(0, 256, size=(5, 7), dtype=np.uint8)
    ga = rng.integers(0, 256, size=(5, 7, 2), dtype=np.uint8)
    rgb = rng.integers(0, 256, size=(5, 7, 3), dtype=np.uint8)
    rgba = rng.integers(0, 256, size=(5, 7, 4), dtype=np.uint8)
    written = (grey, ga, rgb, rgba)
    for i, img in enumerate(written):
        flow_io.write_png(str(tmp_path / f"f_{i}.png"), img)
        assert flow_io.read_png(str(tmp_path / f"f_{i}.png")).shape == img.shape       # the files hold what their names say
    want = (np.repeat(grey[:, :, None], 3, axis=2), np.repeat(ga[:, :, :1], 3, axis=2), rgb, rgba[:, :, :3])
    fd = video.FrameDir(str(tmp_path))
    assert len(fd) == 4 and fd.hw == (5, 7)
    for i in range(4):
        path = str(tmp_path / f"f_{i}.png")
        a, b, t = fd[i], datasets.read_frame(path), evaluate._image(path)
        assert a.dtype == b.dtype == np.uint8 and a.shape == b.shape == (5, 7, 3) and b.flags["C_CONTIGUOUS"]
        assert t.dtype.is_floating_point and tuple(t.shape) == (3, 5, 7)
        c = t.permute(1, 2, 0).numpy()
        assert np.array_equal(c, c.astype(np.uint8))                     # whole numbers in 0..255: the conversion back is exact
        assert np.array_equal(a, want[i]) and np.array_equal(b, want[i]) and np.array_equal(c.astype(np.uint8), want[i]), i
