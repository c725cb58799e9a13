"""CPU: the numpy restatements of point tracking and track drawing (tests/track_cases.py) held to scalar loops and to closed forms;
the query helpers and the Tracks record of streamflow_amd.track; the C ABI of libstreamflow_track (declared = bound = exported, the
main library's exports unchanged, bad arguments refused before any launch); and the per-point core (csrc/track_core.h) as a host
program under AddressSanitizer and UBSan, bitwise equal to the restatement on the special-value cases."""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import track_cases as tc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same(got, want):
    return np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]) and (len(got) < 3 or np.array_equal(got[2], want[2]))


def small_cases():
    out = []
    for seed, (K, h, w, P) in enumerate([(1, 1, 1, 3), (2, 2, 2, 9), (7, 5, 7, 40), (3, 3, 30, 33)]):
        fwd, bwd = tc.smooth_flows(seed, K, h, w), -tc.smooth_flows(seed + 50, K, h, w)
        xy, st, start = tc.initial_state(tc.random_queries(seed, P, h, w, n_frames=K + 1), h, w)
        out.append(dict(fwd=fwd, bwd=bwd, xy=xy, status=st, start=start, sticky=bool(seed % 2)))
        out.append(dict(fwd=fwd, bwd=None, xy=xy, status=st, start=None))
        sf, sb, q = tc.special_case(seed + 7, K, h, w, max(P, 16))
        xy, st, start = tc.initial_state(q, h, w)
        out.append(dict(fwd=sf, bwd=sb, xy=xy, status=st, start=start, beta=4.0))
    return out


def run32(c, fn=tc.advance32, **kw):
    args = dict(bwd=c.get("bwd"), state_xy=c["xy"], state_status=c["status"], start=c.get("start"), frame0=c.get("frame0", 0),
                alpha=c.get("alpha", tc.ALPHA), beta=c.get("beta", tc.BETA), sticky=c.get("sticky", False))
    args.update(kw)
    return fn(c["fwd"], **args)


def test_vectorised_restatement_equals_the_scalar_loop():
    seen = set()
    for c in small_cases():
        got, want = run32(c), run32(c, tc.advance_scalar)
        assert same(got, want)
        seen |= set(np.unique(got[1]).tolist())
        assert (got[2].sum(axis=1) == c["xy"].shape[1]).all()
    assert seen == {tc.VISIBLE, tc.OCCLUDED, tc.LOST, tc.PENDING}
    fwd = tc.smooth_flows(3, 2, 4, 6)
    assert same(tc.advance32(fwd, -fwd), tc.advance_scalar(fwd, -fwd))   # dense mode


def test_integer_translation_is_exact_until_the_point_leaves():
    h, w, K, d = 9, 12, 4, (2, -1)
    fwd = np.empty((K, 2, h, w), F32)
    fwd[:, 0], fwd[:, 1] = d
    xy0, st0 = tc.grid_state(h, w)
    xy, st, _ = tc.advance32(fwd, None, xy0, st0)
    for k in range(K):
        for i in range(h * w):
            x0, y0 = i % w, i // w
            steps = 0                                                    # the steps the point could take before leaving the frame
            while steps < k + 1 and 0 <= x0 + (steps + 1) * d[0] <= w - 1 and 0 <= y0 + (steps + 1) * d[1] <= h - 1:
                steps += 1
            lost = steps < k + 1
            assert st[k, i] == (tc.LOST if lost else tc.VISIBLE)
            assert (xy[k, 0, i], xy[k, 1, i]) == (x0 + steps * d[0], y0 + steps * d[1])       # frozen where it last stood
    assert (st[-1] == tc.LOST).any() and (st[-1] == tc.VISIBLE).any()


def test_affine_field_composes_within_the_derived_bound():
    """flow(x) = A x + t - x sampled bilinearly is A x + t - x again in exact arithmetic (bilinear interpolation reproduces affine
    functions), so K steps are M^K(x), M(x) = A x + t.  The bound on the fp32 result, per coordinate, with u = 2^-24, F the largest
    |field value| and S = max(h, w):
      one sampled component carries at most 7 roundings in a chain -- the stored value (1), the weight 1 - fx or 1 - fy (1 each, 2;
      fx = px - floor(px) itself is exact), product and sum of the row blend (2), product and sum of the column blend (2) -- on
      magnitudes <= F (the weights are in [0, 1]), so its error is <= 7 u F, and 8 u F covers every second-order term (< 30 u^2 F);
      q = p + value rounds once on a magnitude < S: + u S.
    A step's error e = (8 F + S) u enters the next steps through M, whose Lipschitz constant in the maximum norm is ||A||_inf, so
      |p_K - M^K(p_0)|_inf <= e (1 + ||A||_inf + ... + ||A||_inf^(K-1)).
    The reference is the float64 composition, whose own error (1e-16 S per step) is five orders below e."""
    h, w, K = 24, 40, 7
    th = 0.02
    A = np.array([[1.01 * np.cos(th), -np.sin(th)], [np.sin(th), 0.99 * np.cos(th)]])
    t = np.array([0.6, -0.35])
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    grid = np.stack([xs, ys])
    field = (np.einsum("ij,jhw->ihw", A, grid) + t[:, None, None] - grid).astype(F32)
    fwd = np.broadcast_to(field, (K, 2, h, w))
    rng = np.random.default_rng(5)
    q = np.stack([np.zeros(200), rng.uniform(8, w - 9, 200), rng.uniform(6, h - 7, 200)], axis=1).astype(F32)
    xy0, st0, start = tc.initial_state(q, h, w)
    xy, st, _ = tc.advance32(fwd, None, xy0, st0, start)
    u, F, S = 2.0 ** -24, float(np.abs(field).max()), float(max(h, w))
    e, norm = (8 * F + S) * u, np.abs(A).sum(axis=1).max()
    p = xy0.astype(np.float64)
    worst = 0.0
    for k in range(K):
        p = A @ p + t[:, None]
        assert (p.min() > 1) and (p[0].max() < w - 2) and (p[1].max() < h - 2)          # the case keeps every point well inside
        bound = e * sum(norm ** j for j in range(k + 1))
        err = np.abs(xy[k] - p).max()
        worst = max(worst, err / bound)
        assert err <= bound, (k, err, bound)
        assert (st[k] == tc.VISIBLE).all()
    assert worst > 0.01                                                  # (the bound is not vacuous: within two orders of what is seen)


def test_status_logic():
    h, w, K = 6, 8, 5
    zero = np.zeros((K, 2, h, w), F32)
    q = np.array([[0, 1, 1], [3, 2, 2], [9, 3, 3], [2, np.nan, 1], [2, 8, 1], [0, -0.0, 0], [1, 7, 5]], F32)
    xy0, st0, start = tc.initial_state(q, h, w)
    xy, st, counts = tc.advance32(zero, None, xy0, st0, start, frame0=0)
    P, L, V = tc.PENDING, tc.LOST, tc.VISIBLE
    assert st[:, 0].tolist() == [V] * 5                                  # started at frame 0: active on entry
    assert st[:, 1].tolist() == [P, P, V, V, V]                          # starts at frame 3 = row 2, in the middle of the batch
    assert st[:, 2].tolist() == [P] * 5                                  # starts after the batch
    assert st[:, 3].tolist() == [P, L, L, L, L] and st[:, 4].tolist() == [P, L, L, L, L]     # a NaN query, a query at x = w
    assert st[:, 5].tolist() == [V] * 5 and st[:, 6].tolist() == [V] * 5                     # -0.0 and the far corner are inside
    assert np.array_equal(bits(xy[:, :, 3]), bits(np.broadcast_to(xy0[:, 3], (K, 2))))       # rows hold the query, NaN bits and all
    assert counts.tolist()[0] == [3, 0, 0, 4] and counts.tolist()[-1] == [4, 0, 2, 1]
    # the same batch entered at frame0 = 3: the point of frame 3 is active on entry, and steps in row 0
    move = zero.copy()
    move[:, 0] = 1.0
    xy3, st3, _ = tc.advance32(move, None, xy0, st0, start, frame0=3)
    assert st3[0, 1] == V and xy3[0, 0, 1] == 3.0 and st3[:, 2].tolist() == [P, P, P, P, P][:5]
    # occlusion: bwd = -fwd is consistent, bwd = 0 with a large fwd is not; sticky keeps OCCLUDED, without it the point recovers
    fwd = np.zeros((3, 2, h, w), F32)
    fwd[0, 0] = 2.0
    bwd = np.zeros_like(fwd)
    one = (np.array([[1.0], [1.0]], F32), np.array([tc.PENDING], np.uint8))
    assert tc.advance32(fwd, bwd, *one)[1][:, 0].tolist() == [tc.OCCLUDED, V, V]
    assert tc.advance32(fwd, bwd, *one, sticky=True)[1][:, 0].tolist() == [tc.OCCLUDED] * 3
    assert tc.advance32(fwd, -fwd, *one, sticky=True)[1][:, 0].tolist() == [V, V, V]
    assert tc.advance32(fwd, None, *one)[1][:, 0].tolist() == [V, V, V]
    bwd[...] = np.nan
    assert tc.advance32(fwd, bwd, *one)[1][:, 0].tolist() == [tc.OCCLUDED] * 3               # a NaN tap: not visible, still advancing
    for c in small_cases():
        if c["bwd"] is None:
            assert not (run32(c)[1] == tc.OCCLUDED).any()
    # a state byte above PENDING reads as LOST
    assert tc.advance32(zero, None, one[0], np.array([77], np.uint8))[1][:, 0].tolist() == [L] * 5


def test_split_with_carried_state_is_the_single_call():
    for c in small_cases():
        if c["fwd"].shape[0] != 7:
            continue
        whole = run32(c)
        a = run32(dict(c, fwd=c["fwd"][:3], bwd=None if c["bwd"] is None else c["bwd"][:3]))
        b = run32(dict(c, fwd=c["fwd"][3:], bwd=None if c["bwd"] is None else c["bwd"][3:], xy=a[0][-1], status=a[1][-1], frame0=3))
        assert same((np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]])), whole)


def test_line_points():
    assert tc.line_points(0, 0, 3, 0) == [(1, 0), (2, 0), (3, 0)]
    assert tc.line_points(5, 5, 1, 3) == [(4, 4), (3, 4), (2, 3), (1, 3)]                     # y: (2 * 2 s + 4) // 8 = 1, 1, 2, 2
    assert tc.line_points(2, 2, 2, 2) == [] and tc.line_points(0, 0, 65, 1) == [] and len(tc.line_points(0, 0, -64, 1)) == 64
    for a, b in [((0, 0), (7, 3)), ((9, 1), (2, 8)), ((3, 3), (3, -4))]:
        pts = tc.line_points(*a, *b)
        assert pts[-1] == b and all(max(abs(p[0] - q[0]), abs(p[1] - q[1])) == 1 for p, q in zip([a] + pts, pts))


@pytest.mark.parametrize("P,trail", [(1, 1), (1, 4), (6, 4), (6, 1)])
def test_draw_restatement_equals_the_scalar_loop(P, trail):
    h, w, n_rows = 13, 70, 6
    xy, status = tc.draw_case(P, n_rows, P, h, w)
    rng = np.random.default_rng(P)
    frames = rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    alpha = np.linspace(255, 60, trail).astype(np.uint8)
    for first_frame, first_row, occ in [(3, 0, False), (2, 1, True)]:
        args = (frames, first_frame, xy, status, first_row, trail, 3, 1, tc.small_palette(), alpha, occ)
        got, want = tc.draw32(*args), tc.draw_scalar(*args)
        assert np.array_equal(got, want)
        assert (got != frames).any()
    if trail > 1 and P == 1:                                             # the 69-step jump of point 0 is not drawn: no key in the middle of the bottom row
        assert np.array_equal(got[:, h - 1, 20:50], frames[:, h - 1, 20:50])


def test_queries_and_the_tracks_record(tmp_path):
    from streamflow_amd import track
    q = track.grid_queries((10, 17), 4, frame=2)
    assert q.dtype == np.float32 and q.shape == (3 * 5, 3) and (q[:, 0] == 2).all()
    assert sorted(set(q[:, 1].tolist())) == [0, 4, 8, 12, 16] and sorted(set(q[:, 2].tolist())) == [0, 4, 8]
    assert track.grid_queries((10, 16), 4)[:, 1].min() == 1                 # centred: 1, 5, 9, 13 of 0 .. 15
    with pytest.raises(ValueError):
        track.grid_queries((10, 16), 0)
    np.save(tmp_path / "q.npy", q)
    assert np.array_equal(track.load_queries(str(tmp_path / "q.npy")), q)
    (tmp_path / "q.txt").write_text("# t x y\n0 1.5 2\n\n3, 4 5.25  # later\n")
    assert track.load_queries(str(tmp_path / "q.txt")).tolist() == [[0, 1.5, 2], [3, 4, 5.25]]
    (tmp_path / "bad.txt").write_text("0 1\n")
    with pytest.raises(ValueError, match="line 1"):
        track.load_queries(str(tmp_path / "bad.txt"))
    (tmp_path / "neg.txt").write_text("-1 1 1\n")
    with pytest.raises(ValueError, match="frame number"):
        track.load_queries(str(tmp_path / "neg.txt"))
    assert np.array_equal(track.parse_track_arg("grid:4", (10, 17)), track.grid_queries((10, 17), 4))
    status = np.array([[0, 3, 0], [0, 0, 2], [1, 0, 2], [1, 0, 2]], np.uint8)
    t = track.Tracks(np.zeros((4, 3, 2), np.float32), status, q[:3])
    assert (t.n_frames, t.n_points) == (4, 3) and t.lengths().tolist() == [4, 3, 1]
    r = t.report()
    assert (r["visible"], r["occluded"], r["lost"], r["median_length"]) == (1 / 3, 1 / 3, 1 / 3, 3.0)
    assert t.report_line().startswith("Tracks points: 3, frames: 4")
    xy, st = t.planar()
    assert tuple(xy.shape) == (4, 2, 3) and xy.is_contiguous() and tuple(st.shape) == (4, 3)
    t.save(str(tmp_path / "t.npz"))
    with np.load(tmp_path / "t.npz") as z:
        assert sorted(z.files) == ["queries", "status", "xy"] and np.array_equal(z["status"], status)
    with pytest.raises(ValueError):
        track.Tracks(np.zeros((4, 3, 2), np.float32), status[:3], q[:3])
    pal, fade = track.default_palette(), track.alpha_fade(16)
    assert pal.shape == (55, 3) and pal.dtype == np.uint8 and len({tuple(c) for c in pal}) == 55
    assert fade[0] == 255 and fade[-1] == 48 and (np.diff(fade.astype(int)) < 0).all() and track.alpha_fade(1).tolist() == [255]


def test_no_cpu_fallback():
    from streamflow_amd import ops, track
    frames = torch.zeros(5, 16, 16, 3, dtype=torch.uint8)
    if not torch.cuda.is_available():                                    # (with a GPU these two run: tests/test_gpu_track_video.py)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            track.track_points(lambda imgs: [], frames, track.grid_queries((16, 16), 4))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            track.dense_tracks(lambda imgs: [], frames)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.track_advance(torch.zeros(1, 2, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.draw_tracks(frames, torch.zeros(5, 2, 3), torch.zeros(5, 3, dtype=torch.uint8), 0)


def test_dense_tracks_refuses_what_does_not_fit_the_budget():
    from streamflow_amd import track
    frames = torch.zeros(9, 32, 48, 3, dtype=torch.uint8)
    with pytest.raises(MemoryError, match=str(9 * 32 * 48 * (8 + 8))):
        track.dense_tracks(lambda imgs: [], frames, budget_bytes=1000)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from streamflow_amd import _track_lib, build
    if not os.path.exists(_track_lib.LIB_PATH):
        build.build(verbose=False)
    return _track_lib.load()


def _exports(path):
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    assert os.path.exists(nm)
    syms = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in syms.splitlines() if ln.split()}


def test_declared_bound_and_exported_are_one_set(lib):
    from streamflow_amd import _lib, _track_lib
    hdr = open(os.path.join(REPO, "include", "streamflow_track.h")).read()
    declared = set(re.findall(r"^\s*(?:int|int64_t|const char\*)\s+(sft_\w+)\s*\(", hdr, flags=re.M))
    assert len(declared) == 6 and declared == set(_track_lib.SIGNATURES)
    exported = _exports(_track_lib.LIB_PATH)
    assert {s for s in exported if s.startswith("sft_")} == declared
    # hidden visibility: nothing else of the library's own is exported (the HIP fat-binary handle is the toolchain's)
    assert all(s.startswith("sft_") or s.startswith("__hip") for s in exported), exported
    assert not any(s.startswith("sf_") for s in exported)
    assert lib.sft_version() == int(re.search(r"#define SFT_VERSION (\d+)", hdr).group(1)) == _track_lib.VERSION == 1
    for name in ("VISIBLE", "OCCLUDED", "LOST", "PENDING"):
        assert getattr(_track_lib, name) == int(re.search(r"SFT_%s = (\d+)" % name, hdr).group(1)) == getattr(tc, name)
    assert int(re.search(r"#define SFT_MAX_STEPS (\d+)", hdr).group(1)) == _track_lib.MAX_STEPS >= 256
    assert int(re.search(r"#define SFT_DRAW_MAX_SEG (\d+)", hdr).group(1)) == _track_lib.DRAW_MAX_SEG == tc.MAX_SEG == 64
    # the main library still exports exactly what it did: the 104 entry points of SF_VERSION 141, none of the new ones
    if not os.path.exists(_lib.LIB_PATH):
        from streamflow_amd import build
        build.build(verbose=False)
    main = sorted(s for s in _exports(_lib.LIB_PATH) if s.startswith("sf_") or s.startswith("sft_"))
    assert main == sorted(_lib.SIGNATURES) and len(main) == 104
    assert hashlib.sha256("\n".join(main).encode()).hexdigest() == "c3c65de0f558683e884f71c61679203383454450cb60196358bcfb3ca33dbe6d"
    assert _lib.load().sf_version() == 141
    main_hdr = open(os.path.join(REPO, "include", "streamflow_hip.h")).read()
    assert "#define SF_VERSION 141" in main_hdr and "sft_" not in main_hdr


def test_the_loader_says_when_the_library_is_missing(monkeypatch, tmp_path):
    from streamflow_amd import _track_lib
    monkeypatch.setattr(_track_lib, "_lib", None)
    monkeypatch.setattr(_track_lib, "LIB_PATH", str(tmp_path / "libstreamflow_track.so"))
    with pytest.raises(RuntimeError, match="has not been built.*no CPU/PyTorch fallback"):
        _track_lib.load()


def _advance(lib, **kw):
    a = dict(fwd=0x10000, fs=200, cs=100, rs=10, bwd=0x20000, bfs=200, bcs=100, brs=10, K=2, h=10, w=10, frame0=0, sxy=0x30000,
             sst=0x40000, start=0x50000, P=5, alpha=0.01, beta=0.5, sticky=0, oxy=0x60000, ost=0x70000, sxo=None, sso=None, counts=None,
             ws=None, wsb=0)
    a.update(kw)
    return lib.sft_track_advance(a["fwd"], a["fs"], a["cs"], a["rs"], a["bwd"], a["bfs"], a["bcs"], a["brs"], a["K"], a["h"], a["w"],
                                 a["frame0"], a["sxy"], a["sst"], a["start"], a["P"], a["alpha"], a["beta"], a["sticky"], a["oxy"],
                                 a["ost"], a["sxo"], a["sso"], a["counts"], a["ws"], a["wsb"], None)


def _draw(lib, **kw):
    a = dict(src=0x10000, sf=300, sr=30, sp=3, sc=1, n=1, h=10, w=10, first=0, xy=0x20000, st=0x30000, rows=4, P=5, first_row=0, trail=4,
             r=3, tr=1, occ=0, pal=0x40000, L=7, at=0x50000, out=0x60000, ws=0x70000, wsb=400)
    a.update(kw)
    return lib.sft_draw_tracks(a["src"], a["sf"], a["sr"], a["sp"], a["sc"], a["n"], a["h"], a["w"], a["first"], a["xy"], a["st"], a["rows"],
                               a["P"], a["first_row"], a["trail"], a["r"], a["tr"], a["occ"], a["pal"], a["L"], a["at"], a["out"], a["ws"],
                               a["wsb"], None)


def test_bad_arguments_are_refused_before_any_launch(lib):
    """Dummy, never dereferenced pointers on a machine without a GPU: every one of these returns SFT_ERR_BAD_ARG with a message."""
    bad_advance = [dict(fwd=None), dict(oxy=None), dict(ost=None), dict(sxy=None), dict(sst=None), dict(sxy=None, sst=None, P=99),
                   dict(sxo=0x1000), dict(sso=0x1000), dict(rs=0), dict(rs=9), dict(cs=0), dict(fs=0), dict(brs=0), dict(bcs=0),
                   dict(bfs=-1), dict(K=0), dict(K=4097), dict(P=0), dict(P=2 ** 31), dict(h=0), dict(w=0), dict(h=2 ** 16, w=2 ** 15),
                   dict(frame0=-1), dict(alpha=float("nan")), dict(fwd=0x10002), dict(wsb=-1)]
    for kw in bad_advance:
        assert _advance(lib, **kw) == -1, kw
        assert lib.sft_last_error().startswith(b"sft_track_advance"), kw
    assert b"dense mode" in (_advance(lib, sxy=None, sst=None, P=99), lib.sft_last_error())[1]
    assert b"come together" in (_advance(lib, sst=None), lib.sft_last_error())[1]
    assert b"n_steps" in (_advance(lib, K=4097), lib.sft_last_error())[1]
    assert lib.sft_track_advance_ws_bytes(0, 5) == -1 and lib.sft_track_advance_ws_bytes(3, 0) == -1
    assert lib.sft_track_advance_ws_bytes(3, 5) == 0
    bad_draw = [dict(src=None), dict(xy=None), dict(st=None), dict(pal=None), dict(at=None), dict(out=None), dict(ws=None), dict(P=1 << 20),
                dict(P=0), dict(trail=0), dict(trail=256), dict(r=17), dict(tr=-1), dict(L=0), dict(n=0), dict(h=0), dict(rows=0),
                dict(sr=-1), dict(first=-1), dict(wsb=399), dict(xy=0x20001)]
    for kw in bad_draw:
        assert _draw(lib, **kw) == -1, kw
        assert lib.sft_last_error().startswith(b"sft_draw_tracks"), kw
    assert b"2^20" in (_draw(lib, P=1 << 20), lib.sft_last_error())[1]
    assert lib.sft_draw_tracks_ws_bytes(2, 10, 10) == 800 and lib.sft_draw_tracks_ws_bytes(0, 10, 10) == -1


# ---- the per-point core as a host program under the sanitizers ------------------------------------------------------------------------

HOST_SRC = os.path.join(REPO, "streamflow_amd", "csrc", "host", "track_host_main.cpp")


def _clang():
    from streamflow_amd import build
    cands = [os.path.join(os.path.dirname(os.path.realpath(build.hipcc())), "..", "lib", "llvm", "bin", "clang++"),
             "/opt/rocm/lib/llvm/bin/clang++"]
    return next((c for c in cands if os.path.exists(c)), None) or shutil.which("clang++")


def test_the_core_runs_clean_under_the_sanitizers_and_equals_the_restatement(tmp_path):
    """csrc/host/track_host_main.cpp with -fsanitize=address,undefined -ffp-contract=off as its own process (nothing preloaded, nothing
    loaded into Python).  Every field and state array is a heap buffer of exactly its size: a tap formed from a NaN, an infinity or
    1e30 would be a read outside one."""
    cc = _clang()
    assert cc, "the ROCm clang++ is needed to build the host program"
    exe = str(tmp_path / "track_host")
    r = subprocess.run([cc, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        "-Wall", "-Werror", HOST_SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    cases = small_cases()
    # states that hold anything: positions far outside with an active status, every status byte
    sf, sb, q = tc.special_case(91, 7, 5, 7, 24)
    xy, st, start = tc.initial_state(q, 5, 7)
    st = (np.arange(24) % 6).astype(np.uint8)
    xy[0, 12:18] = [1e30, -5, 7.5, np.inf, -np.inf, np.nan]
    cases.append(dict(fwd=sf, bwd=sb, xy=xy, status=st, start=start, frame0=2, sticky=True))
    fin, fout = str(tmp_path / "cases.bin"), str(tmp_path / "rows.bin")
    tc.write_host_cases(fin, cases)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-4000:])
    for c, got in zip(cases, tc.read_host_rows(fout, cases)):
        assert same(got, run32(c)[:2])
