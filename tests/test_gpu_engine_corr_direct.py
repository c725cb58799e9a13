"""The volume-free correlation route through the layers above the kernels (-m gpu): HotPathEngine with EngineOptions(corr_direct=True)
against the reference's golden forwards under the contract the volume route is held to in tests/test_gpu_parity.py (EPE <= 1e-3 px;
low-resolution flows 1e-3 / 2e-3), the buffers a direct plan has and has not, the default options bitwise what they were,
corr_direct_min_px switching the route between two grids of one engine, CorrBlock(layout="direct") beside CorrBlock(layout="blocked")
with both held to float64 by bounds of their own, and the public surface: args.corr, `evaluate --corr`, `demo --corr`."""
import os

import numpy as np
import pytest
import torch

from tests import cases, corr_cases as cc, corr_direct_cases as dc, poison

pytestmark = pytest.mark.gpu
PRESETS = ("fp32_class", "config2_fp16", "config2_mixed")
T, ITERS, D = 3, 3, 256
GRID_A, GRID_C = (2, 16, 24), (1, 24, 40)                      # (clips, h, w): 384 and 960 pixels


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _engine(dev, preset, graph=False, params=None, Tn=T, **opt):
    from streamflow_amd import presets, synthetic as syn
    from streamflow_amd.engine import EngineOptions, HotPathEngine
    return HotPathEngine(params if params is not None else syn.make_params(3, T), device=dev, T=Tn, use_graph=graph,
                         options=EngineOptions(**opt), **presets.engine_kwargs(preset))


def _features(dev, grid, seed=1):
    from streamflow_amd import synthetic as syn
    B, h, w = grid
    f, c = syn.make_features(100 * seed + h, B, T, h, w)
    return f.to(dev), c.to(dev)


def _run(eng, x, iters=ITERS):
    ups, low = eng.forward(x[0], x[1], iters=iters)
    out = [t.clone() for t in list(ups) + list(low)]
    torch.cuda.synchronize()
    return out


def _assert_same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(a).all()), f"{what}: non-finite values in flow {i}"
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), \
            f"{what}: flow {i} differs, max |diff| {float((a.double() - b.double()).abs().max()):.3e}"


# ---- against the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(cases.FORWARD_CASES))
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("preset", PRESETS)
def test_direct_engine_forward_vs_golden(golden, dev, tag, graph, preset):
    from oracle import streamflow_oracle as orc
    g = golden(tag)
    B, Tn, H, W, iters, seed, use_init = cases.FORWARD_CASES[tag]
    P, fmaps, cnets, finit, iters = cases.forward_inputs(tag)
    eng = _engine(dev, preset, graph, params=P, Tn=Tn, corr_direct=True)
    finit_d = None if finit is None else [f.to(dev) for f in finit]
    for rep in range(2):                                    # the second call: graph replay / buffer reuse
        ups, low = eng.forward(fmaps.to(dev), cnets.to(dev), iters=iters, flow_init=finit_d)
        for i in range(Tn - 1):
            e = orc.epe(ups[i].cpu(), torch.from_numpy(g[f"up{i}"]))
            print(f"{tag} {preset} corr_direct graph={graph} rep={rep} pair {i}: EPE vs reference = {e:.3e}")
            assert e <= 1e-3, f"{tag} {preset} pair {i}: EPE {e}"
            if use_init:
                err = (low[i].cpu() - torch.from_numpy(g[f"low{i}"])).abs().max().item()
                assert err <= (1e-3 if preset == "fp32_class" else 2e-3), (tag, preset, i, err)
    pl, = eng._plans.values()
    assert pl.corr_direct and pl.vol is None and pl.lvls is None and (pl.graph is not None) == graph


# ---- plans -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", PRESETS)
def test_direct_plan_keeps_no_volume_and_the_default_plan_is_unchanged(dev, preset):
    from streamflow_amd import ops
    from streamflow_amd.engine import EngineOptions
    x = _features(dev, GRID_A)
    Bc, h, w = GRID_A
    eng = _engine(dev, preset, corr_direct=True)
    got = _run(eng, x)
    pl = eng.plan(Bc, h, w, D)
    prec = ops.PRECISION_F16X3 if preset == "fp32_class" else ops.PRECISION_F16
    assert pl.corr_direct and pl.vol is None and pl.lvls is None and pl.corr_prec == prec
    assert pl.corr_ws.numel() * pl.corr_ws.element_size() == ops.corr_direct_ws_bytes(Bc, T - 1, D, h, w, prec)
    assert pl.corr_blocked == (preset != "fp32_class")               # the hand-over formats of the volume route it replaces
    assert [n for n, _ in poison.plan_buffers(pl)][0] == "corr_ws"
    with pytest.raises(RuntimeError, match="no correlation volume"):
        pl.taps(["volume"])
    assert pl.taps(["corr"])["corr"].shape == (pl.n, 324, h, w)
    # the defaults: bitwise the flows of corr_direct=False spelled out, and a volume
    eng_d, eng_f = _engine(dev, preset), _engine(dev, preset, corr_direct=False, corr_direct_min_px=0)
    assert eng_d.options == EngineOptions() == eng_f.options
    want = _run(eng_d, x)
    _assert_same(_run(eng_f, x), want, f"{preset}: defaults vs corr_direct=False")
    pv = eng_d.plan(Bc, h, w, D)
    assert not pv.corr_direct and pv.vol is not None and len(pv.taps(["volume"])["volume"]) == 4
    # the two routes are two computations of one function: close, not equal
    diff = max(float((a - b).abs().max()) for a, b in zip(got, want))
    print(f"{preset}: direct vs volume, max |flow difference| {diff:.3e} px")
    assert 0 < diff < 1e-2
    with pytest.raises(RuntimeError, match="corr_direct"):
        from streamflow_amd import synthetic as syn
        from streamflow_amd.engine import HotPathEngine
        HotPathEngine(syn.make_params(3, T), device=dev, T=T, precision="fp32", options=EngineOptions(corr_direct=True)).plan(Bc, h, w, D)


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("preset", ["config2_mixed", "fp32_class"])
def test_min_px_switches_the_route_between_two_grids_of_one_engine(dev, preset, graph):
    """corr_direct_min_px = 960: the 16 x 24 grid keeps its volume, the 24 x 40 grid runs direct.  A, C, A, C on one engine with the
    plans' buffers destroyed in between: bitwise the flows of fresh engines (the default one at A, corr_direct=True at C)."""
    xa, xc = _features(dev, GRID_A), _features(dev, GRID_C)
    want_a = _run(_engine(dev, preset, graph), xa)
    want_c = _run(_engine(dev, preset, graph, corr_direct=True), xc)
    eng = _engine(dev, preset, graph, corr_direct_min_px=GRID_C[1] * GRID_C[2])
    for rep, byte in enumerate((None, 0xFF, 0x7B)):
        for grid, x, want in ((GRID_A, xa, want_a), (GRID_C, xc, want_c)):
            pl = eng.plan(grid[0], grid[1], grid[2], D)
            assert pl.corr_direct == (grid is GRID_C) and (pl.vol is None) == (grid is GRID_C)
            if byte is not None:
                poison.poison_plan(pl, byte)
            _assert_same(_run(eng, x), want, f"{preset} graph={graph} visit {rep} grid {grid}")
            assert eng.plan(grid[0], grid[1], grid[2], D) is pl
    assert len(eng._plans) == 2


# ---- CorrBlock -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,k", [(torch.float16, "f16"), (torch.float32, "x3")], ids=["fp16", "fp32"])
@pytest.mark.parametrize("case_id", ["24x40-D64-B1p1", "8x9-D256-B2p1"])
def test_corr_block_direct_and_blocked_against_float64(dev, case_id, dtype, k):
    """Unit-normal features.  The two layouts differ -- the blocked one rounds (fp16) or stores (fp32) every cell, the direct one
    never does, and the summation orders differ -- so each is held to the float64 reference by its own derived bound; their
    difference is then inside the sum of the two bounds."""
    from streamflow_amd.corr import CorrBlock
    ref = dc.reference(case_id, "noise", cc.CROSS_AMP)
    case, F = ref["case"], ref["F"]
    assert case["pairs"] == 1
    B, h, w, Dn = case["B"], case["h"], case["w"], case["D"]
    f1 = torch.from_numpy(F[:, 0].reshape(B, Dn, h, w).copy()).to(dev)
    f2 = torch.from_numpy(F[:, 1].reshape(B, Dn, h, w).copy()).to(dev)
    xy = torch.from_numpy(ref["xy"].reshape(B, 2, h, w).copy()).to(dev)
    direct = CorrBlock(f1, f2, dtype=dtype, layout="direct")
    blocked = CorrBlock(f1, f2, dtype=dtype, layout="blocked")
    od = direct(xy).cpu().numpy().reshape(B, 324, h * w).astype(np.float64)
    ob = blocked(xy).cpu().numpy().reshape(B, 324, h * w).astype(np.float64)
    K = cc.klass("b16", Dn, 1, False) if k == "f16" else cc.klass("x3")
    for b in range(B):
        Bm, exact = cc.build_bound(F[b, 0], F[b, 1], h, w, K)                    # per STORED cell, its factor 2 included
        _, asum, _ = cc.lookup(exact, ref["xy"][b])
        wsum, usum, _ = cc.lookup(Bm, ref["xy"][b])
        bound_b = wsum + cc.lookup_bound(asum + usum)
        rd = np.abs(od[b] - ref["out"][b]) / ref["bound"][k][b]
        rb = np.abs(ob[b] - ref["out"][b]) / bound_b
        print(f"CorrBlock {case_id} {k} image {b}: direct err / bound {rd.max():.3f}, blocked err / bound {rb.max():.3f}, "
              f"max |direct - blocked| {np.abs(od[b] - ob[b]).max():.3e}")
        assert rd.max() <= 1.0 and rb.max() <= 1.0
        assert (od[b][ref["dead"][b]] == 0).all() and (ob[b][ref["dead"][b]] == 0).all()
    pyr_d, pyr_b = direct.corr_pyramid, blocked.corr_pyramid
    assert [tuple(p.shape) for p in pyr_d] == [(B * h * w, 1, h >> l, w >> l) for l in range(4)] == [tuple(p.shape) for p in pyr_b]
    for l in range(4):
        ex = np.concatenate([cc.pyramid(F[b, 0], F[b, 1], h, w)[l] for b in range(B)])
        assert np.abs(pyr_d[l].cpu().numpy().reshape(ex.shape) - ex).max() <= 1e-5 * max(1.0, np.abs(ex).max())
    assert direct.vol is None and direct.direct_ws is not None


# ---- the public surface ----------------------------------------------------------------------------------------------------------
def _state(Tn, seed):
    from streamflow_amd import synthetic as syn
    sd = dict(syn.make_params(seed, Tn))
    sd.update({"fnet." + k: v for k, v in syn.make_twins_params(seed + 1).items()})
    sd.update({"cnet." + k: v for k, v in syn.make_twins_params(seed + 2).items()})
    return sd


@pytest.fixture()
def engines(monkeypatch):
    """Every HotPathEngine the model layer builds while the test runs."""
    from streamflow_amd import model
    made = []

    class Spy(model.HotPathEngine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(model, "HotPathEngine", Spy)
    return made


def test_model_args_and_evaluate_command_line(tmp_path, dev, engines, capsys):
    """SKFlow_MF8 with args.corr = "direct" against args.corr = None on one frame triple, then `evaluate --corr direct` against
    `--corr volume` on the synthetic Sintel tree of tests/test_gpu_evaluate.py (one scene): the reports agree within the contract of
    the preset (EPE 1e-3, rates 5e-3) and the engines behind them ran the route that was asked for."""
    from streamflow_amd import evaluate, flow_io
    from streamflow_amd.model import SKFlow_MF8, default_args
    from tests.test_gpu_evaluate import _smooth_frames
    H, W, iters = 124, 188, 3
    rng = np.random.default_rng(3)
    sd = _state(T, 31)
    frames = [torch.from_numpy(f).permute(2, 0, 1)[None].float().to(dev) for f in _smooth_frames(rng, T, 128, 192)]
    flows = {}
    for corr in (None, "volume", "direct"):
        m = SKFlow_MF8(default_args(T=T, corr=corr)).to(dev)
        m.load_state_dict(sd, strict=True)
        flows[corr] = [u.clone() for u in m(frames, iters=iters, test_mode=True)]
        assert m._engine.options.corr_direct == (corr == "direct")
        assert all(pl.corr_direct == (corr == "direct") for pl in m._engine._plans.values())
    _assert_same(flows["volume"], flows[None], "args.corr = 'volume' vs None")
    for a, b in zip(flows["direct"], flows[None]):
        e = float((a - b).pow(2).sum(1).sqrt().mean())
        print(f"model: direct vs volume EPE {e:.3e}")
        assert e <= 1e-3
    with pytest.raises(RuntimeError, match="args.corr"):
        SKFlow_MF8(default_args(T=T, corr="rows")).to(dev)(frames, iters=1, test_mode=True)
    # the command line
    for dstype in ("clean", "final"):
        os.makedirs(tmp_path / "training" / dstype / "cave_9")
        for i, img in enumerate(_smooth_frames(rng, 4, H, W)):
            flow_io.write_png(str(tmp_path / "training" / dstype / "cave_9" / f"frame_{i + 1:04d}.png"), img)
    os.makedirs(tmp_path / "training" / "flow" / "cave_9")
    for i in range(3):
        flow_io.write_flo(str(tmp_path / "training" / "flow" / "cave_9" / f"frame_{i + 1:04d}.flo"), rng.normal(0, 3, size=(H, W, 2)).astype(np.float32))
    ckpt = str(tmp_path / "ckpt.pth")
    torch.save({"model": {"module." + k: v for k, v in sd.items()}}, ckpt)
    report = {}
    for corr in ("volume", "direct"):
        del engines[:]
        capsys.readouterr()
        assert evaluate.main(["--dataset", "sintel", "--ckpt", ckpt, "--root", str(tmp_path), "--T", str(T), "--iters", str(iters),
                              "--clips-per-step", "2", "--corr", corr]) == 0
        out = capsys.readouterr().out
        assert len(engines) == 1 and engines[0].options.corr_direct == (corr == "direct")
        assert engines[0]._plans and all(pl.corr_direct == (corr == "direct") for pl in engines[0]._plans.values())
        report[corr] = {ln.split(")")[0].split("(")[1]: [float(v.split(":")[1]) for v in ln.split(")")[1].split(",")]
                        for ln in out.splitlines() if ln.startswith("Validation (")}
    assert set(report["direct"]) == {"clean", "final"} == set(report["volume"])
    for ds in ("clean", "final"):
        d, v = report["direct"][ds], report["volume"][ds]
        print(ds, d, v)
        assert abs(d[0] - v[0]) <= 1e-3 and all(abs(x - y) <= 5e-3 for x, y in zip(d[1:], v[1:]))


def test_demo_command_line(tmp_path, dev, engines):
    """`demo --corr direct` against the default on six 124 x 188 frames: the .flo files agree within 1e-3 px EPE and the engine
    behind the flag kept no volume."""
    from streamflow_amd import demo, flow_io
    from tests import video_cases as vc
    H, W, n, iters = 124, 188, 6, 3
    (tmp_path / "frames").mkdir()
    for i, f in enumerate(vc.random_frames(5, n, H, W).numpy()):
        flow_io.write_png(str(tmp_path / "frames" / ("%04d.png" % i)), f)
    ckpt = str(tmp_path / "ckpt.pth")
    torch.save({"model": {"module." + k: v for k, v in _state(4, 51).items()}}, ckpt)
    for name, extra in (("volume", []), ("direct", ["--corr", "direct"])):
        del engines[:]
        assert demo.main(["--frames", str(tmp_path / "frames"), "--ckpt", ckpt, "--out", str(tmp_path / name), "--flo", str(tmp_path / name),
                          "--iters", str(iters), "--png-encode", "gpu"] + extra) == 0
        assert len(engines) == 1 and engines[0].options.corr_direct == (name == "direct")
        assert engines[0]._plans and all(pl.corr_direct == (name == "direct") and (pl.vol is None) == (name == "direct")
                                         for pl in engines[0]._plans.values())
    for i in range(n - 1):
        a = flow_io.read_flo(str(tmp_path / "direct" / ("frame_%04d.flo" % i)))
        b = flow_io.read_flo(str(tmp_path / "volume" / ("frame_%04d.flo" % i)))
        e = float(np.sqrt(((a - b) ** 2).sum(-1)).mean())
        print(f"demo pair {i}: direct vs volume EPE {e:.3e}")
        assert a.shape == b.shape == (H, W, 2) and np.isfinite(a).all() and e <= 1e-3
