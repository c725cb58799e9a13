"""What HotPathEngine._setup and ._iteration compose (streamflow_amd/engine.py), unit by unit against float64, in every arithmetic
class (-m gpu).

`_Plan.taps()` hands out fp32 clones of the plan's buffers after a forward.  Three forwards per (case, configuration): iters=0 (the
setup's taps), iters=1 with a seeded warm start of about 2 px (one iteration's taps, the mask head fused where the engine fuses it)
and the same with all_masks=True (the mask as a tensor).  Every unit is compared with the oracle's own function in float64 ON THE
GPU'S PREVIOUS TAPS, with the weights as packed -- cases, references, class emulation and bounds: tests/update_cases.py; the proof that
the bounds tell a wrong composition from the right one: tests/test_update_cases_cpu.py.  No number is fixed in advance:
    fp32, f16x3   rms <= 3 e32 and max <= 3 e32 (e32: the float32 CPU oracle of the unit against float64), and both also
                  <= 0.1 e_cls of F16X2 in every unit with a contraction (a class that silently lost precision shows);
    f16x2, f16    rms <= 2 e_cls and max <= 4 e_cls (e_cls: the float64 unit with the class's documented fp16 roundings);
    the global aggregation holds fp16 softmax weights in every split class: e_cls there, e32 under precision='fp32' only;
    flow_update and the ReLU half of the context split are compared exactly.
Also per test: every tap finite over ALL images (case F's float64 references are evaluated for its first and last clip), the plan
takes the forms update_cases.facts() says, the route of every SK block from resolve_skblock on the plan's descriptors (printed; case
F under the config-2 presets runs convf2, convc2 and conv as sf_sk_tail, case S none), the taps of the all_masks=True call bitwise
those of the fused call, and for the three presets the taps after a graph replay bitwise the eager ones.
test_fp32_engine_volume_is_the_exact_fp32_build: the precision='fp32' engine's volume is sf_corr_build_pyramid at SF_PRECISION_FP32,
bit for bit (it was built by sf_corr_build_blocked32 from split-fp16 products before this test existed).

Measured on an MI355X, worst ratio deviation / yardstick (rms, max) over the three cases, per unit and configuration (every test
prints its own, pytest -s)
(* = in units of e_cls, bound 2, 4; otherwise of e32, bound 3, 3; flow_update and the ReLU half of context: exact in every run):
    unit       fp32         fp32_class   f16x3_matrix  config2_fp16  config2_mixed  f16
    context    1.21 2.77    1.21 2.77    1.21 2.77     1.21 2.77     1.21 2.77      1.21 2.77
    qk         1.31 1.44    1.75 1.60    1.75 1.60     1.00 1.00*    1.00 1.00*     1.00 1.00*
    volume     1.49 2.02    1.96 1.97    1.96 1.97     1.00 1.00*    1.00 1.00*     1.96 1.97
    lookup     0.09 0.10    0.08 0.09    0.08 0.09     1.00 1.00*    1.00 1.00*     0.08 0.09
    convf1     1.29 1.47    3.98 6.05    3.98 6.05     1.00 1.00*    1.00 1.00*     1.00 1.00*      (f16x3: bound 7.8, 14)
    convf2     1.44 1.61    2.46 1.93    2.46 1.93     1.01 1.11*    1.00 1.00*     1.00 1.00*
    convc1     1.21 1.94    1.32 1.51    1.32 1.51     1.00 1.00*    1.02 1.00*     1.00 1.02*
    convc2     0.55 0.89    1.88 1.48    1.88 1.48     1.00 1.15*    1.00 1.24*     1.00 1.00*
    conv       1.13 1.96    2.41 2.78    2.41 2.78     1.00 1.11*    1.00 1.07*     1.00 1.04*
    temporal   1.16 1.11    1.37 1.22    1.37 1.22     1.00 1.03*    1.00 1.00*     1.00 1.00*
    gma        2.86 1.05    1.01 1.03*   1.05 1.06*    1.01 1.00*    1.01 0.99*     0.82 0.83*
    gru        1.45 2.65    1.13 1.60    1.13 1.38     1.00 1.08*    1.00 0.95*     1.00 1.10*
    flow_head  0.67 0.88    2.38 2.23    2.31 2.49     1.01 1.23*    1.02 1.47*     1.01 1.12*
    mask0      2.75 5.40    2.05 3.82    2.05 3.20     1.00 1.00*    1.00 1.00*     1.00 1.00*      (fp32, f16x3: bound 8.2, 12.9)
    mask_up    0.98 1.23    0.98 1.48    0.98 1.30     1.00 1.00*    1.00 1.00*     1.00 1.00*
    mask2      0.63 0.74    1.01 0.88    1.00 0.67     1.00 1.00*    1.00 1.00*     1.00 1.00*
    upsample   0.98 1.09    0.98 1.23    0.98 1.41     0.98 1.37     0.98 1.21      0.99 1.14
  Class separation: precision='fp32' at most 0.032 (rms) and 0.081 (max) of e_cls(F16X2), the two f16x3 configurations 0.008 and
  0.006; the limit is 0.1.  The emulation of the reduced classes is the engine's arithmetic to 2 % in rms in every unit.
  The first run of this file measured three things the 3 e32 rule does not hold, each now with a CPU model beside its margin
  (tests/update_cases.py UNIT_MARGIN, tests/test_update_cases_cpu.py::test_models_of_the_raised_margins): mask0 (one fp32 chain over
  K = 1152: the model alone is 2.73 e32 in rms -- the kernel measures 2.73), convf1 in f16x3 (split8() cuts the flow towards zero to
  2^-20; K = 2, nothing dilutes it), and the matrix form of the aggregation at odd P in f16x3 (case R): attn @ v takes the fp32
  softmax matrix as split8() pairs, the lo halves of weights of 1 / 357 are fp16 subnormals, and the pair holds a weight to 2^-16
  only -- 32 e32 in rms, 2.5e-7 absolute, a sixth of what the fp16 matrix of even P costs; its yardstick is the e_cls of that model
  (1.05 of it measured).
"""
import functools

import pytest
import torch

from tests import update_cases as uc

pytestmark = pytest.mark.gpu
DEVICE = "cuda:0"
SETUP_TAPS = ("nets0", "inps", "qk", "volume")
ITER_TAPS = ("corr", "f128", "cor256", "cat256", "mf", "mft", "mfg", "nets", "delta", "flow", "coords1", "m256", "up")
CONFIG2 = ("config2_fp16", "config2_mixed")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    return torch.device(DEVICE)


def _engine(cfg, T, graph=False):
    from streamflow_amd.engine import HotPathEngine
    return HotPathEngine(uc.params(T), device=DEVICE, T=T, use_graph=graph, **uc.engine_kwargs(cfg))


def _finite(t):
    return all(bool(torch.isfinite(x).all()) for x in (t if isinstance(t, list) else [t]))


def _pick(t, imgs):
    """Images imgs of device taps, on the CPU."""
    idx = torch.tensor(imgs, device=DEVICE)
    return {k: ([x[idx].cpu() for x in v] if isinstance(v, list) else v[idx].cpu()) for k, v in t.items()}


@functools.lru_cache(maxsize=None)
def _run(c, cfg, graph=False):
    """Three forwards -> (taps of images uc.images_of(c) on the CPU, taps of the all_masks call, engine, plan).  Every tap is checked
    finite over all images here."""
    B, T, h, w = uc.CASES[c]
    eng = _engine(cfg, T, graph)
    fm, cn, finit = uc.inputs(c)
    fm, cn, finit = fm.to(DEVICE), cn.to(DEVICE), [f.to(DEVICE) for f in finit]
    imgs = uc.images_of(c)
    def forward(**kw):                                        # use_graph: capture + replay, then a replay alone
        for _ in range(2 if graph else 1):
            eng.forward(fm, cn, **kw)

    forward(iters=0)
    pl = eng.plan(B, h, w, uc.D)
    t = pl.taps(SETUP_TAPS, cpu=False)
    forward(iters=1, flow_init=finit)
    assert eng.plan(B, h, w, uc.D) is pl and (pl.graph is not None) == graph
    t.update(pl.taps(ITER_TAPS, cpu=False))
    forward(iters=1, flow_init=finit, all_masks=True)
    tm = pl.taps(ITER_TAPS + ("mask",), cpu=False)
    for name, v in list(t.items()) + [("all_masks." + k, v) for k, v in tm.items()]:
        assert _finite(v), f"{c} {cfg}: tap {name} is not finite"
    t, tm = _pick(t, imgs), _pick(tm, imgs)
    t.update(uc.data_taps(c, imgs))
    return t, tm, eng, pl


def _routes(eng, pl):
    """{block: SkRoute} from resolve_skblock on the descriptors _iteration hands to run_skblock (the first chain's)."""
    from streamflow_amd.engine import HDIM, _sub, resolve_skblock
    cx, W, n, Pn = eng._ctx(pl), eng.W, pl.n, pl.Pn
    nch = 2 if pl.Bc % 2 == 0 else 1                          # options.split_solo = 2: half-batch chains when the clip count divides
    cnt = n // nch
    io = {"convf2": (pl.f128, pl.cat256.slice(192, 256)),
          "convc1": (_sub(pl.corr, 0, cnt), _sub(pl.cor256, 0, cnt)),
          "convc2": (_sub(pl.cor256, 0, cnt), _sub(pl.cat256.slice(0, 192), 0, cnt)),
          "conv": (_sub(pl.cat256, 0, cnt), _sub(pl.mf.slice(0, HDIM - 2), 0, cnt)),
          "gru": (_sub(pl.concat, 0, cnt), _sub(pl.nets, 0, cnt)),
          "flow_head": (_sub(pl.nets_grouped, 0, cnt // Pn), _sub(pl.delta_fh, 0, cnt // Pn))}
    return {b: resolve_skblock(getattr(W, b), X, Y, cx) for b, (X, Y) in io.items()}


def _check_plan(c, cfg, eng, pl):
    f = uc.facts(cfg, c)
    assert pl.shadows == f["hand"] and pl.koct_io == f["hand"] and pl.corr_blocked == f["lookup16"], (pl.shadows, pl.koct_io, pl.corr_blocked)
    assert (pl.lvls is not None and pl.lvls[0].dtype == torch.float16) == (f["corr16"] and not f["lookup16"])
    assert pl.corr_blocked32 == (not f["corr16"] and f["cls"] != "fp32")
    g = f["gma"]
    assert pl.gma.fused == (g["form"] == "flash") and (pl.gma.fused or pl.gma.form == "matrix")
    assert (pl.attn16 is not None) == (g["form"] == "matrix" and f["cls"] != "fp32" and pl.P % 2 == 0)     # (the matrix kept in fp16)
    if pl.gma.fused:
        assert eng.flash_qk_products == (1 if g["q16"] else 3)
    routes = _routes(eng, pl)
    for b, r in routes.items():
        print(f"route {c} {cfg} {b}: front {r.front} back {r.back} fold {r.fold} x2 {r.x2} x3 {r.x3} x4 {r.x4} hid1 {r.hid1} hid2 {r.hid2}")
        assert r.fold == f["hand"] and (r.x2 == "f16") == f["hand"] and (r.x3 == "f16") == f["hand"], (b, r)
    tails = {b for b, r in routes.items() if r.back == "tail"}
    if c == "F" and cfg in CONFIG2:
        assert uc.fills(c) and {"convf2", "convc2", "conv"} <= tails, tails
    if c == "S":
        assert not uc.fills(c) and not tails, tails
    return routes


def _check_units(c, cfg, t, tm):
    """Every unit of one run against its bound; all failures are reported together."""
    f, Pn = uc.facts(cfg, c), uc.CASES[c][1] - 1
    bad = []
    for u in uc.UNITS:
        src = tm if u in uc.MASK_UNITS else t
        x = uc.unit_inputs(u, dict(t, **{k: tm[k] for k in ("mask", "flow")}) if u in uc.MASK_UNITS else t)
        if u in uc.EXACT_UNITS:
            want = uc.run_unit(u, {k: v.float() for k, v in x.items()}, None, Pn)
            for name in uc.OUTPUTS[u]:
                same = torch.equal(uc.tap_of(src, name), want[name])
                print(f"update {c} {cfg} {u} {name}: exact {same}")
                if not same:
                    bad.append(f"{u} {name}: not the fp32 result of the oracle's unit, max |diff| {uc.dev(uc.tap_of(src, name), want[name])[1]:.3e}")
            continue
        sep_wanted = not f["reduced"] and u not in uc.NO_GEMM and uc.yard_kind(u, f) == "e32"
        y = uc.yardsticks(u, x, cfg, c, separation=sep_wanted)
        kind = uc.yard_kind(u, f)
        for name in uc.OUTPUTS[u]:
            got, ref = uc.tap_of(src, name), y["ref"][name]
            if name == "inps":                                # the ReLU half rounds nothing
                same = torch.equal(got, uc.run_unit(u, {k: v.float() for k, v in x.items()}, None, Pn)[name])
                print(f"update {c} {cfg} {u} {name}: exact {same}")
                if not same:
                    bad.append(f"{u} {name}: not relu(cnets) exactly")
                continue
            d = uc.dev_taps({name: got}, {name: ref})[name]
            yard = y["e_cls"][name] if kind == "e_cls" else y["e32"][name]
            b = uc.bound(u, f, y["e32"][name], y["e_cls"][name])
            line = (f"update {c} {cfg} {f['cls']} {u} {name}: rms {d[0]:.3e} = {d[0] / yard[0]:.2f} x {kind} (bound {b[0] / yard[0]:.1f}), "
                    f"max {d[1]:.3e} = {d[1] / yard[1]:.2f} x (bound {b[1] / yard[1]:.1f})")
            if sep_wanted:
                sep = y["sep"][name]
                line += f"; of e_cls(f16x2) {d[0] / sep[0]:.4f} {d[1] / sep[1]:.4f}"
                if d[0] > uc.SEPARATION * sep[0] or d[1] > uc.SEPARATION * sep[1]:
                    bad.append("CLASS " + line)
            print(line)
            if not (d[0] <= b[0] and d[1] <= b[1]):
                bad.append(line)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cfg", uc.CONFIGS)
@pytest.mark.parametrize("c", tuple(uc.CASES))
def test_units_vs_float64(dev, c, cfg):
    t, tm, eng, pl = _run(c, cfg)
    B, T, h, w = uc.CASES[c]
    n = len(uc.images_of(c))
    assert t["corr"].shape == (n, 324, h, w) and t["mf"].shape == (n, 126, h, w) and t["up"].shape == (n, 2, 8 * h, 8 * w)
    assert [tuple(v.shape) for v in t["volume"]] == [(n, h * w, h >> l, w >> l) for l in range(4)] and tm["mask"].shape == (n, 576, h, w)
    _check_plan(c, cfg, eng, pl)
    # the mask as a tensor of its own changes nothing before it: every other tap of the all_masks call is the fused call's
    for name in ITER_TAPS:
        if name != "up":
            assert torch.equal(tm[name], t[name]), f"{name} differs between all_masks=True and the default call"
    _check_units(c, cfg, t, tm)


@pytest.mark.parametrize("cfg", uc.PRESETS)
@pytest.mark.parametrize("c", tuple(uc.CASES))
def test_taps_after_a_graph_replay_are_the_eager_taps(dev, c, cfg):
    """use_graph=True: each of the three calls captured and replayed, then replayed alone; the taps are bitwise the eager ones."""
    t, tm, _, _ = _run(c, cfg)
    g, gm, _, _ = _run(c, cfg, True)
    for name in SETUP_TAPS + ITER_TAPS:
        a, b = g[name], t[name]
        same = all(torch.equal(x, y) for x, y in zip(a, b)) if isinstance(a, list) else torch.equal(a, b)
        assert same, f"{c} {cfg}: tap {name} after a graph replay differs from the eager tap"
    assert torch.equal(gm["mask"], tm["mask"]) and torch.equal(gm["up"], tm["up"])


@pytest.mark.parametrize("c", ("S", "R"))
def test_fp32_engine_volume_is_the_exact_fp32_build(dev, c):
    """precision='fp32' promises exact fp32 MFMA: level_maps(l) of its plan are sf_corr_build_pyramid at SF_PRECISION_FP32 on the same
    fmaps, bit for bit, l = 0 .. 3 -- at 16 x 24 (dense rows would straddle cache lines: pitched) and at 17 x 21."""
    from streamflow_amd import ops
    B, T, h, w = uc.CASES[c]
    Pn, P = T - 1, h * w
    eng = _engine("fp32", T)
    fm, cn, _ = uc.inputs(c)
    fm, cn = fm.to(DEVICE), cn.to(DEVICE)
    eng.forward(fm, cn, iters=0)
    pl = eng.plan(B, h, w, uc.D)
    strides = [B * P * (h >> l) * (w >> l) for l in range(4)]
    lv = [torch.empty(Pn * s, dtype=torch.float32, device=DEVICE) for s in strides]
    ws = torch.empty(max(ops.corr_build_ws_bytes(B, Pn, uc.D, h, w), 16), dtype=torch.uint8, device=DEVICE)
    ops.corr_build(fm.data_ptr(), fm.data_ptr() + 4 * uc.D * P, T * uc.D * P, uc.D * P, lv, strides, B, Pn, uc.D, h, w, ws=ws,
                   cx=ops.Ctx(precision=ops.PRECISION_FP32))
    torch.cuda.synchronize()
    for l in range(4):
        want = lv[l].view(Pn, B * P, h >> l, w >> l)
        got = pl.level_maps(l)
        assert got.shape == want.shape and torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32)), f"level {l}"
    assert not pl.corr_blocked32 and pl.lvls is not None and pl.vol is None          # ... as the row-major maps themselves
    # ... and it is NOT what the split-fp16 build gives (the comparison can see the difference)
    other = _engine("f16x3_matrix", T)
    other.forward(fm, cn, iters=0)
    assert not torch.equal(other.plan(B, h, w, uc.D).level_maps(0), pl.level_maps(0))
