"""The layer that composes the kernels -- HotPathEngine, its plans and graphs, Twins_CSC.forward, SKFlow_MF8's caches and the ops
wrappers that allocate their own scratch -- must compute a function of weights, inputs and options ONLY:

  A  what an allocation held when it was handed out does not matter (tests/poison.poisoned: zeros, NaN, a huge finite value);
  B  what the previous forward left in a plan's buffers does not matter (tests/poison.poison_plan between two forwards / replays);
  C  the calls an engine has served before do not matter (other inputs, a warm start, other iteration counts, other batch sizes and
     grids, evicted and kept plans), and what it returned for one grid survives a forward at another;
  D  weights changed after the first forward rebuild the engine and the encoder packs; unchanged weights rebuild nothing;
  E  the same for the wrappers with per-call scratch (flow_to_image, flow_score(_batch), png_encode / png_unfilter, the video
     kernels, forward_interpolate, CorrBlock).

Every comparison is BITWISE (the engine kernels use no floating-point atomics; eager == capture == replay, flash == stored and the
chain schedules are asserted bitwise elsewhere in the suite), and every flow is also checked finite.  Shapes are the smallest at which
every path still runs: T = 3, 2-3 iterations, the grid 16 x 24 with two clips (P % 4 == 0: fp16 hand-over and shadows on, half-batch
chains), 17 x 21 with one clip (P % 4 != 0: hand-over formats off, fp32 planes, pitched volume rows, no fp16 attention matrix) and
24 x 40 for the shape changes; the model-level tests run frames of 128 x 192 through random Twins_CSC weights.

Integer reads of unwritten memory were excluded by reading before the first run (an unwritten index would be an address): the
workspaces of sf_png_encode hold scanlines and table records written by its first three kernels before the fourth reads them, the
rad_max slot of sf_flow_to_image and the output slots of sf_png_encode are cleared by the entry points, the scoring and
correlation-build workspaces hold floating-point partials / packed features only, and the header of the fused GMA workspace is
compared, never used as an address."""
from dataclasses import replace

import numpy as np
import pytest
import torch

from tests import eval_cases, png_cases, png_encode_cases, poison, score_cases, video_cases, viz_cases

pytestmark = pytest.mark.gpu

T, ITERS, D = 3, 3, 256
GRID_A, GRID_B, GRID_C = (2, 16, 24), (1, 17, 21), (1, 24, 40)          # (clips, h, w)
PRESETS = ("fp32_class", "config2_fp16", "config2_mixed")


def _configs():
    from streamflow_amd import presets
    from streamflow_amd.engine import EngineOptions
    cfg = {p: (lambda p=p: presets.engine_kwargs(p)) for p in PRESETS}
    cfg["fp32"] = lambda: dict(precision="fp32")                          # materialised fp32 attention matrix, no split precision
    cfg["f16x3_matrix"] = lambda: dict(precision="f16x3", gma_mode="matrix")          # attn16 and the split-K `part` slabs
    cfg["f16x3_chunked"] = lambda: dict(precision="f16x3", gma_mode="matrix", options=EngineOptions(attn_chunk_rows=100))
    cfg["config2_stored"] = lambda: dict(precision="f16x2", corr_dtype="f16", gma_mode="stored", flash_qk_products=1)
    # two more ways to the k-octet copy of the correlation features (324 rows: the one shadow whose last octet is partial): row-major
    # fp16 volumes, whose lookup writes the copy itself, and fp32 volumes under fp16 activations, where a pack pass follows the lookup
    cfg["config2_rows"] = lambda: dict(presets.engine_kwargs("config2_fp16"), options=EngineOptions(corr_blocked=False))
    cfg["f16x2_f32vol"] = lambda: dict(precision="f16x2", corr_dtype="f32")
    return cfg


OTHERS = ("fp32", "f16x3_matrix", "f16x3_chunked", "config2_stored", "config2_rows", "f16x2_f32vol")
ALL = PRESETS + OTHERS
# call-history tests: the bench preset where everything is on, the library default where the hand-over formats are off
HISTORY = [("config2_mixed", GRID_A), ("fp32_class", GRID_B), ("config2_fp16", GRID_B), ("fp32_class", GRID_A), ("f16x3_matrix", GRID_A),
           ("fp32", GRID_B)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


_CACHE = {}


def _params():
    from streamflow_amd import synthetic as syn
    if "params" not in _CACHE:
        _CACHE["params"] = syn.make_params(3, T)
    return _CACHE["params"]


def features(dev, grid, seed=1):
    """(fmaps, cnets) on the device for (clips, h, w), made once per (grid, seed)."""
    from streamflow_amd import synthetic as syn
    key = ("x", grid, seed)
    if key not in _CACHE:
        B, h, w = grid
        f, c = syn.make_features(100 * seed + h, B, T, h, w)
        _CACHE[key] = (f.to(dev), c.to(dev))
    return _CACHE[key]


def warm_start(dev, grid):
    from streamflow_amd import synthetic as syn
    B, h, w = grid
    return [syn.randn(77, f"finit{i}", (B, 2, h, w), 2.0).to(dev) for i in range(T - 1)]


def engine(dev, cfg, graph=False, **opt):
    from streamflow_amd.engine import EngineOptions, HotPathEngine
    kw = dict(_configs()[cfg]())
    options = kw.pop("options", None) or EngineOptions()
    return HotPathEngine(_params(), device=dev, T=T, use_graph=graph, options=replace(options, **opt), **kw)


def run(eng, x, iters=ITERS, **kw):
    """One forward -> copies of the T - 1 upsampled and the T - 1 low-resolution flows."""
    ups, low = eng.forward(x[0], x[1], iters=iters, **kw)
    out = [t.clone() for t in list(ups) + list(low)]
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(torch.uint8)


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i)
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), f"{what}: non-finite values in flow {i}"
        if not torch.equal(bits(a), bits(b)):
            d = (a.double() - b.double()).abs()
            raise AssertionError(f"{what}: flow {i}: {int((bits(a) != bits(b)).sum())} of {a.numel()} values differ, max |diff| {float(d.max()):.3e}")


def fresh(dev, cfg, graph, grid, seed=1, iters=ITERS, all_masks=False, warm=False, every=False):
    """What a NEW engine returns for this call, computed once and shared (every: forward_all_iterations)."""
    key = ("fresh", cfg, graph, grid, seed, iters, all_masks, warm, every)
    if key not in _CACHE:
        eng = engine(dev, cfg, graph and not every)
        x = features(dev, grid, seed)
        finit = warm_start(dev, grid) if warm else None
        if every:
            _CACHE[key] = flat(eng.forward_all_iterations(x[0], x[1], iters=iters, flow_init=finit))
        else:
            _CACHE[key] = run(eng, x, iters, all_masks=all_masks, flow_init=finit)
    return _CACHE[key]


def flat(preds):
    out = [t.clone() for per_pair in preds for t in per_pair]
    torch.cuda.synchronize()
    return out


def test_the_poison_reaches_device_memory(dev):
    """The helper on the device: every byte of a new tensor, nothing while a stream capture runs (the capture still works), and
    poison_plan's fill of a slice stays inside it."""
    for b in poison.BYTES:
        with poison.poisoned(b):
            for dt in (torch.float16, torch.float32, torch.uint8, torch.int64):
                t = torch.empty(5, 37, dtype=dt, device=dev)
                assert bool((t.view(-1).view(torch.uint8) == b).all())
            assert bool((torch.empty_like(torch.ones(3, 5, device=dev)).view(torch.uint8) == b).all())
            assert not torch.zeros(64, device=dev).any()
    with poison.poisoned(0xFF):
        assert bool(torch.isnan(torch.empty(8, device=dev)).all())
        src = torch.arange(64, dtype=torch.float32, device=dev)
        g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(g, stream=s):
            out = torch.empty(64, device=dev)
            out.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, src)
    buf = torch.zeros(256, dtype=torch.uint8, device=dev)
    poison.fill_view(buf[64:128].view(torch.float32), 0x7B)
    assert bool((buf[64:128] == 0x7B).all()) and not buf[:64].any() and not buf[128:].any()


# ---- the ground everything below stands on ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", [GRID_A, GRID_B], ids=str)
@pytest.mark.parametrize("cfg", OTHERS)
def test_two_fresh_engines_agree_bitwise(dev, cfg, grid):
    """The presets' run-to-run equality is asserted elsewhere (eager == capture == replay, two threads); here the configurations no
    preset selects -- the materialised matrix in fp32 and in fp16 with its split-K slabs, the chunked recompute, the stored weights."""
    x = features(dev, grid)
    assert_same(run(engine(dev, cfg), x), fresh(dev, cfg, False, grid), f"{cfg} {grid}: two fresh engines")


def test_configurations_take_the_paths_they_are_named_for(dev):
    P_a, P_b = GRID_A[1] * GRID_A[2], GRID_B[1] * GRID_B[2]
    assert P_a % 4 == 0 and P_b % 4 != 0 and P_b % 2 != 0
    pl = {(c, g): engine(dev, c).plan(g[0], g[1], g[2], D) for c in ALL for g in (GRID_A, GRID_B)}
    for c in PRESETS + ("config2_stored",):
        assert pl[c, GRID_A].flash and pl[c, GRID_B].flash
    for c in ("config2_fp16", "config2_mixed", "config2_stored"):
        assert pl[c, GRID_A].shadows and pl[c, GRID_A].corr_blocked and pl[c, GRID_A].koct_io
        assert not pl[c, GRID_B].shadows and not pl[c, GRID_B].corr_blocked and pl[c, GRID_B].lvls is not None
    assert pl["fp32_class", GRID_A].corr_blocked32 and pl["fp32_class", GRID_A].pbuf is not None       # split logits: stored
    assert pl["config2_stored", GRID_A].pbuf is not None and pl["config2_fp16", GRID_A].pbuf is None
    for c in ("fp32", "f16x3_matrix"):
        assert not pl[c, GRID_A].flash and pl[c, GRID_A].attn_rows == P_a and pl[c, GRID_B].attn_rows == P_b
    assert not pl["fp32", GRID_A].corr_blocked32 and pl["fp32", GRID_A].lvls is not None       # exact fp32: the row-major build
    assert pl["fp32", GRID_A].attn16 is None and pl["f16x3_matrix", GRID_A].attn16 is not None and pl["f16x3_matrix", GRID_B].attn16 is None
    assert pl["config2_rows", GRID_A].shadows and not pl["config2_rows", GRID_A].corr_blocked and pl["config2_rows", GRID_A].lvls is not None
    assert pl["config2_rows", GRID_A].corr.shadow is not None
    assert pl["f16x2_f32vol", GRID_A].shadows and pl["f16x2_f32vol", GRID_A].corr_blocked32 and not pl["f16x2_f32vol", GRID_A].flash
    assert pl["f16x2_f32vol", GRID_A].corr.shadow is not None and not pl["f16x2_f32vol", GRID_B].shadows
    for g, P in ((GRID_A, P_a), (GRID_B, P_b)):
        assert not pl["f16x3_chunked", g].flash and pl["f16x3_chunked", g].attn_rows == 100 and P % 100 != 0


CORR_ENTRY_POINTS = {"direct": ["sf_corr_direct_pack", "sf_corr_direct_lookup"],
                     "blocked16": ["sf_corr_build_blocked", "sf_corr_lookup_blocked"],
                     "blocked32": ["sf_corr_build_blocked32", "sf_corr_lookup_blocked32"],
                     "rows": ["sf_corr_build_pyramid_pitched", "sf_corr_lookup_pitched"]}
# (form, configuration, options off their defaults, the CorrBlock of that form, grid): every form at both grids where it is reachable --
# blocked fp16 volumes need the fp16 hand-over, so only GRID_A has them; at GRID_B the same configuration keeps row-major fp16 maps
CORR_CASES = [("direct", "config2_fp16", {"corr_direct": True}, (torch.float16, "direct"), GRID_A),
              ("direct", "config2_fp16", {"corr_direct": True}, (torch.float16, "direct"), GRID_B),
              ("direct", "fp32_class", {"corr_direct": True}, (torch.float32, "direct"), GRID_B),
              ("blocked16", "config2_fp16", {}, (torch.float16, "blocked"), GRID_A),
              ("blocked32", "fp32_class", {}, (torch.float32, "blocked"), GRID_A),
              ("blocked32", "fp32_class", {}, (torch.float32, "blocked"), GRID_B),
              ("rows", "fp32", {}, (torch.float32, "rows"), GRID_A),
              ("rows", "fp32", {}, (torch.float32, "rows"), GRID_B),
              ("rows", "config2_fp16", {}, (torch.float16, "rows"), GRID_B)]


@pytest.mark.parametrize("form,cfg,opt,block,grid", CORR_CASES, ids=[f"{f}-{c}-{g}" for f, c, _, _, g in CORR_CASES])
def test_engine_and_corr_block_issue_the_correlation_calls_of_one_form(dev, monkeypatch, form, cfg, opt, block, grid):
    """One eager forward(iters=1): of the library's sf_corr_* entry points that launch (all but the host-only sizing functions) exactly
    the build and the lookup of the form the configuration is named for are called, once each, in that order -- and a CorrBlock of
    the matching layout and dtype on one pair (a corr.CorrStore of that form) calls the same two."""
    from streamflow_amd import _lib
    from streamflow_amd.corr import CorrBlock
    eng, x = engine(dev, cfg, **opt), features(dev, grid)
    lib, calls = _lib.load(), []

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            return lambda *a: (calls.append(name), fn(*a))[1]

    launches = lambda: [c for c in calls if c.startswith("sf_corr_") and not c.endswith(("_bytes", "_geometry"))]
    monkeypatch.setattr(_lib, "load", lambda: Recorder())
    ups, low = eng.forward(x[0], x[1], iters=1)
    torch.cuda.synchronize()
    assert launches() == CORR_ENTRY_POINTS[form]
    assert "sf_gemm" in calls and all(bool(torch.isfinite(u).all()) for u in ups)          # (the recorder saw the rest of the forward)
    del calls[:]
    B, h, w = grid
    coords = torch.stack(torch.meshgrid(torch.arange(w, device=dev), torch.arange(h, device=dev), indexing="xy")).float()
    blk = CorrBlock(x[0][:, 0], x[0][:, 1], dtype=block[0], layout=block[1])
    out = blk(coords[None].expand(B, 2, h, w) + 1.5)
    torch.cuda.synchronize()
    assert blk.store.plan.form == form and launches() == CORR_ENTRY_POINTS[form]
    assert out.shape == (B, 324, h, w) and bool(torch.isfinite(out).all())
    # the same store handing over fp16 k-octets only (the engine's hand-over: fp16 cells, P % 4 == 0): the wrapper's call, bit for bit
    if blk.store.plan.f16 and form != "rows" and (h * w) % 4 == 0:
        from streamflow_amd import ops
        from streamflow_amd.corr import CorrPlan, CorrStore
        f1, f2 = blk._keep
        st = CorrStore(CorrPlan(form, True, koct_out=True), B, 1, D, h, w, dev)
        st.build(f1.data_ptr(), f2.data_ptr(), D * h * w, 0)
        c = ops.Planes.of((coords[None].expand(B, 2, h, w) + 1.5).contiguous())
        got, want = (ops.new_shadow(ops.Planes.of(out), dev) for _ in range(2))
        del calls[:]
        st.lookup(c, got)
        if form == "direct":
            ops.corr_direct_lookup(st.ws, c, None, want, B, 1, D, h, w, ops.PRECISION_F16)
        else:
            ops.corr_lookup_blocked(st.vol, c, None, want, B, 1)
        torch.cuda.synchronize()
        assert launches() == 2 * CORR_ENTRY_POINTS[form][1:]
        assert torch.equal(got.base.view(torch.int32), want.base.view(torch.int32))
        assert bool(torch.isfinite(got.tensor().float()).all())


# ---- A. allocation contents do not matter ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", [GRID_A, GRID_B], ids=str)
@pytest.mark.parametrize("cfg,graph", [(c, False) for c in ALL] + [(c, True) for c in PRESETS])
def test_allocation_contents_do_not_matter(dev, cfg, graph, grid):
    """Engine, packs, plan and (graph) staging buffers built and one forward run inside poisoned(b): the flows of the three bytes
    are finite and bitwise equal."""
    x = features(dev, grid)
    outs = {}
    for b in poison.BYTES:
        with poison.poisoned(b):
            outs[b] = run(engine(dev, cfg, graph), x)
    for b in poison.BYTES[1:]:
        assert_same(outs[b], outs[0x00], f"{cfg} graph={graph} {grid}: allocations filled with {b:#04x} vs zeros")


# (configuration, SF_ENGINE_OPTS): the scheduling and hand-over switches one at a time and in the combinations that send a tensor
# through another buffer -- the unfused launches hand the 1.5 C hidden activations (486 rows at C = 324: a partial last octet)
# and x2 / x3 / x4 through scratch views of the workspace that the fused chains keep in registers
SWITCHES = [("config2_fp16", s) for s in (
    "ffn_pairs=0", "sk_tail=0", "ffn_pairs=0,sk_tail=0", "ffn_pairs=0,sk_tail=0,hidden_koct=0", "ffn_pairs=0,sk_tail=0,pw_fold=0",
    "ffn_pairs=0,sk_tail=0,x2_f16=0", "ffn_pairs=0,sk_tail=0,koct_io=0,shadow_fused=0", "hidden_f16=0", "koct_io=0", "shadow_fused=0",
    "shadows=0", "temporal_block=0", "mask_upsample=0", "project_v=0", "flash_stats=0", "gma_per_chain=0", "parallel_branches=0",
    "setup_overlap=0", "split_solo=0", "split_solo=4", "sk_tail_all=1", "head_pairs=1", "auto_split_k=0")]
SWITCHES += [("config2_mixed", s) for s in ("ffn_pairs=0,sk_tail=0", "sk_tail_all=1,head_pairs=1", "temporal_block=0,mask_upsample=0")]
SWITCHES += [("fp32_class", s) for s in ("corr_blocked32=0", "stored_auto_px=0", "temporal_block=0", "mask_upsample=0",
                                         "parallel_branches=0", "auto_split_k=0")]
SWITCHES += [("f16x3_matrix", s) for s in ("attn_k_splits=1", "attn_k_splits=4", "corr_blocked32=0")]
SWITCHES += [("fp32", "corr_blocked32=0")]


@pytest.mark.parametrize("grid", [GRID_A, GRID_B], ids=str)
@pytest.mark.parametrize("cfg,spec", SWITCHES)
def test_allocation_contents_and_used_plans_under_option_switches(dev, monkeypatch, cfg, spec, grid):
    """A and B again with one engine option (or a combination) off its default, set the way an experiment sets it -- through
    SF_ENGINE_OPTS, which the engine reads at construction.  fp32 volumes with corr_blocked32=0 are the row-major maps with pitched
    rows at both grids (24 and 21 cells are no multiple of 32)."""
    from streamflow_amd.engine import EngineOptions
    monkeypatch.setenv("SF_ENGINE_OPTS", spec)
    want = EngineOptions.from_env()
    assert want != EngineOptions()
    x = features(dev, grid)
    outs = {}
    for b in poison.BYTES:
        with poison.poisoned(b):
            eng = engine(dev, cfg)
            outs[b] = run(eng, x)
        assert eng.options == want
    for b in poison.BYTES[1:]:
        assert_same(outs[b], outs[0x00], f"{cfg} {spec} {grid}: allocations filled with {b:#04x} vs zeros")
    pl = eng.plan(grid[0], grid[1], grid[2], D)
    if "corr_blocked32=0" in spec:
        assert pl.lvls is not None and pl.corr_pitch is not None and pl.lvls[0].dtype == torch.float32
    for b in (0xFF, 0x7B):
        poison.poison_plan(pl, b)
        assert_same(run(eng, x), outs[0x00], f"{cfg} {spec} {grid}: plan buffers overwritten with {b:#04x}")


def _model_state(seed):
    from streamflow_amd import synthetic as syn
    key = ("sd", seed)
    if key not in _CACHE:
        sd = dict(syn.make_params(seed, T))
        sd.update({"fnet." + k: v for k, v in syn.make_twins_params(seed + 1).items()})
        sd.update({"cnet." + k: v for k, v in syn.make_twins_params(seed + 2).items()})
        _CACHE[key] = sd
    return _CACHE[key]


def _frames(dev):
    from streamflow_amd import synthetic as syn
    if "frames" not in _CACHE:
        _CACHE["frames"] = [(syn.randn(24, f"frame{t}", (1, 3, 128, 192)).sigmoid() * 255.0).to(dev) for t in range(T)]
    return _CACHE["frames"]


def _model(dev, preset, seed, graph=False):
    from streamflow_amd.model import SKFlow_MF8, default_args
    model = SKFlow_MF8(default_args(T=T, preset=preset, use_graph=graph)).to(dev)
    model.load_state_dict(_model_state(seed), strict=True)
    return model


def _model_run(model, dev, iters=ITERS):
    ups = model(_frames(dev), iters=iters, test_mode=True)
    pl = next(iter(model._engine._plans.values()))
    out = [u.clone() for u in ups] + [pl.flow.tensor().clone()]
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("preset", PRESETS)
def test_allocation_contents_do_not_matter_to_the_model(dev, preset):
    """Frames -> Twins_CSC fnet / cnet -> loop: the encoder's per-call intermediates (fp32 planes, fp16 k-octet planes, split-K
    scratch), its packs and the engine are all allocated inside poisoned(b)."""
    outs = {}
    for b in poison.BYTES:
        model = _model(dev, preset, 21)
        with poison.poisoned(b):
            outs[b] = _model_run(model, dev)
    for b in poison.BYTES[1:]:
        assert_same(outs[b], outs[0x00], f"model {preset}: allocations filled with {b:#04x} vs zeros")


# ---- B. a used plan does not matter ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", [GRID_A, GRID_B], ids=str)
@pytest.mark.parametrize("cfg,graph", [(c, False) for c in ALL] + [(c, True) for c in PRESETS])
def test_a_used_plan_does_not_matter(dev, cfg, graph, grid):
    """forward, destroy everything the plan holds (NaN, then a huge finite value), forward again: the same bits.  With a graph the
    buffers are destroyed between two replays of one capture."""
    x = features(dev, grid)
    eng = engine(dev, cfg, graph)
    first = run(eng, x)
    pl = eng.plan(grid[0], grid[1], grid[2], D)
    g = pl.graph
    assert (g is not None) == graph
    names = [n for n, _ in poison.plan_buffers(pl)]
    assert "ws.buf" in names and "up" in names and ("vol" in names or "lvls[0]" in names)
    for b in (0xFF, 0x7B):
        poison.poison_plan(pl, b)
        assert bool((pl.up.view(-1).view(torch.uint8) == b).all())
        assert_same(run(eng, x), first, f"{cfg} graph={graph} {grid}: plan buffers overwritten with {b:#04x}")
        assert eng.plan(grid[0], grid[1], grid[2], D) is pl and pl.graph is g


# ---- C. call history does not matter ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("cfg,grid", HISTORY, ids=str)
def test_inputs_change_between_calls(dev, cfg, grid, graph):
    """x1, x2, x1 on one engine (with a graph: three replays through the staging copy)."""
    eng = engine(dev, cfg, graph)
    r = [run(eng, features(dev, grid, s)) for s in (1, 2, 1)]
    assert_same(r[0], fresh(dev, cfg, graph, grid, 1), "first input")
    assert_same(r[1], fresh(dev, cfg, graph, grid, 2), "second input after the first")
    assert_same(r[2], r[0], "first input again")
    assert not torch.equal(r[0][0], r[1][0])
    if graph:
        assert len(eng._plans) == 1 and next(iter(eng._plans.values())).graph is not None


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("cfg,grid", HISTORY, ids=str)
def test_warm_start_then_none(dev, cfg, grid, graph):
    x, f = features(dev, grid), warm_start(dev, grid)
    eng = engine(dev, cfg, graph)
    r = [run(eng, x, flow_init=fi) for fi in (f, None, f)]
    assert_same(r[0], fresh(dev, cfg, graph, grid, warm=True), "warm start")
    assert_same(r[1], fresh(dev, cfg, graph, grid), "no warm start after one")
    assert_same(r[2], r[0], "warm start again")
    assert not torch.equal(r[0][0], r[1][0])
    assert_same(run(eng, x, flow_init=[torch.zeros_like(t) for t in f]), r[1], "a warm start of zeros")


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("cfg,grid", HISTORY, ids=str)
def test_iteration_count_and_masks_change(dev, cfg, grid, graph):
    """iters 3, 2, 3, then all_masks on and off on one plan: with a graph every change of the key recaptures."""
    x = features(dev, grid)
    eng = engine(dev, cfg, graph)
    pl = eng.plan(grid[0], grid[1], grid[2], D)
    graphs = []
    for it, masks in ((3, False), (2, False), (3, False), (3, True), (3, False)):
        assert_same(run(eng, x, it, all_masks=masks), fresh(dev, cfg, graph, grid, iters=it, all_masks=masks), f"iters={it} all_masks={masks}")
        graphs.append(pl.graph)
        assert eng.plan(grid[0], grid[1], grid[2], D) is pl
    if graph:
        assert all(a is not None and a is not b for a, b in zip(graphs, graphs[1:]))
    assert not torch.equal(fresh(dev, cfg, graph, grid, iters=2)[0], fresh(dev, cfg, graph, grid, iters=3)[0])


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("cfg,grid", HISTORY, ids=str)
def test_forward_all_iterations_beside_forward(dev, cfg, grid, graph):
    """The training-mode return runs eagerly on the plan a (graph) forward uses, before it and after it."""
    x = features(dev, grid)
    every = fresh(dev, cfg, graph, grid, iters=2, every=True)
    assert len(every) == (T - 1) * 2
    eng = engine(dev, cfg, graph)
    assert_same(run(eng, x), fresh(dev, cfg, graph, grid), "forward")
    assert_same(flat(eng.forward_all_iterations(x[0], x[1], iters=2)), every, "forward_all_iterations after forward")
    assert_same(run(eng, x), fresh(dev, cfg, graph, grid), "forward after forward_all_iterations")
    eng = engine(dev, cfg, graph)
    assert_same(flat(eng.forward_all_iterations(x[0], x[1], iters=2)), every, "forward_all_iterations first")
    assert_same(run(eng, x), fresh(dev, cfg, graph, grid), "forward after forward_all_iterations on a new engine")
    # the last prediction of the training-mode return is the test-mode flow after as many iterations
    assert_same([every[1], every[3]], fresh(dev, cfg, graph, grid, iters=2, all_masks=True)[:2], "last prediction vs forward(all_masks)")


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("cfg,grid", HISTORY, ids=str)
def test_batch_size_changes(dev, cfg, grid, graph):
    """Two clips, one, two again: the shorter last clip batch of a video."""
    _, h, w = grid
    eng = engine(dev, cfg, graph)
    for B in (2, 1, 2):
        g = (B, h, w)
        assert_same(run(eng, features(dev, g)), fresh(dev, cfg, graph, g), f"{B} clip(s)")
    assert len(eng._plans) == 2


@pytest.mark.parametrize("byte", [None, 0xFF])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("cfg", ["config2_mixed", "fp32_class"])
def test_shapes_alternate_and_plans_are_evicted(dev, cfg, graph, byte):
    """Grids A, B, A with room for one plan (A is rebuilt) and for two (A is kept, its graph too); then A, B, C with room for two:
    A goes, B stays.  Also with every allocation of the rebuilt plans filled with NaN."""
    import contextlib
    key = lambda g: (g[0], g[1], g[2], D)
    for g in (GRID_A, GRID_B, GRID_C):                                       # the references come from friendly memory
        fresh(dev, cfg, graph, g)
    with (poison.poisoned(byte) if byte is not None else contextlib.nullcontext()):
        for max_plans in (1, 2):
            eng = engine(dev, cfg, graph, max_plans=max_plans)
            seen = []
            for g in (GRID_A, GRID_B, GRID_A):
                assert_same(run(eng, features(dev, g)), fresh(dev, cfg, graph, g), f"max_plans={max_plans}: grid {g}")
                assert len(eng._plans) <= max_plans and list(eng._plans)[-1] == key(g)
                seen.append((eng._plans[key(g)], eng._plans[key(g)].graph))            # (kept alive: identities stay distinct)
            if max_plans == 1:
                assert seen[2][0] is not seen[0][0] and list(eng._plans) == [key(GRID_A)]
            else:
                assert seen[2][0] is seen[0][0] and seen[2][1] is seen[0][1] and list(eng._plans) == [key(GRID_B), key(GRID_A)]
            assert (seen[0][1] is not None) == graph
        eng = engine(dev, cfg, graph, max_plans=2)
        plans = {}
        for g in (GRID_A, GRID_B, GRID_C):
            assert_same(run(eng, features(dev, g)), fresh(dev, cfg, graph, g), f"A, B, C: grid {g}")
            assert len(eng._plans) <= 2
            plans[g] = eng._plans[key(g)]
        assert list(eng._plans) == [key(GRID_B), key(GRID_C)] and eng._plans[key(GRID_B)] is plans[GRID_B]


@pytest.mark.parametrize("max_plans", [2, 1])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("cfg", ["config2_mixed", "fp32_class"])
def test_returned_views_survive_another_grid(dev, cfg, graph, max_plans):
    """forward returns views into the plan's buffers, 'valid until the next forward of the same shape': a forward at another grid
    leaves them alone, with the plan kept and with the plan evicted."""
    eng = engine(dev, cfg, graph, max_plans=max_plans)
    xa, xb = features(dev, GRID_A), features(dev, GRID_B)
    ups, low = eng.forward(xa[0], xa[1], iters=ITERS)
    views = list(ups) + list(low)
    torch.cuda.synchronize()
    assert_same(views, fresh(dev, cfg, graph, GRID_A), "grid A")
    assert_same(run(eng, xb), fresh(dev, cfg, graph, GRID_B), "grid B")
    assert ((GRID_A[0], GRID_A[1], GRID_A[2], D) in eng._plans) == (max_plans == 2)
    assert_same(views, fresh(dev, cfg, graph, GRID_A), "grid A's returned tensors after a forward at grid B")


# ---- D. weight caches ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("preset", ["fp32_class", "config2_fp16"])
def test_weights_changed_after_the_first_forward(dev, preset, graph):
    model = _model(dev, preset, 21, graph)
    r1 = _model_run(model, dev)
    eng, packs = model._engine, (model.fnet._pack, model.cnet._pack)
    assert eng is not None and packs[0] is not None and packs[1] is not None and packs[0] is not packs[1]
    assert_same(_model_run(model, dev), r1, "second forward, weights unchanged")
    assert model._engine is eng and model.fnet._pack is packs[0] and model.cnet._pack is packs[1]           # nothing rebuilt
    model.load_state_dict(_model_state(31), strict=True)                                                    # hot path AND encoders
    r2 = _model_run(model, dev)
    assert model._engine is not eng and model.fnet._pack is not packs[0] and model.cnet._pack is not packs[1]
    want = ("model", preset, graph, 31)
    if want not in _CACHE:
        _CACHE[want] = _model_run(_model(dev, preset, 31, graph), dev)
    assert_same(r2, _CACHE[want], "after load_state_dict vs a new model with those weights")
    assert not torch.equal(r1[0], r2[0])
    eng2 = model._engine
    assert_same(_model_run(model, dev), r2, "again, weights unchanged")
    assert model._engine is eng2
    # only the encoders' weights change: the engine stays, the packs go
    enc_only = {k: v for k, v in _model_state(21).items() if k.startswith(("fnet.", "cnet."))}
    model.load_state_dict(enc_only, strict=False)
    pk = model.fnet._pack
    r3 = _model_run(model, dev)
    assert model._engine is eng2 and model.fnet._pack is not pk
    assert not torch.equal(r3[0], r2[0])


# ---- E. wrappers that allocate their own scratch ---------------------------------------------------------------------------------

def _both(fn):
    """fn() inside poisoned(0xFF) and inside poisoned(0x00) -> the two results (lists of host arrays)."""
    out = []
    for b in (0xFF, 0x00):
        with poison.poisoned(b):
            r = fn()
            torch.cuda.synchronize()
        out.append([t.cpu().numpy() for t in r])
    return out


def _assert_bytes(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: output {i} differs"


def test_flow_to_image_scratch(dev):
    from streamflow_amd import ops
    flows = torch.from_numpy(viz_cases.gaussian_fields(3, 37, 53, [3e-3, 40.0, 1.5], seed=5)).to(dev)
    a, b = _both(lambda: ops.flow_to_image(flows, return_rad_max=True))
    _assert_bytes(a, b, "flow_to_image")
    assert np.isfinite(a[1]).all() and (a[1] > 0).all() and a[0].any()
    for i in range(3):
        assert a[1][i].tobytes() == viz_cases.rad_max_np(flows[i].permute(1, 2, 0).cpu().numpy()).tobytes()


def test_flow_score_scratch(dev):
    from streamflow_amd import ops, scoring
    rng = np.random.default_rng(8)
    h, w, step = 37, 53, 2
    gt = torch.from_numpy(score_cases.random_gt(rng, h, w, step, 0.05)).to(dev)
    pred = torch.from_numpy(score_cases.subsample(gt.cpu().numpy(), step, h, w) + rng.standard_normal((2, h, w)).astype(np.float32)).to(dev)
    pred = torch.nan_to_num(pred, nan=1.0)

    def call():
        acc = torch.zeros(scoring.LEN, dtype=torch.float64, device=dev)
        ops.flow_score(pred, gt, acc, step)
        return [acc]

    a, b = _both(call)
    _assert_bytes(a, b, "flow_score")
    # (the ground truth has NaN pixels: the sum over ALL pixels is NaN by the reference's definition, every other entry is a number)
    assert np.isfinite(np.delete(a[0], score_cases.ENTRY["sum_epe"])).all() and a[0][score_cases.ENTRY["pixels"]] == h * w


@pytest.mark.parametrize("kind", ["flo", "kitti"])
def test_flow_score_batch_scratch(dev, kind):
    """35 fields: one call of 32 and one of 3, which takes a workspace of its own size."""
    from streamflow_amd import ops, scoring
    n, h, w = scoring.SCORE_BATCH_MAX + 3, 9, 13
    rng = np.random.default_rng([n, kind == "kitti"])
    fields = [eval_cases.make_field(rng, h, w, kind, 3 * i, True) for i in range(n)]
    preds = list(torch.from_numpy(np.stack([f[0] for f in fields])).to(dev))
    gts = np.stack([f[1] for f in fields])
    gts = list(torch.from_numpy(gts if kind == "flo" else gts.view(np.int16)).to(dev))
    masks = list(torch.from_numpy(np.stack([f[2] for f in fields])).to(dev))

    def call():
        acc = torch.zeros(n, scoring.EVAL_LEN, dtype=torch.float64, device=dev)
        ops.flow_score_batch(preds, gts, acc, kind, masks)
        return [acc]

    a, b = _both(call)
    _assert_bytes(a, b, f"flow_score_batch {kind}")
    for k in (0, n - 1):
        eval_cases.assert_row_matches(a[0][k], eval_cases.restate(*fields[k][:2], kind, fields[k][2]), f"{kind} field {k}")


def test_png_encode_scratch(dev):
    """Each stream up to its returned length (the bytes behind it are unspecified)."""
    from streamflow_amd import ops
    h, w, c = 37, 45, 3
    images = [png_encode_cases.make(k, h, w, c, 31 + i) for i, k in enumerate(("smooth", "noise", "zeros"))]
    batch = torch.from_numpy(np.stack(images).reshape(3, h, w, c)).to(dev)

    def call():
        streams, lengths = ops.png_encode(batch)
        return [lengths] + [streams[i, :int(lengths[i])] for i in range(3)]

    a, b = _both(call)
    _assert_bytes(a, b, "png_encode")
    for i in range(3):
        assert a[1 + i].tobytes() == png_encode_cases.encode_ref(images[i], False), i


def test_png_unfilter_scratch(dev):
    from streamflow_amd import ops
    h, w, ch, depth, how, seed = png_cases.CASES[2]                       # 37 x 53 RGB, filter types drawn per row
    imgs = [png_cases.image(h, w, ch, depth, seed + i) for i in range(2)]
    scan = np.stack([png_cases.encode(im, png_cases.filter_types(how, h, seed + i), None, depth).reshape(-1) for i, im in enumerate(imgs)])
    scan = torch.from_numpy(scan).to(dev)
    a, b = _both(lambda: [ops.png_unfilter(scan, h, w, ch * depth // 8)])
    _assert_bytes(a, b, "png_unfilter")
    assert np.array_equal(a[0], np.stack([png_cases.raw_rows(im, depth)[0] for im in imgs]))


def test_video_kernels_scratch(dev):
    from streamflow_amd import ops, video
    n, Tv, H, W = 6, 4, 36, 52
    pad = [2, 2, 3, 1]                                                     # left, right, top, bottom: 40 x 56
    frames = video_cases.random_frames(3, n, H, W).to(dev)
    n_clips = video.clip_count(n, Tv)
    a, b = _both(lambda: [ops.frames_to_clips(frames, n, Tv, 0, n_clips, pad)])
    _assert_bytes(a, b, "frames_to_clips")
    assert np.isfinite(a[0]).all() and a[0].shape == (n_clips, Tv, 3, 40, 56)
    g = torch.Generator().manual_seed(4)
    pairs = [torch.randn(n_clips, 2, 40, 56, generator=g).to(dev) for _ in range(Tv - 1)]
    a, b = _both(lambda: [ops.clips_to_flows(pairs, n, Tv, 0, 0, n - 1, (H, W), pad)])
    _assert_bytes(a, b, "clips_to_flows")
    assert np.isfinite(a[0]).all() and a[0].shape == (n - 1, 2, H, W)


def test_forward_interpolate_scratch(dev):
    from streamflow_amd import ops, synthetic as syn
    flow = syn.randn(6, "interp", (2, 2, 23, 37), 3.0).to(dev)
    a, b = _both(lambda: [ops.forward_interpolate(flow)])
    _assert_bytes(a, b, "forward_interpolate")
    assert np.isfinite(a[0]).all()


@pytest.mark.parametrize("layout", ["rows", "blocked"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("hw", [(16, 24), (17, 21)], ids=str)
def test_corr_block_scratch(dev, hw, dtype, layout):
    """Build and lookup: the volume, the build's scratch and the lookup's output all come from torch.empty.  Compared: the defined
    cells of the pyramid (the row pitch of the fp32 maps and the padding of the blocks are not part of it) and the lookup, with
    coordinates whose footprints hang over every border."""
    from streamflow_amd import synthetic as syn
    from streamflow_amd.corr import CorrBlock
    h, w = hw
    f1, f2 = (syn.randn(9, f"f{i}", (2, 64, h, w)).to(dev) for i in (1, 2))
    coords = (syn.randn(9, "coords", (2, 2, h, w), 6.0) + torch.tensor([w / 2, h / 2]).view(1, 2, 1, 1)).to(dev)

    def call():
        blk = CorrBlock(f1, f2, dtype=dtype, layout=layout)
        return [blk(coords)] + [p.contiguous() for p in blk.corr_pyramid]

    a, b = _both(call)
    _assert_bytes(a, b, f"CorrBlock {layout} {dtype} {hw}")
    assert all(np.isfinite(t.astype(np.float32)).all() for t in a) and a[0].shape == (2, 324, h, w)


# ---- F. the SK block launches what its route says --------------------------------------------------------------------------------

@pytest.mark.parametrize("flags,front,back", [({}, "pair", "pair"), ({"sk_tail_all": True}, "pair", "tail"),
                                              ({"ffn_pairs": False, "sk_tail": False}, "gemms", "gemms")])
def test_skblock_issues_the_calls_of_its_route(dev, monkeypatch, flags, front, back):
    """A 128 -> 64 block at 2 images of 8 x 8 from a k-octet-only input, f16x2: the C-ABI calls of engine.run_skblock are those of
    engine.resolve_skblock's route -- the default context (a small launch: pair + pw + pair), sk_tail_all (pair + tail) and with both
    fused forms off (five GEMMs) cover every value of front and back.  Each output against torch in float64 within the bound
    tests/test_gpu_parity.py::test_skblock_pw_fold_vs_float64 sets for this block in this mode."""
    import torch.nn.functional as F
    from streamflow_amd import _lib, ops
    from streamflow_amd.engine import SKBlockWeights, resolve_skblock, run_skblock
    from streamflow_amd.ops import Planes
    C, Cm, Co, k, n, h, w = 128, 192, 64, 15, 2, 8, 8
    P = h * w
    if "skblock" not in _CACHE:
        g = torch.Generator().manual_seed(C + k)
        r = lambda *s: torch.randn(*s, generator=g)
        sd = {"b.ffn1.0.weight": r(Cm, C, 1, 1) / C ** 0.5, "b.ffn1.0.bias": r(Cm) * 0.1,
              "b.ffn1.2.weight": r(C, Cm, 1, 1) / Cm ** 0.5, "b.ffn1.2.bias": r(C) * 0.1,
              "b.conv_list.0.weight": r(C, 1, 1, 1) * 0.3, "b.conv_list.0.bias": r(C) * 0.1,
              "b.conv_list.1.weight": r(C, 1, k, k) / k, "b.conv_list.1.bias": r(C) * 0.1,
              "b.pw.weight": r(C, C, 1, 1) / C ** 0.5, "b.pw.bias": r(C) * 0.1,
              "b.ffn2.0.weight": r(Cm, C, 1, 1) / C ** 0.5, "b.ffn2.0.bias": r(Cm) * 0.1,
              "b.ffn2.2.weight": r(Co, Cm, 1, 1) / Cm ** 0.5, "b.ffn2.2.bias": r(Co) * 0.1}
        x = r(n, C, h, w)
        d = {kk: v.double() for kk, v in sd.items()}
        c1 = lambda t, nm: F.conv2d(t, d["b." + nm + ".weight"], d["b." + nm + ".bias"])
        t = F.gelu(x.double() + c1(F.gelu(c1(x.double(), "ffn1.0")), "ffn1.2"))
        t = F.gelu(t + F.conv2d(t, d["b.conv_list.0.weight"], d["b.conv_list.0.bias"], groups=C))
        t = F.gelu(t + F.conv2d(t, d["b.conv_list.1.weight"], d["b.conv_list.1.bias"], padding=k // 2, groups=C))
        t = F.gelu(t + c1(t, "pw"))
        _CACHE["skblock"] = (SKBlockWeights(sd, "b", dev), x, c1(F.gelu(c1(t, "ffn2.0")), "ffn2.2").view(n, Co, P))
    W, x, ref = _CACHE["skblock"]
    x32 = Planes.of(x.view(n, C, P).to(dev))
    X = ops.new_shadow(x32, dev)                         # the block input as fp16 k-octet planes only
    ops.pack_koct(x32, X)
    y = torch.full((n, Co, P), float("nan"), device=dev)
    mk = lambda rows: Planes.of(torch.zeros(n, rows + 8, P, device=dev))
    cx = ops.Ctx(ops.PRECISION_F16X2, **flags)
    route = resolve_skblock(W, X, Planes.of(y), cx)
    assert (route.front, route.back) == (front, back)
    calls, check = [], _lib.check
    monkeypatch.setattr(_lib, "check", lambda status, what="": (calls.append(what), check(status, what))[1])
    run_skblock(W, X, Planes.of(y), mk(Cm), mk(C), mk(C), h, w, cx=cx)
    torch.cuda.synchronize()
    want = {"pair": ["sf_ffn_pair"], "gemms": ["sf_gemm", "sf_gemm"]}[front] + ["sf_dwconv_res_gelu_f16in"]
    want += {"tail": ["sf_sk_tail"], "pair": ["sf_gemm", "sf_ffn_pair"], "gemms": ["sf_gemm", "sf_gemm", "sf_gemm"]}[back]
    assert calls == want
    err, scale = (y.double().cpu() - ref).abs().max().item(), ref.abs().max().item()
    assert err < 4e-3 * scale, (err, scale)
