"""The Twins_CSC encoder (streamflow_amd/encoders.py) unit by unit against float64, in all four arithmetic classes (-m gpu).

`Twins_CSC.forward(..., taps=d)` hands out the fp32 token planes after each of its eight steps (embed_i, block_i.0, peg_i, block_i.1).
Every unit is compared with the oracle's own function in float64 ON THE GPU'S PREVIOUS TAP, with the weights as packed -- cases,
references, class emulation and bounds: tests/twins_cases.py; the proof that the bounds tell a wrong composition (pad tokens, frame
stacking, sr remainder, LayerNorm eps) from the right one: tests/test_twins_cases_cpu.py.  No number is fixed in advance:
    fp32, f16x3   rms <= 3 e32 and max <= 3 e32 (e32: the float32 CPU oracle of the unit against float64), and both also
                  <= 0.1 e_cls of F16X2 (a class that silently lost precision shows);
    f16x2, f16    rms <= 2 e_cls and max <= 4 e_cls (e_cls: the float64 unit with the class's documented fp16 roundings).
Also: the switches (koct_handover=False, exact_attention=True) in the reduced classes, each against the emulation of its own form;
finite taps, the output = the last tap under the documented view, two calls and a call with taps bitwise equal; a clip of a
batch-2 call inside the bounds of the clip alone; SKFlow_MF8._features runs both encoders in the preset's class.

Measured on an MI355X, worst ratio deviation / yardstick (rms, max) over the four cases, the switch forms and the single clips
(every test prints its own, pytest -s); the positional conv is 1.00, 1.00 in every class (the same fp32 kernel, the same order):
             embed0      block0.0    block0.1    embed1      block1.0    block1.1    bound
    fp32     1.00 1.21   1.28 2.49   2.46 2.70   2.46 5.12   1.72 2.77   2.33 2.79   3, 3 (embed1: 7.2, 11)
    f16x3    1.04 0.93   0.97 1.05   0.84 0.90   1.14 1.22   0.98 1.17   1.02 1.11   3, 3
    f16x2    1.00 1.00   1.01 1.07   1.00 1.11   1.00 1.00   1.00 1.13   1.00 1.05   2, 4
    f16      1.00 1.00   1.00 1.08   1.00 1.20   1.00 1.00   1.01 1.15   1.00 1.09   2, 4
  Class separation: fp32 at most 0.0036 (rms) and 0.0050 (max) of e_cls(F16X2), f16x3 0.0011 and 0.0014; the limit is 0.1.
  The emulation of the reduced classes is the kernels' arithmetic to 1 % in rms; exact_attention lowers the rms of the four
  attention units by 7 - 16 % (block0.1 in f16x2: 3.13e-4 against 3.71e-4).
  The exact-fp32 class is the least accurate of the two fp32 classes: its GEMM adds the K products of an output in one fp32 chain.
  In embed1 (a bare K = 512 conv + LayerNorm) that alone is 2.4 e32, and the unit missed 3 e32 in max (3.2 - 5.1): its margin is
  raised to 3 times a CPU model of that chain (tests/twins_cases.py UNIT_MARGIN, tests/test_twins_cases_cpu.py); every other
  unit keeps 3.  Found by this file and fixed: exact_attention=True with the hand-over taken asked the exact cores for k-octet
  operands and raised -- the forward now keeps the qkv and attention planes fp32 for them.
"""
import functools

import pytest
import torch

from tests import twins_cases as tc

pytestmark = pytest.mark.gpu
DEVICE = "cuda:0"
HAND_CASE, PLAIN_CASE = (1, 4, 32, 64), (2, 3, 40, 72)       # hand-over taken / the automatic fp32-plane fall-back
REPEAT_FLOOR = 1.1          # "no worse" between two forms: their rms are estimates over >= 128 tokens of correlated noise,
                            # relative standard deviation 1 / sqrt(2 * 128) = 6 % -- 10 % is the floor below which they are the same


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    return torch.device(DEVICE)


@functools.lru_cache(maxsize=None)
def _encoder():
    from streamflow_amd.encoders import Twins_CSC
    enc = Twins_CSC().to(DEVICE)
    enc.load_state_dict(dict(tc.params()), strict=True)
    return enc


def _call(x, cls, koct=True, exact=False, taps=None):
    enc = _encoder()
    enc.koct_handover, enc.exact_attention = koct, exact
    try:
        out = enc(x.to(DEVICE), precision=cls, taps=taps)
        torch.cuda.synchronize()
    finally:
        enc.koct_handover, enc.exact_attention = True, False
    return out.cpu()


@functools.lru_cache(maxsize=None)
def _run(c, cls, koct=True, exact=False, clip=None):
    """(images, {unit: tap}, output) on the CPU; clip: that clip of the case alone."""
    x = tc.images(c)
    if clip is not None:
        x = x[clip:clip + 1].contiguous()
    taps = {}
    out = _call(x, cls, koct, exact, taps)
    return x, {k: v.cpu() for k, v in taps.items()}, out


def _check_units(c, cls, x, taps, koct=True, exact=False, what=""):
    """Every unit of one run against its bound; returns {unit: (rms, max) deviation}.  All failures are reported together."""
    T, reduced = c[1], cls in tc.REDUCED
    hand = tc.handover(c) and (koct or not reduced)
    bad, devs = [], {}
    for u in tc.UNITS:
        inp = x if tc.previous(u) is None else taps[tc.previous(u)]
        y = tc.yardsticks(u, inp, T, hand, classes=(cls,) if reduced else ("f16x2",), exact_attention=exact and reduced)
        d = devs[u] = tc.dev(taps[u], y["ref"][cls])
        yard = y["e_cls"][cls] if reduced else y["e32"]
        b = tc.bound(u, cls, y["e32"], y["e_cls"].get(cls))
        line = (f"twins {tc.case_id(c)} {cls}{what} {u}: rms {d[0]:.3e} = {d[0] / yard[0]:.2f} x yardstick (bound {b[0] / yard[0]:.1f}), "
                f"max {d[1]:.3e} = {d[1] / yard[1]:.2f} x (bound {b[1] / yard[1]:.1f})")
        if not reduced and not u.startswith("peg"):
            sep = y["e_cls"]["f16x2"]
            line += f"; of e_cls(f16x2) {d[0] / sep[0]:.4f} {d[1] / sep[1]:.4f}"
            if d[0] > tc.SEPARATION * sep[0] or d[1] > tc.SEPARATION * sep[1]:
                bad.append("CLASS " + line)
        print(line)
        if not (d[0] <= b[0] and d[1] <= b[1]):
            bad.append(line)
    assert not bad, "\n".join(bad)
    return devs


@pytest.mark.parametrize("cls", tc.CLASSES)
@pytest.mark.parametrize("c", tc.CASES, ids=tc.case_id)
def test_units_vs_float64(dev, c, cls):
    x, taps, out = _run(c, cls)
    B, T, H, W = c
    assert set(taps) == set(tc.UNITS)
    for u, t in taps.items():
        gh, gw = tc.CASE_FACTS[c][1][int(u[5] if u.startswith(("embed", "block")) else u[3])]
        assert t.dtype == torch.float32 and t.shape == (B, 128 if gh == T * H // 4 else 256, gh, gw), u
        assert bool(torch.isfinite(t).all()), u
    assert out.shape == (B, T, 256, H // 8, W // 8) and bool(torch.isfinite(out).all())
    assert torch.equal(out, tc.output_view(taps["block1.1"], T))
    _check_units(c, cls, x, taps)


@pytest.mark.parametrize("cls", tc.CLASSES)
def test_calls_repeat_and_taps_change_nothing(dev, cls):
    """Two calls are bitwise equal, and a call with taps is bitwise the call without, in every case."""
    for c in tc.CASES:
        x = tc.images(c)
        first = _call(x, cls)
        assert torch.equal(first, _call(x, cls)), c
        assert torch.equal(first, _run(c, cls)[2]), c
        assert torch.equal(first, _call(x, cls, taps={})), c


@pytest.mark.parametrize("cls", tc.REDUCED)
def test_switches(dev, cls):
    """Hand-over case: the default, koct_handover=False and exact_attention=True each inside the class bound of their own
    emulation, per unit; exact attention no worse than the default in the four attention units.  The case whose T*H*W is no
    multiple of 256 takes the fp32-plane fall-back by itself: koct_handover=False is bitwise the default there."""
    c = HAND_CASE
    base = _check_units(c, cls, *_run(c, cls)[:2])
    _check_units(c, cls, *_run(c, cls, koct=False)[:2], koct=False, what=" koct_handover=False")
    ex = _check_units(c, cls, *_run(c, cls, exact=True)[:2], exact=True, what=" exact_attention")
    for u in tc.ATTENTION_UNITS:
        print(f"twins {tc.case_id(c)} {cls} {u}: exact attention rms {ex[u][0]:.3e} against {base[u][0]:.3e} by default")
        assert ex[u][0] <= REPEAT_FLOOR * base[u][0], (u, ex[u], base[u])
    c = PLAIN_CASE
    assert not tc.handover(c)
    _, taps, out = _run(c, cls)
    _, taps_off, out_off = _run(c, cls, koct=False)
    assert torch.equal(out, out_off) and all(torch.equal(taps[u], taps_off[u]) for u in tc.UNITS)


@pytest.mark.parametrize("cls", tc.CLASSES)
@pytest.mark.parametrize("c", [c for c in tc.CASES if c[0] == 2], ids=tc.case_id)
def test_clip_of_a_batch(dev, c, cls):
    """Clip b of the batch-2 call meets the per-unit bounds of clip b, and so does clip b run alone (split-K and the tile choice
    depend on the batch: the two need not be bitwise equal)."""
    x, taps, _ = _run(c, cls)
    for b in range(2):
        _check_units(c, cls, x[b:b + 1], {u: t[b:b + 1].contiguous() for u, t in taps.items()}, what=f" clip {b} of 2")
        xa, ta, _ = _run(c, cls, clip=b)
        assert torch.equal(xa, x[b:b + 1]) and ta["block1.1"].shape[0] == 1
        _check_units(c, cls, xa, ta, what=f" clip {b} alone")


@pytest.mark.parametrize("preset", ("fp32_class", "config2_fp16", "config2_mixed"))
def test_model_features_run_in_the_presets_class(dev, preset):
    """SKFlow_MF8._features = fnet over the T frames and cnet over the first T - 1, both in presets.PRESETS[name]['precision']."""
    from streamflow_amd import presets, synthetic as syn
    from streamflow_amd.model import SKFlow_MF8, default_args
    c = HAND_CASE
    model = SKFlow_MF8(default_args(T=c[1], preset=preset)).to(dev)
    model.fnet.load_state_dict(dict(syn.make_twins_params(22)), strict=True)
    model.cnet.load_state_dict(dict(syn.make_twins_params(23)), strict=True)
    x = tc.images(c).to(dev)
    p = presets.PRESETS[preset]["precision"]
    assert p == {"fp32_class": "f16x3", "config2_fp16": "f16x2", "config2_mixed": "f16x2"}[preset]
    fmaps, cnets = model._features(x)
    want_f, want_c = model.fnet(x, precision=p), model.cnet(x[:, :-1], precision=p)
    assert fmaps.shape == (c[0], c[1], 256, c[2] // 8, c[3] // 8) and cnets.shape == (c[0], c[1] - 1, 256, c[2] // 8, c[3] // 8)
    assert torch.equal(fmaps, want_f) and torch.equal(cnets, want_c)
    other = "f16x2" if p == "f16x3" else "f16x3"              # the comparison can see a wrong class: the other one differs
    assert not torch.equal(fmaps, model.fnet(x, precision=other)) and not torch.equal(cnets, model.cnet(x[:, :-1], precision=other))
    assert not torch.equal(fmaps[:, :-1], cnets)             # two encoders, two sets of weights
