"""tests/twins_cases.py on the CPU: the units chain to the oracle's whole forward, the class emulation without its roundings IS the
oracle's unit, the weight split restates ops.PackedLinear, the case table says what the issue's table says -- and the proof that the
bounds of tests/test_gpu_twins_stages.py discriminate: every wrong variant of the reference (a pad tokens out of the window softmax,
b frames one by one, c sr remainder zero-padded, d eps 1e-5 in the blocks' LayerNorms) is at least TWICE the bound away from the
right reference, rms and max, in one unit of one case at least; a, b, c against the bound of every class, d against the fp32-class
bound.  This is a condition on the cases and margins, met by the reference alone; the yardsticks are printed (pytest -s).
A unit's input here is the float64 chain's previous tap rounded to fp32 (on the GPU: the GPU's own previous tap)."""
import functools

import pytest
import torch

from oracle import twins_oracle as two
from tests import twins_cases as tc


@functools.lru_cache(maxsize=None)
def _inputs(c):
    """{unit: its fp32 input} from the float64 chain."""
    x = tc.images(c)
    taps = tc.chain(x.double(), tc.effective_params("fp32"), c[1])
    return {u: (x if tc.previous(u) is None else taps[tc.previous(u)].float()) for u in tc.UNITS}, taps


@functools.lru_cache(maxsize=None)
def _yard(c, unit):
    return tc.yardsticks(unit, _inputs(c)[0][unit], c[1], tc.handover(c), classes=tc.REDUCED)


def _variant_defined(wrong, unit, c):
    """b runs the sr convolution on one frame's grid: undefined where that grid is smaller than the kernel."""
    if wrong != "b" or not unit.endswith(".1"):
        return True
    i = int(unit[5])
    gh, gw = tc.CASE_FACTS[c][1][i]
    return gh // c[1] >= two.SR_RATIOS[i] and gw >= two.SR_RATIOS[i]


@functools.lru_cache(maxsize=None)
def _wrong_dev(c, unit, wrong):
    got = tc.run_unit(unit, _inputs(c)[0][unit].double(), tc.effective_params("fp32"), c[1], wrong=wrong)
    return tc.dev(got, _yard(c, unit)["ref"]["fp32"])


def test_case_table():
    assert len(tc.CASES) == 4 and set(tc.CASES) == set(tc.CASE_FACTS)
    for c in tc.CASES:
        B, T, H, W = c
        hand, grids, keys = tc.CASE_FACTS[c]
        assert H % 8 == 0 and W % 8 == 0 and tc.handover(c) == hand
        assert grids == ((T * H // 4, W // 4), (T * H // 8, W // 8))
        assert keys == tuple((gh // sr) * (gw // sr) for (gh, gw), sr in zip(grids, two.SR_RATIOS))
    assert (3 * 40 * 72) % 256 == 192                         # the one case without the hand-over
    assert [tc.handover(c) for c in tc.CASES] == [True, False, True, True]
    pad = lambda g: any(v % two.WINDOW for v in g)
    assert [all(pad(g) for g in tc.CASE_FACTS[c][1]) for c in tc.CASES] == [True, True, False, True]
    g = tc.CASE_FACTS[(1, 2, 56, 112)][1]
    assert (g[0][0] % 8, g[1][0] % 4) == (4, 2) and (g[1][0] * g[1][1]) % 32 != 0      # dropped sr remainders; N2 = 196
    assert tc.CASE_FACTS[(2, 3, 40, 72)][1][0][0] % 8 and tc.CASE_FACTS[(2, 3, 40, 72)][1][1][0] % 4
    g = tc.CASE_FACTS[(2, 4, 24, 40)][1]
    assert (g[0][0] * g[0][1], g[1][0] * g[1][1]) == (240, 60)
    assert sorted(c[0] for c in tc.CASES) == [1, 1, 2, 2]
    assert set(tc.ATTENTION_UNITS) == {u for u in tc.UNITS if u.startswith("block")}


@pytest.mark.parametrize("c", tc.CASES, ids=tc.case_id)
def test_units_chain_to_the_whole_oracle(c):
    """The eight units, each on the one before, are twins_csc_forward; the last tap under output_view is its output."""
    taps = _inputs(c)[1]
    whole = two.twins_csc_forward(tc.images(c).double(), tc.effective_params("fp32"))
    out = tc.output_view(taps["block1.1"], c[1])
    assert out.shape == whole.shape == (c[0], c[1], 256, c[2] // 8, c[3] // 8)
    assert tc.dev(out, whole)[1] <= 1e-12
    for u, (gh, gw) in zip(tc.UNITS, [g for g in tc.CASE_FACTS[c][1] for _ in range(4)]):
        assert taps[u].shape == (c[0], two.EMBED_DIMS[int(u[-3] if u.startswith("block") else u[-1])], gh, gw), u


@pytest.mark.parametrize("c", tc.CASES, ids=tc.case_id)
def test_emulation_without_rounding_is_the_oracle(c):
    """The emulation's own data flow (channel-major attention through tests/attn_cases.py, bias pad tokens, dropped sr remainder)
    with every rounding switched off equals the oracle's unit: what e_cls measures is the roundings and nothing else."""
    for u in tc.UNITS:
        for hand in (False, True):
            got = tc.emulate_unit(u, _inputs(c)[0][u], tc.effective_params("fp32"), c[1], hand, rounding=False)
            assert tc.dev(got, _yard(c, u)["ref"]["fp32"])[1] <= 1e-12, (u, hand)


def test_effective_params_restate_the_packing():
    """split_weight against ops.PackedLinear (built on the CPU): the same hi and lo images and scale, for every GEMM layer."""
    from streamflow_amd.ops import PackedLinear
    n = 0
    for k, t in tc.params().items():
        if not tc.is_gemm_weight(k, t):
            assert torch.equal(tc.effective_params("f16")[k], t.double())
            continue
        A = PackedLinear(t, None, "cpu")
        unpack = lambda img: img.float().permute(1, 0, 2).reshape(A.lda_h, -1)[: A.M, : A.K].double()          # noqa: E731
        hi, lo, s = tc.split_weight(t)
        assert s == A.split_scale and torch.equal(hi.reshape(A.M, A.K), unpack(A.hi)) and torch.equal(lo.reshape(A.M, A.K), unpack(A.lo)), k
        assert torch.equal(tc.effective_params("f16x2")[k].reshape(A.M, A.K), (unpack(A.hi) + unpack(A.lo)) / s)
        assert torch.equal(tc.effective_params("f16")[k].reshape(A.M, A.K), unpack(A.hi) / s)
        assert float((tc.effective_params("f16x3")[k] - t.double()).abs().max()) <= 2.0 ** -20 * float(t.abs().max())
        n += 1
    assert n == 2 * (1 + 4 + 6)          # per stage: patch embed; qkv, proj, fc1, fc2; q, kv, sr, proj, fc1, fc2


def test_single_chain_model_of_embed1():
    """The reason for twins_cases.UNIT_MARGIN[('embed1', 'fp32')]: embed1 with the K = 512 products of every conv output added
    one after the other into ONE fp32 accumulator (one rounding per step, as a fused multiply-add chain) is 2.4 e32 away from
    float64 (rms; max 2.8 - 3.7 over the four cases), where e32 comes from the CPU GEMM's interleaved partial sums.  The raised
    margin is 3 times this model, no more."""
    c = (2, 4, 24, 40)
    T, inp = c[1], _inputs(c)[0]["embed1"]
    p, p64 = tc.params(), tc.effective_params("fp32")
    B, C, gh, gw = inp.shape
    cols = torch.nn.functional.unfold(tc._frames(inp, T).reshape(B * T, C, gh // T, gw), 2, stride=2)        # [BT, 4C, n]: c, ky, kx
    w = p["svt.patch_embeds.1.proj.weight"].reshape(256, -1)
    acc = p["svt.patch_embeds.1.proj.bias"][None, :, None].expand(B * T, 256, cols.shape[-1]).clone()
    for k in range(w.shape[1]):
        acc = (acc.double() + w[None, :, k, None].double() * cols[:, None, k, :].double()).float()
    tok = acc.reshape(B, T, 256, -1).permute(0, 1, 3, 2).reshape(B, -1, 256).double()
    out = two._ln(tok, p64["svt.patch_embeds.1.norm.weight"], p64["svt.patch_embeds.1.norm.bias"], two.LN_EPS)
    y = _yard(c, "embed1")
    d = tc.dev(tc._planes(out, (gh // 2, gw // 2)), y["ref"]["fp32"])
    print(f"embed1 single fp32 chain: rms {d[0] / y['e32'][0]:.2f} e32, max {d[1] / y['e32'][1]:.2f} e32")
    m = tc.UNIT_MARGIN[("embed1", "fp32")]
    assert 2.0 <= d[0] / y["e32"][0] and m[0] <= 3.0 * 1.05 * d[0] / y["e32"][0]
    assert m[1] <= 3.0 * 3.7 and m == tc.bound("embed1", "fp32", (1.0, 1.0), None)
    assert set(tc.UNIT_MARGIN) == {("embed1", "fp32")}


def test_yardsticks_are_recorded_and_separate_the_classes():
    """Prints e32 and e_cls per unit and case.  The class-separation condition of the GPU test (fp32-class deviations at most
    0.1 e_cls of F16X2) leaves room for the fp32-class bound: 3 e32 <= 0.1 e_cls in every unit that rounds anything."""
    for c in tc.CASES:
        for u in tc.UNITS:
            y = _yard(c, u)
            print(f"{tc.case_id(c):>12} {u:9s} e32 rms {y['e32'][0]:.2e} max {y['e32'][1]:.2e} | " +
                  " | ".join(f"e_{k} rms {v[0]:.2e} max {v[1]:.2e}" for k, v in y["e_cls"].items()))
            assert 0 < y["e32"][0] <= y["e32"][1] < 1e-5
            if u.startswith("peg"):
                assert y["e_cls"]["f16x2"] == y["e32"]
                continue
            for k in (0, 1):
                assert tc.bound(u, "fp32", y["e32"], None)[k] <= tc.SEPARATION * y["e_cls"]["f16x2"][k], (c, u)
                assert 2.0 ** -14 < y["e_cls"]["f16x2"][k] < 2.0 ** -8 and 2.0 ** -14 < y["e_cls"]["f16"][k] < 2.0 ** -8


@pytest.mark.parametrize("wrong", tc.WRONG)
def test_wrong_variants_are_outside_every_bound(wrong):
    """At least twice the bound away, rms AND max, in one unit of one case -- a, b, c for every class, d for the fp32 class."""
    classes = ("fp32",) if wrong == "d" else tc.CLASSES
    hit = {cls: [] for cls in classes}
    for c in tc.CASES:
        for u in tc.ATTENTION_UNITS:
            if not _variant_defined(wrong, u, c):
                continue
            d, y = _wrong_dev(c, u, wrong), _yard(c, u)
            print(f"variant {wrong} {tc.case_id(c):>12} {u}: rms {d[0]:.2e} max {d[1]:.2e} "
                  f"(fp32 bound {tc.bound(u, 'fp32', y['e32'], None)[0]:.2e} {tc.bound(u, 'fp32', y['e32'], None)[1]:.2e})")
            for cls in classes:
                b = tc.bound(u, cls, y["e32"], y["e_cls"].get(cls))
                if d[0] >= 2.0 * b[0] and d[1] >= 2.0 * b[1]:
                    hit[cls].append((c, u))
    for cls in classes:
        assert hit[cls], (wrong, cls)
    if wrong == "d":
        # the eps shows in the window blocks of every case (rms 4 - 5e-6 against a bound of 9e-7 - 1.2e-6).  In the sub-sampled
        # blocks it does NOT: their input has a larger variance behind the positional conv, the eps moves them by rms 1.0 - 1.2e-6,
        # inside the fp32-class bound of 1.3 - 1.8e-6 -- a wrong eps in blocks.i.1 alone is below what fp32 noise lets a test see
        assert set(hit["fp32"]) == {(c, u) for c in tc.CASES for u in ("block0.0", "block1.0")}, hit


def test_wrong_variants_are_zero_where_they_must_be():
    """No pad tokens on the 28 x 28 and 14 x 14 grids: a is exactly the reference; windows of 7 rows do not straddle frames of 14
    or 7 rows: b leaves the window blocks alone there; c changes nothing where the sr convolution has no remainder."""
    c = (1, 2, 56, 112)
    for u in tc.ATTENTION_UNITS:
        assert _wrong_dev(c, u, "a") == (0.0, 0.0), u
    for u in ("block0.0", "block1.0"):
        assert _wrong_dev(c, u, "b") == (0.0, 0.0), u
    c = (1, 4, 32, 64)                                        # 32 x 16 over sr 8, 16 x 8 over sr 4: no remainder
    for u in tc.ATTENTION_UNITS:
        assert _wrong_dev(c, u, "c") == (0.0, 0.0), u
    for c in tc.CASES:                                        # and each is far off somewhere in every other case
        if any(v % two.WINDOW for g in tc.CASE_FACTS[c][1] for v in g):
            assert _wrong_dev(c, "block0.0", "a")[0] > 1e-2 and _wrong_dev(c, "block1.0", "a")[0] > 1e-2, c
