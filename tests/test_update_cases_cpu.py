"""tests/update_cases.py on the CPU: the units chain to the oracle's whole forward, the class emulation without its roundings IS the
oracle's unit, the packed weights restate ops.PackedLinear, the restated GMA and fp16-volume models are the suite's own
(tests/attn_cases.py, tests/corr_cases.py), the case table says what the cases are for -- and the proof that the bounds of
tests/test_gpu_update_stages.py discriminate: every wrong composition (a mfg / mft swapped in the GRU's concat, b post-update flow
rows in mf, c mask alpha dropped, d GMA scale dropped, e lookup at the next pair's coordinates, f convc1 without its final GELU,
g the flow head fed pair-major images) is outside the bound, rms and max, and at least TWICE the bound away in rms, in cases S
and R under every configuration.  This is a condition on the cases and margins, met by the reference alone; the yardsticks are printed
(pytest -s).  A unit's input here is the float64 chain's taps rounded to fp32 (on the GPU: the GPU's own taps)."""
import functools

import pytest
import torch

from oracle import streamflow_oracle as orc
from tests import attn_cases as ac, corr_cases as cc, twins_cases as tc, update_cases as uc

SMALL = ("S", "R")


@functools.lru_cache(maxsize=None)
def _taps(c):
    """The float64 chain's taps, rounded to fp32 (what a GPU tap is)."""
    T = uc.CASES[c][1]
    t = uc.oracle_taps(c, {k: v.double() for k, v in uc.params(T).items()})
    return {k: ([v.float() for v in t[k]] if isinstance(t[k], list) else t[k].float()) for k in t}


@functools.lru_cache(maxsize=None)
def _yard(unit, cfg, c, separation=False):
    return uc.yardsticks(unit, uc.unit_inputs(unit, _taps(c)), cfg, c, separation=separation)


def test_case_table():
    assert uc.CASES == {"S": (2, 3, 16, 24), "R": (1, 4, 17, 21), "F": (3, 4, 48, 68)}
    P = {c: v[2] * v[3] for c, v in uc.CASES.items()}
    assert P["S"] % 4 == 0 and P["R"] % 4 != 0 and P["R"] % 2 != 0 and P["F"] % 4 == 0
    assert 9 * P["F"] == 29376 >= 4 * 7040 == 28160
    assert [uc.fills(c) for c in ("S", "R", "F")] == [False, False, True]
    assert len(uc.images_of("F")) == 6 and uc.images_of("F") == [0, 1, 2, 6, 7, 8] and uc.images_of("S") == [0, 1, 2, 3]
    for cfg in uc.CONFIGS:
        f = {c: uc.facts(cfg, c) for c in uc.CASES}
        assert f["S"]["hand"] == f["F"]["hand"] == f["S"]["reduced"] and not f["R"]["hand"]
        assert f["S"]["lookup16"] == (cfg in ("config2_fp16", "config2_mixed")) and not f["R"]["lookup16"]
    assert not uc.gma_rounds(uc.facts("fp32", "S")) and not uc.gma_rounds(uc.facts("fp32", "R"))
    assert uc.facts("f16x3_matrix", "R")["gma"]["w16"] == "split8" and uc.facts("f16", "R")["gma"]["w16"] == "norm"
    assert uc.facts("f16x3_matrix", "S")["gma"]["w16"] == "norm" and uc.facts("fp32_class", "R")["gma"]["w16"] == "exp2"
    assert uc.facts("config2_mixed", "S")["gma"] == dict(form="flash", q16=True, k16=True, w16="exp2", v16=True)
    assert len(uc.facts("config2_mixed", "S")["singles"]) == 24 and not uc.facts("config2_fp16", "S")["singles"]
    assert set(uc.WRONG.values()) <= set(uc.UNITS) and set(uc.OUTPUTS) == set(uc.UNITS)
    for c in uc.CASES:                                        # a seeded warm start of about 2 px, off the integer grid
        fl = uc.pre_state(c)[1]
        assert 1.5 < float(fl.std()) < 2.5 and float((fl - fl.round()).abs().mean()) > 0.2


@pytest.mark.parametrize("c", SMALL)
def test_units_chain_to_the_whole_oracle(c):
    """Every unit on the units before it is orc.hotpath_forward for one iteration (both in float32: the oracle's lookup returns
    float32 whatever it is given); the float64 chain is the same function to float32 accuracy."""
    B, T, h, w = uc.CASES[c]
    n = B * (T - 1)
    fm, cn, finit = uc.inputs(c)
    ups, low = orc.hotpath_forward(fm, cn, uc.params(T), 1, flow_init=finit)
    up, lo = torch.stack(ups, 1).reshape(n, 2, 8 * h, 8 * w), torch.stack(low, 1).reshape(n, 2, h, w)
    t32 = uc.oracle_taps(c, uc.params(T), torch.float32)
    assert tc.dev(t32["flow"], lo)[1] <= 1e-6 and tc.dev(t32["up"], up)[1] <= 1e-5
    t64 = uc.oracle_taps(c, {k: v.double() for k, v in uc.params(T).items()})
    assert tc.dev(t64["flow"], lo)[1] <= 1e-4 and tc.dev(t64["up"], up)[1] <= 1e-4
    assert float(t64["delta"].abs().max()) > 0.01             # the iteration moves the flow
    for u in uc.UNITS:
        for name in uc.OUTPUTS[u]:
            v = uc.tap_of(t64, name)
            assert all(bool(torch.isfinite(x).all()) for x in (v if isinstance(v, list) else [v])), name


@pytest.mark.parametrize("c", SMALL)
def test_emulation_without_rounding_is_the_oracle(c):
    """emulate_unit's own data flow (ref_pair / ref_tail with the folded pw weights, the token views, the GMA through the qk tap)
    with every rounding switched off equals the oracle's unit, with the weights of every configuration."""
    for cfg in uc.CONFIGS:
        f, pe = uc.facts(cfg, c), uc.effective_params(cfg, c)
        for hand in {f["hand"], f["reduced"]}:                # (the folded form also where this case does not take it)
            if hand and not f["hand"]:
                continue
            for u in uc.UNITS:
                x = uc.unit_inputs(u, _taps(c))
                got = uc.dev_taps(uc.emulate_unit(u, x, pe, dict(f, hand=hand), rounding=False), _yard(u, cfg, c)["ref"])
                assert all(d[1] <= 1e-11 for d in got.values()), (cfg, u, got)


def test_effective_params_restate_the_packing():
    """split_weight and effective_params against ops.PackedLinear (built on the CPU): hi, lo and scale of every contraction layer,
    the folded pw_res, the mask head's 3 x 3 layer in its packed order; single layers and precision='f16' take hi alone."""
    from streamflow_amd.ops import PackedLinear
    T = 3
    p = uc.params(T)
    unpack = lambda A, img: img.float().permute(1, 0, 2).reshape(A.lda_h, -1)[: A.M, : A.K].double()      # noqa: E731
    names = uc.layer_names()
    assert len(names) == 9 + 6 * 5
    split, mixed, half = (uc._effective(T, "f16x2", (), True), uc._effective(T, "f16x2", uc.facts("config2_mixed", "S")["singles"], True),
                          uc._effective(T, "f16", (), True))
    singles = uc.facts("config2_mixed", "S")["singles"]
    for nm in names:
        k = uc.layer_key(nm)
        w = p[k]
        A = PackedLinear(w, None, "cpu", conv3x3=nm == "mask0")
        hi, lo = unpack(A, A.hi), unpack(A, A.lo)
        if nm == "mask0":                                     # packed k = (ky * 3 + kx) * Cin + c
            hi, lo = (t.reshape(A.M, 3, 3, -1).permute(0, 3, 1, 2) for t in (hi, lo))
        h2, l2, s = tc.split_weight(w)
        assert s == A.split_scale and torch.equal(h2.reshape(hi.shape), hi) and torch.equal(l2.reshape(hi.shape), lo), nm
        if nm.endswith(".pw"):
            eye = torch.eye(w.shape[0]).reshape(w.shape[0], w.shape[0], 1, 1)
            R = PackedLinear(w + eye, None, "cpu")
            res = (unpack(R, R.hi) + unpack(R, R.lo)) / R.split_scale
            assert torch.equal(split[k.replace(".pw.", ".pw_res.")].reshape(res.shape), res)
            assert torch.equal(split[k].reshape(res.shape), res - eye.double().reshape(res.shape))
            one = unpack(R, R.hi) / R.split_scale
            assert torch.equal(half[k.replace(".pw.", ".pw_res.")].reshape(res.shape), one)
            assert torch.equal(mixed[k.replace(".pw.", ".pw_res.")].reshape(res.shape), one if nm in singles else res)
            continue
        assert torch.equal(split[k].reshape(hi.shape), (hi + lo) / s) and torch.equal(half[k].reshape(hi.shape), hi / s), nm
        assert torch.equal(mixed[k].reshape(hi.shape), (hi if nm in singles else hi + lo) / s), nm
        assert float((split[k] - w.double()).abs().max()) <= 2.0 ** -20 * float(w.abs().max())
    plain = uc._effective(T, "f16x3", (), False)
    assert not any("pw_res" in k for k in plain) and all(torch.equal(uc._effective(T, "fp32", (), False)[k], v.double()) for k, v in p.items())
    for blk, (prefix, _) in uc.SK_UNITS.items():
        k = prefix + ".conv_list.1.weight"
        assert torch.equal(half[k], tc.r16(p[k])) and torch.equal(split[k], p[k].double())
        assert torch.equal(mixed[k], tc.r16(p[k]) if blk + ".dw" in singles else p[k].double())
    assert {"convf2.dw", "conv.dw"} <= set(singles)


def test_fft_depthwise_is_conv2d():
    """update_cases.dwconv (the float64 depthwise layers of the references) against F.conv2d, 15 x 15 and 7 x 7, and through the
    oracle's skblock as run_unit calls it."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(5)
    for k, C in ((15, 324), (7, 640)):
        x, w, b = (torch.randn(*sh, generator=g, dtype=torch.float64) for sh in ((3, C, 17, 21), (C, 1, k, k), (C,)))
        want = F.conv2d(x, w, b, padding=k // 2, groups=C)
        assert tc.dev(uc.dwconv(x, w, b, k // 2, C), want)[1] <= 1e-13 * float(want.abs().max())
        assert torch.equal(uc.dwconv(x.float(), w.float(), b.float(), k // 2, C), F.conv2d(x.float(), w.float(), b.float(), padding=k // 2, groups=C))
    p = {k: v.double() for k, v in uc.params(3).items()}
    x = _taps("S")["cat256"].double()
    assert tc.dev(uc.run_unit("conv", dict(x=x), p, 2)["mf"], orc.skblock(x, p, *uc.SK_UNITS["conv"]))[1] <= 1e-13


def test_gma_model_is_the_attention_cases_model():
    """gma_model('flash') against tests/attn_cases.py's model of gma1 / gma3 on one image of case S's grid: the same function."""
    t = _taps("S")
    P = 16 * 24
    qk, mf = t["qk"][:1].reshape(1, 256, P).double(), torch.cat([t["mf"], t["flow0"]], 1)[:1].reshape(1, 128, P).double()
    v = torch.einsum("mk,nkp->nmp", uc.params(3)["update_block.aggregator.to_v.weight"].reshape(128, 128).double(), mf)
    exact, _, model = ac.gma_reference(qk.numpy(), v.numpy(), mf.numpy(), 0.5, products=(1, 3))
    ref = uc.run_unit("gma", dict(qk=qk.reshape(1, 256, 16, 24), mf=mf.reshape(1, 128, 16, 24)), {k: x.double() for k, x in uc.params(3).items()}, 2)
    assert tc.dev(ref["mfg"].reshape(1, 128, P), torch.from_numpy(exact))[1] <= 1e-12
    for products, g in ((1, uc.facts("config2_fp16", "S")["gma"]), (3, uc.facts("fp32_class", "S")["gma"])):
        got = uc.gma_model(qk, v, mf, 0.5, g)
        e = tc.dev(torch.from_numpy(model[products]), torch.from_numpy(exact))
        d = tc.dev(got, torch.from_numpy(model[products]))
        print(f"gma products {products}: model - exact rms {e[0]:.2e}, restatement - model rms {d[0]:.2e} max {d[1]:.2e}")
        # r16 rounds the fp32 value a kernel holds, attn_cases.f16 the float64 one: one weight in 2^13 falls the other way (2 % of the
        # model's own rms); gma3: attn_cases splits q and k into hi + lo (2^-21), the restatement keeps them
        assert d[0] <= 0.05 * e[0], (products, d, e)


def test_corr16_is_the_correlation_cases_model():
    """corr16 against tests/corr_cases.py's model of fp16 cells from fp16 features (class 'f16'; 'b16' folds exact powers of two) on
    one pair of case S: the same roundings; the fp32 accumulation steps it leaves out move a cell by less than its fp16 rounding."""
    t = _taps("S")
    f1, f2 = t["f1"][:1].double(), t["f2"][:1].double()
    mine = uc.corr16(f1, f2)
    exact = uc.run_unit("volume", dict(f1=f1, f2=f2), None, 1)["volume"]
    theirs = cc.model(f1[0].reshape(256, -1).numpy(), f2[0].reshape(256, -1).numpy(), 16, 24, cc.klass("f16", D=256))
    for l in range(4):
        e_mine = tc.dev(mine[l][0], exact[l][0])
        e_theirs = tc.dev(torch.from_numpy(theirs[l]), exact[l][0])
        same = float((mine[l][0] == torch.from_numpy(theirs[l])).double().mean())
        print(f"level {l}: corr16 rms {e_mine[0]:.3e}, corr_cases.model rms {e_theirs[0]:.3e}, equal cells {same:.4f}")
        assert abs(e_mine[0] / e_theirs[0] - 1.0) <= 0.02 and same >= 0.99


def test_yardsticks_are_recorded_and_separate_the_classes():
    """Prints e32, e_cls per unit, configuration and case.  The class-separation condition of the GPU test (fp32-class deviations at
    most 0.1 e_cls of F16X2) leaves room for the fp32-class bound, 3 e32 <= 0.1 e_cls, in every unit with a contraction."""
    for c in SMALL:
        for cfg in ("fp32_class", "config2_mixed", "f16"):
            for u in uc.UNITS:
                y = _yard(u, cfg, c, separation=cfg == "fp32_class")
                for name in uc.OUTPUTS[u]:
                    e32, ecl = y["e32"][name], y["e_cls"][name]
                    print(f"{c} {cfg:13s} {u:11s} {name:10s} e32 rms {e32[0]:.2e} max {e32[1]:.2e} | e_cls rms {ecl[0]:.2e} max {ecl[1]:.2e}")
                    if cfg == "fp32_class" and u not in uc.NO_GEMM + ("gma",):
                        sep = y["sep"][name]
                        for k in (0, 1):
                            assert 3.0 * e32[k] <= tc.SEPARATION * sep[k], (c, u, name, e32, sep)


def test_models_of_the_raised_margins():
    """The reasons for update_cases.UNIT_MARGIN, each as a CPU model against the unit's float64 reference, in units of e32: the margin
    is 3 times the model (within 5 %), no more.  And the model behind the matrix form's yardstick at odd P in f16x3: softmax weights
    as split8() pairs are 25 - 28 e32 away by themselves -- the lo halves of weights of 1 / 357 are fp16 subnormals."""
    worst = {k: [0.0, 0.0] for k in uc.UNIT_MARGIN}
    for c in SMALL:
        T = uc.CASES[c][1]
        t = _taps(c)
        y = _yard("mask0", "fp32", c)
        d, e = tc.dev(uc.single_chain_mask0(t["nets"], uc.params(T)), y["ref"]["m256"]), y["e32"]["m256"]
        print(f"{c} mask0, one fp32 chain: rms {d[0] / e[0]:.2f} e32, max {d[1] / e[1]:.2f} e32")
        for cls in ("fp32", "f16x3"):
            worst["mask0", cls] = [max(a, b) for a, b in zip(worst["mask0", cls], (d[0] / e[0], d[1] / e[1]))]
        y = _yard("convf1", "fp32_class", c)
        got = uc.run_unit("convf1", dict(flow=uc.split8_image(t["flow0"])), uc.effective_params("fp32_class", c), T - 1)["f128"]
        d, e = tc.dev(got, y["ref"]["f128"]), y["e32"]["f128"]
        print(f"{c} convf1 on split8(flow): rms {d[0] / e[0]:.2f} e32, max {d[1] / e[1]:.2f} e32")
        worst["convf1", "f16x3"] = [max(a, b) for a, b in zip(worst["convf1", "f16x3"], (d[0] / e[0], d[1] / e[1]))]
    for k, m in uc.UNIT_MARGIN.items():
        assert 2.0 <= worst[k][0] and m[0] <= 3.0 * 1.05 * worst[k][0] and m[1] <= 3.0 * 1.05 * worst[k][1], (k, m, worst[k])
        assert uc.bound(k[0], dict(cls=k[1], reduced=False), (1.0, 1.0), None) == m
    assert set(uc.UNIT_MARGIN) == {("mask0", "fp32"), ("mask0", "f16x3"), ("convf1", "f16x3")}
    y = _yard("gma", "f16x3_matrix", "R")
    r = y["e_cls"]["mfg"][0] / y["e32"]["mfg"][0]
    print(f"R gma, matrix form, split8 softmax weights: e_cls = {r:.1f} e32")
    assert 20.0 <= r <= 35.0 and uc.yard_kind("gma", uc.facts("f16x3_matrix", "R")) == "e_cls"


@pytest.mark.parametrize("wrong", sorted(uc.WRONG))
def test_wrong_compositions_are_outside_every_bound(wrong):
    """Outside the bound in rms AND in max (either fails the GPU test), the rms -- the stable statistic -- at least twice, under
    every configuration, in S and in R.  (b moves the GRU's input by one iteration's flow update, 0.07 px at most here: under
    the fp16 classes it is 3.7 bounds away in rms and 1.8 in max, everything else is orders of magnitude away.)  g is the right
    reference where a batch is one clip (R): pair-major and clip-major are the same order there."""
    unit = uc.WRONG[wrong]
    for c in SMALL:
        Pn = uc.CASES[c][1] - 1
        for cfg in uc.CONFIGS:
            f, pe, y = uc.facts(cfg, c), uc.effective_params(cfg, c), _yard(unit, cfg, c)
            x = uc.unit_inputs(unit, _taps(c), wrong=wrong)
            x64 = {k: ([t.double() for t in v] if isinstance(v, list) else v.double()) for k, v in x.items()}
            d = uc.dev_taps(uc.run_unit(unit, x64, pe, Pn, wrong=wrong if wrong != "b" else None), y["ref"])
            for name in uc.OUTPUTS[unit]:
                b = uc.bound(unit, f, y["e32"][name], y["e_cls"][name])
                print(f"variant {wrong} {c} {cfg:13s} {name}: rms {d[name][0]:.2e} max {d[name][1]:.2e} (bound {b[0]:.2e} {b[1]:.2e})")
                if wrong == "g" and uc.CASES[c][0] == 1:
                    assert d[name] == (0.0, 0.0)
                    continue
                assert d[name][0] >= 2.0 * b[0] and d[name][1] >= b[1], (wrong, c, cfg, name, d[name], b)
