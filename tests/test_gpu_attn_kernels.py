"""The attention family through the C ABI (-m gpu): sf_gma_flash_ws_bytes / _pack_qk / _aggregate / _aggregate_f16v / _project_v,
sf_gma_stored_p_bytes / sf_gma_flash_store_p / sf_gma_stored_aggregate (csrc/attn.hip), sf_window_attn / _mfma, sf_subsample_attn /
_ws_bytes / _mfma (csrc/encoder.hip) -- raw pointers and strides handed to streamflow_amd._lib.load(), not the ops wrappers (which
only ever pass dense image strides), at the smallest shapes at which each path can go wrong (tests/attn_cases.py).

Operands sit NaN-filled in guard-banded buffers (tests/guarded.py), outputs in a finite sentinel, `ws` and `pbuf` are exactly the bytes
the size functions return between guard bands.  Every case asserts: status 0; every output element written; nothing outside a view
and no guard byte changed; the placed run (every image stride beyond dense and different from operand to operand, bases off the
allocation's start, aligned where include/streamflow_hip.h demands it) BITWISE the contiguous run; image z of a batch bitwise the
call on image z alone, for every z; the forms the header calls identical bitwise identical (pipelined = round-5 kernel, stored weights = recompute with
statistics, fp16 rows of v = fp32 planes of v, the k-octet copy = fp16(out) of the same launch); and every element within the
per-element bound of tests/attn_cases.py (err / bound is printed per case: "ATTN ...").  tests/test_attn_cases_cpu.py shows that this
bound tells a wrong kernel from a right one.

The bound's fp32 accumulation term of the second contraction is derived in tests/attn_cases.py: without it sf_window_attn reads 1.08
at ws = 3, 4 x 5, 4 heads, as an fp32 emulation of its loop order on the CPU does."""
import functools

import numpy as np
import pytest
import torch

from tests import attn_cases as ac
from tests import glue_cases as gc
from tests.guarded import SENTINEL, Guarded, GuardedBytes

pytestmark = pytest.mark.gpu
NAN = float("nan")
TAIL = 64
F16X3, F16X2, F16 = 1, 2, 3                                  # SF_PRECISION_*


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X; torch.cuda.is_available() is False")
    return torch.device("cuda:0")


def _L():
    from streamflow_amd import _lib as L
    return L


def _ids(cases):
    return [c["id"] for c in cases]


def _view(dev, shape, layout, placed, k, fill=NAN, data=None, ld=None):
    """A guard-banded [batch][rows][cols] view at the placement of glue_cases.place (operand number k: its own image stride)."""
    batch, rows, cols = shape
    ld = cols if ld is None else ld
    off, stride = gc.place(layout, rows, ld, placed, True, k)
    dtype = torch.float32 if layout == "f32" else torch.float16
    G = Guarded(dev, batch, rows, cols, off, ld, stride, fill, dtype, koct=layout == "koct", tail=TAIL)
    assert G.ptr % gc.BASE_ALIGN[layout] == 0
    return G if data is None else G.put(torch.as_tensor(np.ascontiguousarray(data)).reshape(shape))


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _call(fn, names, args, **over):
    a = dict(args, **over)
    status = fn(*[a[k] for k in names], _L().stream())
    torch.cuda.synchronize()
    return status


def _ok(status, what):
    assert status == 0, f"{what}: refused ({status}): {_L().load().sf_last_error().decode(errors='replace')}"


def _reset(*outs):
    for G in outs:
        if G is not None:
            G.buf.fill_(G.fill)


def _is_fill(G, t):
    """Elementwise: t still holds G's fill (as G's dtype rounds it)."""
    return t == torch.tensor(G.fill, dtype=t.dtype, device=t.device)


def _untouched(G):
    return bool(_is_fill(G, G.buf).all())


def _written(what, G):
    assert not bool(_is_fill(G, G.region()).any()), (what, "an output element was not written")


def _intact(what, views, spaces=()):
    for name, G in views.items():
        if G is not None:
            assert G.outside_unchanged(), (what, name, "an element outside the view changed")
    for S in spaces:
        assert S.guards_unchanged(), (what, "a guard byte of a workspace changed")


def _check_bound(entry, cls, what, got, exact, bound):
    r = np.abs(got.double().cpu().numpy().reshape(exact.shape) - exact) / bound
    worst = float(r.max())
    print(f"ATTN {entry} {cls} {what}: err/bound {worst:.3f}")
    assert worst <= 1.0, (entry, cls, what, worst, np.unravel_index(int(np.argmax(r)), r.shape))


def _check_koct_alone(entry, cls, what, got16, exact, bound):
    r = np.abs(got16.double().cpu().numpy().reshape(exact.shape) - exact) / ac.koct_alone_bound(exact, bound)
    assert float(r.max()) <= 1.0, (entry, cls, what, float(r.max()))


# ---- GMA ---------------------------------------------------------------------------------------------------------------------------------
PACK = ("qk", "qk_img_stride", "ws", "ws_bytes", "n_img", "P", "scale", "stats")
AGG = ("ws", "ws_bytes", "v", "v_img_stride", "mf", "mf_img_stride", "gamma", "out", "out_img_stride", "out_koct", "out_koct_img_stride",
       "n_img", "P", "qk_products", "use_stats")
PROJ = ("ws", "ws_bytes", "x_koct", "x_koct_img_stride", "ldx", "w_hi", "w_lo", "lda_h", "alpha", "products", "n_img", "P")
STORE = ("ws", "ws_bytes", "pbuf", "pbuf_bytes", "n_img", "P", "qk_products")
STORED = ("ws", "ws_bytes", "pbuf", "pbuf_bytes", "v", "v_f16", "v_img_stride", "mf", "mf_img_stride", "gamma", "out", "out_img_stride",
          "out_koct", "out_koct_img_stride", "n_img", "P")


class Gma:
    """The buffers of one GMA run (n images of P pixels) and its calls."""

    def __init__(self, dev, qk, v, mf, gamma, placed, out_fill=SENTINEL):
        self.lib = _L().load()
        n, _, P = qk.shape
        self.n, self.P, self.dev = n, P, dev
        self.qk = _view(dev, (n, 256, P), "f32", placed, 0, data=qk)
        self.v = _view(dev, (n, 128, P), "f32", placed, 1, data=v)
        self.v16 = _view(dev, (n, 128, P), "rows16", placed, 2, data=v)
        self.mf = _view(dev, (n, 128, P), "f32", placed, 3, data=mf)
        self.out = _view(dev, (n, 128, P), "f32", placed, 4, fill=out_fill)
        self.o16 = _view(dev, (n, 128, P), "koct", placed, 5, fill=out_fill)
        ws_bytes, p_bytes = self.lib.sf_gma_flash_ws_bytes(n, P), self.lib.sf_gma_stored_p_bytes(n, P)
        assert ws_bytes == ac.gma_ws_bytes(n, P) and p_bytes == n * (-(-P // 128) * 128) ** 2 * 2
        self.ws = GuardedBytes(dev, ws_bytes, fill=0x7F)            # (fp16 0x7F7F = NaN: a padded key that is read shows)
        self.pbuf = GuardedBytes(dev, p_bytes, fill=0x7E)
        self.gamma = torch.tensor([gamma], dtype=torch.float32, device=dev)
        self.args = dict(qk=self.qk.ptr, qk_img_stride=self.qk.stride, ws=self.ws.ptr, ws_bytes=ws_bytes, n_img=n, P=P,
                         scale=ac.GMA_SCALE, pbuf=self.pbuf.ptr, pbuf_bytes=p_bytes, mf=self.mf.ptr, mf_img_stride=self.mf.stride,
                         gamma=self.gamma.data_ptr(), out=self.out.ptr, out_img_stride=self.out.stride, out_koct=self.o16.ptr,
                         out_koct_img_stride=self.o16.stride)

    def views(self):
        return dict(qk=self.qk, v=self.v, v16=self.v16, mf=self.mf, out=self.out, o16=self.o16)

    def pack(self, stats, **over):
        _ok(_call(self.lib.sf_gma_flash_pack_qk, PACK, self.args, stats=stats, **over), "sf_gma_flash_pack_qk")
        _intact("pack_qk", self.views(), (self.ws, self.pbuf))

    def _v(self, v):
        if v == "f32":
            return dict(v=self.v.ptr, v_img_stride=self.v.stride, v_f16=0)
        if v == "f16":
            return dict(v=self.v16.ptr, v_img_stride=self.v16.stride, v_f16=1)
        return dict(v=None, v_img_stride=0, v_f16=0)

    def _result(self, what, koct, poisoned=False, nans=False):
        """nans: the inputs hold a NaN, so out may: the k-octet copy is then NaN at exactly the elements where out is (fp16(NaN) has no
        one bit pattern) and bitwise fp16(out) at every other."""
        _intact(what, self.views(), (self.ws, self.pbuf))
        out = self.out.region().clone()
        if poisoned:
            assert bool(torch.isnan(out).all()), (what, "stale state must poison every output element")
        else:
            _written(what, self.out)
        if koct:
            o16 = self.o16.region().clone()
            if poisoned:
                assert bool(torch.isnan(o16).all()), what
            elif nans:
                nan = torch.isnan(out)
                assert bool(torch.equal(torch.isnan(o16), nan)), (what, "the k-octet copy is NaN at other elements than out")
                assert _same(o16.masked_fill(nan, 0), out.masked_fill(nan, 0).half()), (what, "the k-octet copy is not fp16(out) of the same launch")
            else:
                assert _same(o16, out.half()), (what, "the k-octet copy is not fp16(out) of the same launch")
        else:
            assert _untouched(self.o16), (what, "out_koct == NULL, yet the k-octet buffer changed")
        return out

    def aggregate(self, qkp, use_stats, v="f32", koct=True, poisoned=False, nans=False):
        _reset(self.out, self.o16)
        fn = self.lib.sf_gma_flash_aggregate_f16v if v == "f16" else self.lib.sf_gma_flash_aggregate
        over = {} if koct else dict(out_koct=None, out_koct_img_stride=0)
        what = f"aggregate qkp={qkp} stats={use_stats} v={v}"
        _ok(_call(fn, AGG, dict(self.args, **self._v(v)), qk_products=qkp, use_stats=use_stats, **over), what)
        return self._result(what, koct, poisoned, nans)

    def store_p(self, qkp):
        _ok(_call(self.lib.sf_gma_flash_store_p, STORE, self.args, qk_products=qkp), "sf_gma_flash_store_p")
        _intact("store_p", self.views(), (self.ws, self.pbuf))

    def stored(self, v="f32", koct=True, poisoned=False, nans=False):
        _reset(self.out, self.o16)
        over = {} if koct else dict(out_koct=None, out_koct_img_stride=0)
        _ok(_call(self.lib.sf_gma_stored_aggregate, STORED, dict(self.args, **self._v(v)), **over), "sf_gma_stored_aggregate")
        return self._result(f"stored v={v}", koct, poisoned, nans)


def _pipe(monkeypatch, value):
    """SF_FLASH_PIPE: '0' the round-5 kernel, '2' the pipelined kernel for every product count, None the default choice."""
    if value is None:
        monkeypatch.delenv("SF_FLASH_PIPE", raising=False)
    else:
        monkeypatch.setenv("SF_FLASH_PIPE", value)


def _gma_forms(G, qkp, monkeypatch, first):
    """Every form of one product count on the buffers of G: {form: out}."""
    r = {}
    if first:
        G.pack(0)                                                 # (no statistics: the online form must not need them)
    else:
        G.pack(qkp)
    r["online"] = G.aggregate(qkp, 0)
    if first:
        G.pack(qkp)
    _pipe(monkeypatch, "0")
    r["stats"] = G.aggregate(qkp, 1)
    _pipe(monkeypatch, "2")
    r["pipe"] = G.aggregate(qkp, 1)
    _pipe(monkeypatch, None)
    r["nokoct"] = G.aggregate(qkp, 1, koct=False)
    G.store_p(qkp)
    r["stored"] = G.stored()
    if qkp <= 2:
        r["f16v"] = G.aggregate(qkp, 1, v="f16")
        r["stored_f16v"] = G.stored(v="f16")
    return r


# the contiguous batch of three first (the base), the placed batch, then every image alone: image 0 in both layouts, 1 placed, 2 contiguous
SETUPS = ((None, False), (None, True), (0, False), (0, True), (1, True), (2, False))


@pytest.mark.parametrize("case", ac.gma_cases(), ids=_ids(ac.gma_cases()))
def test_gma(dev, case, monkeypatch):
    P, fam = case["P"], case["family"]
    qk, v, mf = ac.gma_inputs(P, 3, fam, case["seed"])
    gamma = ac.gma_gamma(fam)
    exact, bound, _ = ac.gma_reference(qk, v, mf, gamma)
    res = {}
    for z, placed in SETUPS:                                      # z: the batch, or image z alone
        sl = slice(0, 3) if z is None else slice(z, z + 1)
        G = Gma(dev, qk[sl], v[sl], mf[sl], gamma, placed)
        for qkp in ac.GMA_PRODUCTS:
            res[(z, placed, qkp)] = _gma_forms(G, qkp, monkeypatch, first=qkp == 1)
    for qkp in ac.GMA_PRODUCTS:
        base = res[(None, False, qkp)]
        for form in ("pipe", "nokoct", "stored", "f16v", "stored_f16v"):
            if form in base:
                assert _same(base[form], base["stats"]), (case["id"], qkp, form, "not bitwise the statistics form of the round-5 kernel")
        for form, out in base.items():
            for z, placed in SETUPS[1:]:
                want = out if z is None else out[z:z + 1]
                assert _same(res[(z, placed, qkp)][form], want), (case["id"], qkp, form, z, placed, "differs from the contiguous batch")
        for form in ("online", "stats"):
            _check_bound("gma_flash_aggregate", f"qkp{qkp}-{form}", case["id"], base[form], exact, bound[qkp])
            if fam == "gamma0":                                   # attn.hip:441: mf + (0 * st_inv) * o with o finite, or mf + 0 + 0 in the combine
                assert bool(torch.equal(base[form].cpu(), torch.from_numpy(mf))), (case["id"], qkp, form, "gamma = 0: out must be mf")


@functools.lru_cache(maxsize=None)
def _split_reference():
    qk, v, mf = ac.gma_split_inputs()
    exact, bound, _ = ac.gma_reference(qk, v, mf, ac.GMA_GAMMA)
    return qk, v, mf, exact, bound


@pytest.mark.parametrize("n", ac.GMA_SPLIT_N)
def test_gma_both_sides_of_the_key_split(dev, n, monkeypatch):
    """P = 385 (Ppad = 512): 95 images split the key range (with the combine pass), 96 do not.  Image z of the run is image z % 4 of
    four distinct ones (one per family): the reference runs four images, and every repeat must be bitwise its first occurrence."""
    qk, v, mf, exact, bound = _split_reference()
    B, P = ac.GMA_SPLIT_BASE, ac.GMA_SPLIT_P
    rep = lambda a: np.concatenate([a] * (-(-n // B)))[:n]      # noqa: E731
    lib = _L().load()
    assert (lib.sf_gma_flash_ws_bytes(n, P) > n * (5 * 256 * 512 + 8 * 512 + 16)) == ac.use_key_split(n, P) == (n == 95)
    res = {}
    for placed in (False, True):
        G = Gma(dev, rep(qk), rep(v), rep(mf), ac.GMA_GAMMA, placed)
        for qkp in ac.GMA_PRODUCTS:
            res[(placed, qkp)] = _gma_forms(G, qkp, monkeypatch, first=qkp == 1)
        del G
    for qkp in ac.GMA_PRODUCTS:
        r = res[(False, qkp)]
        for form, out in r.items():
            if form not in ("online", "stats"):
                assert _same(out, r["stats"]), (n, qkp, form, "not bitwise the statistics form of the round-5 kernel")
            assert _same(res[(True, qkp)][form], out), (n, qkp, form, "placed run differs from the contiguous run")
            for z in range(B, n):
                assert _same(out[z], out[z % B]), (n, qkp, form, z, "a repeated image differs from its first occurrence")
            if form in ("online", "stats"):
                _check_bound("gma_flash_aggregate", f"qkp{qkp}-{form}", f"P385-n{n}", out[:B], exact, bound[qkp])


@pytest.mark.parametrize("P", ac.GMA_P)
@pytest.mark.parametrize("products", [1, 2])
def test_gma_project_v(dev, P, products):
    """sf_gma_flash_project_v with ldx > P: v = alpha (w_hi [+ w_lo]) x is exact in fp32 for these operands (attn_cases.project_v_inputs),
    so the aggregates behind it (v == NULL) are bitwise the ones fed with that v as fp32 planes -- the batch and every image alone."""
    x, w_hi, w_lo, alpha = ac.project_v_inputs(P, 3, 4000 + P)
    v = alpha * np.einsum("dc,ncp->ndp", w_hi + (w_lo if products == 2 else 0.0), x)
    qk, _, mf = ac.gma_inputs(P, 3, "randn", 4100 + P)
    exact, bound, _ = ac.gma_reference(qk, v, mf, ac.GMA_GAMMA, products=(1,))
    lib = _L().load()
    planes = lambda w: np.ascontiguousarray(w.reshape(128, 16, 8).transpose(1, 0, 2)).reshape(1, 2048, 8)      # noqa: E731  [c / 8][d][8]
    ref = {}
    for z, placed in SETUPS:
        sl = slice(0, 3) if z is None else slice(z, z + 1)
        n = sl.stop - sl.start
        G = Gma(dev, qk[sl], v[sl], mf[sl], ac.GMA_GAMMA, placed)
        G.pack(1)
        want = G.aggregate(1, 1)
        G.store_p(1)
        assert _same(G.stored(), want)
        ldx = P + (5 if placed else 0)
        X = _view(dev, (n, 128, P), "koct", placed, 6, data=x[sl], ld=ldx)
        WH = _view(dev, (1, 2048, 8), "rows16", False, 0, data=planes(w_hi))
        WL = _view(dev, (1, 2048, 8), "rows16", False, 0, data=planes(w_lo))
        G.v.buf.fill_(NAN)                                        # the fp32 planes are not an input any more
        args = dict(G.args, x_koct=X.ptr, x_koct_img_stride=X.stride, ldx=ldx, w_hi=WH.ptr, w_lo=WL.ptr if products == 2 else None,
                    lda_h=128, alpha=alpha, products=products)
        _ok(_call(lib.sf_gma_flash_project_v, PROJ, args), "sf_gma_flash_project_v")
        _intact("project_v", dict(G.views(), x=X, wh=WH, wl=WL), (G.ws, G.pbuf))
        got = G.aggregate(1, 1, v=None)
        assert _same(got, want), (P, products, z, placed, "project_v + aggregate differs from the aggregate of the exact v planes")
        assert _same(G.stored(v=None), want)
        ref[(z, placed)] = got
    base = ref[(None, False)]
    for (z, placed), got in ref.items():
        assert _same(got, base if z is None else base[z:z + 1]), (P, products, z, placed, "differs from the contiguous batch")
    _check_bound("gma_flash_project_v", f"products{products}", f"P{P}", base, exact, bound[1])


STALE = ("other_P_same_Ppad", "other_product_count", "stored_without_store_p", "use_stats_without_stats")


@pytest.mark.parametrize("P", [193, 386])
@pytest.mark.parametrize("state", STALE)
def test_gma_stale_state_poisons_every_output(dev, P, state, monkeypatch):
    """The header of ws (attn.hip:62-63, :241, :496, :728): statistics or stored weights that do not belong to this call give NaN in
    every output element, fp32 and k-octet, in the unsplit (P = 193) and the key-split (P = 386) form, and nothing else is written.
    (The other P of the first state is P - 1: the same Ppad, so the same workspace layout, and no read past the operand.)"""
    qk, v, mf = ac.gma_inputs(P, 3, "randn", 4200 + P)
    G = Gma(dev, qk, v, mf, ac.GMA_GAMMA, placed=True)
    qkp = 2 if state == "other_product_count" else 1
    if state == "other_P_same_Ppad":
        G.pack(1, P=P - 1)
    elif state == "use_stats_without_stats":
        G.pack(0)
    else:
        G.pack(1)
    for pipe in ("0", "2"):
        _pipe(monkeypatch, pipe)
        if state != "stored_without_store_p":
            G.aggregate(qkp, 1, poisoned=True)
    _pipe(monkeypatch, None)
    if state != "stored_without_store_p":
        G.store_p(qkp)
    G.stored(poisoned=True)
    if state == "stored_without_store_p":                         # ... and the statistics themselves were fine
        assert bool(torch.isfinite(G.aggregate(1, 1)).all())


@pytest.mark.parametrize("P", [129, 385])
def test_gma_non_finite_inputs_stay_where_they_are(dev, P, monkeypatch):
    """A NaN in mf shows at exactly that element; a NaN in one query leaves every other query finite and within the bound -- in out, and
    in the k-octet copy of the same launch (Gma._result: written everywhere, NaN where out is, bitwise fp16(out) elsewhere)."""
    qk, v, mf = ac.gma_inputs(P, 3, "randn", 4300 + P)
    exact, bound, _ = ac.gma_reference(qk, v, mf, ac.GMA_GAMMA, products=(1, 3))
    mfn, qkn = mf.copy(), qk.copy()
    mfn[1, 5, P - 1] = NAN
    qkn[1, 3, P // 2] = NAN
    for what, G in (("mf", Gma(dev, qk, v, mfn, ac.GMA_GAMMA, True)), ("q", Gma(dev, qkn, v, mf, ac.GMA_GAMMA, True))):
        for qkp in (1, 3):
            G.pack(qkp)
            res = {}
            for form, pipe in (("online", None), ("stats", "0"), ("pipe", "2")):
                _pipe(monkeypatch, pipe)
                res[form] = G.aggregate(qkp, int(form != "online"), nans=True)
            _pipe(monkeypatch, None)
            G.store_p(qkp)
            res["stored"] = G.stored(nans=True)
            for form, out in res.items():
                bad = torch.isnan(out).cpu().numpy()
                want = np.zeros_like(bad)
                if what == "mf":
                    want[1, 5, P - 1] = True
                    assert np.array_equal(bad, want), (what, qkp, form, "NaN elsewhere than at the NaN of mf")
                else:
                    want[1, :, P // 2] = True
                    assert not np.any(bad & ~want), (what, qkp, form, "a NaN query reached another query")
                keep = ~want
                got = out.double().cpu().numpy()
                assert np.all(np.abs(got - exact)[keep] <= bound[qkp][keep]), (what, qkp, form)


# ---- the window cores ------------------------------------------------------------------------------------------------------------------------
WIN = ("qkv", "qkv_img_stride", "bias", "out", "out_img_stride", "n_img", "C", "heads", "H", "W", "ws")
WINM = ("qkv", "qkv_img_stride", "qkv_koct", "bias", "out", "out_img_stride", "out_koct", "out_koct_img_stride", "n_img", "C", "heads",
        "H", "W", "ws", "precision")
WIN_RUNS = (("fp32", None, 0), ("x3", F16X3, 0), ("x1", F16X2, 0), ("x1", F16, 0), ("koct", F16X2, 1), ("koct", F16, 1))


def _out_modes(lib_call, out, o16, what, entry):
    """Run the three output requests of an *_mfma core: {mode: (out or None, koct or None)}, with the identities between them."""
    got = {}
    for mode in ac.OUT_MODES:
        _reset(out, o16)
        over = {}
        if mode == "koct":
            over.update(out=None, out_img_stride=0)
        if mode == "out":
            over.update(out_koct=None, out_koct_img_stride=0)
        _ok(lib_call(**over), f"{entry} {what} {mode}")
        if mode != "koct":
            _written((what, mode), out)
        else:
            assert _untouched(out), (what, "out == NULL, yet the fp32 buffer changed")
        if mode != "out":
            _written((what, mode), o16)
        else:
            assert _untouched(o16), (what, "out_koct == NULL, yet the k-octet buffer changed")
        got[mode] = (out.region().clone() if mode != "koct" else None, o16.region().clone() if mode != "out" else None)
    assert _same(got["both"][0], got["out"][0]) and _same(got["both"][1], got["koct"][1]), (what, "the output requests disagree")
    assert _same(got["both"][1], got["both"][0].half()), (what, "the k-octet copy is not fp16(out) of the same launch")
    return got


@pytest.mark.parametrize("case", ac.win_cases(), ids=_ids(ac.win_cases()))
def test_window_attn(dev, case):
    lib = _L().load()
    ws, H, W = case["ws"], case["H"], case["W"]
    N = H * W
    for heads in ac.WIN_HEADS:
        C = heads * 32
        data = {0: ac.window_inputs(3, heads, H, W, case["seed"] + heads), 1: ac.window_inputs(3, heads, H, W, case["seed"] + heads, koct=True)}
        ref = {0: ac.window_reference(*data[0], heads, H, W, ws, ["fp32", "x3", "x1"]), 1: ac.window_reference(*data[1], heads, H, W, ws, ["koct"])}
        res = {}
        for z, placed in SETUPS:
            sl = slice(0, 3) if z is None else slice(z, z + 1)
            n = sl.stop - sl.start
            views = {}
            for koct_in in (0, 1):
                views[koct_in] = _view(dev, (n, 3 * C, N), "koct" if koct_in else "f32", placed, koct_in, data=data[koct_in][0][sl])
                views[2 + koct_in] = torch.from_numpy(data[koct_in][1]).to(dev)
            out = _view(dev, (n, C, N), "f32", placed, 2, fill=SENTINEL)
            o16 = _view(dev, (n, C, N), "koct", placed, 3, fill=SENTINEL)
            for cls, prec, koct_in in WIN_RUNS:
                Q = views[koct_in]
                args = dict(qkv=Q.ptr, qkv_img_stride=Q.stride, qkv_koct=koct_in, bias=views[2 + koct_in].data_ptr(), out=out.ptr,
                            out_img_stride=out.stride, out_koct=o16.ptr, out_koct_img_stride=o16.stride, n_img=n, C=C, heads=heads, H=H,
                            W=W, ws=ws, precision=prec)
                what = (case["id"], heads, z, placed, cls, prec)
                if prec is None:
                    _reset(out, o16)
                    _ok(_call(lib.sf_window_attn, WIN, args), what)
                    _written(what, out)
                    got = {"out": (out.region().clone(), None)}
                else:
                    got = _out_modes(lambda **o: _call(lib.sf_window_attn_mfma, WINM, args, **o), out, o16, what, "sf_window_attn_mfma")
                _intact(what, dict(qkv=Q, out=out, o16=o16))
                res[(z, placed, cls, prec)] = got
        for cls, prec, koct_in in WIN_RUNS:
            base = res[(None, False, cls, prec)]
            exact, bound, _ = ref[koct_in]
            for mode, (o, o16) in base.items():
                for t, idx in ((o, 0), (o16, 1)):
                    if t is None:
                        continue
                    for z, placed in SETUPS[1:]:
                        assert _same(res[(z, placed, cls, prec)][mode][idx], t if z is None else t[z:z + 1]), \
                            (case["id"], heads, cls, prec, mode, z, placed, "differs from the contiguous batch")
            entry = "window_attn" if prec is None else f"window_attn_mfma-p{prec}"
            _check_bound(entry, cls, f"{case['id']}-h{heads}", base["out"][0], exact, bound[cls])
            if prec is not None:
                _check_koct_alone(entry, cls, case["id"], base["koct"][1], exact, bound[cls])
        for koct_in, cls in ((0, "x1"), (1, "koct")):             # F16X2 and F16 are one arithmetic class (the header: one product)
            assert _same(res[(None, False, cls, F16X2)]["out"][0], res[(None, False, cls, F16)]["out"][0]), (case["id"], heads, cls)


# ---- the sub-sample cores ------------------------------------------------------------------------------------------------------------------------
SUB = ("q", "q_img_stride", "kv", "kv_img_stride", "out", "out_img_stride", "n_img", "C", "heads", "N", "M")
SUBM = ("q", "q_img_stride", "kv", "kv_img_stride", "out", "out_img_stride", "out_koct", "out_koct_img_stride", "n_img", "C", "heads", "N", "M",
        "ws", "ws_bytes", "precision")
SUB_RUNS = (("fp32", None), ("x3", F16X3), ("x1", F16X2), ("x1", F16))


@pytest.mark.parametrize("case", ac.sub_cases(), ids=_ids(ac.sub_cases()))
def test_subsample_attn(dev, case):
    lib = _L().load()
    N, M, heads = case["N"], case["M"], case["heads"]
    C = heads * 32
    q, kv = ac.subsample_inputs(3, heads, N, M, case["seed"])
    exact, bound, _ = ac.subsample_reference(q, kv, heads, list(ac.SUB_CLASSES))
    res = {}
    for z, placed in SETUPS:
        sl = slice(0, 3) if z is None else slice(z, z + 1)
        n = sl.stop - sl.start
        Q = _view(dev, (n, C, N), "f32", placed, 0, data=q[sl])
        KV = _view(dev, (n, 2 * C, M), "f32", placed, 1, data=kv[sl])
        out = _view(dev, (n, C, N), "f32", placed, 2, fill=SENTINEL)
        o16 = _view(dev, (n, C, N), "koct", placed, 3, fill=SENTINEL)
        ws_bytes = lib.sf_subsample_attn_ws_bytes(n, heads, M)
        assert ws_bytes == n * heads * -(-M // 32) * 8192
        S = GuardedBytes(dev, ws_bytes, fill=0x7E)            # (fp16 0x7E7E = NaN: every fragment that is read must have been packed)
        args = dict(q=Q.ptr, q_img_stride=Q.stride, kv=KV.ptr, kv_img_stride=KV.stride, out=out.ptr, out_img_stride=out.stride,
                    out_koct=o16.ptr, out_koct_img_stride=o16.stride, n_img=n, C=C, heads=heads, N=N, M=M, ws=S.ptr, ws_bytes=ws_bytes)
        for cls, prec in SUB_RUNS:
            what = (case["id"], z, placed, cls, prec)
            if prec is None:
                _reset(out, o16)
                _ok(_call(lib.sf_subsample_attn, SUB, args), what)
                _written(what, out)
                got = {"out": (out.region().clone(), None)}
            else:
                S.view().fill_(0x7E)
                got = _out_modes(lambda **o: _call(lib.sf_subsample_attn_mfma, SUBM, dict(args, precision=prec), **o), out, o16, what,
                                 "sf_subsample_attn_mfma")
            _intact(what, dict(q=Q, kv=KV, out=out, o16=o16), (S,))
            res[(z, placed, cls, prec)] = got
    for cls, prec in SUB_RUNS:
        base = res[(None, False, cls, prec)]
        for mode, (o, o16) in base.items():
            for t, idx in ((o, 0), (o16, 1)):
                if t is None:
                    continue
                for z, placed in SETUPS[1:]:
                    assert _same(res[(z, placed, cls, prec)][mode][idx], t if z is None else t[z:z + 1]), \
                        (case["id"], cls, prec, mode, z, placed, "differs from the contiguous batch")
        entry = "subsample_attn" if prec is None else f"subsample_attn_mfma-p{prec}"
        _check_bound(entry, cls, case["id"], base["out"][0], exact, bound[cls])
        if prec is not None:
            _check_koct_alone(entry, cls, case["id"], base["koct"][1], exact, bound[cls])
    assert _same(res[(None, False, "x1", F16X2)]["out"][0], res[(None, False, "x1", F16)]["out"][0])


# ---- refusals: every argument check of these entry points, on the host; nothing is launched ------------------------------------------------------
BIG = 1 << 62


def _refusal_setup(dev, entry):
    """((function, argument names), valid arguments, outputs and workspaces a refused call must leave bitwise alone, what must stay alive)."""
    lib = _L().load()
    if entry in ("pack_qk", "aggregate", "aggregate_f16v", "project_v", "store_p", "stored_aggregate"):
        P, n = 65, 2
        qk, v, mf = ac.gma_inputs(P, n, "randn", 5000)
        G = Gma(dev, qk, v, mf, ac.GMA_GAMMA, placed=True)
        X = _view(dev, (n, 128, P), "koct", True, 6, data=np.zeros((n, 128, P)), ld=P + 5)
        Wt = _view(dev, (1, 2048, 8), "rows16", False, 0, data=np.zeros((1, 2048, 8)))
        args = dict(G.args, stats=1, qk_products=1, use_stats=0, x_koct=X.ptr, x_koct_img_stride=X.stride, ldx=P + 5, w_hi=Wt.ptr,
                    w_lo=Wt.ptr, lda_h=128, alpha=1.0, products=2, **G._v("f16" if entry == "aggregate_f16v" else "f32"))
        fn, names = {"pack_qk": (lib.sf_gma_flash_pack_qk, PACK), "aggregate": (lib.sf_gma_flash_aggregate, AGG),
                     "aggregate_f16v": (lib.sf_gma_flash_aggregate_f16v, AGG), "project_v": (lib.sf_gma_flash_project_v, PROJ),
                     "store_p": (lib.sf_gma_flash_store_p, STORE), "stored_aggregate": (lib.sf_gma_stored_aggregate, STORED)}[entry]
        return (fn, names), args, [G.out, G.o16], [G.ws, G.pbuf], (G, X, Wt)
    heads, n = 4, 2
    C = heads * 32
    if entry in ("window_attn", "window_attn_mfma"):
        H, W, ws = 3, 5, 2
        qkv, bias = ac.window_inputs(n, heads, H, W, 5001, koct=True)
        koct = entry == "window_attn_mfma"
        Q = _view(dev, (n, 3 * C, H * W), "koct" if koct else "f32", True, 0, data=qkv)
        b = torch.from_numpy(bias).to(dev)
        out = _view(dev, (n, C, H * W), "f32", True, 2, fill=SENTINEL)
        o16 = _view(dev, (n, C, H * W), "koct", True, 3, fill=SENTINEL)
        args = dict(qkv=Q.ptr, qkv_img_stride=Q.stride, qkv_koct=int(koct), bias=b.data_ptr(), out=out.ptr, out_img_stride=out.stride,
                    out_koct=o16.ptr, out_koct_img_stride=o16.stride, n_img=n, C=C, heads=heads, H=H, W=W, ws=ws, precision=F16X2)
        return (lib.sf_window_attn_mfma, WINM) if koct else (lib.sf_window_attn, WIN), args, [out, o16], [], (Q, b)
    N, M = 33, 40
    q, kv = ac.subsample_inputs(n, heads, N, M, 5002)
    Q, KV = _view(dev, (n, C, N), "f32", True, 0, data=q), _view(dev, (n, 2 * C, M), "f32", True, 1, data=kv)
    out = _view(dev, (n, C, N), "f32", True, 2, fill=SENTINEL)
    o16 = _view(dev, (n, C, N), "koct", True, 3, fill=SENTINEL)
    ws_bytes = lib.sf_subsample_attn_ws_bytes(n, heads, M)
    S = GuardedBytes(dev, ws_bytes)
    args = dict(q=Q.ptr, q_img_stride=Q.stride, kv=KV.ptr, kv_img_stride=KV.stride, out=out.ptr, out_img_stride=out.stride,
                out_koct=o16.ptr, out_koct_img_stride=o16.stride, n_img=n, C=C, heads=heads, N=N, M=M, ws=S.ptr, ws_bytes=ws_bytes,
                precision=F16X3)
    return ((lib.sf_subsample_attn_mfma, SUBM) if entry == "subsample_attn_mfma" else (lib.sf_subsample_attn, SUB)), args, [out, o16], [S], (Q, KV)


def _null(*names):
    return [(f"null_{k}", lambda a, k=k: {k: None}) for k in names]


_DIMS_GMA = [("n_img_0", lambda a: dict(n_img=0)), ("P_0", lambda a: dict(P=0)), ("n_img_65536", lambda a: dict(n_img=65536, ws_bytes=BIG, pbuf_bytes=BIG))]
_WS = [("ws_one_byte_short", lambda a: dict(ws_bytes=a["ws_bytes"] - 1)), ("ws_misaligned", lambda a: dict(ws=a["ws"] + 8, ws_bytes=BIG))]
_QKP = [("qk_products_0", lambda a: dict(qk_products=0)), ("qk_products_4", lambda a: dict(qk_products=4))]
_KOCT = [("out_koct_misaligned", lambda a: dict(out_koct=a["out_koct"] + 8)),
         ("out_koct_stride_not_octets", lambda a: dict(out_koct_img_stride=a["out_koct_img_stride"] + 4))]
_PBUF = [("pbuf_one_byte_short", lambda a: dict(pbuf_bytes=a["pbuf_bytes"] - 1)), ("pbuf_misaligned", lambda a: dict(pbuf=a["pbuf"] + 8, pbuf_bytes=BIG))]
_HEADS = [("heads_2", lambda a: dict(heads=2, C=64)), ("heads_6", lambda a: dict(heads=6, C=192)), ("C_not_32_heads", lambda a: dict(C=a["C"] + 32))]
_WSIZE = [("ws_1", lambda a: dict(ws=1)), ("ws_8", lambda a: dict(ws=8))]
REFUSALS = {
    "pack_qk": [("stats_4", lambda a: dict(stats=4)), ("stats_negative", lambda a: dict(stats=-1))] + _null("qk", "ws") + _DIMS_GMA + _WS +
               [("image_too_large", lambda a: dict(P=1 << 22, ws_bytes=BIG))],
    "aggregate": _KOCT + _null("ws", "mf", "gamma", "out") + _DIMS_GMA + _QKP + _WS + [("image_too_large", lambda a: dict(P=1 << 22, ws_bytes=BIG))],
    "aggregate_f16v": _KOCT[:1] + _null("out") + _QKP[:1] + _WS[:1],
    "project_v": _null("ws", "x_koct", "w_hi", "w_lo") + [("products_0", lambda a: dict(products=0)), ("products_3", lambda a: dict(products=3)),
                 ("n_img_0", lambda a: dict(n_img=0)), ("P_0", lambda a: dict(P=0)), ("n_img_65536", lambda a: dict(n_img=65536, ws_bytes=BIG)),
                 ("ldx_below_P", lambda a: dict(ldx=a["P"] - 1)),
                 ("lda_h_64", lambda a: dict(lda_h=64)), ("x_koct_misaligned", lambda a: dict(x_koct=a["x_koct"] + 8)),
                 ("w_hi_misaligned", lambda a: dict(w_hi=a["w_hi"] + 8)), ("w_lo_misaligned", lambda a: dict(w_lo=a["w_lo"] + 8)),
                 ("x_koct_stride_not_octets", lambda a: dict(x_koct_img_stride=a["x_koct_img_stride"] + 4)),
                 ("image_of_1_GiB", lambda a: dict(ldx=1 << 22))] + _WS,
    "store_p": _null("ws", "pbuf") + _DIMS_GMA + _QKP + _WS + _PBUF + [("weights_of_4_GiB", lambda a: dict(P=46400, ws_bytes=BIG, pbuf_bytes=BIG))],
    "stored_aggregate": _KOCT + _null("ws", "pbuf", "mf", "gamma", "out") + _DIMS_GMA + [("v_f16_2", lambda a: dict(v_f16=2))] + _WS + _PBUF +
                        [("weights_of_4_GiB", lambda a: dict(P=46400, ws_bytes=BIG, pbuf_bytes=BIG))],
    "window_attn": _null("qkv", "bias", "out") + [("n_img_0", lambda a: dict(n_img=0)), ("H_0", lambda a: dict(H=0)), ("W_0", lambda a: dict(W=0)),
                   ("n_img_65536", lambda a: dict(n_img=65536))] + _HEADS + _WSIZE,
    "window_attn_mfma": _null("qkv", "bias") + [("null_out_and_out_koct", lambda a: dict(out=None, out_koct=None))] + _KOCT +
                        [("n_img_0", lambda a: dict(n_img=0)), ("H_0", lambda a: dict(H=0)), ("W_0", lambda a: dict(W=0))] + _HEADS + _WSIZE +
                        [("precision_fp32", lambda a: dict(precision=0)), ("precision_7", lambda a: dict(precision=7)),
                         ("koct_input_at_f16x3", lambda a: dict(precision=F16X3)), ("koct_input_misaligned", lambda a: dict(qkv=a["qkv"] + 8)),
                         ("koct_input_stride_not_octets", lambda a: dict(qkv_img_stride=a["qkv_img_stride"] + 4))],
    "subsample_attn": _null("q", "kv", "out") + [("n_img_0", lambda a: dict(n_img=0)), ("N_0", lambda a: dict(N=0)), ("M_0", lambda a: dict(M=0)),
                      ("heads_0", lambda a: dict(heads=0, C=0)), ("C_not_32_heads", lambda a: dict(C=a["C"] + 32))],
    "subsample_attn_mfma": _null("q", "kv", "ws") + [("null_out_and_out_koct", lambda a: dict(out=None, out_koct=None))] + _KOCT +
                           [("n_img_0", lambda a: dict(n_img=0)), ("N_0", lambda a: dict(N=0)), ("M_0", lambda a: dict(M=0)),
                            ("heads_0", lambda a: dict(heads=0, C=0)), ("C_not_32_heads", lambda a: dict(C=a["C"] + 32)),
                            ("precision_fp32", lambda a: dict(precision=0)), ("precision_7", lambda a: dict(precision=7))] + _WS,
}


# label of a refusal (its start) -> a fragment of the message of the SF_REQUIRE it is aimed at
MESSAGES = (("null_", "null pointer"), ("stats_", "stats_qk_products must be"), ("qk_products_", "qk_products must be"),
            ("products_", "products must be"), ("v_f16_", "v_f16 must be"), ("out_koct_", "out_koct must be 16-byte aligned"),
            ("ws_one_byte_short", "workspace too small or misaligned"), ("ws_misaligned", "workspace too small or misaligned"),
            ("pbuf_", "pbuf must hold"), ("image_too_large", "image too large"), ("weights_of_4_GiB", "image too large"),
            ("x_koct_", "operands must be 16-byte aligned"), ("w_hi_", "operands must be 16-byte aligned"),
            ("w_lo_", "operands must be 16-byte aligned"), ("image_of_1_GiB", "operands must be 16-byte aligned"),
            ("heads_", "needs C = heads * 32"), ("C_not_32_heads", "needs C = heads * 32"), ("ws_1", "window size must be 2..7"),
            ("ws_8", "window size must be 2..7"), ("precision_", "precision must be one of"),
            ("koct_input_at_f16x3", "one-product classes only"), ("koct_input_", "k-octet qkv must be 16-byte aligned"),
            ("n_img_", "bad dims"), ("P_0", "bad dims"), ("H_0", "bad dims"), ("W_0", "bad dims"), ("N_0", "bad dims"), ("M_0", "bad dims"),
            ("ldx_below_P", "bad dims"), ("lda_h_64", "bad dims"))
ENTRY_NAME = {"pack_qk": "sf_gma_flash_pack_qk", "aggregate": "sf_gma_flash_aggregate", "aggregate_f16v": "sf_gma_flash_aggregate",
              "project_v": "sf_gma_flash_project_v", "store_p": "sf_gma_flash_store_p", "stored_aggregate": "sf_gma_stored_aggregate",
              "window_attn": "sf_window_attn:", "window_attn_mfma": "sf_window_attn_mfma", "subsample_attn": "sf_subsample_attn:",
              "subsample_attn_mfma": "sf_subsample_attn_mfma"}


def _message(label):
    return next(msg for start, msg in MESSAGES if label.startswith(start))


@pytest.mark.parametrize("entry", list(REFUSALS))
def test_refusals(dev, entry):
    """One call per SF_REQUIRE of the entry point: a non-zero status, the message of THAT check in sf_last_error(), and the
    sentinel-filled outputs, the workspaces and their guard bands bitwise untouched.  Every check is made on the host before anything
    is launched.  The arguments the changes start from are accepted first (behind the pack_qk / store_p they need), so that no case
    passes because the base call was refused already."""
    (fn, names), args, outs, spaces, keep = _refusal_setup(dev, entry)
    lib = _L().load()
    if entry in ("aggregate", "aggregate_f16v", "project_v", "store_p", "stored_aggregate"):
        keep[0].pack(1)
    if entry == "stored_aggregate":
        keep[0].store_p(1)
    _ok(_call(fn, names, args), entry)
    _reset(*outs)
    before = [S.buf.clone() for S in spaces]
    labels = [label for label, _ in REFUSALS[entry]]
    assert len(set(labels)) == len(labels)
    for label, change in REFUSALS[entry]:
        status = _call(fn, names, args, **change(args))
        assert status != 0, (entry, label, "accepted")
        msg = lib.sf_last_error().decode(errors="replace")
        assert _message(label) in msg and ENTRY_NAME[entry] in msg, (entry, label, "refused by another check", msg)
        for G in outs:
            assert _untouched(G), (entry, label, "a refused call wrote to an output")
        for S, b in zip(spaces, before):
            assert bool(torch.equal(S.buf, b)), (entry, label, "a refused call wrote to a workspace")
