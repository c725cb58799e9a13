"""Case lists, float64 references and per-element bounds of tests/test_gpu_attn_kernels.py: the attention family through the C ABI --
sf_gma_flash_pack_qk / _aggregate / _aggregate_f16v / _project_v, sf_gma_flash_store_p / sf_gma_stored_aggregate (csrc/attn.hip),
sf_window_attn / _mfma, sf_subsample_attn / _mfma (csrc/encoder.hip).  Pure numpy on the CPU; tests/test_attn_cases_cpu.py pins
what is here (oracle equality, model inside the bound, wrong kernels outside it, the case sets).

One rule for all cores.  With logits l_j in log2 units, weights w_j = exp2(l_j - max), a_j = w_j / sum w, o = sum a_j v_j:

    exact  the header's formula on the unrounded inputs, float64;
    model  the same with exactly the roundings the code documents for the class under test (CLASSES), everything else exact;
    bound  per output element, the first-order sensitivity of a softmax-weighted mean:

        bound = |gamma| * 2 * [ sum_j a_j |v_j - o| ln2 dl_j  +  sum_j (e_j / sum w) (|v_j| + |o|)  +  sum_j a_j dv_j
                                + J 2^-24 (sum_j a_j |v_j| + |o|) ] + 4 ulp_fp32(|exact|)                     J = number of keys

        dl_j = sum_d (dq_d |k_dj| + |q_d| dk_dj) + D * 2^-24 sum_d |q_d k_dj|        operand rounding, fp32 accumulation (D = head dim)
        e_j  = max(eps_w w_j, 2^-25) for fp16 / hi + lo weights, 2^-24 w_j for fp32 weights
        dx   = max(eps_x |x|, 2^-25) for an operand x held as fp16 (eps 2^-11) or as an fp16 hi + lo pair (eps 2^-21), 0 for fp32

    The factor 2 covers second order and the statistics pass's row sum (rounded relative to the running maximum).  Two terms are added
    to the formula this work was specified with.  (1) J 2^-24 (sum a |v| + |o|): the second contraction and the row sum are fp32
    running sums over the J keys, each of the J - 1 additions rounds a partial sum that is at most sum_j w_j |v_j| (resp. sum_j w_j) --
    the twin of the logits' D 2^-24 term.  Next to 2^-11 weights it is nothing; for the exact fp32 cores it is the largest term: an
    fp32 emulation of window_attn_kernel's loop order misses the bound without it by 8 % at ws = 3 (4.4e-7 against 4.1e-7 at a peaked row;
    1e-10 with the two sums in float64) and is at 0.24 with it.  (2) The max(., 2^-25) in dx: an fp16 value below 2^-14 is subnormal, its spacing is 2^-24 whatever its
    size, so the lo half of a pair (|lo| <= 2^-11 |x|: subnormal for every |x| < 2^-3) carries an ABSOLUTE error of up to 2^-25 --
    with unit inputs that is a third of the 2^-21 |x| term, not a second-order effect.

CLASSES: which operand is held how (file:line of the rounding):
    gma1   q fp16, k fp16                       attn.hip:87-90 (hi planes), attn.hip:316 (one product)
    gma2   q hi + lo, k fp16                    attn.hip:311 (q_lo k_hi)
    gma3   q hi + lo, k hi + lo (no lo * lo)    attn.hip:312-315 (q_hi k_lo)
           all three: q times fp32(scale * log2 e) in fp32 first (attn.hip:87, :873); weights fp16(exp2(l - m)), subnormals kept
           (attn.hip:359-363); v fp16 (attn.hip:110, :174); row normalised by the sum of the ROUNDED weights (attn.hip:364)
    fp32   nothing rounded below fp32            encoder.hip:19-72, :77-124 (the VALU cores)
    x3     q, k, weights, v hi + lo, no lo * lo  encoder.hip:145-152, :254-258, :274-282, :303-307; row sum of the UNROUNDED weights (:278)
    x1     q, k, weights, v fp16                 encoder.hip:283-294 (row sum of the rounded weights), :460-470
    koct   q, k, v are fp16 on entry (exact); the bias tokens' k, v rounded to fp16 (encoder.hip:527-528); weights fp16 (:577-578)
"""
import math

import numpy as np

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
SUB = 2.0 ** -25                                           # half the spacing of fp16's subnormals
EPS = {"f32": 0.0, "f16": 2.0 ** -11, "split": 2.0 ** -21}
ACC = 2.0 ** -24                                           # fp32 accumulation of a logit: head dim times this, relative to sum |q_d k_dj|

CLASSES = {
    "gma1": dict(q="f16", k="f16", v="f16", w="f16"),
    "gma2": dict(q="split", k="f16", v="f16", w="f16"),
    "gma3": dict(q="split", k="split", v="f16", w="f16"),
    "fp32": dict(q="f32", k="f32", v="f32", w="f32"),
    "x3": dict(q="split", k="split", v="split", w="split"),
    "x1": dict(q="f16", k="f16", v="f16", w="f16"),
    "koct": dict(q="f32", k="f16", v="f16", w="f16"),
}
GMA_CLASS = {1: "gma1", 2: "gma2", 3: "gma3"}

# ---- case sets (asserted in tests/test_attn_cases_cpu.py) ------------------------------------------------------------------------
GMA_P = (1, 63, 64, 65, 127, 128, 129, 193, 385, 512, 513, 641)
GMA_N = (1, 3)
GMA_FAMILIES = ("randn", "sharp", "dominant", "flat", "gamma0")
GMA_PRODUCTS = (1, 2, 3)
GMA_GAMMA = 0.61
GMA_SCALE = 128 ** -0.5
GMA_SPLIT_P, GMA_SPLIT_N = 385, (95, 96)                   # Ppad = 512: split at n = 95 (4 * 95 = 380 < 384), not at 96
GMA_SPLIT_BASE = 4                                         # the 96 images repeat these (one per family: the reference runs four)
WIN_WS = (2, 3, 4, 5, 6, 7)
WIN_HEADS = (4, 8)
WIN_N = (1, 3)
WIN_CLASSES = ("fp32", "x3", "x1", "koct")
SUB_N = (1, 31, 32, 33, 127, 128, 129, 255, 256, 257)
SUB_M = (1, 31, 32, 33, 63, 64, 65, 97)
SUB_RAGGED_M, SUB_RAGGED_N = 97, 129                       # every N edge runs with this M, every M edge with this N
SUB_HEADS = (1, 4, 8)
SUB_CLASSES = ("fp32", "x3", "x1")
OUT_MODES = ("out", "koct", "both")


def win_grids(ws):
    return ((1, 1), (ws, ws), (ws + 1, 2 * ws - 1), (1, 3 * ws + 1))


def gma_cases():
    return [dict(id=f"P{P}-{fam}", P=P, family=fam, seed=1000 + 10 * i + j) for i, P in enumerate(GMA_P) for j, fam in enumerate(GMA_FAMILIES)]


def win_cases():
    return [dict(id=f"ws{ws}-{H}x{W}", ws=ws, H=H, W=W, seed=2000 + 10 * ws + g) for ws in WIN_WS for g, (H, W) in enumerate(win_grids(ws))]


def sub_cases():
    keys = [(N, SUB_RAGGED_M) for N in SUB_N] + [(SUB_RAGGED_N, M) for M in SUB_M if M != SUB_RAGGED_M]
    return [dict(id=f"N{N}-M{M}-h{SUB_HEADS[i % 3]}", N=N, M=M, heads=SUB_HEADS[i % 3], seed=3000 + i) for i, (N, M) in enumerate(keys)]


def use_key_split(n_img, P):
    """attn.hip:854, restated: the statistics forms split the key range exactly when this holds."""
    Ppad = -(-P // 128) * 128
    return Ppad // 64 >= 8 and (Ppad // 128) * n_img < 384


def gma_ws_bytes(n_img, P):
    """attn.hip:65, :71, :857-861, restated."""
    Ppad = -(-P // 128) * 128
    return n_img * (5 * 256 * Ppad + 8 * Ppad + 16) + (2 * n_img * 128 * Ppad * 4 if use_key_split(n_img, P) else 0)


# ---- roundings -------------------------------------------------------------------------------------------------------------------
def f16(x):
    """Round to nearest even to IEEE fp16, subnormals kept; returned as float64."""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def _parts(x, how):
    if how == "f32":
        return x, None
    hi = f16(x)
    return (hi, None) if how == "f16" else (hi, f16(x - hi))


def _err(x, how):
    return np.zeros_like(x) if how == "f32" else np.maximum(EPS[how] * np.abs(x), SUB)


def _werr(w, how):
    return 2.0 ** -24 * w if how == "f32" else np.maximum(EPS[how] * w, SUB)


# ---- the one core: a softmax-weighted mean ------------------------------------------------------------------------------------------
def attend(q2, k, v, classes, q2m=None, model_kv=None, wrong=None, split_at=None, chunk=32):
    """q2 [Nq][D]: queries times scale * log2 e, unrounded; k [Nk][D]; v [Nk][Dv]; float64.  q2m: q2 as the code forms it (fp32).
    model_kv: (k, v) for the model alone (a wrong kernel's view of the keys).  Returns exact [Nq][Dv], {class: bound}, {class: model};
    the bound without gamma and the ulp term.  wrong: 'ftz', 'no_klo', 'rowsum_unrounded', 'drop_second_partial' (keys >= split_at)."""
    q2, k, v = (np.asarray(t, np.float64) for t in (q2, k, v))
    l = q2 @ k.T
    w = np.exp2(l - l.max(1, keepdims=True))
    sw = w.sum(1, keepdims=True)
    a = w / sw
    o = a @ v
    absq, absk, absv = np.abs(q2), np.abs(k), np.abs(v)
    absl = absq @ absk.T
    A, T23 = [], []
    for c in classes:
        C = CLASSES[c]
        dl = _err(q2, C["q"]) @ absk.T + absq @ _err(k, C["k"]).T + q2.shape[1] * ACC * absl
        A.append(a * dl * LN2)
        e = _werr(w, C["w"]) / sw
        T23.append(e @ absv + e.sum(1, keepdims=True) * np.abs(o) + a @ _err(v, C["v"]) + k.shape[0] * ACC * (a @ absv + np.abs(o)))
    A = np.stack(A)
    T1 = np.empty((len(classes),) + o.shape)
    for s in range(0, q2.shape[0], chunk):
        D = np.abs(v[None, :, :] - o[s:s + chunk, None, :])                       # [chunk][Nk][Dv]
        T1[:, s:s + chunk] = np.matmul(A[:, s:s + chunk, None, :], D[None])[:, :, 0, :]
    bounds = {c: 2.0 * (T1[i] + T23[i]) for i, c in enumerate(classes)}
    models = {}
    qm = f32(q2) if q2m is None else np.asarray(q2m, np.float64)
    km, vm = (k, v) if model_kv is None else (np.asarray(t, np.float64) for t in model_kv)
    for c in classes:
        C = CLASSES[c]
        qh, ql = _parts(qm, C["q"])
        kh, kl = _parts(km, C["k"])
        lm = qh @ kh.T
        if ql is not None:
            lm = lm + ql @ kh.T
        if kl is not None and wrong != "no_klo":
            lm = lm + qh @ kl.T
        p = np.exp2(lm - lm.max(1, keepdims=True))
        ph, pl = _parts(p, C["w"])
        if wrong == "ftz":
            ph = np.where(ph < 2.0 ** -14, 0.0, ph)
        den = ph.sum(1, keepdims=True) if (C["w"] == "f16" and wrong != "rowsum_unrounded") else p.sum(1, keepdims=True)
        if wrong == "drop_second_partial":
            ph = ph.copy()
            ph[:, split_at:] = 0.0
        vh, vl = _parts(vm, C["v"])
        num = ph @ vh
        if pl is not None:
            num = num + pl @ vh
        if vl is not None:
            num = num + ph @ vl
        models[c] = num / den
    return o, bounds, models


# ---- GMA: out = mf + gamma * softmax(scale q k^T) v, heads = 1, dim 128 ----------------------------------------------------------------
def gma_qscale32(scale):
    """attn.hip:873: the factor q is multiplied with, formed in fp32."""
    return np.float32(scale) * np.float32(1.44269504088896340736)


def gma_reference(qk, v, mf, gamma, scale=GMA_SCALE, products=GMA_PRODUCTS, wrong=None):
    """qk [n][256][P], v, mf [n][128][P].  Returns exact [n][128][P], {products: bound}, {products: model}.
    wrong (the model alone): 'pad_key' (key < P -> key <= P: one zero key with v = 0 enters), 'drop_last_tile' (the last 64-key tile
    that holds a key), 'no_log2e', 'mf_neighbour', or one of attend()'s."""
    qk, v, mf = (np.asarray(t, np.float64) for t in (qk, v, mf))
    n, _, P = qk.shape
    classes = [GMA_CLASS[p] for p in products]
    exact = np.empty((n, 128, P))
    bound = {p: np.empty((n, 128, P)) for p in products}
    model = {p: np.empty((n, 128, P)) for p in products}
    Ppad = -(-P // 128) * 128
    for z in range(n):
        q, k, vv = qk[z, :128].T, qk[z, 128:].T, v[z].T
        q2 = q * (scale * LOG2E)                          # (the ABI's fp32 scale is 2^-25 off: inside the accumulation term)
        q2m = (q.astype(np.float32) * gma_qscale32(scale)).astype(np.float64)
        kv, kw = None, {}
        if wrong == "pad_key":
            kv = (np.vstack([k, np.zeros((1, 128))]), np.vstack([vv, np.zeros((1, 128))]))
        elif wrong == "drop_last_tile":
            keep = ((P - 1) // 64) * 64
            kv = (k[:keep], vv[:keep])
        elif wrong == "no_log2e":
            q2m = q2m / LOG2E
        elif wrong == "drop_second_partial":
            kw = dict(wrong=wrong, split_at=(Ppad // 64 // 2) * 64)
        elif wrong in ("ftz", "no_klo", "rowsum_unrounded"):
            kw = dict(wrong=wrong)
        o, bd, mo = attend(q2, k, vv, classes, q2m=q2m, model_kv=kv, **kw)
        mfm = mf[(z + 1) % n] if wrong == "mf_neighbour" else mf[z]
        exact[z] = mf[z] + gamma * o.T
        for p, c in zip(products, classes):
            bound[p][z] = abs(gamma) * bd[c].T + 4.0 * ulp32(exact[z])
            model[p][z] = mfm + gamma * mo[c].T
    return exact, bound, model


def gma_gamma(family):
    return 0.0 if family == "gamma0" else GMA_GAMMA


def gma_inputs(P, n, family, seed):
    """(qk [n][256][P], v [n][128][P], mf [n][128][P]) fp32.
    randn / gamma0: unit normal.  sharp: the project's family, half the queries times 6 (logits of +-40).
    dominant: for every third query one key (the LAST real key in image 0: next to the padding; P / 3 elsewhere) 16 to 22 log2
        units above all others -- weight 1 beside P - 1 weights in fp16's subnormal range -- with a small v at the dominant key and
        v = 8 + 8 randn elsewhere, so that the tail's mass (P 2^-19 8) is what the result is made of.
    flat: v = 2 + randn; every fourth query is zero (a row of identical logits); image 0's keys are all the same key, and every
        fourth query there is that key times a negative factor: all its logits are -19 log2 units, so a zero-padded key let into
        the row (logit 0, v = 0) would take all of it."""
    rng = np.random.default_rng(seed)
    qk = rng.standard_normal((n, 256, P))
    v = rng.standard_normal((n, 128, P))
    mf = rng.standard_normal((n, 128, P))
    if family == "sharp":
        qk[:, :128, : P // 2] *= 6.0
    elif family == "dominant":
        qmul = GMA_SCALE * LOG2E
        v[:] = 8.0 + 8.0 * v
        for z in range(n):
            js = P - 1 if z == 0 else P // 3
            ks = rng.standard_normal(128)
            qk[z, 128:] *= 0.5
            qk[z, 128:, js] = ks
            beta = 19.0 / (qmul * float(ks @ ks))
            qk[z, :128, 0::3] = 0.3 * qk[z, :128, 0::3] + beta * ks[:, None]
            v[z, :, js] = 0.05 * rng.standard_normal(128)
    elif family == "flat":
        v[:] = 2.0 + v
        qk[:, :128, 1::4] = 0.0
        k0 = qk[0, 128:, 0].copy()
        qk[0, 128:, :] = k0[:, None]
        qk[0, :128, 2::4] = (-19.0 / (GMA_SCALE * LOG2E * float(k0 @ k0))) * k0[:, None]
    return qk.astype(np.float32), v.astype(np.float32), mf.astype(np.float32)


def gma_klo_inputs(P=65, L=480.0):
    """Aimed at the lo plane of k (qk_products = 3): every query is the constant c > 0 in all 128 dims (every logit L log2 units), the
    even keys are 1 + 2^-12 in every dim and the odd keys 1 - 2^-12 -- both round to fp16(1.0), the difference lives in k_lo alone,
    all 128 rounding errors of a key have one sign -- and v is +1 at even keys, -1 at odd ones.  Exact: the logits of the two groups
    differ by L 2^-11; without k_lo they are equal."""
    c = L / (GMA_SCALE * LOG2E * 128.0)
    qk = np.empty((1, 256, P))
    qk[0, :128] = c
    qk[0, 128:, 0::2] = 1.0 + 2.0 ** -12
    qk[0, 128:, 1::2] = 1.0 - 2.0 ** -12
    v = np.empty((1, 128, P))
    v[0, :, 0::2], v[0, :, 1::2] = 1.0, -1.0
    return qk.astype(np.float32), v.astype(np.float32), np.zeros((1, 128, P), np.float32)


def gma_split_inputs():
    """The GMA_SPLIT_BASE distinct images of the n = 95 / 96 runs (image z of a run = image z % 4 of these): one per family."""
    P = GMA_SPLIT_P
    parts = [gma_inputs(P, 1, fam, 1900 + i) for i, fam in enumerate(("randn", "sharp", "dominant", "flat"))]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def project_v_inputs(P, n, seed):
    """x [n][128][P] (multiples of 2^-6 below 4: fp16 exact), w_hi, w_lo [128 d][128 c] (integers -2..2; 0 or +-2^-3) and alpha = 2^-4:
    every partial sum of W x is exact in fp32 in any order, so v = alpha (w_hi [+ w_lo]) x is THE value sf_gma_flash_project_v must
    round to fp16 -- the aggregate behind it is bitwise the one fed with these v as fp32 planes."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-255, 256, (n, 128, P)) / 64.0
    w_hi = rng.integers(-2, 3, (128, 128)).astype(np.float64)
    w_lo = rng.integers(-1, 2, (128, 128)) / 8.0
    return x, w_hi, w_lo, 2.0 ** -4


# ---- the encoder cores (head dim 32, scale 32^-0.5) --------------------------------------------------------------------------------------
ENC_QMUL = 32 ** -0.5 * LOG2E


def window_inputs(n, heads, H, W, seed, koct=False):
    """qkv [n][3C][H*W], bias [3C]; q and k times 2 (logits spread over about +-8 log2 units).  koct: qkv fp16-representable."""
    rng = np.random.default_rng(seed)
    C = heads * 32
    qkv = rng.standard_normal((n, 3 * C, H * W))
    qkv[:, : 2 * C] *= 2.0
    bias = rng.standard_normal(3 * C)
    if koct:
        qkv = f16(qkv)
    return qkv.astype(np.float32), bias.astype(np.float32)


def window_reference(qkv, bias, heads, H, W, ws, classes, wrong=None):
    """Pad the grid with bias tokens (k = v = the qkv bias) to a multiple of ws, attend inside windows, crop.
    Returns exact [n][C][H*W], {class: bound}, {class: model}.  wrong: 'pad_zero' (padding tokens with k = v = 0), 'heads_v'."""
    qkv, bias = np.asarray(qkv, np.float64), np.asarray(bias, np.float64)
    n, C = qkv.shape[0], heads * 32
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    full = np.broadcast_to(bias[None, :, None, None], (n, 3 * C, Hp, Wp)).copy()
    full[:, :, :H, :W] = qkv.reshape(n, 3 * C, H, W)
    real = np.zeros((Hp, Wp), bool)
    real[:H, :W] = True
    exact = np.empty((n, C, H, W))
    bound = {c: np.empty((n, C, H, W)) for c in classes}
    model = {c: np.empty((n, C, H, W)) for c in classes}
    for z in range(n):
        for h in range(heads):
            hv = h % 4 if wrong == "heads_v" else h
            for y0 in range(0, Hp, ws):
                for x0 in range(0, Wp, ws):
                    sl = (slice(y0, y0 + ws), slice(x0, x0 + ws))
                    r = real[sl].reshape(-1)
                    tok = lambda row0: full[(z, slice(row0, row0 + 32)) + sl].reshape(32, -1).T      # noqa: E731
                    q, k, v = tok(h * 32)[r], tok(C + h * 32), tok(2 * C + h * 32)
                    kv = None
                    if wrong == "pad_zero":
                        kv = (np.where(r[:, None], k, 0.0), np.where(r[:, None], v, 0.0))
                    elif wrong == "heads_v":
                        kv = (k, tok(2 * C + hv * 32))
                    o, bd, mo = attend(q * ENC_QMUL, k, v, classes, model_kv=kv)
                    ys, xs = np.nonzero(real[sl])
                    exact[z, h * 32:(h + 1) * 32, y0 + ys, x0 + xs] = o
                    for c in classes:
                        bound[c][z, h * 32:(h + 1) * 32, y0 + ys, x0 + xs] = bd[c]
                        model[c][z, h * 32:(h + 1) * 32, y0 + ys, x0 + xs] = mo[c]
    exact = exact.reshape(n, C, H * W)
    return (exact, {c: bound[c].reshape(n, C, H * W) + 4.0 * ulp32(exact) for c in classes},
            {c: model[c].reshape(n, C, H * W) for c in classes})


def subsample_inputs(n, heads, N, M, seed):
    """q [n][C][N], kv [n][2C][M]; q and k times 2."""
    rng = np.random.default_rng(seed)
    C = heads * 32
    q = 2.0 * rng.standard_normal((n, C, N))
    kv = rng.standard_normal((n, 2 * C, M))
    kv[:, :C] *= 2.0
    return q.astype(np.float32), kv.astype(np.float32)


def subsample_reference(q, kv, heads, classes, wrong=None):
    """softmax(q k^T / sqrt 32) v per head.  Returns exact [n][C][N], {class: bound}, {class: model}.  wrong: 'heads_v'."""
    q, kv = np.asarray(q, np.float64), np.asarray(kv, np.float64)
    n, C, N = q.shape
    exact = np.empty((n, C, N))
    bound = {c: np.empty((n, C, N)) for c in classes}
    model = {c: np.empty((n, C, N)) for c in classes}
    for z in range(n):
        for h in range(heads):
            rows = slice(h * 32, (h + 1) * 32)
            k, v = kv[z, rows].T, kv[z, C + h * 32: C + (h + 1) * 32].T
            kvm = None
            if wrong == "heads_v":
                hv = h % 4
                kvm = (k, kv[z, C + hv * 32: C + (hv + 1) * 32].T)
            o, bd, mo = attend(q[z, rows].T * ENC_QMUL, k, v, classes, model_kv=kvm)
            exact[z, rows] = o.T
            for c in classes:
                bound[c][z, rows] = bd[c].T
                model[c][z, rows] = mo[c].T
    return exact, {c: bound[c] + 4.0 * ulp32(exact) for c in classes}, model


def koct_alone_bound(exact, bound):
    """A k-octet-only output (out == NULL): one fp16 rounding of a value within `bound` of exact."""
    return bound + np.maximum(2.0 ** -11 * (np.abs(exact) + bound), SUB)
