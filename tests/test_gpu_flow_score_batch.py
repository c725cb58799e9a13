"""Sintel / KITTI scoring on the GPU: the sf_flow_score_batch kernel (csrc/flow_score_batch.hip, ops.flow_score_batch) against the
numpy restatement of tests/eval_cases.py -- 1 to 32 fields per call (33 and 49 through the wrapper's split), shapes from 1 x 1 to
436 x 1024 and KITTI's 375 x 1242, both ground-truth kinds, with and without occlusion masks, predictions as windows of buffers
filled with 7e7 (unaligned windows take the element loads), pixels exactly on (and one ulp either side of) every threshold in
every field at shifted positions.

Criterion: every count of every row equal to the restatement's of THAT field (the fields differ), the fp64 sums within 1e-8
relative (eval_cases.assert_row_matches gives the bound), two runs bitwise equal, a second call adds, the accumulator's neighbours
in a sentinel-filled buffer untouched, the host twin on the same counters, bad arguments refused before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from tests import eval_cases as ec

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FF4DEADBEEF0001                                       # a NaN payload no computation produces
GUARD = 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _guarded_acc(dev, n):
    buf = torch.full((n * ec.LEN + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=dev).view(torch.float64)
    acc = buf[GUARD:GUARD + n * ec.LEN].view(n, ec.LEN)
    acc.zero_()
    return buf, acc


def _guards_intact(buf, n):
    raw = buf.view(torch.int64).cpu().numpy()
    return bool((raw[:GUARD] == SENTINEL).all() and (raw[GUARD + n * ec.LEN:] == SENTINEL).all())


_FIELDS = {}


def _fields(h, w, kind, with_mask, n):
    """n case fields and their restated counts, computed once per (shape, kind, mask) and shared (a shorter list is a prefix)."""
    key = (h, w, kind, with_mask)
    have = _FIELDS.setdefault(key, [])
    rng = np.random.default_rng([h, w, kind == "kitti", with_mask, len(have)])
    while len(have) < n:
        pred, gt, mask = ec.make_field(rng, h, w, kind, 3 * len(have), with_mask)
        have.append((pred, gt, mask, ec.restate(pred, gt, kind, mask)))
    return have[:n]


def _upload(fields, kind, dev, top, left):
    """(windows of one 7e7-filled buffer, ground truths, masks or None) on the device."""
    n = len(fields)
    h, w = fields[0][0].shape[1:]
    wp = w + left + 8 + (-(w + left)) % 4                               # row pitch: a multiple of 4 floats
    buf = np.full((n, 2, h + top + 3, wp), 7e7, np.float32)             # padding that would wreck every score if read
    for i, f in enumerate(fields):
        buf[i, :, top:top + h, left:left + w] = f[0]
    dbuf = torch.from_numpy(buf).to(dev)
    preds = [dbuf[i, :, top:top + h, left:left + w] for i in range(n)]
    if kind == "flo":
        gts = list(torch.from_numpy(np.stack([f[1] for f in fields])).to(dev))
    else:
        gts = list(torch.from_numpy(np.stack([f[1] for f in fields]).view(np.int16)).to(dev))
    masks = None if fields[0][2] is None else list(torch.from_numpy(np.stack([f[2] for f in fields])).to(dev))
    return preds, gts, masks


SMALL = [(1, 1), (3, 5), (37, 53), (124, 188)]
CASES = [(h, w, kind, m, n) for (h, w) in SMALL for kind in ("flo", "kitti") for m in (False, True) for n in (1, 3, 24, 32)]
CASES += [(37, 53, kind, m, n) for kind in ("flo", "kitti") for m in (False, True) for n in (33, 49)]       # split into calls
CASES += [(436, 1024, "flo", True, 24), (436, 1024, "flo", False, 3), (436, 1024, "kitti", True, 3), (436, 1024, "kitti", False, 1),
          (436, 1024, "flo", False, 32),
          (375, 1242, "kitti", False, 3), (375, 1242, "kitti", True, 1), (375, 1242, "kitti", False, 24)]


@pytest.mark.parametrize("h,w,kind,with_mask,n", CASES)
def test_kernel_vs_restatement(dev, h, w, kind, with_mask, n):
    from streamflow_amd import ops, scoring
    i = CASES.index((h, w, kind, with_mask, n))
    top, left = (3 * i) % 8, (5 * i + 1) % 8                           # left 0 or 4: aligned windows (float4 loads)
    fields = _fields(h, w, kind, with_mask, n)
    preds, gts, masks = _upload(fields, kind, dev, top, left)
    accs = []
    for run in range(2):
        buf, acc = _guarded_acc(dev, n)
        ops.flow_score_batch(preds, gts, acc, kind, masks)
        torch.cuda.synchronize()
        assert _guards_intact(buf, n), "sf_flow_score_batch wrote outside the accumulator"
        accs.append(acc.cpu().numpy())
    for k in range(n):
        ec.assert_row_matches(accs[0][k], fields[k][3], f"{h}x{w} {kind} mask={with_mask} field {k} of {n} offsets {(top, left)}")
    assert accs[0].tobytes() == accs[1].tobytes(), "two runs differ"
    if h * w > 100 and n > 1:
        assert len({tuple(r[[2, 3, 5, 7]]) for r in accs[0]}) == n, "the fields must differ, or row i need not hold field i"
    if not with_mask:
        assert not accs[0][:, scoring.EVAL_OCC:].any()
    # a second call adds (x + x is exact)
    ops.flow_score_batch(preds, gts, acc, kind, masks)
    torch.cuda.synchronize()
    assert _guards_intact(buf, n)
    assert np.array_equal(acc.cpu().numpy(), 2 * accs[0], equal_nan=True)
    # the host twin fills the same counters from the same arithmetic
    for k in range(min(n, 3)):
        row = np.zeros(scoring.EVAL_LEN)
        scoring.score_host_fields(fields[k][0], fields[k][1], row, kind, fields[k][2])
        ec.assert_row_matches(row, fields[k][3], "host")
        assert (row[[0, 2, 3, 4, 5, 7, 8, 10]] == accs[0][k][[0, 2, 3, 4, 5, 7, 8, 10]]).all()


@pytest.mark.parametrize("kind", ["flo", "kitti"])
@pytest.mark.parametrize("w", [96, 94, 93])
def test_aligned_and_unaligned_views_agree(dev, kind, w):
    """The same fields through the vector loads (aligned windows and bases; w = 96, 94, 93 allow 16 / 8-byte, 8 / 4-byte and element
    loads of the ground truth) and through the element loads (prediction window at an odd column, ground truth and mask one element
    into a larger allocation): bitwise equal accumulators."""
    from streamflow_amd import ops
    h, n = 64, 3
    fields = _fields(h, w, kind, True, n)
    p1, g1, m1 = _upload(fields, kind, dev, 0, 0)
    p2, _, _ = _upload(fields, kind, dev, 1, 3)
    g2, m2 = [], []
    for g, m in zip(g1, m1):
        flat = torch.zeros(g.numel() + 1, dtype=g.dtype, device=dev)
        flat[1:] = g.reshape(-1)
        g2.append(flat[1:].view(g.shape))
        flat = torch.zeros(m.numel() + 1, dtype=m.dtype, device=dev)
        flat[1:] = m.reshape(-1)
        m2.append(flat[1:].view(m.shape))
    assert g2[0].data_ptr() % 8 != 0 and m2[0].data_ptr() % 4 != 0 and p2[0].data_ptr() % 16 != 0 and p1[0].data_ptr() % 16 == 0
    a1, a2, a3 = (torch.zeros(n, ec.LEN, dtype=torch.float64, device=dev) for _ in range(3))
    ops.flow_score_batch(p1, g1, a1, kind, m1)
    ops.flow_score_batch(p2, g2, a2, kind, m2)
    ops.flow_score_batch(p1, [g1[0], g2[1], g1[2]], a3, kind, [m2[0], m1[1], m1[2]])      # one misaligned pointer decides for all
    assert a1.cpu().numpy().tobytes() == a2.cpu().numpy().tobytes() == a3.cpu().numpy().tobytes()
    for k in range(n):
        ec.assert_row_matches(a1[k].cpu().numpy(), fields[k][3], f"{kind} w={w} field {k}")


def test_bad_arguments(dev):
    from streamflow_amd import _lib, ops, scoring
    lib = _lib.load()
    h, w, n = 4, 6, 2
    pred = torch.zeros(n, 2, h, w, device=dev)
    gt = torch.zeros(n, h, w, 2, device=dev)
    gt16 = torch.zeros(n, h, w, 3, dtype=torch.int16, device=dev)
    mask = torch.zeros(n, h, w, dtype=torch.uint8, device=dev)
    acc = torch.zeros(n, scoring.EVAL_LEN, dtype=torch.float64, device=dev)
    need = lib.sf_flow_score_batch_ws_bytes(n, h, w)
    assert need == n * 1 * scoring.EVAL_LEN * 8
    assert lib.sf_flow_score_batch_ws_bytes(24, 436, 1024) == 24 * (2048 // 24) * scoring.EVAL_LEN * 8
    for bad in ((0, h, w), (33, h, w), (1, 0, w), (1, h, -1), (1, 1 << 15, 1 << 15)):
        assert lib.sf_flow_score_batch_ws_bytes(*bad) == -1, bad
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s = _lib.stream()

    def table(preds=(pred[0].data_ptr(), pred[1].data_ptr()), gts=(gt[0].data_ptr(), gt[1].data_ptr()), masks=(None, None)):
        t = _lib.SfScoreFields()
        for i in range(n):
            t.pred[i], t.gt[i], t.mask[i] = preds[i], gts[i], masks[i]
        return t

    def call(tab=None, null_table=False, nf=n, cs=h * w, rs=w, kind=0, hh=h, ww=w, acc_p=acc.data_ptr(), ws_p=ws.data_ptr(), wsb=need):
        t = table() if tab is None else tab
        return lib.sf_flow_score_batch(None if null_table else ctypes.byref(t), nf, cs, rs, kind, hh, ww, acc_p, ws_p, wsb, s)

    assert call() == 0
    assert call(table(masks=(mask[0].data_ptr(), mask[1].data_ptr()))) == 0
    assert call(table(gts=(gt16[0].data_ptr(), gt16[1].data_ptr())), kind=1) == 0
    torch.cuda.synchronize()
    acc.zero_()
    torch.cuda.synchronize()
    g16 = gt16[0].data_ptr()
    for kw in ({"null_table": True}, {"acc_p": None}, {"ws_p": None}, {"nf": 0}, {"nf": 33}, {"nf": -1}, {"kind": 2}, {"kind": -1},
               {"hh": 0}, {"ww": -1}, {"hh": 1 << 15, "ww": 1 << 15, "rs": 1 << 15}, {"rs": w - 1}, {"cs": 0}, {"wsb": need - 8},
               {"acc_p": acc.data_ptr() + 4}, {"ws_p": ws.data_ptr() + 4, "wsb": need},
               {"tab": table(preds=(pred[0].data_ptr(), None))}, {"tab": table(gts=(None, gt[1].data_ptr()))},
               {"tab": table(masks=(mask[0].data_ptr(), None))}, {"tab": table(masks=(None, mask[1].data_ptr()))},
               {"tab": table(gts=(gt[0].data_ptr(), gt[1].data_ptr() + 2))},
               {"tab": table(gts=(g16 + 1, gt16[1].data_ptr())), "kind": 1}):
        assert call(**kw) == -1, kw                                     # SF_ERR_BAD_ARG
    assert call(table(gts=(g16 + 2, gt16[1].data_ptr())), kind=1, hh=h - 1) == 0      # 2-byte alignment is enough for 16-bit samples
    torch.cuda.synchronize()
    # the refused calls launched nothing: the accumulator they were given is still zero
    acc.zero_()
    for kw in ({"nf": 33}, {"wsb": need - 8}, {"tab": table(masks=(mask[0].data_ptr(), None))}):
        assert call(**kw) == -1
    torch.cuda.synchronize()
    assert not acc.cpu().numpy().any()
    P, G, M = list(pred), list(gt), list(mask)
    for bad in (lambda: ops.flow_score_batch([p.cpu() for p in P], G, acc), lambda: ops.flow_score_batch(P, [g.cpu() for g in G], acc),
                lambda: ops.flow_score_batch(P, G, acc.float()), lambda: ops.flow_score_batch(P, G, acc[:1]),
                lambda: ops.flow_score_batch(P, G, acc.cpu()),
                lambda: ops.flow_score_batch([p.transpose(1, 2) for p in P], G, acc),
                lambda: ops.flow_score_batch([P[0], P[1][:, :, :5]], G, acc),
                lambda: ops.flow_score_batch([P[0], pred[:, 0]], G, acc),
                lambda: ops.flow_score_batch(P, [g[:3] for g in G], acc), lambda: ops.flow_score_batch(P, list(gt16), acc),
                lambda: ops.flow_score_batch(P, G, acc, "kitti"), lambda: ops.flow_score_batch(P, G, acc, "flo", [m.float() for m in M]),
                lambda: ops.flow_score_batch(P, G, acc, "flo", [m[:3] for m in M]),
                lambda: ops.flow_score_batch(P, [g.half() for g in G], acc)):
        with pytest.raises(RuntimeError):
            bad()
    for bad in (lambda: ops.flow_score_batch(P, G[:1], acc), lambda: ops.flow_score_batch(P, G, acc, "spring"),
                lambda: ops.flow_score_batch(P, G, acc, "flo", M[:1]), lambda: ops.flow_score_batch([], [], acc)):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert not acc.cpu().numpy().any()
