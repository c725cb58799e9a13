"""CPU: the restatement of tests/resize_cases.py is Pillow, byte for byte; the product tables (streamflow_amd/resize.py) are the
restatement's; scaled_size; and the bound of the fp32 kernel holds for a numpy emulation of its stated arithmetic.

Pillow is imported plainly: this file pins the arithmetic of csrc/resize.hip to PIL.Image.resize through the restatement (the GPU
test compares the kernels with the restatement), and a skip would hide the pin.  The same expected outputs are committed under
tests/golden/resize/ (tools/make_resize_golden.py), so the pin does not depend on the Pillow of the machine that runs the tests."""
import hashlib
import os

import numpy as np
import pytest
from PIL import Image

from tests import resize_cases as rc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize")
PIL_FILTERS = {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def restated_u8():
    """{(case index, kind, filter): the restatement's output}: computed once, shared by the Pillow and the fixture test."""
    return {(i, kind, name): rc.resize_u8(rc.u8_input(case, kind), case[1], name)
            for i, case in enumerate(rc.U8_SHAPES) for kind in rc.U8_KINDS for name in rc.FILTER_NAMES}


@pytest.fixture(scope="module")
def restated_float():
    return {(i, name): rc.resize_float(rc.f32_input(case, 1)[0, 0], case[1], name)
            for i, case in enumerate(rc.F32_SHAPES) for name in rc.FILTER_NAMES}


def test_u8_restatement_is_pillow_bitwise(restated_u8):
    for (i, kind, name), got in restated_u8.items():
        case = rc.U8_SHAPES[i]
        img = rc.u8_input(case, kind)
        want = np.stack([np.asarray(Image.fromarray(f, "RGB").resize((case[1][1], case[1][0]), PIL_FILTERS[name])) for f in img])
        assert got.shape == want.shape and got.dtype == np.uint8
        assert np.array_equal(got, want), (rc.shape_id(case), kind, name, int((got != want).sum()))


def test_float_restatement_is_pillow_mode_f_bitwise(restated_float):
    for (i, name), got in restated_float.items():
        case = rc.F32_SHAPES[i]
        plane = rc.f32_input(case, 1)[0, 0]
        want = np.asarray(Image.fromarray(plane, "F").resize((case[1][1], case[1][0]), PIL_FILTERS[name]), np.float32)
        assert got.tobytes() == want.tobytes(), (rc.shape_id(case), name, float(np.abs(got - want).max()))


def test_restatements_match_the_committed_fixtures(restated_u8, restated_float):
    u8 = np.load(os.path.join(GOLDEN, "u8.npz"))
    stored = 0
    for (i, kind, name), got in restated_u8.items():
        case = rc.U8_SHAPES[i]
        key = f"{rc.shape_id(case)}/{kind}/{name}"
        assert str(u8[f"{rc.shape_id(case)}/{kind}.in.sha"]) == sha(rc.u8_input(case, kind)), f"{key}: the seeded input changed"
        assert str(u8[key + ".sha"]) == sha(got), key
        if key in u8.files:
            assert np.array_equal(u8[key], got), key
            stored += 1
    assert stored >= 4 * 2 * 8                                            # the small shapes are stored as bytes, not digests alone
    f32 = np.load(os.path.join(GOLDEN, "f32.npz"))
    for (i, name), got in restated_float.items():
        case = rc.F32_SHAPES[i]
        key = f"{rc.shape_id(case)}/{name}"
        assert str(f32[f"{rc.shape_id(case)}.in.sha"]) == sha(rc.f32_input(case, 1)[0, 0]), f"{key}: the seeded input changed"
        assert str(f32[key + ".sha"]) == sha(got), key
        if key in f32.files:
            assert f32[key].tobytes() == got.tobytes(), key


SIZE_PAIRS = sorted({(a, b) for (H, W), (h, w), _ in rc.U8_SHAPES for a, b in ((H, h), (W, w))}
                    | {(a, b) for (H, W), (h, w) in rc.F32_SHAPES for a, b in ((H, h), (W, w))} | {(1920, 120), (436, 224), (1024, 2048)})


def test_product_tables_equal_the_restatement():
    from streamflow_amd import resize
    assert set(resize.FILTERS) == set(rc.FILTER_NAMES) and resize.PRECISION_BITS == rc.PRECISION_BITS
    for name in rc.FILTER_NAMES:
        for a, b in SIZE_PAIRS:
            bounds, k = resize.coeff_table(a, b, name)
            wb, wk = rc.table(a, b, name)
            assert bounds.dtype == np.int32 and k.dtype == np.float64 and k.shape == wk.shape
            assert np.array_equal(bounds, wb), (name, a, b)
            assert k.tobytes() == wk.tobytes(), (name, a, b, float(np.abs(k - wk).max()))
            q = resize.quantise(k)
            assert q.dtype == np.int32 and np.array_equal(q, rc.fixed(wk)), (name, a, b)
            # every quantised row sums to 2^22 within the rounding of its taps (half a unit each)
            assert int(np.abs(q.astype(np.int64).sum(1) - (1 << 22)).max()) <= k.shape[1] / 2, (name, a, b)
            assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= a).all() and (bounds[:, 1] <= k.shape[1]).all()
    assert resize.coeff_table(1920, 120, "lanczos")[1].shape[1] == 97 == resize.MAX_KSIZE      # a 16-fold reduction, 3 lobes


def test_identity_sizes_give_the_identity_table():
    from streamflow_amd import resize
    for name in rc.FILTER_NAMES:
        for size in (1, 2, 17, 64):
            bounds, k = resize.coeff_table(size, size, name)
            q = resize.quantise(k)
            for xx in range(size):
                row = np.zeros(size, np.int64)
                row[bounds[xx, 0]:bounds[xx, 0] + bounds[xx, 1]] = q[xx, :bounds[xx, 1]]
                want = np.zeros(size, np.int64)
                want[xx] = 1 << 22
                assert np.array_equal(row, want), (name, size, xx)


def test_scaled_size():
    from streamflow_amd.resize import scaled_size
    assert scaled_size((436, 1024), scale=0.5) == (216, 512)
    assert scaled_size((2160, 3840), max_side=1280) == (720, 1280)
    assert scaled_size((240, 426), max_side=4000) == (240, 424)          # max_side never enlarges
    assert scaled_size((240, 426), scale=2) == (480, 848)
    assert scaled_size((5, 9), scale=0.1) == (8, 8) and scaled_size((100, 100), scale=0.5, multiple=32) == (64, 64)
    for hw in ((436, 1024), (375, 1242), (1080, 1920), (17, 23)):
        assert scaled_size(hw, scale=1) == tuple(max(8, 8 * round(s / 8)) for s in hw)
        last = (0, 0)
        for f in np.linspace(0.05, 3.0, 60):
            got = scaled_size(hw, scale=float(f))
            assert got[0] % 8 == 0 and got[1] % 8 == 0 and got[0] >= 8 and got[1] >= 8
            assert got[0] >= last[0] and got[1] >= last[1], (hw, f)      # monotone in the factor
            last = got
        last = (0, 0)
        for m in range(16, 2200, 97):
            got = scaled_size(hw, max_side=m)
            assert got[0] % 8 == 0 and got[1] % 8 == 0 and got[0] >= last[0] and got[1] >= last[1]
            last = got
    for bad in (dict(), dict(scale=0.5, max_side=100), dict(scale=0), dict(scale=-1.0), dict(scale=float("nan")), dict(max_side=0)):
        with pytest.raises(ValueError):
            scaled_size((100, 200), **bad)
    with pytest.raises(ValueError):
        scaled_size((0, 200), scale=1)


@pytest.mark.parametrize("case", rc.F32_SHAPES, ids=rc.shape_id)
def test_fp32_emulation_stays_within_the_bound(case):
    """The kernel's stated arithmetic (fp32 products and sums in tap order, fp32 intermediate, one final multiply) against the
    float64 result from the same fp32-rounded tables: within (T_h + T_v + 6) 2^-24 |s| A everywhere, for every filter and scale."""
    flow = rc.f32_input(case)
    for name in rc.FILTER_NAMES:
        for sx, sy in rc.F32_SCALES:
            got = rc.emulate_f32(flow, case[1], name, sx, sy).astype(np.float64)
            want = rc.resize_f64(flow, case[1], name, sx, sy)
            bound = rc.bound_f32(flow, case[1], name, sx, sy)
            assert got.shape == want.shape == bound.shape == (flow.shape[0], 2) + case[1]
            err = np.abs(got - want)
            assert (err <= bound).all(), (name, sx, sy, float((err / np.maximum(bound, 1e-300)).max()))
