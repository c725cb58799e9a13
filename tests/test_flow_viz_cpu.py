"""Flow colouring on the CPU side: the wheel (package, test restatement and the kernel's table against the reference's recorded
wheel), the numpy restatement of tests/viz_cases.py against the reference's recorded images (tests/golden/flow_viz.npz, written by
tests/golden/make_viz_golden.py), loud failure without a GPU, and the argument checks of sf_flow_to_image (which run before any
device is touched)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import viz_cases as vc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from streamflow_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def test_colorwheel_equals_the_reference_wheel(golden):
    from streamflow_amd import flow_viz
    want = golden("flow_viz")["colorwheel"]
    got = flow_viz.make_colorwheel()
    assert got.shape == want.shape == (55, 3) and got.dtype == want.dtype == np.float64
    assert np.array_equal(got, want)
    assert np.array_equal(vc.make_colorwheel(), want)


def test_kernel_table_equals_the_wheel():
    """csrc/flow_viz.hip holds the wheel as a compile-time table: every entry must be make_colorwheel()'s."""
    from streamflow_amd import flow_viz
    src = open(os.path.join(REPO, "streamflow_amd", "csrc", "flow_viz.hip")).read()
    body = re.search(r"kWheel\[kWheelN \* 3\] = \{(.*?)\};", src, flags=re.S).group(1)
    table = np.array([int(t) for t in re.findall(r"\d+", body)], np.float64).reshape(-1, 3)
    assert np.array_equal(table, flow_viz.make_colorwheel())
    assert "fp contract(off)" in src


@pytest.mark.parametrize("name", list(vc.CASES))
def test_restatement_matches_the_reference_images(golden, name):
    """The checker of the GPU tests against what the reference's own flow_to_image returned (float32 input)."""
    want = golden("flow_viz")[name]
    got = vc.flow_to_image_np(vc.field(name), **vc.KWARGS.get(name, {}))
    vc.assert_image_close(got, want, name)


def test_golden_ramp_pins_the_sign_of_zero(golden):
    """At least 128 pixels with v = +0 and 128 with v = -0 at u > 0, which the reference colours differently (the wheel's one
    discontinuity): a missed sign of zero cannot hide inside the 1e-4 of the image criterion."""
    ramp, img = vc.field("ramp"), golden("flow_viz")["ramp"]
    u, v = ramp[..., 0], ramp[..., 1]
    pos, neg = (u > 0) & (v == 0) & ~np.signbit(v), (u > 0) & (v == 0) & np.signbit(v)
    assert pos.sum() >= 128 and neg.sum() >= 128
    assert (u == 0).any() and ((u < 0) & (v == 0)).any()
    row_p, row_n = np.argwhere(pos)[0][0], np.argwhere(neg)[0][0]
    differ = (img[row_p] != img[row_n]).any(axis=1)
    assert differ[u[0] > 0].all() and not differ[u[0] < 0].any()
    assert (golden("flow_viz")["zero"] == 255).all()                       # an all-zero field is white
    flipped = ramp.copy()
    flipped[..., 1] = np.where(v == 0, -v, v)                              # the criterion sees a swapped sign of zero
    worst, n, allowed = vc.image_mismatch(vc.flow_to_image_np(flipped), img)
    assert worst > 1 and n > allowed


def test_flow_to_image_raises_without_a_gpu(monkeypatch):
    """ops takes device tensors only; flow_viz moves host input to the GPU and raises where there is none."""
    from streamflow_amd import flow_viz, ops
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.flow_to_image(torch.zeros(1, 2, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flow_viz.flow_to_image(np.zeros((4, 4, 2), np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flow_viz.flow_to_image(torch.zeros(2, 4, 4))


def test_flow_to_image_rejects_bad_shapes():
    from streamflow_amd import flow_viz
    with pytest.raises(ValueError, match="expected"):
        flow_viz.flow_to_image(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(TypeError):
        flow_viz.flow_to_image([[0.0, 0.0]])


def test_abi_rejects_bad_arguments(lib):
    """Null pointers, non-positive and oversize shapes are refused with SF_ERR_BAD_ARG before any launch."""
    flows = (ctypes.c_float * 64)()
    out = (ctypes.c_uint8 * 96)()
    ws = (ctypes.c_float * 4)()
    f, o, r = ctypes.addressof(flows), ctypes.addressof(out), ctypes.addressof(ws)
    call = lib.sf_flow_to_image
    assert call(None, o, r, 1, 4, 4, -1.0, -1.0, 0, None) == -1 and b"null" in lib.sf_last_error()
    assert call(f, None, r, 1, 4, 4, -1.0, -1.0, 0, None) == -1 and b"null" in lib.sf_last_error()
    assert call(f, o, None, 1, 4, 4, -1.0, -1.0, 0, None) == -1 and b"rad_max_ws" in lib.sf_last_error()
    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4)):
        assert call(f, o, r, n, h, w, -1.0, -1.0, 0, None) == -1 and b"bad shape" in lib.sf_last_error()
    assert call(f, o, r, 1, 32768, 32768, -1.0, -1.0, 0, None) == -1 and b"too large" in lib.sf_last_error()
    assert call(f, o, r, 65536, 4, 4, -1.0, -1.0, 0, None) == -1 and b"65535" in lib.sf_last_error()
    assert call(f, o, r, 1, 4, 4, float("nan"), -1.0, 0, None) == -1 and b"NaN" in lib.sf_last_error()
