#!/usr/bin/env python3
"""Generate flow_viz.npz by EXECUTING THE REFERENCE's own core/utils/flow_viz.py on the CPU.

Run in the build container only (needs /root/reference; the GPU box never sees it):

    python tests/golden/make_viz_golden.py

The reference file imports ``cv2`` and never uses it in these functions, so it is loaded over an empty in-memory module of that
name (nothing from the reference is copied into the repo).  Recorded: ``make_colorwheel()`` and the uint8 image that
``flow_to_image`` returns for every case of tests/viz_cases.py (float32 inputs, rebuilt from seeds, not stored).
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = "/root/reference"

from tests import viz_cases as vc  # noqa: E402


def load_reference():
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("ref_flow_viz", os.path.join(REF, "core", "utils", "flow_viz.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    out = {"colorwheel": ref.make_colorwheel()}
    for name in vc.CASES:
        flow = vc.field(name)
        assert flow.dtype == np.float32 and flow.shape == vc.CASES[name] + (2,)
        out[name] = ref.flow_to_image(flow, **vc.KWARGS.get(name, {}))
        assert out[name].dtype == np.uint8 and out[name].shape == vc.CASES[name] + (3,)
    ramp = vc.field("ramp")
    u, v = ramp[..., 0], ramp[..., 1]
    pos, neg = (u > 0) & (v == 0) & ~np.signbit(v), (u > 0) & (v == 0) & np.signbit(v)
    assert pos.sum() >= 128 and neg.sum() >= 128, (pos.sum(), neg.sum())      # the sign-of-zero rule cannot hide in the 1e-4
    assert (out["ramp"][pos] != out["ramp"][neg][:1]).any(axis=1).all()       # ... and the reference does colour them differently
    path = os.path.join(HERE, "flow_viz.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote flow_viz.npz  {os.path.getsize(path) / 1024:.0f} KiB  ({len(vc.CASES)} cases)")


if __name__ == "__main__":
    main()
