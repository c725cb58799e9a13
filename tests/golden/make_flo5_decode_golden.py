#!/opt/conda/bin/python3.9
"""Golden .flo5 files for the device reader (flo5_gpu.read_batch), written by the REAL h5py / libhdf5 with the reference's own call
(core/utils/frame_utils.py:46-47: one dataset 'flow', gzip, h5py's automatic chunking), so that sf_inflate and sf_flo5_assemble are
checked against chunk streams and chunk B-trees they did not produce.  tests/golden/make_flo5_golden.py's small files stay as they are;
these are large enough for automatic chunking to split the channels -- (34, 120, 1) tiles of a 272 x 480 x 2 field, (34, 60, 1) of its 136 x 240 corner, the layout of a
Spring file in small -- and for the chunk index to be a B-tree of more than one node.

Run with the interpreter that has h5py (this repository's own python has none):
    /opt/conda/bin/python3.9 tests/golden/make_flo5_decode_golden.py
Outputs (committed, data only) under tests/golden/flo5_decode/:
    auto_gzip5.flo5      the field at gzip 5, automatic chunks
    shuffle_gzip9.flo5   the same field, shuffle=True, gzip 9
    stored_gzip0.flo5    its upper-left 136 x 240 at gzip 0 (every chunk a stream of stored blocks; the whole field stored would pass the
                         repository's size limit for a committed file)
    expected.npz         `field`: the 272 x 480 x 2 array that was written (stored_gzip0 holds field[:136, :240])
The field is smooth, rounded to 1/256 px (the files stay small) and has NaN holes, as Spring marks invalid pixels."""
import os

import h5py
import numpy as np

here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "flo5_decode")
os.makedirs(here, exist_ok=True)
rng = np.random.default_rng(20261019)
h, w = 272, 480
y, x = np.mgrid[0:h, 0:w].astype(np.float64)
u = 9 * np.sin(x / 97.0 + 0.3) * np.cos(y / 61.0) + 4 * np.sin((x + y) / 29.0) + x / 200.0
v = 7 * np.cos(x / 83.0) * np.sin(y / 71.0 + 0.9) - 3 * np.cos((x - 2 * y) / 37.0) + y / 150.0
flow = (np.round(np.stack([u, v], -1) * 256) / 256).astype(np.float32)
for _ in range(12):                                               # rectangular holes, some touching the border
    cy, cx, ry, rx = rng.integers(0, h), rng.integers(0, w), rng.integers(2, 30), rng.integers(2, 50)
    flow[max(0, cy - ry):cy + ry, max(0, cx - rx):cx + rx] = np.nan
with h5py.File(os.path.join(here, "auto_gzip5.flo5"), "w") as f:   # frame_utils.py:46-47, verbatim call
    f.create_dataset("flow", data=flow, compression="gzip", compression_opts=5)
    print("auto chunks", f["flow"].chunks)
with h5py.File(os.path.join(here, "shuffle_gzip9.flo5"), "w") as f:
    f.create_dataset("flow", data=flow, compression="gzip", compression_opts=9, shuffle=True)
crop = np.ascontiguousarray(flow[:136, :240])
with h5py.File(os.path.join(here, "stored_gzip0.flo5"), "w") as f:
    f.create_dataset("flow", data=crop, compression="gzip", compression_opts=0)
    print("stored chunks", f["flow"].chunks)
np.savez_compressed(os.path.join(here, "expected.npz"), field=flow)
print({n: os.path.getsize(os.path.join(here, n)) for n in sorted(os.listdir(here))}, "h5py", h5py.__version__, "hdf5",
      h5py.version.hdf5_version)
