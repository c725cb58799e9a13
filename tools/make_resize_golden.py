"""Generate tests/golden/resize/{u8,f32}.npz from Pillow: the expected outputs of PIL.Image.resize for the seeded inputs of
tests/resize_cases.py, so that a machine whose Pillow differs (or is missing) still pins the restatement to the same bytes.

    python tools/make_resize_golden.py

Per case and filter the file holds the expected array under "<shape>/<kind>/<filter>" when it has at most MAX_BYTES bytes, and
always its SHA-256 under "<key>.sha" (larger outputs are pinned by the digest alone); "<shape>/<kind>.in.sha" is the digest of the
seeded input, so a changed random stream is told apart from a changed resampler.  "pillow" records the version used."""
import hashlib
import os
import sys

import numpy as np
import PIL
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import resize_cases as rc  # noqa: E402

MAX_BYTES = 30000
PIL_FILTERS = {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def pil_u8(img: np.ndarray, hw, name: str) -> np.ndarray:
    """uint8 [n, H, W, 3] through PIL.Image.resize, frame by frame."""
    return np.stack([np.asarray(Image.fromarray(f, "RGB").resize((hw[1], hw[0]), PIL_FILTERS[name])) for f in img])


def pil_f32(plane: np.ndarray, hw, name: str) -> np.ndarray:
    """One float32 plane [H, W] through PIL.Image.resize in mode F."""
    return np.asarray(Image.fromarray(plane, "F").resize((hw[1], hw[0]), PIL_FILTERS[name]), np.float32)


def put(store: dict, key: str, a: np.ndarray) -> None:
    store[key + ".sha"] = np.array(sha(a))
    if a.nbytes <= MAX_BYTES:
        store[key] = a


def main() -> None:
    out = os.path.join(REPO, "tests", "golden", "resize")
    os.makedirs(out, exist_ok=True)
    u8 = {"pillow": np.array(PIL.__version__)}
    for case in rc.U8_SHAPES:
        for kind in rc.U8_KINDS:
            img = rc.u8_input(case, kind)
            u8[f"{rc.shape_id(case)}/{kind}.in.sha"] = np.array(sha(img))
            for name in rc.FILTER_NAMES:
                put(u8, f"{rc.shape_id(case)}/{kind}/{name}", pil_u8(img, case[1], name))
    np.savez_compressed(os.path.join(out, "u8.npz"), **u8)
    f32 = {"pillow": np.array(PIL.__version__)}
    for case in rc.F32_SHAPES:
        plane = rc.f32_input(case, 1)[0, 0]
        f32[f"{rc.shape_id(case)}.in.sha"] = np.array(sha(plane))
        for name in rc.FILTER_NAMES:
            put(f32, f"{rc.shape_id(case)}/{name}", pil_f32(plane, case[1], name))
    np.savez_compressed(os.path.join(out, "f32.npz"), **f32)
    for f in ("u8.npz", "f32.npz"):
        print(f, os.path.getsize(os.path.join(out, f)), "bytes")


if __name__ == "__main__":
    main()
