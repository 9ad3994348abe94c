"""Writes tests/golden/resize_lanczos.npz: Pillow's own `Image.resize((w, h), Image.LANCZOS)` of the seeded inputs of
tests/resize_ref.py (every case, both contents).  Only the outputs are stored; the inputs are regenerated from the seed.
    python tests/golden/make_golden_resize.py
Needs Pillow and numpy only; the file records the Pillow version it was written with (key `pillow_version`)."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resize_ref as R  # noqa: E402


def pillow_resize(frames, h, w):
    """uint8 [N, H, W, C] (C = 1: mode L, C = 3: mode RGB) -> uint8 [N, h, w, C]."""
    out = []
    for f in frames:
        img = Image.fromarray(f[:, :, 0] if f.shape[2] == 1 else f)
        out.append(np.asarray(img.resize((w, h), Image.LANCZOS)).reshape(h, w, f.shape[2]))
    return np.stack(out)


def main():
    data = {"pillow_version": np.array(PIL.__version__)}
    for (name, N, H, W, C, h, w), content in R.all_cases():
        data[f"{name}/{content}"] = pillow_resize(R.case_input(name, content), h, w)
    path = os.path.join(HERE, "resize_lanczos.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
