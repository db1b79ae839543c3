"""Writes tests/golden/g14_resize.npz: small uint8 images and what PIL.Image.resize makes of them, so that the GPU tests can compare
the kernel with Pillow's own bytes on a machine without Pillow.  Needs Pillow; run it from the repository root:

    python tools/gen_golden_resize.py

Per case i: in_i (H, W) or (H, W, 3) uint8, out_i = Pillow's resized image cut to the window, and a row of `meta`:
(oh, ow, filter id, top, left, h, w) with filter ids 0 box, 1 bilinear, 2 bicubic.  The cases whose resized image is 224 pixels
and more on a side keep a window of it only (the file stays small); the GPU tests compare every pixel of those with the NumPy twin.
`pillow_version` records who wrote the bytes."""
from pathlib import Path

import numpy as np
import PIL
from PIL import Image

FILTERS = ("box", "bilinear", "bicubic")
PIL_FILTERS = (Image.BOX, Image.BILINEAR, Image.BICUBIC)
OUT = Path(__file__).resolve().parent.parent / "tests" / "golden" / "g14_resize.npz"


def images(rng, shape):
    """a random image and one of 0 / 255 only (bicubic overshoots on it and reaches both ends of the clamp)"""
    return rng.integers(0, 256, shape, dtype=np.uint8), (rng.integers(0, 2, shape) * 255).astype(np.uint8)


def main():
    rng = np.random.default_rng(14)
    cases = []                                                  # (image, oh, ow, filter id, window)
    for f in range(3):
        for img in images(rng, (64, 48, 3)) + images(rng, (64, 48)):
            cases.append((img, 17, 64, f, (0, 0, 17, 64)))
    for (H, W, oh, ow) in ((9, 200, 9, 31), (200, 9, 31, 9), (5, 7, 3, 2)):
        for img in images(rng, (H, W, 3)):
            cases.append((img, oh, ow, 2, (0, 0, oh, ow)))
    for img in images(rng, (9, 2000)):
        cases.append((img, 9, 31, 2, (0, 0, 9, 31)))
    # CLIP's resize of the short side to 224: a window that starts and ends inside a tile of 64 columns and 4 rows
    for (H, W, oh, ow) in ((37, 53, 224, 320), (53, 37, 320, 224), (100, 151, 224, 338), (1, 1, 224, 224)):
        for img in images(rng, (H, W, 3)):
            cases.append((img, oh, ow, 2, (oh - 224) // 2 + 5, (ow - 224) // 2 + 70, 46, 83))
    data, meta = {}, []
    for i, c in enumerate(cases):
        img, oh, ow, f = c[:4]
        top, left, h, w = c[4] if len(c) == 5 else c[4:]
        out = np.asarray(Image.fromarray(img).resize((ow, oh), PIL_FILTERS[f]))[top:top + h, left:left + w]
        data[f"in_{i}"], data[f"out_{i}"] = img, np.ascontiguousarray(out)
        meta.append((oh, ow, f, top, left, h, w))
    data["meta"] = np.asarray(meta, np.int32)
    data["pillow_version"] = np.asarray(PIL.__version__)
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **data)
    print(f"{len(cases)} cases, {OUT.stat().st_size} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
