"""Write tests/golden/pil_resize.npz from Pillow: Image.resize of the RGB cases of tests/imageprep_ref.py under BILINEAR and BICUBIC, and the
app's preprocess_image flow (Image.new / paste / resize / float32(v) / float32(255)) on the one padded case.  Needs PIL; run once:

    python tools/gen_golden_imageprep.py

The inputs are not stored: the tests regenerate them from the seeds in imageprep_ref."""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import imageprep_ref as R  # noqa: E402


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for case in R.CASES:
        i, c, f = case
        if c != 3:
            continue
        _, (oh, ow) = R.SHAPES[i]
        out[R.case_id(case)] = np.array(Image.fromarray(R.case_image(case)).resize((ow, oh), R.PIL_FILTER[f]))
    (h, w, c), S = R.PREPROCESS_CASE
    img = Image.fromarray(R.make_image(h, w, c, seed=99))
    side = max(w, h)
    sq = Image.new("RGB", (side, side), (0, 0, 0))
    sq.paste(img, ((side - w) // 2, (side - h) // 2))
    u8 = np.array(sq.resize((S, S), Image.BILINEAR))
    out["preprocess"] = (u8.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)[None]
    path = os.path.join(ROOT, "tests", "golden", "pil_resize.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, Pillow {PIL.__version__}, {len(out) - 2} resize cases")


if __name__ == "__main__":
    main()
