"""Writes tests/golden/pil_resize.npz: what Pillow's 8-bit bilinear resize makes of seeded frames, for the resize of the host-fed data
path (video-gcp_amd/dataset.py: resize_frames_numpy, csrc/batch_assemble.hip: gcpx_resize_assemble_batch).

    python tests/golden/make_pil_resize_goldens.py          (needs Pillow; the tests do not)

The reference resizes every item with `resize_video(images, (img_sz, img_sz))` (gcp/datasets/data_loader.py:213-220); its dataset class
uses torchvision's `Resize([img_sz, img_sz])` (data_loader.py:9,124), which on a PIL image is `Image.resize(size, BILINEAR)`.  The file
holds only the OUTPUTS of `Image.fromarray(frame).resize((img_sz, img_sz), Image.BILINEAR)` and the case list; `make_input` below
regenerates each input from its seed, in the generator and in the tests alike.
"""
import os

import numpy as np

# (H_s, W_s, img_sz, seed, kind)   kind: 0 uniform random, 1 saturated 0 / 255 noise, 2 constant 0, 3 constant 255
CASES = [
    (128, 128, 32, 1, 0), (128, 128, 64, 2, 0), (128, 128, 64, 3, 1), (128, 128, 32, 4, 1),        # the reference's recording size
    (64, 64, 32, 5, 0), (48, 48, 32, 6, 0), (100, 100, 64, 7, 0), (100, 100, 64, 8, 1), (33, 33, 32, 9, 1),   # 2, 1.5, 1.5625, 1.03
    (40, 40, 64, 10, 0), (16, 16, 32, 11, 0), (16, 16, 32, 12, 1),                                 # up-sampling
    (96, 128, 32, 13, 0), (64, 128, 64, 14, 0), (64, 128, 64, 15, 1),                              # non-square; vertical pass skipped
    (128, 128, 32, 16, 2), (128, 128, 32, 17, 3), (100, 100, 64, 18, 3), (40, 40, 64, 19, 3), (48, 48, 32, 20, 3),
]


def make_input(Hs, Ws, seed, kind):
    rs = np.random.RandomState(seed)
    if kind == 0:
        return rs.randint(0, 256, size=(Hs, Ws, 3)).astype(np.uint8)
    if kind == 1:
        return (rs.randint(0, 2, size=(Hs, Ws, 3)) * 255).astype(np.uint8)
    return np.full((Hs, Ws, 3), 0 if kind == 2 else 255, dtype=np.uint8)


def main():
    import PIL
    from PIL import Image
    out = {"cases": np.array(CASES, dtype=np.int32), "pillow_version": np.array(PIL.__version__)}
    for i, (Hs, Ws, sz, seed, kind) in enumerate(CASES):
        im = Image.fromarray(make_input(Hs, Ws, seed, kind)).resize((sz, sz), Image.BILINEAR)
        out[f"out{i}"] = np.asarray(im, dtype=np.uint8)
        assert out[f"out{i}"].shape == (sz, sz, 3)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pil_resize.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(CASES)} cases, Pillow {PIL.__version__}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
