"""Writes tests/golden/png_golden.npz and tests/golden/png_host_corpus.bin (needs Pillow; run from the repository root:
``python tests/golden/make_png_golden.py``).

png_golden.npz: Pillow-written PNG streams of every colour type and bit depth Pillow writes -- 1-bit and 8-bit gray, gray +
alpha, RGB, RGBA, palette at 1, 2, 4 and 8 bits -- with and without ``transparency``, at compress_level 0, 1 and 9, and the
frames Pillow (libpng) decodes them to under the mapping of include/scannertools_hip.h: ``L`` for gray, ``convert("RGB")``
for palette and RGB, ``convert("RGBA")`` for palette / RGB with transparency and for gray + alpha.  It arbitrates that the
library's layout agrees with libpng's reader.  (Pillow writes no 2- or 4-bit gray; tests/test_png.py lets Pillow decode the
hand-written streams of those depths instead.)

png_host_corpus.bin: the streams scripts/png_host_check.cpp runs under the sanitizers -- the malformed streams of
tests/png_cases.py ('M') and a few valid ones ('V', also cut at every length there).  Format: "PNGC", then per stream one
byte 'V' or 'M', the length as 4 little-endian bytes, the bytes.
"""
import io
import os
import struct
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import png_cases  # noqa: E402

H, W = 21, 33


def pictures():
    rng = np.random.default_rng(5)
    y, x = np.mgrid[0:H, 0:W]
    smooth = ((4 * x + 6 * y)[..., None] + np.array([0, 60, 120, 200]) + rng.integers(0, 4, (H, W, 4))) & 255
    smooth = smooth.astype(np.uint8)
    out = {}
    out["L"] = (Image.fromarray(smooth[..., 0], "L"), {}, "L")
    out["L_trns"] = (Image.fromarray(smooth[..., 0], "L"), {"transparency": int(smooth[3, 3, 0])}, "L")   # ignored: 1 channel
    out["1"] = (Image.fromarray(((x + y) % 3 == 0).astype(np.uint8) * 255, "L").convert("1"), {}, "L")
    out["LA"] = (Image.fromarray(smooth[..., [0, 3]], "LA"), {}, "RGBA")
    out["RGB"] = (Image.fromarray(smooth[..., :3], "RGB"), {}, "RGB")
    flat = smooth[..., :3].copy()
    flat[5:9, 4:20] = (9, 8, 7)
    out["RGB_trns"] = (Image.fromarray(flat, "RGB"), {"transparency": (9, 8, 7)}, "RGBA")
    out["RGBA"] = (Image.fromarray(smooth, "RGBA"), {}, "RGBA")
    for bits in (1, 2, 4, 8):
        k = 1 << bits
        im = Image.fromarray(((x // 2 + y) % k).astype(np.uint8), "P")
        im.putpalette(rng.integers(0, 256, 3 * k).astype(np.uint8).tobytes())
        out["P%d" % bits] = (im, {"bits": bits}, "RGB")
        out["P%d_trns" % bits] = (im, {"bits": bits, "transparency": bytes(rng.integers(0, 256, max(1, k // 2)).astype(np.uint8))}, "RGBA")
    out["P8_trns_index"] = (out["P8"][0], {"bits": 8, "transparency": 3}, "RGBA")
    return out


def main():
    arrays, names = {}, []
    for name, (im, kw, mode) in pictures().items():
        for level in (0, 1, 9):
            buf = io.BytesIO()
            im.save(buf, "PNG", compress_level=level, **kw)
            data = buf.getvalue()
            frame = np.asarray(Image.open(io.BytesIO(data)).convert(mode))
            key = "%s_z%d" % (name, level)
            arrays[key + "__png"] = np.frombuffer(data, np.uint8)
            arrays[key + "__img"] = frame.reshape(frame.shape[0], frame.shape[1], -1)
            names.append(key)
    arrays["cases"] = np.array(names)
    path = os.path.join(HERE, "png_golden.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(names), "cases")

    cases = png_cases.cases()
    valid = [png_cases.small_valid(), png_cases.small_valid(splits=[1, 1, 3, 40], level=0), png_cases.small_valid(strategy=4),
             cases["bits_pal_d2_w5"][0], cases["pal8_trns_past"][0], cases["rgb_key_hit"][0], cases["gray_alpha"][0], cases["geom_2x3_bpp4"][0]]
    with open(os.path.join(HERE, "png_host_corpus.bin"), "wb") as f:
        f.write(b"PNGC")
        for s in valid:
            f.write(b"V" + struct.pack("<I", len(s)) + s)
        for _, s, _, _ in png_cases.malformed():
            f.write(b"M" + struct.pack("<I", len(s)) + s)
    print(f.name, os.path.getsize(f.name), "bytes")


if __name__ == "__main__":
    main()
