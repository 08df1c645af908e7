"""Writes tests/golden/jpeg_reduced_golden.npz: baseline JPEG streams made by Pillow (libjpeg-turbo) and the frames Pillow hands
out for them at scale 1/2, 1/4 and 1/8 (im.draft(), libjpeg's scaled decoding: what cv::imdecode's IMREAD_REDUCED_* flags
return too) -- what ImageDecoder's `scale` is held to.  Needs Pillow; run from the repository root:

    python tests/golden/make_jpeg_reduced_golden.py

Keys: "<case>__jpg" the stream (uint8), "<case>__cfg" its settings (JSON), and per denominator d either "<case>__d<d>" the
(ceil(h/d), ceil(w/d), c) uint8 frame or, where the frame has more than FRAME_BYTES bytes, "<case>__d<d>_sha" the SHA-256 of
its bytes and "<case>__d<d>_shape".  "cases" lists "<case>/<d>" for every frame Pillow produced; "restatement_only" lists the
"<case>/<d>" whose frame Pillow cannot be asked for (a side shorter than the denominator, or than 4 where draft() then picks
a smaller denominator): those frames are tests/ref_jpeg_reduced_np.py's.  Every Pillow frame is checked here against that
restatement, byte for byte.
"""
import hashlib
import io
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ref_jpeg_reduced_np as RR  # noqa: E402
from make_jpeg_golden import content, encode  # noqa: E402

FRAME_BYTES = 2048
SIZES = [(8, 8), (16, 16), (17, 33), (37, 53), (40, 3), (3, 40), (64, 128), (128, 256), (100, 131)]   # (w, h)
SUBPIXEL = [(1, 1), (7, 9)]                                                                              # restatement only
SAMPLINGS = [("444", "4:4:4"), ("422", "4:2:2"), ("420", "4:2:0"), ("gray", None)]


def calm(w, h, seed):
    """The larger frames: sinusoids under little noise, so that their streams stay small at quality 95."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ph = rng.uniform(0, 6.28, 6)
    img = np.stack([127 + 110 * np.sin(x / 9.1 + ph[0]) * np.cos(y / 11.3 + ph[1]),
                    127 + 110 * np.sin((x + y) / 13.7 + ph[2]) * np.cos(y / 7.9 + ph[3]),
                    127 + 110 * np.cos(x / 17.3 + ph[4]) * np.sin((x - y) / 8.7 + ph[5])], axis=-1)
    return np.clip(img + rng.normal(0, 1.5, img.shape), 0, 255).astype(np.uint8)


def draft(jpg, d):
    """Pillow's frame at 1/d, or None where draft() cannot be asked for that denominator."""
    im = Image.open(io.BytesIO(jpg))
    w, h = im.size
    im.draft(im.mode, (max(1, w // d), max(1, h // d)))
    if im.decoderconfig[:1] != (d,):          # draft() settled on a smaller denominator (a side below 2 d, or below d)
        return None
    assert im.size == (-(-w // d), -(-h // d))
    a = np.asarray(im)
    return np.ascontiguousarray(a if a.ndim == 3 else a[..., None])


def main():
    out, cases, ref_only = {}, [], []
    seed = 3000
    for si, (w, h) in enumerate(SIZES + SUBPIXEL):
        for ci, (sname, sub) in enumerate(SAMPLINGS):
            for qi, q in enumerate((30, 95)):
                seed += 1
                rst = (si + ci + qi) % 2 == 0          # a restart interval per MCU row on every other stream
                if (w, h) in SUBPIXEL and (sname in ("422", "gray") or qi == 1):
                    continue
                if (w, h) in ((40, 3), (3, 40)) and qi == 0:
                    continue
                pic = calm(w, h, seed) if w * h > 4096 else content("noise" if qi else "smooth", w, h, seed)
                kw = dict(quality=q)
                if sub is None:
                    pic = pic[..., 1]
                else:
                    kw["subsampling"] = sub
                if rst:
                    kw["restart_marker_rows"] = 1
                name = "%dx%d_%s_q%d%s" % (w, h, sname, q, "_rst" if rst else "")
                jpg = encode(pic, **kw)
                assert (b"\xff\xdd" in jpg[:jpg.index(b"\xff\xda")]) == rst, name
                out[name + "__jpg"] = np.frombuffer(jpg, np.uint8)
                out[name + "__cfg"] = np.array(json.dumps(dict(kw, w=w, h=h)))
                for d in (2, 4, 8):
                    ref = RR.decode(jpg, d)
                    img = draft(jpg, d)
                    if img is None:
                        assert min(w, h) < max(d, 4), (name, d)
                        img = ref
                        ref_only.append("%s/%d" % (name, d))
                    else:
                        assert min(w, h) >= d and np.array_equal(img, ref), (name, d)
                        cases.append("%s/%d" % (name, d))
                    if img.size > FRAME_BYTES:
                        out["%s__d%d_sha" % (name, d)] = np.array(hashlib.sha256(img.tobytes()).hexdigest())
                        out["%s__d%d_shape" % (name, d)] = np.array(img.shape)
                    else:
                        out["%s__d%d" % (name, d)] = img
    out["cases"], out["restatement_only"] = np.array(cases), np.array(ref_only)
    path = os.path.join(HERE, "jpeg_reduced_golden.npz")
    np.savez_compressed(path, **out)
    print("%s: %d Pillow frames, %d restatement-only, %d bytes" % (path, len(cases), len(ref_only), os.path.getsize(path)))


if __name__ == "__main__":
    main()
