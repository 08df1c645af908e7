"""Shared synthetic-input helpers for the test-suite (deterministic, seeded)."""
import os

import numpy as np


class env_threads:
    """The environment variable `name` (ST_JPEG_THREADS, ST_PNG_THREADS) set to n for the calls inside the block: the library
    reads it at each call."""

    def __init__(self, name, n):
        self.name, self.n = name, n

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ[self.name] = str(self.n)

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.old


def random_frames(seed, n, h, w):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def smooth_texture(seed, h, w, sigma=3.0):
    """Gaussian-filtered noise scaled to 0..255 (float64)."""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    t = gaussian_filter(rng.standard_normal((h, w)), sigma)
    t = (t - t.min()) / (t.max() - t.min()) * 255.0
    return t


def translated_rgb_pair(seed, h, w, tx, ty, margin=24):
    """Two RGB frames cut from one texture so that next(x+tx, y+ty) == prev(x, y)."""
    tex = [smooth_texture(seed * 3 + c, h + 2 * margin, w + 2 * margin) for c in range(3)]
    f0 = np.stack([t[margin:margin + h, margin:margin + w] for t in tex], axis=-1)
    f1 = np.stack([t[margin - ty:margin - ty + h, margin - tx:margin - tx + w] for t in tex], axis=-1)
    return f0.astype(np.uint8), f1.astype(np.uint8)


def texture_stream(seed, n, h, w, margin=24, max_step=3):
    """n RGB frames: a texture under an integer random-walk translation (non-trivial flow)."""
    rng = np.random.default_rng(seed)
    tex = [smooth_texture(seed * 3 + c, h + 2 * margin, w + 2 * margin) for c in range(3)]
    pos = np.zeros(2, int)
    frames, steps = [], []
    for i in range(n):
        ox, oy = margin - pos[0], margin - pos[1]
        frames.append(np.stack([t[oy:oy + h, ox:ox + w] for t in tex], axis=-1).astype(np.uint8))
        step = rng.integers(-max_step, max_step + 1, 2)
        newpos = np.clip(pos + step, -margin, margin)
        steps.append(newpos - pos)
        pos = newpos
    return np.stack(frames), np.array(steps[:-1])


def torch_stream(n, h, w, seed, step=2):
    """n frames of a smooth texture under a steady translation, generated on the GPU (big sizes):
    frame i is the texture window shifted by (-step * i) columns and (+i) rows, so next(x + step, y - 1) = prev(x, y)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    m = step * n + 8
    low = torch.rand((1, 3, (h + 2 * m) // 8 + 2, (w + 2 * m) // 8 + 2), device="cuda", generator=g)
    tex = torch.nn.functional.interpolate(low, size=(h + 2 * m, w + 2 * m), mode="bicubic", align_corners=False)[0]
    tex = ((tex - tex.amin()) / (tex.amax() - tex.amin()) * 235 + 10).permute(1, 2, 0)
    fr = [tex[m + i:m + i + h, m - step * i:m - step * i + w] + torch.randint(-2, 3, (h, w, 3), device="cuda", generator=g)
          for i in range(n)]
    return torch.stack([f.clamp(0, 255).to(torch.uint8) for f in fr]).contiguous()


# ------------------------------------------------------------------------------------------------
# Motion that is NOT a whole-pixel shift (round-5 verdict, item 2).  The reference op runs on decoded video
# (scannertools/tests/test_all.py:162-177, scannertools_infra/tests.py:17-86): sub-pixel, zooming, rotating, occluding
# motion.  Every kind is one texture resampled through a backward map (scipy map_coordinates, cubic), so the second frame
# is what a camera would see, not a crop.
# ------------------------------------------------------------------------------------------------
MOTION_KINDS = ("subpixel", "zoom", "rotate", "occlusion", "jump", "static", "noise")


def _warp(tex, yy, xx):
    """tex (H,W,3) float sampled at (yy, xx) (float coordinate grids), cubic, reflected borders."""
    from scipy.ndimage import map_coordinates
    return np.stack([map_coordinates(tex[..., c], [yy, xx], order=3, mode="reflect") for c in range(3)], -1)


def motion_pair(kind, seed, h, w):
    """Two uint8 RGB frames (h,w,3) related by `kind` of motion; +-1 grey level of independent sensor noise on each.
      subpixel   translation by (2.37, -1.61) px           zoom       1.5 % about the centre
      rotate     0.8 degrees about the centre              occlusion  a textured rectangle moving (+5.3, +2.2) over a
      jump       translation by (-24, 17) px                          background moving (-1.4, 0.6)
      static     the same view twice (noise only)          noise      two independent random frames
    """
    assert kind in MOTION_KINDS, kind
    rng = np.random.default_rng(1000 * MOTION_KINDS.index(kind) + seed)
    if kind == "noise":
        return (rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
    m = 32
    sig = 3.0 if min(h, w) >= 200 else 2.0
    tex = np.stack([smooth_texture(7 * seed + 31 * MOTION_KINDS.index(kind) + c, h + 2 * m, w + 2 * m, sig) for c in range(3)], -1)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cy, cx = (h - 1) / 2.0, (w - 1) / 2.0
    a = tex[m:m + h, m:m + w].copy()
    if kind == "subpixel":
        b = _warp(tex, yy + m + 1.61, xx + m - 2.37)
    elif kind == "zoom":
        b = _warp(tex, cy + (yy - cy) / 1.015 + m, cx + (xx - cx) / 1.015 + m)
    elif kind == "rotate":
        t = np.deg2rad(0.8)
        b = _warp(tex, cy + (yy - cy) * np.cos(t) - (xx - cx) * np.sin(t) + m, cx + (yy - cy) * np.sin(t) + (xx - cx) * np.cos(t) + m)
    elif kind == "jump":
        b = tex[m - 17:m - 17 + h, m + 24:m + 24 + w].copy()
    elif kind == "static":
        b = a.copy()
    else:  # occlusion
        fg = np.stack([smooth_texture(900 + 7 * seed + c, h + 2 * m, w + 2 * m, sig * 0.7) for c in range(3)], -1)
        b = _warp(tex, yy + m - 0.6, xx + m + 1.4)
        y0, y1, x0, x1 = h // 4, h // 4 + max(h // 3, 4), w // 3, w // 3 + max(w // 4, 4)
        a[y0:y1, x0:x1] = fg[m + y0:m + y1, m + x0:m + x1]
        # the rectangle keeps its own texture and moves by (+5.3, +2.2): backward map of the foreground layer
        fgw = _warp(fg, yy + m - 2.2, xx + m - 5.3)
        inside = (yy - 2.2 >= y0) & (yy - 2.2 < y1) & (xx - 5.3 >= x0) & (xx - 5.3 < x1)
        b = np.where(inside[..., None], fgw, b)
    na, nb = rng.integers(-1, 2, a.shape), rng.integers(-1, 2, a.shape)
    return (np.clip(np.rint(a) + na, 0, 255).astype(np.uint8), np.clip(np.rint(b) + nb, 0, 255).astype(np.uint8))


def planar5(a):
    """(h,w,5) -> (5,h,w) contiguous."""
    return np.ascontiguousarray(np.moveaxis(a, -1, 0))


def interleaved5(a):
    """(5,h,w) -> (h,w,5)."""
    return np.ascontiguousarray(np.moveaxis(a, 0, -1))


def synthetic_pose_maps(seed, H, W, n_people, max_peaks=64, clutter=3, drop=0.1):
    """Network outputs of the CPM2 pose model for planted people (COCO_18): heat maps (57,H,W) whose
    part-affinity planes carry the unit vector of every planted limb along its segment (+ noise), and
    the joint candidates (18,max_peaks+1,3) an NMS layer would report: the planted joints (some
    dropped), jittered, plus `clutter` false candidates per part.  Returns (heatmap, peaks, truth) with
    truth (n_people,18,2) joint positions (NaN where dropped)."""
    import oracle
    rng = np.random.default_rng(seed)
    hm = (rng.standard_normal((57, H, W)) * 0.01).astype(np.float32)
    # people stand side by side, each in its own column of the map, so that no limb crosses another person's
    centres = np.array([[(p + 0.5) * W / max(n_people, 1), 0.52 * H] for p in range(n_people)]).reshape(n_people, 2)
    # a loose stick figure around each centre (offsets in units of body size)
    layout = np.array([[0, -1.0], [0, -0.7], [-0.3, -0.7], [-0.45, -0.35], [-0.5, 0.0], [0.3, -0.7], [0.45, -0.35], [0.5, 0.0],
                       [-0.2, 0.0], [-0.22, 0.5], [-0.24, 1.0], [0.2, 0.0], [0.22, 0.5], [0.24, 1.0], [-0.08, -1.08],
                       [0.08, -1.08], [-0.17, -1.0], [0.17, -1.0]])
    truth = np.full((n_people, 18, 2), np.nan)
    peaks = np.zeros((18, max_peaks + 1, 3), np.float32)
    for p in range(n_people):
        size = min(0.4 * H, 0.8 * W / n_people) * rng.uniform(0.8, 1.0)
        pts = centres[p] + layout * size + rng.normal(0, 0.01 * size, (18, 2))
        pts[:, 0] = np.clip(pts[:, 0], 2, W - 3)
        pts[:, 1] = np.clip(pts[:, 1], 2, H - 3)
        keep = rng.random(18) > drop
        keep[1] = True
        for k in range(19):
            a, b = oracle.CPM2_LIMB_SEQ[2 * k], oracle.CPM2_LIMB_SEQ[2 * k + 1]
            d = pts[b] - pts[a]
            n = np.hypot(*d)
            if n < 1e-3:
                continue
            u = d / n
            for t in np.linspace(0, 1, int(2 * n) + 2):
                cx, cy = pts[a] + t * d
                x0, y0 = int(round(cx)), int(round(cy))
                for yy in range(max(0, y0 - 2), min(H, y0 + 3)):
                    for xx in range(max(0, x0 - 2), min(W, x0 + 3)):
                        hm[oracle.CPM2_MAP_IDX[2 * k], yy, xx] = u[0]
                        hm[oracle.CPM2_MAP_IDX[2 * k + 1], yy, xx] = u[1]
        for j in range(18):
            if keep[j]:
                truth[p, j] = pts[j]
                c = int(peaks[j, 0, 0]) + 1
                peaks[j, c] = (np.round(pts[j, 0]), np.round(pts[j, 1]), rng.uniform(0.5, 0.95))
                peaks[j, 0, 0] = c
    for j in range(18):
        for _ in range(clutter):
            c = int(peaks[j, 0, 0]) + 1
            if c > max_peaks:
                break
            peaks[j, c] = (rng.integers(0, W), rng.integers(0, H), rng.uniform(0.1, 0.4))
            peaks[j, 0, 0] = c
    hm += (rng.standard_normal(hm.shape) * 0.02).astype(np.float32)
    return hm, peaks, truth


def cvt_source(rng, code, h, w):
    """A random uint8 frame of the shape cv::cvtColor code `code` takes, near (h, w): 1-, 2-, 3- or 4-channel pixels, the
    (3H/2, W, 1) YUV 4:2:0 frames of codes 90..106 and the (H, W, 2) packed 4:2:2 frames of codes 107..124 (even sizes)."""
    import oracle
    if 90 <= code <= 106:
        H, W = max(2, h - h % 2), max(2, w - w % 2)
        return rng.integers(0, 256, (H * 3 // 2, W, 1), dtype=np.uint8)
    if 107 <= code <= 124:
        return rng.integers(0, 256, (max(1, h), max(2, w - w % 2), 2), dtype=np.uint8)
    cin = next(c for c in (1, 2, 3, 4) if oracle.lib().orc_cvt_out_channels(code, c) > 0)
    return rng.integers(0, 256, (h, w, cin), dtype=np.uint8)


def float64_flow(frame_a, frame_b, params=None):
    """The independent float64 derivation's flow between two RGB frames; params: a dict of st_fb_params fields that differ
    from the defaults (None: the reference's parameters)."""
    import oracle
    import ref_farneback_np as exact
    p = dict(params or {})
    bits = p.get("gray_bits", 15)
    return exact.farneback(oracle.gray_u8(frame_a, bits), oracle.gray_u8(frame_b, bits), num_levels=p.get("num_levels", 3),
                           pyr_scale=p.get("pyr_scale", 0.5), win=p.get("win_size", 15), iters=p.get("num_iters", 3),
                           poly_n=p.get("poly_n", 5), poly_sigma=p.get("poly_sigma", 1.2))


def within_half_again(got, ref, f64, size=45):
    """The second tier-2 rule of assert_flow_close: the kernel is as close to exact arithmetic as the oracle is, within half
    again -- every pixel against the oracle's worst distance within its size x size neighbourhood, and in L2 over the field."""
    from scipy import ndimage as _ndi
    noise = np.abs(ref - f64).max(-1)
    eg = np.abs(got - f64).max(-1)
    local = _ndi.maximum_filter(noise, size=size, mode="nearest")
    return bool((eg <= 1.5 * local + 5e-3).all() and
                np.linalg.norm(got - f64) <= 1.5 * np.linalg.norm(ref - f64) + 1e-4 * np.linalg.norm(f64) + 1e-6)


def assert_flow_close(got, ref, frame_a, frame_b, what="", params=None):
    """Flow of the HIP path against the oracle: max-abs <= 5e-3 px and relative L2 <= 1e-4 -- tier 1, what all but a few
    in ten thousand fuzz pairs (and every benchmark-sized, textured pair) meet.

    The algorithm itself is discontinuous in two places, and there two correct float implementations can differ by
    1e-2 px on a handful of pixels: (i) on low-texture stretches the 2x2 solve divides by a determinant of ~1e-3..1e-2,
    i.e. it amplifies the float32 matrices' rounding residue a hundredfold -- the oracle then sits as far from exact
    arithmetic as the kernel; (ii) UpdateMatrices switches formula where the warped position leaves [0, w-1) x [0, h-1)
    (the reference's last-row / last-column quirk included): a flow component that is rounding noise around zero
    decides the branch, and the box filter spreads the jump over its 15 x 15 window.  Campaigns of 300 and 1 500 flow
    seeds (round 3) met six such pairs, 7-126 pixels each, all on flat borders of 86..192-pixel frames.
    When tier 1 fails, the independent float64 derivation (tests/ref_farneback_np.py) arbitrates:
      tier 2 (noise): every pixel within max(5e-3, 2 x the oracle's own distance from exact arithmetic + 1e-3), at most
              0.5 % of the field needing that, and relative L2 <= 1e-4 (or RMS <= 5e-4 px where the whole flow is noise,
              as for identical frames) over the pixels where the oracle is within 1e-3 px of exact arithmetic -- or
              the kernel within half again of the oracle's own distance from exact arithmetic: every pixel against the
              oracle's worst distance within its 45 x 45 neighbourhood, and in L2 over the field;
      tier 3 (branch flip): the pixels beyond 5e-3 are at most 0.75 % of the field (or two 15 x 15 box windows, whichever is
              more: one flipped pixel moves its whole window), each lies within 24 px of the frame
              border or where the float64 normal equations have det + 1e-3 <= 0.05 (textured 8-bit images: 1e2..1e4),
              none is beyond 0.1 px, relative L2 <= 1e-4 over the other pixels and <= 1e-3 (the north-star bound)
              over the whole field (fields below 20 000 pixels: 1e-3 x sqrt(20 000 / n), the footprint of a flip being fixed).
    params: a dict of the st_fb_params fields that differ from the defaults, when `ref` was computed with other parameters
    than the reference's: the float64 arbitration then runs with the same parameters, and the neighbourhood of the
    half-again rule is 3 x win_size instead of the fixed 45 (three box filters of win_size carry one pixel's rounding
    residue that far).
    Returns the tier that passed (1, 2 or 3)."""
    d = np.abs(got - ref).max(-1)
    nref = max(float(np.linalg.norm(ref)), 1e-30)
    if d.max() <= 5e-3 and np.linalg.norm(got - ref) <= 1e-4 * nref + 1e-6:
        return 1
    import oracle
    import ref_farneback_np as exact
    prm = dict(params or {})
    win = prm.get("win_size", 15)
    g0, g1 = oracle.gray_u8(frame_a, prm.get("gray_bits", 15)), oracle.gray_u8(frame_b, prm.get("gray_bits", 15))
    f64 = float64_flow(frame_a, frame_b, prm)
    noise = np.abs(ref - f64).max(-1)
    out = d > 5e-3

    def rel_or_rms(keep):
        dk = (got - ref)[keep]
        if dk.size == 0:
            return True
        rel_ok = np.linalg.norm(dk) <= 1e-4 * max(float(np.linalg.norm(ref[keep])), 1e-30) + 1e-6
        return rel_ok or float(np.sqrt((dk.astype(np.float64) ** 2).mean())) <= 5e-4

    if (d <= np.maximum(5e-3, 2.0 * noise + 1e-3)).all() and out.mean() <= 5e-3 and rel_or_rms(noise <= 1e-3):
        return 2
    # ... or: the kernel is as close to exact arithmetic as the oracle is (within half again) -- pixel by pixel against the
    # oracle's own distance in the pixel's neighbourhood (45 x 45: three iterations of the 15 x 15 box filter carry one pixel's
    # rounding residue that far), not against the worst pixel of the field, so that one noisy pixel in a corner cannot excuse
    # an error somewhere else
    if within_half_again(got, ref, f64, 3 * win):
        return 2
    # tier 3: where are the outliers?
    # one flipped pixel moves its whole 15 x 15 box window: on frames of a few thousand pixels two windows are more than 0.75 %
    assert out.sum() <= max(7.5e-3 * out.size, 2 * 15 * 15), (what, "pixels beyond 5e-3 px", int(out.sum()), out.size)
    assert d.max() <= 0.1, (what, "max-abs", float(d.max()))
    from scipy import ndimage
    h, w = d.shape
    yy, xx = np.mgrid[0:h, 0:w]
    near_border = (yy < 24) | (yy >= h - 24) | (xx < 24) | (xx >= w - 24)
    pn, ps = prm.get("poly_n", 5), prm.get("poly_sigma", 1.2)
    R0, R1 = exact.poly_expansion(exact.pyramid_image(g0, 0), pn, ps), exact.poly_expansion(exact.pyramid_image(g1, 0), pn, ps)
    B = np.stack([ndimage.uniform_filter(exact.update_matrices(R0, R1, f64)[..., c], size=win, mode="nearest") for c in range(3)], -1)
    flat = B[..., 0] * B[..., 2] - B[..., 1] * B[..., 1] + 1e-3 <= 0.05
    bad = out & ~(near_border | flat)
    assert not bad.any(), (what, "pixels beyond 5e-3 px in the textured interior", int(bad.sum()), float(d[bad].max()))
    assert rel_or_rms(~out), (what, "relative L2 outside the outliers")
    # whole field: the north-star bound 1e-3 -- for fields of >= 20 000 pixels; a flip's footprint is a fixed number of pixels,
    # so on a smaller field of n pixels the same event weighs sqrt(20 000 / n) more
    lim = 1e-3 * max(1.0, float(np.sqrt(20000.0 / out.size)))
    assert np.linalg.norm(got - ref) <= lim * nref + 1e-6 or float(np.sqrt(((got - ref).astype(np.float64) ** 2).mean())) <= 5e-3, (what, "whole-field relative L2")
    return 3
