"""The marching flow iteration (k_flow_iter3) with unequal segments against the tile kernel, which has no segments: both form
the window sums in the same association (anchors every 32 rows / 8 columns), so their flows agree bit for bit whatever the
segment heights.  Heights that are no whole number of 32-row periods: 135 x 240 (the headline's level 3) and 200 x 328, at 1, 3
and 17 pairs -- there the last segment is a short remainder (7 / 8 rows) -- and 135 x 240 at 256 pairs, the one call of this
file whose level 0 fills more than one round of resident workgroups, so that the planner takes the rounded-down height and
the last segment is the TALLER one (64 + 71 rows; tests/test_iter_segments.py restates the planner).
"""
import os

import numpy as np
import pytest

import oracle
from util import assert_flow_close, texture_stream

pytestmark = pytest.mark.gpu

KEYS = ("ST_ITER_TILE", "ST_PYR_FOLD_GRAY", "ST_ITER_ROLES", "ST_ROLES_NCW", "ST_ROLES_ROWS", "ST_PYR_ROLES", "ST_POLY_U8",
        "ST_CONCURRENT", "ST_PYR_ROLES_RGB")
CASES = [(135, 240, 1), (135, 240, 3), (135, 240, 17), (200, 328, 1), (200, 328, 3), (200, 328, 17), (135, 240, 256)]


def _ctx_under(env):
    from scannertools_amd.hip import HipContext
    saved = {k: os.environ.get(k) for k in KEYS}
    try:
        for k in KEYS:
            os.environ.pop(k, None)
        os.environ.update(env)
        return HipContext(0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctxs():
    import torch
    from scannertools_amd import _native
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    c = {"march": _ctx_under({"ST_ITER_TILE": "0", "ST_ITER_ROLES": "0", "ST_PYR_ROLES": "0"}), "tile": _ctx_under({"ST_ITER_TILE": "1"})}
    for x in c.values():
        x.timing_enable([_native.K_BLUR_UPDATE])
    yield c
    for x in c.values():
        x.close()


_streams = {}


def _stream(h, w):
    """257 frames per geometry, made once; a call of n pairs takes the first n + 1."""
    if (h, w) not in _streams:
        _streams[(h, w)] = texture_stream(5 + h, 257 if (h, w) == (135, 240) else 18, h, w)[0]
    return _streams[(h, w)]


@pytest.mark.parametrize("h,w,n_pairs", CASES)
def test_marching_and_tile_kernels_agree_with_unequal_segments(ctxs, h, w, n_pairs):
    import torch
    from scannertools_amd import _native
    frames = _stream(h, w)[:n_pairs + 1]
    dev = torch.from_numpy(frames).cuda()
    got = {}
    for name, ctx in ctxs.items():
        ctx.timing_reset()
        out = ctx.optical_flow(dev)
        ctx.sync()
        got[name] = out.cpu().numpy()
        # every iteration launch carries its own timing events: 3 iterations per level, each with a duration
        launches, ms = ctx.timing_read(_native.K_BLUR_UPDATE)
        assert launches == 3 * (oracle.fb_levels(h, w) + 1) and ms > 0.0, (name, launches, ms)
    a, b = got["march"], got["tile"]
    assert a.shape == (n_pairs, h, w, 2)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (
        "flows differ", int((a.view(np.uint32) != b.view(np.uint32)).sum()), float(np.abs(a - b).max()))
    for i in sorted({0, n_pairs - 1} if n_pairs <= 17 else {0}):
        ref = oracle.optical_flow_rgb(frames[i], frames[i + 1])
        assert_flow_close(a[i], ref, frames[i], frames[i + 1], "%dx%d pair %d of %d" % (h, w, i, n_pairs))
