"""The RGB-source instance of the role-split pyramid (k_pyr_roles<false, true>): calls above 16 pairs on a one-pass-pyramid
geometry with 4-byte aligned frames read the RGB frames in the pyramid pass itself and leave the gray frames behind for the
level-0 expansion (k_polyexp_u8) -- no luma pass.  ST_PYR_ROLES_RGB=0 restores the separate pass (k_gray4), which is also what
a call with unaligned frames falls back to.  Both must give the same bits.

Shapes (17 pairs = 18 frames, the smallest call above the 16-pair limit):
  256 x 256    one strip, the smallest one-pass-pyramid geometry (level 3 is 32 x 32)
  264 x 1032   two strips of 520 columns (the second is cut short by the frame: 512 columns), 16-row segments over 264 rows
               (the last segment has 8)
Which path a call took is read from the luma pass's launch counter (st_ctx_timing_read of the gray kernel class).
"""
import os

import numpy as np
import pytest

import oracle
from util import assert_flow_close, random_frames, texture_stream

pytestmark = pytest.mark.gpu

N_FRAMES = 18
SHAPES = [(256, 256), (264, 1032)]
KEYS = ("ST_ITER_TILE", "ST_PYR_FOLD_GRAY", "ST_ITER_ROLES", "ST_ROLES_NCW", "ST_ROLES_ROWS", "ST_PYR_ROLES", "ST_POLY_U8",
        "ST_CONCURRENT", "ST_PYR_ROLES_RGB")


def _ctx_under(env):
    """A HipContext created under `env` alone (the switches are read when a context is created)."""
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
    c = {"rgb": _ctx_under({}), "gray": _ctx_under({"ST_PYR_ROLES_RGB": "0"})}
    for x in c.values():
        x.timing_enable([_native.K_GRAY])
    yield c
    for x in c.values():
        x.close()


def _frames(kind, h, w):
    if kind == "random":
        return random_frames(7 + h, N_FRAMES, h, w)
    return texture_stream(11 + w, N_FRAMES, h, w)[0]


def _flow(ctx, dev_frames):
    """(flows, launches of the luma pass) of one call."""
    from scannertools_amd import _native
    ctx.timing_reset()
    out = ctx.optical_flow(dev_frames)
    ctx.sync()
    return out.cpu().numpy(), ctx.timing_read(_native.K_GRAY)[0]


def test_geometries_take_the_one_pass_pyramid():
    for h, w in SHAPES:
        assert oracle.fb_levels(h, w) == 3 and h % 8 == 0 and w % 8 == 0
        assert [oracle.fb_level_geom(h, w, k)[:2] for k in range(4)] == [(h >> k, w >> k) for k in range(4)]


@pytest.mark.parametrize("kind", ["random", "texture"])
@pytest.mark.parametrize("h,w", SHAPES)
def test_rgb_source_pyramid_is_bit_identical_to_the_separate_luma_pass(ctxs, h, w, kind):
    import torch
    frames = _frames(kind, h, w)
    dev = torch.from_numpy(frames).cuda()
    assert all(dev[i].data_ptr() % 4 == 0 for i in range(N_FRAMES))
    got, gray_launches = _flow(ctxs["rgb"], dev)
    want, gray_launches_off = _flow(ctxs["gray"], dev)
    assert gray_launches == 0, "the default context still ran the luma pass"
    assert gray_launches_off == 1, "ST_PYR_ROLES_RGB=0 did not restore the luma pass"
    assert got.shape == (N_FRAMES - 1, h, w, 2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (
        "flows differ", int((got.view(np.uint32) != want.view(np.uint32)).sum()), float(np.abs(got - want).max()))
    ref = oracle.optical_flow_rgb(frames[0], frames[1])
    assert_flow_close(got[0], ref, frames[0], frames[1], "%dx%d %s" % (h, w, kind))


def test_unaligned_frames_fall_back_to_the_luma_pass(ctxs):
    """The same frames from a view shifted by one byte: no frame starts on a 4-byte boundary, the call runs the byte luma
    kernel and the gray-source pyramid, and the flows are the aligned call's bit for bit."""
    import torch
    h, w = 256, 256
    frames = _frames("texture", h, w)
    dev = torch.from_numpy(frames).cuda()
    flat = torch.empty(frames.size + 1, dtype=torch.uint8, device="cuda")
    shifted = flat[1:].view(N_FRAMES, h, w, 3)
    shifted.copy_(dev)
    assert all(shifted[i].data_ptr() % 4 != 0 for i in range(N_FRAMES))
    want, n_aligned = _flow(ctxs["rgb"], dev)
    got, n_shifted = _flow(ctxs["rgb"], shifted)
    assert n_aligned == 0 and n_shifted == 1
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
