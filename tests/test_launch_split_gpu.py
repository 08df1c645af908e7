"""Calls of more than 65 535 frames: every batched entry point that puts the frame index in gridDim.y / gridDim.z cuts
such a call into launches of at most 65 535 frames, each rebasing its pointer tables, output pointer, strided base,
stats or tile slot.  Each entry point runs once over N = 65 538 tiny frames whose content is derived from the frame
index (a misplaced frame shows), and must equal

  * the same frames run as calls of at most 65 535 frames, concatenated, bit for bit, and
  * the C oracle at frames 0, 65 534, 65 535, 65 536 and 65 537 (the last of the first launch and the second launch).

st_cpm2_resize_maps / st_cpm2_resize_merge_maps launch one grid over n and refuse n > 65 535: that refusal must be a
clean StError that leaves the context usable.

Three of the calls of N frames (one per source file: FlowHistogram, Blur, CPM2Input) are also counted: with timing enabled
for the op's kernel class they record exactly two launches."""
import ctypes

import numpy as np
import pytest

import oracle
from scannertools_amd import _native

N = 65538
LIMIT = 65535
IDX = (0, 65534, 65535, 65536, 65537)

pytestmark = pytest.mark.gpu


def pattern(n, shape, mod, salt=0):
    """(n,) + shape int64 CUDA tensor of hashed values in [0, mod): a function of (frame index, element index, salt)."""
    import torch
    m = int(np.prod(shape))
    i = torch.arange(n, device="cuda", dtype=torch.int64).view(n, 1)
    j = torch.arange(m, device="cuda", dtype=torch.int64).view(1, m)
    h = (i * 1000003 + j * 7919 + salt * 104729) % (1 << 31)
    h = (h ^ (h >> 5)) * 2654435761 % (1 << 31)
    h = h ^ (h >> 11)
    return (h % mod).view((n,) + tuple(shape))


def frames_u8(shape, salt=0):
    import torch
    return pattern(N, shape, 256, salt).to(torch.uint8)


def flows_f32(h, w, salt=0):
    import torch
    return (pattern(N, (h, w, 2), 2000, salt).to(torch.float32) / 20.0 - 50.0).contiguous()


def split(fn, x, *more):
    """fn over calls of at most LIMIT frames, concatenated along the frame axis."""
    import torch
    return torch.cat([fn(x[lo:lo + LIMIT], *[m[lo:lo + LIMIT] for m in more]) for lo in range(0, N, LIMIT)])


def counted(ctx, kernel_id, call):
    """(call(), the launches of kernel class kernel_id it recorded)."""
    ctx.timing_enable([kernel_id])
    ctx.timing_reset()
    try:
        got = call()
        return got, ctx.timing_read(kernel_id)[0]
    finally:
        ctx.timing_enable([])


def same(a, b, what):
    assert a.shape == b.shape, what
    eq = (a == b).reshape(a.shape[0], -1).all(1)
    bad = (~eq).nonzero().flatten()
    assert bad.numel() == 0, "%s: %d frames differ from the split calls, first %s" % (what, bad.numel(), bad[:8].tolist())


# -- Histogram -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [16, 256])
def test_histogram_pointer_table_and_strided(hip_ctx, bins):
    import torch
    h, w = 3, 5
    fr = frames_u8((h, w, 3))
    whole = hip_ctx.histogram(list(fr.unbind(0)), bins)
    same(whole, split(lambda x: hip_ctx.histogram(list(x.unbind(0)), bins), fr), "histogram table bins=%d" % bins)
    # strided: 53-byte frame stride (> 45 bytes of frame, not a multiple of 16)
    stride = 53
    buf = torch.full((N * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[:N * stride].view(N, stride)[:, :3 * h * w] = fr.view(N, -1)

    def strided(base_off, n):
        out = torch.empty((n, 3, bins), dtype=torch.int32, device="cuda")
        hip_ctx._bind()
        hip_ctx._check(hip_ctx._L.st_hist_u8c3_strided(hip_ctx._h, ctypes.c_void_p(buf.data_ptr() + base_off * stride), stride, n, h, w,
                                                       bins, ctypes.c_void_p(out.data_ptr())))
        return out
    ws = strided(0, N)
    parts = torch.cat([strided(lo, min(LIMIT, N - lo)) for lo in range(0, N, LIMIT)])
    same(ws, parts, "histogram strided bins=%d" % bins)
    same(ws, whole, "histogram strided vs table bins=%d" % bins)
    fc = fr.cpu().numpy()
    got = whole.cpu().numpy()
    for i in IDX:
        np.testing.assert_array_equal(got[i], oracle.hist_u8c3(fc[i], bins), err_msg="histogram frame %d bins %d" % (i, bins))


# -- FlowHistogram and DrawFlow ------------------------------------------------------------------------------------
def test_flow_histogram_pointer_table_and_strided(hip_ctx):
    import torch
    h, w = 3, 5
    fl = flows_f32(h, w)
    whole, launches = counted(hip_ctx, _native.K_FLOW_HIST, lambda: hip_ctx.flow_histogram(list(fl.unbind(0))))
    assert launches == 2, "flow histogram of %d frames: %d launches" % (N, launches)
    same(whole, split(lambda x: hip_ctx.flow_histogram(list(x.unbind(0))), fl), "flow histogram table")
    stride = 136                                                # > 120 bytes of flow, 8-aligned, not a multiple of 16
    buf = torch.zeros((N * stride // 4,), dtype=torch.float32, device="cuda")
    buf.view(N, stride // 4)[:, :h * w * 2] = fl.view(N, -1)

    def strided(lo, n):
        out = torch.empty((n, 2, 64), dtype=torch.int32, device="cuda")
        hip_ctx._bind()
        hip_ctx._check(hip_ctx._L.st_flow_hist_strided(hip_ctx._h, ctypes.c_void_p(buf.data_ptr() + lo * stride), stride, n, h, w,
                                                       ctypes.c_void_p(out.data_ptr())))
        return out
    ws = strided(0, N)
    same(ws, torch.cat([strided(lo, min(LIMIT, N - lo)) for lo in range(0, N, LIMIT)]), "flow histogram strided")
    same(ws, whole, "flow histogram strided vs table")
    flc, got = fl.cpu().numpy(), whole.cpu().numpy()
    for i in IDX:
        np.testing.assert_array_equal(got[i], oracle.flow_hist(flc[i]), err_msg="flow histogram frame %d" % i)


@pytest.mark.parametrize("w", [4, 5])                         # 4: the four-pixel kernel (aligned rows), 5: pixel per thread
def test_draw_flow(hip_ctx, w):
    h = 3
    fr, fl = frames_u8((h, w, 3), 1), flows_f32(h, w, 2)
    whole = hip_ctx.draw_flow(fr, fl)
    same(whole, split(hip_ctx.draw_flow, fr, fl), "draw flow w=%d" % w)
    frc, flc, got = fr.cpu().numpy(), fl.cpu().numpy(), whole.cpu().numpy()
    for i in IDX:
        np.testing.assert_array_equal(got[i], oracle.draw_flow(frc[i], flc[i]), err_msg="draw flow frame %d" % i)


# -- Blur, Resize, Montage, ConvertColor -------------------------------------------------------------------------------
def test_box_blur(hip_ctx):
    fr = frames_u8((5, 7, 3), 3)
    whole, launches = counted(hip_ctx, _native.K_BLUR_OP, lambda: hip_ctx.box_blur(fr, 3))
    assert launches == 2, "blur of %d frames: %d launches" % (N, launches)
    same(whole, split(lambda x: hip_ctx.box_blur(x, 3), fr), "blur")
    frc, got = fr.cpu().numpy(), whole.cpu().numpy()
    for i in IDX:
        np.testing.assert_array_equal(got[i], oracle.box_blur(frc[i], 3), err_msg="blur frame %d" % i)


# (channels, interpolation, kernel reached): a vector kernel, the generic kernel, Lanczos4 with its coefficient tables
@pytest.mark.parametrize("cn,interp,kernel", [(3, oracle.INTER_LINEAR, "k_resize_linear_c3_v4<false>"),
                                              (2, oracle.INTER_AREA, "k_resize_u8"),
                                              (3, oracle.INTER_LANCZOS4, "k_resize_lanczos4_c3")])
def test_resize(hip_ctx, cn, interp, kernel):
    fr = frames_u8((3, 5, cn), 4 + cn)
    dw, dh = 7, 2
    whole = hip_ctx.resize(fr, dw, dh, interp)
    same(whole, split(lambda x: hip_ctx.resize(x, dw, dh, interp), fr), "resize %s" % kernel)
    frc, got = fr.cpu().numpy(), whole.cpu().numpy()
    for i in IDX:
        np.testing.assert_array_equal(got[i], oracle.resize_u8(frc[i], dw, dh, interp), err_msg="resize %s frame %d" % (kernel, i))


def test_montage_split_mid_row(hip_ctx):
    """first_slot 3 and 7 tiles per row (7 divides neither 65 535 nor 65 535 + 3): the second launch starts mid-row."""
    import torch
    fr = frames_u8((3, 5, 3), 6)
    tw, th, fpr, first = 4, 2, 7, 3
    rows = (first + N + fpr - 1) // fpr
    canvas = torch.full((rows * th, fpr * tw, 3), 77, dtype=torch.uint8, device="cuda")
    ref = canvas.clone()
    hip_ctx.montage(fr, canvas, tw, th, fpr, first_slot=first)
    for lo in range(0, N, LIMIT):
        hip_ctx.montage(fr[lo:lo + LIMIT], ref, tw, th, fpr, first_slot=first + lo)
    assert torch.equal(canvas, ref), "montage: one call differs from the split calls"
    cv, frc = canvas.cpu().numpy(), fr.cpu().numpy()
    tiles = cv.reshape(rows, th, fpr, tw, 3).transpose(0, 2, 1, 3, 4).reshape(rows * fpr, th, tw, 3)
    for i in IDX:
        s = first + i
        y, x = (s // fpr) * th, (s % fpr) * tw
        np.testing.assert_array_equal(cv[y:y + th, x:x + tw], oracle.resize_u8(frc[i], tw, th), err_msg="montage tile of frame %d" % i)
    untouched = np.r_[0:first, first + N:rows * fpr]          # slots before first_slot and after the last frame
    assert (tiles[untouched] == 77).all(), "montage wrote outside its tiles"


# (code, frame shape): 16-pixel path (every frame and row 16-byte aligned) and byte-wise path, for a YUV 4:2:0 code and a
# general one
@pytest.mark.parametrize("code,shape", [(oracle.COLOR_BGR2GRAY, (4, 4, 3)), (oracle.COLOR_BGR2GRAY, (3, 5, 3)),
                                        (90, (3, 16, 1)), (90, (3, 6, 1))], ids=["gray-px16", "gray-px1", "nv12-px16", "nv12-px1"])
def test_cvt_color(hip_ctx, code, shape):
    fr = frames_u8(shape, 8)
    whole = hip_ctx.cvt_color(fr, code)
    same(whole, split(lambda x: hip_ctx.cvt_color(x, code), fr), "cvt_color %d %s" % (code, shape))
    frc, got = fr.cpu().numpy(), whole.cpu().numpy()
    for i in IDX:
        np.testing.assert_array_equal(got[i], oracle.cvt_color(frc[i], code), err_msg="cvt_color %d frame %d" % (code, i))


# -- pose ----------------------------------------------------------------------------------------------------------
def test_cpm2_input(hip_ctx):
    fr = frames_u8((6, 5, 3), 9)                                # 6 x 5 at scale 1 -> padded to an 8 x 8 network input
    whole, launches = counted(hip_ctx, _native.K_CPM2_INPUT, lambda: hip_ctx.cpm2_input(fr, 1.0))
    assert launches == 2, "cpm2_input of %d frames: %d launches" % (N, launches)
    same(whole, split(lambda x: hip_ctx.cpm2_input(x, 1.0), fr), "cpm2_input")
    frc, got = fr.cpu().numpy(), whole.cpu().numpy()
    for i in IDX:
        np.testing.assert_array_equal(got[i], oracle.cpm2_input(frc[i], 1.0), err_msg="cpm2_input frame %d" % i)


def test_cpm2_nms_and_limb_scores(hip_ctx):
    import torch
    mp = 4
    hm = (pattern(N, (57, 8, 8), 1000, 10).to(torch.float32) / 1000.0).contiguous()
    joints = hip_ctx.cpm2_nms(hm, parts=18, max_peaks=mp, threshold=0.05)
    same(joints, split(lambda x: hip_ctx.cpm2_nms(x, parts=18, max_peaks=mp, threshold=0.05), hm), "cpm2_nms")
    scores = hip_ctx.cpm2_limb_scores(hm, joints)
    same(scores, split(hip_ctx.cpm2_limb_scores, hm, joints), "cpm2_limb_scores")
    hmc, jc, sc = hm.cpu().numpy(), joints.cpu().numpy(), scores.cpu().numpy()
    assert (sc[list(IDX)] >= 0).any(), "no limb candidate scored: the test would not see a misplaced frame"
    for i in IDX:
        np.testing.assert_array_equal(jc[i], oracle.cpm2_nms(hmc[i], 18, mp, 0.05), err_msg="cpm2_nms frame %d" % i)
        np.testing.assert_array_equal(sc[i], oracle.cpm2_limb_scores(hmc[i], jc[i]), err_msg="cpm2_limb_scores frame %d" % i)


def test_cpm2_resize_maps_refuse_more_than_65535_frames(hip_ctx):
    import torch
    from scannertools_amd.hip import StError
    maps = torch.zeros((LIMIT + 1, 2, 2, 1), dtype=torch.float32, device="cuda")
    with pytest.raises(StError):
        hip_ctx.cpm2_resize_maps(maps, 4, 4)
    with pytest.raises(StError):
        hip_ctx.cpm2_resize_merge_maps([maps], [(2.0, 2.0)], 4, 4)
    # the context is still usable: the same calls at the limit, and another op
    ok = hip_ctx.cpm2_resize_maps(maps[:LIMIT], 4, 4)
    assert ok.shape == (LIMIT, 1, 4, 4) and bool((ok == 0).all())
    f = np.arange(3 * 5 * 3, dtype=np.uint8).reshape(1, 3, 5, 3)
    np.testing.assert_array_equal(hip_ctx.resize(torch.from_numpy(f).cuda(), 7, 2).cpu().numpy()[0], oracle.resize_u8(f[0], 7, 2))
