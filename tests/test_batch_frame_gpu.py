"""The host-side frame every batched entry point begins with: a null table, a null row, an aliased row (Resize,
ConvertColor, Blur) and a misaligned map (FacenetOutput) are refused with ST_ERR_INVALID and a message that names the
row, and an empty call with null tables is ST_OK.  One line of CASES per entry point, called through the C ABI with
n = 2 tiny frames in real device buffers; the expected texts are the library's own, byte for byte.  Then one valid tiny
call per source file, through HipContext, must still give the right answer."""
import ctypes

import numpy as np
import pytest

import oracle
from scannertools_amd import _native
from scannertools_amd._native import ST_ERR_INVALID, ST_OK

pytestmark = pytest.mark.gpu

VP, F3 = ctypes.c_void_p, ctypes.c_float * 3


def _u8(*shape):
    import torch
    return [torch.zeros(shape, dtype=torch.uint8, device="cuda") for _ in range(2)]


def _f32(*shape):
    import torch
    return [torch.zeros(shape, dtype=torch.float32, device="cuda") for _ in range(2)]


def _one(dtype, *shape):
    import torch
    return torch.zeros(shape, dtype=getattr(torch, dtype), device="cuda")


class Case:
    """name: the entry point.  tables: one list of two device buffers per pointer-table argument.  call(L, ctx, n, *tables)
    makes the call with the given tables (ctypes arrays or None).  null: the refusal of a null table; row: of a null row
    (takes the index); alias: of table 0 and table 1 holding the same pointer in a row, where the entry point refuses
    that; n0: the status of n = 0 with null tables."""

    def __init__(self, name, tables, call, null, row, alias=None, n0=ST_OK):
        self.name, self.tables, self.call, self.null, self.row, self.alias, self.n0 = name, tables, call, null, row, alias, n0


def cases():
    mean = F3(0, 0, 0)
    boxes = (ctypes.c_int32 * 5)(0, 0, 0, 4, 4)
    hist_out, fh_out, fm_out, bb_out, sh_out = _one("int32", 2, 3, 16), _one("int32", 2, 2, 64), _one("int64", 2, 8), _one("int64", 1, 8), _one("float32", 1)
    canvas, scores, nhwc = _one("uint8", 4, 8, 3), _one("float32", 2, 19, 2, 2), _one("float32", 2, 4, 4, 16)
    tpl = (ctypes.c_float * 100)(*([1.0] * 100))
    counts = (ctypes.c_int32 * 2)()
    one_scale = lambda: ((ctypes.c_int * 1)(4), (ctypes.c_int * 1)(4), (ctypes.c_float * 1)(4.0), (ctypes.c_float * 1)(4.0))  # noqa: E731
    merge_src = (VP * 1)(nhwc.data_ptr())
    keep = [hist_out, fh_out, fm_out, bb_out, sh_out, canvas, scores, nhwc]   # the buffers the lambdas point into
    return keep, [
        Case("st_hist_u8c3_batch", [_u8(4, 4, 3)], lambda L, c, n, f: L.st_hist_u8c3_batch(c, f, n, 4, 4, 16, VP(hist_out.data_ptr())),
             "histogram: null frame table", "histogram: frame %d is null"),
        Case("st_flow_hist_batch", [_f32(4, 4, 2)], lambda L, c, n, f: L.st_flow_hist_batch(c, f, n, 4, 4, VP(fh_out.data_ptr())),
             "flow histogram: null argument", "flow histogram: flow %d is null"),
        Case("st_draw_flow_batch", [_u8(4, 4, 3), _f32(4, 4, 2), _u8(4, 8, 3)], lambda L, c, n, f, g, o: L.st_draw_flow_batch(c, f, g, n, 4, 4, o),
             "draw flow: null argument", "draw flow: row %d is null"),
        Case("st_box_blur_u8c3_batch", [_u8(4, 4, 3), _u8(4, 4, 3)], lambda L, c, n, f, o: L.st_box_blur_u8c3_batch(c, f, n, 4, 4, 3, o),
             "blur: null argument", "blur: row %d is null", alias="blur: row %d aliases its output"),
        Case("st_resize_u8_batch", [_u8(4, 4, 3), _u8(8, 8, 3)], lambda L, c, n, f, o: L.st_resize_u8_batch(c, f, n, 4, 4, 3, 8, 8, 1, o),
             "resize: null argument", "resize: row %d is null or aliased", alias="resize: row %d is null or aliased"),
        Case("st_resize_u8_batch (Lanczos4)", [_u8(4, 4, 3), _u8(8, 8, 3)], lambda L, c, n, f, o: L.st_resize_u8_batch(c, f, n, 4, 4, 3, 8, 8, 4, o),
             "resize: null argument", "resize: row %d is null or aliased", alias="resize: row %d is null or aliased"),
        Case("st_montage_u8c3_batch", [_u8(4, 4, 3)], lambda L, c, n, f: L.st_montage_u8c3_batch(c, f, n, 4, 4, VP(canvas.data_ptr()), 8, 4, 4, 2, 0),
             "montage: null argument", "montage: row %d is null"),
        Case("st_cvt_color_u8_batch", [_u8(4, 4, 3), _u8(4, 4, 3)], lambda L, c, n, f, o: L.st_cvt_color_u8_batch(c, f, n, 4, 4, 3, 4, 15, o),
             "cvt_color: null argument", "cvt_color: row %d is null or aliased", alias="cvt_color: row %d is null or aliased"),
        Case("st_cvt_color_u8_batch (NV12)", [_u8(6, 4, 1), _u8(4, 4, 3)], lambda L, c, n, f, o: L.st_cvt_color_u8_batch(c, f, n, 6, 4, 1, 90, 15, o),
             "cvt_color: null argument", "cvt_color: row %d is null or aliased", alias="cvt_color: row %d is null or aliased"),
        Case("st_cpm2_input_batch", [_u8(8, 8, 3), _f32(3, 8, 8)], lambda L, c, n, f, o: L.st_cpm2_input_batch(c, f, n, 8, 8, 1.0, o),
             "cpm2_input: null argument", "cpm2_input: row %d is null"),
        Case("st_cpm2_limb_scores", [_f32(57, 4, 4), _f32(18, 3, 3)],
             lambda L, c, n, h, p: L.st_cpm2_limb_scores(c, h, p, n, 4, 4, 2, 0.05, 9, VP(scores.data_ptr())),
             "cpm2_limb_scores: null argument", "cpm2_limb_scores: row %d is null"),
        Case("st_cpm2_resize_maps", [_f32(2, 8, 8)],
             lambda L, c, n, o: L.st_cpm2_resize_maps(c, VP(nhwc.data_ptr()), n, 4, 4, 16, None, 2, 8, 8, o),
             "cpm2_resize_maps: null argument", "cpm2_resize_maps: row %d is null"),
        Case("st_cpm2_resize_merge_maps", [_f32(2, 8, 8)],
             lambda L, c, n, o: L.st_cpm2_resize_merge_maps(c, merge_src, *one_scale(), 1, n, 16, None, 2, 8, 8, o),
             "cpm2_resize_merge_maps: null argument", "cpm2_resize_merge_maps: row %d is null"),
        Case("st_cpm2_nms", [_f32(18, 4, 4), _f32(18, 3, 3)], lambda L, c, n, m, j: L.st_cpm2_nms(c, m, n, 4, 4, 18, 2, 0.05, j),
             "cpm2_nms: null argument", "cpm2_nms: row %d is null"),
        Case("st_facenet_input_batch", [_u8(8, 8, 3), _f32(3, 8, 8)], lambda L, c, n, f, o: L.st_facenet_input_batch(c, f, n, 8, 8, 1.0, mean, o),
             "facenet_input: null argument", "facenet_input: row %d is null"),
        Case("st_caffe_input_batch", [_u8(8, 8, 3), _f32(3, 8, 8)], lambda L, c, n, f, o: L.st_caffe_input_batch(c, f, n, 8, 8, 8, 8, mean, 0, o),
             "caffe_input: null argument", "caffe_input: row %d is null"),
        # the one entry point without an empty call: n = 0 is among its bad arguments, as a null table is
        Case("st_nhwc_to_planar_f32", [_f32(2, 4, 4)], lambda L, c, n, o: L.st_nhwc_to_planar_f32(c, VP(nhwc.data_ptr()), n, 4, 4, 2, 16, 0, o),
             "nhwc_to_planar: bad arguments", "nhwc_to_planar: row %d is null", n0=ST_ERR_INVALID),
        Case("st_facenet_output_batch", [_f32(125, 1, 1)],
             lambda L, c, n, m: L.st_facenet_output_batch(c, m, n, 8, 8, 1.0, tpl, 0.5, 0.1, 0.0, counts),
             "facenet_output: null argument", "facenet_output: map %d is null or not 4-byte aligned"),
        Case("st_frame_moments_u8c3_batch", [_u8(4, 4, 3)], lambda L, c, n, f: L.st_frame_moments_u8c3_batch(c, f, n, 4, 4, 3, VP(fm_out.data_ptr())),
             "frame moments: null frame table", "frame moments: frame %d is null"),
        Case("st_bbox_moments_u8c3_batch", [_u8(4, 4, 3)],
             lambda L, c, n, f: L.st_bbox_moments_u8c3_batch(c, f, n, 4, 4, boxes, 1 if n else 0, VP(bb_out.data_ptr())),
             "bbox moments: null frame table", "bbox moments: frame %d is null"),
        Case("st_bbox_sharpness_u8c3_batch", [_u8(4, 4, 3)],
             lambda L, c, n, f: L.st_bbox_sharpness_u8c3_batch(c, f, n, 4, 4, boxes, 1 if n else 0, 2, VP(sh_out.data_ptr())),
             "bbox moments: null frame table", "bbox moments: frame %d is null"),
        Case("st_jpeg_encode_batch", [_u8(8, 8, 3)], lambda L, c, n, f: L.st_jpeg_encode_batch(c, f, n, 8, 8, 90, 2, 2),
             "jpeg_encode: null frame table", "jpeg_encode: frame %d is a null pointer"),
        Case("st_jpeg_encode_batch_rst", [_u8(8, 8, 3)], lambda L, c, n, f: L.st_jpeg_encode_batch_rst(c, f, n, 8, 8, 90, 2, 2, 0),
             "jpeg_encode: null frame table", "jpeg_encode: frame %d is a null pointer"),
        Case("st_jpeg_encode_batch_opt", [_u8(8, 8, 3)], lambda L, c, n, f: L.st_jpeg_encode_batch_opt(c, f, n, 8, 8, 90, 2, 2, 1, 1),
             "jpeg_encode: null frame table", "jpeg_encode: frame %d is a null pointer"),
    ]


def test_every_batched_entry_point_refuses_bad_tables_and_rows(hip_ctx):
    L = _native.lib()
    assert L is hip_ctx._L
    hip_ctx._bind()
    ctx = hip_ctx._h
    keep, table = cases()

    def refused(c, status, want, what):
        got = (L.st_ctx_last_error(ctx) or b"").decode()
        assert (status, got) == (ST_ERR_INVALID, want), "%s, %s: status %d, %r" % (c.name, what, status, got)

    for c in table:
        ptrs = [[b.data_ptr() for b in bufs] for bufs in c.tables]
        full = [(VP * 2)(*p) for p in ptrs]
        for t in range(len(full)):
            refused(c, c.call(L, ctx, 2, *[None if k == t else a for k, a in enumerate(full)]), c.null, "table %d null" % t)
            holed = [(VP * 2)(p[0], None if k == t else p[1]) for k, p in enumerate(ptrs)]
            refused(c, c.call(L, ctx, 2, *holed), c.row % 1, "row 1 of table %d null" % t)
        if c.alias:
            shared = [(VP * 2)(p[0], ptrs[0][1] if k == 1 else p[1]) for k, p in enumerate(ptrs)]
            refused(c, c.call(L, ctx, 2, *shared), c.alias % 1, "row 1 aliased")
        if c.name == "st_facenet_output_batch":
            refused(c, c.call(L, ctx, 2, (VP * 2)(ptrs[0][0], ptrs[0][1] + 2)), c.row % 1, "map 1 misaligned")
        status = c.call(L, ctx, 0, *[None] * len(full))
        assert status == c.n0, "%s, n = 0 with null tables: status %d (%s)" % (c.name, status, (L.st_ctx_last_error(ctx) or b"").decode())
        # and the call as it is meant is taken
        status = c.call(L, ctx, 2, *full)
        assert status == ST_OK, "%s, valid call: status %d (%s)" % (c.name, status, (L.st_ctx_last_error(ctx) or b"").decode())
    hip_ctx.sync()
    del keep


def test_a_valid_tiny_call_per_source_file_is_still_right(hip_ctx):
    import torch
    import ref_facenet_output_np as fo
    import ref_frame_stats_np as fs
    import ref_net_input_np as ni
    rng = np.random.default_rng(5)
    fr = rng.integers(0, 256, (2, 4, 4, 3), dtype=np.uint8)
    big = rng.integers(0, 256, (2, 8, 8, 3), dtype=np.uint8)
    fl = rng.normal(0, 4, (2, 4, 4, 2)).astype(np.float32)
    d, dbig, dfl = torch.from_numpy(fr).cuda(), torch.from_numpy(big).cuda(), torch.from_numpy(fl).cuda()
    rows = list(d.unbind(0))
    # st_hist.hip: against numpy, from a pointer table and from one tensor
    want = np.stack([[np.bincount(f[..., c].ravel() >> 4, minlength=16) for c in range(3)] for f in fr]).astype(np.int32)
    np.testing.assert_array_equal(hip_ctx.histogram(rows, 16).cpu().numpy(), want)
    np.testing.assert_array_equal(hip_ctx.histogram(d, 16).cpu().numpy(), want)
    # st_flowvis.hip
    np.testing.assert_array_equal(hip_ctx.flow_histogram(list(dfl.unbind(0))).cpu().numpy(), np.stack([oracle.flow_hist(f) for f in fl]))
    np.testing.assert_array_equal(hip_ctx.draw_flow(d, dfl).cpu().numpy(), np.stack([oracle.draw_flow(f, g) for f, g in zip(fr, fl)]))
    # st_imgproc.hip
    np.testing.assert_array_equal(hip_ctx.box_blur(rows, 3).cpu().numpy(), np.stack([oracle.box_blur(f, 3) for f in fr]))
    np.testing.assert_array_equal(hip_ctx.resize(d, 7, 5).cpu().numpy(), np.stack([oracle.resize_u8(f, 7, 5) for f in fr]))
    np.testing.assert_array_equal(hip_ctx.cvt_color(d, "COLOR_BGR2RGB").cpu().numpy(), fr[..., ::-1])
    # st_pose.hip
    np.testing.assert_array_equal(hip_ctx.cpm2_input(dbig, 1.0).cpu().numpy(), np.stack([oracle.cpm2_input(f, 1.0) for f in big]))
    # st_netinput.hip
    np.testing.assert_array_equal(hip_ctx.caffe_input(dbig, 4, 4, (1.0, 2.0, 3.0)).cpu().numpy(), ni.caffe_input(big, 4, 4, (1.0, 2.0, 3.0)))
    # st_nn.hip
    x = torch.from_numpy(rng.normal(0, 1, (2, 3, 4, 4)).astype(np.float32))
    xd = torch.zeros((2, 4, 4, 16), dtype=torch.float32, device="cuda")
    xd[..., :3] = x.permute(0, 2, 3, 1).cuda()
    assert torch.equal(hip_ctx.nhwc_to_planar(xd, 3).cpu(), x)
    # st_detect.hip
    h, w, scale, thr = 67, 93, 0.73, 0.5
    maps = np.stack([fo.make_map(100 + i, 9, 6, -1.3) for i in range(2)])
    T = fo.templates()
    for got, m in zip(hip_ctx.facenet_output(torch.from_numpy(maps).cuda(), h, w, scale, T, thr), maps):
        assert fo.threshold_margin(m, h, w, scale, T, thr) > 1e-6
        np.testing.assert_array_equal(np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(fo.facenet_output(m, h, w, scale, T, thr), np.float32).view(np.uint32))
    # st_framestats.hip
    np.testing.assert_array_equal(hip_ctx.frame_moments(rows).cpu().numpy(), np.stack([fs.moments(f) for f in fr]))
    got = hip_ctx.bbox_moments(dbig, [[1, 1, 2, 7, 8]]).cpu().numpy()
    assert got.shape == (1, 8) and (got[0, :2] == 0).all() and (got[0, 5:] > 0).all()
    # st_jpeg_enc.hip and st_jpeg.hip: what was encoded decodes to a picture close to the original
    back = hip_ctx.decode_jpeg(hip_ctx.encode_jpeg(dbig, quality=100, subsampling="4:4:4")).cpu().numpy()
    assert back.shape == big.shape and np.abs(back.astype(int) - big.astype(int)).max() <= 8
