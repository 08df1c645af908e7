"""FacenetInput and CaffeInput on the GPU.  Every comparison is bit for bit: FacenetInput against
oracle.resize_u8 followed by the numpy lines of the contract, CaffeInput against the float32 restatement
(tests/ref_net_input_np.py)."""
import numpy as np
import pytest
import torch

import oracle
import ref_net_input_np as ref
from scannertools_amd import _native
from scannertools_amd.engine import CacheMode, Client, DeviceType, NamedStream, NamedVideoStream, PerfParams
from scannertools_amd.hip import facenet_geometry
from util import random_frames

pytestmark = pytest.mark.gpu

MEANS = {"caffe": (104.00699, 116.66877, 122.67892), "negative": (-3.25, -117.1, -0.001), "zero": (0.0, 0.0, 0.0)}
# (h, w, scale): the contract's cases, then three whose frames and rows are 16-byte aligned in every path of the kernel
FACENET_CASES = [(37, 53, 1.0),     # resized and padded to 40 x 56
                 (48, 64, 0.5),     # the exact 2 x 2 reroute (aligned rows)
                 (8, 8, 1.0),       # equal size is a copy
                 (45, 61, 0.73),
                 (130, 70, 1.37),   # enlarging; three row tiles, two column tiles
                 (1, 1, 1.0),       # one pixel to 8 x 8
                 (200, 9, 0.5),
                 (32, 64, 0.75),    # INTER_LINEAR from aligned rows
                 (16, 32, 1.0),     # the copy from aligned rows
                 (20, 400, 0.9)]    # a long row: six column tiles
# (h, w, net_h, net_w); net_w -1: the frame's own size
CAFFE_CASES = [(37, 53, 16, 20), (97, 100, 29, 33), (180, 200, 21, 23),   # the last: 8 to 9 taps
               (48, 64, 24, 32), (31, 33, 7, 11), (64, 64, -1, -1), (16, 16, 32, 32),
               (3, 2100, 2, 30),    # a source row wider than a wave stages: two column chunks
               (2, 600, 2, 300)]    # more than 256 output columns: two column chunks


def facenet_ref(frames, scale, mean):
    nh, nw = ref.facenet_geometry(frames.shape[1], frames.shape[2], scale)
    resized = np.stack([oracle.resize_u8(f, nw, nh) for f in frames])
    return ref.facenet_from_resized(resized, mean)


@pytest.fixture(scope="module")
def facenet_refs():
    """case -> (frames, {mean name: reference}) for 33 frames, computed once; smaller batches are prefixes."""
    out = {}
    for i, (h, w, scale) in enumerate(FACENET_CASES):
        frames = random_frames(100 + i, 33, h, w)
        out[(h, w, scale)] = (frames, {k: facenet_ref(frames, scale, m) for k, m in MEANS.items()})
    return out


@pytest.fixture(scope="module")
def caffe_refs():
    out = {}
    for i, (h, w, nh, nw) in enumerate(CAFFE_CASES):
        frames = random_frames(200 + i, 33, h, w)
        rh, rw = (h, w) if nw == -1 else (nh, nw)
        out[(h, w, nh, nw)] = (frames, {nz: ref.caffe_input(frames, rh, rw, MEANS["caffe"], nz) for nz in (False, True)})
    return out


@pytest.mark.parametrize("mean", list(MEANS))
@pytest.mark.parametrize("n", [1, 3, 33])
@pytest.mark.parametrize("h,w,scale", FACENET_CASES)
def test_facenet_input_bit_exact(hip_ctx, facenet_refs, h, w, scale, n, mean):
    frames, refs = facenet_refs[(h, w, scale)]
    assert facenet_geometry(h, w, scale) == ref.facenet_geometry(h, w, scale)
    got = hip_ctx.facenet_input(torch.from_numpy(frames[:n]).cuda(), scale, MEANS[mean])
    assert got.dtype == torch.float32 and tuple(got.shape) == refs[mean][:n].shape
    np.testing.assert_array_equal(got.cpu().numpy(), refs[mean][:n])


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("n", [1, 3, 33])
@pytest.mark.parametrize("h,w,nh,nw", CAFFE_CASES)
def test_caffe_input_bit_exact(hip_ctx, caffe_refs, h, w, nh, nw, n, normalize):
    frames, refs = caffe_refs[(h, w, nh, nw)]
    got = hip_ctx.caffe_input(torch.from_numpy(frames[:n]).cuda(), nw, nh, MEANS["caffe"], normalize)
    assert got.dtype == torch.float32 and tuple(got.shape) == refs[normalize][:n].shape
    np.testing.assert_array_equal(got.cpu().numpy(), refs[normalize][:n])


def _offset_view(a, offset_bytes):
    """`a` copied to the GPU into a buffer that starts `offset_bytes` past an allocation (which is 256-byte aligned)."""
    t = torch.from_numpy(a).cuda()
    raw = torch.empty(t.numel() * t.element_size() + offset_bytes, dtype=torch.uint8, device="cuda")
    v = raw[offset_bytes:].view(t.dtype).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == offset_bytes % 16 and v.is_contiguous()
    return v


@pytest.mark.parametrize("h,w,scale", [(48, 64, 0.5), (32, 64, 0.75), (16, 32, 1.0), (37, 53, 1.0)])
def test_facenet_input_unaligned_views_and_out(hip_ctx, facenet_refs, h, w, scale):
    """Frames that start 1 byte past an aligned address take the byte loads; an `out=` view 4 bytes past one takes the
    scalar stores; what surrounds the view stays as it was."""
    frames, refs = facenet_refs[(h, w, scale)]
    want = refs["caffe"][:3]
    np.testing.assert_array_equal(hip_ctx.facenet_input(_offset_view(frames[:3], 1), scale, MEANS["caffe"]).cpu().numpy(), want)
    raw = torch.full((want.size + 9,), 7.0, dtype=torch.float32, device="cuda")
    out = raw[1:1 + want.size].view(want.shape)
    assert out.data_ptr() % 16 == 4
    res = hip_ctx.facenet_input(torch.from_numpy(frames[:3]).cuda(), scale, MEANS["caffe"], out=out)
    assert res.data_ptr() == out.data_ptr()
    got = raw.cpu().numpy()
    np.testing.assert_array_equal(got[1:1 + want.size].reshape(want.shape), want)
    assert got[0] == 7.0 and (got[1 + want.size:] == 7.0).all()
    with pytest.raises(ValueError):
        hip_ctx.facenet_input(torch.from_numpy(frames[:3]).cuda(), scale, MEANS["caffe"], out=torch.empty((3, 3, 8, 8), device="cuda"))
    with pytest.raises(ValueError):
        hip_ctx.facenet_input(torch.from_numpy(frames[:3]).cuda(), scale, (1.0, 2.0))


@pytest.mark.parametrize("h,w,nh,nw", [(48, 64, 24, 32), (64, 64, -1, -1), (37, 53, 16, 20)])
def test_caffe_input_unaligned_views_and_out(hip_ctx, caffe_refs, h, w, nh, nw):
    frames, refs = caffe_refs[(h, w, nh, nw)]
    want = refs[True][:3]
    np.testing.assert_array_equal(hip_ctx.caffe_input(_offset_view(frames[:3], 1), nw, nh, MEANS["caffe"], True).cpu().numpy(), want)
    raw = torch.full((want.size + 9,), 7.0, dtype=torch.float32, device="cuda")
    out = raw[1:1 + want.size].view(want.shape)
    hip_ctx.caffe_input(torch.from_numpy(frames[:3]).cuda(), nw, nh, MEANS["caffe"], True, out=out)
    got = raw.cpu().numpy()
    np.testing.assert_array_equal(got[1:1 + want.size].reshape(want.shape), want)
    assert got[0] == 7.0 and (got[1 + want.size:] == 7.0).all()


@pytest.mark.parametrize("size,net", [(16, 24), (20, 30)])
def test_caffe_input_refuses_empty_windows_and_writes_nothing(hip_ctx, size, net):
    frames = torch.from_numpy(random_frames(3, 2, size, size)).cuda()
    out = torch.full((2, 3, net, net), 7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(_native.StError) as e:
        hip_ctx.caffe_input(frames, net, net, MEANS["zero"], out=out)
    assert e.value.status == _native.ST_ERR_UNSUPPORTED and "empty" in str(e.value)
    with pytest.raises(_native.StError) as e:     # the refusal is remembered per geometry: the same answer again
        hip_ctx.caffe_input(frames, net, net, MEANS["zero"], out=out)
    assert e.value.status == _native.ST_ERR_UNSUPPORTED
    hip_ctx.sync()
    assert bool((out == 7.0).all())
    # one enlarged axis is enough, and the context goes on working afterwards
    with pytest.raises(_native.StError):
        hip_ctx.caffe_input(frames, size, net, MEANS["zero"])
    np.testing.assert_array_equal(hip_ctx.caffe_input(frames, size, size, MEANS["zero"]).cpu().numpy(),
                                  ref.caffe_input(frames.cpu().numpy(), size, size, MEANS["zero"]))


def test_results_do_not_depend_on_how_a_batch_is_cut(hip_ctx, facenet_refs, caffe_refs):
    for (h, w, scale) in ((45, 61, 0.73), (48, 64, 0.5)):
        frames = torch.from_numpy(facenet_refs[(h, w, scale)][0]).cuda()
        whole = hip_ctx.facenet_input(frames, scale, MEANS["caffe"])
        parts = torch.cat([hip_ctx.facenet_input(frames[a:b], scale, MEANS["caffe"]) for a, b in ((0, 1), (1, 8), (8, 33))])
        assert torch.equal(whole, parts)
        assert torch.equal(whole, hip_ctx.facenet_input(list(frames.unbind(0)), scale, MEANS["caffe"]))    # a list of frames
    for key in ((97, 100, 29, 33), (48, 64, 24, 32)):
        frames = torch.from_numpy(caffe_refs[key][0]).cuda()
        whole = hip_ctx.caffe_input(frames, key[3], key[2], MEANS["caffe"])
        parts = torch.cat([hip_ctx.caffe_input(frames[a:b], key[3], key[2], MEANS["caffe"]) for a, b in ((0, 1), (1, 8), (8, 33))])
        assert torch.equal(whole, parts)
    # geometries alternate on one context: the tables of each are rebuilt, not mixed up
    a = torch.from_numpy(caffe_refs[(37, 53, 16, 20)][0][:2]).cuda()
    b = torch.from_numpy(caffe_refs[(31, 33, 7, 11)][0][:2]).cuda()
    for _ in range(2):
        np.testing.assert_array_equal(hip_ctx.caffe_input(a, 20, 16, MEANS["caffe"]).cpu().numpy(), caffe_refs[(37, 53, 16, 20)][1][False][:2])
        np.testing.assert_array_equal(hip_ctx.caffe_input(b, 11, 7, MEANS["caffe"]).cpu().numpy(), caffe_refs[(31, 33, 7, 11)][1][False][:2])
    assert tuple(hip_ctx.facenet_input(a[:0], 0.5, MEANS["zero"]).shape) == (0, 3, 0, 0)
    assert tuple(hip_ctx.caffe_input(a[:0], 4, 4, MEANS["zero"]).shape) == (0, 3, 0, 0)


def test_more_than_65535_frames_per_call(hip_ctx):
    """65 537 frames of 8 x 8: each entry point splits the call into launches of at most 65 535 frames."""
    n = 65537
    frames = random_frames(9, n, 8, 8)
    dev = torch.from_numpy(frames).cuda()
    for f in frames[:4]:
        np.testing.assert_array_equal(oracle.resize_u8(f, 8, 8), f)       # equal size is a copy: the resized batch is the batch
    got = hip_ctx.facenet_input(dev, 1.0, MEANS["caffe"])
    np.testing.assert_array_equal(got.cpu().numpy(), ref.facenet_from_resized(frames, MEANS["caffe"]))
    del got
    got = hip_ctx.caffe_input(dev, 4, 4, MEANS["caffe"], True)
    np.testing.assert_array_equal(got.cpu().numpy(), ref.caffe_input(frames, 4, 4, MEANS["caffe"], True))


@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("device", [DeviceType.GPU, DeviceType.CPU])
def test_ops_through_the_kernel_classes(hip_ctx, device, packed):
    """sc.ops.FacenetInput and sc.ops.CaffeInput on both registrations == the direct calls, with mean_colors packed and
    unpacked on the wire."""
    frames = random_frames(21, 5, 45, 61)
    dev = torch.from_numpy(frames).cuda()
    sc = Client()
    sc.ingest_frames("v", frames)
    frame = sc.io.Input([NamedVideoStream(sc, "v")])
    mean = MEANS["caffe"]
    for op, direct in ((sc.ops.FacenetInput(frame=frame, scale=0.73, mean_colors=mean, templates_path="unused", threshold=0.5,
                                            device=device, batch=3, packed=packed), hip_ctx.facenet_input(dev, 0.73, mean)),
                       (sc.ops.CaffeInput(frame=frame, input_width=20, input_height=16, mean_colors=mean, normalize=True,
                                          device=device, batch=2, packed=packed), hip_ctx.caffe_input(dev, 20, 16, mean, True)),
                       (sc.ops.CaffeInput(frame=frame, input_width=-1, input_height=0, mean_colors=mean, device=device,
                                          batch=8, packed=packed), hip_ctx.caffe_input(dev, -1, 0, mean))):
        out = NamedStream(sc, "net_in")
        sc.run(sc.io.Output(op, [out]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
        rows = list(out.load())
        assert len(rows) == 5
        for i, o in enumerate(rows):
            o = o.cpu().numpy() if isinstance(o, torch.Tensor) else np.asarray(o)
            assert o.dtype == np.float32
            np.testing.assert_array_equal(o, direct[i].cpu().numpy())


def test_ops_fail_validation_with_the_cause():
    frames = random_frames(22, 2, 8, 8)
    sc = Client()
    sc.ingest_frames("v", frames)
    frame = sc.io.Input([NamedVideoStream(sc, "v")])
    for op, what in ((lambda: sc.ops.FacenetInput(frame=frame, scale=0.0, mean_colors=(1, 2, 3), device=DeviceType.GPU), "scale must be positive"),
                     (lambda: sc.ops.FacenetInput(frame=frame, scale=1.0, mean_colors=(1, 2), device=DeviceType.GPU), "mean_colors must hold 3 values, got 2"),
                     (lambda: sc.ops.CaffeInput(frame=frame, input_width=4, input_height=4, mean_colors=(1, 2), device=DeviceType.GPU),
                      "mean_colors must hold 3 values, got 2")):
        with pytest.raises(RuntimeError, match=what):
            sc.run(sc.io.Output(op(), [NamedStream(sc, "o")]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)


def test_timing_slot(hip_ctx):
    frames = torch.from_numpy(random_frames(5, 2, 16, 32)).cuda()
    hip_ctx.timing_enable([_native.K_NET_INPUT])
    try:
        hip_ctx.timing_reset()
        hip_ctx.facenet_input(frames, 1.0, MEANS["zero"])
        hip_ctx.caffe_input(frames, 8, 8, MEANS["zero"])
        launches, ms = hip_ctx.timing_read(_native.K_NET_INPUT)
        assert launches == 2 and ms > 0.0          # one launch per call
    finally:
        hip_ctx.timing_enable([])


def test_full_hd_frames(hip_ctx):
    """The sizes the benchmark times (scripts/bench_net_input.py), two 1080p frames: aligned rows, every tile width the
    host picks at this size, a source row that fills a wave's staging slot."""
    frames = random_frames(31, 2, 1080, 1920)
    dev = torch.from_numpy(frames).cuda()
    for scale in (0.5, 1.0):
        np.testing.assert_array_equal(hip_ctx.facenet_input(dev, scale, MEANS["caffe"]).cpu().numpy(), facenet_ref(frames, scale, MEANS["caffe"]))
    for side in (224, 300):
        np.testing.assert_array_equal(hip_ctx.caffe_input(dev, side, side, MEANS["caffe"]).cpu().numpy(),
                                      ref.caffe_input(frames, side, side, MEANS["caffe"]))
