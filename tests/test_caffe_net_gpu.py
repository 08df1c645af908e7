"""The Caffe and Facenet ops on the GPU: every new layer kernel through the C ABI against torch in
float64 on the CPU, then both fixture networks end to end through the kernel classes against tests/ref_caffe_net.py.

Per-layer bound (the one test_conv_layer_matches_torch uses): max |err| <= 2e-5 * max(max |ref|, 1) and relative L2 <= 2e-6.
End-to-end bound (test_pose_network_end_to_end's, for a deeper network): max |err| <= 1e-3 * max |ref|."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_caffe_net as ref
from scannertools_amd import _native, engine
from scannertools_amd.engine import CacheMode, Client, DeviceType, NamedStream, NamedVideoStream, PerfParams
from util import random_frames

pytestmark = pytest.mark.gpu

GARBAGE = 3.0e30    # what the pad channels of an input hold in these tests: a kernel that let them take part would show it


def within_layer_bound(got, want, what=""):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double()
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    rel = float((got - want).norm() / want.norm())
    print("%s max |err| %.3g (scale %.3g), relative L2 %.3g" % (what, err, scale, rel))
    assert err <= 2e-5 * max(scale, 1.0), (err, scale)
    assert rel <= 2e-6, rel


def nhwc(x, stride=None, fill=GARBAGE):
    """(n, c, h, w) -> (n, h, w, stride) on the GPU, pad channels = fill."""
    n, c, h, w = x.shape
    out = torch.full((n, h, w, stride or (c + 15) // 16 * 16), fill, dtype=torch.float32)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out.cuda()


# ---- InnerProduct ----------------------------------------------------------------------------------------------------------
IP_CASES = [(1, 48, 10), (5, 4096, 96), (32, 1000, 130), (33, 2304, 1000)]


def _ip_operands(n, k, nout):
    g = torch.Generator().manual_seed(n * 7 + k + nout)
    return torch.randn((n, k), generator=g), torch.randn((nout, k), generator=g) * float(np.sqrt(2.0 / k)), torch.randn((nout,), generator=g) * 0.1


@pytest.mark.parametrize("relu,bias", [(False, True), (True, True), (True, False), (False, False)])
@pytest.mark.parametrize("n,k,nout", IP_CASES)
def test_inner_product_matches_torch(hip_ctx, n, k, nout, relu, bias):
    x, w, b = _ip_operands(n, k, nout)
    want = F.linear(x.double(), w.double(), b.double() if bias else None)
    if relu:
        want = torch.relu(want)
    packed = hip_ctx.inner_product_pack(w.cuda())
    out = torch.full((n, nout + 3), -7.0, dtype=torch.float32, device="cuda")
    hip_ctx.inner_product(x.cuda(), packed, nout, b.cuda() if bias else None, relu, out=out)
    got = out.cpu()
    within_layer_bound(got[:, :nout], want, "inner_product %s" % ((n, k, nout),))
    assert (got[:, nout:] == -7.0).all()                        # the guard beyond nout is untouched


def test_inner_product_bits_do_not_depend_on_the_batch(hip_ctx):
    n, k, nout = 33, 2304, 1000
    x, w, b = _ip_operands(n, k, nout)
    packed = hip_ctx.inner_product_pack(w.cuda())
    xd, bd = x.cuda(), b.cuda()
    whole = hip_ctx.inner_product(xd, packed, nout, bd, True)
    five = hip_ctx.inner_product(xd[:5].contiguous(), packed, nout, bd, True)
    assert torch.equal(whole[:5], five)
    for i in range(5):
        assert torch.equal(hip_ctx.inner_product(xd[i:i + 1].contiguous(), packed, nout, bd, True)[0], whole[i])
    assert torch.equal(hip_ctx.inner_product(xd[32:].contiguous(), packed, nout, bd, True)[0], whole[32])   # the second launch's row
    with pytest.raises(_native.StError):
        hip_ctx.inner_product(xd[:, :2301].contiguous(), packed, nout)                                           # k not a multiple of 8


# ---- general convolution ---------------------------------------------------------------------------------------------------
GCONV_CASES = [(7, 2, 3, 1, 3, 32, 35, 43), (11, 4, 0, 1, 3, 24, 51, 47), (5, 1, 2, 2, 32, 48, 13, 17), (3, 2, 0, 1, 20, 20, 13, 17),
               (1, 2, 0, 1, 64, 64, 13, 17)]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("k,s,p,g,ci,co,h,w", GCONV_CASES)
def test_general_convolution_matches_torch(hip_ctx, k, s, p, g, ci, co, h, w, relu):
    gen = torch.Generator().manual_seed(k * 100 + ci + co)
    x = torch.randn((2, ci, h, w), generator=gen)
    wt = torch.randn((co, ci // g, k, k), generator=gen) * float(np.sqrt(2.0 / (ci // g * k * k)))
    b = torch.randn((co,), generator=gen) * 0.1
    want = F.conv2d(x.double(), wt.double(), b.double(), stride=s, padding=p, groups=g)
    if relu:
        want = torch.relu(want)
    out = torch.full((2, want.shape[2], want.shape[3], co + 9), -7.0, dtype=torch.float32, device="cuda")
    hip_ctx.conv2d_general(nhwc(x), ci, wt.permute(0, 2, 3, 1).contiguous().cuda(), b.cuda(), s, p, g, relu, out=out, y_offset=5)
    got = out.cpu()
    within_layer_bound(got[..., 5:5 + co].permute(0, 3, 1, 2), want, "conv %s" % ((k, s, p, g, ci, co),))
    assert (got[..., :5] == -7.0).all() and (got[..., 5 + co:] == -7.0).all()


def test_general_convolution_agrees_with_the_mfma_kernel(hip_ctx):
    import ctypes
    gen = torch.Generator().manual_seed(9)
    n, ci, co, h, w, k = 2, 16, 64, 13, 17, 3
    x = torch.randn((n, ci, h, w), generator=gen)
    wt = torch.randn((co, ci, k, k), generator=gen) * float(np.sqrt(2.0 / (ci * k * k)))
    b = torch.randn((co,), generator=gen) * 0.1
    want = torch.relu(F.conv2d(x.double(), wt.double(), b.double(), padding=1))
    xd = nhwc(x)
    wd = wt.permute(0, 2, 3, 1).contiguous().cuda()
    general = hip_ctx.conv2d_general(xd, ci, wd, b.cuda(), 1, 1, 1, True)
    mfma = torch.zeros_like(general)
    hip_ctx._bind()
    hip_ctx._check(hip_ctx._L.st_conv2d_nhwc_f32(hip_ctx._h, ctypes.c_void_p(xd.data_ptr()), n, h, w, ci, ci, 0, ctypes.c_void_p(wd.data_ptr()),
                                                 ctypes.c_void_p(b.cuda().data_ptr()), k, k, co, co, 1, ctypes.c_void_p(mfma.data_ptr()), co, 0))
    within_layer_bound(general.permute(0, 3, 1, 2), want, "general")
    within_layer_bound(mfma.permute(0, 3, 1, 2), want, "mfma")
    within_layer_bound(general, mfma.cpu(), "general against mfma")


# ---- Pooling ---------------------------------------------------------------------------------------------------------------
POOL_MAPS = [(13, 17, 20), (5, 7, 64)]
POOL_GEOM = [(3, 2, 0), (3, 1, 1), (2, 2, 0), (5, 3, 2), (2, 2, 1), None]    # None: global


@pytest.mark.parametrize("method", ["MAX", "AVE"])
@pytest.mark.parametrize("geom", POOL_GEOM)
@pytest.mark.parametrize("h,w,c", POOL_MAPS)
def test_pooling_matches_torch(hip_ctx, h, w, c, geom, method):
    gen = torch.Generator().manual_seed(h * w + c)
    x = torch.randn((3, c, h, w), generator=gen)
    xd = x.double()
    if geom is None:
        want = xd.mean(dim=(2, 3), keepdim=True) if method == "AVE" else xd.amax(dim=(2, 3), keepdim=True)
        got = hip_ctx.pool(nhwc(x), c, getattr(_native, "POOL_" + method), global_pooling=True)
    else:
        k, s, p = geom
        want = (F.avg_pool2d(xd, k, s, p, ceil_mode=True, count_include_pad=True) if method == "AVE" else F.max_pool2d(xd, k, s, p, ceil_mode=True))
        got = hip_ctx.pool(nhwc(x), c, getattr(_native, "POOL_" + method), k, s, p)
    got = got.cpu()
    assert tuple(got.shape[:3]) == (3, want.shape[2], want.shape[3])
    if method == "MAX":
        np.testing.assert_array_equal(got[..., :c].permute(0, 3, 1, 2).numpy(), want.float().numpy())    # bit-exact
    else:
        within_layer_bound(got[..., :c].permute(0, 3, 1, 2), want, "AVE %s" % (geom,))
    assert got.shape[3] == (c + 15) // 16 * 16 and (got[..., c:] == 0.0).all()      # pad channels stay zero


def test_pooling_less_one_rule_and_slices(hip_ctx):
    x = torch.arange(2 * 4 * 5 * 5, dtype=torch.float32).reshape(2, 4, 5, 5)
    want = F.max_pool2d(x, 2, 2, 1, ceil_mode=True)
    assert tuple(want.shape) == (2, 4, 3, 3)
    buf = nhwc(torch.cat([torch.full_like(x, GARBAGE), x], dim=1), 16)     # the layer reads channels 4 .. 7 of a wider buffer
    out = torch.full((2, 3, 3, 16), -7.0, dtype=torch.float32, device="cuda")
    hip_ctx.pool(buf, 4, _native.POOL_MAX, 2, 2, 1, x_offset=4, out=out, y_offset=9)
    got = out.cpu()
    np.testing.assert_array_equal(got[..., 9:13].permute(0, 3, 1, 2).numpy(), want.numpy())
    assert (got[..., :9] == -7.0).all() and (got[..., 13:] == -7.0).all()
    with pytest.raises(_native.StError):
        hip_ctx.pool(buf, 4, _native.POOL_MAX, 2, 2, 2)                    # pad >= kernel: Caffe refuses it


# ---- LRN, Softmax, copies ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [5, 3])
@pytest.mark.parametrize("c", [20, 64])
def test_lrn_matches_torch(hip_ctx, c, size):
    x = torch.randn((2, c, 7, 9), generator=torch.Generator().manual_seed(c + size)) * 3
    for alpha, beta, k in ((1e-2, 0.75, 1.0), (1e-4, 0.75, 2.0)):
        want = F.local_response_norm(x.double(), size, alpha, beta, k)
        got = hip_ctx.lrn(nhwc(x), c, size, alpha, beta, k).cpu()
        within_layer_bound(got[..., :c].permute(0, 3, 1, 2), want, "lrn %s" % ((c, size, alpha, k),))
        assert (got[..., c:] == 0.0).all()


@pytest.mark.parametrize("c", [10, 12, 1000])
def test_softmax_matches_torch(hip_ctx, c):
    x = torch.randn((5, c, 2, 3), generator=torch.Generator().manual_seed(c)) * 4
    want = torch.softmax(x.double(), dim=1)
    got = hip_ctx.softmax(nhwc(x), c).cpu()
    within_layer_bound(got[..., :c].permute(0, 3, 1, 2), want, "softmax %d" % c)
    sums = got[..., :c].double().sum(dim=3)
    print("softmax %d: rows sum to 1 within %.3g" % (c, float((sums - 1).abs().max())))
    assert float((sums - 1).abs().max()) <= 1e-6
    assert (got[..., c:] == 0.0).all()
    big = torch.full((1, 4, 1, 1), 1000.0)                        # the maximum is subtracted: no overflow
    np.testing.assert_array_equal(hip_ctx.softmax(nhwc(big), 4).cpu()[0, 0, 0, :4].numpy(), np.full(4, 0.25, np.float32))


def test_planar_output_and_channel_copies_are_exact(hip_ctx):
    x = torch.randn((3, 20, 5, 7), generator=torch.Generator().manual_seed(4))
    xd = nhwc(x)
    assert torch.equal(hip_ctx.nhwc_to_planar(xd, 20).cpu(), x)
    assert torch.equal(hip_ctx.nhwc_to_planar(xd, 7, x_offset=11).cpu(), x[:, 11:18])
    out = torch.full((3, 5, 7, 48), -7.0, dtype=torch.float32, device="cuda")
    hip_ctx.copy_channels(xd, 12, 3, out, 20)
    hip_ctx.copy_channels(xd, 5, 0, out, 40, relu=True)
    got = out.cpu()
    assert torch.equal(got[..., 20:32].permute(0, 3, 1, 2), x[:, 3:15]) and torch.equal(got[..., 40:45].permute(0, 3, 1, 2), torch.relu(x[:, :5]))
    assert (got[..., :20] == -7.0).all() and (got[..., 32:40] == -7.0).all() and (got[..., 45:] == -7.0).all()


# ---- end to end through the kernel classes -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nets(tmp_path_factory):
    """Both fixture networks, 7 input frames each and the float64 reference's blobs, computed once."""
    d = str(tmp_path_factory.mktemp("caffe_nets"))
    out = {}
    for name, make, shape in (("vgg", ref.mini_vgg, (3, 32, 32)), ("inception", ref.mini_inception, (3, 35, 43))):
        prototxt, caffemodel = make(d)
        x = (np.random.default_rng(len(name)).standard_normal((7,) + shape) * 40).astype(np.float32)
        out[name] = (prototxt, caffemodel, x, ref.forward(prototxt, caffemodel, x))
    return out


def run_caffe(frames, prototxt, caffemodel, blob, device=DeviceType.GPU, batch_size=0, batch=None, op="Caffe", **kw):
    sc = Client()
    sc.ingest_frames("v", frames)
    frame = sc.io.Input([NamedVideoStream(sc, "v")])
    node = getattr(sc.ops, op)(frame, prototxt, caffemodel, ["data"], [blob], batch_size=batch_size, device=device, batch=batch, **kw)
    out = NamedStream(sc, "o")
    sc.run(sc.io.Output(node, [out]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    rows = [np.asarray(r) for r in out.load()]
    assert sc.live_device_buffers() == 0 and engine._caffe().stshim_live_buffers(DeviceType.GPU) == 0
    return np.stack(rows), sc


def within_net_bound(got, want, what):
    err, scale = float(np.abs(got.astype(np.float64) - want).max()), float(np.abs(want).max())
    print("%s: max |err| %.3g, max |ref| %.3g, ratio %.3g" % (what, err, scale, err / scale))
    assert err <= 1e-3 * scale, (err, scale)


@pytest.mark.parametrize("device", [DeviceType.GPU, DeviceType.CPU])
@pytest.mark.parametrize("name,blob", [("vgg", "prob"), ("vgg", "fc7"), ("inception", "prob"), ("inception", "inc2/output")])
def test_networks_end_to_end(nets, name, blob, device):
    prototxt, caffemodel, x, blobs = nets[name]
    want = ref.frame_shaped(blobs[blob])
    got, sc = run_caffe(x, prototxt, caffemodel, blob, device, batch_size=3, batch=4)
    assert got.dtype == np.float32 and got.shape == want.shape
    within_net_bound(got, want, "%s %s" % (name, blob))
    # the engine hands over 4 + 3 frames, the kernel runs them 3 at a time: 3 + 1 and 3
    assert sc.profile["caffe:net"][0] == 3 and sc.profile["caffe:net"][1] > 0


@pytest.mark.parametrize("name,blob", [("vgg", "prob"), ("inception", "prob"), ("inception", "inc2/output")])
def test_network_bits_do_not_depend_on_batching_or_kernel_choice(nets, name, blob, monkeypatch):
    prototxt, caffemodel, x, _ = nets[name]
    first, _ = run_caffe(x, prototxt, caffemodel, blob, batch_size=3, batch=4)
    for batch_size, batch, device in ((1, 7, DeviceType.GPU), (7, 2, DeviceType.GPU), (0, 5, DeviceType.GPU), (0, 7, DeviceType.CPU)):
        again, _ = run_caffe(x, prototxt, caffemodel, blob, device, batch_size=batch_size, batch=batch)
        np.testing.assert_array_equal(again, first)
    for tile in ("0", "1"):                                         # the convolution kernel the library picks (read at st_ctx_create)
        monkeypatch.setenv("ST_CONV_TILE", tile)
        again, _ = run_caffe(x, prototxt, caffemodel, blob, batch_size=0, batch=7)
        np.testing.assert_array_equal(again, first)


def test_a_new_frame_size_replans(nets):
    """One kernel instance would re-plan; here two sizes through the same description: everything before the global pooling
    scales with the frame."""
    prototxt, caffemodel, _, _ = nets["inception"]
    x = (np.random.default_rng(5).standard_normal((2, 3, 50, 38)) * 40).astype(np.float32)
    blobs = ref.forward(prototxt, caffemodel, x)
    for blob in ("inc1/output", "prob"):
        got, _ = run_caffe(x, prototxt, caffemodel, blob, batch=2)
        want = ref.frame_shaped(blobs[blob])
        assert got.shape == want.shape
        within_net_bound(got, want, "50 x 38 " + blob)


def test_caffe_input_feeds_caffe(hip_ctx, nets):
    """frames -> CaffeInput(32 x 32) -> Caffe as one graph."""
    prototxt, caffemodel, _, _ = nets["vgg"]
    frames = random_frames(41, 5, 45, 61)
    mean = (104.00699, 116.66877, 122.67892)
    net_in = hip_ctx.caffe_input(torch.from_numpy(frames).cuda(), 32, 32, mean).cpu().numpy()     # bit-exact: test_net_input_gpu.py
    want = ref.frame_shaped(ref.forward(prototxt, caffemodel, net_in)["prob"])
    sc = Client()
    sc.ingest_frames("v", frames)
    frame = sc.io.Input([NamedVideoStream(sc, "v")])
    caffe_frame = sc.ops.CaffeInput(frame=frame, input_width=32, input_height=32, mean_colors=mean, device=DeviceType.GPU, batch=3)
    prob = sc.ops.Caffe(caffe_frame, prototxt, caffemodel, ["data"], ["prob"], batch_size=2, device=DeviceType.GPU, batch=5,
                        input_width=32, input_height=32)
    out = NamedStream(sc, "prob")
    sc.run(sc.io.Output(prob, [out]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    got = np.stack([np.asarray(r) for r in out.load()])
    assert got.shape == (5, 10, 1, 1)
    within_net_bound(got, want, "CaffeInput -> Caffe")
    assert sc.profile["caffe:net"][0] == 3                           # 5 frames, 2 at a time


def test_facenet_input_feeds_facenet(hip_ctx, nets):
    """frames -> FacenetInput(scale 0.5) -> Facenet on the convolutional trunk: FacenetInput's planes are W x H, and the network runs
    on them as they are -- the reference fed the transposed input."""
    prototxt, caffemodel, _, _ = nets["inception"]
    frames = random_frames(42, 3, 70, 86)
    mean = (104.00699, 116.66877, 122.67892)
    net_in = hip_ctx.facenet_input(torch.from_numpy(frames).cuda(), 0.5, mean).cpu().numpy()       # bit-exact: test_net_input_gpu.py
    assert net_in.shape == (3, 3, 48, 40)                            # (3, net_w, net_h): 43 -> 48 columns, 35 -> 40 rows
    want = ref.frame_shaped(ref.forward(prototxt, caffemodel, net_in)["inc2/output"])
    assert want.shape[2] != want.shape[3]                            # a swapped plane order could not pass
    for device in (DeviceType.GPU, DeviceType.CPU):
        sc = Client()
        sc.ingest_frames("v", frames)
        frame = sc.io.Input([NamedVideoStream(sc, "v")])
        fin = sc.ops.FacenetInput(frame=frame, scale=0.5, mean_colors=mean, device=device, batch=2)
        feat = sc.ops.Facenet(fin, prototxt, caffemodel, ["data"], ["inc2/output"], scale=0.5, mean_colors=mean, batch_size=2, device=device, batch=3)
        out = NamedStream(sc, "feat")
        sc.run(sc.io.Output(feat, [out]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
        got = np.stack([np.asarray(r) for r in out.load()])
        assert got.shape == want.shape
        within_net_bound(got, want, "FacenetInput -> Facenet")
        assert sc.profile["caffe:net"][0] == 2
        assert sc.live_device_buffers() == 0 and engine._caffe().stshim_live_buffers(DeviceType.GPU) == 0


def test_timing_goes_to_the_conv_slot(hip_ctx):
    x = torch.randn((2, 16), generator=torch.Generator().manual_seed(1))
    w = torch.randn((4, 16), generator=torch.Generator().manual_seed(2))
    packed = hip_ctx.inner_product_pack(w.cuda())
    hip_ctx.timing_enable([_native.K_CONV])
    try:
        hip_ctx.timing_reset()
        hip_ctx.inner_product(x.cuda(), packed, 4)
        hip_ctx.softmax(nhwc(torch.zeros(1, 4, 2, 2)), 4)
        launches, ms = hip_ctx.timing_read(_native.K_CONV)
        assert launches == 2 and ms > 0.0
    finally:
        hip_ctx.timing_enable([])
