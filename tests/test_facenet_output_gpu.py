"""FacenetOutput on the GPU: st_facenet_output_batch and st_bbox_nms_f32 against the numpy restatement
(tests/ref_facenet_output_np.py), bit for bit on count, order, coordinates and score; then the op through the engine on both
registrations, alone and behind FacenetInput -> Facenet.  Every test first checks on the CPU that no score lies within 1e-6 of
the threshold, so that no decision rests on a last bit of the sigmoid."""
import numpy as np
import pytest
import torch

import ref_facenet_output_np as ref
from scannertools_amd import _native, caffe_net, engine, types
from scannertools_amd.engine import CacheMode, Client, DeviceType, NamedStream, NamedVideoStream, PerfParams
from util import random_frames

pytestmark = pytest.mark.gpu

F = np.float32
T = ref.templates()
# (h, w, scale, threshold, logit bias, seed): grid_w != grid_h everywhere
CASES = {
    "9x6": (67, 93, 0.73, 0.5, -1.3, 1),          # 810 candidates, 74 survivors
    "24x12": (96, 192, 1.0, 0.5, -2.1, 2),        # 4 320 candidates, 79 survivors
    "12x9-big": (48, 64, 1.5, 0.5, -0.3, 3),      # scale above 1: the 8-template list, 339 survivors
    "40x23-all": (184, 320, 1.0, 0.0, 0.0, 4),    # threshold 0: all 13 800 candidates survive -- more than LDS holds; equal scores
}
_cache = {}


def case(name):
    """(map, the restatement's kept rows, survivors), computed once."""
    if name not in _cache:
        h, w, scale, thr, bias, seed = CASES[name]
        _, _, gh, gw = ref.geometry(h, w, scale)
        m = ref.make_map(seed, gw, gh, bias)
        assert ref.threshold_margin(m, h, w, scale, T, thr) > 1e-6
        rows, _, _ = ref.decode(m, h, w, scale, T, thr)
        _cache[name] = (m, rows[ref.nms(rows)], rows)
    return _cache[name]


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("name", list(CASES))
def test_single_frames_match_the_restatement(hip_ctx, name):
    h, w, scale, thr, _, _ = CASES[name]
    m, want, survivors = case(name)
    print("%s: %d survivors, %d kept, %d equal scores" % (name, len(survivors), len(want), len(survivors) - len(np.unique(survivors[:, 4]))))
    assert len(want) >= 2 and (np.diff(want[:, 4]) <= 0).all()
    if name == "40x23-all":
        assert len(survivors) == 13800 and len(np.unique(survivors[:, 4])) < 13800
    got = hip_ctx.facenet_output(torch.from_numpy(m)[None].cuda(), h, w, scale, T, thr)
    assert len(got) == 1
    same_bits(got[0], want)
    # the other overlap and the pixel offset take the same path through the entry point
    for overlap, offset in ((0.3, 0.0), (0.1, 1.0)):
        got = hip_ctx.facenet_output(torch.from_numpy(m)[None].cuda(), h, w, scale, T, thr, overlap, offset)
        same_bits(got[0], survivors[ref.nms(survivors, overlap, offset)])


@pytest.fixture(scope="module")
def batch33():
    """33 maps of one geometry with different survivor counts, frame 1 with none, and their restated rows."""
    h, w, scale, thr = 67, 93, 0.73, 0.5
    biases = [-1.3, -30.0, 0.5, -2.5, -0.5, -1.8]
    maps = np.stack([ref.make_map(100 + i, 9, 6, biases[i % 6] - 0.01 * (i // 6)) for i in range(33)])
    for m in maps:
        assert ref.threshold_margin(m, h, w, scale, T, thr) > 1e-6
    want = [ref.facenet_output(m, h, w, scale, T, thr) for m in maps]
    assert len(want[1]) == 0 and len({len(r) for r in want}) >= 4
    return (h, w, scale, thr), maps, want


@pytest.mark.parametrize("n", [1, 5, 33])
def test_batches_do_not_change_a_frame(hip_ctx, batch33, n):
    (h, w, scale, thr), maps, want = batch33
    got = hip_ctx.facenet_output(torch.from_numpy(maps[:n]).cuda(), h, w, scale, T, thr)
    assert len(got) == n
    for g, r in zip(got, want):
        same_bits(g, r)
    # every map its own allocation, 4 bytes past a 16-byte boundary, in another order
    order = list(range(n))[::-1]
    views = []
    for i in order:
        buf = torch.empty(maps[i].size + 1, dtype=torch.float32, device="cuda")
        buf[1:] = torch.from_numpy(maps[i].reshape(-1)).cuda()
        views.append(buf[1:])
        assert views[-1].data_ptr() % 16 == 4
    got = hip_ctx.facenet_output(views, h, w, scale, T, thr)
    for g, i in zip(got, order):
        same_bits(g, want[i])


def test_a_threshold_nothing_passes_and_an_empty_batch(hip_ctx, batch33):
    (h, w, scale, _), maps, _ = batch33
    thr = 0.9999999
    for m in maps[:5]:
        _, _, score = ref.decode(m, h, w, scale, T, thr)
        assert score.max() < thr - 1e-6
    got = hip_ctx.facenet_output(torch.from_numpy(maps[:5]).cuda(), h, w, scale, T, thr)
    assert [g.shape for g in got] == [(0, 5)] * 5
    assert hip_ctx.facenet_output([], h, w, scale, T, thr) == []


def test_bad_arguments_are_errors(hip_ctx):
    m = torch.zeros((1, 125, 9, 6), device="cuda")
    for kw in (dict(threshold=float("nan")), dict(threshold=float("inf")), dict(overlap=float("nan")), dict(scale=0.0), dict(scale=1e-4)):
        args = dict(h=67, w=93, scale=0.73, templates=T, threshold=0.5)
        args.update(kw)
        with pytest.raises(_native.StError):
            hip_ctx.facenet_output(m, **args)
    L, c = hip_ctx._L, hip_ctx._h
    import ctypes
    one = (ctypes.c_int32 * 1)()
    tp = T.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    ptr = (ctypes.c_void_p * 1)(m.data_ptr())
    assert L.st_facenet_output_batch(c, ptr, -1, 67, 93, 0.73, tp, 0.5, 0.1, 0.0, one) == _native.ST_ERR_INVALID
    assert L.st_facenet_output_batch(c, None, 1, 67, 93, 0.73, tp, 0.5, 0.1, 0.0, one) == _native.ST_ERR_INVALID
    assert L.st_facenet_output_batch(c, ptr, 1, 67, 93, 0.73, None, 0.5, 0.1, 0.0, one) == _native.ST_ERR_INVALID
    assert L.st_facenet_output_batch(c, ptr, 1, 67, 93, 0.73, tp, 0.5, 0.1, 0.0, None) == _native.ST_ERR_INVALID
    assert L.st_facenet_output_batch(c, (ctypes.c_void_p * 1)(None), 1, 67, 93, 0.73, tp, 0.5, 0.1, 0.0, one) == _native.ST_ERR_INVALID
    assert L.st_facenet_output_fetch(c, None, 0) == _native.ST_ERR_INVALID       # after a failed call there is nothing to fetch
    assert L.st_bbox_nms_f32(c, None, one, -1, 0.1, 0.0, None, one) == _native.ST_ERR_INVALID
    assert L.st_bbox_nms_f32(c, None, None, 1, 0.1, 0.0, None, one) == _native.ST_ERR_INVALID
    assert L.st_bbox_nms_f32(c, None, (ctypes.c_int32 * 1)(-2), 1, 0.1, 0.0, None, one) == _native.ST_ERR_INVALID
    assert L.st_bbox_nms_f32(c, None, (ctypes.c_int32 * 1)(3), 1, 0.1, 0.0, None, one) == _native.ST_ERR_INVALID   # rows are null
    assert L.st_bbox_nms_f32(c, ctypes.c_void_p(m.data_ptr()), (ctypes.c_int32 * 1)(3), 1, float("nan"), 0.0, ctypes.c_void_p(m.data_ptr()), one) == _native.ST_ERR_INVALID


# ---- the suppression alone --------------------------------------------------------------------------------------------------
def hand_made_sets():
    a, b, c, z, d = (0, 0, 1, 1), (0, 0, .5, .5), (2, 2, 3, 3), (5, 5, 5, 6), (1.5, 0, 2.5, 1)
    nan = float("nan")
    rows = lambda *bs: np.asarray([box + (s,) for box, s in bs], F)
    return [rows((a, .9), (b, .8), (c, .7)),                       # nested and disjoint
            rows((a, .8), (b, .9), (c, .7)),                       # a quarter of the larger box: the overlap threshold decides
            rows((c, .5), (a, .5), (a, .5), (b, .5)),              # equal scores, identical boxes
            rows((a, .9), (z, .8)), rows((z, .9), (a, .8)),        # a zero-area box, second and first
            rows((a, .9), (d, .8)),                                # half a unit apart: the offset decides
            rows((c, .9), ((nan, 0, 1, 1), .8), (a, .7)),          # a NaN coordinate in a box under test
            rows(((0, nan, 1, 1), .9), (a, .8), (c, .7)),          # ... and in the kept box
            rows((a, nan), (b, .8), (c, 0.0)),                     # a NaN score goes first (its bit pattern is the largest)
            rows((a, .3)),
            np.zeros((0, 5), F)]


@pytest.mark.parametrize("overlap,offset", [(0.1, 0.0), (0.3, 0.0), (0.1, 1.0), (0.3, 1.0)])
def test_bbox_nms_on_hand_made_boxes(hip_ctx, overlap, offset):
    sets = hand_made_sets()
    want = [ref.nms(s, overlap, offset) for s in sets]
    if (overlap, offset) == (0.1, 0.0):                               # the answers worked out in tests/test_facenet_output.py
        assert [k.tolist() for k in want[:6]] == [[0, 2], [1, 2], [0, 1], [0], [0, 1], [0, 1]]
    if (overlap, offset) == (0.3, 0.0):
        assert want[1].tolist() == [1, 0, 2]
    if (overlap, offset) == (0.1, 1.0):
        assert want[5].tolist() == [0]
    # one call for all sets, and each set on its own
    got = hip_ctx.bbox_nms(torch.from_numpy(np.concatenate(sets)).cuda(), [len(s) for s in sets], overlap, offset)
    assert [g.tolist() for g in got] == [k.tolist() for k in want]
    for s, k in zip(sets, want):
        if len(s):
            assert hip_ctx.bbox_nms(torch.from_numpy(s).cuda(), None, overlap, offset)[0].tolist() == k.tolist()


def random_boxes(seed, m):
    """m boxes in the unit square, small enough that hundreds survive, scores drawn from 512 values so that many are equal."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0, 1, (m, 2))
    s = rng.uniform(0.005, 0.03, (m, 2))
    score = rng.integers(1, 513, m) / 512.0
    return np.concatenate([c - s, c + s, score[:, None]], axis=1).astype(F)


def test_bbox_nms_at_the_lds_capacity_and_around_the_workgroup_size(hip_ctx):
    """6 144 boxes are sorted in LDS, 6 145 in global scratch; 1 023 .. 1 025 straddle the workgroup; 2 and 3 the smallest
    networks.  All in one call, so sets on both paths share a launch."""
    sizes = [6144, 6145, 1023, 1024, 1025, 2, 3, 0, 2049]
    sets = [random_boxes(10 + i, m) for i, m in enumerate(sizes)]
    want = [ref.nms(s) for s in sets]
    print("kept:", [len(k) for k in want])
    assert len(want[0]) > 300 and len(want[1]) > 300
    got = hip_ctx.bbox_nms(torch.from_numpy(np.concatenate(sets)).cuda(), sizes)
    for g, k in zip(got, want):
        assert g.tolist() == k.tolist()
    # the same boxes give the same answer on either path: 6 145 boxes of which the last is a copy of the first
    s = np.concatenate([sets[0], sets[0][:1]])
    assert hip_ctx.bbox_nms(torch.from_numpy(s).cuda())[0].tolist() == want[0].tolist()


def test_launches_are_counted_in_the_nms_slot_only(hip_ctx):
    h, w, scale, thr, _, _ = CASES["9x6"]
    m, want, _ = case("9x6")
    hip_ctx.timing_enable(range(_native.K_COUNT))
    try:
        hip_ctx.timing_reset()
        got = hip_ctx.facenet_output(torch.from_numpy(m)[None].cuda(), h, w, scale, T, thr)
        same_bits(got[0], want)
        counts = [hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)]
        assert counts[_native.K_CPM2_NMS] == 3 and sum(counts) == 3               # decode, sort + suppression, pack
        assert hip_ctx.timing_read(_native.K_CPM2_NMS)[1] > 0
        hip_ctx.timing_reset()
        hip_ctx.bbox_nms(torch.from_numpy(random_boxes(1, 50)).cuda())
        counts = [hip_ctx.timing_read(k)[0] for k in range(_native.K_COUNT)]
        assert counts[_native.K_CPM2_NMS] == 1 and sum(counts) == 1
    finally:
        hip_ctx.timing_enable([])
        hip_ctx.timing_reset()


# ---- through the engine ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def templates_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("facenet_output") / "templates.bin"
    p.write_bytes(T.tobytes())
    return str(p)


def no_live_buffers(sc):
    assert sc.live_device_buffers() == 0 and engine._caffe().stshim_live_buffers(DeviceType.GPU) == 0


@pytest.mark.parametrize("device", [DeviceType.GPU, DeviceType.CPU])
def test_the_op_equals_the_direct_call(hip_ctx, batch33, templates_file, device):
    (h, w, scale, thr), maps, want = batch33
    n = 7
    direct = hip_ctx.facenet_output(torch.from_numpy(maps[:n]).cuda(), h, w, scale, T, thr)
    sc = Client()
    sc.ingest_frames("maps", maps[:n])
    sc.ingest_frames("v", np.zeros((n, h, w, 3), np.uint8))
    info = sc.ops.InfoFromFrame(frame=sc.io.Input([NamedVideoStream(sc, "v")]))
    boxes = sc.ops.FacenetOutput(facenet_output=sc.io.Input([NamedVideoStream(sc, "maps")]), original_frame_info=info, scale=scale,
                                 threshold=thr, templates_path=templates_file, device=device, batch=3)
    out = NamedStream(sc, "boxes")
    sc.run(sc.io.Output(boxes, [out]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    raw = out._frames()
    assert len(raw) == n
    for i, (e, r) in enumerate(zip(raw, out.load())):
        same_bits(r, direct[i])
        same_bits(r, want[i])
        assert e == types.write_scored_bboxes(want[i])                           # the element's bytes, field for field
    assert raw[1] == (0).to_bytes(8, "little")                                   # a frame without boxes: the 8-byte count
    no_live_buffers(sc)


@pytest.mark.parametrize("device", [DeviceType.GPU, DeviceType.CPU])
def test_frames_to_boxes_through_the_whole_chain(tmp_path, templates_file, device):
    """frames -> FacenetInput -> Facenet -> FacenetOutput with a three-convolution detector, against the restatement applied to the
    Facenet column downloaded in the same run.  The grid is 9 x 6: a swapped xi / yi cannot pass."""
    h, w, scale, thr = 67, 93, 0.73, 0.5
    nh, nw, gh, gw = ref.geometry(h, w, scale)
    net = caffe_net.NetBuilder(3, nw, nh, seed=7, name="detector")             # FacenetInput's planes are W x H
    top = net.conv("conv1", "data", 16, 3, stride=2, pad=1)
    top = net.conv("conv2", top, 32, 3, stride=2, pad=1)
    top = net.conv("conv3", top, 125, 3, stride=2, pad=1, relu=False)
    assert net.shapes[top] == (125, gw, gh)
    net.weights["conv1"][0] *= F(1 / 64)                                        # pixels minus the mean are of the order of 100
    net.weights["conv3"][0][:25] *= F(1.5)                                      # logits of deviation 1.3 around -1.5: one candidate
    net.weights["conv3"][1][:25] -= F(1.5)                                      # in seven passes the threshold
    net.weights["conv3"][0][25:] *= F(0.25)                                     # adjustments of deviation 0.25
    prototxt, caffemodel = net.write(str(tmp_path))
    frames = random_frames(43, 5, h, w)
    mean = (104.00699, 116.66877, 122.67892)
    sc = Client()
    sc.ingest_frames("v", frames)
    frame = sc.io.Input([NamedVideoStream(sc, "v")])
    fin = sc.ops.FacenetInput(frame=frame, scale=scale, mean_colors=mean, device=device, batch=2)
    maps = sc.ops.Facenet(fin, prototxt, caffemodel, ["data"], [top], scale=scale, mean_colors=mean, batch_size=2, device=device, batch=3)
    boxes = sc.ops.FacenetOutput(facenet_output=maps, original_frame_info=sc.ops.InfoFromFrame(frame=frame), scale=scale, threshold=thr,
                                 templates_path=templates_file, mean_colors=mean, device=device, batch=4)
    out_maps, out_boxes = NamedStream(sc, "maps"), NamedStream(sc, "boxes")
    sc.run([sc.io.Output(maps, [out_maps]), sc.io.Output(boxes, [out_boxes])], PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    got_maps = [np.asarray(m) for m in out_maps.load()]
    got = list(out_boxes.load())
    assert len(got) == 5 and got_maps[0].shape == (125, gw, gh)
    kept = []
    for m, g in zip(got_maps, got):
        assert ref.threshold_margin(m, h, w, scale, T, thr) > 1e-6
        survivors, _, _ = ref.decode(m, h, w, scale, T, thr)
        same_bits(g, survivors[ref.nms(survivors)])
        kept.append((len(survivors), len(g)))
    print("survivors, kept per frame:", kept)
    assert sum(k for _, k in kept) >= 5 and max(s for s, _ in kept) < 810        # the detector neither sleeps nor fires everywhere
    no_live_buffers(sc)
