"""The Caffe and Facenet ops without a GPU: registration, the C ABI's new symbols, the proto writers, the
planner (scannertools_caffe_plan_net) against the torch restatement's shapes, every refusal with its named cause, and the model
file writers."""
import os
import struct

import numpy as np
import pytest
import torch

import ref_caffe_net as ref
from scannertools_amd import _native, _proto, caffe_net, engine, pose_net


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("caffe_nets"))
    return {"vgg": ref.mini_vgg(d), "inception": ref.mini_inception(d), "dir": d}


def test_registration_and_symbols():
    regs = {(name, dev): (kind, cb) for name, dev, kind, cb in engine.registered_kernels("caffe")}
    imgproc = {(n, d) for n, d, _, _ in engine.registered_kernels()}
    for op in ("Caffe", "Facenet"):
        assert regs[(op, 0)] == (1, True) and regs[(op, 1)] == (1, True)    # DeviceType CPU = 0 and GPU = 1, Batched, .batch()
        assert (op, 0) not in imgproc and (op, 1) not in imgproc
    ci, fi = engine.op_info("Caffe"), engine.op_info("Facenet")
    assert ci["frame_output"] and ci["input_names"] == ["caffe_frame"] and ci["output_names"] == ["caffe_output"]
    assert fi["frame_output"] and fi["input_names"] == ["facenet_input"] and fi["output_names"] == ["facenet_output"]
    L = _native.lib()
    for sym in ("st_inner_product_f32", "st_inner_product_pack_weights", "st_inner_product_packed_bytes", "st_conv2d_general_nhwc_f32",
                "st_pool_nhwc_f32", "st_lrn_nhwc_f32", "st_softmax_nhwc_f32", "st_nhwc_to_planar_f32", "st_copy_channels_nhwc_f32",
                "st_conv_out_size", "st_pool_out_size"):
        assert sym in _native.SIGNATURES and hasattr(L, sym), sym
    assert _native.K_COUNT == 19 and L.st_abi_version() == 1               # no new timing slot, no new ABI version
    assert hasattr(engine._caffe(), "scannertools_caffe_plan_net")


def test_output_size_rules():
    L = _native.lib()
    # Pooling: ceil((H + 2p - k) / s) + 1, less one when p > 0 and the last window would start in the padding
    assert L.st_pool_out_size(5, 2, 2, 1) == 3                             # 4 by the ceiling, the rule takes one off
    for h, k, s, p in ((13, 3, 2, 0), (17, 3, 2, 0), (13, 3, 1, 1), (13, 2, 2, 0), (13, 5, 3, 2), (17, 2, 2, 1), (5, 2, 2, 1), (7, 3, 2, 1)):
        want = torch.nn.functional.max_pool2d(torch.zeros(1, 1, h, h), k, s, p, ceil_mode=True).shape[2]
        assert L.st_pool_out_size(h, k, s, p) == want, (h, k, s, p)
    for h, k, s, p in ((35, 7, 2, 3), (51, 11, 4, 0), (13, 5, 1, 2), (13, 3, 2, 0), (13, 1, 2, 0)):
        assert L.st_conv_out_size(h, k, s, p) == (h + 2 * p - k) // s + 1
    assert L.st_pool_out_size(5, 2, 2, 2) == 0 and L.st_conv_out_size(3, 7, 1, 1) == 0     # what Caffe refuses


def test_proto_writers_match_the_wire_format():
    f = lambda v: struct.pack("<f", v)
    mean = (1.5, -2.0, 0.0)
    packed = b"\x3a\x0c" + f(1.5) + f(-2.0) + f(0.0)
    # the bytes of the descriptor the network-input ops read are what they were
    assert _proto.net_descriptor(300, 200, mean, True) == b"\x28\xac\x02\x30\xc8\x01" + packed + b"\x58\x01"
    assert _proto.net_descriptor() == b"" and _proto.net_descriptor(-1, 0, ()) == b"\x28" + b"\xff" * 9 + b"\x01"
    # NetDescriptor{model_path (1), model_weights_path (2), input_layer_names (3), output_layer_names (4), input_width (5),
    # input_height (6), mean_colors (7), normalize (11), preserve_aspect_ratio (12), transpose (13), pad_mod (14)}
    nd = (b"\x0a\x01m" + b"\x12\x02wt" + b"\x1a\x04data" + b"\x22\x04prob" + b"\x22\x03fc7" + b"\x28\xac\x02\x30\xc8\x01" + packed + b"\x58\x01" +
          b"\x60\x01" + b"\x68\x01" + b"\x70\x08")
    kw = dict(model_path="m", model_weights_path="wt", input_layer_names=["data"], output_layer_names=["prob", "fc7"], input_width=300,
              input_height=200, mean_colors=mean, normalize=True, preserve_aspect_ratio=True, transpose=True, pad_mod=8)
    assert _proto.net_descriptor(**kw) == nd
    # CaffeArgs{net_descriptor (1), batch_size (2)}
    assert _proto.caffe_args(3, **kw) == b"\x0a" + bytes([len(nd)]) + nd + b"\x10\x03"
    assert _proto.caffe_args(**kw) == b"\x0a" + bytes([len(nd)]) + nd and _proto.caffe_args() == b""
    # FacenetArgs{caffe_args (1), templates_path (2), scale (3), threshold (4)}
    nd2 = b"\x0a\x01m" + b"\x12\x02wt" + b"\x1a\x04data" + b"\x22\x04feat" + packed
    ca = b"\x0a" + bytes([len(nd2)]) + nd2 + b"\x10\x05"
    got = _proto.facenet_args(0.5, mean, "t", 0.25, batch_size=5, model_path="m", model_weights_path="wt", input_layer_names=["data"],
                              output_layer_names=["feat"])
    assert got == b"\x0a" + bytes([len(ca)]) + ca + b"\x12\x01t" + b"\x1d" + f(0.5) + b"\x25" + f(0.25)
    assert _proto.facenet_args(0.0, ()) == b""


def test_caffemodel_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    weights = {"conv": [rng.standard_normal((4, 3, 5, 5), dtype=np.float32), rng.standard_normal(4, dtype=np.float32)],
               "fc_nobias": [rng.standard_normal((7, 12), dtype=np.float32)]}
    path = str(tmp_path / "m.caffemodel")
    caffe_net.write_caffemodel(path, weights, {"fc_nobias": "InnerProduct"})
    back = pose_net.read_caffemodel(path)
    assert sorted(back) == sorted(weights)
    for name, blobs in weights.items():
        assert len(back[name]) == len(blobs)
        for a, b in zip(back[name], blobs):
            assert a.shape == b.shape and a.dtype == np.float32
            np.testing.assert_array_equal(a, b)


def test_prototxt_writer_is_read_back(fixtures):
    net = pose_net.parse_prototxt(open(fixtures["inception"][0]).read())
    layers = {l["name"][0]: l for l in net["layer"]}
    assert layers["conv1"]["convolution_param"][0] == {"num_output": ["32"], "kernel_size": ["7"], "pad": ["3"], "stride": ["2"]}
    assert layers["pool1"]["pooling_param"][0]["pool"] == ["MAX"] and layers["pool5"]["pooling_param"][0]["global_pooling"] == ["true"]
    assert layers["inc2/output"]["bottom"] == ["inc2/1x1", "inc2/3x3", "inc2/5x5", "inc2/pool_proj"]
    assert layers["data"]["input_param"][0]["shape"][0]["dim"] == ["1", "3", "35", "43"]


@pytest.mark.parametrize("which,blob", [("vgg", "prob"), ("vgg", "fc7"), ("vgg", "pool2"), ("inception", "prob"), ("inception", "inc1/output"),
                                        ("inception", "inc2/output"), ("inception", "norm1")])
def test_planned_shapes_match_the_reference(fixtures, which, blob):
    prototxt, caffemodel = fixtures[which]
    c, h, w = (3, 32, 32) if which == "vgg" else (3, 35, 43)
    blobs = ref.forward(prototxt, caffemodel, np.zeros((1, c, h, w)))
    want = ref.frame_shaped(blobs[blob]).shape[1:]
    steps, shape = caffe_net.plan_net(prototxt, caffemodel, output_blob=blob)
    assert shape == want and steps > 0
    assert caffe_net.plan_net(prototxt, None, c, h, w, output_blob=blob) == (steps, shape)       # without the weights, explicit size
    if which == "inception":    # another frame size re-plans: everything before the global pooling scales with it
        blobs = ref.forward(prototxt, caffemodel, np.zeros((1, 3, 50, 38)))
        assert caffe_net.plan_net(prototxt, caffemodel, 3, 50, 38, output_blob=blob)[1] == ref.frame_shaped(blobs[blob]).shape[1:]


def test_planner_counts_fused_and_aliased_layers(fixtures):
    # mini-VGG to prob: 3 convolutions, 2 poolings, 2 InnerProducts, 1 Softmax carry launches; ReLU and Dropout do not
    assert caffe_net.plan_net(*fixtures["vgg"], output_blob="prob")[0] == 8
    assert caffe_net.plan_net(*fixtures["vgg"], output_blob="fc7")[0] == 7
    assert caffe_net.plan_net(*fixtures["vgg"], output_blob="conv1_1") == (1, (16, 32, 32))


def test_pooling_less_one_rule_in_the_planner(tmp_path):
    net = caffe_net.NetBuilder(4, 5, 5, seed=1)
    net.pool("pool", "data", "MAX", 2, 2, 1)
    prototxt, caffemodel = net.write(str(tmp_path))
    blobs = ref.forward(prototxt, caffemodel, np.zeros((1, 4, 5, 5)))
    assert tuple(blobs["pool"].shape[1:]) == (4, 3, 3)
    assert caffe_net.plan_net(prototxt, output_blob="pool") == (1, (4, 3, 3))


def _refusal(tmp_path, edit, output_blob="prob", weights=True, size=(0, 0, 0)):
    net = caffe_net.NetBuilder(3, 16, 16, seed=2, name="r")
    top = net.conv("conv1", "data", 8, 3, pad=1)
    top = net.lrn("norm1", top)
    top = net.fc("fc", net.pool("pool1", top, "MAX", 2, 2), 5, relu=False)
    net.softmax("prob", top)
    edit(net)
    prototxt, caffemodel = net.write(str(tmp_path))
    with pytest.raises(ValueError) as e:
        caffe_net.plan_net(prototxt, caffemodel if weights else None, *size, output_blob=output_blob)
    return str(e.value)


def _layer(net, name):
    return next(l for l in net.layers if l["name"] == name)


def test_planner_refusals_name_the_cause(tmp_path):
    def eltwise(net):
        net.layers.insert(3, {"name": "sum1", "type": "Eltwise", "bottom": ["conv1", "conv1"], "top": ["conv1"]})
    msg = _refusal(tmp_path, eltwise)
    assert "sum1" in msg and "Eltwise" in msg and "not implemented" in msg
    for typ in ("BatchNorm", "Scale", "Deconvolution", "Python"):
        def other(net, typ=typ):
            net.layers.insert(3, {"name": "odd", "type": typ, "bottom": ["conv1"], "top": ["conv1"]})
        msg = _refusal(tmp_path, other)
        assert "odd" in msg and typ in msg
    # a layer of another type that the output does not depend on is not in the way
    net = caffe_net.NetBuilder(3, 8, 8, seed=1)
    net.conv("conv1", "data", 4, 3, pad=1)
    net.layers.append({"name": "side", "type": "Eltwise", "bottom": ["conv1", "conv1"], "top": ["side"]})
    assert caffe_net.plan_net(*net.write(str(tmp_path)), output_blob="conv1") == (1, (4, 8, 8))
    # weights absent / of the wrong element count
    msg = _refusal(tmp_path, lambda net: net.weights.pop("conv1"))
    assert "conv1" in msg and "no blobs" in msg
    msg = _refusal(tmp_path, lambda net: net.weights.__setitem__("conv1", [np.zeros((8, 3, 3, 2), np.float32), np.zeros(8, np.float32)]))
    assert "conv1" in msg and "144" in msg and "216" in msg
    msg = _refusal(tmp_path, lambda net: net.weights.__setitem__("fc", [net.weights["fc"][0], np.zeros(4, np.float32)]))
    assert "fc" in msg and "bias" in msg
    msg = _refusal(tmp_path, lambda net: net.weights.__setitem__("fc", [net.weights["fc"][0]]))
    assert "fc" in msg and "1 blobs" in msg
    # an InnerProduct whose input length differs from its weights: what a frame of another size runs into
    msg = _refusal(tmp_path, lambda net: None, size=(3, 20, 16))
    assert "fc" in msg and "InnerProduct" in msg and "8 x 10 x 8 = 640" in msg and "512" in msg
    msg = _refusal(tmp_path, lambda net: None, size=(4, 16, 16))
    assert "4 channels" in msg and "3" in msg
    # blob names
    assert "produces no blob named nope" in _refusal(tmp_path, lambda net: None, output_blob="nope")
    # parameters outside the set
    msg = _refusal(tmp_path, lambda net: _layer(net, "norm1")["lrn_param"].__setitem__("norm_region", "@WITHIN_CHANNEL"))
    assert "norm1" in msg and "WITHIN_CHANNEL" in msg
    msg = _refusal(tmp_path, lambda net: _layer(net, "conv1")["convolution_param"].__setitem__("dilation", 2))
    assert "conv1" in msg and "dilation" in msg
    msg = _refusal(tmp_path, lambda net: _layer(net, "relu_conv1").__setitem__("relu_param", {"negative_slope": 0.1}))
    assert "relu_conv1" in msg and "negative_slope" in msg
    msg = _refusal(tmp_path, lambda net: _layer(net, "pool1")["pooling_param"].__setitem__("pool", "@STOCHASTIC"))
    assert "pool1" in msg and "STOCHASTIC" in msg
    msg = _refusal(tmp_path, lambda net: _layer(net, "norm1")["lrn_param"].__setitem__("local_size", 4))
    assert "norm1" in msg and "odd" in msg


def test_malformed_descriptions_are_value_errors(tmp_path):
    # a cycle: conv1 reads the blob a later layer produces
    msg = _refusal(tmp_path, lambda net: _layer(net, "conv1").__setitem__("bottom", ["pool1"]))
    assert "malformed" in msg and "conv1" in msg and "pool1" in msg
    # layers without blobs
    msg = _refusal(tmp_path, lambda net: _layer(net, "pool1").pop("top"))
    assert "malformed" in msg and "pool1" in msg and "no top blob" in msg
    msg = _refusal(tmp_path, lambda net: _layer(net, "fc").pop("bottom"))
    assert "malformed" in msg and "fc" in msg and "no bottom blob" in msg
    # no input blob, an input without a shape
    msg = _refusal(tmp_path, lambda net: net.layers.pop(0))
    assert "malformed" in msg
    msg = _refusal(tmp_path, lambda net: net.layers[0].pop("input_param"), weights=False)
    assert "malformed" in msg and "no shape" in msg
    # text that is no prototxt, files that are not there
    bad = tmp_path / "bad.prototxt"
    bad.write_text("layer { name: \"x\" ")
    with pytest.raises(ValueError, match="missing '}'"):
        caffe_net.plan_net(str(bad))
    with pytest.raises(ValueError, match="cannot read the model description"):
        caffe_net.plan_net(str(tmp_path / "absent.prototxt"))
    net = caffe_net.NetBuilder(3, 8, 8)
    net.conv("conv1", "data", 4, 3, pad=1)
    prototxt, _ = net.write(str(tmp_path))
    with pytest.raises(ValueError, match="cannot read the weights file"):
        caffe_net.plan_net(prototxt, str(tmp_path / "absent.caffemodel"), output_blob="conv1")
    with pytest.raises(ValueError, match="cannot read the weights file"):
        caffe_net.plan_net(prototxt, str(tmp_path), output_blob="conv1")                    # a directory


def test_legacy_header_and_v1_type_names(tmp_path):
    text = ('name: "old"\ninput: "data"\ninput_dim: 1\ninput_dim: 3\ninput_dim: 9\ninput_dim: 11\n'
            'layers { name: "c" type: CONVOLUTION bottom: "data" top: "c" convolution_param { num_output: 6 kernel_size: 3 stride: 2 } }\n'
            'layers { name: "r" type: RELU bottom: "c" top: "c" }\n'
            'layers { name: "ip" type: INNER_PRODUCT bottom: "c" top: "ip" inner_product_param { num_output: 5 } }\n'
            'layers { name: "p" type: SOFTMAX bottom: "ip" top: "p" }\n')
    path = tmp_path / "old.prototxt"
    path.write_text(text)
    assert caffe_net.plan_net(str(path), output_blob="p") == (3, (5, 1, 1))
    assert caffe_net.plan_net(str(path), output_blob="c") == (1, (6, 4, 5))
    path.write_text(text.replace("input_dim: 1\ninput_dim: 3\ninput_dim: 9\ninput_dim: 11\n", "input_shape { dim: 1 dim: 3 dim: 9 dim: 11 }\n"))
    assert caffe_net.plan_net(str(path), output_blob="c") == (1, (6, 4, 5))


def _run_error(make_op):
    from scannertools_amd.engine import Client, NamedStream, NamedVideoStream, PerfParams
    sc = Client()
    sc.ingest_frames("v", np.zeros((2, 3, 8, 8), np.float32))
    frame = sc.io.Input([NamedVideoStream(sc, "v")])
    with pytest.raises(RuntimeError) as e:
        sc.run(sc.io.Output(make_op(sc, frame), [NamedStream(sc, "o")]), PerfParams.estimate())
    return str(e.value)


def test_validate_refusals_name_the_cause(fixtures, tmp_path):
    """Everything validate() refuses is decided before the context is opened, so it is reached with or without a GPU."""
    from scannertools_amd.engine import _CppOpNode
    prototxt, caffemodel = fixtures["vgg"]
    absent = os.path.join(fixtures["dir"], "absent")

    def caffe(**kw):
        args = dict(model_path=prototxt, model_weights_path=caffemodel, input_layer_names=["data"], output_layer_names=["prob"])
        args.update(kw)
        return lambda sc, fr: sc.ops.Caffe(caffe_frame=fr, **args)

    def facenet(**kw):
        args = dict(model_path=prototxt, model_weights_path=caffemodel, input_layer_names=["data"], output_layer_names=["prob"])
        args.update(kw)
        return lambda sc, fr: sc.ops.Facenet(facenet_input=fr, **args)

    for make in (caffe, facenet):
        assert "Model path %s does not exist" % absent in _run_error(make(model_path=absent))
        assert "Model weights path %s does not exist" % absent in _run_error(make(model_weights_path=absent))
        assert "Model weights path %s does not exist" % fixtures["dir"] in _run_error(make(model_weights_path=fixtures["dir"]))
        assert "# output columns in net descriptor (2) does not match" in _run_error(make(output_layer_names=["prob", "fc7"]))
        assert "# output columns in net descriptor (0) does not match" in _run_error(make(output_layer_names=[]))
        assert "input_layer_names is empty" in _run_error(make(input_layer_names=[]))
        assert "no input blob named image" in _run_error(make(input_layer_names=["image"]))
        assert "produces no blob named fc9" in _run_error(make(output_layer_names=["fc9"]))
    # a description with a layer outside the set, weights that do not fit it
    net = caffe_net.NetBuilder(3, 8, 8, seed=1)
    net.conv("conv1", "data", 4, 3, pad=1)
    net.layers.append({"name": "sum", "type": "Eltwise", "bottom": ["conv1", "conv1"], "top": ["sum"]})
    p2, m2 = net.write(str(tmp_path))
    msg = _run_error(caffe(model_path=p2, model_weights_path=m2, output_layer_names=["sum"]))
    assert "sum" in msg and "Eltwise" in msg
    msg = _run_error(caffe(model_weights_path=m2))
    assert "conv1_1" in msg and "no blobs" in msg
    # arguments: unparsable bytes, uses_python (NetDescriptor field 15), a negative batch size
    assert "Could not parse CaffeArgs" in _run_error(lambda sc, fr: _CppOpNode(sc, "Caffe", fr, None, None, None, b"\x0a\x7f\x01"))
    assert "Could not parse FacenetArgs" in _run_error(lambda sc, fr: _CppOpNode(sc, "Facenet", fr, None, None, None, b"\x0a\x7f\x01"))
    assert "Could not parse FacenetArgs" in _run_error(lambda sc, fr: _CppOpNode(sc, "Facenet", fr, None, None, None, b"\x0a\x03\x0a\x05\x01"))
    nd = _proto.net_descriptor(model_path=prototxt, model_weights_path=caffemodel, input_layer_names=["data"], output_layer_names=["prob"])
    py = _proto.message(1, nd + b"\x78\x01")
    assert "uses_python" in _run_error(lambda sc, fr: _CppOpNode(sc, "Caffe", fr, None, None, None, py))
    assert "batch_size must not be negative" in _run_error(caffe(batch_size=-2))
