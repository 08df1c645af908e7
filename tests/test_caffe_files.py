"""The shared model-file code (scannertools_amd/caffe_files.py, scanner_kernels/caffe_files.h, caffe_args.h) without a GPU: the
writers' files are what they were byte for byte, both C++ entry points read a caffemodel through one reader, and CPM2 decides
its argument refusals through the NetDescriptor reader every caffe op uses."""
import hashlib
import os

import numpy as np
import pytest

from scannertools_amd import _proto, caffe_files, caffe_net, pose_net


def _digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for chunk in iter(lambda: fh.read(1 << 24), b""):
            h.update(chunk)
    return h.hexdigest()[:16], os.path.getsize(path)


def _renamed():
    return ["L%02d_%s" % (i, n) for i, n in enumerate(pose_net.caffe_layer_names())]


def _four_layer_net():
    """The net of test_caffe_net._refusal, unedited."""
    net = caffe_net.NetBuilder(3, 16, 16, seed=2, name="r")
    top = net.conv("conv1", "data", 8, 3, pad=1)
    top = net.lrn("norm1", top)
    top = net.fc("fc", net.pool("pool1", top, "MAX", 2, 2), 5, relu=False)
    net.softmax("prob", top)
    return net


def test_prototxt_writers_are_byte_stable(tmp_path):
    """sha256[:16] and size of the written descriptions, taken before the writers moved."""
    p = str(tmp_path / "pose.prototxt")
    pose_net.write_prototxt(p)
    assert _digest(p) == ("119fabec47a6e14c", 24140)
    pose_net.write_prototxt(p, interleaved=True)
    assert _digest(p) == ("5fa550297ee1fe79", 24140)
    pose_net.write_prototxt(p, names=_renamed(), interleaved=True)
    assert _digest(p) == ("147c79caa9456e13", 26220)
    prototxt, _ = _four_layer_net().write(str(tmp_path))
    assert _digest(prototxt) == ("8fd10756b8738aee", 883)


def test_caffemodel_writers_are_byte_stable(tmp_path):
    """The same for the caffemodels: the pose network's with zero weights (plain; renamed, reversed, with blob-less entries in
    between), and the four-layer net's with every blob replaced by (arange(size) % 251) in its shape -- seeded random weights
    are not pinned, numpy's stream may differ between versions.  All digests were computed with the writers as they were
    before caffe_files.write_caffemodel existed."""
    p = str(tmp_path / "pose.caffemodel")
    zeros = {name: (np.zeros((co, ci, k, k), np.float32), np.zeros(co, np.float32)) for name, ci, co, k, _ in pose_net.all_layers()}
    pose_net.write_caffemodel(p, zeros)
    assert _digest(p) == ("596f328a444f33af", 209251849)
    pose_net.write_caffemodel(p, zeros, names=_renamed(), order=list(range(92))[::-1], extra_layers=["relu_%d" % i for i in range(40)])
    assert _digest(p) == ("ea052c38d213cbcc", 209252927)
    os.remove(p)
    net = _four_layer_net()
    for name, blobs in net.weights.items():
        net.weights[name] = [(np.arange(b.size) % 251).astype(np.float32).reshape(b.shape) for b in blobs]
    _, caffemodel = net.write(str(tmp_path))
    assert _digest(caffemodel) == ("1e15f8465d431136", 11252)
    back = caffe_files.read_caffemodel(caffemodel)
    assert list(back) == ["conv1", "fc"] and [b.shape for b in back["conv1"] + back["fc"]] == [(8, 3, 3, 3), (8,), (5, 512), (5,)]


def test_both_op_library_entry_points_read_through_one_reader(tmp_path):
    """One caffemodel with a two-blob layer, a one-blob layer (an InnerProduct without bias) and a blob-less ReLU entry: the
    Caffe planner takes it for the matching description, the pose check refuses it by the first layer it misses; the hostile
    length field of test_pose.test_op_library_checks_a_model_file is refused by both with the same words."""
    net = caffe_net.NetBuilder(3, 8, 8, seed=5, name="two")
    net.fc("fc", net.conv("conv1", "data", 4, 3, pad=1), 5, relu=False, bias=False)
    prototxt, _ = net.write(str(tmp_path))
    model = str(tmp_path / "three.caffemodel")
    caffe_files.write_caffemodel(model, [("conv1", "Convolution", net.weights["conv1"]), ("relu_conv1", "ReLU", []),
                                         ("fc", "InnerProduct", net.weights["fc"])])
    assert [len(b) for b in caffe_files.read_caffemodel(model).values()] == [2, 1]
    assert caffe_net.plan_net(prototxt, model, output_blob="fc") == (2, (5, 1, 1))
    with pytest.raises(ValueError, match="no weights for layer conv1_1"):
        pose_net.check_caffemodel(model)
    hostile = tmp_path / "hostile.caffemodel"
    hostile.write_bytes(b"\xa2\x06" + b"\xff" * 9 + b"\x01\x00")  # length-delimited field with a length of 2**64 - 1
    with pytest.raises(ValueError, match="NetParameter"):
        pose_net.check_caffemodel(hostile)
    with pytest.raises(ValueError, match="NetParameter"):
        caffe_net.plan_net(prototxt, str(hostile), output_blob="fc")


def test_cpm2_argument_refusals_name_the_cause(tmp_path):
    """CPM2 reads CPM2Args{caffe_args = 1} through the reader of the other caffe ops; what it refuses about them is decided
    before the context is opened, so it is reached with or without a GPU."""
    from scannertools_amd.engine import Client, NamedStream, NamedVideoStream, PerfParams, _CppOpColumn, _CppOpNode

    def run_error(args):
        sc = Client()
        sc.ingest_frames("v", np.zeros((2, 3, 8, 8), np.float32))
        frame = sc.io.Input([NamedVideoStream(sc, "v")])
        with pytest.raises(RuntimeError) as e:
            sc.run(sc.io.Output(_CppOpColumn(_CppOpNode(sc, "CPM2", frame, None, None, None, args), 0), [NamedStream(sc, "o")]), PerfParams.estimate())
        return str(e.value)

    assert "Could not parse CPM2Args" in run_error(b"\x0a\x7f\x01")
    assert "model_weights_path is empty" in run_error(b"")
    # past both refusals: whatever stops the kernel then (no device, or the absent file) is neither of them
    msg = run_error(_proto.message(1, _proto.caffe_args(model_weights_path=str(tmp_path / "absent.caffemodel"))))
    assert "Could not parse" not in msg and "is empty" not in msg
