"""The independent definition of a Caffe forward pass for the Caffe / Facenet op tests: the deploy prototxt is parsed with
caffe_files.parse_prototxt, the weights read with caffe_files.read_caffemodel, and every layer evaluated with torch ON THE CPU IN
FLOAT64 by the rules of DESIGN.md section 4.14 ([EXT] Caffe's public sources).  It shares nothing with the C++ planner
(scanner_kernels/caffe_net.h).  Also the two fixture networks of the tests."""
import numpy as np
import torch
import torch.nn.functional as F

from scannertools_amd import caffe_files, caffe_net


def _p(layer, key):
    return layer.get(key, [{}])[0]


def _i(msg, key, default):
    return int(msg.get(key, [default])[0])


def forward(prototxt, caffemodel, x, input_blob="data"):
    """x: (n, C, H, W) array.  Returns {blob name: float64 tensor} after the whole description ran in file order (an in-place layer
    overwrites its blob, as in Caffe)."""
    net = caffe_files.parse_prototxt(open(prototxt).read())
    weights = caffe_files.read_caffemodel(caffemodel)
    blobs = {input_blob: torch.as_tensor(np.asarray(x), dtype=torch.float64)}
    for layer in net.get("layer", []) + net.get("layers", []):
        typ = str(layer["type"][0]).replace("_", "").lower()
        name = layer["name"][0]
        if typ == "input":
            continue
        bottoms = [blobs[b] for b in layer.get("bottom", [])]
        b = bottoms[0]
        wts = [torch.as_tensor(np.asarray(a), dtype=torch.float64) for a in weights.get(name, [])]
        if typ == "convolution":
            p = _p(layer, "convolution_param")
            bias = str(p.get("bias_term", ["true"])[0]) == "true"
            w = wts[0].reshape(_i(p, "num_output", 0), -1, _i(p, "kernel_size", 1), _i(p, "kernel_size", 1))
            y = F.conv2d(b, w, wts[1] if bias else None, stride=_i(p, "stride", 1), padding=_i(p, "pad", 0), groups=_i(p, "group", 1))
        elif typ == "relu":
            y = torch.clamp(b, min=0)
        elif typ == "pooling":
            p = _p(layer, "pooling_param")
            ave = str(p.get("pool", ["MAX"])[0]) == "AVE"
            if str(p.get("global_pooling", ["false"])[0]) == "true":
                y = b.mean(dim=(2, 3), keepdim=True) if ave else b.amax(dim=(2, 3), keepdim=True)
            else:
                k, s, pad = _i(p, "kernel_size", 0), _i(p, "stride", 1), _i(p, "pad", 0)
                y = (F.avg_pool2d(b, k, s, pad, ceil_mode=True, count_include_pad=True) if ave else F.max_pool2d(b, k, s, pad, ceil_mode=True))
        elif typ == "lrn":
            p = _p(layer, "lrn_param")
            y = F.local_response_norm(b, _i(p, "local_size", 5), float(p.get("alpha", [1.0])[0]), float(p.get("beta", [0.75])[0]),
                                      float(p.get("k", [1.0])[0]))
        elif typ == "concat":
            y = torch.cat(bottoms, dim=1)
        elif typ == "innerproduct":
            p = _p(layer, "inner_product_param")
            bias = str(p.get("bias_term", ["true"])[0]) == "true"
            y = F.linear(b.reshape(b.shape[0], -1), wts[0].reshape(_i(p, "num_output", 0), -1), wts[1] if bias else None)
        elif typ in ("dropout", "split"):
            y = b
        elif typ == "softmax":
            y = torch.softmax(b, dim=1)
        else:
            raise ValueError("reference: layer type %r" % layer["type"][0])
        for t in layer["top"]:
            blobs[t] = y
    return blobs


def frame_shaped(t):
    """A blob's items as the op's output frames: (n, C, H or 1, W or 1) float64 numpy."""
    a = t.numpy()
    return a.reshape(a.shape[0], a.shape[1], a.shape[2] if a.ndim > 2 else 1, a.shape[3] if a.ndim > 3 else 1)


# ---- the fixture networks -------------------------------------------------------------------------------------------------
def mini_vgg(directory, seed=11):
    """3 x 32 x 32 -> conv3x3(16) conv3x3(24) pool conv3x3(64) pool fc(96) drop fc(10) softmax; blobs `fc7` and `prob`."""
    net = caffe_net.NetBuilder(3, 32, 32, seed, name="mini_vgg")
    top = net.conv("conv1_1", "data", 16, 3, pad=1)
    top = net.pool("pool1", net.conv("conv1_2", top, 24, 3, pad=1), "MAX", 2, 2)
    top = net.pool("pool2", net.conv("conv2_1", top, 64, 3, pad=1), "MAX", 2, 2)
    top = net.dropout("drop6", net.fc("fc6", top, 96))
    net.softmax("prob", net.fc("fc7", top, 10, relu=False))
    return net.write(directory)


def mini_inception(directory, seed=12):
    """3 x 35 x 43 -> conv7x7/2 MAX3/2 LRN conv1x1 conv3x3 LRN MAX3/2, two inception modules (Concat offsets 0/16/48/64, then
    0/20/56/68), global AVE, drop, fc(12), softmax; blobs `inc1/output`, `inc2/output`, `prob`."""
    net = caffe_net.NetBuilder(3, 35, 43, seed, name="mini_inception")
    top = net.conv("conv1", "data", 32, 7, stride=2, pad=3)
    top = net.lrn("norm1", net.pool("pool1", top, "MAX", 3, 2), 5, 1e-2)
    top = net.conv("conv2", net.conv("conv2_reduce", top, 32, 1), 48, 3, pad=1)
    top = net.pool("pool2", net.lrn("norm2", top, 5, 1e-2), "MAX", 3, 2)
    top = net.inception("inc1", top, 16, 24, 32, 8, 16, 16)
    top = net.inception("inc2", top, 20, 28, 36, 8, 12, 12)
    top = net.dropout("drop", net.pool("pool5", top, "AVE", global_pooling=True))
    net.softmax("prob", net.fc("classifier", top, 12, relu=False))
    return net.write(directory)
