"""Model files for the Caffe and Facenet ops (scanner_kernels/caffe_net.h), written without Caffe: a deploy prototxt and a
caffemodel from random weights, for tests and the benchmark (no trained model can be fetched), and the op library's planner
(scannertools_caffe_plan_net: shapes and refusals without a GPU).

    net = NetBuilder(3, 32, 32, seed=1)
    top = net.conv("conv1", "data", 16, 3, pad=1)
    top = net.pool("pool1", top, "MAX", 2, 2)
    top = net.fc("fc", top, 10, relu=False)
    top = net.softmax("prob", top)
    prototxt, caffemodel = net.write(directory)
    plan_net(prototxt, caffemodel, output_blob="prob")      # -> (launches, (10, 1, 1))
"""
import ctypes
import os

import numpy as np

from . import caffe_files


def write_caffemodel(path, weights, types=None):
    """Writes {layer name: [blob, ...]} (float32 arrays of the blobs' Caffe shapes) as a serialised NetParameter
    (caffe_files.write_caffemodel).  types: {layer name: type string}, "Convolution" where absent.
    caffe_files.read_caffemodel reads it back."""
    caffe_files.write_caffemodel(path, [(name, (types or {}).get(name, "Convolution"), blobs) for name, blobs in weights.items()])


def _text(fields, indent):
    out = []
    pad = "  " * indent
    for key, value in fields:
        for v in (value if isinstance(value, list) else [value]):
            if isinstance(v, (dict, tuple)) and not isinstance(v, str):
                items = list(v.items()) if isinstance(v, dict) else list(v)
                out.append("%s%s {" % (pad, key))
                out += _text(items, indent + 1)
                out.append("%s}" % pad)
            elif isinstance(v, bool):
                out.append("%s%s: %s" % (pad, key, "true" if v else "false"))
            elif isinstance(v, str) and not v.startswith("@"):
                out.append('%s%s: "%s"' % (pad, key, v))
            else:
                out.append("%s%s: %s" % (pad, key, str(v)[1:] if isinstance(v, str) else repr(v)))
    return out


def write_prototxt(path, layers, name="net"):
    """Writes a deploy description: layers is a list of dicts {name, type, bottom: [..], top: [..], <x>_param: {...}} in
    execution order; values that are dicts become messages, lists repeated fields, strings quoted values ("@MAX": the
    enum value MAX, unquoted)."""
    lines = ['name: "%s"' % name]
    for layer in layers:
        lines.append("layer {")
        lines += _text(list(layer.items()), 1)
        lines.append("}")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def _conv_out(size, k, stride, pad):
    return (size + 2 * pad - k) // stride + 1


def _pool_out(size, k, stride, pad):
    out = -(-(size + 2 * pad - k) // stride) + 1
    if pad > 0 and (out - 1) * stride >= size + pad:
        out -= 1
    return out


class NetBuilder:
    """A network of the supported layer set, layer by layer, with seeded He-initialised weights (normal, variance 2 / fan-in;
    biases normal with deviation 0.1).  Every method returns the name of its top blob."""

    def __init__(self, c, h, w, seed=0, input_blob="data", name="net"):
        self.name, self.input_blob = name, input_blob
        self.rng = np.random.default_rng(seed)
        self.layers = [{"name": input_blob, "type": "Input", "top": [input_blob], "input_param": {"shape": {"dim": [1, c, h, w]}}}]
        self.shapes = {input_blob: (c, h, w)}
        self.weights, self.types = {}, {}

    def _relu(self, name, top, relu):
        if relu:
            self.layers.append({"name": "relu_" + name, "type": "ReLU", "bottom": [top], "top": [top]})
        return top

    def conv(self, name, bottom, cout, k, stride=1, pad=0, group=1, relu=True, bias=True, top=None):
        c, h, w = self.shapes[bottom]
        top = top or name
        param = {"num_output": cout, "kernel_size": k}
        if pad:
            param["pad"] = pad
        if stride != 1:
            param["stride"] = stride
        if group != 1:
            param["group"] = group
        if not bias:
            param["bias_term"] = False
        self.layers.append({"name": name, "type": "Convolution", "bottom": [bottom], "top": [top], "convolution_param": param})
        fan = (c // group) * k * k
        blobs = [(self.rng.standard_normal((cout, c // group, k, k), dtype=np.float32) * np.float32(np.sqrt(2.0 / fan)))]
        if bias:
            blobs.append(self.rng.standard_normal(cout, dtype=np.float32) * np.float32(0.1))
        self.weights[name], self.types[name] = blobs, "Convolution"
        self.shapes[top] = (cout, _conv_out(h, k, stride, pad), _conv_out(w, k, stride, pad))
        return self._relu(name, top, relu)

    def fc(self, name, bottom, nout, relu=True, bias=True, top=None):
        c, h, w = self.shapes[bottom]
        top = top or name
        param = {"num_output": nout}
        if not bias:
            param["bias_term"] = False
        self.layers.append({"name": name, "type": "InnerProduct", "bottom": [bottom], "top": [top], "inner_product_param": param})
        fan = c * h * w
        blobs = [self.rng.standard_normal((nout, fan), dtype=np.float32) * np.float32(np.sqrt(2.0 / fan))]
        if bias:
            blobs.append(self.rng.standard_normal(nout, dtype=np.float32) * np.float32(0.1))
        self.weights[name], self.types[name] = blobs, "InnerProduct"
        self.shapes[top] = (nout, 1, 1)
        return self._relu(name, top, relu)

    def pool(self, name, bottom, method, k=0, stride=1, pad=0, global_pooling=False, top=None):
        c, h, w = self.shapes[bottom]
        top = top or name
        param = {"pool": "@" + method}
        if global_pooling:
            param["global_pooling"] = True
        else:
            param.update({"kernel_size": k, "stride": stride})
            if pad:
                param["pad"] = pad
        self.layers.append({"name": name, "type": "Pooling", "bottom": [bottom], "top": [top], "pooling_param": param})
        self.shapes[top] = (c, 1, 1) if global_pooling else (c, _pool_out(h, k, stride, pad), _pool_out(w, k, stride, pad))
        return top

    def lrn(self, name, bottom, local_size=5, alpha=1e-4, beta=0.75, k=1.0, top=None):
        top = top or name
        self.layers.append({"name": name, "type": "LRN", "bottom": [bottom], "top": [top],
                            "lrn_param": {"local_size": local_size, "alpha": alpha, "beta": beta, "k": k}})
        self.shapes[top] = self.shapes[bottom]
        return top

    def concat(self, name, bottoms, top=None):
        top = top or name
        self.layers.append({"name": name, "type": "Concat", "bottom": list(bottoms), "top": [top]})
        self.shapes[top] = (sum(self.shapes[b][0] for b in bottoms),) + self.shapes[bottoms[0]][1:]
        return top

    def dropout(self, name, bottom):
        self.layers.append({"name": name, "type": "Dropout", "bottom": [bottom], "top": [bottom], "dropout_param": {"dropout_ratio": 0.5}})
        return bottom

    def softmax(self, name, bottom, top=None):
        top = top or name
        self.layers.append({"name": name, "type": "Softmax", "bottom": [bottom], "top": [top]})
        self.shapes[top] = self.shapes[bottom]
        return top

    def inception(self, name, bottom, c1, c3r, c3, c5r, c5, cp):
        """GoogLeNet's module: 1x1 | 1x1 -> 3x3 | 1x1 -> 5x5 | MAX 3x3 / 1 -> 1x1, concatenated in that order."""
        b1 = self.conv(name + "/1x1", bottom, c1, 1)
        b3 = self.conv(name + "/3x3", self.conv(name + "/3x3_reduce", bottom, c3r, 1), c3, 3, pad=1)
        b5 = self.conv(name + "/5x5", self.conv(name + "/5x5_reduce", bottom, c5r, 1), c5, 5, pad=2)
        bp = self.conv(name + "/pool_proj", self.pool(name + "/pool", bottom, "MAX", 3, 1, 1), cp, 1)
        return self.concat(name + "/output", [b1, b3, b5, bp])

    def write(self, directory, stem=None):
        stem = stem or self.name
        prototxt, caffemodel = os.path.join(directory, stem + ".prototxt"), os.path.join(directory, stem + ".caffemodel")
        write_prototxt(prototxt, self.layers, self.name)
        write_caffemodel(caffemodel, self.weights, self.types)
        return prototxt, caffemodel


def vgg16(seed=0, size=224, classes=1000):
    """VGG-16's topology ([EXT] the published deploy description) with random weights."""
    net = NetBuilder(3, size, size, seed, name="vgg16")
    top = "data"
    for block, (reps, cout) in enumerate(((2, 64), (2, 128), (3, 256), (3, 512), (3, 512)), 1):
        for i in range(1, reps + 1):
            top = net.conv("conv%d_%d" % (block, i), top, cout, 3, pad=1)
        top = net.pool("pool%d" % block, top, "MAX", 2, 2)
    top = net.dropout("drop6", net.fc("fc6", top, 4096))
    top = net.dropout("drop7", net.fc("fc7", top, 4096))
    return net, net.softmax("prob", net.fc("fc8", top, classes, relu=False))


def googlenet(seed=0, size=224, classes=1000):
    """bvlc_googlenet's deploy topology ([EXT]) with random weights."""
    net = NetBuilder(3, size, size, seed, name="googlenet")
    top = net.conv("conv1/7x7_s2", "data", 64, 7, stride=2, pad=3)
    top = net.lrn("pool1/norm1", net.pool("pool1/3x3_s2", top, "MAX", 3, 2))
    top = net.conv("conv2/3x3", net.conv("conv2/3x3_reduce", top, 64, 1), 192, 3, pad=1)
    top = net.pool("pool2/3x3_s2", net.lrn("conv2/norm2", top), "MAX", 3, 2)
    top = net.inception("inception_3a", top, 64, 96, 128, 16, 32, 32)
    top = net.inception("inception_3b", top, 128, 128, 192, 32, 96, 64)
    top = net.pool("pool3/3x3_s2", top, "MAX", 3, 2)
    top = net.inception("inception_4a", top, 192, 96, 208, 16, 48, 64)
    top = net.inception("inception_4b", top, 160, 112, 224, 24, 64, 64)
    top = net.inception("inception_4c", top, 128, 128, 256, 24, 64, 64)
    top = net.inception("inception_4d", top, 112, 144, 288, 32, 64, 64)
    top = net.inception("inception_4e", top, 256, 160, 320, 32, 128, 128)
    top = net.pool("pool4/3x3_s2", top, "MAX", 3, 2)
    top = net.inception("inception_5a", top, 256, 160, 320, 32, 128, 128)
    top = net.inception("inception_5b", top, 384, 192, 384, 48, 128, 128)
    top = net.dropout("pool5/drop_7x7_s1", net.pool("pool5/7x7_s1", top, "AVE", 7, 1))
    return net, net.softmax("prob", net.fc("loss3/classifier", top, classes, relu=False))


def plan_net(prototxt, caffemodel=None, c=0, h=0, w=0, output_blob="prob"):
    """(number of launch-carrying layers, (C, H, W) of the output blob) for an input of (c, h, w) -- 0: the description's own --
    through the op library's planner (scannertools_caffe_plan_net; no GPU needed).  With `caffemodel` the weights of every
    layer on the path are checked too.  Raises ValueError with the planner's message."""
    from . import engine
    L = engine._caffe()
    L.scannertools_caffe_plan_net.restype = ctypes.c_int
    L.scannertools_caffe_plan_net.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                                              ctypes.POINTER(ctypes.c_int), ctypes.c_char_p, ctypes.c_size_t]
    err = ctypes.create_string_buffer(1024)
    shape = (ctypes.c_int * 3)()
    n = L.scannertools_caffe_plan_net(str(prototxt).encode(), str(caffemodel).encode() if caffemodel else None, int(c), int(h), int(w),
                                      str(output_blob).encode(), shape, err, 1024)
    if n < 0:
        raise ValueError(err.value.decode())
    return n, tuple(shape)
