"""Caffe's two model file formats, read and written without Caffe: the deploy description (protobuf text format) and the
caffemodel (a serialised NetParameter, [EXT] caffe.proto).  Shared by every network of this package (pose_net.py: the pose
network; caffe_net.py: any network of the Caffe / Facenet ops' layer set) and by the tests' float64 restatement; the C++
twin is scanner_kernels/caffe_files.h."""
import re

import numpy as np

from . import _proto


def parse_prototxt(text):
    """Protobuf text format -> nested {field: [values]} (every field a list: repeated fields are the rule in a NetParameter)."""
    tok = re.findall(r'#[^\n]*|"(?:[^"\\]|\\.)*"|\'(?:[^\'\\]|\\.)*\'|[{}:]|[^\s{}:#"\']+', text)
    tok = [t for t in tok if not t.startswith("#")]
    pos = 0

    def message(closing):
        nonlocal pos
        out = {}
        while pos < len(tok):
            t = tok[pos]
            if t == "}":
                if not closing:
                    raise ValueError("prototxt: unbalanced '}'")
                pos += 1
                return out
            name = t
            pos += 1
            if pos < len(tok) and tok[pos] == ":":
                pos += 1
            if pos >= len(tok):
                raise ValueError("prototxt: field %r has no value" % name)
            if tok[pos] == "{":
                pos += 1
                val = message(True)
            else:
                val = tok[pos]
                pos += 1
                if val[0] in "\"'":
                    val = val[1:-1]
            out.setdefault(name, []).append(val)
        if closing:
            raise ValueError("prototxt: missing '}'")
        return out

    return message(False)


def _varints(mv):
    vals, v, shift = [], 0, 0
    for b in bytes(mv):
        v |= (b & 0x7F) << shift
        shift += 7
        if not b & 0x80:
            vals.append(v)
            v, shift = 0, 0
    return vals


def _read_blob(mv):
    data, dims, legacy = None, [], {}
    for num, wt, v in _proto.fields(mv):
        if num == 5 and wt == 2:
            data = np.frombuffer(v, dtype="<f4")
        elif num == 5 and wt == 5:   # unpacked repeated float
            data = np.append(data if data is not None else np.zeros(0, "<f4"), np.frombuffer(v.to_bytes(4, "little"), "<f4"))
        elif num == 7 and wt == 2:
            for n2, w2, v2 in _proto.fields(v):
                if n2 == 1 and w2 == 2:   # packed int64 dims
                    dims += _varints(v2)
                elif n2 == 1 and w2 == 0:
                    dims.append(v2)
        elif num in (1, 2, 3, 4) and wt == 0:
            legacy[num] = v
    if data is None:
        data = np.zeros(0, "<f4")
    if not dims and legacy:
        dims = [legacy.get(k, 1) for k in (1, 2, 3, 4)]
    return np.array(data, dtype=np.float32).reshape(dims) if dims and int(np.prod(dims)) == data.size else np.array(data, dtype=np.float32)


def read_caffemodel(path):
    """Weights of a Caffe model file: {layer name: [blob, ...]} with every blob a float32 array of its stored
    shape.  Reads the NetParameter wire format directly (caffe.proto, [EXT]: NetParameter.layer = 100 and the V1
    `layers` = 2; LayerParameter.name = 1, .blobs = 7 (V1: name = 4, blobs = 6); BlobProto.data = 5 packed float,
    .shape = 7 {dim = 1}, legacy num/channels/height/width = 1..4)."""
    with open(path, "rb") as fh:
        buf = fh.read()
    out = {}
    for num, wt, v in _proto.fields(buf):
        if wt != 2 or num not in (100, 2):
            continue
        name_field, blob_field = (1, 7) if num == 100 else (4, 6)
        name, blobs = None, []
        for n2, w2, v2 in _proto.fields(v):
            if n2 == name_field and w2 == 2:
                name = bytes(v2).decode()
            elif n2 == blob_field and w2 == 2:
                blobs.append(_read_blob(v2))
        if name is not None and blobs:
            out[name] = blobs
    return out


def write_caffemodel(path, entries, name="net"):
    """Writes (layer name, type, [blob, ...]) entries, in their order, as a serialised NetParameter:
    NetParameter{name = 1, layer = 100 {name = 1, type = 2, blobs = 7 {shape = 7 {dim = 1}, data = 5}}}.  The blobs are
    float32 arrays of their Caffe shapes; an entry without blobs (ReLU, Pooling ...) is written as a real file holds it."""
    def blob(arr):
        arr = np.ascontiguousarray(arr, dtype="<f4")
        return _proto.message(7, _proto.message(1, b"".join(_proto._varint(d) for d in arr.shape))) + _proto.message(5, arr.tobytes())

    with open(path, "wb") as fh:
        fh.write(_proto.message(1, name.encode()))
        for layer, typ, blobs in entries:
            fh.write(_proto.message(100, _proto.message(1, layer.encode()) + _proto.message(2, typ.encode()) +
                                    b"".join(_proto.message(7, blob(b)) for b in blobs)))
