"""Wire-format readers for the hot path's outputs; mirrors
``/root/reference/scannertools/scannertools/types.py:23-41``."""
import numpy as np


def histograms(buf, protobufs=None):
    """One Histogram element: 3 x int32[bins], channel-major (types.py:23-27)."""
    # bufs[0] is None when element is null
    if buf is None:
        return None
    return np.split(np.frombuffer(buf, dtype=np.dtype(np.int32)), 3)


def flow(buf, height, width):
    """One OpticalFlow element: float32 (h, w, 2).  The reference's reader (types.py:36-41)
    takes the shape from a FrameInfo protobuf through an undefined ``db`` (dead code); here the
    shape is passed explicitly."""
    if buf is None:
        return None
    return np.frombuffer(buf, dtype=np.dtype(np.float32)).reshape((height, width, 2))


def flow_histograms(buf, protobufs=None):
    """One FlowHistogram element: 2 x int32[64], magnitude then angle
    (``flow_hist_reader``, scannertools/old/histograms.py:43-46)."""
    if buf is None:
        return None
    return np.split(np.frombuffer(buf, dtype=np.dtype(np.int32)), 2)


def frame_stat(buf, protobufs=None):
    """One BrightnessCPP / ContrastCPP / SharpnessCPP element: a 4-byte float (the reference runners' parser,
    ``struct.unpack('f', buf)[0]``, scannertools/old/imgproc.py:64,84,104)."""
    if buf is None:
        return None
    import struct
    return struct.unpack("f", buf)[0]


def pickled(buf, protobufs=None):
    """One Brightness / Contrast / Sharpness element: a pickled np.float64 (``pickle.loads``, old/imgproc.py:54,74,94)."""
    if buf is None:
        return None
    import pickle
    return pickle.loads(buf)


def poses(buf, protobufs=None):
    """Reader of the CPM2Output op's element (cpm2_output_kernel_cpu.cpp:177-180:
    serialize_proto_vector_of_vectors<scanner::Point>): u64 people; per person u64 joints; per joint
    an i32 byte size and the proto3 bytes of Point{float x = 1; y = 2; score = 3}.
    Returns float32 (people, 18, 3)."""
    import struct
    (n,), off = struct.unpack_from("<Q", buf, 0), 8
    out = []
    for _ in range(n):
        (m,) = struct.unpack_from("<Q", buf, off)
        off += 8
        person = np.zeros((m, 3), np.float32)
        for j in range(m):
            (sz,) = struct.unpack_from("<i", buf, off)
            off += 4
            end = off + sz
            while off < end:
                tag = buf[off]
                field, wire = tag >> 3, tag & 7
                if wire != 5 or not 1 <= field <= 3:
                    raise ValueError("unexpected field in a Point message")
                person[j, field - 1] = struct.unpack_from("<f", buf, off + 1)[0]
                off += 5
        out.append(person)
    return np.stack(out) if out else np.zeros((0, 18, 3), np.float32)


# ---- SharpnessBBoxCPP / SharpnessBBox elements ---------------------------------------------------------------------------
class BBox(tuple):
    """One bounding box (x1, y1, x2, y2) in pixel coordinates, the four fields of Scanner's ``BoundingBox`` message that the
    SharpnessBBox ops read (old/cpp_ops/imgproc.cpp:205-208).  A plain 4-tuple works wherever a BBox does."""
    __slots__ = ()

    def __new__(cls, x1, y1, x2, y2):
        return tuple.__new__(cls, (float(x1), float(y1), float(x2), float(y2)))

    x1 = property(lambda self: self[0])
    y1 = property(lambda self: self[1])
    x2 = property(lambda self: self[2])
    y2 = property(lambda self: self[3])


# BoundingBox is Scanner's message (scanner/types.proto), which is not part of the reference tree.  These field numbers are
# stated from knowledge of that file and have NOT been checked against it: float x1 = 1, y1 = 2, x2 = 3, y2 = 4; score = 5 and
# further fields follow and are skipped by wire type.
BBOX_FIELDS = {"x1": 1, "y1": 2, "x2": 3, "y2": 4}
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def bbox_message(box, extra=b""):
    """The proto3 bytes of one BoundingBox: the four coordinates as float fields 1..4 (a coordinate that is 0 is left out, as
    proto3 does), then ``extra`` (already serialised further fields, e.g. a score)."""
    from . import _proto
    return _proto.encode([(k + 1, "float", float(v)) for k, v in enumerate(tuple(box)[:4])]) + bytes(extra)


def write_bboxes(boxes):
    """One ``bboxes`` element as the reference's writer emits it (scannertools/types.py:68-74, Scanner's serialised proto
    vector): u64 count, then per box a u64 byte length and the BoundingBox message.  boxes: iterable of (x1, y1, x2, y2) or of
    ready message bytes."""
    import struct
    msgs = [bytes(b) if isinstance(b, (bytes, bytearray)) else bbox_message(b) for b in boxes]
    return struct.pack("<Q", len(msgs)) + b"".join(struct.pack("<Q", len(m)) + m for m in msgs)


def bboxes(buf, protobufs=None):
    """Reader of a ``bboxes`` element: list of BBox (float32 values, absent coordinates 0).  ValueError on truncated or
    over-long bytes, on a coordinate field that is not a float and on a malformed message; unknown fields are skipped."""
    import struct
    if buf is None:
        return None
    buf = bytes(buf)
    if len(buf) < 8:
        raise ValueError("bboxes element of %d bytes is shorter than its u64 count" % len(buf))
    (m,), off = struct.unpack_from("<Q", buf, 0), 8
    if m > (len(buf) - off) // 8:
        raise ValueError("bboxes element of %d bytes is shorter than its count of %d boxes says" % (len(buf), m))
    from . import _proto
    out = []
    for i in range(m):
        if len(buf) - off < 8:
            raise ValueError("box %d: bboxes element ends inside a length" % i)
        (ln,) = struct.unpack_from("<Q", buf, off)
        off += 8
        if ln > len(buf) - off:
            raise ValueError("box %d: bboxes element ends inside the message" % i)
        c = [0.0, 0.0, 0.0, 0.0]
        try:
            for number, wt, v in _proto.fields(buf[off:off + ln]):
                if 1 <= number <= 4:
                    if wt != 5:
                        raise ValueError("coordinate field %d is not a float" % number)
                    c[number - 1] = float(struct.unpack("<f", struct.pack("<I", v))[0])
        except ValueError as e:
            raise ValueError("box %d: malformed BoundingBox message (%s)" % (i, e)) from None
        off += ln
        out.append(BBox(*c))
    if off != len(buf):
        raise ValueError("bboxes element is %d bytes longer than its %d boxes" % (len(buf) - off, m))
    return out


# ---- FacenetOutput elements: boxes with a score --------------------------------------------------------------------------
BBOX_SCORE_FIELD = 5   # BoundingBox.score, stated from knowledge of scanner/types.proto like BBOX_FIELDS, not checked against it


def write_scored_bboxes(rows):
    """One ``bboxes`` element of the FacenetOutput op from rows [x1, y1, x2, y2, score] (any (m, 5) array-like): write_bboxes'
    format with the score as float field 5; like a coordinate, a score that is 0 is left out."""
    from . import _proto
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 5)
    return write_bboxes([bbox_message(r[:4], _proto.encode([(BBOX_SCORE_FIELD, "float", float(r[4]))])) for r in rows])


def scored_bboxes(buf, protobufs=None):
    """Reader of a FacenetOutput ``bboxes`` element: float32 (m, 5) rows [x1, y1, x2, y2, score], absent fields 0, in the
    element's order (descending score).  ValueError as for ``bboxes``, and on a score field that is not a float."""
    import struct
    if buf is None:
        return None
    buf = bytes(buf)
    boxes = bboxes(buf)                      # every structural check, and the coordinates
    from . import _proto
    out = np.zeros((len(boxes), 5), np.float32)
    off = 8
    for i, b in enumerate(boxes):
        (ln,) = struct.unpack_from("<Q", buf, off)
        off += 8
        out[i, :4] = b
        for number, wt, v in _proto.fields(buf[off:off + ln]):
            if number == BBOX_SCORE_FIELD:
                if wt != 5:
                    raise ValueError("box %d: score field is not a float" % i)
                out[i, 4] = np.frombuffer(struct.pack("<I", v), np.float32)[0]
        off += ln
    return out


def truncate_bboxes(boxes, h, w, where=""):
    """(int)coordinate per box as the reference truncates it (toward zero; imgproc.cpp:205-208, old/imgproc.py:47-50):
    int32 (m, 4) rows x1, y1, x2, y2.  ValueError, naming the box, for a coordinate that is not finite or does not fit an
    int32 and for a box that does not satisfy 0 <= x1 < x2 <= w and 0 <= y1 < y2 <= h (the reference trips a CV_Assert or
    slices garbage there)."""
    import math
    out = np.zeros((len(boxes), 4), np.int32)
    for i, b in enumerate(boxes):
        t = []
        for v in tuple(b)[:4]:
            v = float(v)
            if not math.isfinite(v) or not INT32_MIN <= math.trunc(v) <= INT32_MAX:
                raise ValueError("%sbox %d: coordinate %r is not finite or does not fit an int32" % (where, i, v))
            t.append(math.trunc(v))
        if len(t) != 4:
            raise ValueError("%sbox %d: needs x1, y1, x2, y2" % (where, i))
        x1, y1, x2, y2 = t
        if not (0 <= x1 < x2 <= w and 0 <= y1 < y2 <= h):
            raise ValueError("%sbox %d: x %d..%d, y %d..%d is empty or not inside the %dx%d frame" % (where, i, x1, x2, y1, y2, w, h))
        out[i] = t
    return out


def sharpness_bbox(buf, protobufs=None):
    """One SharpnessBBoxCPP element: a 4-byte float per box (``struct.unpack('{}f'.format(len(buf) // 4), buf)``,
    old/imgproc.py:145); a row without boxes is an element of zero bytes and reads as an empty tuple."""
    if buf is None:
        return None
    import struct
    if len(buf) % 4:
        raise ValueError("sharpness_bbox element of %d bytes is not a whole number of floats" % len(buf))
    return struct.unpack("<%df" % (len(buf) // 4), buf)
