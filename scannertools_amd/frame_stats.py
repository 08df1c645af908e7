"""Frame statistics for MI355X: mirror of ``/root/reference/scannertools/scannertools/old/imgproc.py``.

The reference's legacy op library has three per-frame statistics in two flavours: the C++ ops ``BrightnessCPP``,
``ContrastCPP`` and ``SharpnessCPP`` (old/cpp_ops/imgproc.cpp:50-175; a 4-byte float per row) and the Python ops
``Brightness``, ``Contrast`` and ``Sharpness`` (old/imgproc.py:11-37; a pickled float64 per row).  Here the C++ ops are
kernel classes of the op library (scanner_kernels/frame_stats_kernel_hip.cpp) and the Python ops run the same HIP kernels
(``HipContext.frame_stats``): one exact moments pass over the frame and a finishing launch.  The six ``compute_*`` runners
mirror the reference's pipelines (old/imgproc.py:57-167), in the shape of ``scannertools_amd.histograms``.  There is no
CPU fallback: without the HIP library or a GPU the ops raise.
"""
import pickle

import numpy as np

from . import types as _types
from .engine import CacheMode, DeviceType, NamedStream, NamedVideoStream, PerfParams

_CTX = {}


def _ctx(device):
    from .hip import HipContext
    if device not in _CTX:
        _CTX[device] = HipContext(device)
    return _CTX[device]


def check_frames(name, frames):
    """Every frame (h, w, 3) uint8, as the reference's ops read them (frame_to_mat of an RGB frame)."""
    import torch
    for i, f in enumerate(frames):
        if len(f.shape) != 3 or f.shape[2] != 3 or f.dtype not in (np.uint8, torch.uint8):
            raise ValueError("%s: frame %d is %s %s, not (h, w, 3) uint8" % (name, i, tuple(f.shape), f.dtype))


def stat_values(kind, frames, device=0):
    """Statistic ``kind`` (a name of scannertools_amd._native.FS_KINDS) of every frame: numpy float32 for the *CPP kinds,
    float64 for the others.  frames: (h, w, 3) uint8 numpy arrays or CUDA tensors; frames of one shape share a launch."""
    import torch
    check_frames(kind, frames)
    cpp = kind.endswith("CPP")
    out = np.empty(len(frames), np.float32 if cpp else np.float64)
    if not len(frames):
        return out
    dev = torch.device("cuda", device)
    groups = {}
    for i, f in enumerate(frames):
        groups.setdefault(tuple(f.shape), []).append(i)
    for rows in groups.values():
        fr = [(frames[i] if isinstance(frames[i], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames[i])))
              .to(device=dev).contiguous() for i in rows]
        out[rows] = _ctx(device).frame_stats(fr, kind).cpu().numpy()
    return out


def stat_rows(kind, frames, device=0):
    """Rows of the Python op ``kind`` (Brightness, Contrast or Sharpness): ``pickle.dumps(np.float64(v))`` per frame, the
    element old/imgproc.py:17,30,36 emit."""
    return [pickle.dumps(np.float64(v)) for v in stat_values(kind, frames, device)]


def bbox_records(name, frames, bbox_rows, row_ids=None):
    """The (m, 5) int64 records [row, x1, y1, x2, y2] and the per-row box counts of a SharpnessBBox call: every ``bboxes``
    element parsed (scannertools_amd.types.bboxes) and every box truncated and checked against its frame
    (types.truncate_bboxes).  ValueError naming the row (``row_ids[i]`` if given, else i) and the box; nothing has touched the GPU at that point."""
    check_frames(name, frames)
    if len(frames) != len(bbox_rows):
        raise ValueError("%s: %d frames but %d bboxes rows" % (name, len(frames), len(bbox_rows)))
    rec, counts = [], []
    for i, (f, e) in enumerate(zip(frames, bbox_rows)):
        where = "%s: row %d: " % (name, row_ids[i] if row_ids is not None else i)
        try:
            boxes = _types.bboxes(e) if isinstance(e, (bytes, bytearray, memoryview)) else list(e)
        except ValueError as err:
            raise ValueError(where + str(err)) from None
        t = _types.truncate_bboxes(boxes, int(f.shape[0]), int(f.shape[1]), where)
        rec.append(np.concatenate([np.full((len(t), 1), i, np.int64), t.astype(np.int64)], axis=1))
        counts.append(len(t))
    return (np.concatenate(rec) if rec else np.zeros((0, 5), np.int64)), counts


def bbox_values(kind, frames, bbox_rows, device=0):
    """Sharpness ``kind`` ("SharpnessCPP": float32, "Sharpness": float64) of every box of every row: a list with one numpy
    array per row.  frames: (h, w, 3) uint8 numpy arrays or CUDA tensors; bbox_rows: per frame a ``bboxes`` element (bytes) or
    a list of (x1, y1, x2, y2).  All boxes of frames of one shape share one launch (HipContext.bbox_sharpness)."""
    import torch
    name = "SharpnessBBoxCPP" if kind.endswith("CPP") else "SharpnessBBox"
    rec, counts = bbox_records(name, frames, bbox_rows)
    vals = np.empty(len(rec), np.float32 if kind.endswith("CPP") else np.float64)
    if len(rec):
        dev = torch.device("cuda", device)
        groups = {}
        for i in sorted(set(rec[:, 0].tolist())):      # rows that have a box
            groups.setdefault(tuple(frames[i].shape), []).append(i)
        for rows in groups.values():
            fr = [(frames[i] if isinstance(frames[i], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames[i])))
                  .to(device=dev).contiguous() for i in rows]
            slot = {r: k for k, r in enumerate(rows)}
            sel = np.flatnonzero(np.isin(rec[:, 0], rows))
            sub = rec[sel].copy()
            sub[:, 0] = [slot[r] for r in sub[:, 0].tolist()]
            vals[sel] = _ctx(device).bbox_sharpness(fr, sub, kind).cpu().numpy()
    ends = np.cumsum(counts)
    return [vals[e - c:e] for c, e in zip(counts, ends)]


def bbox_rows_cpp(frames, bbox_rows, device=0):
    """Rows of SharpnessBBoxCPP: 4 bytes per box (imgproc.cpp:227-228), zero bytes for a row without boxes."""
    return [v.astype("<f4").tobytes() for v in bbox_values("SharpnessCPP", frames, bbox_rows, device)]


def bbox_rows_py(frames, bbox_rows, device=0):
    """Rows of the Python op SharpnessBBox: ``pickle.dumps`` of the list of float64 values (old/imgproc.py:44-54)."""
    return [pickle.dumps([np.float64(x) for x in v]) for v in bbox_values("Sharpness", frames, bbox_rows, device)]


def brightness(config, frame):
    """Signature of the reference's python op (old/imgproc.py:11-17): the mean of the frame's COLOR_RGB2YUV luma."""
    return stat_rows("Brightness", [frame])[0]


def contrast(config, frame):
    """old/imgproc.py:20-30: the population standard deviation of the luma."""
    return stat_rows("Contrast", [frame])[0]


def sharpness(config, frame):
    """old/imgproc.py:33-36: the variance of cv2.Laplacian(frame, CV_64F) over all three channels."""
    return stat_rows("Sharpness", [frame])[0]


def sharpness_bbox(config, frame, bboxes):
    """What old/imgproc.py:44-54 means (line 46 reads ``bboxes.self.config...`` and cannot run as written): per box of the
    ``bboxes`` element, the variance of cv2.Laplacian(cv2.resize(frame[y1:y2, x1:x2], (200, 200)), CV_64F); the pickled list."""
    return bbox_rows_py([frame], [bboxes])[0]


try:  # register with Scanner when it is installed, exactly as the reference module does
    import scannerpy as _sp

    brightness = _sp.register_python_op(name='Brightness')(brightness)
    contrast = _sp.register_python_op(name='Contrast')(contrast)
    sharpness = _sp.register_python_op(name='Sharpness')(sharpness)
    sharpness_bbox = _sp.register_python_op(name='SharpnessBBox')(sharpness_bbox)
except ImportError:  # scannerpy absent: the in-process engine (scannertools_amd.engine) is used
    pass


# ---- runners: old/imgproc.py:57-167 ---------------------------------------------------------------------------------------
def _run(sc, name, suffix, build):
    frame = sc.io.Input([NamedVideoStream(sc, name)])
    out = NamedStream(sc, '%s_%s' % (name, suffix))
    sc.run(sc.io.Output(build(frame), [out]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    return out


def _cpp(op, suffix):
    def runner(sc, videos, device=DeviceType.GPU, batch=1):
        return [_run(sc, v, suffix, lambda f: getattr(sc.ops, op)(frame=f, device=device, batch=batch)) for v in videos]
    runner.__name__ = "compute_" + suffix
    runner.__doc__ = ("%s(frame) per video (old/imgproc.py); rows read with scannertools_amd.types.frame_stat (a float).  The "
                      "reference places the op on DeviceType.CPU; ``batch=1`` as there, ``batch=64`` and up fills the GPU." % op)
    return runner


def _py(op, suffix):
    def runner(sc, videos):
        return [_run(sc, v, suffix, lambda f: getattr(sc.ops, op)(frame=f)) for v in videos]
    runner.__name__ = "compute_" + suffix
    runner.__doc__ = "%s(frame) per video (old/imgproc.py); rows read with scannertools_amd.types.pickled (np.float64)." % op
    return runner


compute_brightness = _py("Brightness", "brightness")
compute_brightness_cpp = _cpp("BrightnessCPP", "brightness_cpp")
compute_contrast = _py("Contrast", "contrast")
compute_contrast_cpp = _cpp("ContrastCPP", "contrast_cpp")
compute_sharpness = _py("Sharpness", "sharpness")
compute_sharpness_cpp = _cpp("SharpnessCPP", "sharpness_cpp")



def _bbox_run(sc, video, bboxes, suffix, build):
    frame = sc.io.Input([NamedVideoStream(sc, video)])
    boxes = sc.io.Input([bboxes if isinstance(bboxes, NamedStream) else NamedStream(sc, bboxes)])
    out = NamedStream(sc, '%s_%s' % (video, suffix))
    sc.run(sc.io.Output(build(frame, boxes), [out]), PerfParams.estimate(), cache_mode=CacheMode.Overwrite)
    return out


def compute_sharpness_bbox(sc, videos, bboxes):
    """SharpnessBBox(frame, bboxes) per video (old/imgproc.py:129-147); ``bboxes``: per video a stream of bboxes elements (a
    NamedStream or its name, see Client.ingest_rows).  Rows read with scannertools_amd.types.pickled (a list of np.float64)."""
    return [_bbox_run(sc, v, b, "sharpness_bbox", lambda f, bb: sc.ops.SharpnessBBox(frame=f, bboxes=bb)) for v, b in zip(videos, bboxes)]


def compute_sharpness_bbox_cpp(sc, videos, bboxes, device=DeviceType.GPU, batch=1):
    """SharpnessBBoxCPP(frame, bboxes) per video (old/imgproc.py:149-167, with the ``bboxes`` column its pipeline forgets to
    pass at :156).  Rows read with scannertools_amd.types.sharpness_bbox (a tuple of floats)."""
    return [_bbox_run(sc, v, b, "sharpness_bbox_cpp",
                      lambda f, bb: sc.ops.SharpnessBBoxCPP(frame=f, bboxes=bb, device=device, batch=batch)) for v, b in zip(videos, bboxes)]


reader_cpp = _types.frame_stat   # parser_fn of the *CPPPipeline classes (old/imgproc.py:64,84,104)
reader = _types.pickled          # parser_fn of the Python-op pipelines (old/imgproc.py:54,74,94)
reader_bbox_cpp = _types.sharpness_bbox   # old/imgproc.py:145
