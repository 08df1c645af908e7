"""Device-side ops: thin Python over the C ABI (include/scannertools_hip.h).

PyTorch is used only for device memory and streams: inputs/outputs are ``torch`` CUDA tensors
whose ``data_ptr()`` is handed to the library, and kernels are enqueued on torch's current
stream of the context's device.  All arithmetic happens in the HIP kernels under ``csrc/``.
"""
import ctypes

import numpy as np
import torch

from . import _native
from ._native import FbParams, StError, default_params  # noqa: F401


def _require_cuda(t, dtype, name, device=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("%s must be a CUDA tensor (no CPU fallback exists)" % name)
    if t.dtype != dtype:
        raise TypeError("%s must have dtype %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if device is not None and t.device != device:
        raise ValueError("%s lives on %s but the context runs on %s" % (name, t.device, device))


def _check_out(out, shape, dtype, device):
    """A caller-supplied output buffer is written through its raw pointer: it must be exactly the
    dense device array the kernel will produce."""
    _require_cuda(out, dtype, "out", device)
    if tuple(out.shape) != tuple(shape):
        raise ValueError("out must have shape %s, got %s" % (tuple(shape), tuple(out.shape)))
    return out


def _ptr_table(addresses):
    """A ctypes array of the given addresses (at least one entry, so that an empty batch still hands over a table)."""
    addresses = list(addresses)
    return (ctypes.c_void_p * max(len(addresses), 1))(*addresses)


class HipContext:
    """One ``st_ctx``: per-kernel-instance state (stream binding, scratch).  Mirrors the role of
    a Scanner kernel instance's private GPU state (optical_flow_kernel_gpu.cpp:101-107)."""

    def __init__(self, device=0, workspace_limit=None):
        self._L = _native.lib()
        if not torch.cuda.is_available():
            raise RuntimeError("HipContext needs a GPU: torch.cuda.is_available() is False")
        self.device = torch.device("cuda", device if isinstance(device, int) else torch.device(device).index or 0)
        h = ctypes.c_void_p()
        st = self._L.st_ctx_create(self.device.index, ctypes.byref(h))
        if st != 0:
            raise StError(st, "st_ctx_create(%d) failed" % self.device.index)
        self._h = h
        self._bound_stream = -1
        if workspace_limit:
            self._check(self._L.st_ctx_set_workspace_limit(self._h, int(workspace_limit)))

    # -- plumbing ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._L.st_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, st):
        if st != 0:
            raise StError(st, (self._L.st_ctx_last_error(self._h) or b"").decode() or
                          self._L.st_status_string(st).decode())

    def _bind(self):
        """Enqueue on torch's current stream so that torch ops and events order with ours."""
        s = torch.cuda.current_stream(self.device).cuda_stream
        if s != self._bound_stream:
            self._check(self._L.st_ctx_set_stream(self._h, ctypes.c_void_p(s)))
            self._bound_stream = s

    def sync(self):
        self._check(self._L.st_ctx_sync(self._h))

    def flow_concurrent(self):
        """True if the last optical_flow call chose its kernels for a GPU shared with other kernel instances (diagnostic)."""
        return bool(self._L.st_ctx_flow_concurrent(self._h))

    def release_workspace(self):
        self._check(self._L.st_ctx_release_workspace(self._h))

    def timing_enable(self, kernel_ids):
        mask = 0
        for k in kernel_ids:
            mask |= 1 << k
        self._check(self._L.st_ctx_timing_enable(self._h, mask))

    def timing_reset(self):
        self._check(self._L.st_ctx_timing_reset(self._h))

    def timing_read(self, kernel_id):
        n, ms = ctypes.c_int(), ctypes.c_double()
        self._check(self._L.st_ctx_timing_read(self._h, kernel_id, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value

    # -- the front of a batched method: rows, pointer tables, the output ---------------------------
    def _rows(self, x, dtype, what, tail=None, shaped=True):
        """(rows, n, shape) of a batch given as a list / tuple of per-row tensors or as one tensor, which is split along its
        first dimension.  Every row is a contiguous CUDA tensor of ``dtype`` on this device; unless ``shaped`` is False, all
        are (h, w, c) of one shape, with c == ``tail`` when given.  An empty batch has shape ()."""
        rows = list(x) if isinstance(x, (list, tuple)) else list(x.unbind(0))
        for r in rows:
            _require_cuda(r, dtype, what, self.device)
        shape = tuple(rows[0].shape) if rows else ()
        if shaped and rows and (len(shape) != 3 or tail not in (None, shape[2]) or any(tuple(r.shape) != shape for r in rows)):
            raise ValueError("all %ss must be (h,w,%s) with equal shape" % (what, "c" if tail is None else tail))
        return rows, len(rows), shape

    @staticmethod
    def _table(rows):
        """The host pointer table of a batch: ``rows`` is a list of tensors, or one tensor whose rows along the first
        dimension are the entries (an output that the kernels write frame by frame)."""
        if isinstance(rows, torch.Tensor):
            step = rows.stride(0) * rows.element_size()
            return _ptr_table(rows.data_ptr() + i * step for i in range(rows.shape[0]))
        return _ptr_table(r.data_ptr() for r in rows)

    def _out(self, out, shape, dtype):
        """The output of a call: a new tensor, or the caller's once it is found to be exactly that dense device array."""
        return torch.empty(shape, dtype=dtype, device=self.device) if out is None else _check_out(out, shape, dtype, self.device)

    # -- Histogram --------------------------------------------------------------------------
    def histogram(self, frames, bins=16, out=None):
        """Per-channel histograms of U8 RGB frames.

        frames: CUDA uint8 tensor (n,h,w,3) (one contiguous stream) or a list of (h,w,3)
        tensors (one buffer per Scanner element).  Returns int32 (n,3,bins): row i is the
        192-byte element the reference's Histogram op emits for bins=16
        (histogram_kernel_cpu.cpp:20,40-44)."""
        self._bind()
        front = self._rows_or_strided(frames, torch.uint8, "frame", 3)
        out = self._out(out, (front[1], 3, bins), torch.int32)
        return self._call_rows("st_hist_u8c3", front, 3, out, bins, ctypes.c_void_p(out.data_ptr()))

    # -- frame statistics -------------------------------------------------------------------
    def frame_moments(self, frames, luma=True, laplacian=True, out=None):
        """Exact moments of U8 RGB frames (st_frame_moments_u8c3_*): int64 (n, 8), row i = [sum Y, sum Y^2, sum L_R, sum L_G,
        sum L_B, sum L_R^2, sum L_G^2, sum L_B^2] of frame i, Y the COLOR_RGB2YUV luma byte and L_c the reflect-101 Laplacian of
        channel c.  ``luma`` / ``laplacian`` pick the moments computed (the others are 0).  frames: CUDA uint8 tensor
        (n,h,w,3) or a list of (h,w,3) tensors of one shape."""
        self._bind()
        what = (_native.FM_LUMA if luma else 0) | (_native.FM_LAPLACIAN if laplacian else 0)
        front = self._rows_or_strided(frames, torch.uint8, "frame", 3)
        out = self._out(out, (front[1], 8), torch.int64)
        return self._call_rows("st_frame_moments_u8c3", front, 3, out, what, ctypes.c_void_p(out.data_ptr()))

    def frame_stats(self, frames, kind):
        """One frame statistic per frame (st_frame_stats_finish over st_frame_moments_u8c3_*): ``kind`` is a name of
        _native.FS_KINDS or its value.  BrightnessCPP / ContrastCPP / SharpnessCPP give float32 (the element of the legacy C++
        ops, old/cpp_ops/imgproc.cpp:50-175), Brightness / Contrast / Sharpness float64 (the value their Python twins
        pickle, old/imgproc.py:11-37).  frames as for frame_moments."""
        k = _native.FS_KINDS[kind] if isinstance(kind, str) else int(kind)
        if k not in _native.FS_KINDS.values():
            raise ValueError("unknown frame statistic %r" % (kind,))
        sharp = k in (_native.FS_KINDS["SharpnessCPP"], _native.FS_KINDS["Sharpness"])
        m = self.frame_moments(frames, luma=not sharp, laplacian=sharp)
        n = m.shape[0]
        out = torch.empty((n,), dtype=torch.float32 if k < 3 else torch.float64, device=self.device)
        if n == 0:
            return out
        h, w = (frames[0].shape[0], frames[0].shape[1]) if isinstance(frames, (list, tuple)) else (frames.shape[1], frames.shape[2])
        self._check(self._L.st_frame_stats_finish(self._h, ctypes.c_void_p(m.data_ptr()), n, h, w, k, ctypes.c_void_p(out.data_ptr())))
        return out

    def _rows_or_strided(self, x, dtype, what, tail):
        """The front of an op with a *_batch and a *_strided entry point: x is a list of (h,w,tail) rows, one buffer per Scanner
        element, or one (n,h,w,tail) tensor.  Returns (is a list?, n, h, w, the pointer table or the base pointer); an empty
        list has h = w = 1."""
        if isinstance(x, (list, tuple)):
            rows, n, shape = self._rows(x, dtype, what, tail)
            return (True, n) + (tuple(int(v) for v in shape[:2]) if n else (1, 1)) + (self._table(rows),)
        _require_cuda(x, dtype, what + "s", self.device)
        if x.dim() != 4 or x.shape[3] != tail:
            raise ValueError("%ss must be (n,h,w,%d)" % (what, tail))
        return (False,) + tuple(int(v) for v in x.shape[:3]) + (ctypes.c_void_p(x.data_ptr()),)

    def _call_rows(self, name, front, pixel_bytes, out, *rest):
        """name_batch or name_strided (dense frames of pixel_bytes * h * w bytes) on a front of _rows_or_strided, unless
        ``out`` is empty; returns out."""
        is_list, n, h, w, arg = front
        if out.shape[0]:
            if is_list:
                self._check(getattr(self._L, name + "_batch")(self._h, arg, n, h, w, *rest))
            else:
                self._check(getattr(self._L, name + "_strided")(self._h, arg, pixel_bytes * h * w, n, h, w, *rest))
        return out

    def _bbox_args(self, frames, boxes):
        """(front of the frames, int32 (m, 5) box records) of a bbox_* call.  Every box is checked here, against the frame
        count and size, before the library is entered."""
        boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.int64).reshape(-1, 5))
        front = self._rows_or_strided(frames, torch.uint8, "frame", 3)
        _, n, h, w, _ = front
        f, x1, y1, x2, y2 = boxes.T
        bad = ~((0 <= f) & (f < n) & (0 <= x1) & (x1 < x2) & (x2 <= w) & (0 <= y1) & (y1 < y2) & (y2 <= h))
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError("box %d {frame %d, x %d..%d, y %d..%d} is empty or not inside one of %d frames of %dx%d"
                             % ((i,) + tuple(boxes[i].tolist()[k] for k in (0, 1, 3, 2, 4)) + (n, w, h)))
        return front, np.ascontiguousarray(boxes.astype(np.int32))

    def bbox_moments(self, frames, boxes, out=None):
        """Exact Laplacian moments of boxes of U8 RGB frames, each box resized to 200 x 200 with the Resize op's INTER_LINEAR
        arithmetic (st_bbox_moments_u8c3_*; the SharpnessBBox ops, old/cpp_ops/imgproc.cpp:177-234): int64 (m, 8) in the
        layout of frame_moments, row i = [0, 0, sum L_R, sum L_G, sum L_B, sum L_R^2, sum L_G^2, sum L_B^2] of box i.
        frames: CUDA uint8 tensor (n,h,w,3) or a list of (h,w,3) tensors of one shape.  boxes: (m, 5) integers
        [frame index, x1, y1, x2, y2], the region being rows y1 .. y2-1 and columns x1 .. x2-1 of that frame; a box that is
        empty or not inside its frame is a ValueError and nothing is launched.  One launch for all boxes."""
        self._bind()
        front, rec = self._bbox_args(frames, boxes)
        m = rec.shape[0]
        out = self._out(out, (m, 8), torch.int64)
        return self._call_rows("st_bbox_moments_u8c3", front, 3, out, rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), m,
                               ctypes.c_void_p(out.data_ptr()))

    def bbox_sharpness(self, frames, boxes, kind):
        """One sharpness value per box (st_bbox_sharpness_u8c3_*: the moments launch with the finishing formula fused):
        ``kind`` "SharpnessCPP" gives float32, the element of SharpnessBBoxCPP (imgproc.cpp:210-226), "Sharpness" float64, the
        value SharpnessBBox pickles (old/imgproc.py:44-54).  frames and boxes as for bbox_moments."""
        k = _native.FS_KINDS[kind] if isinstance(kind, str) else int(kind)
        if k not in (_native.FS_KINDS["SharpnessCPP"], _native.FS_KINDS["Sharpness"]):
            raise ValueError("bbox_sharpness: kind must be SharpnessCPP or Sharpness, not %r" % (kind,))
        self._bind()
        front, rec = self._bbox_args(frames, boxes)
        m = rec.shape[0]
        out = torch.empty((m,), dtype=torch.float32 if k < 3 else torch.float64, device=self.device)
        return self._call_rows("st_bbox_sharpness_u8c3", front, 3, out, rec.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), m, k,
                               ctypes.c_void_p(out.data_ptr()))

    # -- flow consumers ---------------------------------------------------------------------
    def shot_boundaries(self, hist, window=500, k_std=2.5, return_diffs=False):
        """ShotBoundaries on device-resident histograms (shot_detection.py:12-28): hist = CUDA int32 (n, 3, bins) as
        `histogram` returns them.  Returns the list of boundary frame indices (the reference op's row 0), bit for bit
        the host op's; with return_diffs also the float64 distances diffs[i]."""
        self._bind()
        _require_cuda(hist, torch.int32, "hist", self.device)
        if hist.dim() != 3 or hist.shape[1] != 3:
            raise ValueError("hist must be (n, 3, bins)")
        hist = hist.contiguous()
        n, _, bins = hist.shape
        flags = torch.empty((n,), dtype=torch.uint8, device=self.device)
        diffs = torch.empty((n,), dtype=torch.float64, device=self.device) if return_diffs else None
        self._check(self._L.st_shot_boundaries(self._h, ctypes.c_void_p(hist.data_ptr()), n, bins, int(window), float(k_std),
                                               ctypes.c_void_p(flags.data_ptr()), ctypes.c_void_p(diffs.data_ptr()) if return_diffs else None))
        self.sync()
        idx = [int(i) for i in torch.nonzero(flags).flatten().cpu()]
        return (idx, diffs) if return_diffs else idx

    def flow_histogram(self, flows, out=None):
        """FlowHistogram (old/cpp_ops/flow_histogram_kernel_cpu.cpp:26-57): magnitude and angle
        histograms (64 bins on [0,64) px and [0,360) degrees) of flow frames.

        flows: CUDA float32 tensor (n,h,w,2) or a list of (h,w,2) tensors.  Returns int32
        (n,2,64): row i is the 512-byte element the reference op emits."""
        self._bind()
        front = self._rows_or_strided(flows, torch.float32, "flow", 2)
        out = self._out(out, (front[1], 2, 64), torch.int32)
        return self._call_rows("st_flow_hist", front, 8, out, ctypes.c_void_p(out.data_ptr()))

    def draw_flow(self, frames, flows, out=None):
        """DrawFlow (scannertools/vis.py:8-12): frames (n,h,w,3) uint8 and flows (n,h,w,2) float32
        (tensors or lists of per-row tensors) -> (n,h,2w,3) uint8, the frame beside its flow map."""
        self._bind()
        fr, n, shape = self._rows(frames, torch.uint8, "frame", 3)
        fl, nfl, fshape = self._rows(flows, torch.float32, "flow", 2)
        if nfl != n:
            raise ValueError("frames and flows must have the same number of rows")
        if n == 0:
            return torch.zeros((0, 0, 0, 3), dtype=torch.uint8, device=self.device)
        h, w, _ = shape
        if fshape[:2] != (h, w):
            raise ValueError("frames must be (h,w,3) and flows (h,w,2) with equal h,w")
        out = self._out(out, (n, h, 2 * w, 3), torch.uint8)
        self._check(self._L.st_draw_flow_batch(self._h, self._table(fr), self._table(fl), n, h, w, self._table(out)))
        return out

    # -- sibling imgproc ops ----------------------------------------------------------------
    def box_blur(self, frames, kernel_size, out=None):
        """Blur op (blur_kernel_cpu.cpp:50-81): k x k integer box filter of (n,h,w,3) uint8 frames
        (a tensor or a list of (h,w,3) tensors); border pixels are 0."""
        self._bind()
        fr, n, shape = self._rows(frames, torch.uint8, "frame", 3)
        if n == 0:
            return torch.zeros((0, 0, 0, 3), dtype=torch.uint8, device=self.device)
        h, w, _ = shape
        out = self._out(out, (n, h, w, 3), torch.uint8)
        self._check(self._L.st_box_blur_u8c3_batch(self._h, self._table(fr), n, h, w, int(kernel_size), self._table(out)))
        return out

    def resize(self, frames, width, height, interpolation=_native.INTER_LINEAR, out=None):
        """Resize op (resize_kernel.cpp:68-73): (n,h,w,c) uint8 frames (a tensor or a list of (h,w,c)
        tensors) -> (n,height,width,c) uint8, cv::resize semantics for 8-bit frames."""
        self._bind()
        fr, n, shape = self._rows(frames, torch.uint8, "frame")
        if n == 0:
            c = frames.shape[3] if isinstance(frames, torch.Tensor) and frames.dim() == 4 else 3
            return torch.zeros((0, height, width, c), dtype=torch.uint8, device=self.device)
        h, w, c = shape
        out = self._out(out, (n, height, width, c), torch.uint8)
        self._check(self._L.st_resize_u8_batch(self._h, self._table(fr), n, h, w, c, int(height), int(width), int(interpolation),
                                               self._table(out)))
        return out

    def montage(self, frames, canvas, target_width, target_height, frames_per_row, first_slot=0):
        """Montage op's tile writes (montage_kernel_gpu.cpp): (n,h,w,3) uint8 frames (a tensor or a list of (h,w,3) tensors)
        resized INTER_LINEAR to (target_height, target_width) into tiles first_slot .. first_slot+n-1 of `canvas`, a
        (montage_h, montage_w, 3) uint8 tensor, tile s at ((s % frames_per_row) * target_width, (s // frames_per_row) *
        target_height).  One launch; the rest of the canvas is left as it is.  Returns canvas."""
        self._bind()
        _require_cuda(canvas, torch.uint8, "canvas", self.device)
        if canvas.dim() != 3 or canvas.shape[2] != 3 or not canvas.is_contiguous():
            raise ValueError("canvas must be a contiguous (montage_h, montage_w, 3) tensor")
        fr, n, shape = self._rows(frames, torch.uint8, "frame", 3)
        if n == 0:
            return canvas
        h, w, _ = shape
        last = int(first_slot) + n - 1
        if (frames_per_row * target_width > canvas.shape[1] or
                (last // frames_per_row + 1) * target_height > canvas.shape[0]):
            raise ValueError("tiles %d..%d of %dx%d do not fit a %dx%d canvas" % (first_slot, last, target_width, target_height,
                                                                                  canvas.shape[1], canvas.shape[0]))
        self._check(self._L.st_montage_u8c3_batch(self._h, self._table(fr), n, h, w, canvas.data_ptr(), int(canvas.shape[1]),
                                                  int(target_width), int(target_height), int(frames_per_row), int(first_slot)))
        return canvas

    def cvt_color(self, frames, code, gray_bits=15, out=None):
        """ConvertColor op (convert_color_kernel.cpp:268-271): cv::cvtColor on (n,h,w,c) uint8 frames;
        ``code`` is a cv::ColorConversionCodes value or one of the names in _native.COLOR_CODES."""
        self._bind()
        if isinstance(code, str):
            if code not in _native.COLOR_CODES:
                raise ValueError("conversion %r is not implemented" % code)
            code = _native.COLOR_CODES[code]
        fr, n, shape = self._rows(frames, torch.uint8, "frame")
        if n == 0:
            return torch.zeros((0, 0, 0, 3), dtype=torch.uint8, device=self.device)
        h, w, c = shape
        oh, ow, oc = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        if self._L.st_cvt_color_out_shape(int(code), h, w, c, ctypes.byref(oh), ctypes.byref(ow), ctypes.byref(oc)) != 0:
            raise ValueError("conversion code %d on %dx%d frames of %d channel(s) is not implemented" % (code, w, h, c))
        out = self._out(out, (n, oh.value, ow.value, oc.value), torch.uint8)
        self._check(self._L.st_cvt_color_u8_batch(self._h, self._table(fr), n, h, w, c, int(code), int(gray_bits), self._table(out)))
        return out

    def decode_jpeg(self, streams, out=None, entropy="host", split="interval", subseq_bytes=None, max_rounds=None, scale=1):
        """ImageDecoder op (image_decoder_kernel_cpu.cpp:16-29): a list of baseline JPEG streams (bytes) of one shape ->
        (n, h, w, c) uint8 CUDA tensor, c = 3 in R, G, B order or 1; bit-exact to libjpeg's defaults.  The shape is the first
        stream's; a stream of another shape, or one that is refused or malformed, raises StError naming it, and nothing is
        written.  entropy="host" (the default): entropy decoding runs on host threads (ST_JPEG_THREADS), the rest in HIP
        kernels on the current stream.  entropy="gpu": the Huffman decoder is a HIP kernel too, one lane per restart interval
        (what st_jpeg_decode_batch_gpu does); every stream must have restart intervals (StError naming the one that has none).
        entropy="auto": "gpu" when every stream's probe reports a restart interval, else "host".  Same frames either way.
        split="subsequence" (with entropy "gpu" or "auto", which then mean the same): one lane per subsequence of
        ``subseq_bytes`` raw bytes, at most ``max_rounds`` round launches (None: the library's defaults), what
        st_jpeg_decode_batch_gpu_split does; streams need no restart intervals.  ``last_jpeg_rounds()`` then tells the round
        launches the call took.  scale = 2, 4 or 8: the frames at 1/2, 1/4 or 1/8, (n, ceil(h / scale), ceil(w / scale), c),
        bit-exact to libjpeg's scaled decoding (cv::IMREAD_REDUCED_COLOR_* / _GRAYSCALE_*, Pillow's draft()); anything but
        1, 2, 4 or 8 raises ValueError.  It composes with every entropy and split: whatever the arguments, the call made is
        ONE st_jpeg_decode_batch_scaled(scale, ST_JPEG_ENTROPY_HOST | _INTERVAL | _SUBSEQUENCE, opts)."""
        if isinstance(scale, bool) or scale not in JPEG_SCALES:
            raise ValueError("scale must be one of 1, 2, 4, 8, got %r" % (scale,))
        scale = int(scale)
        if entropy not in JPEG_ENTROPY_MODES:
            raise ValueError("entropy must be one of %s, got %r" % (", ".join(repr(m) for m in JPEG_ENTROPY_MODES), entropy))
        if split not in JPEG_ENTROPY_SPLITS:
            raise ValueError("split must be one of %s, got %r" % (", ".join(repr(m) for m in JPEG_ENTROPY_SPLITS), split))
        if split == "subsequence" and entropy == "host":
            raise ValueError("split='subsequence' decodes on the device: entropy must be 'gpu' or 'auto', got 'host'")
        self._bind()
        streams = [bytes(s) for s in streams]
        n = len(streams)
        if n == 0:
            return torch.zeros((0, 0, 0, 3), dtype=torch.uint8, device=self.device)
        info = probe_jpeg(streams[0])
        h, w = info["h"], info["w"]
        shape = (n,) + jpeg_scaled_size(h, w, scale) + (info["channels"],)
        out = self._out(out, shape, torch.uint8)
        bufs = _ptr_table(ctypes.cast(ctypes.c_char_p(s), ctypes.c_void_p).value for s in streams)
        sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
        to = self._table(out)
        if split != "subsequence" and entropy == "auto":
            entropy = "gpu" if all(_jpeg_has_restarts(s) for s in streams) else "host"
        opts = _native.JpegSplitOpts(int(subseq_bytes or 0), int(max_rounds or 0))
        mode = 2 if split == "subsequence" else (1 if entropy == "gpu" else 0)   # ST_JPEG_ENTROPY_*
        self._check(self._L.st_jpeg_decode_batch_scaled(self._h, bufs, sizes, n, h, w, shape[3], scale, mode, ctypes.byref(opts), to))
        return out

    def decode_png(self, streams, out=None):
        """ImageDecoder op with png = DECODE (st_png_decode_batch): a list of PNG streams (bytes) that decode to one shape ->
        (n, h, w, c) uint8 CUDA tensor, c = 1 (gray), 3 (R, G, B) or 4 (R, G, B, A); lossless, so exactly the stored picture.
        The shape is the first stream's; a stream of another shape, or one that is refused or malformed, raises StError naming
        it, and nothing is written.  Inflate runs on host threads (ST_PNG_THREADS), filter reconstruction and expansion in HIP
        kernels on the current stream.  ``out`` may be any (n, h, w, c) uint8 tensor whose frames are dense, at any address."""
        self._bind()
        streams = [bytes(s) for s in streams]
        n = len(streams)
        if n == 0:
            return torch.zeros((0, 0, 0, 3), dtype=torch.uint8, device=self.device)
        info = probe_png(streams[0])
        shape = (n, info["h"], info["w"], info["channels"])
        out = self._out(out, shape, torch.uint8)
        bufs = _ptr_table(ctypes.cast(ctypes.c_char_p(s), ctypes.c_void_p).value for s in streams)
        sizes = (ctypes.c_size_t * n)(*[len(s) for s in streams])
        to = self._table(out)
        self._check(self._L.st_png_decode_batch(self._h, bufs, sizes, n, shape[1], shape[2], shape[3], to))
        return out

    def last_jpeg_rounds(self):
        """st_jpeg_split_last_rounds: the round launches the last decode_jpeg(split="subsequence") call took (the most over its
        sub-batches; the cap where a segment fell back to the interval decoder)."""
        self._bind()
        return int(self._L.st_jpeg_split_last_rounds(self._h))

    def encode_jpeg(self, frames, quality=95, subsampling="4:2:0", restart="row", optimize=False):
        """ImageEncoder op: (n, h, w, 3) uint8 CUDA frames (a tensor or a list of (h, w, 3) tensors of one shape), R, G, B
        order -> a list of n baseline JPEG streams (bytes), byte for byte what libjpeg writes at this quality and sampling
        with one restart interval per MCU row (restart="row") or without restart markers (restart="none": libjpeg's, Pillow's
        and cv::imencode's default).  Colour conversion, downsampling, DCT, quantisation and Huffman coding run in
        HIP kernels on the current stream; only the streams cross to the host, in one copy.  optimize=True: libjpeg's
        optimize_coding (Pillow's optimize=True) -- each frame's Huffman tables are built from its own symbol counts, on the
        device, and the stream is what libjpeg writes with that switch."""
        hs, vs = jpeg_sampling(subsampling)
        rst = jpeg_restart(restart)
        opt = jpeg_optimize(optimize)
        self._bind()
        fr, n, shape = self._rows(frames, torch.uint8, "frame", 3)
        if n == 0:
            return []
        h, w, _ = shape
        tf = self._table(fr)
        if opt:
            self._check(self._L.st_jpeg_encode_batch_opt(self._h, tf, n, h, w, int(quality), hs, vs, rst, opt))
        else:
            self._check(self._L.st_jpeg_encode_batch_rst(self._h, tf, n, h, w, int(quality), hs, vs, rst))
        sizes = (ctypes.c_size_t * n)()
        self._check(self._L.st_jpeg_encode_fetch(self._h, None, sizes, 0))   # the sizes alone
        most = max(sizes)
        store = np.empty((n, most), np.uint8)
        bufs = _ptr_table(store[i].ctypes.data for i in range(n))
        self._check(self._L.st_jpeg_encode_fetch(self._h, bufs, sizes, most))
        return [store[i, :sizes[i]].tobytes() for i in range(n)]

    def encode_png(self, frames, filter="adaptive"):
        """ImageEncoder op with format = PNG (st_png_encode_batch): (n, h, w, c) uint8 CUDA frames (a tensor or a list of
        (h, w, c) tensors of one shape), c = 1 (gray), 3 (R, G, B) or 4 (R, G, B, A) -> a list of n PNG streams (bytes), lossless,
        byte for byte what png_encode_host writes.  ``filter``: "adaptive" (per row the type with the least sum of
        min(b, 256 - b)) or one of "none", "sub", "up", "average", "paeth" for every row.  Filtering, deflate (runs only, one
        dynamic-Huffman block per 32 768 filtered bytes), the CRCs and the Adler-32 run in HIP kernels on the current stream;
        only the streams cross to the host, in one copy.  A number for ``filter`` is an ST_PNG_FILTER_* value (PNG's filter types
        0..4, adaptive = 5), NOT the argument message's PngFilter enum that sc.ops.ImageEncoder(png_filter=<number>) takes (ADAPTIVE = 0,
        NONE = 1 .. PAETH = 5): 3 is AVERAGE here and UP there.  Names mean the same at both."""
        flt = png_filter(filter)
        self._bind()
        fr, n, shape = self._rows(frames, torch.uint8, "frame")
        if n == 0:
            return []
        h, w, c = shape
        self._check(self._L.st_png_encode_batch(self._h, self._table(fr), n, h, w, c, flt))
        sizes = (ctypes.c_size_t * n)()
        self._check(self._L.st_png_encode_fetch(self._h, None, sizes, 0))   # the sizes alone
        most = max(sizes)
        store = np.empty((n, most), np.uint8)
        bufs = _ptr_table(store[i].ctypes.data for i in range(n))
        self._check(self._L.st_png_encode_fetch(self._h, bufs, sizes, most))
        return [store[i, :sizes[i]].tobytes() for i in range(n)]

    def last_jpeg_symbol_stats(self, n):
        """st_jpeg_encode_fetch_stats: the (n, 4, 256) uint64 symbol counts of the last encode_jpeg(optimize=True) call of n
        frames (tables DC luma, AC luma, DC chroma, AC chroma), as the device counted them."""
        self._bind()
        out = np.empty((int(n), 4, 256), np.uint64)
        self._check(self._L.st_jpeg_encode_fetch_stats(self._h, out.ctypes.data, out.size))
        return out

    # -- pose path (scannertools_caffe) -------------------------------------------------------
    def cpm2_input(self, frames, scale, out=None):
        """CPM2Input (scannertools_caffe_cpp/cpm2_input_kernel_gpu.cpp:104-140): (n,h,w,3) uint8 RGB frames
        -> (n,3,net_h,net_w) float32 network input (planes B,G,R; bicubic resize by ``scale``, padded to
        a multiple of 8 with 128, x/256 - 0.5)."""
        self._bind()
        fr, n, shape = self._rows(frames, torch.uint8, "frame", 3)
        if n == 0:
            return torch.zeros((0, 3, 0, 0), dtype=torch.float32, device=self.device)
        h, w, _ = shape
        _, _, nh, nw = cpm2_geometry(h, w, scale)
        out = self._out(out, (n, 3, nh, nw), torch.float32)
        self._check(self._L.st_cpm2_input_batch(self._h, self._table(fr), n, h, w, float(scale), self._table(out)))
        return out

    # -- network inputs (scannertools_caffe) ----------------------------------------------------
    def facenet_input(self, frames, scale, mean_colors, out=None):
        """FacenetInput (scannertools_caffe_cpp/facenet_input_kernel_cpu.cpp:81-117): (n,h,w,3) uint8 RGB frames (a tensor or a
        list of (h,w,3) tensors) -> (n,3,net_w,net_h) float32: INTER_LINEAR resize to `facenet_geometry(h, w, scale)`, minus
        ``mean_colors[c]`` per channel (frame order R, G, B), every plane transposed."""
        self._bind()
        mean = [float(v) for v in mean_colors]
        if len(mean) != 3:
            raise ValueError("mean_colors must hold 3 values, got %d" % len(mean))
        fr, n, shape = self._rows(frames, torch.uint8, "frame", 3)
        if n == 0:
            return torch.zeros((0, 3, 0, 0), dtype=torch.float32, device=self.device)
        h, w, _ = shape
        nh, nw = facenet_geometry(h, w, scale)
        out = self._out(out, (n, 3, nw, nh), torch.float32)
        self._check(self._L.st_facenet_input_batch(self._h, self._table(fr), n, h, w, float(scale), (ctypes.c_float * 3)(*mean), self._table(out)))
        return out

    def caffe_input(self, frames, input_width, input_height, mean_colors, normalize=False, out=None):
        """CaffeInput (scannertools_caffe_cpp/caffe_input_kernel.cpp:75-138): (n,h,w,3) uint8 RGB frames (a tensor or a list of
        (h,w,3) tensors) -> (n,3,input_height,input_width) float32, planes B, G, R: the reference's box filter, clamped to
        0..255, minus ``mean_colors`` (B, G, R order), divided by 255 when ``normalize``.  ``input_width`` -1: the frame's
        own size.  A geometry with an empty filter window (non-integer enlargements) raises StError (unsupported) and
        nothing is written."""
        self._bind()
        mean = [float(v) for v in mean_colors]
        if len(mean) != 3:
            raise ValueError("mean_colors must hold 3 values, got %d" % len(mean))
        fr, n, shape = self._rows(frames, torch.uint8, "frame", 3)
        if n == 0:
            return torch.zeros((0, 3, 0, 0), dtype=torch.float32, device=self.device)
        h, w, _ = shape
        nw, nh = (w, h) if int(input_width) == -1 else (int(input_width), int(input_height))
        out = self._out(out, (n, 3, nh, nw), torch.float32)
        self._check(self._L.st_caffe_input_batch(self._h, self._table(fr), n, h, w, nh, nw, (ctypes.c_float * 3)(*mean), int(bool(normalize)),
                                                 self._table(out)))
        return out

    # -- FacenetOutput (scannertools_caffe) -----------------------------------------------------
    def facenet_output(self, maps, h, w, scale, templates, threshold, overlap=0.1, offset=0.0):
        """FacenetOutput (scannertools_caffe_cpp/facenet_output_kernel_cpu.cpp:72-163; st_facenet_output_batch): the Facenet
        op's maps of frames of (h, w) at ``scale`` -> per frame a float32 numpy array (kept, 5) of rows
        [x1, y1, x2, y2, score], normalised coordinates, descending score.  maps: a CUDA float32 tensor (n, 125, grid_w,
        grid_h) or a list of contiguous tensors of 125 * grid_w * grid_h values each; templates: the 25 x 4 floats of the
        templates file; overlap / offset: best_nms's threshold and the formula's pixel offset (the op passes 0.1 and 0)."""
        self._bind()
        tpl = np.ascontiguousarray(np.asarray(templates, dtype=np.float32).reshape(-1))
        if tpl.size != 100:
            raise ValueError("templates must hold 25 x 4 values, got %d" % tpl.size)
        nh, nw = facenet_geometry(h, w, scale)
        cells = 125 * ((nw + 7) // 8) * ((nh + 7) // 8)
        fr, n, _ = self._rows(maps, torch.float32, "map", shaped=False)
        for f in fr:
            if f.numel() != cells:
                raise ValueError("a map of a %dx%d frame at scale %g holds 125 x %d x %d values, got %d"
                                 % (w, h, scale, (nw + 7) // 8, (nh + 7) // 8, f.numel()))
        counts = (ctypes.c_int32 * max(n, 1))()
        self._check(self._L.st_facenet_output_batch(self._h, self._table(fr), n, int(h), int(w), float(scale), tpl.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                    float(threshold), float(overlap), float(offset), counts))
        counts = [int(c) for c in counts[:n]]
        rows = np.empty((sum(counts), 5), np.float32)
        self._check(self._L.st_facenet_output_fetch(self._h, rows.ctypes.data_as(ctypes.c_void_p), rows.shape[0]))
        return np.split(rows, np.cumsum(counts)[:-1]) if n else []

    def bbox_nms(self, rows, counts=None, overlap=0.1, offset=0.0):
        """Greedy non-maximum suppression (st_bbox_nms_f32) of sets of boxes.  rows: CUDA float32
        (total, 5) [x1, y1, x2, y2, score], set after set; counts: the rows of each set (None: one set).  Returns per set
        the int32 numpy array of the kept boxes' row indices within the set, in kept order (descending score, equal scores
        by ascending index)."""
        self._bind()
        _require_cuda(rows, torch.float32, "rows", self.device)
        if rows.dim() != 2 or rows.shape[1] != 5:
            raise ValueError("rows must be (total, 5)")
        counts = [int(rows.shape[0])] if counts is None else [int(c) for c in counts]
        if any(c < 0 for c in counts) or sum(counts) != rows.shape[0]:
            raise ValueError("counts %s do not add up to the %d rows" % (counts, rows.shape[0]))
        n = len(counts)
        kept = torch.empty((max(int(rows.shape[0]), 1),), dtype=torch.int32, device=self.device)
        kc = (ctypes.c_int32 * max(n, 1))()
        self._check(self._L.st_bbox_nms_f32(self._h, ctypes.c_void_p(rows.data_ptr()), (ctypes.c_int32 * max(n, 1))(*counts), n, float(overlap),
                                            float(offset), ctypes.c_void_p(kept.data_ptr()), kc))
        kept = kept.cpu().numpy()
        first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return [kept[first[i]:first[i] + kc[i]].copy() for i in range(n)]

    def cpm2_limb_scores(self, heatmaps, peaks, inter_threshold=0.05, min_above=9):
        """Candidate-pair scores of CPM2Output (cpm2_output_kernel_cpu.cpp:424-487): heatmaps
        (n,57,H,W) float32, peaks (n,18,max_peaks+1,3) float32 -> (n,19,max_peaks,max_peaks) float32."""
        self._bind()
        _require_cuda(heatmaps, torch.float32, "heatmaps", self.device)
        _require_cuda(peaks, torch.float32, "peaks", self.device)
        n, c, H, W = heatmaps.shape
        if c != 57 or peaks.dim() != 4 or peaks.shape[0] != n or peaks.shape[1] != 18 or peaks.shape[3] != 3:
            raise ValueError("heatmaps must be (n,57,H,W) and peaks (n,18,max_peaks+1,3)")
        mp = peaks.shape[2] - 1
        out = torch.empty((n, 19, mp, mp), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        self._check(self._L.st_cpm2_limb_scores(self._h, self._table(heatmaps), self._table(peaks), n, H, W, mp, float(inter_threshold),
                                                int(min_above), ctypes.c_void_p(out.data_ptr())))
        return out

    def cpm2_resize_maps(self, maps, dst_h, dst_w, chan_map=None, nmaps=None, out=None):
        """The CPM2 network's `resize` layer (cpm2_kernel.cpp:16-23 configures it; [EXT] Caffe fork): maps
        (n,h,w,C) channel-last float32 -> (n,nmaps,dst_h,dst_w) planar float32, bicubic; output plane c reads
        channel chan_map[c] (default: the first nmaps channels)."""
        self._bind()
        _require_cuda(maps, torch.float32, "maps", self.device)
        if maps.dim() != 4:
            raise ValueError("maps must be (n,h,w,C)")
        n, h, w, C = maps.shape
        if chan_map is not None:
            nmaps = len(chan_map)
        elif nmaps is None:
            nmaps = C
        shape = (n, nmaps, int(dst_h), int(dst_w))
        out = self._out(out, shape, torch.float32)
        if n == 0:
            return out
        cm = (ctypes.c_int * nmaps)(*[int(v) for v in chan_map]) if chan_map is not None else None
        self._check(self._L.st_cpm2_resize_maps(self._h, ctypes.c_void_p(maps.data_ptr()), n, h, w, C, cm, nmaps, int(dst_h), int(dst_w),
                                                self._table(out)))
        return out

    def cpm2_resize_merge_maps(self, maps_list, eff_sizes, dst_h, dst_w, chan_map=None, nmaps=None):
        """Maps of several network scales merged (st_cpm2_resize_merge_maps): maps_list[s] (n,h_s,w_s,C) float32 channel-last,
        eff_sizes[s] = (eff_h, eff_w) source pixels of scale s that span the whole output -> (n,nmaps,dst_h,dst_w)."""
        self._bind()
        S = len(maps_list)
        for m in maps_list:
            _require_cuda(m, torch.float32, "maps", self.device)
        n, _, _, C = maps_list[0].shape
        if any(m.dim() != 4 or m.shape[0] != n or m.shape[3] != C for m in maps_list) or len(eff_sizes) != S:
            raise ValueError("every scale needs (n,h,w,C) maps with the same n and C, and one (eff_h, eff_w) pair")
        if chan_map is not None:
            nmaps = len(chan_map)
        elif nmaps is None:
            nmaps = C
        out = torch.empty((n, nmaps, int(dst_h), int(dst_w)), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        cm = (ctypes.c_int * nmaps)(*[int(v) for v in chan_map]) if chan_map is not None else None
        src = self._table(maps_list)
        sh = (ctypes.c_int * S)(*[m.shape[1] for m in maps_list])
        sw = (ctypes.c_int * S)(*[m.shape[2] for m in maps_list])
        eh = (ctypes.c_float * S)(*[float(e[0]) for e in eff_sizes])
        ew = (ctypes.c_float * S)(*[float(e[1]) for e in eff_sizes])
        self._check(self._L.st_cpm2_resize_merge_maps(self._h, src, sh, sw, eh, ew, S, n, C, cm, nmaps, int(dst_h), int(dst_w), self._table(out)))
        return out

    def cpm2_nms(self, maps, parts=18, max_peaks=64, threshold=0.05, out=None):
        """The CPM2 network's `nms` layer ([EXT] Caffe fork): maps (n,>=parts,H,W) float32 -> joints
        (n,parts,max_peaks+1,3) float32, row 0 = [count,0,0], rows 1.. = (x, y, score) in raster order."""
        self._bind()
        _require_cuda(maps, torch.float32, "maps", self.device)
        if maps.dim() != 4 or maps.shape[1] < parts:
            raise ValueError("maps must be (n,>=parts,H,W)")
        n, _, H, W = maps.shape
        shape = (n, parts, max_peaks + 1, 3)
        out = self._out(out, shape, torch.float32)
        if n == 0:
            return out
        self._check(self._L.st_cpm2_nms(self._h, self._table(maps), n, H, W, int(parts), int(max_peaks), float(threshold), self._table(out)))
        return out

    # -- OpticalFlow ------------------------------------------------------------------------
    # -- layers of a generic Caffe network (st_nn.hip); activations are NHWC float32 (n, h, w, channel stride) ----------
    @staticmethod
    def _vp(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def _nhwc(self, x, name="x"):
        _require_cuda(x, torch.float32, name, self.device)
        if x.dim() != 4:
            raise ValueError("%s must be (n, h, w, channels)" % name)
        return x.shape

    def _nhwc_out(self, out, n, oh, ow, c, y_offset):
        if out is None:
            return torch.zeros((n, oh, ow, (c + y_offset + 15) // 16 * 16), dtype=torch.float32, device=self.device)
        _require_cuda(out, torch.float32, "out", self.device)
        if out.dim() != 4 or tuple(out.shape[:3]) != (n, oh, ow):
            raise ValueError("out must be (%d, %d, %d, channels), got %s" % (n, oh, ow, tuple(out.shape)))
        return out

    def inner_product_pack(self, w):
        """The InnerProduct weights (nout, k) float32, k a multiple of 8, in the kernel's operand order (a uint8 tensor)."""
        _require_cuda(w, torch.float32, "w", self.device)
        nout, k = w.shape
        nb = self._L.st_inner_product_packed_bytes(k, nout)
        if nb <= 0:
            raise ValueError("inner_product: k must be a positive multiple of 8, got (%d, %d)" % (nout, k))
        packed = torch.empty((nb,), dtype=torch.uint8, device=self.device)
        self._bind()
        self._check(self._L.st_inner_product_pack_weights(self._h, self._vp(w), k, nout, self._vp(packed)))
        return packed

    def inner_product(self, x, packed, nout, bias=None, relu=False, out=None):
        """y = x (n, k) . W^T (+ bias) (+ ReLU) with W packed by inner_product_pack; out: (n, >= nout), columns past nout untouched."""
        _require_cuda(x, torch.float32, "x", self.device)
        n, k = x.shape
        if out is None:
            out = torch.zeros((n, nout), dtype=torch.float32, device=self.device)
        _require_cuda(out, torch.float32, "out", self.device)
        self._bind()
        self._check(self._L.st_inner_product_f32(self._h, self._vp(x), n, k, k, self._vp(packed), self._vp(bias), nout, int(relu),
                                                 self._vp(out), out.shape[1]))
        return out

    def conv2d_general(self, x, cin, w, bias, stride=1, pad=0, group=1, relu=False, x_offset=0, out=None, y_offset=0):
        """Convolution of any geometry; w: (cout, k, k, cin / group)."""
        n, h, wd, xs = self._nhwc(x)
        _require_cuda(w, torch.float32, "w", self.device)
        cout, k = w.shape[0], w.shape[1]
        oh, ow = self._L.st_conv_out_size(h, k, stride, pad), self._L.st_conv_out_size(wd, k, stride, pad)
        out = self._nhwc_out(out, n, oh, ow, cout, y_offset)
        self._bind()
        self._check(self._L.st_conv2d_general_nhwc_f32(self._h, self._vp(x), n, h, wd, cin, xs, x_offset, self._vp(w), self._vp(bias), k, stride, pad,
                                                       group, cout, int(relu), self._vp(out), out.shape[3], y_offset))
        return out

    def pool(self, x, c, method, kernel_size=0, stride=1, pad=0, global_pooling=False, x_offset=0, out=None, y_offset=0):
        """Caffe's Pooling: method _native.POOL_MAX / POOL_AVE."""
        n, h, wd, xs = self._nhwc(x)
        oh = 1 if global_pooling else self._L.st_pool_out_size(h, kernel_size, stride, pad)
        ow = 1 if global_pooling else self._L.st_pool_out_size(wd, kernel_size, stride, pad)
        out = self._nhwc_out(out, n, oh, ow, c, y_offset)
        self._bind()
        self._check(self._L.st_pool_nhwc_f32(self._h, self._vp(x), n, h, wd, c, xs, x_offset, method, kernel_size, stride, pad, int(global_pooling),
                                             self._vp(out), out.shape[3], y_offset))
        return out

    def lrn(self, x, c, local_size=5, alpha=1.0, beta=0.75, k=1.0, x_offset=0, out=None, y_offset=0):
        n, h, wd, xs = self._nhwc(x)
        out = self._nhwc_out(out, n, h, wd, c, y_offset)
        self._bind()
        self._check(self._L.st_lrn_nhwc_f32(self._h, self._vp(x), n * h * wd, c, xs, x_offset, local_size, alpha, beta, k, self._vp(out), out.shape[3],
                                            y_offset))
        return out

    def softmax(self, x, c, x_offset=0, out=None, y_offset=0):
        n, h, wd, xs = self._nhwc(x)
        out = self._nhwc_out(out, n, h, wd, c, y_offset)
        self._bind()
        self._check(self._L.st_softmax_nhwc_f32(self._h, self._vp(x), n * h * wd, c, xs, x_offset, self._vp(out), out.shape[3], y_offset))
        return out

    def copy_channels(self, x, c, x_offset, out, y_offset, relu=False):
        n, h, wd, xs = self._nhwc(x)
        out = self._nhwc_out(out, n, h, wd, c, y_offset)
        self._bind()
        self._check(self._L.st_copy_channels_nhwc_f32(self._h, self._vp(x), n * h * wd, c, xs, x_offset, int(relu), self._vp(out), out.shape[3], y_offset))
        return out

    def nhwc_to_planar(self, x, c, x_offset=0):
        """(n, h, w, stride) -> (n, c, h, w), every frame through its own pointer as the Caffe op writes its output frames."""
        n, h, wd, xs = self._nhwc(x)
        out = torch.empty((n, c, h, wd), dtype=torch.float32, device=self.device)
        self._bind()
        self._check(self._L.st_nhwc_to_planar_f32(self._h, self._vp(x), n, h, wd, c, xs, x_offset, self._table(out)))
        return out

    def optical_flow(self, frames, pairs=None, params=None, out=None):
        """Farneback flow for a batch of frame pairs.

        frames: CUDA uint8 (n,h,w,3) tensor or list of (h,w,3) tensors.  pairs: (p,2) int
        array-like of indices; default = consecutive pairs (i, i+1), i.e. stencil {0,1} over a
        contiguous run (optical_flow_kernel_cpu.cpp:51-54).  Flow p goes from frame pairs[p][0]
        to frame pairs[p][1].  Returns float32 (p,h,w,2)."""
        self._bind()
        if isinstance(frames, (list, tuple)):
            fl = list(frames)
        else:
            _require_cuda(frames, torch.uint8, "frames", self.device)
            if frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError("frames must be (n,h,w,3)")
            fl = [frames[i] for i in range(frames.shape[0])]
        n = len(fl)
        for f in fl:
            _require_cuda(f, torch.uint8, "frame", self.device)
        if n:
            h, w, _ = fl[0].shape
            if any(tuple(f.shape) != (h, w, 3) for f in fl):
                raise ValueError("all frames must be (h,w,3) with equal shape")
        if pairs is None:
            pairs = [(i, i + 1) for i in range(max(n - 1, 0))]
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
        p = len(pairs)
        if n == 0:
            if p:
                raise ValueError("pairs given but no frames")
            return torch.zeros((0, 0, 0, 2), dtype=torch.float32, device=self.device)
        out = self._out(out, (p, h, w, 2), torch.float32)
        if p == 0:
            return out
        prm = params if params is not None else default_params()
        self._check(self._L.st_farneback_pairs(
            self._h, self._table(fl), n, pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), p, h, w, ctypes.byref(prm), self._table(out)))
        return out

    # -- stage-level entry points (used by the parity tests) ----------------------------------
    def gray(self, rgb, bits=15):
        self._bind()
        _require_cuda(rgb, torch.uint8, "rgb", self.device)
        h, w, _ = rgb.shape
        out = torch.empty((h, w), dtype=torch.uint8, device=self.device)
        self._check(self._L.st_gray_u8(self._h, ctypes.c_void_p(rgb.data_ptr()), h, w, bits,
                                       ctypes.c_void_p(out.data_ptr())))
        return out

    def pyr_image(self, gray, level, params=None):
        self._bind()
        _require_cuda(gray, torch.uint8, "gray", self.device)
        prm = params if params is not None else default_params()
        h, w = gray.shape
        lh, lw = ctypes.c_int(), ctypes.c_int()
        self._check(self._L.st_fb_level_geom(h, w, ctypes.byref(prm), level, ctypes.byref(lh), ctypes.byref(lw),
                                             None, None))
        out = torch.empty((lh.value, lw.value), dtype=torch.float32, device=self.device)
        self._check(self._L.st_fb_pyr_image(self._h, ctypes.c_void_p(gray.data_ptr()), h, w, ctypes.byref(prm), level,
                                            ctypes.c_void_p(out.data_ptr())))
        return out

    def polyexp(self, img, poly_n=5, poly_sigma=1.2):
        """(h,w) f32 -> R (h,w,5) f32, OpenCV's interleaved layout (unpacked from the device layout)."""
        self._bind()
        _require_cuda(img, torch.float32, "img", self.device)
        h, w = img.shape
        out = torch.empty(5 * h * w, dtype=torch.float32, device=self.device)
        self._check(self._L.st_fb_polyexp(self._h, ctypes.c_void_p(img.data_ptr()), h, w, poly_n, poly_sigma,
                                          ctypes.c_void_p(out.data_ptr())))
        return unpack_r(out, h, w)

    def update_matrices(self, r0, r1, flow=None, coarse_flow=None, pyr_scale=0.5):
        """R0,R1 (h,w,5) (+ flow (h,w,2) or coarse flow (ch,cw,2)) -> planar M (5,h,w)."""
        self._bind()
        _require_cuda(r0, torch.float32, "r0", self.device)
        _require_cuda(r1, torch.float32, "r1", self.device)
        h, w, _ = r0.shape
        r0, r1 = pack_r(r0), pack_r(r1)
        out = torch.empty((5, h, w), dtype=torch.float32, device=self.device)
        fp = cp = None
        ch = cw = 0
        if coarse_flow is not None:
            _require_cuda(coarse_flow, torch.float32, "coarse_flow", self.device)
            ch, cw, _ = coarse_flow.shape
            cp = ctypes.c_void_p(coarse_flow.data_ptr())
        elif flow is not None:
            _require_cuda(flow, torch.float32, "flow", self.device)
            fp = ctypes.c_void_p(flow.data_ptr())
        self._check(self._L.st_fb_update_matrices(self._h, ctypes.c_void_p(r0.data_ptr()), ctypes.c_void_p(r1.data_ptr()),
                                                  fp, cp, ch, cw, pyr_scale, h, w, ctypes.c_void_p(out.data_ptr())))
        return out

    def update_flow_blur(self, r0, r1, m, block_size=15, update=True):
        """One FarnebackUpdateFlow_Blur pass over planar M (5,h,w) (R0, R1: (h,w,5), needed when
        update=True).  Returns (flow (h,w,2), M' (5,h,w) or None)."""
        self._bind()
        _require_cuda(m, torch.float32, "m", self.device)
        _, h, w = m.shape
        r0 = pack_r(r0) if r0 is not None else None
        r1 = pack_r(r1) if r1 is not None else None
        flow = torch.empty((h, w, 2), dtype=torch.float32, device=self.device)
        mout = torch.empty_like(m) if update else None
        self._check(self._L.st_fb_update_flow_blur(
            self._h, ctypes.c_void_p(r0.data_ptr()) if r0 is not None else None,
            ctypes.c_void_p(r1.data_ptr()) if r1 is not None else None, ctypes.c_void_p(m.data_ptr()), h, w,
            block_size, 1 if update else 0, ctypes.c_void_p(flow.data_ptr()),
            ctypes.c_void_p(mout.data_ptr()) if update else None))
        return flow, mout


    def flow_iteration(self, r0, r1, flow_in=None, coarse_flow=None, pyr_scale=0.5, block_size=15):
        """One fused iteration (UpdateMatrices + box blur + solve) as the production path runs it."""
        self._bind()
        _require_cuda(r0, torch.float32, "r0", self.device)
        _require_cuda(r1, torch.float32, "r1", self.device)
        h, w, _ = r0.shape
        r0, r1 = pack_r(r0), pack_r(r1)
        out = torch.empty((h, w, 2), dtype=torch.float32, device=self.device)
        fp = cp = None
        ch = cw = 0
        if coarse_flow is not None:
            _require_cuda(coarse_flow, torch.float32, "coarse_flow", self.device)
            ch, cw, _ = coarse_flow.shape
            cp = ctypes.c_void_p(coarse_flow.data_ptr())
        elif flow_in is not None:
            _require_cuda(flow_in, torch.float32, "flow_in", self.device)
            fp = ctypes.c_void_p(flow_in.data_ptr())
        self._check(self._L.st_fb_flow_iteration(self._h, ctypes.c_void_p(r0.data_ptr()), ctypes.c_void_p(r1.data_ptr()),
                                                 fp, cp, ch, cw, pyr_scale, h, w, block_size,
                                                 ctypes.c_void_p(out.data_ptr())))
        return out


def pack_r(r):
    """(h,w,5) polynomial expansion -> the device layout of the st_fb_* stage entry points:
    h*w float4 (channels 0..3) followed by h*w floats (channel 4)."""
    return torch.cat([r[..., :4].reshape(-1), r[..., 4].reshape(-1)]).contiguous()


def unpack_r(flat, h, w):
    """Inverse of :func:`pack_r`."""
    n = h * w
    return torch.cat([flat[:4 * n].view(h, w, 4), flat[4 * n:].view(h, w, 1)], dim=2).contiguous()


def probe_jpeg(stream):
    """st_jpeg_probe (host only): {'h', 'w', 'channels', 'h_samp', 'v_samp', 'restart_interval'} of a baseline JPEG stream;
    StError with the library's message for a stream that is refused or malformed."""
    info = _native.JpegInfo()
    data = bytes(stream)
    st = _native.lib().st_jpeg_probe(data, len(data), ctypes.byref(info))
    if st != 0:
        raise StError(st, info.message.decode())
    return {k: getattr(info, k) for k in ("h", "w", "channels", "h_samp", "v_samp", "restart_interval")}


_PNG_INFO_KEYS = ("h", "w", "channels", "color_type", "bit_depth", "interlace", "palette_entries", "trns_entries")


def probe_png(stream):
    """st_png_probe (host only): {'h', 'w', 'channels', 'color_type', 'bit_depth', 'interlace', 'palette_entries',
    'trns_entries'} of a PNG stream, read from its chunks up to the first IDAT (h, w, channels: of the decoded frame); StError
    with the library's message for a stream that is refused or malformed."""
    info = _native.PngInfo()
    data = bytes(stream)
    st = _native.lib().st_png_probe(data, len(data), ctypes.byref(info))
    if st != 0:
        raise StError(st, info.message.decode())
    return {k: getattr(info, k) for k in _PNG_INFO_KEYS}


def zlib_inflate(data, size):
    """st_zlib_inflate (host only): the library's own inflater on one zlib stream, into a buffer of exactly ``size`` bytes;
    returns the bytes produced (there may be fewer than ``size``).  StError with the cause for a malformed stream or one that
    produces more than ``size`` bytes."""
    data = bytes(data)
    out = np.empty(max(int(size), 1), np.uint8)
    produced = ctypes.c_size_t(0)
    msg = ctypes.create_string_buffer(160)
    st = _native.lib().st_zlib_inflate(data, len(data), out.ctypes.data, int(size), ctypes.byref(produced), msg, 160)
    if st != 0:
        raise StError(st, msg.value.decode())
    return out[:produced.value].tobytes()


def png_filtered(stream):
    """st_png_filtered (host only): stage 1 alone, the (h, 1 + rowbytes) uint8 array of the stream's inflated scanlines, every
    row its filter type and its still-filtered bytes."""
    data = bytes(stream)
    info = _native.PngInfo()
    st = _native.lib().st_png_probe(data, len(data), ctypes.byref(info))
    if st != 0:
        raise StError(st, info.message.decode())
    samples = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[info.color_type]
    rowbytes = (info.w * samples * info.bit_depth + 7) // 8
    raw = np.empty((info.h, 1 + rowbytes), np.uint8)
    st = _native.lib().st_png_filtered(data, len(data), raw.ctypes.data, raw.size, ctypes.byref(info))
    if st != 0:
        raise StError(st, info.message.decode())
    return raw


def png_decode_host(stream):
    """st_png_decode_host (host only): the (h, w, c) uint8 frame of a PNG stream, decoded in plain C++ the way the device
    computes it (the CPU twin of decode_png's kernels)."""
    data = bytes(stream)
    info = _native.PngInfo()
    st = _native.lib().st_png_probe(data, len(data), ctypes.byref(info))
    if st != 0:
        raise StError(st, info.message.decode())
    frame = np.empty((info.h, info.w, info.channels), np.uint8)
    st = _native.lib().st_png_decode_host(data, len(data), frame.ctypes.data, frame.size, ctypes.byref(info))
    if st != 0:
        raise StError(st, info.message.decode())
    return frame


PNG_FILTERS = ("none", "sub", "up", "average", "paeth", "adaptive")   # encode_png's filter=; ImageEncoderArgs.png_filter, ST_PNG_FILTER_*


def png_filter(filter):
    """The ST_PNG_FILTER_* value of a filter name (or of the value itself: none = 0 .. paeth = 4 as in PNG, adaptive = 5 -- not the
    numbering of ImageEncoderArgs.png_filter, where ADAPTIVE is 0); ValueError for anything else."""
    if isinstance(filter, str) and filter.lower() in PNG_FILTERS:
        return PNG_FILTERS.index(filter.lower())
    if isinstance(filter, int) and not isinstance(filter, bool) and 0 <= filter < len(PNG_FILTERS):
        return filter
    raise ValueError("png filter must be one of %s, got %r" % (", ".join(PNG_FILTERS), filter))


def _png_encode_refusal(h, w, c, flt):
    msg = ctypes.create_string_buffer(160)
    st = _native.lib().st_png_encode_check(int(h), int(w), int(c), int(flt), msg, 160)
    return st, msg.value.decode()


def png_encode_bound(h, w, c):
    """st_png_encode_bound (host only): no PNG stream of an (h, w, c) frame is longer, whatever its content and filter."""
    v = _native.lib().st_png_encode_bound(int(h), int(w), int(c))
    if v < 0:
        raise StError(*_png_encode_refusal(h, w, c, 5))
    return v


def png_encode_host(frame, filter="adaptive"):
    """st_png_encode_host (host only): the PNG stream of one (h, w, c) or (h, w) uint8 host frame in plain C++, byte for byte
    what encode_png writes for it (the CPU twin of its kernels)."""
    flt = png_filter(filter)
    f = np.ascontiguousarray(frame, np.uint8)
    if f.ndim == 2:
        f = f[:, :, None]
    if f.ndim != 3:
        raise ValueError("png_encode_host takes an (h, w, c) frame, got shape %s" % (f.shape,))
    h, w, c = f.shape
    st, msg = _png_encode_refusal(h, w, c, flt)
    if st != 0:
        raise StError(st, "png_encode: " + msg)
    cap = png_encode_bound(h, w, c)
    buf, size = np.empty(cap, np.uint8), ctypes.c_size_t()
    st = _native.lib().st_png_encode_host(f.ctypes.data, h, w, c, flt, buf.ctypes.data, cap, ctypes.byref(size))
    if st != 0:
        raise StError(st, "st_png_encode_host(h=%d, w=%d, c=%d)" % (h, w, c))
    return buf[:size.value].tobytes()


def png_huff_limited(counts, limit):
    """st_png_huff_limited (host only): the code lengths (uint8, 0: no code) the PNG encoder's length-limited construction
    gives a histogram of 2..286 counts at ``limit`` bits (15: literal/length codes, 7: the code-length code)."""
    f = np.ascontiguousarray(counts, np.uint32)
    out = np.zeros(f.shape, np.uint8)
    st = _native.lib().st_png_huff_limited(f.ctypes.data, f.size, int(limit), out.ctypes.data) if f.ndim == 1 else 1
    if st != 0:
        raise StError(st, "st_png_huff_limited(%d symbols, limit %r): 2..286 symbols, limit 1..15 with 2^limit >= symbols, counts below 2^32 in all" % (f.size, limit))
    return out


JPEG_ENTROPY_MODES = ("host", "gpu", "auto")   # decode_jpeg's entropy=; ImageDecoderArgs.entropy HOST = 0, GPU = 1, AUTO = 2
JPEG_ENTROPY_SPLITS = ("interval", "subsequence")   # decode_jpeg's split=; ImageDecoderArgs.split INTERVAL = 0, SUBSEQUENCE = 1


JPEG_SCALES = (1, 2, 4, 8)   # decode_jpeg's scale=; ImageDecoderArgs.scale_denom (0 or absent: 1)


def jpeg_scaled_size(h, w, scale):
    """st_jpeg_scaled_size (host only): (ceil(h / scale), ceil(w / scale)), the frame decode_jpeg(scale=scale) writes for an
    (h, w) stream.  ValueError: a scale other than 1, 2, 4 or 8, or a size outside 1..65535."""
    oh, ow = ctypes.c_int(0), ctypes.c_int(0)
    if isinstance(scale, bool) or scale not in JPEG_SCALES or _native.lib().st_jpeg_scaled_size(int(h), int(w), int(scale), ctypes.byref(oh), ctypes.byref(ow)) != 0:
        raise ValueError("jpeg_scaled_size(h=%r, w=%r, scale=%r): scale must be 1, 2, 4 or 8 and the size within 1..65535" % (h, w, scale))
    return oh.value, ow.value


def jpeg_scaled_geometry(stream, scale):
    """st_jpeg_scaled_geometry (host only): per component of the stream its inverse DCT size and the extent of its reduced
    plane at 1 / scale, as {'S': [...], 'dw': [...], 'dh': [...]} (one entry per channel).  Raises StError on a stream
    st_jpeg_probe refuses or a scale other than 1, 2, 4 or 8."""
    data = bytes(stream)
    info = _native.JpegInfo()
    S, dw, dh = (ctypes.c_int * 3)(), (ctypes.c_int * 3)(), (ctypes.c_int * 3)()
    st = _native.lib().st_jpeg_scaled_geometry(data, len(data), int(scale), S, dw, dh, ctypes.byref(info))
    if st != 0:
        raise StError(st, info.message.decode(errors="replace"))
    c = info.channels
    return {"S": list(S)[:c], "dw": list(dw)[:c], "dh": list(dh)[:c]}


def _jpeg_has_restarts(data):
    """True when the stream's probe succeeds and reports restart_interval > 0 (a refused stream is left to the decoding call)."""
    info = _native.JpegInfo()
    return _native.lib().st_jpeg_probe(data, len(data), ctypes.byref(info)) == 0 and info.restart_interval > 0


def jpeg_restart_intervals(stream):
    """st_jpeg_restart_intervals (host only): the (n, 2) uint32 array of (begin, end) byte offsets of the stream's restart
    intervals; StError for a stream without DRI (ST_ERR_UNSUPPORTED) or with a broken scan (ST_ERR_INVALID)."""
    data = bytes(stream)
    info = _native.JpegInfo()
    count = ctypes.c_size_t(0)
    st = _native.lib().st_jpeg_restart_intervals(data, len(data), None, 0, ctypes.byref(count), ctypes.byref(info))
    if st != 0:
        raise StError(st, info.message.decode())
    table = np.empty((count.value, 2), np.uint32)
    st = _native.lib().st_jpeg_restart_intervals(data, len(data), table.ctypes.data, count.value, ctypes.byref(count), ctypes.byref(info))
    if st != 0:
        raise StError(st, info.message.decode())
    return table


def jpeg_coefficients(stream, by_interval=False, by_subsequence=False, subseq_bytes=None, max_rounds=None):
    """st_jpeg_coefficients (host only): (int16 coefficients in the layout the header documents, (channels, 64) uint16
    quantisation tables in natural order) of a baseline JPEG stream.  by_interval=True: st_jpeg_coefficients_by_interval, the
    same result computed restart interval by restart interval with the core the device kernel runs.  by_subsequence=True:
    st_jpeg_coefficients_by_subsequence, the same result by the iteration over subsequences of ``subseq_bytes`` bytes capped at
    ``max_rounds`` rounds (None: the library's defaults); the return value is then (coefficients, tables, rounds)."""
    data = bytes(stream)
    info = probe_jpeg(data)
    H, V = info["h_samp"], info["v_samp"]
    mcux, mcuy = -(-info["w"] // (8 * H)), -(-info["h"] // (8 * V))
    blocks = mcux * mcuy * (H * V + 2) if info["channels"] == 3 else mcux * mcuy
    coef = np.empty(blocks * 64, np.int16)
    quant = np.empty((info["channels"], 64), np.uint16)
    ji = _native.JpegInfo()
    if by_subsequence:
        opts, rounds = _native.JpegSplitOpts(int(subseq_bytes or 0), int(max_rounds or 0)), ctypes.c_int(0)
        st = _native.lib().st_jpeg_coefficients_by_subsequence(data, len(data), ctypes.byref(opts), coef.ctypes.data, coef.size, quant.ctypes.data,
                                                               ctypes.byref(ji), ctypes.byref(rounds))
        if st != 0:
            raise StError(st, ji.message.decode())
        return coef, quant, rounds.value
    fn = _native.lib().st_jpeg_coefficients_by_interval if by_interval else _native.lib().st_jpeg_coefficients
    st = fn(data, len(data), coef.ctypes.data, coef.size, quant.ctypes.data, ctypes.byref(ji))
    if st != 0:
        raise StError(st, ji.message.decode())
    return coef, quant


JPEG_SUBSAMPLINGS = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}   # name -> luma sampling (h_samp, v_samp)


def jpeg_sampling(subsampling):
    """(h_samp, v_samp) of "4:4:4" / "4:2:2" / "4:2:0"; ValueError for anything else."""
    if subsampling not in JPEG_SUBSAMPLINGS:
        raise ValueError("subsampling %r is not supported (4:4:4, 4:2:2 or 4:2:0)" % (subsampling,))
    return JPEG_SUBSAMPLINGS[subsampling]


JPEG_RESTARTS = {"row": 0, "none": 1}   # name -> ST_JPEG_RESTART_ROW / ST_JPEG_RESTART_NONE


def jpeg_restart(restart):
    """ST_JPEG_RESTART_* of "row" (one restart interval per MCU row) / "none" (no restart markers); ValueError for anything else."""
    if not isinstance(restart, str) or restart not in JPEG_RESTARTS:
        raise ValueError("restart %r is not supported ('row' or 'none')" % (restart,))
    return JPEG_RESTARTS[restart]


def jpeg_optimize(optimize):
    """0 / 1 of False / True / 0 / 1; ValueError for anything else."""
    if isinstance(optimize, (bool, int, np.integer)) and int(optimize) in (0, 1):
        return int(optimize)
    raise ValueError("optimize %r is not supported (False or True)" % (optimize,))


def jpeg_optimal_table(freq):
    """st_jpeg_optimal_table (host only): (bits, vals) of libjpeg's jpeg_gen_optimal_table for 256 symbol counts: bits[k] the
    codes of k + 1 bits as a (16,) uint8 array, vals the symbols that have a code, by code length and then by value."""
    f = np.ascontiguousarray(freq, np.uint64)
    if f.shape != (256,):
        raise ValueError("jpeg_optimal_table takes 256 counts, got shape %s" % (f.shape,))
    bits, vals, n = np.zeros(16, np.uint8), np.zeros(256, np.uint8), ctypes.c_int()
    st = _native.lib().st_jpeg_optimal_table(f.ctypes.data, bits.ctypes.data, vals.ctypes.data, ctypes.byref(n))
    if st != 0:
        raise StError(st, "st_jpeg_optimal_table")
    return bits, vals[:n.value].copy()


def jpeg_optimal_dht(freq, table):
    """st_jpeg_optimal_dht (host only): (the DHT segment's bytes, the code words (length << 16 | code) by symbol) of the table
    built from 256 counts, as table 0 DC luma, 1 AC luma, 2 DC chroma or 3 AC chroma."""
    f = np.ascontiguousarray(freq, np.uint64)
    if f.shape != (256,):
        raise ValueError("jpeg_optimal_dht takes 256 counts, got shape %s" % (f.shape,))
    buf, size = ctypes.create_string_buffer(21 + 256), ctypes.c_size_t()
    codes = np.zeros(256 if int(table) & 1 else 16, np.uint32)
    st = _native.lib().st_jpeg_optimal_dht(f.ctypes.data, int(table), buf, len(buf), ctypes.byref(size), codes.ctypes.data)
    if st != 0:
        raise StError(st, "st_jpeg_optimal_dht(table=%r): tables are 0..3" % (table,))
    return buf.raw[:size.value], codes


def jpeg_symbol_stats(coef, h, w, subsampling="4:2:0", restart="row"):
    """st_jpeg_symbol_stats (host only): the (4, 256) uint64 symbol counts (DC luma, AC luma, DC chroma, AC chroma) of an
    (h, w, 3) frame's int16 coefficients in jpeg_coefficients' layout, the DC predictors as the restart mode has them."""
    hs, vs = jpeg_sampling(subsampling)
    rst = jpeg_restart(restart)
    c = np.ascontiguousarray(coef, np.int16).reshape(-1)
    out = np.zeros((4, 256), np.uint64)
    st = _native.lib().st_jpeg_symbol_stats(c.ctypes.data, c.size, int(h), int(w), hs, vs, rst, out.ctypes.data)
    if st != 0:
        raise StError(st, "st_jpeg_symbol_stats(h=%d, w=%d): size outside 1..65535 or too few coefficients (%d)" % (h, w, c.size))
    return out


def jpeg_quant_tables(quality):
    """st_jpeg_quant_tables (host only): the (luma, chroma) quantisation tables of ``quality``, (64,) uint16 each, natural order."""
    luma, chroma = np.empty(64, np.uint16), np.empty(64, np.uint16)
    st = _native.lib().st_jpeg_quant_tables(int(quality), luma.ctypes.data, chroma.ctypes.data)
    if st != 0:
        raise StError(st, "quality %d is outside 1..100" % int(quality))
    return luma, chroma


def jpeg_encode_header(h, w, quality=95, subsampling="4:2:0", restart="row"):
    """st_jpeg_encode_header_rst (host only): the bytes SOI .. SOS of the stream encode_jpeg writes for such a frame: 629 with
    restart="row", 623 (no DRI segment) with restart="none"."""
    hs, vs = jpeg_sampling(subsampling)
    rst = jpeg_restart(restart)
    buf = ctypes.create_string_buffer(1024)
    size = ctypes.c_size_t()
    st = _native.lib().st_jpeg_encode_header_rst(int(h), int(w), int(quality), hs, vs, rst, buf, 1024, ctypes.byref(size))
    if st != 0:
        raise StError(st, "st_jpeg_encode_header(h=%d, w=%d, quality=%d): quality outside 1..100 or size outside 1..65535" % (h, w, quality))
    return buf.raw[:size.value]


def jpeg_encode_bound(h, w, subsampling="4:2:0"):
    """st_jpeg_encode_bound (host only): no stream of an (h, w, 3) frame at this sampling is longer, whatever its content."""
    hs, vs = jpeg_sampling(subsampling)
    v = _native.lib().st_jpeg_encode_bound(int(h), int(w), hs, vs)
    if v < 0:
        raise StError(1, "frame size %dx%d is outside 1..65535" % (w, h))
    return v


def jpeg_encode_bound_opt(h, w, subsampling="4:2:0"):
    """st_jpeg_encode_bound_opt (host only): jpeg_encode_bound for streams written with optimize=True."""
    hs, vs = jpeg_sampling(subsampling)
    v = _native.lib().st_jpeg_encode_bound_opt(int(h), int(w), hs, vs)
    if v < 0:
        raise StError(1, "frame size %dx%d is outside 1..65535" % (w, h))
    return v


def cpm2_geometry(h, w, scale):
    """(resize_h, resize_w, net_h, net_w) of the CPM2 network input for an (h, w) frame at ``scale``."""
    v = [ctypes.c_int() for _ in range(4)]
    st = _native.lib().st_cpm2_geometry(h, w, float(scale), *[ctypes.byref(x) for x in v])
    if st != 0:
        raise StError(st, "st_cpm2_geometry(%d, %d, %r)" % (h, w, scale))
    return tuple(x.value for x in v)


def facenet_geometry(h, w, scale):
    """(net_h, net_w) of the Facenet network input for an (h, w) frame at ``scale`` (st_facenet_geometry)."""
    nh, nw = ctypes.c_int(), ctypes.c_int()
    st = _native.lib().st_facenet_geometry(int(h), int(w), float(scale), ctypes.byref(nh), ctypes.byref(nw))
    if st != 0:
        raise StError(st, "st_facenet_geometry(%d, %d, %r)" % (h, w, scale))
    return nh.value, nw.value


def caffe_input_axis(n_in, n_out):
    """(status, begin, first, count) of one axis of CaffeInput's box filter (st_caffe_input_axis, host only): int32 arrays
    of n_out entries; status is ST_ERR_UNSUPPORTED when some window is empty (count 0)."""
    begin, first, count = (np.empty(int(n_out), np.int32) for _ in range(3))
    ip = ctypes.POINTER(ctypes.c_int)
    st = _native.lib().st_caffe_input_axis(int(n_in), int(n_out), begin.ctypes.data_as(ip), first.ctypes.data_as(ip),
                                           count.ctypes.data_as(ip))
    if st not in (_native.ST_OK, _native.ST_ERR_UNSUPPORTED):
        raise StError(st, "st_caffe_input_axis(%d, %d)" % (n_in, n_out))
    return st, begin, first, count


def cpm2_scale_for_height(h, target_h):
    """The float scale at which `cpm2_geometry` resizes a frame of height h to exactly target_h rows (what the OpenPose
    op uses for its fixed network input height: 368.f / 1080 truncates to 367)."""
    v = ctypes.c_float()
    st = _native.lib().st_cpm2_scale_for_height(int(h), int(target_h), ctypes.byref(v))
    if st != 0:
        raise StError(st, "st_cpm2_scale_for_height(%d, %d)" % (h, target_h))
    return float(v.value)


def fb_levels(h, w, params=None):
    prm = params if params is not None else default_params()
    return _native.lib().st_fb_levels(h, w, ctypes.byref(prm))


def fb_level_geom(h, w, level, params=None):
    prm = params if params is not None else default_params()
    lh, lw, ks = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    sg = ctypes.c_double()
    st = _native.lib().st_fb_level_geom(h, w, ctypes.byref(prm), level, ctypes.byref(lh), ctypes.byref(lw),
                                        ctypes.byref(sg), ctypes.byref(ks))
    if st != 0:
        raise StError(st, "st_fb_level_geom")
    return lh.value, lw.value, sg.value, ks.value
