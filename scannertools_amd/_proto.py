"""Tiny proto3 wire-format writer for the ops' argument messages
(/root/reference/scannertools/scannertools_cpp/imgproc/scannertools_imgproc.proto and
/root/reference/scannertools_caffe/scannertools_caffe_cpp/scannertools_caffe.proto); the C++ side
reads them with scanner_kernels/proto_lite.h.  Default-valued fields are omitted, as proto3 does."""
import struct


def _varint(v):
    v &= (1 << 64) - 1
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def encode(fields):
    """fields: iterable of (number, kind, value), kind in int32 / int64 / bool / float / string."""
    out = bytearray()
    for number, kind, value in fields:
        if kind in ("int32", "int64", "bool"):
            if int(value) == 0:
                continue
            out += _varint(number << 3 | 0) + _varint(int(value))
        elif kind == "float":
            if float(value) == 0.0:
                continue
            out += _varint(number << 3 | 5) + struct.pack("<f", float(value))
        elif kind == "string":
            data = value.encode() if isinstance(value, str) else bytes(value)
            if not data:
                continue
            out += _varint(number << 3 | 2) + _varint(len(data)) + data
        else:
            raise ValueError("unsupported field kind %r" % kind)
    return bytes(out)


def fields(buf):
    """Iterate a serialized message: yields (number, wire_type, value); value is an int for varint / fixed
    fields and a memoryview for length-delimited ones.  Raises ValueError on a truncated message."""
    mv = memoryview(buf)
    i, n = 0, len(mv)
    while i < n:
        key, shift = 0, 0
        while True:
            if i >= n:
                raise ValueError("truncated varint")
            b = mv[i]
            i += 1
            key |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                break
        number, wt = key >> 3, key & 7
        if wt == 0:
            v, shift = 0, 0
            while True:
                if i >= n:
                    raise ValueError("truncated varint")
                b = mv[i]
                i += 1
                v |= (b & 0x7F) << shift
                shift += 7
                if not b & 0x80:
                    break
            yield number, wt, v
        elif wt == 1:
            if i + 8 > n:
                raise ValueError("truncated fixed64")
            yield number, wt, int.from_bytes(mv[i:i + 8], "little")
            i += 8
        elif wt == 5:
            if i + 4 > n:
                raise ValueError("truncated fixed32")
            yield number, wt, int.from_bytes(mv[i:i + 4], "little")
            i += 4
        elif wt == 2:
            ln, shift = 0, 0
            while True:
                if i >= n:
                    raise ValueError("truncated length")
                b = mv[i]
                i += 1
                ln |= (b & 0x7F) << shift
                shift += 7
                if not b & 0x80:
                    break
            if i + ln > n:
                raise ValueError("truncated field %d" % number)
            yield number, wt, mv[i:i + ln]
            i += ln
        else:
            raise ValueError("unsupported wire type %d" % wt)


def message(number, payload):
    """A length-delimited field (sub-message, bytes, packed repeated) with the given serialized payload."""
    return _varint(number << 3 | 2) + _varint(len(payload)) + bytes(payload)


IMAGE_TYPES = {"PNG": 0, "JPEG": 1, "ANY": 2}   # ImageDecoderArgs.ImageType


ENTROPY_MODES = {"HOST": 0, "GPU": 1, "AUTO": 2}   # ImageDecoderArgs.Entropy


ENTROPY_SPLITS = {"INTERVAL": 0, "SUBSEQUENCE": 1}   # ImageDecoderArgs.Split


PNG_MODES = {"REFUSE": 0, "DECODE": 1}   # ImageDecoderArgs.Png


def image_decoder_args(image_type=None, entropy=None, split=None, scale_denom=None, png=None):
    """A serialised ImageDecoderArgs.  None: the empty message (the op then decodes JPEG).  A named or numeric type is
    written explicitly, PNG = 0 too (proto3 would omit it, and the kernel could not tell it from an absent field).
    entropy (field 2): None leaves the field out (HOST); "host" / "gpu" / "auto" in either case, or a number, is written.
    split (field 3): None leaves the field out (INTERVAL); "interval" / "subsequence" in either case, or a number, is written.
    scale_denom (field 4, int32): None or 0 leaves the field out (full size, as proto3 omits a zero); any other number is
    written, 1, 2, 4 and 8 being the ones the op accepts.
    png (field 5): None leaves the field out (REFUSE: PNG rows are not decoded); "refuse" / "decode" in either case, or a
    number, is written."""
    out = b""
    if image_type is not None:
        v = IMAGE_TYPES[image_type] if isinstance(image_type, str) else int(image_type)
        out += _varint(1 << 3 | 0) + _varint(v)
    if entropy is not None:
        if isinstance(entropy, str) and entropy.upper() not in ENTROPY_MODES:
            raise ValueError("entropy must be one of 'host', 'gpu', 'auto' or a number, got %r" % (entropy,))
        v = ENTROPY_MODES[entropy.upper()] if isinstance(entropy, str) else int(entropy)
        out += _varint(2 << 3 | 0) + _varint(v)
    if split is not None:
        if isinstance(split, str) and split.upper() not in ENTROPY_SPLITS:
            raise ValueError("split must be one of 'interval', 'subsequence' or a number, got %r" % (split,))
        v = ENTROPY_SPLITS[split.upper()] if isinstance(split, str) else int(split)
        out += _varint(3 << 3 | 0) + _varint(v)
    if scale_denom is not None and int(scale_denom) != 0:
        out += _varint(4 << 3 | 0) + _varint(int(scale_denom))
    if png is not None:
        if isinstance(png, str) and png.upper() not in PNG_MODES:
            raise ValueError("png must be one of 'refuse', 'decode' or a number, got %r" % (png,))
        v = PNG_MODES[png.upper()] if isinstance(png, str) else int(png)
        out += _varint(5 << 3 | 0) + _varint(v)
    return out


def parse_image_decoder_args(buf):
    """{'image_type': name or number, 'entropy': name or number, 'split': name or number, 'scale_denom': number, 'png': name or
    number} of a serialised ImageDecoderArgs; a key is missing when its field is absent."""
    names = {v: k for k, v in IMAGE_TYPES.items()}
    modes = {v: k for k, v in ENTROPY_MODES.items()}
    out = {}
    for number, wt, value in fields(buf):
        if number == 1 and wt == 0:
            out["image_type"] = names.get(value, value)
        if number == 2 and wt == 0:
            out["entropy"] = modes.get(value, value)
        if number == 3 and wt == 0:
            out["split"] = {v: k for k, v in ENTROPY_SPLITS.items()}.get(value, value)
        if number == 4 and wt == 0:
            value &= 0xFFFFFFFF                       # an int32 field: the low 32 bits, sign-extended
            out["scale_denom"] = value - (1 << 32) if value >> 31 else value
        if number == 5 and wt == 0:
            out["png"] = {v: k for k, v in PNG_MODES.items()}.get(value, value)
    return out


ENCODER_RESTARTS = {"MCU_ROW": 0, "NONE": 1}   # ImageEncoderArgs.Restart


ENCODER_FORMATS = {"JPEG": 0, "PNG": 1}        # ImageEncoderArgsWithFormat.Format
ENCODER_PNG_FILTERS = {"ADAPTIVE": 0, "NONE": 1, "SUB": 2, "UP": 3, "AVERAGE": 4, "PAETH": 5}   # ImageEncoderArgsWithFormat.PngFilter


def _enum_field(what, names, value):
    if isinstance(value, str):
        if value.upper() not in names:
            raise ValueError("%s must be one of %s or a number, got %r" % (what, ", ".join(repr(k.lower()) for k in names), value))
        return names[value.upper()]
    if value is None or isinstance(value, bool) or not isinstance(value, int):
        raise ValueError("%s must be one of %s or a number, got %r" % (what, ", ".join(repr(k.lower()) for k in names), value))
    return value


def image_encoder_args(quality=0, subsampling="", restart=0, optimize=False, format=0, png_filter=0):
    """A serialised ImageEncoderArgs (scannertools_imgproc_amd.proto): quality = 1, subsampling = 2, restart = 3 (a number, or
    "mcu_row" / "none" in either case), optimize = 4 (False / True, or a number: any other than 0 / 1 fails the op's
    validation).  The defaults (0, "", MCU_ROW = 0, false) are not written, as proto3 does; the op then takes quality 95,
    "4:2:0", one restart interval per MCU row and the Annex K Huffman tables.  format = 5 ("jpeg" / "png" or a number) and
    png_filter = 6 ("adaptive", "none", "sub", "up", "average", "paeth" or a number) likewise: absent when JPEG / ADAPTIVE, so a
    message without them is byte for byte what it was before they existed.  A number for png_filter is the message's PngFilter
    enum (ADAPTIVE = 0, NONE = 1, SUB = 2, UP = 3, AVERAGE = 4, PAETH = 5), NOT the library's ST_PNG_FILTER_* that
    HipContext.encode_png(filter=<number>) takes (PNG's types 0..4, adaptive = 5): 3 is UP here and AVERAGE there."""
    format = _enum_field("format", ENCODER_FORMATS, format)
    png_filter = _enum_field("png_filter", ENCODER_PNG_FILTERS, png_filter)
    if isinstance(optimize, str) or optimize is None or not isinstance(optimize, (bool, int)):
        raise ValueError("optimize must be False, True or a number, got %r" % (optimize,))
    if isinstance(restart, str):
        if restart.upper() not in ENCODER_RESTARTS:
            raise ValueError("restart must be one of 'mcu_row', 'none' or a number, got %r" % (restart,))
        restart = ENCODER_RESTARTS[restart.upper()]
    out = encode([(1, "int32", int(quality)), (2, "string", subsampling or "")])
    if int(restart) != 0:
        out += _varint(3 << 3 | 0) + _varint(int(restart) & ((1 << 64) - 1))
    if int(optimize) != 0:
        out += _varint(4 << 3 | 0) + _varint(int(optimize) & ((1 << 64) - 1))
    if format != 0:
        out += _varint(5 << 3 | 0) + _varint(format & ((1 << 64) - 1))
    if png_filter != 0:
        out += _varint(6 << 3 | 0) + _varint(png_filter & ((1 << 64) - 1))
    return out


def parse_image_encoder_args(buf):
    """{'quality': int, 'subsampling': str, 'restart': name or number, 'optimize': bool or number, 'format': name or number,
    'png_filter': name or number} of a serialised ImageEncoderArgs; an absent field is left out."""
    names = {v: k for k, v in ENCODER_RESTARTS.items()}
    out = {}
    for number, wt, value in fields(buf):
        if number == 1 and wt == 0:
            out["quality"] = value - (1 << 64) if value >> 63 else value
        elif number == 2 and wt == 2:
            out["subsampling"] = bytes(value).decode()
        elif number == 3 and wt == 0:
            value = value - (1 << 64) if value >> 63 else value
            out["restart"] = names.get(value, value)
        elif number == 4 and wt == 0:
            value = value - (1 << 64) if value >> 63 else value
            out["optimize"] = bool(value) if value in (0, 1) else value
        elif number in (5, 6) and wt == 0:
            value = value - (1 << 64) if value >> 63 else value
            table = ENCODER_FORMATS if number == 5 else ENCODER_PNG_FILTERS
            out["format" if number == 5 else "png_filter"] = {v: k for k, v in table.items()}.get(value, value)
    return out


def repeated_float(number, values, packed=True):
    """A `repeated float` field: packed (one length-delimited field, what proto3 writes) or unpacked (one fixed32 field per
    value, zeros included).  No values: nothing."""
    values = [float(v) for v in values]
    if not values:
        return b""
    if packed:
        return message(number, struct.pack("<%df" % len(values), *values))
    return b"".join(_varint(number << 3 | 5) + struct.pack("<f", v) for v in values)


def net_descriptor(input_width=0, input_height=0, mean_colors=(), normalize=False, packed=True, model_path="", model_weights_path="",
                   input_layer_names=(), output_layer_names=(), preserve_aspect_ratio=False, transpose=False, pad_mod=0):
    """A serialised NetDescriptor (scannertools_caffe.proto:5-26): model_path = 1, model_weights_path = 2, input_layer_names = 3,
    output_layer_names = 4 (what the Caffe and Facenet ops read), input_width = 5, input_height = 6, mean_colors = 7,
    normalize = 11 (what the network-input ops read), preserve_aspect_ratio = 12, transpose = 13, pad_mod = 14."""
    names = b"".join(message(3, str(n).encode()) for n in input_layer_names) + b"".join(message(4, str(n).encode()) for n in output_layer_names)
    return (encode([(1, "string", str(model_path)), (2, "string", str(model_weights_path))]) + names +
            encode([(5, "int32", input_width), (6, "int32", input_height)]) + repeated_float(7, mean_colors, packed) +
            encode([(11, "bool", normalize), (12, "bool", preserve_aspect_ratio), (13, "bool", transpose), (14, "int32", pad_mod)]))


def caffe_args(batch_size=0, **descriptor):
    """A serialised CaffeArgs (scannertools_caffe.proto:33-36): net_descriptor = 1 (net_descriptor()'s keywords), batch_size = 2."""
    nd = net_descriptor(**descriptor)
    return (message(1, nd) if nd else b"") + encode([(2, "int32", batch_size)])


def facenet_args(scale, mean_colors, templates_path="", threshold=0.0, packed=True, batch_size=0, **descriptor):
    """A serialised FacenetArgs (scannertools_caffe.proto:38-43): caffe_args = 1 (CaffeArgs{net_descriptor = 1, batch_size = 2}; the
    descriptor takes net_descriptor()'s keywords), templates_path = 2, scale = 3, threshold = 4."""
    ca = caffe_args(batch_size, mean_colors=mean_colors, packed=packed, **descriptor)
    return ((message(1, ca) if ca else b"") +
            encode([(2, "string", templates_path), (3, "float", scale), (4, "float", threshold)]))


def caffe_input_args(input_width, input_height, mean_colors, normalize=False, batch_size=0, packed=True):
    """A serialised CaffeInputArgs (scannertools_caffe.proto:28-31): net_descriptor = 1, batch_size = 2."""
    nd = net_descriptor(input_width, input_height, mean_colors, normalize, packed)
    return (message(1, nd) if nd else b"") + encode([(2, "int32", batch_size)])
