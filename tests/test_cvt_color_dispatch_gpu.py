"""Every kernel instance st_cvt_color_u8_batch (csrc/st_imgproc.hip) can launch, reached by every code that can reach it.

`host_choice` restates the launcher's choice; the case table is built from it and a CPU test checks that it reaches all
36 instances.  Each case runs two frames of different content through its instance twice -- once at a geometry whose
size selects the instance, once on a shared geometry where only the frames' alignment (views at an offset into a
larger buffer) selects it -- and asserts, for each run: the instance is the one the launcher picks, the result equals
the C oracle bit for bit AND lies within tests/ref_color_np.py's bounds of the float64 definition on its own input (so
a kernel and the oracle changed together around one misreading still fail), nothing is written outside the output,
and the shared input gives the same bytes as the code's widest instance.  The widest instance of each code also runs
the code's whole input domain (the byte cube, the cube with alpha, every packed pixel, every gray, every (Y, U, V)
triple in the source's layout) against the oracle and the definition, mean signed error included.  The codes that use
the op's gray table run at gray_bits 14 and 15."""
import functools

import numpy as np
import pytest

import oracle
import ref_color_np as ref

# the 14 (source, destination) channel pairs of the launcher's switch on 10 * scn + dcn (st_cvt_color_u8_batch, "case 33:"
# .. "case 21:"); any other pair, and every pixel count or alignment that gives px = 1, takes the byte-wise kernel
VEC_PAIRS = [(3, 3), (3, 1), (1, 3), (3, 4), (4, 3), (4, 4), (1, 4), (4, 1), (3, 2), (2, 3), (4, 2), (2, 4), (1, 2), (2, 1)]
ALL_INSTANCES = ({"k_cvt_color_u8", "k_cvt_yuv_u8"} | {"k_cvt_color_u8_vec<%d,%d,%d>" % (s, d, px) for s, d in VEC_PAIRS for px in (4, 16)}
                 | {"k_cvt_yuv_u8_vec<%d,%d>" % (d, px) for d in (1, 3, 4) for px in (4, 16)})
PLANAR_420 = range(98, 106)          # cvt_yuv_of kind 1 (YV12 / IYUV to colour); GRAY_420 (106) is kind 3, not planar
PACKED_422 = range(107, 125)         # kinds 2 and 4


def host_choice(code, h, w, c, align):
    """The instance st_cvt_color_u8_batch launches for n frames of (h, w, c) whose addresses (sources and outputs) OR to
    `align`."""
    if code in ref.YUV_SOURCES:
        dcn = ref.YUV_SOURCES[code][2]
        oh, ow = (h, w) if code in PACKED_422 else (h // 3 * 2, w)     # st_cvt_color_out_shape
        planar, packed422 = code in PLANAR_420, code in PACKED_422
        # "const int px = (!packed422 && ow % (planar ? 32 : 16) == 0 && (align & 15) == 0 && (!planar || ((long long)oh * ow
        #  / 4) % 16 == 0)) ? 16 : ((ow % 4 == 0 && (align & 3) == 0) ? 4 : 1);"
        px = (16 if (not packed422 and ow % (32 if planar else 16) == 0 and align & 15 == 0 and (not planar or (oh * ow // 4) % 16 == 0))
              else (4 if ow % 4 == 0 and align & 3 == 0 else 1))
        # "if (px == 1) k_cvt_yuv_u8; else if (yd.dcn == 1) YUV_VEC(1); else if (yd.dcn == 3) YUV_VEC(3); else YUV_VEC(4);"
        return "k_cvt_yuv_u8" if px == 1 else "k_cvt_yuv_u8_vec<%d,%d>" % (dcn, px)
    scn, dcn = ref.channels(code)
    npix = h * w
    # "const int px = (a.npix % 16 == 0 && (align & 15) == 0) ? 16 : ((a.npix % 4 == 0 && (align & 3) == 0) ? 4 : 1);"
    px = 16 if npix % 16 == 0 and align & 15 == 0 else (4 if npix % 4 == 0 and align & 3 == 0 else 1)
    # "const int key = px > 1 ? 10 * a.scn + a.dcn : 0;" then the switch
    if px > 1 and (scn, dcn) in VEC_PAIRS:
        return "k_cvt_color_u8_vec<%d,%d,%d>" % (scn, dcn, px)
    return "k_cvt_color_u8"


def family(code):
    if code in ref.YUV_SOURCES:
        return "422" if code in PACKED_422 else "420"
    return "pixel"


# per family: the source shapes (h, w, c) whose size selects an instance at an aligned address, and the shared shape
# whose instance the alignment alone selects.  The 4:2:0 frames hold 38 rows (H % 4 == 2: an odd number of chroma rows);
# a planar frame 48 wide takes the 4-pixel kernel where a semi-planar one takes the 16-pixel kernel (chroma rows of
# W / 2 bytes); 4:2:2 frames never take 16 pixels per thread.
SIZED = {"pixel": [(32, 48), (36, 53), (37, 53)],                     # 1536 px (% 16), 1908 (% 4, not % 16), 1961 (odd)
         "420": [(57, 64), (57, 48), (57, 52), (57, 54)],             # W 64, 48, 52 (% 4, not % 16), 54 (not % 4)
         "422": [(38, 48), (38, 52), (38, 54)]}
SHARED = {"pixel": (32, 48), "420": (57, 64), "422": (38, 64)}
OFFSETS = (0, 4, 1, 6)


def src_channels(code):
    return {"420": 1, "422": 2}.get(family(code)) or ref.channels(code)[0]


def code_names():
    from scannertools_amd._native import COLOR_CODES
    names = {}
    for n, c in COLOR_CODES.items():
        names.setdefault(c, n)
    return names


def domain_shape(code):
    f = family(code)
    if f == "420":
        return (6144, 4096, 1)
    if f == "422":
        return (4096, 4096, 2)
    return ref.pixel_domain(src_channels(code)).shape


def build_cases():
    cases = []
    for code, name in sorted(code_names().items()):
        c, fam = src_channels(code), family(code)
        widest = host_choice(code, *domain_shape(code), 0)
        seen = {}
        for h, w in SIZED[fam]:
            seen.setdefault(host_choice(code, h, w, c, 0), (h, w))
        shared = {}
        for off in OFFSETS:
            shared.setdefault(host_choice(code, *SHARED[fam], c, off), off)
        assert set(seen) == set(shared), (name, seen, shared)
        for inst in sorted(seen):
            cases.append((name, code, inst, seen[inst], shared[inst], inst == widest))
    return cases


CASES = build_cases()


def test_table_reaches_every_instance_of_the_launcher():
    """CPU-side: the case table covers all 36 kernel instances; every code has one widest instance (the one its whole
    domain runs through) and reaches three instances -- 16 pixels, 4 pixels, byte-wise -- or two for the 4:2:2 sources,
    which never take 16 pixels per thread."""
    assert {c[2] for c in CASES} == ALL_INSTANCES and len(ALL_INSTANCES) == 36
    by_code = {}
    for name, code, inst, _, _, widest in CASES:
        by_code.setdefault(code, []).append((inst, widest))
    assert len(by_code) == 91
    for code, insts in by_code.items():
        assert sum(w for _, w in insts) == 1, code
        assert len(insts) == (2 if family(code) == "422" else 3), (code, insts)


@functools.lru_cache(maxsize=4)
def domain_frame(code_family_key):
    fam, key = code_family_key
    return ref.yuv_full_domain(key) if fam != "pixel" else ref.pixel_domain(key)


def frames_for(code, h, w, seed):
    """Two frames of different content: random bytes, or random 4:2:0 / 4:2:2 planes whose chroma changes per block."""
    rng = np.random.default_rng(seed)
    fam = family(code)
    if fam == "pixel":
        return rng.integers(0, 256, (2, h, w, src_channels(code)), dtype=np.uint8)
    layout = ref.yuv_layout_of(code)
    oh = h if fam == "422" else h // 3 * 2
    return np.stack([ref.encode_yuv(*ref.yuv_block_planes(rng, oh, w, layout), layout) for _ in range(2)])


SENTINEL, GUARD = 0xA5, 64


def run(hip_ctx, code, frames, off, gray_bits):
    """frames (n, h, w, c) -> (instance picked, result), the sources and the output views at `off` bytes past a 64-byte
    guard; asserts the guards around the output are untouched."""
    import torch
    n, h, w, c = frames.shape
    ins = []
    for f in frames:
        buf = torch.zeros(GUARD + off + f.nbytes + GUARD, dtype=torch.uint8, device="cuda")
        v = buf[GUARD + off:GUARD + off + f.nbytes].view(h, w, c)
        v.copy_(torch.from_numpy(np.ascontiguousarray(f)))
        ins.append(v)
    oshape = ref_out_shape(code, h, w)
    ob = int(np.prod(oshape))
    obuf = torch.full((GUARD + off + n * ob + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = obuf[GUARD + off:GUARD + off + n * ob].view(n, *oshape)
    assert obuf.data_ptr() % 256 == 0
    align = 0
    for i in range(n):
        align |= ins[i].data_ptr() | out[i].data_ptr()
    inst = host_choice(code, h, w, c, align)
    hip_ctx.cvt_color(ins, code, gray_bits=gray_bits, out=out)
    o = obuf.cpu().numpy()
    assert (o[:GUARD + off] == SENTINEL).all() and (o[GUARD + off + n * ob:] == SENTINEL).all(), "write outside the output"
    return inst, out.cpu().numpy()


def ref_out_shape(code, h, w):
    if code in ref.YUV_SOURCES:
        return ((h if code in PACKED_422 else h // 3 * 2), w, ref.YUV_SOURCES[code][2])
    return (h, w, ref.channels(code)[1])


def check_definition(code, frame, got, what, gray_bits, bias=False):
    if code in ref.YUV_SOURCES:
        ref.check_yuv(code, frame, got, what, bias=bias)
    else:
        ref.check_pixels(code, frame, got, what, gray_bits=gray_bits, bias=bias)


@pytest.mark.gpu
@pytest.mark.parametrize("name,code,instance,sized,shared_off,widest", CASES, ids=["%s-%s" % (c[0], c[2]) for c in CASES])
def test_cvt_color_instance(hip_ctx, name, code, instance, sized, shared_off, widest):
    fam, c = family(code), src_channels(code)
    for bits in ((14, 15) if code in ref.GRAY_TABLE_CODES else (15,)):
        # the size selects the instance
        f = frames_for(code, *sized, seed=code * 7 + sized[1])
        inst, got = run(hip_ctx, code, f, 0, bits)
        assert inst == instance, (inst, instance)
        for i in range(2):
            what = "%s (%s) %dx%d frame %d gray_bits %d" % (instance, name, sized[1], sized[0], i, bits)
            np.testing.assert_array_equal(got[i], oracle.cvt_color(f[i], code, gray_bits=bits), err_msg=what)
            check_definition(code, f[i], got[i], what, bits)
        # the alignment selects the instance, on the input every instance of this code shares
        f = frames_for(code, *SHARED[fam], seed=code)
        inst, got = run(hip_ctx, code, f, shared_off, bits)
        assert inst == instance, (inst, instance)
        w_inst, w_got = run(hip_ctx, code, f, 0, bits)
        assert w_inst == host_choice(code, *domain_shape(code), 0)
        np.testing.assert_array_equal(got, w_got, err_msg="%s differs from %s on the shared input" % (instance, w_inst))
        for i in range(2):
            what = "%s (%s) shared input at offset %d frame %d gray_bits %d" % (instance, name, shared_off, i, bits)
            np.testing.assert_array_equal(got[i], oracle.cvt_color(f[i], code, gray_bits=bits), err_msg=what)
            check_definition(code, f[i], got[i], what, bits)
        if widest:
            key = (fam, ref.yuv_layout_of(code) if fam != "pixel" else c)
            d = domain_frame(key)[None]
            inst, got = run(hip_ctx, code, d, 0, bits)
            assert inst == instance, (inst, instance)
            what = "%s (%s) whole domain gray_bits %d" % (instance, name, bits)
            exp = oracle.cvt_color(d[0], code, gray_bits=bits)
            if not np.array_equal(got[0], exp):
                bad = np.argwhere(got[0] != exp)[:5]
                raise AssertionError("%s: %d bytes differ from the oracle, first at %s" % (what, int((got[0] != exp).sum()), bad.tolist()))
            check_definition(code, d[0], got[0], what, bits, bias=True)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [14, 15])
def test_flow_gray_whole_cube(hip_ctx, bits):
    """st_gray_u8 (the flow path's gray, OpenCV's BGR table on RGB bytes) over the whole byte cube, through the 4-pixel
    kernel (aligned) and the byte-wise kernel (a view at an odd address): the oracle bit for bit, the definition's bounds."""
    import torch
    cube = ref.pixel_domain(3)
    exp = oracle.gray_u8(cube, bits)
    for off in (0, 1):
        buf = torch.zeros(off + cube.nbytes, dtype=torch.uint8, device="cuda")
        v = buf[off:].view(cube.shape)
        v.copy_(torch.from_numpy(cube))
        got = hip_ctx.gray(v, bits).cpu().numpy()
        np.testing.assert_array_equal(got, exp, err_msg="offset %d" % off)
    st = ref.Stats([("v",)])
    for i in range(0, exp.size, ref.CHUNK):
        st.add(got.reshape(-1)[i:i + ref.CHUNK], ref.flow_gray(cube.reshape(-1, 3)[i:i + ref.CHUNK])[:, None])
    st.check([("v", ref.gray_bound(bits), ref.BIAS)], "st_gray_u8 %d-bit" % bits)
