"""Planar YCbCr of 9 to 16 bits per sample <-> the net's fp32 tensors on the device (csrc/fs_yuv16.hip) against its contract, the arithmetic
that include/faststyle_io.h states.  The first half of this file is an independent numpy restatement of that text (the chroma resampling is
tests/test_yuv.py's, which is depth-agnostic on int64), plus the float64 formulas the fixed-point matrices approximate; every comparison of
the device with the restatement is exact.  The same bodies run on the CPU emulator and, under -m gpu, on the MI355X.
tests/test_video_deep.py builds its expected frames with the restatement."""
import ctypes
import itertools
import math

import numpy as np
import pytest

from faststyle_amd import _lib as L
from tests import backends
from tests.test_yuv import COLOURS, LAYOUT_PARAMS, LAYOUTS, SIZES, downsample, geometry, host_lib, upsample
from tests import test_yuv as T8

FMAX = 65280                                                    # 255 in unsigned 8.8


def constants(matrix, full_range, d):
    """(Kr, Kb, Kg, sy, sc, oy, chroma offset, m) of depth d"""
    k, m = d - 8, 2 ** d - 1
    Kr, Kb = (0.2126, 0.0722) if matrix else (0.299, 0.114)
    Kg = 1.0 - Kr - Kb
    if full_range:
        sy, sc, oy = 65280.0 / m, 65280.0 / m, 0
    else:
        sy, sc, oy = 65280.0 / (219.0 * 2 ** k), 65280.0 / (224.0 * 2 ** k), 16 * 2 ** k
    return Kr, Kb, Kg, sy, sc, oy, 2 ** (d - 1), m


def fix24(c):
    return int(math.floor(c * 16777216.0 + 0.5))


def split(planes, W, H, hs, vs, ncomp, d):
    """One frame's samples (flat uint16, as stored) -> its planes as int64, read as the contract reads them: a value above m is m."""
    cw, ch, n = geometry(W, H, hs, vs, ncomp)
    s = np.minimum(np.asarray(planes, np.uint16).reshape(-1).astype(np.int64), 2 ** d - 1)
    assert s.size == n
    y = s[:W * H].reshape(H, W)
    if ncomp == 1:
        return y, None, None
    return y, s[W * H:W * H + cw * ch].reshape(ch, cw), s[W * H + cw * ch:].reshape(ch, cw)


# ---------------------------------------------------------------- the fixed-point matrices
def ycc_to_F(Y, Cb, Cr, matrix, full_range, d):
    """int64 arrays of equal shape -> F, int64 [..., 3] (R, G, B) in [0, 65280]"""
    Kr, Kb, Kg, sy, sc, oy, off, m = constants(matrix, full_range, d)
    cy = fix24(sy)
    r_cr, b_cb = fix24(2.0 * (1.0 - Kr) * sc), fix24(2.0 * (1.0 - Kb) * sc)
    g_cb, g_cr = fix24(-(2.0 * (1.0 - Kb) * Kb / Kg * sc)), fix24(-(2.0 * (1.0 - Kr) * Kr / Kg * sc))
    Y, u, v = Y.astype(np.int64) - oy, Cb.astype(np.int64) - off, Cr.astype(np.int64) - off
    sums = [cy * Y + r_cr * v, cy * Y + g_cb * u + g_cr * v, cy * Y + b_cb * u]
    assert all(np.abs(s).max() < 2 ** 42 for s in sums)
    return np.stack([np.clip((s + 2 ** 23) >> 24, 0, FMAX) for s in sums], axis=-1)


def F_to_ycc(F, matrix, full_range, d):
    """F int64 [..., 3] (R, G, B) -> (Y, Cb, Cr) int64 arrays in [0, m]"""
    Kr, Kb, Kg, sy, sc, oy, off, m = constants(matrix, full_range, d)
    rows = [([Kr / sy, Kg / sy, Kb / sy], oy),
            ([-Kr / (2.0 * (1.0 - Kb)) / sc, -Kg / (2.0 * (1.0 - Kb)) / sc, (1.0 - Kb) / (2.0 * (1.0 - Kb)) / sc], off),
            ([(1.0 - Kr) / (2.0 * (1.0 - Kr)) / sc, -Kg / (2.0 * (1.0 - Kr)) / sc, -Kb / (2.0 * (1.0 - Kr)) / sc], off)]
    p = F.astype(np.int64)
    out = []
    for coef, o in rows:
        s = sum(fix24(c) * p[..., k] for k, c in enumerate(coef)) + (o << 24) + 2 ** 23
        assert np.abs(s).max() < 2 ** 42
        out.append(np.clip(s >> 24, 0, m))
    return out


def f32_of_F(F):
    """The net's input of F: exact, a power of two times an integer below 2^24"""
    return F.astype(np.float32) * np.float32(0.00390625)


def F_of_f32(x):
    """The net's output on the 8.8 scale: clamped to [0, 255] with NaN -> 0, times 256, truncated"""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        q = np.where(np.isnan(x), np.float32(0), np.minimum(np.maximum(x, np.float32(0)), np.float32(255))).astype(np.float32)
    return (q * np.float32(256)).astype(np.int64)


# ---------------------------------------------------------------- the float64 formulas
def ycc_to_F_exact(Y, Cb, Cr, matrix, full_range, d):
    Kr, Kb, Kg, sy, sc, oy, off, m = constants(matrix, full_range, d)
    Y, u, v = sy * (Y.astype(np.float64) - oy), sc * (Cb.astype(np.float64) - off), sc * (Cr.astype(np.float64) - off)
    R = Y + 2.0 * (1.0 - Kr) * v
    B = Y + 2.0 * (1.0 - Kb) * u
    G = Y - 2.0 * (1.0 - Kb) * Kb / Kg * u - 2.0 * (1.0 - Kr) * Kr / Kg * v
    return np.clip(np.floor(np.stack([R, G, B], axis=-1) + 0.5), 0, FMAX).astype(np.int64)


def F_to_ycc_exact(F, matrix, full_range, d):
    Kr, Kb, Kg, sy, sc, oy, off, m = constants(matrix, full_range, d)
    R, G, B = (F[..., k].astype(np.float64) for k in range(3))
    Yl = Kr * R + Kg * G + Kb * B
    Y = Yl / sy + oy
    Cb = (B - Yl) / (2.0 * (1.0 - Kb)) / sc + off
    Cr = (R - Yl) / (2.0 * (1.0 - Kr)) / sc + off
    return [np.clip(np.floor(v + 0.5), 0, m).astype(np.int64) for v in (Y, Cb, Cr)]


# ---------------------------------------------------------------- whole frames
def frame_to_F(planes, W, H, hs=2, vs=2, ncomp=3, siting=0, matrix=0, full_range=0, bits=10):
    """One frame's samples (flat uint16) -> F int64 [H, W, 3]"""
    y, cb, cr = split(planes, W, H, hs, vs, ncomp, bits)
    if ncomp == 1:
        u = v = np.full((H, W), 2 ** (bits - 1), np.int64)
    else:
        u, v = upsample(cb, H, W, hs, vs, siting), upsample(cr, H, W, hs, vs, siting)
    return ycc_to_F(y, u, v, matrix, full_range, bits)


def frame_to_f32(planes, W, H, swap=False, **kw):
    """One frame's samples -> the net's input, float32 [H, W, 3] (swap: B,G,R)"""
    img = f32_of_F(frame_to_F(planes, W, H, **kw))
    return np.ascontiguousarray(img[..., ::-1]) if swap else img


def f32_to_frame(img, hs=2, vs=2, ncomp=3, siting=0, matrix=0, full_range=0, bits=10, swap=False):
    """float32 [H, W, 3] (swap: the channels are B,G,R) -> one frame's samples (flat uint16)"""
    F = F_of_f32(img)
    if swap:
        F = F[..., ::-1]
    Y, Cb, Cr = F_to_ycc(F, matrix, full_range, bits)
    parts = [Y]
    if ncomp == 3:
        parts += [downsample(Cb, hs, vs, siting), downsample(Cr, hs, vs, siting)]
    return np.concatenate([p.reshape(-1) for p in parts]).astype(np.uint16)


# ================================================================ the tests
DEPTHS = (10, 12, 16)


def pattern(kind, shape, seed, top):
    """uint16 content of a plane: noise over [0, top], a 0 | top checkerboard, a ramp"""
    if kind == "noise":
        return np.random.RandomState(seed).randint(0, top + 1, size=shape).astype(np.uint16)
    idx = np.indices(shape)
    if kind == "checker":
        return (((idx.sum(axis=0) + seed) & 1) * top).astype(np.uint16)
    return ((idx[0] * 701 + idx[1] * 1301 + seed * 97) % (top + 1)).astype(np.uint16)


_cases = {}


def deep_frames(W, H, hs, vs, ncomp, d, top=None):
    """Three frames of one geometry (noise, checkerboard, ramp in every plane over [0, top], top = m unless given): uint16 [3, samples]"""
    top = 2 ** d - 1 if top is None else top
    key = ("yuv", W, H, hs, vs, ncomp, top)
    if key not in _cases:
        cw, ch, _ = geometry(W, H, hs, vs, ncomp)
        frames = []
        for k, kind in enumerate(("noise", "checker", "ramp")):
            planes = [pattern(kind, (H, W), 3 * k, top)] + \
                ([pattern(kind, (ch, cw), 3 * k + 1, top), pattern(kind, (ch, cw), 3 * k + 2, top)] if ncomp == 3 else [])
            frames.append(np.concatenate([p.reshape(-1) for p in planes]))
        _cases[key] = np.stack(frames)
        _cases[key].setflags(write=False)
    return _cases[key]


def f32_images(W, H):
    """Three net outputs of one size: noise over [0, 255], a 0 | 255 checkerboard, a ramp in 1 / 256 steps with a small offset"""
    key = ("f32", W, H)
    if key not in _cases:
        rs = np.random.RandomState(W * 100 + H)
        idx = np.indices((H, W, 3))
        ramp = ((idx[0] * 701 + idx[1] * 1301 + idx[2] * 2903) % (FMAX + 1)).astype(np.float32) / np.float32(256) + np.float32(1e-3)
        _cases[key] = np.stack([rs.uniform(0.0, 255.0, size=(H, W, 3)).astype(np.float32),
                                (((idx.sum(axis=0)) & 1) * 255).astype(np.float32), ramp])
        _cases[key].setflags(write=False)
    return _cases[key]


def plan(eng, W, H, hs, vs, ncomp, siting, matrix, full, bits):
    return eng.yuv_plan(W, H, sampling=(hs, vs), siting=siting, matrix=matrix, full_range=full, components=ncomp, bits=bits)


def as_bytes(frames_u16):
    return np.array(frames_u16, dtype="<u2").view(np.uint8).reshape(frames_u16.shape[0], -1)       # (a copy: the shared cases are read-only)


def to_f32(eng, desc, frames_u16, swap=False):
    """frames: host uint16 [N, samples] -> host float32 [N, H, W, 3] of the device call"""
    out = eng.mem.from_numpy(np.full((frames_u16.shape[0], desc.height, desc.width, 3), -7.0, np.float32))
    eng.yuv_deep_to_f32(eng.mem.upload_u8(as_bytes(frames_u16)), desc, out, swap_rb=swap)
    return np.array(eng.mem.to_numpy(out), copy=True)


def to_yuv(eng, desc, images, swap=False):
    """images: host float32 [N, H, W, 3] -> host uint16 [N, samples] of the device call"""
    out = eng.mem.upload_u8(np.full((images.shape[0], int(desc.frame_bytes)), 0xA5, np.uint8))
    eng.f32_to_yuv_deep(eng.mem.from_numpy(np.array(images, np.float32)), desc, out, swap_rb=swap)      # (a copy: the shared cases are read-only)
    return np.array(eng.mem.to_numpy(out), copy=True).view("<u2")


def same(a, b):
    """array_equal that also holds float images bit for bit"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        return a.shape == b.shape and b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


def check_to_f32(eng, W, H, hs, vs, ncomp, siting, matrix, full, d, top=None):
    desc = plan(eng, W, H, hs, vs, ncomp, siting, matrix, full, d)
    frames = deep_frames(W, H, hs, vs, ncomp, d, top)
    kw = dict(hs=hs, vs=vs, ncomp=ncomp, siting=siting, matrix=matrix, full_range=full, bits=d)
    where = (W, H, d, matrix, full)
    want = np.stack([frame_to_f32(f, W, H, **kw) for f in frames])
    assert same(to_f32(eng, desc, frames), want), where                                       # N = 3 frames in one call
    assert same(to_f32(eng, desc, frames[1:], swap=True), want[1:, :, :, ::-1]), where


def check_to_yuv(eng, W, H, hs, vs, ncomp, siting, matrix, full, d):
    desc = plan(eng, W, H, hs, vs, ncomp, siting, matrix, full, d)
    images = f32_images(W, H)
    kw = dict(hs=hs, vs=vs, ncomp=ncomp, siting=siting, matrix=matrix, full_range=full, bits=d)
    where = (W, H, d, matrix, full)
    want = np.stack([f32_to_frame(im, **kw) for im in images])
    assert same(to_yuv(eng, desc, images), want), where
    assert same(to_yuv(eng, desc, np.ascontiguousarray(images[:2, :, :, ::-1]), swap=True), want[:2]), where


def test_plan_deep_reports_the_layout_in_16_bit_words():
    h = host_lib()
    for (_, hs, vs, ncomp, siting), (W, H), d in itertools.product(LAYOUTS, SIZES, (9, 10, 12, 14, 16)):
        desc = h.yuv_plan(W, H, sampling=(hs, vs), siting=siting, matrix=1, full_range=True, components=ncomp, bits=d)
        cw, ch, n = geometry(W, H, hs, vs, ncomp)
        assert (desc.width, desc.height, desc.hs, desc.vs, desc.ncomp, desc.siting, desc.matrix, desc.full_range) == (W, H, hs, vs, ncomp, siting, 1, 1)
        assert (desc.chroma_w, desc.chroma_h, desc.frame_bytes) == (cw, ch, 2 * n)
        assert list(desc.reserved) == [d, 0]
        assert list(desc.plane_bytes) == [2 * W * H, 2 * cw * ch, 2 * cw * ch]
        assert list(desc.plane_offset) == ([0, 2 * W * H, 2 * (W * H + cw * ch)] if ncomp == 3 else [0, 0, 0])
    assert ctypes.sizeof(L.fs_yuv_desc) == 104
    assert list(h.yuv_plan(8, 8).reserved) == [0, 0] and h.yuv_plan(8, 8, bits=8).frame_bytes == 96


def test_plan_deep_refusals():
    lib = host_lib().lib
    d = L.fs_yuv_desc()
    ref = ctypes.byref(d)
    good = (16, 16, 2, 2, 3, 0, 0, 0)
    assert lib.fs_yuv_plan_deep(*(good + (10, ref))) == 0
    before = bytes(d)
    for bits in (8, 17, 0, -1, 32):
        assert lib.fs_yuv_plan_deep(*(good + (bits, ref))) == -2, bits
        assert lib.fs_last_error().startswith(b"fs_yuv_plan_deep")
    for args, code in (((0, 16) + good[2:], -1), ((16, 40000) + good[2:], -1), ((16, 16, 1, 2, 3, 0, 0, 0), -2), ((16, 16, 2, 2, 2, 0, 0, 0), -2),
                       ((16, 16, 2, 1, 1, 0, 0, 0), -2), ((16, 16, 2, 2, 3, 2, 0, 0), -2), ((16, 16, 2, 2, 3, 0, 2, 0), -2), ((16, 16, 2, 2, 3, 0, 0, 2), -2)):
        assert lib.fs_yuv_plan_deep(*(args + (10, ref))) == code, args
    assert bytes(d) == before                                                              # a refused plan writes nothing
    assert lib.fs_yuv_plan_deep(*(good + (10, None))) == -1
    with pytest.raises(L.FaststyleError):
        host_lib().yuv_plan(16, 16, bits=17)
    with pytest.raises(L.FaststyleError):
        host_lib().yuv_plan(16, 16, bits=7)


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("hs,vs,ncomp,siting", LAYOUT_PARAMS)
def test_deep_to_f32_equals_the_restatement(kind, hs, vs, ncomp, siting):
    eng = backends.get_engine(kind)
    for (W, H), d, (matrix, full) in itertools.product(SIZES, DEPTHS, COLOURS):
        check_to_f32(eng, W, H, hs, vs, ncomp, siting, matrix, full, d)


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("hs,vs,ncomp,siting", LAYOUT_PARAMS)
def test_f32_to_deep_equals_the_restatement(kind, hs, vs, ncomp, siting):
    eng = backends.get_engine(kind)
    for (W, H), d, (matrix, full) in itertools.product(SIZES, DEPTHS, COLOURS):
        check_to_yuv(eng, W, H, hs, vs, ncomp, siting, matrix, full, d)


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("d", (9, 14))
def test_depths_9_and_14_both_directions(kind, d):
    eng = backends.get_engine(kind)
    for (W, H), (matrix, full) in itertools.product(SIZES, COLOURS):
        check_to_f32(eng, W, H, 2, 2, 3, 0, matrix, full, d)
        check_to_yuv(eng, W, H, 2, 2, 3, 0, matrix, full, d)


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("hs,vs,ncomp,siting", [pytest.param(*l[1:], id=l[0]) for l in LAYOUTS if l[0] in ("444", "420_cosited", "mono")])
def test_stored_values_above_the_depth_read_as_its_maximum(kind, hs, vs, ncomp, siting):
    """Noise over the full 16 bits in a 10-bit stream: every sample above 1023 is read as 1023, on both access paths."""
    eng = backends.get_engine(kind)
    for (W, H), (matrix, full) in itertools.product(SIZES, COLOURS):
        check_to_f32(eng, W, H, hs, vs, ncomp, siting, matrix, full, 10, top=65535)
    frames = deep_frames(64, 48, hs, vs, ncomp, 10, 65535)
    assert (frames > 1023).mean() > 0.5
    clamped = np.minimum(frames, 1023)
    desc = plan(eng, 64, 48, hs, vs, ncomp, siting, 0, 0, 10)
    assert same(to_f32(eng, desc, frames), to_f32(eng, desc, clamped))


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("hs,vs,ncomp,siting", LAYOUT_PARAMS)
def test_misaligned_buffers_take_the_narrow_path_with_the_same_values(kind, hs, vs, ncomp, siting):
    """64 x 48 in aligned buffers is eligible for the 8- and 16-byte accesses; the same planes two bytes further, or the same tensor one float
    further, are not, and give the same values."""
    eng = backends.get_engine(kind)
    lib, mem = eng.lib, eng.mem
    W, H, d = 64, 48, 12
    desc = plan(eng, W, H, hs, vs, ncomp, siting, 1, 0, d)
    n = int(desc.frame_bytes)
    kw = dict(hs=hs, vs=vs, ncomp=ncomp, siting=siting, matrix=1, full_range=0, bits=d)
    frames, images = deep_frames(W, H, hs, vs, ncomp, d)[:2], f32_images(W, H)[:2]
    want_f32 = np.stack([frame_to_f32(f, W, H, **kw) for f in frames])
    want_yuv = np.stack([f32_to_frame(im, **kw) for im in images])
    # planes -> fp32: aligned, planes + 2 bytes, tensor + 1 float
    src = mem.upload_u8(np.concatenate([[0x33, 0x33], as_bytes(frames).reshape(-1)]).astype(np.uint8))
    for src_off, dst_off in ((2, 0), (2, 1)):
        dst = mem.from_numpy(np.full(1 + 2 * H * W * 3 + 3, -7.0, np.float32))
        eng._sync_stream()
        assert lib.fs_yuv_deep_to_f32(eng.ctx, ctypes.byref(desc), mem.ptr_u8(src) + src_off, 2, 0, mem.ptr(dst) + 4 * dst_off) == 0
        got = np.array(mem.to_numpy(dst), copy=True)
        assert (got[:dst_off] == -7.0).all() and (got[dst_off + 2 * H * W * 3:] == -7.0).all()
        assert same(got[dst_off:dst_off + 2 * H * W * 3].reshape(2, H, W, 3), want_f32)
    assert same(to_f32(eng, desc, frames), want_f32)
    # fp32 -> planes
    src = mem.from_numpy(np.concatenate([[np.float32(3.0)], images.reshape(-1)]))
    aligned = mem.from_numpy(images)
    for use_aligned, dst_off in ((True, 2), (False, 0), (False, 2)):
        dst = mem.upload_u8(np.full(2 + 2 * n + 6, 0x5A, np.uint8))
        eng._sync_stream()
        p = mem.ptr(aligned) if use_aligned else mem.ptr(src) + 4
        assert lib.fs_f32_to_yuv_deep(eng.ctx, ctypes.byref(desc), p, 0, 2, mem.ptr_u8(dst) + dst_off) == 0
        got = np.array(mem.to_numpy(dst), copy=True)
        assert (got[:dst_off] == 0x5A).all() and (got[dst_off + 2 * n:] == 0x5A).all()
        assert same(got[dst_off:dst_off + 2 * n].view("<u2").reshape(2, -1), want_yuv)
    assert same(to_yuv(eng, desc, images), want_yuv)


@pytest.mark.parametrize("kind", backends.engine_params())
def test_output_floats_outside_the_scale_and_at_the_steps(kind):
    """Floats below 0, above 255, NaN and both infinities, and the values v + j / 256 -+ 1e-4 about every 8.8 step: the planes are the
    restatement's, and F >> 8 is the byte fs_f32_to_u8 writes for the same tensor."""
    eng = backends.get_engine(kind)
    mem = eng.mem
    special = np.array([-1.0, -1e-6, -0.0, 0.0, 255.0, 255.0001, 256.0, 1e9, -1e9, np.nan, np.inf, -np.inf, 254.99998, 0.0039, 0.00390625], np.float32)
    v = np.arange(0, 255, 5, dtype=np.float64)[:, None, None] + np.arange(0, 256, 17)[None, :, None] / 256.0 + np.array([-1e-4, 0.0, 1e-4])[None, None, :]
    values = np.concatenate([special, v.reshape(-1).astype(np.float32)])
    W, H = 24, -(-values.size // 24)
    flat = np.resize(values, H * W)
    img = np.stack([np.roll(flat, s) for s in (0, 1, 2)], axis=-1).reshape(1, H, W, 3).astype(np.float32)   # every value in each of the channels
    F = F_of_f32(img)
    assert F.min() == 0 and F.max() == FMAX and F[np.isnan(img)].max() == 0
    u8 = mem.upload_u8(np.full((1, H, W, 3), 0xA5, np.uint8))
    eng.f32_to_u8(mem.from_numpy(img), u8)
    assert np.array_equal(np.array(mem.to_numpy(u8)), (F >> 8).astype(np.uint8))
    for (_, hs, vs, ncomp, siting), d in ((LAYOUTS[0], 16), (LAYOUTS[4], 10), (LAYOUTS[3], 12)):
        desc = plan(eng, W, H, hs, vs, ncomp, siting, 0, 1, d)
        want = f32_to_frame(img[0], hs=hs, vs=vs, ncomp=ncomp, siting=siting, matrix=0, full_range=1, bits=d)
        assert same(to_yuv(eng, desc, img)[0], want), d
    # at full range and 16 bits a grey F maps to Y = F * 65535 / 65280 rounded: the 8.8 steps stay apart
    grey = np.repeat((np.arange(0, 4096, dtype=np.float32) / np.float32(256)).reshape(1, 64, 64, 1), 3, axis=3)
    Y = to_yuv(eng, plan(eng, 64, 64, 1, 1, 1, 0, 0, 1, 16), grey)[0].astype(np.int64)
    assert np.abs(Y - np.arange(4096) * 65535.0 / 65280.0).max() <= 0.5 + 1e-3 and (np.diff(Y) >= 1).all()


@pytest.mark.parametrize("kind", backends.engine_params())
def test_known_answers(kind):
    eng = backends.get_engine(kind)
    # limited range, 10 bits: black 64, white 940, the middle 502 = 127.5 exactly; chroma 512
    assert fix24(constants(0, 0, 10)[3]) == 1250247329
    ycc = np.array([[64, 512, 512], [940, 512, 512], [502, 512, 512]], np.uint16)
    for matrix in (0, 1):
        desc = plan(eng, 3, 1, 1, 1, 3, 0, matrix, 0, 10)
        got = to_f32(eng, desc, np.ascontiguousarray(ycc.T).reshape(1, -1))[0, 0]
        assert same(got, np.repeat(np.array([0.0, 255.0, 127.5], np.float32)[:, None], 3, axis=1))
        assert np.array_equal(ycc_to_F(ycc[:, 0], ycc[:, 1], ycc[:, 2], matrix, 0, 10), np.repeat(np.array([[0], [65280], [32640]]), 3, axis=1))
        back = to_yuv(eng, desc, np.repeat(np.array([0.0, 255.0, 127.5], np.float32)[None, None, :, None], 3, axis=3))
        assert np.array_equal(back[0].reshape(3, 3).T, ycc)
    # below black and above white clamp
    desc = plan(eng, 2, 1, 1, 1, 1, 0, 0, 0, 10)
    assert same(to_f32(eng, desc, np.array([[0, 1023]], np.uint16))[0, 0], np.array([[0.0] * 3, [255.0] * 3], np.float32))
    # full range, 16 bits: Y = 257 v is exactly F = 256 v
    v = np.arange(256, dtype=np.int64)
    assert np.array_equal(ycc_to_F(257 * v, np.full(256, 2 ** 15), np.full(256, 2 ** 15), 1, 1, 16), np.repeat((256 * v)[:, None], 3, axis=1))
    got = to_f32(eng, plan(eng, 16, 16, 1, 1, 1, 0, 1, 1, 16), (257 * v).astype(np.uint16)[None])[0]
    assert same(got, np.repeat(v.astype(np.float32).reshape(16, 16, 1), 3, axis=2))


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("d", DEPTHS)
def test_eight_bit_samples_shifted_up_agree_with_the_eight_bit_kernel(kind, d):
    """A d-bit 4:4:4 limited-range stream whose samples are 8-bit samples << (d - 8): (F + 128) >> 8 is within 1 of the 8-bit kernel's byte."""
    eng = backends.get_engine(kind)
    W, H = 64, 48
    for matrix in (0, 1):
        f8 = T8.yuv_frames(W, H, 1, 1, 3)
        u8 = T8.to_rgb(eng, T8.plan(eng, W, H, 1, 1, 3, 0, matrix, 0), f8).astype(np.int64)
        f32 = to_f32(eng, plan(eng, W, H, 1, 1, 3, 0, matrix, 0, d), f8.astype(np.uint16) << (d - 8))
        F = (f32.astype(np.float64) * 256.0).astype(np.int64)
        assert np.abs(((F + 128) >> 8) - u8).max() <= 1


_cube = {}


def cube(top, seed):
    key = (top, seed)
    if key not in _cube:
        _cube[key] = np.random.RandomState(seed).randint(0, top + 1, size=(2 ** 20, 3)).astype(np.int64)
        _cube[key].setflags(write=False)
    return _cube[key]


@pytest.mark.parametrize("d", DEPTHS)
def test_fixed_point_matrices_are_within_one_of_float64(d):
    """The restatement alone, 2^20 random triples per depth, matrix and range, both directions: within 1 of floor(exact + 0.5) of the float64
    formulas and equal in at least 99.7 % of the samples (measured: 99.85 % and above).  The cap keeps a wrong coefficient from hiding inside
    the tolerance."""
    for matrix, full in COLOURS:
        s = cube(2 ** d - 1, 11)
        diff = np.abs(ycc_to_F(s[:, 0], s[:, 1], s[:, 2], matrix, full, d) - ycc_to_F_exact(s[:, 0], s[:, 1], s[:, 2], matrix, full, d))
        print("d %d planes->F matrix %d full %d: max |diff| %d, equal %.4f %%" % (d, matrix, full, diff.max(), 100.0 * (diff == 0).mean()))
        assert diff.max() <= 1 and (diff == 0).mean() >= 0.997
        s = cube(FMAX, 13)
        diff = np.abs(np.stack(F_to_ycc(s, matrix, full, d)) - np.stack(F_to_ycc_exact(s, matrix, full, d)))
        print("d %d F->planes matrix %d full %d: max |diff| %d, equal %.4f %%" % (d, matrix, full, diff.max(), 100.0 * (diff == 0).mean()))
        assert diff.max() <= 1 and (diff == 0).mean() >= 0.997


@pytest.mark.parametrize("kind", backends.engine_params())
def test_device_call_refusals_leave_the_destination_untouched(kind):
    eng = backends.get_engine(kind)
    lib, mem = eng.lib, eng.mem
    W, H, d = 17, 31, 10
    desc = plan(eng, W, H, 2, 2, 3, 1, 0, 0, d)
    desc8 = T8.plan(eng, W, H, 2, 2, 3, 1, 0, 0)
    n = int(desc.frame_bytes)
    guard = 16
    frame = as_bytes(deep_frames(W, H, 2, 2, 3, d)[:1]).reshape(-1)
    yuv = mem.upload_u8(np.concatenate([np.full(guard, 0x5A, np.uint8), frame, np.full(guard, 0x5A, np.uint8)]))
    f32 = mem.from_numpy(np.concatenate([np.full(guard, -7.0, np.float32), f32_images(W, H)[0].reshape(-1), np.full(guard, -7.0, np.float32)]))
    u8 = mem.upload_u8(np.full(guard + H * W * 4 + guard, 0x5A, np.uint8))
    yuv0, f320, u80 = (np.array(mem.to_numpy(t), copy=True) for t in (yuv, f32, u8))
    p_yuv, p_f32, p_u8 = mem.ptr_u8(yuv) + guard, mem.ptr(f32) + 4 * guard, mem.ptr_u8(u8) + guard
    good, eight = ctypes.byref(desc), ctypes.byref(desc8)

    def copy_of(**changes):
        c = L.fs_yuv_desc.from_buffer_copy(desc)
        for k, v in changes.items():
            setattr(c, k, v)
        return ctypes.byref(c)

    def bits_of(b):
        c = L.fs_yuv_desc.from_buffer_copy(desc)
        c.reserved[0] = b
        return ctypes.byref(c)

    edited = [copy_of(width=W + 1), copy_of(height=0), copy_of(hs=4), copy_of(ncomp=2), copy_of(siting=2), copy_of(matrix=3), copy_of(full_range=-1),
              copy_of(chroma_w=desc.chroma_w + 1), copy_of(frame_bytes=n + 2), copy_of(frame_bytes=n // 2), copy_of(frame_bytes=0),
              bits_of(8), bits_of(17), bits_of(0), bits_of(-10), eight]
    # (ctx, desc, yuv, N, swap_rb, dst)
    to_f32_calls = [((None, good, p_yuv, 1, 0, p_f32), -1), ((eng.ctx, None, p_yuv, 1, 0, p_f32), -1), ((eng.ctx, good, None, 1, 0, p_f32), -1),
                    ((eng.ctx, good, p_yuv, 1, 0, None), -1), ((eng.ctx, good, p_yuv, 0, 0, p_f32), -1), ((eng.ctx, good, p_yuv, -1, 0, p_f32), -1),
                    ((eng.ctx, good, p_yuv, 65536, 0, p_f32), -1), ((eng.ctx, good, p_yuv + 1, 1, 0, p_f32), -5)] + \
        [((eng.ctx, e, p_yuv, 1, 0, p_f32), -1) for e in edited]
    # (ctx, desc, src, swap_rb, N, yuv)
    to_yuv_calls = [((None, good, p_f32, 0, 1, p_yuv), -1), ((eng.ctx, None, p_f32, 0, 1, p_yuv), -1), ((eng.ctx, good, None, 0, 1, p_yuv), -1),
                    ((eng.ctx, good, p_f32, 0, 1, None), -1), ((eng.ctx, good, p_f32, 0, 0, p_yuv), -1), ((eng.ctx, good, p_f32, 0, 65536, p_yuv), -1),
                    ((eng.ctx, good, p_f32, 0, 1, p_yuv + 1), -5)] + \
        [((eng.ctx, e, p_f32, 0, 1, p_yuv), -1) for e in edited]
    eng._sync_stream()
    for args, code in to_f32_calls:
        assert lib.fs_yuv_deep_to_f32(*args) == code, args
        assert lib.fs_last_error().startswith(b"fs_yuv_deep_to_f32")
    for args, code in to_yuv_calls:
        assert lib.fs_f32_to_yuv_deep(*args) == code, args
        assert lib.fs_last_error().startswith(b"fs_f32_to_yuv_deep")
    # a deep desc handed to the 8-bit calls
    for pb in (3, 4):
        assert lib.fs_yuv_to_rgb_u8(eng.ctx, good, p_yuv, 1, pb, 0, p_u8) == -1
        assert lib.fs_rgb_to_yuv_u8(eng.ctx, good, p_u8, pb, 0, 1, p_yuv) == -1
    with pytest.raises(L.FaststyleError):                                              # the engine's own shape checks
        eng.yuv_deep_to_f32(mem.upload_u8(np.zeros(n + 2, np.uint8)), desc, mem.from_numpy(np.zeros((H, W, 3), np.float32)))
    with pytest.raises(L.FaststyleError):
        eng.f32_to_yuv_deep(mem.from_numpy(np.zeros((H, W, 4), np.float32)), desc, mem.upload_u8(np.zeros(n, np.uint8)))
    with pytest.raises(L.FaststyleError):
        eng.yuv_deep_to_f32(mem.upload_u8(np.zeros(n // 2, np.uint8)), desc8, mem.from_numpy(np.zeros((H, W, 3), np.float32)))
    for t, t0 in ((yuv, yuv0), (f32, f320), (u8, u80)):
        assert same(np.array(mem.to_numpy(t)), t0)
    # and the same buffers work when asked properly, writing nothing outside their frame
    kw = dict(hs=2, vs=2, ncomp=3, siting=1, matrix=0, full_range=0, bits=d)
    assert lib.fs_f32_to_yuv_deep(eng.ctx, good, p_f32, 0, 1, p_yuv) == 0
    got = np.array(mem.to_numpy(yuv), copy=True)
    assert (got[:guard] == 0x5A).all() and (got[-guard:] == 0x5A).all()
    assert same(got[guard:-guard].view("<u2"), f32_to_frame(f32_images(W, H)[0], **kw))
    yuv = mem.upload_u8(yuv0)
    assert lib.fs_yuv_deep_to_f32(eng.ctx, good, mem.ptr_u8(yuv) + guard, 1, 0, p_f32) == 0
    got = np.array(mem.to_numpy(f32), copy=True)
    assert (got[:guard] == -7.0).all() and (got[-guard:] == -7.0).all()
    assert same(got[guard:-guard].reshape(H, W, 3), frame_to_f32(deep_frames(W, H, 2, 2, 3, d)[0], W, H, **kw))
