"""Planar YCbCr <-> RGB on the device (csrc/fs_yuv.hip) against its contract, the arithmetic that include/faststyle_io.h states.  The first half
of this file is an independent numpy restatement of that text, written case by case (not in the kernels' common-denominator form), plus the
float64 formulas the fixed-point matrix approximates; every comparison with the restatement is exact.  The same bodies run on the CPU emulator
and, under -m gpu, on the MI355X.  tests/test_video_stream.py builds its expected frames with the restatement."""
import ctypes
import itertools
import math

import numpy as np
import pytest
from PIL import Image

from faststyle_amd import _lib as L, engine as fsengine
from tests import backends


def constants(matrix, full_range):
    Kr, Kb = (0.2126, 0.0722) if matrix else (0.299, 0.114)
    Kg = 1.0 - Kr - Kb
    sy, sc, oy = (1.0, 1.0, 0) if full_range else (255.0 / 219.0, 255.0 / 224.0, 16)
    return Kr, Kb, Kg, sy, sc, oy


def fix16(c):
    return int(math.floor(c * 65536.0 + 0.5))


def geometry(W, H, hs, vs, ncomp):
    """(chroma width, chroma height, frame bytes)"""
    if ncomp == 1:
        return 0, 0, W * H
    cw, ch = -(-W // hs), -(-H // vs)
    return cw, ch, W * H + 2 * cw * ch


def split(planes, W, H, hs, vs, ncomp):
    cw, ch, n = geometry(W, H, hs, vs, ncomp)
    planes = np.asarray(planes, np.uint8).reshape(-1)
    assert planes.size == n
    y = planes[:W * H].reshape(H, W)
    if ncomp == 1:
        return y, None, None
    return y, planes[W * H:W * H + cw * ch].reshape(ch, cw), planes[W * H + cw * ch:].reshape(ch, cw)


# ---------------------------------------------------------------- chroma resampling
def upsample(c, H, W, hs, vs, siting):
    """Chroma plane [ch, cw] -> one value per pixel [H, W] (int64)."""
    c = c.astype(np.int64)
    ch, cw = c.shape
    x, y = np.arange(W), np.arange(H)
    if hs == 1:
        return c.copy()
    xn = x // 2
    xf = np.clip(np.where(x & 1, xn + 1, xn - 1), 0, cw - 1)       # centre siting: the neighbour on the pixel's side
    xr = np.clip(xn + 1, 0, cw - 1)                                # co-sited: the right neighbour of an odd column
    odd = (x & 1).astype(bool)[None, :]
    if vs == 1:
        if siting == 0:
            return (3 * c[:, xn] + c[:, xf] + 2) >> 2
        return np.where(odd, (c[:, xn] + c[:, xr] + 1) >> 1, c[:, xn])
    yn = y // 2
    yf = np.clip(np.where(y & 1, yn + 1, yn - 1), 0, ch - 1)
    near, far = c[yn], c[yf]
    if siting == 0:
        return (9 * near[:, xn] + 3 * near[:, xf] + 3 * far[:, xn] + far[:, xf] + 8) >> 4
    even_col = (3 * near[:, xn] + far[:, xn] + 2) >> 2
    odd_col = (3 * near[:, xn] + 3 * near[:, xr] + far[:, xn] + far[:, xr] + 4) >> 3
    return np.where(odd, odd_col, even_col)


def downsample(p, hs, vs, siting):
    """Per-pixel u8 chroma [H, W] -> chroma plane [ceil(H / vs), ceil(W / hs)] (int64)."""
    p = p.astype(np.int64)
    H, W = p.shape
    if hs == 1:
        return p.copy()
    cw, ch = -(-W // hs), -(-H // vs)
    m = 2 * np.arange(cw)
    left, right = np.clip(m - 1, 0, W - 1), np.clip(m + 1, 0, W - 1)
    if vs == 1:
        if siting == 0:
            return (p[:, m] + p[:, right] + 1) >> 1
        return (p[:, left] + 2 * p[:, m] + p[:, right] + 2) >> 2
    r0 = 2 * np.arange(ch)
    r1 = np.clip(r0 + 1, 0, H - 1)
    top, bottom = p[r0], p[r1]
    if siting == 0:
        return (top[:, m] + top[:, right] + bottom[:, m] + bottom[:, right] + 2) >> 2
    return (top[:, left] + 2 * top[:, m] + top[:, right] + bottom[:, left] + 2 * bottom[:, m] + bottom[:, right] + 4) >> 3


# ---------------------------------------------------------------- the fixed-point matrices
def ycc_to_rgb_fixed(Y, Cb, Cr, matrix, full_range):
    """int arrays of equal shape -> uint8 [..., 3] (R, G, B)"""
    Kr, Kb, Kg, sy, sc, oy = constants(matrix, full_range)
    cy = fix16(sy)
    r_cr, b_cb = fix16(2.0 * (1.0 - Kr) * sc), fix16(2.0 * (1.0 - Kb) * sc)
    g_cb, g_cr = fix16(-(2.0 * (1.0 - Kb) * Kb / Kg * sc)), fix16(-(2.0 * (1.0 - Kr) * Kr / Kg * sc))
    Y, u, v = Y.astype(np.int64) - oy, Cb.astype(np.int64) - 128, Cr.astype(np.int64) - 128
    sums = [cy * Y + r_cr * v, cy * Y + g_cb * u + g_cr * v, cy * Y + b_cb * u]
    assert all(np.abs(s).max() < 2 ** 31 - 32768 for s in sums)                   # (the kernels sum in int32)
    return np.stack([np.clip((s + 32768) >> 16, 0, 255) for s in sums], axis=-1).astype(np.uint8)


def rgb_to_ycc_fixed(rgb, matrix, full_range):
    """uint8 [..., 3] -> (Y, Cb, Cr) int64 arrays in [0, 255]"""
    Kr, Kb, Kg, sy, sc, oy = constants(matrix, full_range)
    rows = [([Kr / sy, Kg / sy, Kb / sy], oy),
            ([-Kr / (2.0 * (1.0 - Kb)) / sc, -Kg / (2.0 * (1.0 - Kb)) / sc, (1.0 - Kb) / (2.0 * (1.0 - Kb)) / sc], 128),
            ([(1.0 - Kr) / (2.0 * (1.0 - Kr)) / sc, -Kg / (2.0 * (1.0 - Kr)) / sc, -Kb / (2.0 * (1.0 - Kr)) / sc], 128)]
    p = rgb.astype(np.int64)
    out = []
    for coef, off in rows:
        s = sum(fix16(c) * p[..., k] for k, c in enumerate(coef)) + (off << 16) + 32768
        assert s.max() < 2 ** 31
        out.append(np.clip(s >> 16, 0, 255))
    return out


# ---------------------------------------------------------------- the float64 formulas
def ycc_to_rgb_exact(Y, Cb, Cr, matrix, full_range):
    Kr, Kb, Kg, sy, sc, oy = constants(matrix, full_range)
    Y, u, v = sy * (Y.astype(np.float64) - oy), sc * (Cb.astype(np.float64) - 128.0), sc * (Cr.astype(np.float64) - 128.0)
    R = Y + 2.0 * (1.0 - Kr) * v
    B = Y + 2.0 * (1.0 - Kb) * u
    G = Y - 2.0 * (1.0 - Kb) * Kb / Kg * u - 2.0 * (1.0 - Kr) * Kr / Kg * v
    return np.clip(np.floor(np.stack([R, G, B], axis=-1) + 0.5), 0, 255).astype(np.uint8)


def rgb_to_ycc_exact(rgb, matrix, full_range):
    Kr, Kb, Kg, sy, sc, oy = constants(matrix, full_range)
    R, G, B = (rgb[..., k].astype(np.float64) for k in range(3))
    Yl = Kr * R + Kg * G + Kb * B
    Y = Yl / sy + oy
    Cb = (B - Yl) / (2.0 * (1.0 - Kb)) / sc + 128.0
    Cr = (R - Yl) / (2.0 * (1.0 - Kr)) / sc + 128.0
    return [np.clip(np.floor(v + 0.5), 0, 255).astype(np.int64) for v in (Y, Cb, Cr)]


# ---------------------------------------------------------------- whole frames
def frame_to_rgb(planes, W, H, hs=2, vs=2, ncomp=3, siting=0, matrix=0, full_range=0):
    """One frame's planes (flat uint8) -> uint8 [H, W, 3]"""
    y, cb, cr = split(planes, W, H, hs, vs, ncomp)
    if ncomp == 1:
        u = v = np.full((H, W), 128, np.int64)
    else:
        u, v = upsample(cb, H, W, hs, vs, siting), upsample(cr, H, W, hs, vs, siting)
    return ycc_to_rgb_fixed(y, u, v, matrix, full_range)


def rgb_to_frame(rgb, hs=2, vs=2, ncomp=3, siting=0, matrix=0, full_range=0):
    """uint8 [H, W, 3] -> one frame's planes (flat uint8)"""
    Y, Cb, Cr = rgb_to_ycc_fixed(rgb, matrix, full_range)
    parts = [Y]
    if ncomp == 3:
        parts += [downsample(Cb, hs, vs, siting), downsample(Cr, hs, vs, siting)]
    return np.concatenate([p.reshape(-1) for p in parts]).astype(np.uint8)


# ================================================================ the tests
# (name, hs, vs, ncomp, siting)
LAYOUTS = [("444", 1, 1, 3, 0), ("444_cosited", 1, 1, 3, 1), ("422_centre", 2, 1, 3, 0), ("422_cosited", 2, 1, 3, 1),
           ("420_centre", 2, 2, 3, 0), ("420_cosited", 2, 2, 3, 1), ("mono", 1, 1, 1, 0)]
LAYOUT_PARAMS = [pytest.param(*l[1:], id=l[0]) for l in LAYOUTS]
SIZES = [(1, 1), (2, 2), (3, 5), (17, 31), (64, 48)]             # (W, H): odd chroma extents, one-sample chroma rows and columns, all four edges; the
#                                                                 last is three blocks and takes the dword path
COLOURS = list(itertools.product((0, 1), (0, 1)))               # (matrix, full_range)

_host = {}


def host_lib():
    """The library's host calls without an engine: the emulator build holds the same host code as the product."""
    if "h" not in _host:
        from tests import emu_lib
        _host["h"] = fsengine.YuvHost(lib=L.bind(ctypes.CDLL(emu_lib.build_emu())))
    return _host["h"]


def pattern(kind, shape, seed):
    """uint8 content of a plane or an image: noise, a 0 | 255 checkerboard, a ramp"""
    if kind == "noise":
        return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)
    idx = np.indices(shape)
    if kind == "checker":
        return ((idx.sum(axis=0) + seed) & 1).astype(np.uint8) * 255
    return ((idx[0] * 7 + idx[1] * 13 + idx[-1] * 29 * (len(shape) > 2) + seed) % 256).astype(np.uint8)


_cases = {}


def yuv_frames(W, H, hs, vs, ncomp):
    """Three frames of one geometry (noise, checkerboard, ramp in every plane), computed once: uint8 [3, frame_bytes]"""
    key = ("yuv", W, H, hs, vs, ncomp)
    if key not in _cases:
        cw, ch, _ = geometry(W, H, hs, vs, ncomp)
        frames = []
        for k, kind in enumerate(("noise", "checker", "ramp")):
            planes = [pattern(kind, (H, W), 3 * k)] + ([pattern(kind, (ch, cw), 3 * k + 1), pattern(kind, (ch, cw), 3 * k + 2)] if ncomp == 3 else [])
            frames.append(np.concatenate([p.reshape(-1) for p in planes]))
        _cases[key] = np.stack(frames)
        _cases[key].setflags(write=False)
    return _cases[key]


def rgb_images(W, H):
    key = ("rgb", W, H)
    if key not in _cases:
        _cases[key] = np.stack([pattern(kind, (H, W, 3), 5 * k) for k, kind in enumerate(("noise", "checker", "ramp"))])
        _cases[key].setflags(write=False)
    return _cases[key]


def want_rgb(W, H, hs, vs, ncomp, siting, matrix, full):
    key = ("want_rgb", W, H, hs, vs, ncomp, siting, matrix, full)
    if key not in _cases:
        _cases[key] = np.stack([frame_to_rgb(f, W, H, hs, vs, ncomp, siting, matrix, full) for f in yuv_frames(W, H, hs, vs, ncomp)])
        _cases[key].setflags(write=False)
    return _cases[key]


def want_yuv(W, H, hs, vs, ncomp, siting, matrix, full):
    key = ("want_yuv", W, H, hs, vs, ncomp, siting, matrix, full)
    if key not in _cases:
        _cases[key] = np.stack([rgb_to_frame(im, hs, vs, ncomp, siting, matrix, full) for im in rgb_images(W, H)])
        _cases[key].setflags(write=False)
    return _cases[key]


def plan(eng, W, H, hs, vs, ncomp, siting, matrix, full):
    return eng.yuv_plan(W, H, sampling=(hs, vs), siting=siting, matrix=matrix, full_range=full, components=ncomp)


def to_rgb(eng, desc, frames, pb=3, swap=False):
    """frames: host uint8 [N, frame_bytes] -> host [N, H, W, pb] of the device call"""
    frames = np.ascontiguousarray(frames)
    out = eng.mem.upload_u8(np.full((frames.shape[0], desc.height, desc.width, pb), 0xA5, np.uint8))
    eng.yuv_to_rgb_u8(eng.mem.upload_u8(frames), desc, out, swap_rb=swap)
    return np.array(eng.mem.to_numpy(out), copy=True)


def to_yuv(eng, desc, images, swap=False):
    """images: host uint8 [N, H, W, 3 | 4] -> host [N, frame_bytes] of the device call"""
    images = np.ascontiguousarray(images)
    out = eng.mem.upload_u8(np.full((images.shape[0], int(desc.frame_bytes)), 0xA5, np.uint8))
    eng.rgb_to_yuv_u8(eng.mem.upload_u8(images), desc, out, swap_rb=swap)
    return np.array(eng.mem.to_numpy(out), copy=True)


def rgbx(images, poison=0xEE):
    x = np.full(images.shape[:-1] + (1,), poison, np.uint8)
    x[..., ::2, 0] = 0x11
    return np.concatenate([images, x], axis=-1)


def test_plan_reports_the_y4m_layout():
    h = host_lib()
    for _, hs, vs, ncomp, siting in LAYOUTS:
        for W, H in SIZES:
            d = h.yuv_plan(W, H, sampling=(hs, vs), siting=siting, matrix=1, full_range=True, components=ncomp)
            cw, ch, n = geometry(W, H, hs, vs, ncomp)
            assert (d.width, d.height, d.hs, d.vs, d.ncomp, d.siting, d.matrix, d.full_range) == (W, H, hs, vs, ncomp, siting, 1, 1)
            assert (d.chroma_w, d.chroma_h, d.frame_bytes) == (cw, ch, n)
            assert list(d.plane_bytes) == [W * H, cw * ch, cw * ch]
            assert list(d.plane_offset) == ([0, W * H, W * H + cw * ch] if ncomp == 3 else [0, 0, 0])
    assert ctypes.sizeof(L.fs_yuv_desc) == 104
    assert h.yuv_plan(8, 8, matrix="bt709").matrix == 1 and h.yuv_plan(8, 8, matrix="bt601").matrix == 0


@pytest.mark.parametrize("kind", backends.engine_params())
def test_fixed_point_coefficients(kind):
    """BT.601 limited range: the luma coefficient the contract names and the classic 16-bit set around it; every row's sum; and the library's own
    coefficients, read off single pixels that isolate them."""
    eng = backends.get_engine(kind)
    Kr, Kb, Kg, sy, sc, oy = constants(0, 0)
    assert fix16(sy) == 76309 and oy == 16
    assert (fix16(2 * (1 - Kr) * sc), fix16(2 * (1 - Kb) * sc)) == (104597, 132201)
    grey = np.array([[255, 255, 255], [0, 0, 0], [77, 77, 77]], np.uint8)
    for matrix, full in COLOURS:                       # a grey pixel has no chroma, white is the top of the range: the rows sum to 0 and to 1 / sy
        Y, Cb, Cr = rgb_to_ycc_fixed(grey, matrix, full)
        assert list(Cb) == [128] * 3 and list(Cr) == [128] * 3 and list(Y[:2]) == ([255, 0] if full else [235, 16])
        desc = plan(eng, 3, 1, 1, 1, 3, 0, matrix, full)
        assert np.array_equal(to_yuv(eng, desc, grey[None, None])[0].reshape(3, 3), np.stack([Y, Cb, Cr]))
    # one step of one input at a time from mid-scale, where nothing clamps: the library's output moves as the stated coefficient says.  The probes
    # (Y, Cb, Cr) are 128 with one component raised by 100; the expected pixel is written out from the coefficients, not through the restatement
    desc = plan(eng, 4, 1, 1, 1, 3, 0, 0, 0)
    probes = np.array([[128, 128, 128], [228, 128, 128], [128, 228, 128], [128, 128, 228]], np.uint8)
    got = to_rgb(eng, desc, np.ascontiguousarray(probes.T).reshape(1, -1))[0, 0].astype(int)
    base = 76309 * (128 - 16) + 32768
    g_cb, g_cr = fix16(-(2 * (1 - Kb) * Kb / Kg * sc)), fix16(-(2 * (1 - Kr) * Kr / Kg * sc))
    assert (g_cb, g_cr) == (-25675, -53279)
    want = [[base >> 16] * 3, [(base + 76309 * 100) >> 16] * 3,
            [base >> 16, (base + g_cb * 100) >> 16, (base + 132201 * 100) >> 16],
            [(base + 104597 * 100) >> 16, (base + g_cr * 100) >> 16, base >> 16]]
    assert np.array_equal(got, np.clip(want, 0, 255))


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("hs,vs,ncomp,siting", LAYOUT_PARAMS)
def test_yuv_to_rgb_equals_the_restatement(kind, hs, vs, ncomp, siting):
    eng = backends.get_engine(kind)
    for (W, H), (matrix, full) in itertools.product(SIZES, COLOURS):
        desc = plan(eng, W, H, hs, vs, ncomp, siting, matrix, full)
        frames, want = yuv_frames(W, H, hs, vs, ncomp), want_rgb(W, H, hs, vs, ncomp, siting, matrix, full)
        where = (W, H, matrix, full)
        assert np.array_equal(to_rgb(eng, desc, frames[:2]), want[:2]), where                  # a batch of two
        got = to_rgb(eng, desc, frames[2:], pb=4, swap=True)                                   # one frame, RGBX, written B,G,R
        assert np.array_equal(got[..., :3], want[2:, :, :, ::-1]) and (got[..., 3] == 255).all(), where
        if (matrix, full) == (0, 0):                                                           # the other two combinations of pixel size and swap
            assert np.array_equal(to_rgb(eng, desc, frames[1:], swap=True), want[1:, :, :, ::-1]), where
            got = to_rgb(eng, desc, frames[:2], pb=4)
            assert np.array_equal(got[..., :3], want[:2]) and (got[..., 3] == 255).all(), where


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("hs,vs,ncomp,siting", LAYOUT_PARAMS)
def test_rgb_to_yuv_equals_the_restatement(kind, hs, vs, ncomp, siting):
    eng = backends.get_engine(kind)
    for (W, H), (matrix, full) in itertools.product(SIZES, COLOURS):
        desc = plan(eng, W, H, hs, vs, ncomp, siting, matrix, full)
        images, want = rgb_images(W, H), want_yuv(W, H, hs, vs, ncomp, siting, matrix, full)
        where = (W, H, matrix, full)
        assert np.array_equal(to_yuv(eng, desc, images[:2]), want[:2]), where
        assert np.array_equal(to_yuv(eng, desc, rgbx(images[2:, :, :, ::-1]), swap=True), want[2:]), where     # one image, B,G,R,X with a poisoned X
        if (matrix, full) == (0, 0):
            assert np.array_equal(to_yuv(eng, desc, np.ascontiguousarray(images[1:, :, :, ::-1]), swap=True), want[1:]), where
            assert np.array_equal(to_yuv(eng, desc, rgbx(images[:2])), want[:2]), where


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("hs,vs,ncomp,siting", [pytest.param(*l[1:], id=l[0]) for l in LAYOUTS if l[0] in ("444", "420_centre", "420_cosited", "mono")])
def test_misaligned_buffers_take_the_byte_path_with_the_same_values(kind, hs, vs, ncomp, siting):
    """64 x 48 is eligible for dword loads and stores; the same buffers one byte further are not, and give the same values."""
    eng = backends.get_engine(kind)
    lib, mem = eng.lib, eng.mem
    W, H = 64, 48
    desc = plan(eng, W, H, hs, vs, ncomp, siting, 0, 0)
    n = int(desc.frame_bytes)
    frames, images = yuv_frames(W, H, hs, vs, ncomp)[:2], rgb_images(W, H)[:2]
    src = mem.upload_u8(np.concatenate([[0x33], frames.reshape(-1)]).astype(np.uint8))
    dst = mem.upload_u8(np.full(1 + 2 * H * W * 3 + 3, 0x5A, np.uint8))
    eng._sync_stream()
    assert lib.fs_yuv_to_rgb_u8(eng.ctx, ctypes.byref(desc), mem.ptr_u8(src) + 1, 2, 3, 0, mem.ptr_u8(dst) + 1) == 0
    got = np.array(mem.to_numpy(dst), copy=True)
    assert got[0] == 0x5A and (got[-3:] == 0x5A).all()
    assert np.array_equal(got[1:-3].reshape(2, H, W, 3), want_rgb(W, H, hs, vs, ncomp, siting, 0, 0)[:2])
    src = mem.upload_u8(np.concatenate([[0x33], images.reshape(-1)]).astype(np.uint8))
    dst = mem.upload_u8(np.full(1 + 2 * n + 3, 0x5A, np.uint8))
    assert lib.fs_rgb_to_yuv_u8(eng.ctx, ctypes.byref(desc), mem.ptr_u8(src) + 1, 3, 0, 2, mem.ptr_u8(dst) + 1) == 0
    got = np.array(mem.to_numpy(dst), copy=True)
    assert got[0] == 0x5A and (got[-3:] == 0x5A).all()
    assert np.array_equal(got[1:-3].reshape(2, n), want_yuv(W, H, hs, vs, ncomp, siting, 0, 0)[:2])


_cube = {}


def cube_sample():
    """2^20 random triples as a 1024 x 1024 4:4:4 image, shared by every configuration"""
    if "s" not in _cube:
        _cube["s"] = np.random.RandomState(7).randint(0, 256, size=(1024, 1024, 3)).astype(np.uint8)
        _cube["s"].setflags(write=False)
    return _cube["s"]


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("matrix,full", [pytest.param(m, f, id="%s_%s" % (("bt601", "bt709")[m], ("limited", "full")[f])) for m, f in COLOURS])
def test_fixed_point_matrix_is_within_one_of_float64(kind, matrix, full):
    """Both directions on 2^20 random triples: within 1 of floor(exact + 0.5) of the float64 formulas and equal in at least 99.8 % of the samples
    (99.899 % over the whole 2^24 cube): the cap keeps a wrong coefficient from hiding inside the tolerance."""
    eng = backends.get_engine(kind)
    s = cube_sample()
    H, W = s.shape[:2]
    desc = plan(eng, W, H, 1, 1, 3, 0, matrix, full)
    planes = np.ascontiguousarray(s.transpose(2, 0, 1)).reshape(1, -1)                  # the triples as (Y, Cb, Cr) planes
    got = to_rgb(eng, desc, planes)[0].astype(np.int64)
    exact = ycc_to_rgb_exact(s[..., 0], s[..., 1], s[..., 2], matrix, full).astype(np.int64)
    diff = np.abs(got - exact)
    print("yuv->rgb matrix %d full %d: max |diff| %d, equal %.4f %%" % (matrix, full, diff.max(), 100.0 * (diff == 0).mean()))
    assert diff.max() <= 1 and (diff == 0).mean() >= 0.998
    got = to_yuv(eng, desc, s[None])[0].reshape(3, H, W).astype(np.int64)                # the triples as (R, G, B) pixels
    exact = np.stack(rgb_to_ycc_exact(s, matrix, full))
    diff = np.abs(got - exact)
    print("rgb->yuv matrix %d full %d: max |diff| %d, equal %.4f %%" % (matrix, full, diff.max(), 100.0 * (diff == 0).mean()))
    assert diff.max() <= 1 and (diff == 0).mean() >= 0.998


@pytest.mark.parametrize("kind", backends.engine_params())
def test_bt601_full_range_is_within_one_of_pil(kind):
    eng = backends.get_engine(kind)
    s = cube_sample()[:256, :256]
    H, W = s.shape[:2]
    desc = plan(eng, W, H, 1, 1, 3, 0, 0, 1)
    got = to_rgb(eng, desc, np.ascontiguousarray(s.transpose(2, 0, 1)).reshape(1, -1))[0]
    pil = np.asarray(Image.fromarray(s, "YCbCr").convert("RGB"))
    assert np.abs(got.astype(int) - pil.astype(int)).max() <= 1
    got = to_yuv(eng, desc, s[None])[0].reshape(3, H, W).transpose(1, 2, 0)
    pil = np.asarray(Image.fromarray(s, "RGB").convert("YCbCr"))
    assert np.abs(got.astype(int) - pil.astype(int)).max() <= 1


KNOWN = [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)), ((81, 90, 240), (255, 0, 0)), ((145, 54, 34), (0, 255, 0)),
         ((41, 240, 110), (0, 0, 255))]


@pytest.mark.parametrize("kind", backends.engine_params())
def test_known_answers_bt601_limited(kind):
    eng = backends.get_engine(kind)
    ycc = np.array([k[0] for k in KNOWN], np.uint8)
    rgb = np.array([k[1] for k in KNOWN], np.uint8)
    desc = plan(eng, len(KNOWN), 1, 1, 1, 3, 0, 0, 0)
    back = to_yuv(eng, desc, rgb[None, None])[0].reshape(3, len(KNOWN)).T
    assert np.array_equal(back, ycc)                                                    # RGB -> YCbCr: the five named triples, exactly
    got = to_rgb(eng, desc, np.ascontiguousarray(ycc.T).reshape(1, -1))[0, 0]
    assert np.array_equal(got[:2], rgb[:2])                                             # the reverse: black and white exactly,
    assert np.abs(got.astype(int) - rgb.astype(int)).max() <= 1                         # the primaries within 1: their YCbCr triples are rounded themselves


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("hs,vs,ncomp,siting", [pytest.param(*l[1:], id=l[0]) for l in LAYOUTS if l[3] == 3 and l[1] == 2])
def test_constant_chroma_stays_constant(kind, hs, vs, ncomp, siting):
    eng = backends.get_engine(kind)
    W, H = 17, 31
    cw, ch, n = geometry(W, H, hs, vs, ncomp)
    for cb, cr in ((0, 255), (255, 0), (77, 201)):
        frame = np.concatenate([np.full(W * H, 120, np.uint8), np.full(cw * ch, cb, np.uint8), np.full(cw * ch, cr, np.uint8)])
        assert (upsample(split(frame, W, H, hs, vs, 3)[1], H, W, hs, vs, siting) == cb).all()
        got = to_rgb(eng, plan(eng, W, H, hs, vs, 3, siting, 0, 1), frame[None])[0]
        assert (got == got[0, 0]).all() and np.array_equal(got[0, 0], ycc_to_rgb_fixed(np.array(120), np.array(cb), np.array(cr), 0, 1))


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("hs,vs,ncomp,siting", LAYOUT_PARAMS)
def test_grey_ramp_round_trip_is_the_identity_at_full_range(kind, hs, vs, ncomp, siting):
    eng = backends.get_engine(kind)
    W, H = 32, 8
    grey = np.repeat(np.arange(256, dtype=np.uint8).reshape(H, W)[:, :, None], 3, axis=2)
    for matrix in (0, 1):
        desc = plan(eng, W, H, hs, vs, ncomp, siting, matrix, 1)
        planes = to_yuv(eng, desc, grey[None])
        assert np.array_equal(planes[0, :W * H].reshape(H, W), grey[..., 0]) and (planes[0, W * H:] == 128).all()
        assert np.array_equal(to_rgb(eng, desc, planes)[0], grey)


def test_plan_refusals():
    lib = host_lib().lib
    d = L.fs_yuv_desc()
    ref = ctypes.byref(d)
    good = (16, 16, 2, 2, 3, 0, 0, 0)
    assert lib.fs_yuv_plan(*(good + (ref,))) == 0
    for args, code in (((0, 16) + good[2:], -1), ((16, 0) + good[2:], -1), ((32768, 16) + good[2:], -1), ((16, 40000) + good[2:], -1),
                       ((16, 16, 1, 2, 3, 0, 0, 0), -2), ((16, 16, 4, 1, 3, 0, 0, 0), -2), ((16, 16, 2, 4, 3, 0, 0, 0), -2), ((16, 16, 0, 0, 3, 0, 0, 0), -2),
                       ((16, 16, 2, 2, 2, 0, 0, 0), -2), ((16, 16, 2, 2, 4, 0, 0, 0), -2), ((16, 16, 2, 2, 1, 0, 0, 0), -2), ((16, 16, 2, 1, 1, 0, 0, 0), -2),
                       ((16, 16, 2, 2, 3, 2, 0, 0), -2), ((16, 16, 2, 2, 3, -1, 0, 0), -2), ((16, 16, 2, 2, 3, 0, 2, 0), -2), ((16, 16, 2, 2, 3, 0, 0, 2), -2)):
        assert lib.fs_yuv_plan(*(args + (ref,))) == code, args
        assert lib.fs_last_error().startswith(b"fs_yuv_plan")
    assert lib.fs_yuv_plan(*(good + (None,))) == -1
    with pytest.raises(L.FaststyleError):
        host_lib().yuv_plan(16, 16, sampling=(4, 1))


@pytest.mark.parametrize("kind", backends.engine_params())
def test_device_call_refusals_leave_the_destination_untouched(kind):
    eng = backends.get_engine(kind)
    lib, mem = eng.lib, eng.mem
    W, H = 17, 31
    desc = plan(eng, W, H, 2, 2, 3, 1, 0, 0)
    n = int(desc.frame_bytes)
    guard = 16
    yuv = mem.upload_u8(np.concatenate([np.full(guard, 0x5A, np.uint8), yuv_frames(W, H, 2, 2, 3)[0], np.full(guard, 0x5A, np.uint8)]))
    rgb = mem.upload_u8(np.concatenate([np.full(guard, 0x5A, np.uint8), rgbx(rgb_images(W, H)[:1]).reshape(-1), np.full(guard, 0x5A, np.uint8)]))
    yuv0, rgb0 = np.array(mem.to_numpy(yuv), copy=True), np.array(mem.to_numpy(rgb), copy=True)
    p_yuv, p_rgb = mem.ptr_u8(yuv) + guard, mem.ptr_u8(rgb) + guard
    good = ctypes.byref(desc)

    def copy_of(**changes):
        c = L.fs_yuv_desc.from_buffer_copy(desc)
        for k, v in changes.items():
            setattr(c, k, v)
        return ctypes.byref(c)

    edited = [copy_of(width=W + 1), copy_of(height=0), copy_of(hs=4), copy_of(ncomp=2), copy_of(siting=2), copy_of(matrix=3), copy_of(full_range=-1),
              copy_of(chroma_w=desc.chroma_w + 1), copy_of(frame_bytes=n + 1), copy_of(frame_bytes=0)]
    # (ctx, desc, yuv, N, pixel_bytes, swap_rb, rgb)
    to_rgb_calls = [((eng.ctx, good, p_yuv, 1, 2, 0, p_rgb), -2), ((eng.ctx, good, p_yuv, 1, 5, 0, p_rgb), -2),
                    ((None, good, p_yuv, 1, 3, 0, p_rgb), -1), ((eng.ctx, None, p_yuv, 1, 3, 0, p_rgb), -1), ((eng.ctx, good, None, 1, 3, 0, p_rgb), -1),
                    ((eng.ctx, good, p_yuv, 1, 3, 0, None), -1), ((eng.ctx, good, p_yuv, 0, 3, 0, p_rgb), -1), ((eng.ctx, good, p_yuv, -1, 3, 0, p_rgb), -1),
                    ((eng.ctx, good, p_yuv, 65536, 3, 0, p_rgb), -1), ((eng.ctx, good, p_yuv, 1, 4, 0, p_rgb + 1), -5), ((eng.ctx, good, p_yuv, 1, 4, 0, p_rgb + 2), -5)] + \
        [((eng.ctx, e, p_yuv, 1, 3, 0, p_rgb), -1) for e in edited]
    # (ctx, desc, rgb, pixel_bytes, swap_rb, N, yuv)
    to_yuv_calls = [((eng.ctx, good, p_rgb, 2, 0, 1, p_yuv), -2), ((eng.ctx, good, p_rgb, 0, 0, 1, p_yuv), -2),
                    ((None, good, p_rgb, 3, 0, 1, p_yuv), -1), ((eng.ctx, None, p_rgb, 3, 0, 1, p_yuv), -1), ((eng.ctx, good, None, 3, 0, 1, p_yuv), -1),
                    ((eng.ctx, good, p_rgb, 3, 0, 1, None), -1), ((eng.ctx, good, p_rgb, 3, 0, 0, p_yuv), -1), ((eng.ctx, good, p_rgb, 3, 0, 65536, p_yuv), -1),
                    ((eng.ctx, good, p_rgb + 1, 4, 0, 1, p_yuv), -5)] + \
        [((eng.ctx, e, p_rgb, 3, 0, 1, p_yuv), -1) for e in edited]
    eng._sync_stream()
    for args, code in to_rgb_calls:
        assert lib.fs_yuv_to_rgb_u8(*args) == code, args
        assert lib.fs_last_error().startswith(b"fs_yuv_to_rgb_u8")
    for args, code in to_yuv_calls:
        assert lib.fs_rgb_to_yuv_u8(*args) == code, args
        assert lib.fs_last_error().startswith(b"fs_rgb_to_yuv_u8")
    with pytest.raises(L.FaststyleError):                                              # the engine's own shape check
        eng.yuv_to_rgb_u8(mem.upload_u8(np.zeros(n + 1, np.uint8)), desc, mem.upload_u8(np.zeros((H, W, 3), np.uint8)))
    assert np.array_equal(mem.to_numpy(yuv), yuv0) and np.array_equal(mem.to_numpy(rgb), rgb0)
    # and the same buffers work when asked properly, writing nothing outside their frame
    assert lib.fs_yuv_to_rgb_u8(eng.ctx, good, p_yuv, 1, 4, 0, p_rgb) == 0
    got = np.array(mem.to_numpy(rgb), copy=True)
    assert (got[:guard] == 0x5A).all() and (got[-guard:] == 0x5A).all()
    assert np.array_equal(got[guard:-guard].reshape(H, W, 4)[..., :3], want_rgb(W, H, 2, 2, 3, 1, 0, 0)[0])
    rgb = mem.upload_u8(rgb0)
    assert lib.fs_rgb_to_yuv_u8(eng.ctx, good, mem.ptr_u8(rgb) + guard, 4, 0, 1, p_yuv) == 0
    got = np.array(mem.to_numpy(yuv), copy=True)
    assert (got[:guard] == 0x5A).all() and (got[-guard:] == 0x5A).all()
    assert np.array_equal(got[guard:-guard], want_yuv(W, H, 2, 2, 3, 1, 0, 0)[0])
