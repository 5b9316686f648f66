"""Resampling between fp32 tensors (csrc/fs_resample.hip) against its contract, the arithmetic stated in include/faststyle_io.h.  The module
opens with an independent numpy restatement of that text (python floats for the tables, float64 accumulation in tap order, float32 between the
passes); the restatement is held to Pillow's Image.resize on mode-F images, the library's tables and the kernel to the restatement.  Every
comparison is bit for bit on float32 (NaN positions compared as positions).  The kernel tests run on the CPU emulator and, under -m gpu, on
the MI355X."""
import ctypes
import math

import numpy as np
import pytest
from PIL import Image

from faststyle_amd import _lib as L, engine as fsengine
from tests import backends

FILTERS = ("box", "bilinear", "bicubic", "lanczos")
PIL_FILTER = {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}
# (source H, W, destination H, W): a single pixel, each axis alone, mixed up / down, a shrink by 7, taps that span the whole source, several tiles
# with ragged edges in both directions (135 x 240 against 16 x 64 tiles)
SIZES = [(1, 1, 3, 5), (7, 5, 20, 13), (16, 24, 48, 72), (45, 80, 135, 240), (40, 52, 17, 33), (64, 48, 9, 7), (30, 30, 30, 61),
         (33, 17, 100, 17), (12, 9, 1, 1), (90, 160, 34, 61), (23, 31, 24, 30)]
SIZE_IDS = ["%dx%d-%dx%d" % s for s in SIZES]
# one pair per tile height the plan can choose (tall and narrow: the vertical factor alone decides): (Hs, Ws, Hd, Wd, filter, tile_h)
TILE_CASES = [(45, 80, 135, 240, "bicubic", 16), (96, 8, 16, 9, "bicubic", 8), (120, 5, 12, 5, "bicubic", 4), (200, 6, 20, 6, "lanczos", 2),
              (208, 4, 16, 4, "lanczos", 1)]


# ---------------------------------------------------------------- the restatement
def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTER_DEF = {"box": (0.5, _box), "bilinear": (1.0, _bilinear), "bicubic": (2.0, _bicubic), "lanczos": (3.0, _lanczos)}


def axis_tables(n_in, n_out, name):
    """(xmin, cnt, weights per output index, ksize) of one axis, in python floats (IEEE double, every operation rounded on its own)."""
    s, f = FILTER_DEF[name]
    scale = n_in / n_out
    fscale = max(scale, 1.0)
    support = s * fscale
    inv = 1.0 / fscale
    xmins, cnts, ws = [], [], []
    for d in range(n_out):
        center = (d + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(n_in, int(center + support + 0.5))
        w = [f((k + xmin - center + 0.5) * inv) for k in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmins.append(xmin)
        cnts.append(xmax - xmin)
        ws.append(w)
    return xmins, cnts, ws, 2 * int(math.ceil(support)) + 1


def _pass(a, axis, n_out, name):
    """One pass along ``axis`` of a float32 array: float64 products and sums in tap order from 0.0, a float32 result."""
    a = np.moveaxis(a, axis, 0)
    xmins, cnts, ws, _ = axis_tables(a.shape[0], n_out, name)
    out = np.empty((n_out,) + a.shape[1:], np.float32)
    with np.errstate(all="ignore"):
        for d in range(n_out):
            ss = np.zeros(a.shape[1:], np.float64)
            for k in range(cnts[d]):
                ss = ss + a[xmins[d] + k].astype(np.float64) * ws[d][k]
            out[d] = ss.astype(np.float32)
    return np.moveaxis(out, 0, axis)


def restate(a, Hd, Wd, name):
    """float32 [..., H, W, C] -> [..., Hd, Wd, C]: the horizontal pass first, a pass of an unchanged axis skipped."""
    a = np.asarray(a, np.float32)
    if a.shape[-2] != Wd:
        a = _pass(a, a.ndim - 2, Wd, name)
    if a.shape[-3] != Hd:
        a = _pass(a, a.ndim - 3, Hd, name)
    return np.array(a, copy=True)


def same_bits(got, want):
    """Bit for bit, except that NaNs are compared as positions."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]))


# ---------------------------------------------------------------- inputs
def noise(H, W, seed=0, N=None):
    shape = (H, W, 3) if N is None else (N, H, W, 3)
    return (np.random.RandomState(seed).rand(*shape) * 255.0).astype(np.float32)


def steps(H, W):
    a = np.zeros((H, W, 3), np.float32)
    a[:, W // 2:, 0] = 255.0
    a[H // 2:, :, 1] = 255.0
    y, x = np.mgrid[:H, :W]
    a[:, :, 2] = ((y // 2 + x // 2) & 1) * 255.0           # a checkerboard
    return a


def far(H, W, seed=5):
    r = np.random.RandomState(seed)
    return (r.randn(H, W, 3) * 10.0 ** r.randint(-30, 30, size=(H, W, 3))).astype(np.float32)


def special(H, W, seed=6):
    a = noise(H, W, seed)
    r = np.random.RandomState(seed)
    flat = a.reshape(-1)
    idx = r.permutation(flat.size)[:max(3, flat.size // 17)]
    flat[idx[0::3]] = np.nan
    flat[idx[1::3]] = np.inf
    flat[idx[2::3]] = -np.inf
    return a


INPUTS = {"noise": noise, "steps": steps, "far": far, "special": special}

_want = {}


def want(kind, Hs, Ws, Hd, Wd, name):
    """The restatement's answer, computed once per case and shared."""
    key = (kind, Hs, Ws, Hd, Wd, name)
    if key not in _want:
        _want[key] = restate(INPUTS[kind](Hs, Ws), Hd, Wd, name)
        _want[key].setflags(write=False)
    return _want[key]


_host = {}


def host_lib():
    """The library's host calls without an engine: the emulator build holds the same host code as the product."""
    if "h" not in _host:
        from tests import emu_lib
        _host["h"] = fsengine.ResampleHost(lib=L.bind(ctypes.CDLL(emu_lib.build_emu())))
    return _host["h"]


def run(eng, a, Hd, Wd, name, plan=None):
    a = np.ascontiguousarray(a, np.float32)
    plan = plan or eng.resample_plan(a.shape[-3], a.shape[-2], Hd, Wd, name)
    dst = eng.mem.from_numpy(np.full(a.shape[:-3] + (Hd, Wd, 3), -7.0, np.float32))
    eng.resample_f32(eng.mem.from_numpy(a), plan, dst)
    return np.array(eng.mem.to_numpy(dst), copy=True)


# ---------------------------------------------------------------- the restatement against Pillow (CPU, no engine)
@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("kind", ["noise", "steps", "far"])
@pytest.mark.parametrize("Hs,Ws,Hd,Wd", SIZES, ids=SIZE_IDS)
def test_restatement_equals_pillow(Hs, Ws, Hd, Wd, kind, name):
    a = INPUTS[kind](Hs, Ws)
    ref = want(kind, Hs, Ws, Hd, Wd, name)
    for c in range(3):
        im = Image.fromarray(np.ascontiguousarray(a[:, :, c]))
        assert im.mode == "F"
        got = np.asarray(im.resize((Wd, Hd), PIL_FILTER[name]), np.float32)
        assert same_bits(ref[:, :, c], got), (c, np.abs(ref[:, :, c] - got).max())


def test_bicubic_overshoot_is_kept():
    ref = want("steps", 16, 24, 48, 72, "bicubic")
    assert ref.min() < -15.0 and ref.max() > 270.0


# ---------------------------------------------------------------- plan and tables
@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("Hs,Ws,Hd,Wd", SIZES, ids=SIZE_IDS)
def test_plan_and_tables_equal_the_restatement(Hs, Ws, Hd, Wd, name):
    plan = host_lib().resample_plan(Hs, Ws, Hd, Wd, name)
    i = plan.info
    assert (i.src_h, i.src_w, i.dst_h, i.dst_w, i.filter, i.tile_w) == (Hs, Ws, Hd, Wd, L.FS_RESAMPLE_FILTERS[name], 64)
    assert i.x_offset % 16 == 0 and i.y_offset % 16 == 0 and i.table_bytes % 16 == 0 and plan.tables.nbytes == i.table_bytes
    assert i.tile_h in (16, 8, 4, 2, 1) and 1 <= i.tile_rows <= i.lds_rows <= L.FS_RESAMPLE_LDS_ROWS and i.lds_rows in (16, 40, 85)
    spans = []
    for axis, n_in, n_out, ksize in (("x", Ws, Wd, i.x_ksize), ("y", Hs, Hd, i.y_ksize)):
        got = plan.axis_table(axis)
        if n_in == n_out:
            assert got is None and ksize == 0
            continue
        xmins, cnts, ws, ks = axis_tables(n_in, n_out, name)
        s = FILTER_DEF[name][0] * max(n_in / n_out, 1.0)
        assert ksize == ks == 2 * int(math.ceil(s)) + 1
        assert got[0].tolist() == xmins and got[1].tolist() == cnts and got[2].shape == (n_out, ksize)
        for d in range(n_out):
            row = np.array(ws[d] + [0.0] * (ksize - cnts[d]), np.float64)
            assert np.array_equal(got[2][d].view(np.uint64), row.view(np.uint64)), (axis, d)
        if axis == "y":
            th = i.tile_h
            spans = [max(xmins[d] + cnts[d] for d in range(d0, min(d0 + th, n_out))) - xmins[d0] for d0 in range(0, n_out, th)]
    assert i.tile_rows == (max(spans) if spans else i.tile_h)


@pytest.mark.parametrize("Hs,Ws,Hd,Wd,name,tile_h", TILE_CASES)
def test_plan_picks_the_largest_tile_height_that_fits(Hs, Ws, Hd, Wd, name, tile_h):
    h = host_lib()
    i = h.resample_plan(Hs, Ws, Hd, Wd, name).info
    assert i.tile_h == tile_h and i.tile_rows <= 85
    xmins, cnts, _, _ = axis_tables(Hs, Hd, name)
    if tile_h < 16:                                        # twice the height would not fit
        th = 2 * tile_h
        assert max(max(xmins[d] + cnts[d] for d in range(d0, min(d0 + th, Hd))) - xmins[d0] for d0 in range(0, Hd, th)) > 85


def test_plan_takes_a_shrink_by_eight_with_every_filter_and_any_enlargement():
    h = host_lib()
    for name in FILTERS:
        assert h.resample_plan(2160, 3840, 270, 480, name).info.tile_h >= 1
        assert h.resample_plan(32767, 64, 4096, 8, name).info.tile_h >= 1
        assert h.resample_plan(1, 1, 32767, 32767, name).info.tile_h == 16
        assert h.resample_plan(720, 1280, 2160, 3840, name).info.lds_rows == 16
    same = h.resample_plan(40, 50, 40, 50, "lanczos")
    assert same.info.table_bytes == 0 and same.tables.size == 0 and (same.info.x_ksize, same.info.y_ksize) == (0, 0)


def test_plan_and_table_refusals():
    lib = host_lib().lib
    info = L.fs_resample_info()
    ref = ctypes.byref(info)
    for args, code in (((0, 4, 4, 4, 2), -1), ((4, 0, 4, 4, 2), -1), ((4, 4, 0, 4, 2), -1), ((4, 4, 4, 0, 2), -1), ((32768, 4, 4, 4, 2), -1),
                       ((4, 32768, 4, 4, 2), -1), ((4, 4, 32768, 4, 2), -1), ((4, 4, 4, 32768, 2), -1), ((4, 4, 4, 4, -1), -2), ((4, 4, 4, 4, 4), -2),
                       ((160, 4, 10, 4, 3), -2),              # lanczos by 16: one output row takes 97 source rows
                       ((1000, 4, 10, 4, 0), -2)):            # box by 100: 101 rows
        assert lib.fs_resample_plan(*(args + (ref,))) == code, args
        assert lib.fs_last_error().startswith(b"fs_resample_plan")
    assert lib.fs_resample_plan(4, 4, 8, 8, 2, None) == -1
    assert lib.fs_resample_plan(4, 160, 4, 10, 3, ref) == 0          # the horizontal factor is free
    h = host_lib()
    for bad in (dict(filter="nearest"), dict(Hd=0), dict(Wd=2.5), dict(Hs="tall"), dict(Hs=160, Ws=4, Hd=10, Wd=4, filter="lanczos")):
        kw = dict(dict(Hs=8, Ws=8, Hd=16, Wd=16, filter="bicubic"), **bad)
        with pytest.raises(L.FaststyleError):
            h.resample_plan(**kw)
    plan = h.resample_plan(7, 5, 20, 13, "bicubic")
    buf = np.zeros(plan.tables.nbytes // 8 + 2, np.float64).view(np.uint8)
    good = ctypes.byref(plan.info)
    assert lib.fs_resample_tables(None, buf.ctypes.data, buf.nbytes) == -1
    assert lib.fs_resample_tables(good, None, buf.nbytes) == -1
    assert lib.fs_resample_tables(good, buf.ctypes.data, plan.tables.nbytes - 1) == -1
    assert lib.fs_resample_tables(good, buf.ctypes.data + 4, plan.tables.nbytes) == -5
    edited = L.fs_resample_info.from_buffer_copy(plan.info)
    edited.tile_h = 8
    assert lib.fs_resample_tables(ctypes.byref(edited), buf.ctypes.data, buf.nbytes) == -1
    assert lib.fs_last_error().startswith(b"fs_resample_tables")
    assert lib.fs_resample_tables(good, buf.ctypes.data, buf.nbytes) == 0
    assert np.array_equal(buf[:plan.tables.nbytes], plan.tables)


# ---------------------------------------------------------------- the kernel
@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("Hs,Ws,Hd,Wd", SIZES, ids=SIZE_IDS)
def test_kernel_equals_the_restatement(kind, Hs, Ws, Hd, Wd, name):
    eng = backends.get_engine(kind)
    assert same_bits(run(eng, noise(Hs, Ws), Hd, Wd, name), want("noise", Hs, Ws, Hd, Wd, name))


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("Hs,Ws,Hd,Wd,name,tile_h", TILE_CASES)
def test_kernel_at_every_tile_height(kind, Hs, Ws, Hd, Wd, name, tile_h):
    eng = backends.get_engine(kind)
    plan = eng.resample_plan(Hs, Ws, Hd, Wd, name)
    assert plan.tile_h == tile_h
    assert same_bits(run(eng, noise(Hs, Ws), Hd, Wd, name, plan), want("noise", Hs, Ws, Hd, Wd, name))


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("inp", ["steps", "far", "special"])
@pytest.mark.parametrize("Hs,Ws,Hd,Wd", [(16, 24, 48, 72), (40, 52, 17, 33), (30, 30, 30, 61), (33, 17, 100, 17)])
def test_kernel_inputs_steps_far_values_nan_and_infinities(kind, Hs, Ws, Hd, Wd, inp, name):
    eng = backends.get_engine(kind)
    ref = want(inp, Hs, Ws, Hd, Wd, name)
    if inp == "steps" and name == "bicubic" and (Hd, Wd) == (48, 72):
        assert ref.min() < -15.0 and ref.max() > 270.0      # the overshoot is kept: nothing clamps
    if inp == "special":
        assert np.isnan(ref).any() and not np.isnan(ref).all()
    assert same_bits(run(eng, INPUTS[inp](Hs, Ws), Hd, Wd, name), ref)


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("N", [1, 2, 3])
def test_kernel_batches(kind, N):
    eng = backends.get_engine(kind)
    a = noise(23, 31, seed=9, N=N)
    got = run(eng, a, 24, 30, "lanczos")
    assert got.shape == (N, 24, 30, 3)
    for n in range(N):
        assert same_bits(got[n], restate(a[n], 24, 30, "lanczos"))


@pytest.mark.parametrize("kind", backends.engine_params())
def test_equal_sizes_copy(kind):
    eng = backends.get_engine(kind)
    a = special(19, 70)
    assert same_bits(run(eng, a, 19, 70, "bicubic"), a)


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("Hs,Ws,Hd,Wd,name", [(16, 24, 48, 72, "bicubic"), (40, 52, 17, 33, "lanczos"), (30, 30, 30, 61, "bilinear"),
                                              (33, 17, 100, 17, "box")])
def test_crop_form_never_reads_the_margin(kind, Hs, Ws, Hd, Wd, name):
    eng = backends.get_engine(kind)
    plan = eng.resample_plan(Hs, Ws, Hd, Wd, name)
    a = noise(Hs, Ws, N=2)
    ref = np.stack([restate(a[n], Hd, Wd, name) for n in range(2)])
    for dr, dp in ((1, 3), (2, 2), (3, 1)):
        big = np.full((2, Hs + dr, Ws + dp, 3), np.nan, np.float32)
        big[:, :Hs, :Ws] = a
        dst = eng.mem.from_numpy(np.zeros((2, Hd, Wd, 3), np.float32))
        eng.resample_f32(eng.mem.from_numpy(big), plan, dst)
        got = np.asarray(eng.mem.to_numpy(dst))
        assert not np.isnan(got).any() and same_bits(got, ref)


GUARD = 300                                                  # floats of sentinel on either side
SENTINEL = np.float32(-12345.5)


def guarded(eng, shape, offset=0):
    """A sentinel-filled device buffer and a view of ``shape`` inside it, GUARD + offset floats in (offset 1..3: off 16-byte alignment)."""
    n = int(np.prod(shape))
    whole = eng.mem.from_numpy(np.full(n + 2 * GUARD + 4, SENTINEL, np.float32))
    return whole, eng.mem.view(whole, GUARD + offset, shape)


def guards_intact(eng, whole, shape, offset=0):
    n = int(np.prod(shape))
    a = np.asarray(eng.mem.to_numpy(whole))
    return bool((a[:GUARD + offset] == SENTINEL).all() and (a[GUARD + offset + n:] == SENTINEL).all())


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_destination_guards_and_unaligned_tensors(kind, offset):
    eng = backends.get_engine(kind)
    for Hs, Ws, Hd, Wd, name in ((7, 5, 20, 13, "bicubic"), (64, 48, 9, 7, "lanczos"), (23, 31, 24, 30, "bilinear")):
        a = noise(Hs, Ws)
        swhole, sview = guarded(eng, (Hs, Ws, 3), offset)
        swhole_host = np.asarray(eng.mem.to_numpy(swhole)).copy()
        swhole_host[GUARD + offset:GUARD + offset + a.size] = a.reshape(-1)
        swhole = eng.mem.from_numpy(swhole_host)
        sview = eng.mem.view(swhole, GUARD + offset, (Hs, Ws, 3))
        whole, view = guarded(eng, (Hd, Wd, 3), offset)
        eng.resample_f32(sview, eng.resample_plan(Hs, Ws, Hd, Wd, name), view)
        assert guards_intact(eng, whole, (Hd, Wd, 3), offset)
        got = np.asarray(eng.mem.to_numpy(whole))[GUARD + offset:GUARD + offset + Hd * Wd * 3].reshape(Hd, Wd, 3)
        assert same_bits(got, want("noise", Hs, Ws, Hd, Wd, name))


@pytest.mark.parametrize("kind", backends.engine_params())
def test_stale_tables_give_wrong_pixels_only(kind):
    """xmin and cnt far outside the source in the device tables: the kernel clamps them, the call returns and writes only the destination."""
    eng = backends.get_engine(kind)
    for Hs, Ws, Hd, Wd, name in ((16, 24, 48, 72, "bicubic"), (40, 52, 17, 33, "lanczos"), (96, 8, 16, 9, "bicubic")):
        for xmin_bad, cnt_bad in ((0x7FFFFFF0, 0x7FFFFFF0), (-0x7FFFFFF0, 0x7FFFFFF0), (0x7FFFFFF0, -5), (-3, 1000)):
            plan = eng.resample_plan(Hs, Ws, Hd, Wd, name)
            bad = plan.tables.copy()
            i = plan.info
            for off, n_dst, ksize in ((i.x_offset, Wd, i.x_ksize), (i.y_offset, Hd, i.y_ksize)):
                rows = bad[off:off + n_dst * (8 + 8 * ksize)].view(np.dtype([("xmin", "<i4"), ("cnt", "<i4"), ("w", "<f8", (ksize,))]))
                rows["xmin"][::2] = xmin_bad
                rows["cnt"][1::3] = cnt_bad
                rows["xmin"][-1] = xmin_bad
                rows["cnt"][0] = cnt_bad
            plan.tables_dev = eng.mem.upload_u8(bad)
            src_whole, src = guarded(eng, (Hs, Ws, 3))
            whole, view = guarded(eng, (Hd, Wd, 3))
            eng.resample_f32(src, plan, view)
            assert guards_intact(eng, whole, (Hd, Wd, 3))
            assert (np.asarray(eng.mem.to_numpy(src_whole)) == SENTINEL).all()


@pytest.mark.parametrize("kind", backends.engine_params())
def test_device_call_refusals_leave_the_destination_untouched(kind):
    eng = backends.get_engine(kind)
    lib, mem = eng.lib, eng.mem
    Hs, Ws, Hd, Wd = 7, 5, 20, 13
    plan = eng.resample_plan(Hs, Ws, Hd, Wd, "bicubic")
    src = mem.from_numpy(noise(Hs, Ws))
    whole, dst = guarded(eng, (Hd, Wd, 3))
    tab = mem.upload_u8(plan.tables)
    good = ctypes.byref(plan.info)
    p_src, p_dst, p_tab = mem.ptr(src), mem.ptr(dst), mem.ptr_u8(tab)

    def copy_of(**changes):
        c = L.fs_resample_info.from_buffer_copy(plan.info)
        for k, v in changes.items():
            setattr(c, k, v)
        return ctypes.byref(c)

    unfilled = ctypes.byref(L.fs_resample_info())
    calls = [
        ((None, good, p_tab, p_src, Hs, Ws, 1, p_dst), -1),                         # null pointers
        ((eng.ctx, None, p_tab, p_src, Hs, Ws, 1, p_dst), -1),
        ((eng.ctx, good, None, p_src, Hs, Ws, 1, p_dst), -1),
        ((eng.ctx, good, p_tab, None, Hs, Ws, 1, p_dst), -1),
        ((eng.ctx, good, p_tab, p_src, Hs, Ws, 1, None), -1),
        ((eng.ctx, good, p_tab, p_src, Hs, Ws, 0, p_dst), -1),                      # N outside [1, 65535]
        ((eng.ctx, good, p_tab, p_src, Hs, Ws, 65536, p_dst), -1),
        ((eng.ctx, good, p_tab, p_src, Hs - 1, Ws, 1, p_dst), -1),                  # rows or pitch below the plan's
        ((eng.ctx, good, p_tab, p_src, Hs, Ws - 1, 1, p_dst), -1),
        ((eng.ctx, unfilled, p_tab, p_src, Hs, Ws, 1, p_dst), -1),                  # an unfilled plan
        ((eng.ctx, copy_of(dst_w=Wd + 1), p_tab, p_src, Hs, Ws, 1, p_dst), -1),     # a plan that was edited
        ((eng.ctx, copy_of(tile_h=8), p_tab, p_src, Hs, Ws, 1, p_dst), -1),
        ((eng.ctx, copy_of(lds_rows=85), p_tab, p_src, Hs, Ws, 1, p_dst), -1),
        ((eng.ctx, good, p_tab, p_dst, Hs, Ws, 1, p_dst), -1),                      # dst is src
        ((eng.ctx, good, p_tab, p_src + 2, Hs, Ws, 1, p_dst), -5),                  # float pointers off 4 bytes
        ((eng.ctx, good, p_tab, p_src, Hs, Ws, 1, p_dst + 1), -5),
        ((eng.ctx, good, p_tab + 8, p_src, Hs, Ws, 1, p_dst), -5),                  # tables off 16 bytes
    ]
    eng._sync_stream()
    for args, code in calls:
        assert lib.fs_resample_f32(*args) == code, args
        assert lib.fs_last_error().startswith(b"fs_resample_f32")
    for bad_src, bad_dst in ((mem.from_numpy(noise(Hs - 1, Ws)), dst), (mem.from_numpy(noise(Hs, Ws)[:, :, :2]), dst),
                             (src, mem.from_numpy(np.zeros((Hd, Wd + 1, 3), np.float32))),
                             (mem.from_numpy(noise(Hs, Ws, N=2)), dst)):
        with pytest.raises(L.FaststyleError):
            eng.resample_f32(bad_src, plan, bad_dst)
    assert (np.asarray(mem.to_numpy(whole)) == SENTINEL).all()
    eng.resample_f32(src, plan, dst)                                                # and the same buffers work when asked properly
    assert guards_intact(eng, whole, (Hd, Wd, 3))
    assert same_bits(np.asarray(mem.to_numpy(dst)).reshape(Hd, Wd, 3), want("noise", Hs, Ws, Hd, Wd, "bicubic"))


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("name", FILTERS)
def test_device_equals_pillow(kind, name):
    eng = backends.get_engine(kind)
    Hs, Ws, Hd, Wd = (40, 52, 17, 33) if name in ("box", "lanczos") else (16, 24, 48, 72)
    a = steps(Hs, Ws) + noise(Hs, Ws, seed=4) * np.float32(0.25)
    got = run(eng, a, Hd, Wd, name)
    for c in range(3):
        ref = np.asarray(Image.fromarray(np.ascontiguousarray(a[:, :, c])).resize((Wd, Hd), PIL_FILTER[name]), np.float32)
        assert same_bits(got[:, :, c], ref)
