"""cv2.resize on the device (csrc/fs_cvresize.hip) against its contract, the host restatement faststyle_amd/cvresize.py: every comparison is
exact -- the arithmetic is integer or separately rounded float32.  The same bodies run on the CPU emulator and, under -m gpu, on the MI355X."""
import ctypes

import numpy as np
import pytest

from faststyle_amd import _lib as L, cvresize, engine as fsengine, utils
from tests import backends

CUBIC, AREA = L.FS_CV_INTER_CUBIC, L.FS_CV_INTER_AREA
P_CUBIC, P_FAST, P_AREA = L.FS_CVRESIZE_PATH_CUBIC, L.FS_CVRESIZE_PATH_AREA_FAST, L.FS_CVRESIZE_PATH_AREA

# (id, source H, W, fx, fy, interpolation, path, result H, W)
CASES = [
    ("cubic_aniso", 37, 45, 56 / 45, 48 / 37, CUBIC, P_CUBIC, 48, 56),
    ("cubic_one_axis_shrinks", 60, 50, 56 / 50, 48 / 60, CUBIC, P_CUBIC, 48, 56),
    ("cubic_tie_size", 45, 61, 1.5, 1.5, CUBIC, P_CUBIC, 68, 92),
    ("cubic_no_tie", 45, 61, 1.37, 1.37, CUBIC, P_CUBIC, 62, 84),
    ("area_2x2", 96, 112, 0.5, 0.5, AREA, P_FAST, 48, 56),
    ("area_2x2_edge", 99, 115, 0.5, 0.5, AREA, P_FAST, 50, 58),
    ("area_4", 192, 224, 0.25, 0.25, AREA, P_FAST, 48, 56),
    ("area_3_edge", 100, 101, 1 / 3, 1 / 3, AREA, P_FAST, 33, 34),
    ("area_frac_aniso", 61, 83, 56 / 83, 48 / 61, AREA, P_AREA, 48, 56),
    ("area_frac_06", 45, 61, 0.6, 0.6, AREA, P_AREA, 27, 37),
    ("area_frac_50_99", 99, 99, 50 / 99, 50 / 99, AREA, P_AREA, 50, 50),
]
CASE_PARAMS = [pytest.param(*c[1:], id=c[0]) for c in CASES]

_host = {}


def host_lib():
    """The library's host calls without an engine: the emulator build holds the same host code as the product."""
    if "h" not in _host:
        from tests import emu_lib
        _host["h"] = fsengine.CvResizeHost(lib=L.bind(ctypes.CDLL(emu_lib.build_emu())))
    return _host["h"]


def image(H, W, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(H, W, 3)).astype(np.uint8)


_want = {}


def want(H, W, fx, fy, interp, seed=0):
    """cvresize.py's answer, computed once per case."""
    key = (H, W, fx, fy, interp, seed)
    if key not in _want:
        fn = cvresize.resize_cubic_u8 if interp == CUBIC else cvresize.resize_area_u8
        _want[key] = fn(image(H, W, seed), fx, fy)
        _want[key].setflags(write=False)
    return _want[key]


def run(eng, img, fx, fy, interp, swap_rb=False):
    """img: host uint8 [H,W,3|4] or [N,H,W,3|4] -> host result of the device call."""
    img = np.ascontiguousarray(img)
    plan = eng.cvresize_plan(img.shape[-3], img.shape[-2], fx, fy, interp)
    lead = img.shape[:-3]
    out = eng.mem.upload_u8(np.full(lead + plan.dst_shape + (3,), 0xA5, np.uint8))
    eng.cvresize_u8(eng.mem.upload_u8(img), plan, out, swap_rb=swap_rb)
    return np.array(eng.mem.to_numpy(out), copy=True), plan


@pytest.mark.parametrize("H,W,fx,fy,interp,path,Hd,Wd", CASE_PARAMS)
def test_plan_reports_size_and_path(H, W, fx, fy, interp, path, Hd, Wd):
    plan = host_lib().cvresize_plan(H, W, fx, fy, interp)
    assert plan.dst_shape == (Hd, Wd) and plan.path == path
    assert plan.dst_shape == want(H, W, fx, fy, interp).shape[:2]
    assert plan.tables.nbytes == plan.info.table_bytes and (path == P_FAST) == (plan.tables.nbytes == 0)


@pytest.mark.parametrize("H,W,fx,fy,interp,path,Hd,Wd", CASE_PARAMS)
def test_host_tables_equal_cvresize_entry_for_entry(H, W, fx, fy, interp, path, Hd, Wd):
    plan = host_lib().cvresize_plan(H, W, fx, fy, interp)
    for axis, n_src, n_dst, f in (("x", W, Wd, fx), ("y", H, Hd, fy)):
        got = plan.axis_table(axis)
        if path == P_FAST:
            assert got is None
        elif path == P_CUBIC:
            idx, w = cvresize._cubic_axis(n_src, n_dst, 1.0 / f)
            assert np.array_equal(got[0], idx) and np.array_equal(got[1], w)
        else:
            ref = cvresize._area_tab(n_src, n_dst, 1.0 / f)
            assert len(got) == len(ref)
            assert all(g[0] == r[0] and g[1] == r[1] and np.float32(g[2]).tobytes() == np.float32(r[2]).tobytes() for g, r in zip(got, ref))


def test_default_interpolation_is_the_reference_dispatch_on_two_axes():
    h = host_lib()
    assert h.cvresize_plan(40, 40, 0.5, 1.0).info.interpolation == AREA       # one axis shrinks, the other stays
    assert h.cvresize_plan(40, 40, 0.6, 0.7).info.interpolation == AREA
    assert h.cvresize_plan(40, 40, 1.0, 1.0).info.interpolation == CUBIC      # nothing shrinks
    assert h.cvresize_plan(40, 40, 1.2, 0.8).info.interpolation == CUBIC      # one axis enlarges
    assert h.cvresize_plan(40, 40, 1.5, 1.5).info.interpolation == CUBIC


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("H,W,fx,fy,interp,path,Hd,Wd", CASE_PARAMS)
def test_kernel_matches_cvresize(kind, H, W, fx, fy, interp, path, Hd, Wd):
    eng = backends.get_engine(kind)
    got, plan = run(eng, image(H, W), fx, fy, interp)
    assert plan.path == path and got.shape == (Hd, Wd, 3)
    assert np.array_equal(got, want(H, W, fx, fy, interp))


def step_image(H=40, W=44):
    a = np.zeros((H, W, 3), np.uint8)
    a[:, W // 2:] = 255
    return a


def checker_image(H=40, W=44):
    y, x = np.mgrid[:H, :W]
    return np.repeat((((y // 2 + x // 2) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("scale", [1.5, 1.7])
@pytest.mark.parametrize("pattern", ["step", "checker"])
def test_cubic_saturates_at_both_ends_like_cvresize(kind, scale, pattern):
    eng = backends.get_engine(kind)
    img = step_image() if pattern == "step" else checker_image()
    ref = cvresize.resize_cubic_u8(img, scale, scale)
    assert ref.min() == 0 and ref.max() == 255          # the overshoot of the cubic is clipped on both sides
    got, _ = run(eng, img, scale, scale, CUBIC)
    assert np.array_equal(got, ref)


VARIANTS = [pytest.param(*c[1:6], id=c[0]) for c in CASES if c[0] in ("cubic_aniso", "area_2x2_edge", "area_3_edge", "area_frac_aniso")]


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("H,W,fx,fy,interp", VARIANTS)
def test_rgbx_swap_and_batch(kind, H, W, fx, fy, interp):
    eng = backends.get_engine(kind)
    img = image(H, W)
    ref = want(H, W, fx, fy, interp)
    rgbx = np.concatenate([img, np.full((H, W, 1), 0xEE, np.uint8)], axis=2)            # a poisoned fourth byte
    rgbx[::2, ::3, 3] = 0x11
    assert np.array_equal(run(eng, rgbx, fx, fy, interp)[0], ref)
    assert np.array_equal(run(eng, img, fx, fy, interp, swap_rb=True)[0], ref[..., ::-1])
    assert np.array_equal(run(eng, rgbx, fx, fy, interp, swap_rb=True)[0], ref[..., ::-1])
    two = np.stack([img, image(H, W, seed=1)])
    got = run(eng, two, fx, fy, interp)[0]
    assert np.array_equal(got[0], ref) and np.array_equal(got[1], want(H, W, fx, fy, interp, seed=1))
    two_x = np.concatenate([two, np.full((2, H, W, 1), 0x77, np.uint8)], axis=3)
    assert np.array_equal(run(eng, two_x, fx, fy, interp)[0], got)


def test_plan_refusals():
    lib = host_lib().lib
    info = L.fs_cvresize_info()
    ref = ctypes.byref(info)
    for args, code in (((40, 40, 1.5, 0.5, AREA), -2), ((40, 40, 0.5, 1.01, AREA), -2), ((40, 40, 0.5, 0.5, 1), -2),
                       ((0, 40, 0.5, 0.5, AREA), -1), ((40, 40000, 0.5, 0.5, AREA), -1), ((40, 40, 0.0, 0.5, AREA), -1),
                       ((40, 40, float("nan"), 0.5, CUBIC), -1), ((1, 40, 0.5, 0.3, AREA), -1), ((40, 40, 1000.0, 1.0, CUBIC), -1)):
        assert lib.fs_cvresize_plan(*(args + (ref,))) == code, args
        assert lib.fs_last_error().startswith(b"fs_cvresize_plan")
    assert lib.fs_cvresize_plan(40, 40, 0.5, 0.5, AREA, None) == -1
    plan = host_lib().cvresize_plan(37, 45, 1.5, 1.5, CUBIC)
    buf = np.zeros(plan.tables.nbytes + 8, np.uint8)
    assert lib.fs_cvresize_tables(ctypes.byref(plan.info), None, buf.nbytes) == -1
    assert lib.fs_cvresize_tables(ctypes.byref(plan.info), buf.ctypes.data, plan.tables.nbytes - 1) == -1
    assert lib.fs_cvresize_tables(ctypes.byref(plan.info), buf.ctypes.data + 1, plan.tables.nbytes) == -5
    assert lib.fs_last_error().startswith(b"fs_cvresize_tables")


@pytest.mark.parametrize("kind", backends.engine_params())
def test_device_call_refusals_leave_the_destination_untouched(kind):
    eng = backends.get_engine(kind)
    lib, mem = eng.lib, eng.mem
    H, W = 37, 45
    plan = eng.cvresize_plan(H, W, 56 / 45, 48 / 37, CUBIC)
    src = mem.upload_u8(np.concatenate([image(H, W), np.zeros((H, W, 1), np.uint8)], axis=2))
    poison = np.full(plan.dst_shape + (3,), 0x5A, np.uint8)
    dst = mem.upload_u8(poison)
    tab = mem.upload_u8(plan.tables)
    good = ctypes.byref(plan.info)
    p_src, p_dst, p_tab = mem.ptr_u8(src), mem.ptr_u8(dst), mem.ptr_u8(tab)

    def copy_of(**changes):
        c = L.fs_cvresize_info.from_buffer_copy(plan.info)
        for k, v in changes.items():
            setattr(c, k, v)
        return ctypes.byref(c)

    calls = [
        ((eng.ctx, good, p_tab, p_src, 2, 1, 0, p_dst), -2),                       # pixel size 2
        ((None, good, p_tab, p_src, 3, 1, 0, p_dst), -1),                          # null pointers
        ((eng.ctx, None, p_tab, p_src, 3, 1, 0, p_dst), -1),
        ((eng.ctx, good, None, p_src, 3, 1, 0, p_dst), -1),
        ((eng.ctx, good, p_tab, None, 3, 1, 0, p_dst), -1),
        ((eng.ctx, good, p_tab, p_src, 3, 1, 0, None), -1),
        ((eng.ctx, good, p_tab, p_src, 3, 0, 0, p_dst), -1),                       # no image
        ((eng.ctx, copy_of(dst_w=0), p_tab, p_src, 3, 1, 0, p_dst), -1),           # a zero-sized destination
        ((eng.ctx, copy_of(dst_h=0, dst_w=0), p_tab, p_src, 3, 1, 0, p_dst), -1),
        ((eng.ctx, copy_of(interpolation=AREA), p_tab, p_src, 3, 1, 0, p_dst), -1),   # area asked to enlarge, by hand
        ((eng.ctx, copy_of(src_w=W + 1), p_tab, p_src, 3, 1, 0, p_dst), -1),       # a plan that was edited
        ((eng.ctx, good, p_tab + 4, p_src, 3, 1, 0, p_dst), -5),                   # misaligned tables
        ((eng.ctx, good, p_tab, p_src + 1, 4, 1, 0, p_dst), -5),                   # misaligned 4-byte pixels
    ]
    eng._sync_stream()
    for args, code in calls:
        assert lib.fs_cvresize_u8(*args) == code, args
        assert lib.fs_last_error().startswith(b"fs_cvresize_u8")
    with pytest.raises(L.FaststyleError):
        eng.cvresize_plan(H, W, 1.5, 0.5, AREA)
    assert np.array_equal(mem.to_numpy(dst), poison)
    eng.cvresize_u8(src, plan, dst)                                                # and the same buffers work when asked properly
    assert np.array_equal(mem.to_numpy(dst), want(H, W, 56 / 45, 48 / 37, CUBIC))


@pytest.mark.parametrize("kind", backends.engine_params())
def test_stale_table_gives_wrong_pixels_only(kind):
    """Indices far outside the source in the device tables: the kernels clamp them, the call completes and writes the whole destination."""
    eng = backends.get_engine(kind)
    for (H, W, fx, fy, interp) in ((37, 45, 56 / 45, 48 / 37, CUBIC), (61, 83, 56 / 83, 48 / 61, AREA)):
        plan = eng.cvresize_plan(H, W, fx, fy, interp)
        bad = plan.tables.view("<i4").copy()
        bad[::2] = 0x7FFFFFF0
        bad[1::4] = -0x7FFFFFF0
        plan.tables_dev = eng.mem.upload_u8(bad.view(np.uint8))
        out = eng.mem.upload_u8(np.zeros(plan.dst_shape + (3,), np.uint8))
        eng.cvresize_u8(eng.mem.upload_u8(image(H, W)), plan, out)
        assert np.asarray(eng.mem.to_numpy(out)).shape == plan.dst_shape + (3,)


@pytest.mark.parametrize("kind", backends.engine_params())
@pytest.mark.parametrize("scale", [0.5, 0.6, 1.5])
def test_imresize_with_engine_equals_host(kind, scale):
    eng = backends.get_engine(kind)
    img = image(45, 61, seed=3)
    for a in (img, img[:, :, 0]):
        ref = utils.imresize(a, scale)
        got = utils.imresize(a, scale, engine=eng)
        assert got.shape == ref.shape and got.dtype == np.uint8 and np.array_equal(got, ref)
    assert utils.imresize(img, 1.0, engine=eng) is img
