"""Guided delivery on the device (csrc/fs_guided.hip) against the contract, the arithmetic that include/faststyle_io.h states.  The first part
of this file is an independent numpy restatement of that text (int64 throughout); every comparison of the device with the restatement --
the coefficients, their window means and the float result -- is equality.  The same bodies run on the CPU emulator and, under -m gpu, on
the MI355X.  tests/test_guided_stream.py builds its expected tensors with the restatement."""
import ctypes
import itertools

import numpy as np
import pytest

from faststyle_amd import _lib as L
from tests import backends
from tests.test_compose import GUARD, LUMA, SENTINEL, images, placed, same, to88

FILL = 201                                                      # what test_compose.placed puts around a u8 buffer
FMAX = 65280


# ================================================================ the restatement
def box(X, r):
    """int64 [H, W(, 3)] -> the sums over the clamped (2r + 1)^2 windows"""
    P = np.pad(X, [(r, r), (r, r)] + [(0, 0)] * (X.ndim - 2), mode="edge")
    H, W = X.shape[:2]
    return sum(P[j:j + H, i:i + W] for j in range(2 * r + 1) for i in range(2 * r + 1))


def tdiv(a, b):
    """int64 division that truncates towards zero"""
    return np.sign(a) * (np.abs(a) // b)


def axis(nd, ns):
    """the delivery axis of length nd over a grid axis of length ns -> (first tap, second tap, fraction in [0, 255])"""
    X = np.arange(nd, dtype=np.int64)
    num = (2 * X + 1) * ns - nd
    x0 = num // (2 * nd)
    return np.clip(x0, 0, ns - 1), np.clip(x0 + 1, 0, ns - 1), ((num - x0 * 2 * nd) * 256) // (2 * nd)


def up(M, Hd, Wd):
    """int64 [H, W, 3] -> [Hd, Wd, 3]: the four taps by their weights, which sum to 65536"""
    y0, y1, fy = axis(Hd, M.shape[0])
    x0, x1, fx = axis(Wd, M.shape[1])
    fy, fx = fy[:, None, None], fx[None, :, None]
    assert fy.min() >= 0 and fy.max() <= 255 and fx.min() >= 0 and fx.max() <= 255
    return (256 - fy) * (256 - fx) * M[y0][:, x0] + (256 - fy) * fx * M[y0][:, x1] + fy * (256 - fx) * M[y1][:, x0] + fy * fx * M[y1][:, x1]


def guided(I, P, G, r, E):
    """I [H,W], P [H,W,3], G [Hd,Wd]: int64 lumas / 8.8 values -> (F [Hd,Wd,3], a, b, abar, bbar)"""
    n = (2 * r + 1) ** 2
    SI, SP = box(I, r), box(P, r)
    V = n * box(I * I, r) - SI * SI
    assert V.min() >= 0
    C = n * box(I[..., None] * P, r) - SI[..., None] * SP
    a = tdiv(C * 4096, (V + n * n * E * E * 65536)[..., None])
    b = tdiv(SP * 4096 - a * SI[..., None], 256 * n)
    assert np.abs(a).max() < 1 << 18 and np.abs(b).max() < 1 << 27
    am, bm = tdiv(box(a, r), n), tdiv(box(b, r), n)
    U = up(am, *G.shape) * G[..., None] + (up(bm, *G.shape) << 8) + (1 << 27)
    assert np.abs(U).max() < 1 << 52
    return np.clip(U >> 28, 0, FMAX), a, b, am, bm


def luma_of(X, matrix, bgr):
    kr, kg, kb = LUMA[matrix]
    k0, k2 = (kb, kr) if bgr else (kr, kb)
    return (k0 * X[..., 0] + kg * X[..., 1] + k2 * X[..., 2] + 32768) >> 16


def hi88(hi):
    """the full-size source of any kind on the 8.8 scale, int64 [..., 3]"""
    return to88(hi) if hi.dtype == np.float32 else hi[..., :3].astype(np.int64) << 8


def guided_ref(lo_src, lo_out, hi, r=2, E=4, matrix=0, lo_bgr=False, hi_bgr=False):
    """lo_src [N,H,W,3] f32, lo_out [N,Ho,Wo,3] f32, hi [N,Hd,Wd,3|4] u8 or [N,Hd,Wd,3] f32 -> dict(coef, mean int32 [N,H,W,6], dst f32)"""
    H, W = lo_src.shape[1:3]
    coef, mean, dst = [], [], []
    for s, o, h in zip(lo_src, lo_out, hi):
        F, a, b, am, bm = guided(luma_of(to88(s), matrix, lo_bgr), to88(o[:H, :W]), luma_of(hi88(h), matrix, hi_bgr), r, E)
        coef.append(np.concatenate([a, b], axis=-1))
        mean.append(np.concatenate([am, bm], axis=-1))
        dst.append(F.astype(np.float32) * np.float32(0.00390625))
    return dict(coef=np.stack(coef).astype(np.int32), mean=np.stack(mean).astype(np.int32), dst=np.stack(dst))


# ================================================================ running the device call
@pytest.fixture(params=backends.engine_params())
def eng(request):
    return backends.get_engine(request.param)


def place_inputs(eng, lo_src, lo_out, hi, hoff=0):
    u8 = hi.dtype == np.uint8
    return placed(eng, lo_src, 0, 0)[1], placed(eng, lo_out, 0, 0)[1], placed(eng, hi, hoff, 0, u8=u8)[1]


def run(eng, lo_src, lo_out, hi, doff=0, hoff=0, **kw):
    """eng.guided_f32 on host arrays -> dict as guided_ref's; doff / hoff: elements past a 16-byte boundary of dst / hi.  The destination
    and the workspace lie between guards, which must come back untouched."""
    mem = eng.mem
    N, H, W = lo_src.shape[:3]
    s, o, h = place_inputs(eng, lo_src, lo_out, hi, hoff)
    shape = hi.shape[:3] + (3,)
    dbuf, d, d0 = placed(eng, np.full(shape, SENTINEL, np.float32), doff, GUARD)
    nbytes = eng.guided_workspace_bytes(H, W, N)
    assert nbytes % 32 == 0 and nbytes // 2 >= N * H * W * 24 > nbytes // 2 - 16
    wbuf, w, w0 = placed(eng, np.zeros((nbytes,), np.uint8), 0, GUARD, u8=True)
    eng.guided_f32(s, o, h, d, w, **kw)
    whole = np.array(mem.to_numpy(dbuf), copy=True).reshape(-1)
    size = int(np.prod(shape))
    assert np.all(whole[:d0] == SENTINEL) and np.all(whole[d0 + size:] == SENTINEL), "a write outside the destination"
    wwhole = np.array(mem.to_numpy(wbuf), copy=True).reshape(-1)
    assert np.all(wwhole[:w0] == FILL) and np.all(wwhole[w0 + nbytes:] == FILL), "a write outside the workspace"
    coef, mean = eng.guided_parts(w, H, W, N)
    return dict(coef=coef, mean=mean, dst=whole[d0:d0 + size].reshape(shape))


def equal(got, want):
    return np.array_equal(got["coef"], want["coef"]) and np.array_equal(got["mean"], want["mean"]) and same(got["dst"], want["dst"]) and \
        got["coef"].dtype == np.int32 and got["mean"].dtype == np.int32


# ================================================================ data
# (H, W, Ho, Wo, Hd, Wd, radius): the net's grid, the output tensor's size, the delivery.  The coef tile is 32 x 16 and the mean tile 16 x 16:
# 33 x 70 is three tiles by three and five by three.  The last two have a delivery width that is a multiple of 4: the 16-byte accesses.
GRIDS = [(1, 1, 1, 1, 1, 1, 1), (1, 1, 4, 4, 3, 5, 2), (5, 7, 5, 7, 5, 7, 2), (5, 7, 8, 8, 11, 9, 8), (9, 11, 12, 12, 20, 30, 1),
         (14, 30, 16, 32, 43, 91, 2), (33, 70, 36, 72, 70, 150, 8), (9, 11, 9, 11, 21, 32, 2), (33, 70, 33, 70, 67, 152, 1)]
KINDS = [0, 1, 2]
_cases = {}


def hi_of(kind, Hd, Wd, seed):
    """three full-size sources of one kind: noise, the odd floats / a second noise, a 0 | 255 checkerboard"""
    f = images(Hd, Wd, seed)
    if kind == 2:
        return f
    rs = np.random.RandomState(seed + 5)
    u = np.stack([np.clip(f[0], 0, 255).astype(np.uint8), rs.randint(0, 256, (Hd, Wd, 3)).astype(np.uint8), f[2].astype(np.uint8)])
    if kind == 1:
        u = np.concatenate([u, rs.randint(0, 256, (3, Hd, Wd, 1)).astype(np.uint8)], axis=-1)
    return np.ascontiguousarray(u)


def case(g, kind):
    """(lo_src, lo_out, hi) of three images: noise, the odd floats, checkerboards; the margin of lo_out is NaN"""
    key = (g, kind)
    if key not in _cases:
        H, W, Ho, Wo, Hd, Wd, _ = GRIDS[g]
        lo_src = images(H, W, 11 + g)
        lo_out = np.full((3, Ho, Wo, 3), np.nan, np.float32)
        lo_out[:, :H, :W] = images(H, W, 40 + g)[[1, 0, 2]]
        _cases[key] = tuple(np.ascontiguousarray(a) for a in (lo_src, lo_out, hi_of(kind, Hd, Wd, 70 + g)))
        for a in _cases[key]:
            a.setflags(write=False)
    return _cases[key]


# ================================================================ the device against the restatement
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("g", range(len(GRIDS)))
def test_matches_restatement(eng, g, kind):
    """every grid, every source kind; the batch size, the smoothness, the matrix and the channel orders go round with the case"""
    lo_src, lo_out, hi = case(g, kind)
    r = GRIDS[g][6]
    k = g * 3 + kind
    N = (1, 2, 3)[k % 3] if g not in (6, 8) else 3 - kind
    kw = dict(r=r, E=(1, 4, 64)[(k // 2) % 3], matrix=k & 1, lo_bgr=bool(k & 2), hi_bgr=bool((k >> 2) & 1))
    sel = slice(3 - N, 3)                                       # (the checkerboards, the largest a and b, are in every batch)
    want = guided_ref(lo_src[sel], lo_out[sel], hi[sel], **kw)
    got = run(eng, lo_src[sel], lo_out[sel], hi[sel], radius=kw["r"], smoothness=kw["E"], matrix=kw["matrix"], lo_bgr=kw["lo_bgr"],
              hi_bgr=kw["hi_bgr"])
    assert equal(got, want)


@pytest.mark.parametrize("kind", KINDS)
def test_parameters(eng, kind):
    """radius x smoothness x matrix x the four channel orders on the 9 x 11 -> 20 x 30 grid"""
    lo_src, lo_out, hi = case(4, kind)
    for r, E, matrix, lo_bgr, hi_bgr in itertools.product((1, 2, 8), (1, 4, 64), (0, 1), (False, True), (False, True)):
        if (r, E) not in ((1, 1), (2, 4), (8, 64), (1, 64)) and (matrix or lo_bgr or hi_bgr):
            continue                                            # (the full product of the flags at four (r, E) pairs, every pair once)
        want = guided_ref(lo_src, lo_out, hi, r=r, E=E, matrix=matrix, lo_bgr=lo_bgr, hi_bgr=hi_bgr)
        got = run(eng, lo_src, lo_out, hi, radius=r, smoothness=E, matrix="bt709" if matrix else "bt601", lo_bgr=lo_bgr, hi_bgr=hi_bgr)
        assert equal(got, want), (r, E, matrix, lo_bgr, hi_bgr)


def test_channel_orders_differ():
    """the restatement itself: on a source whose red and blue are far apart each flag changes the result, so a wrong flag cannot pass"""
    lo_src, lo_out, hi = case(4, 0)
    ref = [guided_ref(lo_src[:1], lo_out[:1], hi[:1], lo_bgr=a, hi_bgr=b)["dst"] for a in (False, True) for b in (False, True)]
    assert all(not np.array_equal(ref[i], ref[j]) for i in range(4) for j in range(i))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("g", [7, 8])
def test_alignment(eng, g, kind):
    """a delivery width that is a multiple of 4: dst and the source on and off a 16-byte boundary give the same values"""
    lo_src, lo_out, hi = case(g, kind)
    want = guided_ref(lo_src, lo_out, hi, r=2, E=4)
    step = 1 if kind == 2 else 4                                # (elements of hi: floats, bytes)
    for doff, hoff in ((0, 0), (1, 0), (0, step), (2, 2 * step), (0, 1 if kind != 2 else 3)):
        assert equal(run(eng, lo_src, lo_out, hi, doff=doff, hoff=hoff), want), (doff, hoff)


# ================================================================ the known answers
@pytest.mark.parametrize("kind", KINDS)
def test_constant_output(eng, kind):
    """a constant lo_out gives to88 of it everywhere: a = 0, b = 16 to88(v) exactly, for every source, radius and smoothness"""
    lo_src, _, hi = case(5, kind)
    H, W = lo_src.shape[1:3]
    for v, r, E in ((0.0, 1, 1), (255.0, 8, 64), (100.3, 2, 4), (17.99609375, 2, 1)):
        lo_out = np.full((3, H, W, 3), v, np.float32)
        got = run(eng, lo_src, lo_out, hi, radius=r, smoothness=E)
        q = int(to88(np.float32(v)))
        assert np.all(got["coef"][..., :3] == 0) and np.all(got["coef"][..., 3:] == 16 * q)
        assert np.all(got["mean"][..., :3] == 0) and np.all(got["mean"][..., 3:] == 16 * q)
        assert same(got["dst"], np.full(hi.shape[:3] + (3,), np.float32(q) * np.float32(0.00390625)))


@pytest.mark.parametrize("kind", KINDS)
def test_flat_source(eng, kind):
    """a flat lo_src gives a = 0: the result is the bilinear interpolation of the window means of P, whatever the full-size source"""
    _, lo_out, hi = case(4, kind)
    H, W, _, _, Hd, Wd, _ = GRIDS[4]
    lo_src = np.ascontiguousarray(np.broadcast_to(np.array([90.5, 12.0, 201.25], np.float32), (3, H, W, 3)))
    got = run(eng, lo_src, lo_out, hi, radius=2, smoothness=1)
    assert np.all(got["coef"][..., :3] == 0)
    n = 25
    for i in range(3):
        bm = tdiv(box(tdiv(box(to88(lo_out[i, :H, :W]), 2) * 4096, 256 * n), 2), n)
        F = np.clip(((up(bm, Hd, Wd) << 8) + (1 << 27)) >> 28, 0, FMAX)
        assert same(got["dst"][i], F.astype(np.float32) * np.float32(0.00390625))


@pytest.mark.parametrize("kind", KINDS)
def test_identity_grid(eng, kind):
    """Hd = H, Wd = W: one tap of weight 65536 per pixel, no interpolation"""
    lo_src, lo_out, hi = case(2, kind)
    y0, y1, fy = axis(5, 5)
    assert np.array_equal(y0, np.arange(5)) and not fy.any()
    got = run(eng, lo_src, lo_out, hi, radius=1, smoothness=4)
    G = luma_of(hi88(hi), 0, False)[..., None]
    m = got["mean"].astype(np.int64)
    F = np.clip((m[..., :3] * 65536 * G + ((m[..., 3:] * 65536) << 8) + (1 << 27)) >> 28, 0, FMAX)
    assert same(got["dst"], F.astype(np.float32) * np.float32(0.00390625))
    assert equal(got, guided_ref(lo_src, lo_out, hi, r=1, E=4))


# ================================================================ the contract itself
def psnr88(F, T):
    return 10.0 * np.log10(float(FMAX) ** 2 / np.mean((F.astype(np.float64) - T.astype(np.float64)) ** 2))


def edges_case(seed=0):
    """A 144 x 192 source with edges, a per-pixel non-linear style of its luma, the net's grid at 48 x 64 as the 3 x 3 box mean"""
    y, x = np.indices((144, 192)).astype(np.float64)
    R = np.where((x // 17 + y // 13) % 2 == 1, 200.0, 40.0)
    G = np.where(((x + y) // 23) % 2 == 1, 180.0, 60.0)
    B = 128.0 + 100.0 * np.sin(x / 9.0) * np.cos(y / 7.0)
    hi = np.clip(np.stack([R, G, B], axis=-1) + np.random.RandomState(seed).normal(0.0, 4.0, (144, 192, 3)), 0.0, 255.0)

    def style(img):
        Ln = (0.299 * img[..., 0] + 0.587 * img[..., 1] + 0.114 * img[..., 2]) / 255.0
        return np.stack([255.0 * np.sqrt(Ln), 255.0 * (1.0 - Ln), 255.0 * np.abs(np.sin(3.0 * Ln))], axis=-1)

    lo = hi.reshape(48, 3, 64, 3, 3).mean(axis=(1, 3))
    return tuple(np.ascontiguousarray(a, np.float32) for a in (lo, style(lo), hi, style(hi)))


def test_edges_return(eng):
    """The point of the stage, on the restatement, with the device held to it: at radius 1 and smoothness 4 the guided result is at least
    3 dB closer to the style of the full-size source than the plain bilinear interpolation of the same taps.  Measured with the restatement:
    31.3 against 24.6 dB."""
    lo_src, lo_out, hi, target = edges_case()
    T = to88(target)
    I, P, G = luma_of(to88(lo_src), 0, False), to88(lo_out), luma_of(to88(hi), 0, False)
    F = guided(I, P, G, 1, 4)[0]
    plain = np.clip(((up(16 * P, *G.shape) << 8) + (1 << 27)) >> 28, 0, FMAX)
    got, base = psnr88(F, T), psnr88(plain, T)
    print("guided %.2f dB, bilinear %.2f dB" % (got, base))
    assert got >= base + 3.0
    dev = run(eng, lo_src[None], lo_out[None], hi[None], radius=1, smoothness=4)
    assert same(dev["dst"][0], F.astype(np.float32) * np.float32(0.00390625))


# ================================================================ refusals
def raw_call(eng, a, **over):
    """fs_guided_f32 with the arguments of `a` (a dict), some replaced -> (rc, the error text)"""
    v = dict(a, **over)
    rc = eng.lib.fs_guided_f32(v["ctx"], v["lo_src"], v["H"], v["W"], v["lo_out"], v["Ho"], v["Wo"], v["hi_src"], v["hi_kind"], v["Hd"], v["Wd"],
                               v["N"], v["radius"], v["smoothness"], v["matrix"], v["lo_bgr"], v["hi_bgr"], v["work"], v["work_bytes"], v["dst"])
    return rc, (eng.lib.fs_last_error() or b"").decode()


def test_refusals(eng):
    """every refusal of the C call: the code, a message that starts with the function's name, and nothing written"""
    mem = eng.mem
    lo_src, lo_out, hi = case(4, 2)
    H, W, Ho, Wo, Hd, Wd, _ = GRIDS[4]
    s, o, h = place_inputs(eng, lo_src, lo_out, hi)
    dbuf, d, d0 = placed(eng, np.full((3, Hd, Wd, 3), SENTINEL, np.float32), 0, GUARD)
    nbytes = eng.guided_workspace_bytes(H, W, 3)
    wbuf, w, w0 = placed(eng, np.full((nbytes + 16,), FILL, np.uint8), 0, GUARD, u8=True)
    ok = dict(ctx=eng.ctx, lo_src=mem.ptr(s), H=H, W=W, lo_out=mem.ptr(o), Ho=Ho, Wo=Wo, hi_src=mem.ptr(h), hi_kind=2, Hd=Hd, Wd=Wd, N=3, radius=2,
              smoothness=4, matrix=0, lo_bgr=0, hi_bgr=0, work=mem.ptr_u8(w), work_bytes=nbytes, dst=mem.ptr(d))
    bad = [(-1, dict(ctx=None)), (-1, dict(lo_src=None)), (-1, dict(lo_out=None)), (-1, dict(hi_src=None)), (-1, dict(work=None)),
           (-1, dict(dst=None)), (-1, dict(N=0)), (-1, dict(N=65536)), (-1, dict(H=0)), (-1, dict(W=0)), (-1, dict(Ho=H - 1)), (-1, dict(Ho=H + 4)),
           (-1, dict(Wo=W - 1)), (-1, dict(Wo=W + 4)), (-1, dict(Hd=32768)), (-1, dict(Wd=32768)), (-1, dict(Hd=H - 1)), (-1, dict(Wd=W - 1)),
           (-1, dict(work_bytes=nbytes - 1)), (-1, dict(dst=mem.ptr(o))), (-1, dict(dst=mem.ptr(s))), (-1, dict(dst=mem.ptr(h))),
           (-2, dict(radius=0)), (-2, dict(radius=9)), (-2, dict(smoothness=0)), (-2, dict(smoothness=65)), (-2, dict(hi_kind=-1)),
           (-2, dict(hi_kind=3)), (-2, dict(matrix=2)), (-2, dict(matrix=-1)), (-2, dict(lo_bgr=2)), (-2, dict(hi_bgr=-1)),
           (-5, dict(lo_src=mem.ptr(s) + 2)), (-5, dict(lo_out=mem.ptr(o) + 1)), (-5, dict(hi_src=mem.ptr(h) + 2)), (-5, dict(dst=mem.ptr(d) + 2)),
           (-5, dict(work=mem.ptr_u8(w) + 8, work_bytes=nbytes + 8))]
    for rc, over in bad:
        got, text = raw_call(eng, ok, **over)
        assert got == rc and text.startswith("fs_guided_f32"), (over, got, text)
    eng._sync_stream()
    assert np.all(np.array(mem.to_numpy(dbuf)).reshape(-1) == SENTINEL) and np.all(np.array(mem.to_numpy(wbuf)).reshape(-1) == FILL)
    for t, want in ((s, lo_src), (o, lo_out), (h, hi)):             # (the inputs that were offered as dst are as they were)
        assert same(np.array(mem.to_numpy(t)), want)
    h8 = placed(eng, hi_of(0, Hd, Wd, 3), 1, 0, u8=True)[1]
    assert raw_call(eng, ok, hi_src=mem.ptr_u8(h8), hi_kind=0)[0] == 0      # (a u8 source off every boundary is no refusal, and the call runs)
    eng._sync_stream()
    assert not np.any(np.array(mem.to_numpy(d)) == SENTINEL)


def test_workspace_refusals(eng):
    n = ctypes.c_size_t(7)
    for args in ((0, 5, 1), (5, 0, 1), (32768, 5, 1), (5, 32768, 1), (5, 5, 0), (5, 5, 65536)):
        assert eng.lib.fs_guided_workspace(args[0], args[1], args[2], ctypes.byref(n)) == -1
        assert (eng.lib.fs_last_error() or b"").decode().startswith("fs_guided_workspace") and n.value == 7
    assert eng.lib.fs_guided_workspace(5, 5, 1, None) == -1
    assert eng.lib.fs_guided_workspace(5, 7, 3, ctypes.byref(n)) == 0 and n.value == 2 * ((3 * 5 * 7 * 24 + 15) // 16 * 16)


def test_engine_refusals(eng):
    """Engine.guided_f32 checks the shapes against each other before the call"""
    lo_src, lo_out, hi = case(4, 2)
    H, W, Ho, Wo, Hd, Wd, _ = GRIDS[4]
    s, o, h = place_inputs(eng, lo_src, lo_out, hi)
    d = placed(eng, np.zeros((3, Hd, Wd, 3), np.float32), 0, 0)[1]
    w = eng.guided_workspace(H, W, 3)
    view = eng.mem.view
    for bad in (dict(lo_src=view(s, 0, (2, H, W, 3))), dict(dst=view(d, 0, (3, Hd, Wd - 1, 3))), dict(lo_out=view(o, 0, (3, Ho, Wo * 3))),
                dict(hi_src=view(h, 0, (3, Hd, Wd * 3, 1))), dict(work=view(d, 0, (64,))), dict(radius=9), dict(smoothness=0),
                dict(work=view(w, 0, (w.shape[0] - 16,)))):
        a = dict(lo_src=s, lo_out=o, hi_src=h, dst=d, work=w)
        a.update(bad)
        with pytest.raises(L.FaststyleError):
            eng.guided_f32(a.pop("lo_src"), a.pop("lo_out"), a.pop("hi_src"), a.pop("dst"), a.pop("work"), **a)
