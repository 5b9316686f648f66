"""Style strength, colour preservation and the region mask on the device (csrc/fs_compose.hip) against the contract, the arithmetic that
include/faststyle_io.h states.  The first part of this file is an independent numpy restatement of that text (int64 and >>); every
comparison of the device with the restatement is exact.  The same bodies run on the CPU emulator and, under -m gpu, on the MI355X.
tests/test_compose_stream.py and tests/test_compose_cli.py build their expected tensors with the restatement."""
import itertools

import numpy as np
import pytest

from faststyle_amd import _lib as L
from tests import backends

FMAX = 65280                                                    # 255 in unsigned 8.8
LUMA = {0: (19595, 38470, 7471), 1: (13933, 46871, 4732)}       # (kr, kg, kb) by 2^16: BT.601, BT.709


# ================================================================ the restatement
def to88(x):
    """float32 -> int64 on the 8.8 scale: clamped to [0, 255] with NaN -> 0, times 256, truncated"""
    x = np.asarray(x, np.float32)
    q = np.where(np.isnan(x), np.float32(0), np.clip(x, np.float32(0), np.float32(255))).astype(np.float32)
    return (q * np.float32(256)).astype(np.int64)


def luma(X, matrix, bgr):
    kr, kg, kb = LUMA[matrix]
    r, b = (2, 0) if bgr else (0, 2)
    return (kr * X[..., r] + kg * X[..., 1] + kb * X[..., b] + 32768) >> 16


def compose_F(src, net, q8=256, keep=False, matrix=0, bgr=False, mask=None, src_swapped=False):
    """src float32 [N,H,W,3], net float32 [N,Ho,Wo,3], mask uint8 [H,W] or None -> (F int64 [N,Ho,Wo,3], the sums before the clamp)"""
    assert LUMA[matrix][0] + LUMA[matrix][1] + LUMA[matrix][2] == 65536 and 0 <= q8 <= 256
    H, W = src.shape[1:3]
    Ho, Wo = net.shape[1:3]
    assert H <= Ho <= H + 3 and W <= Wo <= W + 3
    yi, xi = np.minimum(np.arange(Ho), H - 1), np.minimum(np.arange(Wo), W - 1)
    A = to88(src)[:, yi][:, :, xi]
    if src_swapped:
        A = A[..., ::-1]
    B = to88(net)
    if keep:
        D = np.repeat((luma(B, matrix, bgr) - luma(A, matrix, bgr))[..., None], 3, axis=-1)
    else:
        D = B - A
    m = np.full((Ho, Wo), 255, np.int64) if mask is None else np.asarray(mask)[yi][:, xi].astype(np.int64)
    w = q8 * (m + (m >> 7))
    assert w.min() >= 0 and w.max() <= 65536
    U = A + ((D * w[None, :, :, None] + 32768) >> 16)
    return np.clip(U, 0, FMAX), U


def f32_of_F(F):
    return F.astype(np.float32) * np.float32(0.00390625)


def compose_ref(src, net, **kw):
    return f32_of_F(compose_F(src, net, **kw)[0])


def same(a, b):
    """bit for bit (float32)"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ================================================================ running the device call
GUARD = 16                                                      # floats in front of and behind every destination (a multiple of 4)
SENTINEL = np.float32(-7.0)


@pytest.fixture(params=backends.engine_params())
def eng(request):
    return backends.get_engine(request.param)


def placed(eng, a, off, pad, u8=False):
    """A device copy of ``a`` that starts ``off`` elements past a 16-byte boundary (plus ``pad`` elements on either side): (buffer, view)"""
    mem = eng.mem
    host = np.full(a.size + 2 * pad + 32, 201 if u8 else SENTINEL, a.dtype)
    buf = mem.upload_u8(host) if u8 else mem.from_numpy(host)
    base = mem.ptr_u8(buf) if u8 else mem.ptr(buf)
    start = (-base // a.itemsize) % (16 // a.itemsize) + pad + off
    view = mem.view(buf, start, a.shape)
    if hasattr(view, "copy_"):
        view.copy_(mem.torch.from_numpy(np.array(a, copy=True)))                                # (a copy: the shared cases are read-only)
    else:
        view[...] = a
    assert ((mem.ptr_u8(view) if u8 else mem.ptr(view)) - off * a.itemsize) % 16 == 0
    return buf, view, start


def run(eng, src, net, mask=None, off=(0, 0, 0, 0), alias=False, **kw):
    """eng.compose_f32 on host arrays -> the host result; off: elements past a 16-byte boundary of src, net, dst, mask.  The destination
    lies between two guards of GUARD floats, which must come back untouched."""
    mem = eng.mem
    _, s, _ = placed(eng, src, off[0], 0)
    nbuf, n, n0 = placed(eng, net, off[1], GUARD)
    m = placed(eng, mask, off[3], 0, u8=True)[1] if mask is not None else None
    if alias:
        dbuf, d, d0 = nbuf, n, n0
    else:
        dbuf, d, d0 = placed(eng, np.full(net.shape, SENTINEL, np.float32), off[2], GUARD)
    eng.compose_f32(s, n, d, mask=m, **kw)
    whole = np.array(mem.to_numpy(dbuf), copy=True).reshape(-1)
    assert np.all(whole[:d0] == SENTINEL) and np.all(whole[d0 + net.size:] == SENTINEL), "a write outside the destination"
    return whole[d0:d0 + net.size].reshape(net.shape)


# ================================================================ data
SHAPES = [(1, 1, 4, 4), (3, 5, 4, 8), (17, 31, 20, 32), (8, 6, 8, 8), (64, 48, 64, 48)]     # H, W, Ho, Wo
N = 3
_cases = {}


def images(H, W, seed):
    """Three float32 images: noise over [0, 255]; values off the scale, NaN, infinities and v + j / 256 -+ 1e-4 (the truncation to 8.8);
    a 0 | 255 checkerboard whose phase differs per channel"""
    rs = np.random.RandomState(seed)
    noise = rs.uniform(0.0, 255.0, (H, W, 3)).astype(np.float32)
    idx = np.indices((H, W, 3))
    lin = idx[0] * W * 3 + idx[1] * 3 + idx[2] + seed
    steps = (lin * 37 % 255).astype(np.float32) + (lin * 101 % 256).astype(np.float32) / np.float32(256) + \
        np.where(lin & 1, np.float32(1e-4), np.float32(-1e-4)).astype(np.float32)
    special = np.array([-1.0, -1e30, 255.5, 300.0, 1e30, np.nan, np.inf, -np.inf, 0.0, 255.0, 254.99998, -0.0], np.float32)
    pick = rs.randint(0, 3 * special.size, (H, W, 3))
    odd = np.where(pick < special.size, special[pick % special.size], steps).astype(np.float32)
    checker = ((((idx[0] + idx[1]) >> (seed & 1)) + idx[2] * (seed & 1)) & 1).astype(np.float32) * np.float32(255)
    return np.stack([noise, odd, checker])


def case(shape):
    """(src [3,H,W,3], net [3,Ho,Wo,3], masks {name: uint8 [H,W] or None}) of one shape, built once and read-only"""
    if shape not in _cases:
        H, W, Ho, Wo = shape
        src, net = images(H, W, 7 + H), images(Ho, Wo, 10 + Wo)
        rs = np.random.RandomState(H * 1000 + W)
        masks = {"none": None, "noise": rs.randint(0, 256, (H, W)).astype(np.uint8),
                 "steps": np.array([0, 127, 128, 255], np.uint8)[rs.randint(0, 4, (H, W))]}
        for a in (src, net, masks["noise"], masks["steps"]):
            a.setflags(write=False)
        _cases[shape] = (src, net, masks)
    return _cases[shape]


STRENGTHS = (0, 1, 77, 128, 255, 256)


def modes():
    """Every mode of the issue's list: plain, and keep_color under both matrices and both channel orders; each at every strength and mask"""
    for q8, mk in itertools.product(STRENGTHS, ("none", "noise", "steps")):
        yield dict(q8=q8, keep=False), mk
        for matrix, bgr in itertools.product((0, 1), (False, True)):
            yield dict(q8=q8, keep=True, matrix=matrix, bgr=bgr), mk


def device_kw(kw):
    return dict(strength_q8=kw["q8"], keep_color=kw["keep"], matrix=kw.get("matrix", 0), bgr=kw.get("bgr", False),
                src_swapped=kw.get("src_swapped", False))


# ================================================================ the restatement itself (CPU)
def test_restatement_known_answers():
    one = lambda v: np.full((1, 1, 1, 3), v, np.float32)
    assert compose_F(one(0.0), one(255.0), q8=128)[0].tolist() == [[[[32640] * 3]]]           # 127.5
    assert f32_of_F(np.array([32640]))[0] == np.float32(127.5)
    assert to88(np.array([1.0 + 3 / 256.0 - 1e-4, 1.0 + 3 / 256.0 + 1e-4, np.nan, -5, 300, np.inf, -np.inf], np.float32)).tolist() == \
        [258, 259, 0, 0, FMAX, FMAX, 0]
    m = np.array([[0, 127, 128, 255]], np.uint8)
    src, net = np.zeros((1, 1, 4, 3), np.float32), np.full((1, 1, 4, 3), 255.0, np.float32)
    assert compose_F(src, net, mask=m)[0][0, 0, :, 0].tolist() == [0, 255 * 127, 255 * 129, FMAX]      # m' = 0, 127, 129, 256 over 256
    # the checkerboards make the clamp act at both ends under keep_color
    src, net, _ = case((64, 48, 64, 48))
    U = compose_F(src[2:], net[2:], keep=True)[1]
    assert U.min() < 0 and U.max() > FMAX


# ================================================================ the device against the restatement
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_every_mode_matches_the_restatement(eng, shape):
    src, net, masks = case(shape)
    assert src.shape == (N,) + shape[:2] + (3,) and net.shape == (N,) + shape[2:] + (3,)
    for kw, mk in modes():
        got = run(eng, src, net, mask=masks[mk], **device_kw(kw))
        assert same(got, compose_ref(src, net, mask=masks[mk], **kw)), (kw, mk)
    # the source read with R and B exchanged (the frame tools' channel handling), once per mode kind
    for kw in (dict(q8=77, keep=False, src_swapped=True), dict(q8=200, keep=True, matrix=1, bgr=False, src_swapped=True),
               dict(q8=256, keep=True, matrix=0, bgr=True, src_swapped=True)):
        got = run(eng, src, net, mask=masks["noise"], **device_kw(kw))
        assert same(got, compose_ref(src, net, mask=masks["noise"], **kw)), kw
    # one image, no batch axis
    got = run(eng, src[0], net[0], mask=masks["steps"], strength_q8=77, keep_color=True, matrix=1)
    assert same(got, compose_ref(src[:1], net[:1], mask=masks["steps"], q8=77, keep=True, matrix=1)[0])


@pytest.mark.parametrize("off", [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (2, 3, 1, 3)], ids=lambda o: "off_%d%d%d%d" % o)
def test_a_misaligned_tensor_takes_the_narrow_path_with_the_same_values(eng, off):
    """64 x 48 -> 64 x 48 is the wide path (16-byte accesses, mask dwords); one float off 16-byte alignment in any tensor takes single floats, one
    byte off in the mask takes single bytes: the values are those of the aligned run."""
    src, net, masks = case((64, 48, 64, 48))
    for kw, mk in (dict(q8=77, keep=False), "noise"), (dict(q8=255, keep=True, matrix=1, bgr=True), "steps"), (dict(q8=128, keep=True), "none"):
        wide = run(eng, src, net, mask=masks[mk], **device_kw(kw))
        got = run(eng, src, net, mask=masks[mk], off=off, **device_kw(kw))
        assert same(got, wide) and same(got, compose_ref(src, net, mask=masks[mk], **kw)), (kw, mk)


@pytest.mark.parametrize("shape", [(17, 31, 20, 32), (64, 48, 64, 48)], ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_the_destination_may_be_the_net_output(eng, shape):
    src, net, masks = case(shape)
    for kw in (dict(q8=77, keep=False), dict(q8=200, keep=True, matrix=1)):
        got = run(eng, src, net, mask=masks["noise"], alias=True, **device_kw(kw))
        assert same(got, compose_ref(src, net, mask=masks["noise"], **kw)), kw


def test_consequences_of_the_contract(eng):
    shape = (17, 31, 20, 32)
    src, net, masks = case(shape)
    H, W, Ho, Wo = shape
    yi, xi = np.minimum(np.arange(Ho), H - 1), np.minimum(np.arange(Wo), W - 1)
    A = f32_of_F(to88(src))[:, yi][:, :, xi]
    # full strength, no mask, plain: the net's output on the 8.8 scale, whose high byte is what fs_f32_to_u8 writes
    got = run(eng, src, net, strength_q8=256)
    assert same(got, f32_of_F(to88(net)))
    with np.errstate(invalid="ignore"):
        u8 = np.where(np.isnan(net), 0, np.clip(net, 0, 255)).astype(np.uint8)
    assert np.array_equal((to88(got) >> 8).astype(np.uint8), u8)
    # strength 0: the source, replicated into the extra rows and columns -- in every mode
    for keep in (False, True):
        assert same(run(eng, src, net, mask=masks["noise"], strength_q8=0, keep_color=keep), A)
    # a zero mask byte: the source at that pixel; a 255 byte: the unmasked result
    half = np.zeros((H, W), np.uint8)
    half[:, W // 2:] = 255
    for keep in (False, True):
        got = run(eng, src, net, mask=half, strength_q8=200, keep_color=keep, matrix=1)
        free = run(eng, src, net, strength_q8=200, keep_color=keep, matrix=1)
        assert same(got[:, :, :W // 2], A[:, :, :W // 2]) and same(got[:, :, W // 2:], free[:, :, W // 2:])
    # half strength between 0 and 255: 127.5
    got = run(eng, np.zeros((1, 5, 7, 3), np.float32), np.full((1, 8, 8, 3), 255.0, np.float32), strength_q8=128)
    assert np.all(got == np.float32(127.5))
    # net == src: the source on the 8.8 scale, in every mode
    sq, _, msq = case((64, 48, 64, 48))
    for kw, mk in modes():
        if kw["q8"] in (77, 256):
            assert same(run(eng, sq, sq, mask=msq[mk], **device_kw(kw)), f32_of_F(to88(sq))), (kw, mk)
    # keep_color over a grey source at full strength: the luma of the net's output in the three channels
    grey = np.repeat(src[..., :1], 3, axis=-1)
    for matrix, bgr in itertools.product((0, 1), (False, True)):
        got = run(eng, grey, net, strength_q8=256, keep_color=True, matrix=matrix, bgr=bgr)
        Lb = f32_of_F(luma(to88(net), matrix, bgr))
        assert same(got, np.repeat(Lb[..., None], 3, axis=-1)), (matrix, bgr)


def test_keep_color_keeps_the_channel_differences_of_the_source(eng):
    """Where no clamp acts, F_c - F_c' = A_c - A_c' for every channel pair: one delta went to the three channels."""
    H, W, Ho, Wo = 17, 31, 20, 32
    rs = np.random.RandomState(3)
    src = rs.uniform(64.0, 192.0, (N, H, W, 3)).astype(np.float32)
    net = rs.uniform(0.0, 255.0, (N, Ho, Wo, 3)).astype(np.float32)
    mask = rs.randint(0, 256, (H, W)).astype(np.uint8)
    yi, xi = np.minimum(np.arange(Ho), H - 1), np.minimum(np.arange(Wo), W - 1)
    A = to88(src)[:, yi][:, :, xi]
    for q8, mk, matrix, bgr in ((256, None, 0, False), (256, None, 1, True), (180, mask, 1, False)):
        F, U = compose_F(src, net, q8=q8, keep=True, matrix=matrix, bgr=bgr, mask=mk)
        free = (U == F).all(axis=-1)
        assert free.mean() >= 0.5                                                               # (of the restatement alone)
        got = to88(run(eng, src, net, mask=mk, strength_q8=q8, keep_color=True, matrix=matrix, bgr=bgr))
        for c, d in ((0, 1), (1, 2), (0, 2)):
            assert np.array_equal((got[..., c] - got[..., d])[free], (A[..., c] - A[..., d])[free])
        assert not np.array_equal(got, A)


def test_refused_calls_return_their_code_and_launch_nothing(eng):
    mem, lib, ctx = eng.mem, eng.lib, eng.ctx
    H, W, Ho, Wo = 17, 31, 20, 32
    src, net, masks = case((H, W, Ho, Wo))
    _, s, _ = placed(eng, src, 0, 0)
    _, n, _ = placed(eng, net, 0, 0)
    dbuf, d, d0 = placed(eng, np.full(net.shape, SENTINEL, np.float32), 0, GUARD)
    m = placed(eng, masks["noise"], 0, 0, u8=True)[1]
    ps, pn, pd, pm = mem.ptr(s), mem.ptr(n), mem.ptr(d), mem.ptr_u8(m)
    eng._sync_stream()

    def call(src=ps, H=H, W=W, net=pn, Ho=Ho, Wo=Wo, N=N, q8=200, keep=1, matrix=0, bgr=0, mask=pm, dst=pd):
        return lib.fs_compose_f32(ctx, src, H, W, net, Ho, Wo, N, q8, keep, matrix, bgr, mask, dst)

    refused = [(-1, dict(src=None)), (-1, dict(net=None)), (-1, dict(dst=None)), (-1, dict(N=0)), (-1, dict(N=65536)), (-1, dict(N=-1)),
               (-1, dict(H=0)), (-1, dict(W=0)), (-1, dict(H=-3)), (-1, dict(Ho=H - 1)), (-1, dict(Ho=H + 4)), (-1, dict(Wo=W - 1)),
               (-1, dict(Wo=W + 4)), (-1, dict(H=2 ** 31 - 1)), (-2, dict(q8=-1)), (-2, dict(q8=257)), (-2, dict(matrix=2)), (-2, dict(matrix=-1)),
               (-2, dict(bgr=4)), (-2, dict(bgr=-1)), (-5, dict(src=ps + 2)), (-5, dict(net=pn + 1)), (-5, dict(dst=pd + 3))]
    for code, kw in refused:
        assert call(**kw) == code, kw
        assert b"fs_compose_f32" in lib.fs_last_error()
    assert np.all(np.asarray(mem.to_numpy(dbuf)) == SENTINEL)                                 # nothing was launched
    assert lib.fs_compose_f32(None, ps, H, W, pn, Ho, Wo, N, 200, 1, 0, 0, pm, pd) == -1
    # the call they were variations of is taken, with or without the mask
    assert call() == 0 and call(mask=None, keep=0) == 0
    got = np.asarray(mem.to_numpy(dbuf)).reshape(-1)[d0:d0 + net.size].reshape(net.shape)
    assert same(got, compose_ref(src, net, q8=200))
    with pytest.raises(L.FaststyleError):
        eng.compose_f32(s, n, d, mask=mem.upload_u8(np.zeros((H, W + 1), np.uint8)))
    with pytest.raises(L.FaststyleError):
        eng.compose_f32(s, s, d)
