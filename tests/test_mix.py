"""Two nets' outputs merged on the device (csrc/fs_mix.hip) against the contract, the arithmetic that include/faststyle_io.h states.  The first
part of this file is an independent numpy restatement of that text (int64 and >>); every comparison of the device with the restatement is
exact.  The same bodies run on the CPU emulator and, under -m gpu, on the MI355X.  tests/test_mix_stream.py builds its expected tensors with
the restatement."""
import numpy as np
import pytest

from faststyle_amd import _lib as L
from tests import backends
from tests.test_compose import FMAX, GUARD, SENTINEL, f32_of_F, images, placed, same, to88


# ================================================================ the restatement
def mix_F(a, b, t=256, mask=None, in_hw=None):
    """a, b float32 [N,Ho,Wo,3]; t: one weight or N of them, clamped to [0, 256] as the kernel clamps what it reads; mask uint8 [H,W] at the
    net's input size in_hw, or None -> F int64 [N,Ho,Wo,3]"""
    N, Ho, Wo = a.shape[:3]
    H, W = in_hw if in_hw is not None else (mask.shape if mask is not None else (Ho, Wo))
    assert a.shape == b.shape and H <= Ho <= H + 3 and W <= Wo <= W + 3
    t = np.clip(np.broadcast_to(np.asarray(t, np.int64), (N,)), 0, 256)
    yi, xi = np.minimum(np.arange(Ho), H - 1), np.minimum(np.arange(Wo), W - 1)
    m = np.full((Ho, Wo), 255, np.int64) if mask is None else np.asarray(mask)[yi][:, xi].astype(np.int64)
    w = t[:, None, None] * (m + (m >> 7))[None]
    assert w.min() >= 0 and w.max() <= 65536
    A, B = to88(a), to88(b)
    F = A + (((B - A) * w[..., None] + 32768) >> 16)
    assert F.min() >= 0 and F.max() <= FMAX                                                     # a convex combination: no clamp
    return F


def mix_ref(a, b, **kw):
    return f32_of_F(mix_F(a, b, **kw))


# ================================================================ running the device call
@pytest.fixture(params=backends.engine_params())
def eng(request):
    return backends.get_engine(request.param)


def run(eng, a, b, in_hw, mask=None, weights=None, off=(0, 0, 0, 0), alias=None, **kw):
    """eng.mix_f32 on host arrays -> the host result; off: elements past a 16-byte boundary of a, b, dst, mask; alias: 'a' / 'b' (dst is that
    tensor) or 'ab' (b is a).  The destination lies between two guards of GUARD floats, which must come back untouched."""
    mem = eng.mem
    abuf, ta, a0 = placed(eng, a, off[0], GUARD)
    bbuf, tb, b0 = (abuf, ta, a0) if alias == "ab" else placed(eng, b, off[1], GUARD)
    m = placed(eng, mask, off[3], 0, u8=True)[1] if mask is not None else None
    if alias == "a":
        dbuf, d, d0 = abuf, ta, a0
    elif alias == "b":
        dbuf, d, d0 = bbuf, tb, b0
    else:
        dbuf, d, d0 = placed(eng, np.full(a.shape, SENTINEL, np.float32), off[2], GUARD)
    w = eng.i32_buffer(weights) if weights is not None else None
    eng.mix_f32(ta, tb, d, weights=w, mask=m, in_hw=in_hw, **kw)
    whole = np.array(mem.to_numpy(dbuf), copy=True).reshape(-1)
    assert np.all(whole[:d0] == SENTINEL) and np.all(whole[d0 + a.size:] == SENTINEL), "a write outside the destination"
    return whole[d0:d0 + a.size].reshape(a.shape)


# ================================================================ data
SHAPES = [(1, 1, 4, 4), (3, 5, 4, 8), (17, 31, 20, 32), (64, 48, 64, 48)]                       # H, W, Ho, Wo
N = 3
WEIGHTS = (0, 1, 77, 128, 255, 256)
DEVICE_WEIGHTS = ([0, 77, 256], [-5, 300, 128])
_cases = {}


def case(shape):
    """(a [3,Ho,Wo,3], b [3,Ho,Wo,3], masks {name: uint8 [H,W] or None}) of one shape, built once and read-only.  Each tensor holds
    test_compose's three images: noise; floats off the scale, NaN, infinities and v + j / 256 -+ 1e-4; a 0 | 255 checkerboard."""
    if shape not in _cases:
        H, W, Ho, Wo = shape
        a, b = images(Ho, Wo, 7 + H), images(Ho, Wo, 10 + Wo)
        rs = np.random.RandomState(H * 1000 + W)
        masks = {"none": None, "noise": rs.randint(0, 256, (H, W)).astype(np.uint8),
                 "steps": np.array([0, 127, 128, 255], np.uint8)[rs.randint(0, 4, (H, W))]}
        for t in (a, b, masks["noise"], masks["steps"]):
            t.setflags(write=False)
        _cases[shape] = (a, b, masks)
    return _cases[shape]


# ================================================================ the restatement itself (CPU)
def test_restatement_known_answers():
    one = lambda v: np.full((1, 1, 1, 3), v, np.float32)
    assert mix_F(one(0.0), one(255.0), t=128).tolist() == [[[[32640] * 3]]]                     # 127.5
    assert mix_F(one(255.0), one(0.0), t=128).tolist() == [[[[32640] * 3]]]
    m = np.array([[0, 127, 128, 255]], np.uint8)
    a, b = np.zeros((1, 1, 4, 3), np.float32), np.full((1, 1, 4, 3), 255.0, np.float32)
    assert mix_F(a, b, mask=m)[0, 0, :, 0].tolist() == [0, 255 * 127, 255 * 129, FMAX]          # m' = 0, 127, 129, 256 over 256
    assert mix_F(a, b, t=[-5]).max() == 0 and mix_F(a, b, t=[300]).min() == FMAX                # the clamp of a weight read from memory
    # the checkerboards put both ends of the scale on either side: the rounding passes neither (mix_F asserts it) at every weight
    a, b, masks = case((64, 48, 64, 48))
    for t in range(0, 257):
        mix_F(a[2:], b[2:], t=t, mask=masks["noise"])


# ================================================================ the device against the restatement
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_every_weight_and_mask_matches_the_restatement(eng, shape):
    a, b, masks = case(shape)
    assert a.shape == b.shape == (N,) + shape[2:] + (3,)
    for mk in ("none", "noise", "steps"):
        for t in WEIGHTS:
            got = run(eng, a, b, shape[:2], mask=masks[mk], weight_q8=t)
            assert same(got, mix_ref(a, b, t=t, mask=masks[mk], in_hw=shape[:2])), (t, mk)
        for ws in DEVICE_WEIGHTS:
            got = run(eng, a, b, shape[:2], mask=masks[mk], weights=ws, weight_q8=999)            # (weight_q8 is ignored beside the buffer)
            assert same(got, mix_ref(a, b, t=ws, mask=masks[mk], in_hw=shape[:2])), (ws, mk)
    # one image, no batch axis
    got = run(eng, a[1], b[1], shape[:2], mask=masks["steps"], weight_q8=77)
    assert same(got, mix_ref(a[1:2], b[1:2], t=77, mask=masks["steps"], in_hw=shape[:2])[0])


@pytest.mark.parametrize("off", [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (2, 3, 1, 3)], ids=lambda o: "off_%d%d%d%d" % o)
def test_a_misaligned_tensor_takes_the_narrow_path_with_the_same_values(eng, off):
    """64 x 48 -> 64 x 48 is the wide path (16-byte accesses, mask dwords); one float off 16-byte alignment in any tensor takes single floats,
    one byte off in the mask takes single bytes: the values are those of the aligned run."""
    shape = (64, 48, 64, 48)
    a, b, masks = case(shape)
    for kw, mk in (dict(weight_q8=77), "noise"), (dict(weights=[0, 77, 256]), "steps"), (dict(weights=[-5, 300, 128]), "none"):
        wide = run(eng, a, b, shape[:2], mask=masks[mk], **kw)
        got = run(eng, a, b, shape[:2], mask=masks[mk], off=off, **kw)
        t = kw.get("weights", kw.get("weight_q8"))
        assert same(got, wide) and same(got, mix_ref(a, b, t=t, mask=masks[mk])), (kw, mk)


@pytest.mark.parametrize("shape", [(17, 31, 20, 32), (64, 48, 64, 48), (3, 5, 4, 8)], ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_the_destination_may_be_either_source_and_the_sources_may_be_one(eng, shape):
    a, b, masks = case(shape)
    for alias in ("a", "b"):
        for kw in (dict(weight_q8=77), dict(weights=[0, 77, 256])):
            got = run(eng, a, b, shape[:2], mask=masks["noise"], alias=alias, **kw)
            assert same(got, mix_ref(a, b, t=kw.get("weights", 77), mask=masks["noise"], in_hw=shape[:2])), (alias, kw)
    for t in (0, 77, 256):                                                                      # a is b: to88 of it at every weight
        assert same(run(eng, a, a, shape[:2], mask=masks["steps"], alias="ab", weight_q8=t), f32_of_F(to88(a))), t
        assert same(run(eng, a, a, shape[:2], alias="a", weight_q8=t), f32_of_F(to88(a))), t


def test_consequences_of_the_contract(eng):
    shape = (17, 31, 20, 32)
    H, W, Ho, Wo = shape
    a, b, masks = case(shape)
    A, B = f32_of_F(to88(a)), f32_of_F(to88(b))
    yi, xi = np.minimum(np.arange(Ho), H - 1), np.minimum(np.arange(Wo), W - 1)
    # weight 0: to88(a), with any mask; weight 256 without a mask: to88(b), whose high byte is what fs_f32_to_u8 writes for b
    for mk in ("none", "noise", "steps"):
        assert same(run(eng, a, b, (H, W), mask=masks[mk], weight_q8=0), A), mk
        assert same(run(eng, a, b, (H, W), mask=masks[mk], weights=[0, -5, 0]), A), mk
    for got in (run(eng, a, b, (H, W), weight_q8=256), run(eng, a, b, (H, W), weights=[256, 300, 256]),
                run(eng, a, b, (H, W), mask=np.full((H, W), 255, np.uint8), weight_q8=256)):
        assert same(got, B)
    for src, F in ((a, A), (b, B)):
        with np.errstate(invalid="ignore"):
            u8 = np.where(np.isnan(src), 0, np.clip(src, 0, 255)).astype(np.uint8)
        assert np.array_equal((to88(F) >> 8).astype(np.uint8), u8)
    # a zero mask byte: a at that pixel; a 255 byte: b at weight 256, the unmasked result otherwise
    half = np.zeros((H, W), np.uint8)
    half[:, W // 2:] = 255
    hx = half[yi][:, xi][0] == 255                                                              # (the last column serves the extra ones)
    for t in (256, 200):
        got = run(eng, a, b, (H, W), mask=half, weight_q8=t)
        free = run(eng, a, b, (H, W), weight_q8=t)
        assert same(got[:, :, ~hx], A[:, :, ~hx]) and same(got[:, :, hx], free[:, :, hx])
        if t == 256:
            assert same(got[:, :, hx], B[:, :, hx])
    # half weight between 0 and 255, either way round: 127.5
    lo, hi = np.zeros((1, 8, 8, 3), np.float32), np.full((1, 8, 8, 3), 255.0, np.float32)
    assert np.all(run(eng, lo, hi, (5, 7), weight_q8=128) == np.float32(127.5))
    assert np.all(run(eng, hi, lo, (5, 7), weights=[128]) == np.float32(127.5))


def test_refused_calls_return_their_code_and_launch_nothing(eng):
    mem, lib, ctx = eng.mem, eng.lib, eng.ctx
    H, W, Ho, Wo = 17, 31, 20, 32
    a, b, masks = case((H, W, Ho, Wo))
    _, ta, _ = placed(eng, a, 0, 0)
    _, tb, _ = placed(eng, b, 0, 0)
    dbuf, d, d0 = placed(eng, np.full(a.shape, SENTINEL, np.float32), 0, GUARD)
    m = placed(eng, masks["noise"], 0, 0, u8=True)[1]
    w = eng.i32_buffer([0, 77, 256, 1])
    pa, pb, pd, pm, pw = mem.ptr(ta), mem.ptr(tb), mem.ptr(d), mem.ptr_u8(m), mem.ptr_u8(w)
    assert pw % 4 == 0
    eng._sync_stream()

    def call(a=pa, b=pb, H=H, W=W, Ho=Ho, Wo=Wo, N=N, q8=200, wdev=None, mask=pm, dst=pd):
        return lib.fs_mix_f32(ctx, a, b, H, W, Ho, Wo, N, q8, wdev, mask, dst)

    refused = [(-1, dict(a=None)), (-1, dict(b=None)), (-1, dict(dst=None)), (-1, dict(N=0)), (-1, dict(N=65536)), (-1, dict(N=-1)),
               (-1, dict(H=0)), (-1, dict(W=0)), (-1, dict(H=-3)), (-1, dict(Ho=H - 1)), (-1, dict(Ho=H + 4)), (-1, dict(Wo=W - 1)),
               (-1, dict(Wo=W + 4)), (-1, dict(H=2 ** 31 - 1)), (-2, dict(q8=-1)), (-2, dict(q8=257)), (-5, dict(a=pa + 2)), (-5, dict(b=pb + 1)),
               (-5, dict(dst=pd + 3)), (-5, dict(wdev=pw + 2)), (-5, dict(wdev=pw + 1, q8=999))]
    for code, kw in refused:
        assert call(**kw) == code, kw
        assert b"fs_mix_f32" in lib.fs_last_error()
    assert np.all(np.asarray(mem.to_numpy(dbuf)) == SENTINEL)                                 # nothing was launched
    assert lib.fs_mix_f32(None, pa, pb, H, W, Ho, Wo, N, 200, None, pm, pd) == -1
    # the call they were variations of is taken: with or without the mask, and with a weight buffer beside any weight_q8
    assert call(mask=None) == 0 and call() == 0
    got = np.asarray(mem.to_numpy(dbuf)).reshape(-1)[d0:d0 + a.size].reshape(a.shape)
    assert same(got, mix_ref(a, b, t=200, mask=masks["noise"]))
    assert call(wdev=pw, q8=999) == 0
    got = np.asarray(mem.to_numpy(dbuf)).reshape(-1)[d0:d0 + a.size].reshape(a.shape)
    assert same(got, mix_ref(a, b, t=[0, 77, 256], mask=masks["noise"]))
    # the engine's own shape checks
    with pytest.raises(L.FaststyleError):
        eng.mix_f32(ta, tb, d, mask=mem.upload_u8(np.zeros((H, W + 1), np.uint8)), in_hw=(H, W))
    with pytest.raises(L.FaststyleError):
        eng.mix_f32(ta, mem.view(tb, 0, (N, Ho * 2, Wo // 2, 3)), d)
    with pytest.raises(L.FaststyleError):
        eng.mix_f32(ta, tb, d, weights=eng.i32_buffer([1, 2]))
    with pytest.raises(L.FaststyleError):
        eng.mix_f32(ta, tb, d, mask=m, in_hw=(Ho, Wo))                                          # (without in_hw the mask's shape is the input size)
