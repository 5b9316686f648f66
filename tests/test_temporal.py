"""Temporal stabilisation on the device (csrc/fs_temporal.hip) against the contract, the arithmetic that include/faststyle_io.h states.  The
first part of this file is an independent numpy restatement of that text (int64 and >>); every comparison of the device with the
restatement -- luma, vectors, the 8.8 state and the float result -- is equality.  The same bodies run on the CPU emulator and, under -m gpu,
on the MI355X.  tests/test_temporal_stream.py builds its expected tensors with the restatement."""
import itertools

import numpy as np
import pytest

from faststyle_amd import _lib as L
from tests import backends
from tests.test_compose import GUARD, LUMA, SENTINEL, images, placed, same, to88

FILL = 201                                                      # what test_compose.placed puts around a u8 buffer


# ================================================================ the restatement
def luma8(src, Ho, Wo, matrix=0, bgr=False):
    """src float32 [H,W,3] -> cur8 uint8 [Ho,Wo]"""
    H, W = src.shape[:2]
    assert H <= Ho <= H + 3 and W <= Wo <= W + 3
    A = to88(src)[np.minimum(np.arange(Ho), H - 1)][:, np.minimum(np.arange(Wo), W - 1)]
    kr, kg, kb = LUMA[matrix]
    k0, k2 = (kb, kr) if bgr else (kr, kb)
    Y = (k0 * A[..., 0] + kg * A[..., 1] + k2 * A[..., 2] + 32768) >> 16
    return (Y >> 8).astype(np.uint8)


def blocks_of(Ho, Wo):
    return (Ho + 15) // 16, (Wo + 15) // 16


def search(cur8, prev8, R, penalty=True):
    """-> mv int8 [nby,nbx,2]; prev8 None: zeros.  penalty=False is NOT the contract: the tests use it to show that a case depends on the
    motion penalty."""
    Ho, Wo = cur8.shape
    nby, nbx = blocks_of(Ho, Wo)
    if prev8 is None:
        return np.zeros((nby, nbx, 2), np.int8)
    ys, xs = np.arange(0, Ho, 16), np.arange(0, Wo, 16)
    npix = np.minimum(16, Ho - ys)[:, None] * np.minimum(16, Wo - xs)[None, :]
    c = cur8.astype(np.int64)
    P = np.pad(prev8.astype(np.int64), R, mode="edge")          # (|dy|, |dx| <= R: the padding is the clamp)
    best = np.full((nby, nbx), np.iinfo(np.int64).max)
    for dy, dx in itertools.product(range(-R, R + 1), repeat=2):
        D = np.abs(c - P[R + dy:R + dy + Ho, R + dx:R + dx + Wo])
        sad = np.add.reduceat(np.add.reduceat(D, ys, axis=0), xs, axis=1)
        mag = abs(dy) + abs(dx)
        cost = sad + (npix >> 5) * mag * int(penalty)
        assert cost.max() < 1 << 17
        best = np.minimum(best, (cost << 12) | (mag << 8) | ((dy + 7) << 4) | (dx + 7))
    return np.stack([((best >> 4) & 15) - 7, (best & 15) - 7], axis=-1).astype(np.int8)


def blend(cur, cur8, prev8, prev88, mv, q8, K):
    """-> F int64 [Ho,Wo,3]"""
    B = to88(cur)
    if prev8 is None:
        return B
    Ho, Wo = cur8.shape
    y, x = np.indices((Ho, Wo))
    v = mv.astype(np.int64)[y >> 4, x >> 4]
    qy, qx = np.clip(y + v[..., 0], 0, Ho - 1), np.clip(x + v[..., 1], 0, Wo - 1)
    e = np.abs(cur8.astype(np.int64) - prev8.astype(np.int64)[qy, qx])
    w = q8 * np.maximum(0, 256 - e * K)
    assert w.min() >= 0 and w.max() <= 65536
    P = prev88.astype(np.int64)[qy, qx]
    F = B + (((P - B) * w[..., None] + 32768) >> 16)
    assert F.min() >= 0 and F.max() <= 65280                    # a convex combination: no clamp
    return F


def temporal_ref(src, cur, prev=None, q8=256, K=16, R=7, matrix=0, bgr=False):
    """src [H,W,3], cur [Ho,Wo,3], prev (luma u8, out88 u16) or None -> dict(luma=, mv=, out88= uint16, dst= float32)"""
    Ho, Wo = cur.shape[:2]
    c8 = luma8(src, Ho, Wo, matrix, bgr)
    p8, p88 = prev if prev is not None else (None, None)
    mv = search(c8, p8, R)
    F = blend(cur, c8, p8, p88, mv, q8, K)
    return dict(luma=c8, mv=mv, out88=F.astype(np.uint16), dst=F.astype(np.float32) * np.float32(0.00390625))


# ================================================================ running the device call
@pytest.fixture(params=backends.engine_params())
def eng(request):
    return backends.get_engine(request.param)


def slot_buffers(eng, Ho, Wo, fill=None, off=0):
    """A guarded state slot: [(buffer, view, start), ...] for luma, out88, mv; fill: host (luma u8, out88 u16) to start from"""
    nby, nbx = blocks_of(Ho, Wo)
    init = [np.zeros((Ho, Wo), np.uint8), np.zeros((Ho, Wo, 3, 2), np.uint8), np.zeros((nby, nbx, 2), np.uint8)]
    if fill is not None:
        init[0] = np.ascontiguousarray(fill[0], np.uint8)
        init[1] = np.ascontiguousarray(fill[1], "<u2").view(np.uint8).reshape(Ho, Wo, 3, 2)
    return [placed(eng, a, off, GUARD, u8=True) for a in init]


def read_slot(eng, bufs, Ho, Wo):
    """The three arrays of a slot, after checking that nothing outside them was written"""
    out = []
    for (buf, view, start), dt in zip(bufs, (np.uint8, "<u2", np.int8)):
        whole = np.array(eng.mem.to_numpy(buf), copy=True).reshape(-1)
        n = int(np.prod(view.shape))
        assert np.all(whole[:start] == FILL) and np.all(whole[start + n:] == FILL), "a write outside the state"
        out.append(whole[start:start + n].view(dt))
    nby, nbx = blocks_of(Ho, Wo)
    return out[0].reshape(Ho, Wo), out[1].reshape(Ho, Wo, 3), out[2].reshape(nby, nbx, 2)


def run(eng, src, cur, prev=None, alias=False, off=(0, 0, 0), soff=0, **kw):
    """eng.temporal_f32 on host arrays -> dict as temporal_ref's; off: floats past a 16-byte boundary of src, cur, dst; soff: bytes of
    the state buffers.  Every output lies between guards, which must come back untouched."""
    mem = eng.mem
    Ho, Wo = cur.shape[:2]
    _, s, _ = placed(eng, src, off[0], 0)
    cbuf, c, c0 = placed(eng, cur, off[1], GUARD)
    dbuf, d, d0 = (cbuf, c, c0) if alias else placed(eng, np.full(cur.shape, SENTINEL, np.float32), off[2], GUARD)
    state = slot_buffers(eng, Ho, Wo, off=soff)
    before = slot_buffers(eng, Ho, Wo, fill=prev, off=soff) if prev is not None else None
    eng.temporal_f32(s, c, d, tuple(b[1] for b in state), prev=None if before is None else tuple(b[1] for b in before), **kw)
    whole = np.array(mem.to_numpy(dbuf), copy=True).reshape(-1)
    assert np.all(whole[:d0] == SENTINEL) and np.all(whole[d0 + cur.size:] == SENTINEL), "a write outside the destination"
    luma, out88, mv = read_slot(eng, state, Ho, Wo)
    if before is not None:                                      # the previous state is read only
        pl, po, _ = read_slot(eng, before, Ho, Wo)
        assert np.array_equal(pl, prev[0]) and np.array_equal(po, prev[1])
    return dict(luma=luma, mv=mv, out88=out88, dst=whole[d0:d0 + cur.size].reshape(cur.shape))


def device_kw(q8=256, K=16, R=7, matrix=0, bgr=False):
    return dict(strength_q8=q8, sensitivity=K, radius=R, matrix=matrix, src_bgr=bgr)


def equal(got, want):
    return all(np.array_equal(got[k], want[k]) for k in ("luma", "mv", "out88")) and same(got["dst"], want["dst"]) and \
        got["mv"].dtype == np.int8 and got["out88"].dtype.kind == "u"


# ================================================================ data
SHAPES = [(1, 1, 1, 1), (16, 16, 16, 16), (14, 30, 17, 33), (40, 52, 40, 52), (64, 48, 64, 48)]     # H, W, Ho, Wo
RADII, SENSITIVITIES, STRENGTHS = (0, 3, 7), (1, 16, 256), (0, 77, 128, 256)
_cases = {}


def case(shape):
    """Two consecutive frames of one shape, in the three kinds of tests.test_compose.images (noise; values off the scale, NaN, infinities
    and v + j / 256 -+ 1e-4; a checkerboard), built once and read-only: (src0, cur0, src1, cur1), each [3, ...].  The second source is the
    first moved by (2, -3) under a little noise, so that the search has something to find and the confidence takes every value."""
    if shape not in _cases:
        H, W, Ho, Wo = shape
        src0, cur0, cur1 = images(H, W, 7 + H), images(Ho, Wo, 10 + Wo), images(Ho, Wo, 12 + Wo)
        rs = np.random.RandomState(H * 1000 + W)
        src1 = np.roll(src0, (2, -3), axis=(1, 2)) + rs.randint(-2, 3, src0.shape).astype(np.float32)
        cur1[0] = cur0[0] + rs.randint(-20, 21, cur0[0].shape).astype(np.float32)
        for a in (src0, cur0, src1, cur1):
            a.setflags(write=False)
        _cases[shape] = (src0, cur0, src1, cur1)
    return _cases[shape]


def grey(a):
    """uint8 [H,W] -> float32 [H,W,3] whose luma is a, under either matrix and channel order (each weight triple sums to 65536)"""
    return np.repeat(a.astype(np.float32)[..., None], 3, axis=-1)


# ================================================================ the restatement itself (CPU)
def test_restatement_known_answers():
    assert luma8(np.array([[[255.0, 0.0, 0.0]]], np.float32), 1, 1, 0, False)[0, 0] == (19595 * 65280 + 32768) >> 24
    assert luma8(np.array([[[255.0, 0.0, 0.0]]], np.float32), 1, 1, 1, True)[0, 0] == (4732 * 65280 + 32768) >> 24
    a = np.random.RandomState(1).randint(0, 256, (40, 52)).astype(np.uint8)
    assert np.array_equal(luma8(grey(a), 40, 52, 1, True), a)
    # a frame against itself: at rest; against itself moved: the move (block (1, 1) of 3 x 4 has its whole window inside the frame)
    assert not search(a, a, 7).any()
    moved = np.roll(a, (-3, 5), axis=(0, 1))                    # moved[y][x] = a[y + 3][x - 5]
    assert search(moved, a, 7)[1, 1].tolist() == [3, -5]
    # half strength between 0 and 255 at full confidence: 127.5
    one = lambda v: np.full((1, 1, 3), v, np.float32)
    F = blend(one(255.0), np.zeros((1, 1), np.uint8), np.zeros((1, 1), np.uint8), np.zeros((1, 1, 3), np.uint16), np.zeros((1, 1, 2), np.int8), 128, 16)
    assert F.tolist() == [[[32640] * 3]]


# ================================================================ the device against the restatement
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_two_frames_match_the_restatement(eng, shape):
    """Both matrices, both channel orders and every radius; the sensitivities and strengths go round so that each of their twelve pairs
    occurs per shape; every data kind; a first frame (no previous state) and a second one fed with the first one's state."""
    src0, cur0, src1, cur1 = case(shape)
    combos = list(itertools.product((0, 1), (False, True), RADII))
    assert len(combos) == 12 and len({(SENSITIVITIES[i % 3], STRENGTHS[i % 4]) for i in range(12)}) == 12
    for i, (matrix, bgr, R) in enumerate(combos):
        kw = dict(q8=STRENGTHS[i % 4], K=SENSITIVITIES[i % 3], R=R, matrix=matrix, bgr=bgr)
        kind = i % 3
        first = run(eng, src0[kind], cur0[kind], **device_kw(**kw))
        assert equal(first, temporal_ref(src0[kind], cur0[kind], **kw)), ("first", kw)
        assert not first["mv"].any() and same(first["dst"], to88(cur0[kind]).astype(np.float32) / np.float32(256))
        prev = (first["luma"], first["out88"])
        second = run(eng, src1[kind], cur1[kind], prev=prev, **device_kw(**kw))
        assert equal(second, temporal_ref(src1[kind], cur1[kind], prev=prev, **kw)), ("second", kw)


def test_the_cases_exercise_the_search_and_the_blend():
    """(of the restatement alone) the second frames find a non-zero vector, and the blend weight takes values strictly between its ends"""
    src0, cur0, src1, cur1 = case((64, 48, 64, 48))
    p8 = luma8(src0[0], 64, 48)
    c8 = luma8(src1[0], 64, 48)
    mv = search(c8, p8, 7)
    assert mv[1, 1].tolist() == [-2, 3]
    y, x = np.indices((64, 48))
    v = mv.astype(np.int64)[y >> 4, x >> 4]
    e = np.abs(c8.astype(np.int64) - p8.astype(np.int64)[np.clip(y + v[..., 0], 0, 63), np.clip(x + v[..., 1], 0, 47)])
    conf = np.maximum(0, 256 - 16 * e)
    assert (conf == 256).any() and (conf == 0).any() and ((conf > 0) & (conf < 256)).any()


@pytest.mark.parametrize("shift", [(0, 0), (3, -5), (-7, 7), (7, -7)], ids=lambda s: "dy%d_dx%d" % s)
def test_a_moved_noise_texture_yields_its_vector(eng, shift):
    Ho, Wo = 64, 48
    a = np.random.RandomState(5).randint(0, 256, (Ho, Wo)).astype(np.uint8)
    dy, dx = shift
    moved = np.roll(a, (-dy, -dx), axis=(0, 1))                 # moved[y][x] = a[y + dy][x + dx]
    got = run(eng, grey(moved), grey(moved), prev=(a, np.zeros((Ho, Wo, 3), np.uint16)), **device_kw())
    assert np.array_equal(got["luma"], moved)
    inside = [(by, bx) for by in range(4) for bx in range(3) if by * 16 >= 7 and by * 16 + 23 <= Ho and bx * 16 >= 7 and bx * 16 + 23 <= Wo]
    assert inside == [(1, 1), (2, 1)]
    for by, bx in inside:
        assert got["mv"][by, bx].tolist() == [dy, dx]
    assert np.array_equal(got["mv"], search(moved, a, 7))


def test_flat_and_periodic_frames_follow_the_tie_rule(eng):
    Ho, Wo = 64, 48
    zero88 = np.zeros((Ho, Wo, 3), np.uint16)
    # a constant frame: every candidate has SAD 0, the smallest motion wins
    flat = np.full((Ho, Wo), 93, np.uint8)
    assert not run(eng, grey(flat), grey(flat), prev=(flat, zero88), **device_kw())["mv"].any()
    # period 4 in x, moved by half a period: dx = -2 and dx = +2 both match exactly (as do -6 and +6, with more motion), at one cost and one
    # magnitude; dy is 0 for both, so the smaller dx wins.  The same along y: the smaller dy.
    px = np.broadcast_to(np.array([10, 200, 90, 140], np.uint8)[np.arange(Wo) % 4], (Ho, Wo))
    got = run(eng, grey(np.roll(px, 2, axis=1)), grey(px), prev=(px, zero88), **device_kw())["mv"]
    assert all(got[by, 1].tolist() == [0, -2] for by in (1, 2)) and np.array_equal(got, search(np.roll(px, 2, axis=1), px, 7))
    py = np.ascontiguousarray(np.broadcast_to(np.array([10, 200, 90, 140], np.uint8)[np.arange(Ho) % 4][:, None], (Ho, Wo)))
    got = run(eng, grey(np.roll(py, 2, axis=0)), grey(py), prev=(py, zero88), **device_kw())["mv"]
    assert all(got[by, 1].tolist() == [-2, 0] for by in (1, 2))
    # unmoved: at rest, although dx = -4 and +4 match as well
    assert not run(eng, grey(px), grey(px), prev=(px, zero88), **device_kw())["mv"][1:3, 1].any()


def test_the_motion_penalty_pulls_a_noisy_flat_frame_towards_rest(eng):
    """Two flat frames under independent noise of one level: every candidate's SAD is about npix / 2 and the differences between them are
    chance (a standard deviation of 8 for a whole block), so without the penalty the vectors are arbitrary; (npix >> 5) per pixel of motion
    leaves only short ones."""
    Ho, Wo = 40, 52
    rs = np.random.RandomState(21)
    p8, c8 = (100 + rs.randint(0, 2, (Ho, Wo))).astype(np.uint8), (100 + rs.randint(0, 2, (Ho, Wo))).astype(np.uint8)
    want = search(c8, p8, 7)
    free = search(c8, p8, 7, penalty=False)
    assert not np.array_equal(want, free) and 2 * np.abs(want).sum() < np.abs(free).sum()   # (of the restatement alone)
    got = run(eng, grey(c8), grey(c8), prev=(p8, np.zeros((Ho, Wo, 3), np.uint16)), **device_kw())
    assert np.array_equal(got["luma"], c8) and np.array_equal(got["mv"], want)


@pytest.mark.parametrize("shift", [(-7, -7), (7, 7), (-7, 7), (7, -7)], ids=lambda s: "dy%d_dx%d" % s)
def test_vectors_that_point_out_of_the_frame_follow_the_clamp(eng, shift):
    """cur8[y][x] = prev8[clampy(y + dy)][clampx(x + dx)] by construction, so the candidate (dy, dx) has SAD 0 in every block only if the
    search clamps both coordinates at both ends as the contract says; 40 x 52 has ragged blocks on the right (4 wide) and at the bottom (8
    high).  Where whole rows or columns of a block are replicas, a smaller vector matches as well and the tie rule names it."""
    Ho, Wo = 40, 52
    dy, dx = shift
    p8 = np.random.RandomState(22).randint(0, 256, (Ho, Wo)).astype(np.uint8)
    c8 = p8[np.clip(np.arange(Ho) + dy, 0, Ho - 1)][:, np.clip(np.arange(Wo) + dx, 0, Wo - 1)]
    got = run(eng, grey(c8), grey(c8), prev=(p8, np.zeros((Ho, Wo, 3), np.uint16)), **device_kw())["mv"]
    assert np.array_equal(got, search(c8, p8, 7))
    assert got[1, 1].tolist() == [dy, dx]                       # rows 16 .. 31, columns 16 .. 31: nothing clamps, nothing is replicated
    if shift == (-7, -7):                                       # rows and columns 0 .. 7 are replicas of the first; 8 .. 15 are not
        assert got[0, 0].tolist() == [-7, -7]
    if shift == (7, 7):                                         # the 8 x 4 corner block is one value: dy = 7 and any dx >= 3 match
        assert got[2, 3].tolist() == [7, 3]


@pytest.mark.parametrize("shape", [(14, 30, 17, 33), (64, 48, 64, 48)], ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_the_destination_may_be_the_current_tensor(eng, shape):
    src0, cur0, src1, cur1 = case(shape)
    Ho, Wo = shape[2:]
    prev = (luma8(src0[0], Ho, Wo), to88(cur0[0]).astype(np.uint16))
    for kw in (dict(q8=77, K=1), dict(q8=256, K=16, R=3, matrix=1, bgr=True)):
        got = run(eng, src1[0], cur1[0], prev=prev, alias=True, **device_kw(**kw))
        assert equal(got, temporal_ref(src1[0], cur1[0], prev=prev, **kw)), kw


def test_tensors_off_sixteen_byte_alignment_give_the_same_values(eng):
    """(one access path; held at one float / one sample off alignment all the same)"""
    src0, cur0, src1, cur1 = case((40, 52, 40, 52))
    prev = (luma8(src0[0], 40, 52), to88(cur0[0]).astype(np.uint16))
    want = temporal_ref(src1[0], cur1[0], prev=prev, q8=128, K=16)
    for off, soff in (((1, 0, 0), 0), ((0, 1, 0), 0), ((0, 0, 1), 0), ((0, 0, 0), 2), ((3, 2, 1), 6)):
        assert equal(run(eng, src1[0], cur1[0], prev=prev, off=off, soff=soff, **device_kw(q8=128, K=16)), want), (off, soff)


def test_consequences_of_the_contract(eng):
    shape = (14, 30, 17, 33)
    src0, cur0, src1, cur1 = case(shape)
    Ho, Wo = shape[2:]
    rs = np.random.RandomState(11)
    prev88 = rs.randint(0, 65281, (Ho, Wo, 3)).astype(np.uint16)
    for kind in range(3):
        B = to88(cur1[kind])
        prev = (luma8(src0[kind], Ho, Wo), prev88)
        # strength 0 and the first frame: F = to88(cur), whose high byte is what fs_f32_to_u8 writes
        for got in (run(eng, src1[kind], cur1[kind], prev=prev, **device_kw(q8=0)), run(eng, src1[kind], cur1[kind], **device_kw(q8=256))):
            assert np.array_equal(got["out88"], B) and same(got["dst"], B.astype(np.float32) / np.float32(256))
            with np.errstate(invalid="ignore"):
                u8 = np.where(np.isnan(cur1[kind]), 0, np.clip(cur1[kind], 0, 255)).astype(np.uint8)
            assert np.array_equal((got["out88"] >> 8).astype(np.uint8), u8)
    # e K >= 256 everywhere: a luma that differs by at least 1 everywhere at K = 256, by at least 16 at K = 16
    a = rs.randint(0, 100, (Ho, Wo)).astype(np.uint8)
    for K, step in ((256, 1), (16, 16)):
        got = run(eng, grey(a + step + 100), cur1[0], prev=(a, prev88), **device_kw(q8=256, K=K))
        assert np.array_equal(got["out88"], to88(cur1[0]))
    # strength 256 and e = 0: F = P exactly (a frame against itself is at rest, so P is the previous output at the same pixel)
    for K in (1, 256):
        got = run(eng, grey(a), cur1[1], prev=(a, prev88), **device_kw(q8=256, K=K))
        assert not got["mv"].any() and np.array_equal(got["out88"], prev88) and same(got["dst"], prev88.astype(np.float32) / np.float32(256))
    # ... and along a vector: the previous output fetched from where the source came from
    a = rs.randint(0, 256, (64, 48)).astype(np.uint8)
    p88 = rs.randint(0, 65281, (64, 48, 3)).astype(np.uint16)
    moved = np.roll(a, (-3, 5), axis=(0, 1))
    got = run(eng, grey(moved), np.zeros((64, 48, 3), np.float32), prev=(a, p88), **device_kw(q8=256, K=1))
    assert got["mv"][1, 1].tolist() == [3, -5] and np.array_equal(got["out88"][16:32, 16:32], p88[19:35, 11:27])


def test_refused_calls_return_their_code_and_launch_nothing(eng):
    mem, lib, ctx = eng.mem, eng.lib, eng.ctx
    H, W, Ho, Wo = 14, 30, 17, 33
    src0, cur0, src1, cur1 = case((H, W, Ho, Wo))
    _, s, _ = placed(eng, src1[0], 0, 0)
    _, c, _ = placed(eng, cur1[0], 0, 0)
    dbuf, d, d0 = placed(eng, np.full(cur1[0].shape, SENTINEL, np.float32), 0, GUARD)
    state = slot_buffers(eng, Ho, Wo)
    prevh = (luma8(src0[0], Ho, Wo), to88(cur0[0]).astype(np.uint16))
    before = slot_buffers(eng, Ho, Wo, fill=prevh)
    for _, view, _ in state:                                    # (so that a launch of any of the three kernels would show)
        if hasattr(view, "fill_"):
            view.fill_(FILL)
        else:
            view[...] = FILL
    ps, pc, pd = mem.ptr(s), mem.ptr(c), mem.ptr(d)
    pl, po, pm = (mem.ptr_u8(b[1]) for b in state)
    ql, qo = mem.ptr_u8(before[0][1]), mem.ptr_u8(before[1][1])
    eng._sync_stream()

    def call(src=ps, H=H, W=W, cur=pc, Ho=Ho, Wo=Wo, q8=128, K=16, R=7, matrix=0, bgr=0, prev_luma=ql, prev_out88=qo, luma=pl, out88=po, mv=pm,
             dst=pd):
        return lib.fs_temporal_f32(ctx, src, H, W, cur, Ho, Wo, q8, K, R, matrix, bgr, prev_luma, prev_out88, luma, out88, mv, dst)

    refused = [(-1, dict(src=None)), (-1, dict(cur=None)), (-1, dict(luma=None)), (-1, dict(out88=None)), (-1, dict(mv=None)), (-1, dict(dst=None)),
               (-1, dict(prev_luma=None)), (-1, dict(prev_out88=None)), (-1, dict(prev_luma=pl)), (-1, dict(prev_out88=po)),
               (-1, dict(H=0)), (-1, dict(W=0)), (-1, dict(H=-3)), (-1, dict(Ho=H - 1)), (-1, dict(Ho=H + 4)), (-1, dict(Wo=W - 1)),
               (-1, dict(Wo=W + 4)), (-1, dict(H=2 ** 31 - 1)),
               (-2, dict(q8=-1)), (-2, dict(q8=257)), (-2, dict(K=0)), (-2, dict(K=257)), (-2, dict(R=-1)), (-2, dict(R=8)), (-2, dict(matrix=2)),
               (-2, dict(matrix=-1)), (-2, dict(bgr=2)), (-2, dict(bgr=-1)),
               (-5, dict(src=ps + 2)), (-5, dict(cur=pc + 1)), (-5, dict(dst=pd + 3)), (-5, dict(out88=po + 1)), (-5, dict(prev_out88=qo + 1))]
    for code, kw in refused:
        assert call(**kw) == code, kw
        assert b"fs_temporal_f32" in lib.fs_last_error()
    assert lib.fs_temporal_f32(None, ps, H, W, pc, Ho, Wo, 128, 16, 7, 0, 0, ql, qo, pl, po, pm, pd) == -1
    assert np.all(np.asarray(mem.to_numpy(dbuf)) == SENTINEL)                                 # nothing was launched
    assert all(np.all(np.asarray(mem.to_numpy(b[0])) == FILL) for b in state)
    # the call they were variations of is taken, with and without a previous frame
    assert call() == 0
    got = np.asarray(mem.to_numpy(dbuf)).reshape(-1)[d0:d0 + cur1[0].size].reshape(cur1[0].shape)
    want = temporal_ref(src1[0], cur1[0], prev=prevh, q8=128)
    luma, out88, mv = read_slot(eng, state, Ho, Wo)
    assert same(got, want["dst"]) and np.array_equal(luma, want["luma"]) and np.array_equal(out88, want["out88"]) and np.array_equal(mv, want["mv"])
    assert call(prev_luma=None, prev_out88=None) == 0
    assert np.array_equal(read_slot(eng, state, Ho, Wo)[1], to88(cur1[0]))
    # the engine checks the shapes against each other
    views = tuple(b[1] for b in state)
    small = eng.temporal_state(Ho, Wo - 1)
    for bad in (dict(cur=s), dict(state=small), dict(prev=small), dict(state=views[:2])):
        a = dict(dict(src=s, cur=c, dst=d, state=views, prev=None), **bad)
        with pytest.raises(L.FaststyleError):
            eng.temporal_f32(a["src"], a["cur"], a["dst"], a["state"], prev=a["prev"])
    with pytest.raises(L.FaststyleError):
        eng.temporal_f32(s, c, d, views, radius=8)
    assert tuple(tuple(b.shape) for b in eng.temporal_state(Ho, Wo)) == ((17, 33), (17, 33, 3, 2), (2, 3, 2))
