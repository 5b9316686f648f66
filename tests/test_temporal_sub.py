"""Quarter-pixel block vectors of the temporal stage (csrc/fs_temporal.hip: fs_temporal_sub_f32) against its contract in
include/faststyle_io.h.  The first part of this file is an independent numpy restatement of that text (int64, >> and floor division), built on
the luma, the pyramid, the coarse-to-fine search and the whole-pixel blend of tests/test_temporal.py and tests/test_temporal_pyr.py; every
comparison of the device with the restatement -- luma, the pyramid parts, mv, mvf, the 8.8 state and the float result -- is equality.  The
same bodies run on the CPU emulator and, under -m gpu, on the MI355X.  tests/test_temporal_sub_stream.py builds its expected tensors with the
restatement."""
import itertools

import numpy as np
import pytest

from faststyle_amd import _lib as L
from tests import backends
from tests.test_compose import GUARD, SENTINEL, placed, same, to88
from tests.test_temporal import FILL, blend, blocks_of, case, device_kw, grey, luma8, read_slot, slot_buffers
from tests.test_temporal import run as run_one_level
from tests.test_temporal_pyr import COMBOS, ZERO88, ids, interior, moved_pair, pyr_buffer, pyr_ref, pyramid, read_pyr, search_pyr
from tests.test_temporal_pyr import run as run_pyr


# ================================================================ the restatement
def sad(c, p, ys, xs, u, v):
    """c, p int64 [Ho,Wo]; the block's rows ys and columns xs inside the frame -> SAD(u, v), a raw sum"""
    Ho, Wo = c.shape
    return int(np.abs(c[ys][:, xs] - p[np.clip(ys + u, 0, Ho - 1)][:, np.clip(xs + v, 0, Wo - 1)]).sum())


def fit(s0, m, p, S):
    """-> the fraction in quarter pixels along one axis"""
    E = max(m, p) - s0
    if E <= 0:
        return 0
    g = ((m - p) * 2 ** S + E) // (2 * E)                       # (Python's // is a floor)
    g = min(max(g, -(2 ** (S - 1))), 2 ** (S - 1))
    return g * 2 ** (2 - S)


def refine(cur8, prev8, mv, R, S):
    """-> mvf int8 [nby,nbx,2]; without a previous frame, with R = 0 or S = 0: zeros"""
    Ho, Wo = cur8.shape
    nby, nbx = blocks_of(Ho, Wo)
    mvf = np.zeros((nby, nbx, 2), np.int8)
    if prev8 is None or R == 0 or S == 0:
        return mvf
    c, p = cur8.astype(np.int64), prev8.astype(np.int64)
    for by, bx in itertools.product(range(nby), range(nbx)):
        ys, xs = np.arange(by * 16, min(by * 16 + 16, Ho)), np.arange(bx * 16, min(bx * 16 + 16, Wo))
        dy, dx = int(mv[by, bx, 0]), int(mv[by, bx, 1])
        s0 = sad(c, p, ys, xs, dy, dx)
        mvf[by, bx] = (fit(s0, sad(c, p, ys, xs, dy - 1, dx), sad(c, p, ys, xs, dy + 1, dx), S),
                       fit(s0, sad(c, p, ys, xs, dy, dx - 1), sad(c, p, ys, xs, dy, dx + 1), S))
    assert np.abs(mvf).max() <= 2 and (S == 2 or not (mvf & 1).any())
    return mvf


def fetch(prev8, prev88, mv, mvf, bound):
    """-> (pq int64 [Ho,Wo], P int64 [Ho,Wo,3]): the previous luma and output at 4 mv + mvf quarter pixels, bilinear"""
    Ho, Wo = prev8.shape
    y, x = np.indices((Ho, Wo))
    v = np.clip(mv.astype(np.int64), -bound, bound)[y >> 4, x >> 4]
    f = np.clip(mvf.astype(np.int64), -2, 2)[y >> 4, x >> 4]
    Y4, X4 = 4 * (y + v[..., 0]) + f[..., 0], 4 * (x + v[..., 1]) + f[..., 1]
    y0, ay, x0, ax = Y4 >> 2, Y4 & 3, X4 >> 2, X4 & 3
    r0, r1, c0, c1 = np.clip(y0, 0, Ho - 1), np.clip(y0 + 1, 0, Ho - 1), np.clip(x0, 0, Wo - 1), np.clip(x0 + 1, 0, Wo - 1)

    def bil(A, ay, ax):
        return ((4 - ay) * ((4 - ax) * A[r0, c0] + ax * A[r0, c1]) + ay * ((4 - ax) * A[r1, c0] + ax * A[r1, c1]) + 8) >> 4

    return bil(prev8.astype(np.int64), ay, ax), bil(prev88.astype(np.int64), ay[..., None], ax[..., None])


def blend_sub(cur, cur8, prev8, prev88, mv, mvf, q8, K, bound):
    """-> (F int64 [Ho,Wo,3], e int64 [Ho,Wo] or None)"""
    B = to88(cur)
    if prev8 is None:
        return B, None
    pq, P = fetch(prev8, prev88, mv, mvf, bound)
    assert P.min() >= 0 and P.max() <= 65280
    e = np.abs(cur8.astype(np.int64) - pq)
    w = q8 * np.maximum(0, 256 - e * K)
    assert w.min() >= 0 and w.max() <= 65536
    F = B + (((P - B) * w[..., None] + 32768) >> 16)
    assert F.min() >= 0 and F.max() <= 65280                    # still a convex combination: no clamp
    return F, e


def sub_ref(src, cur, prev=None, levels=1, subpel=2, q8=256, K=16, R=7, matrix=0, bgr=False):
    """src [H,W,3], cur [Ho,Wo,3], prev (luma u8, out88 u16, [lumas of the levels 1 ..]) or None -> dict(luma=, mv=, mvf=, out88=, dst=,
    lumas= [levels 1 ..], vs= [levels 1 ..], e= the luma difference the blend saw)"""
    Ho, Wo = cur.shape[:2]
    cl = pyramid(luma8(src, Ho, Wo, matrix, bgr), levels)
    pl = None if prev is None else [prev[0]] + list(prev[2])
    vs = search_pyr(cl, pl, R)
    p8, p88 = (None, None) if prev is None else prev[:2]
    mvf = refine(cl[0], p8, vs[0], R, subpel)
    F, e = blend_sub(cur, cl[0], p8, p88, vs[0], mvf, q8, K, R * ((1 << levels) - 1))
    return dict(luma=cl[0], mv=vs[0], mvf=mvf, out88=F.astype(np.uint16), dst=F.astype(np.float32) * np.float32(0.00390625), lumas=cl[1:],
                vs=vs[1:], e=e)


def texture_pair(Ho, Wo, my, mx, seed, sigma=6.0, noise=0.0):
    """(prev8, cur8) uint8 [Ho,Wo]: a smooth random texture built at four times the size (uniform noise blurred separably with a Gaussian of
    `sigma`), box-sampled 4 x 4 at two offsets so that cur8[y][x] shows what prev8 shows at (y + my / 4, x + mx / 4); `noise`: the sigma of
    independent Gaussian noise added to either frame before rounding.  numpy alone."""
    rs = np.random.RandomState(seed)
    pad = 16                                                    # fine pixels on every side: |my|, |mx| <= 8 stay inside
    k = np.arange(-int(4 * sigma), int(4 * sigma) + 1)
    g = np.exp(-0.5 * (k / sigma) ** 2)
    g /= g.sum()
    T = rs.uniform(-1.0, 1.0, (4 * Ho + 2 * pad + g.size - 1, 4 * Wo + 2 * pad + g.size - 1))
    T = sum(w * T[i:i + 4 * Ho + 2 * pad] for i, w in enumerate(g))
    T = sum(w * T[:, i:i + 4 * Wo + 2 * pad] for i, w in enumerate(g))
    T = 128.0 + 48.0 * T / T.std()

    def frame(oy, ox):
        a = T[pad + oy:pad + oy + 4 * Ho, pad + ox:pad + ox + 4 * Wo].reshape(Ho, 4, Wo, 4).mean(axis=(1, 3))
        if noise:
            a = a + rs.normal(0.0, noise, a.shape)
        return np.clip(np.floor(a + 0.5), 0, 255).astype(np.uint8)

    return frame(0, 0), frame(my, mx)


MOTIONS = ((1, 0), (2, -2), (3, 5), (-6, 1))                    # quarter pixels
SEED = 1                                                        # of texture_pair in the known answers below


def interior_blocks(Ho, Wo):
    """The blocks that lie wholly inside the frame together with their copies displaced by up to two pixels either way"""
    return [b for b in interior(Ho, Wo, 2, 2) if b in interior(Ho, Wo, -2, -2)]


# ================================================================ running the device call
@pytest.fixture(params=backends.engine_params())
def eng(request):
    return backends.get_engine(request.param)


MVF_FILL = 0x55                                                 # what a sentinel-filled mvf holds before the call


def mvf_buffer(eng, Ho, Wo, off=0):
    return placed(eng, np.full(blocks_of(Ho, Wo) + (2,), MVF_FILL, np.uint8), off, GUARD, u8=True)


def read_mvf(eng, buf, Ho, Wo):
    whole = np.array(eng.mem.to_numpy(buf[0]), copy=True).reshape(-1)
    n = 2 * int(np.prod(blocks_of(Ho, Wo)))
    assert np.all(whole[:buf[2]] == FILL) and np.all(whole[buf[2] + n:] == FILL), "a write outside mvf"
    return whole[buf[2]:buf[2] + n].view(np.int8).reshape(blocks_of(Ho, Wo) + (2,))


def run(eng, src, cur, prev=None, levels=1, subpel=2, alias=False, off=(0, 0, 0), soff=0, poff=None, foff=None, **kw):
    """eng.temporal_f32(levels=, subpel=) on host arrays -> dict as sub_ref's (without e); off: floats past a 16-byte boundary of src, cur,
    dst; soff: bytes of the state buffers, poff: of the pyramid buffers, foff: of mvf (both soff).  Every output lies between guards, which
    must come back untouched, and the previous state is read only (its mvf too)."""
    poff, foff = soff if poff is None else poff, soff if foff is None else foff
    mem = eng.mem
    Ho, Wo = cur.shape[:2]
    _, s, _ = placed(eng, src, off[0], 0)
    cbuf, c, c0 = placed(eng, cur, off[1], GUARD)
    dbuf, d, d0 = (cbuf, c, c0) if alias else placed(eng, np.full(cur.shape, SENTINEL, np.float32), off[2], GUARD)
    state, spyr = slot_buffers(eng, Ho, Wo, off=soff), pyr_buffer(eng, Ho, Wo, levels, off=poff) if levels > 1 else None
    smvf = mvf_buffer(eng, Ho, Wo, foff)
    before = bpyr = bmvf = pslot = None
    if prev is not None:
        before = slot_buffers(eng, Ho, Wo, fill=prev[:2], off=soff)
        bpyr = pyr_buffer(eng, Ho, Wo, levels, prev[2], off=poff) if levels > 1 else None
        bmvf = mvf_buffer(eng, Ho, Wo, foff)
        pslot = tuple(b[1] for b in before) + ((bpyr[1],) if levels > 1 else ()) + (bmvf[1],)
    eng.temporal_f32(s, c, d, tuple(b[1] for b in state) + ((spyr[1],) if levels > 1 else ()) + (smvf[1],), prev=pslot, levels=levels,
                     subpel=subpel, **kw)
    whole = np.array(mem.to_numpy(dbuf), copy=True).reshape(-1)
    assert np.all(whole[:d0] == SENTINEL) and np.all(whole[d0 + cur.size:] == SENTINEL), "a write outside the destination"
    luma, out88, mv = read_slot(eng, state, Ho, Wo)
    lumas, vs = read_pyr(eng, spyr, Ho, Wo, levels) if levels > 1 else ([], [])
    if prev is not None:
        pl, po, _ = read_slot(eng, before, Ho, Wo)
        assert np.array_equal(pl, prev[0]) and np.array_equal(po, prev[1])
        assert levels == 1 or all(np.array_equal(a, b) for a, b in zip(read_pyr(eng, bpyr, Ho, Wo, levels)[0], prev[2]))
        assert np.all(read_mvf(eng, bmvf, Ho, Wo).view(np.uint8) == MVF_FILL)
    return dict(luma=luma, mv=mv, mvf=read_mvf(eng, smvf, Ho, Wo), out88=out88, dst=whole[d0:d0 + cur.size].reshape(cur.shape), lumas=lumas, vs=vs)


def equal(got, want, mvf=True):
    return all(np.array_equal(got[k], want[k]) for k in ("luma", "mv", "out88")) and same(got["dst"], want["dst"]) and \
        (not mvf or (np.array_equal(got["mvf"], want["mvf"]) and got["mvf"].dtype == np.int8)) and \
        got["mv"].dtype == np.int8 and got["out88"].dtype.kind == "u" and len(got["lumas"]) == len(want["lumas"]) and \
        all(np.array_equal(a, b) for a, b in zip(got["lumas"], want["lumas"])) and all(np.array_equal(a, b) for a, b in zip(got["vs"], want["vs"]))


def state_of(res):
    return (res["luma"], res["out88"], res["lumas"])


SHAPES = [(1, 1, 1, 1), (16, 16, 16, 16), (14, 30, 17, 33), (33, 47, 33, 47), (48, 64, 48, 64), (96, 128, 96, 128)]   # H, W, Ho, Wo
_slow = {}


def slow_case(shape):
    """tests.test_temporal.case with sources that move slowly: (src0, cur0, src1, cur1), each [3, ...], built once and read-only.  The noise
    and the checkerboard of `case` move by whole pixels and leave nearly every fraction at zero, so the sources of kinds 0 and 2 are smooth
    colour textures here, the second frame moved by (6, -9) and by (-3, 2) quarter pixels under a little noise; kind 1 keeps the source with
    NaN, infinities and values off the scale.  cur0 and cur1 are `case`'s, every kind."""
    if shape not in _slow:
        H, W = shape[:2]
        src0, cur0, src1, cur1 = case(shape)
        src0, src1 = np.array(src0, copy=True), np.array(src1, copy=True)
        rs = np.random.RandomState(H * 77 + W)
        for kind, (my, mx) in ((0, (6, -9)), (2, (-3, 2))):
            pairs = [texture_pair(H, W, my, mx, 40 + 3 * kind + c, sigma=4.0) for c in range(3)]
            src0[kind] = np.stack([p for p, _ in pairs], axis=-1).astype(np.float32)
            src1[kind] = np.stack([c for _, c in pairs], axis=-1).astype(np.float32) + rs.randint(-1, 2, (H, W, 3)).astype(np.float32)
        for a in (src0, src1):
            a.setflags(write=False)
        _slow[shape] = (src0, cur0, src1, cur1)
    return _slow[shape]


# ================================================================ the restatement itself (CPU)
def test_restatement_fit_and_fetch():
    assert fit(10, 10, 10, 2) == 0 and fit(10, 9, 10, 2) == 0 and fit(10, 4, 6, 2) == 0        # flat; E = 0; both neighbours below the winner
    assert fit(0, 8, 8, 2) == 0 and fit(0, 8, 8, 1) == 0                                        # symmetric
    # E = 8: g = floor((4 (m - p) + 8) / 16); the minimum lies towards the smaller neighbour
    assert [fit(0, 8, p, 2) for p in (8, 7, 6, 5, 4, 2, 0)] == [0, 0, 1, 1, 1, 2, 2]
    assert [fit(0, p, 8, 2) for p in (8, 7, 6, 5, 4, 2, 0)] == [0, 0, 0, -1, -1, -1, -2]       # a true floor: (-12 + 8) // 16 = -1
    assert [fit(0, 8, p, 1) for p in (8, 5, 4, 0)] == [0, 0, 2, 2] and [fit(0, p, 8, 1) for p in (5, 4, 3, 0)] == [0, 0, -2, -2]
    assert fit(5, 100, 1, 2) == 2 and fit(5, 1, 100, 2) == -2                                   # a neighbour below the winner: held to the half pixel
    # the fetch: no fraction returns the first argument; a half-pixel fraction is the rounded mean; negative positions floor
    p8 = np.array([[0, 100], [200, 255]], np.uint8)
    p88 = np.repeat((p8.astype(np.uint16) * 256)[..., None], 3, axis=-1)
    mv0 = np.zeros((1, 1, 2), np.int8)
    at = lambda fy, fx: fetch(p8, p88, mv0, np.array([[[fy, fx]]], np.int8), 7)
    assert at(0, 0)[0].tolist() == p8.tolist() and at(0, 0)[1][..., 0].tolist() == (p8.astype(int) * 256).tolist()
    assert at(0, 2)[0].tolist() == [[50, 100], [228, 255]]                                      # (2 x 200 + 2 x 255) x 4 + 8 >> 4 = 228, the right edge clamps
    assert at(2, 2)[0][0, 0] == (2 * (2 * 0 + 2 * 100) + 2 * (2 * 200 + 2 * 255) + 8) >> 4
    assert at(-1, 0)[0].tolist() == [[0, 100], [150, 216]]                                      # Y4 = -1: y0 = -1, ay = 3, r0 clamps to 0; row 1: (1 x 0 + 3 x 200) x 4 + 8 >> 4
    assert at(0, 1)[1][0, 0].tolist() == [(4 * (3 * 0 + 1 * 25600) + 8) >> 4] * 3


def test_restatement_without_fractions_is_the_whole_pixel_blend():
    for shape in ((33, 47, 33, 47), (14, 30, 17, 33)):
        src0, cur0, src1, cur1 = case(shape)
        Ho, Wo = shape[2:]
        p8, c8 = luma8(src0[0], Ho, Wo), luma8(src1[0], Ho, Wo)
        p88 = to88(cur0[0]).astype(np.uint16)
        mv = search_pyr([c8], [p8], 7)[0]
        F, _ = blend_sub(cur1[0], c8, p8, p88, mv, np.zeros_like(mv), 77, 16, 7)
        assert np.array_equal(F, blend(cur1[0], c8, p8, p88, mv, 77, 16))
        for levels in (1, 2):
            prev = (p8, p88, pyramid(p8, levels)[1:])
            want, got = pyr_ref(src1[0], cur1[0], prev=prev, levels=levels, q8=77), sub_ref(src1[0], cur1[0], prev=prev, levels=levels, subpel=0, q8=77)
            assert not got["mvf"].any() and all(np.array_equal(got[k], want[k]) for k in ("luma", "mv", "out88", "dst"))


@pytest.mark.parametrize("motion", MOTIONS, ids=lambda m: "%d_%d" % m)
def test_restatement_known_motions(motion):
    """A smooth texture moved by a known fraction: with quarter-pixel vectors every interior block lands within one quarter unit of the
    motion in both components, with half-pixel vectors within two; with and without independent noise of sigma 2 on both frames."""
    inside = interior_blocks(96, 128)
    assert len(inside) == 24
    for noise in (0.0, 2.0):
        p8, c8 = texture_pair(96, 128, motion[0], motion[1], SEED, noise=noise)
        mv = search_pyr([c8], [p8], 3)[0]
        for S, within in ((2, 1), (1, 2)):
            q = 4 * mv.astype(np.int64) + refine(c8, p8, mv, 3, S)
            assert all(np.abs(q[b] - motion).max() <= within for b in inside), (motion, noise, S)


def test_restatement_stays_whole_where_nothing_moved_by_a_fraction():
    inside = interior_blocks(96, 128)
    p8, c8 = texture_pair(96, 128, 0, 0, SEED, noise=2.0)       # a still scene under noise
    assert not np.array_equal(p8, c8)
    mv = search_pyr([c8], [p8], 3)[0]
    for S in (1, 2):
        assert not mv.any() and not any(refine(c8, p8, mv, 3, S)[b].any() for b in inside)
    for (Ho, Wo), (dy, dx), levels in (((96, 128), (28, -28), 3), ((48, 64), (12, 0), 2)):      # whole-pixel moves of uniform noise
        a, moved = moved_pair(Ho, Wo, dy, dx, 1)
        mv = search_pyr(pyramid(moved, levels), pyramid(a, levels), 7)[0]
        assert not any(refine(moved, a, mv, 7, 2)[b].any() for b in interior(Ho, Wo, dy, dx))
    flat = np.full((33, 47), 90, np.uint8)                      # a flat frame: E = 0 everywhere
    assert not refine(flat, flat, np.zeros((3, 3, 2), np.int8), 7, 2).any()
    one = np.array([[7]], np.uint8)                             # 1 x 1: everything clamps, the three sums of an axis are equal
    assert not refine(one, np.array([[200]], np.uint8), np.zeros((1, 1, 2), np.int8), 7, 2).any()


def test_restatement_quarter_pixel_fetch_lowers_the_luma_difference():
    p8, c8 = texture_pair(96, 128, 2, -2, SEED)
    zero = np.zeros((96, 128, 3), np.uint16)
    e = [sub_ref(grey(c8), grey(c8), prev=(p8, zero, []), subpel=S, R=3)["e"][16:80, 16:112].mean() for S in (0, 2)]
    assert e[1] < e[0]


# ================================================================ the device against the restatement
@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_two_frames_match_the_restatement(eng, shape, levels):
    """Both matrices, both channel orders and every radius, the nine pairs of sensitivity and strength going round, half and quarter pixels
    alternating; every data kind (noise; NaN, infinities and values off the scale; a checkerboard); a first frame (no previous state) and a
    second one fed with the first one's state.  The sources move slowly (slow_case), so that the fractions are there."""
    src0, cur0, src1, cur1 = slow_case(shape)
    fractions = 0
    for i, kw in enumerate(COMBOS):
        kind, S = i % 3, 1 + (i + i // 3 + levels) % 2
        first = run(eng, src0[kind], cur0[kind], levels=levels, subpel=S, **device_kw(**kw))
        assert equal(first, sub_ref(src0[kind], cur0[kind], levels=levels, subpel=S, **kw)), ("first", kw, S)
        assert not first["mv"].any() and not first["mvf"].any() and np.array_equal(first["out88"], to88(cur0[kind]))
        second = run(eng, src1[kind], cur1[kind], prev=state_of(first), levels=levels, subpel=S, **device_kw(**kw))
        want = sub_ref(src1[kind], cur1[kind], prev=state_of(first), levels=levels, subpel=S, **kw)
        assert equal(second, want), ("second", kw, S)
        if kw["R"] == 0:
            assert not second["mv"].any() and not second["mvf"].any()
        if kw["q8"] == 0:
            assert np.array_equal(second["out88"], to88(cur1[kind]))
        fractions += int(np.count_nonzero(want["mvf"]))
    assert (fractions == 0) == (shape[:2] == (1, 1))            # (the cases do exercise the bilinear fetch; at 1 x 1 every sum of an axis is equal)


def run_lumas(eng, cur8, prev8, levels=1, subpel=2, prev88=None, cur=None, **kw):
    """A grey frame of luma cur8 against the state of a grey frame of luma prev8"""
    Ho, Wo = cur8.shape
    prev = (prev8, ZERO88(Ho, Wo) if prev88 is None else prev88, pyramid(prev8, levels)[1:])
    got = run(eng, grey(cur8), grey(cur8) if cur is None else cur, prev=prev, levels=levels, subpel=subpel, **device_kw(**kw))
    assert np.array_equal(got["luma"], cur8)
    return got, prev


def test_known_motions_on_the_device(eng):
    inside = interior_blocks(96, 128)
    e = {}
    for motion, noise in itertools.product(MOTIONS, (0.0, 2.0)):
        p8, c8 = texture_pair(96, 128, motion[0], motion[1], SEED, noise=noise)
        for S, within in ((2, 1), (1, 2)):
            want = sub_ref(grey(c8), grey(c8), prev=(p8, ZERO88(96, 128), []), subpel=S, R=3)
            got, _ = run_lumas(eng, c8, p8, subpel=S, R=3)
            for res in (want, got):
                q = 4 * res["mv"].astype(np.int64) + res["mvf"]
                assert all(np.abs(q[b] - motion).max() <= within for b in inside), (motion, noise, S)
            assert equal(got, want)
            if motion == (2, -2) and S == 2 and not noise:                    # the mean luma difference the blend sees, against whole-pixel vectors
                p88 = np.repeat((p8.astype(np.uint16) << 8)[..., None], 3, axis=-1)     # (prev88 = the grey previous frame: P - cur is the luma difference)
                for s in (0, 2):
                    ref = sub_ref(grey(c8), grey(c8), prev=(p8, p88, []), subpel=s, R=3, q8=256, K=1)
                    dev = run_lumas(eng, c8, p8, subpel=s, prev88=p88, R=3, q8=256, K=1)[0] if s else \
                        dict(run_one_level(eng, grey(c8), grey(c8), prev=(p8, p88), **device_kw(R=3, q8=256, K=1)), lumas=[], vs=[])
                    assert equal(dev, ref, mvf=bool(s))
                    e[s] = ref["e"][16:80, 16:112].mean()
    assert e[2] < e[0]


def test_a_still_scene_under_noise_and_whole_pixel_moves_stay_whole(eng):
    inside = interior_blocks(96, 128)
    p8, c8 = texture_pair(96, 128, 0, 0, SEED, noise=2.0)
    for S in (1, 2):
        got, _ = run_lumas(eng, c8, p8, subpel=S, R=3)
        assert not got["mv"].any() and not any(got["mvf"][b].any() for b in inside)
        assert equal(got, sub_ref(grey(c8), grey(c8), prev=(p8, ZERO88(96, 128), []), subpel=S, R=3))
    for (Ho, Wo), (dy, dx), levels in (((96, 128), (28, -28), 3), ((48, 64), (12, 0), 2)):
        a, moved = moved_pair(Ho, Wo, dy, dx, 1)
        got, prev = run_lumas(eng, moved, a, levels=levels)
        assert all(got["mv"][b].tolist() == [dy, dx] and not got["mvf"][b].any() for b in interior(Ho, Wo, dy, dx))
        assert equal(got, sub_ref(grey(moved), grey(moved), prev=prev, levels=levels))


@pytest.mark.parametrize("levels", [1, 3])
def test_no_fraction_anywhere_is_the_whole_pixel_path(eng, levels):
    """Where the restatement gives mvf == 0 everywhere -- a still picture, a flat frame, a first frame -- out88 and dst are those of the
    existing entry points; strength 256 on a still picture returns the first frame.  (48 x 64 has whole blocks only: a ragged block of one
    row has SAD(dy + 1) = SAD(dy) by the clamp and is given a fraction by the fit, see the next test.)"""
    Ho, Wo = 48, 64
    src0, cur0, src1, cur1 = case((Ho, Wo, Ho, Wo))
    still = luma8(src0[0], Ho, Wo)
    p88 = to88(cur0[0]).astype(np.uint16)
    for c8, cur, q8 in ((still, cur1[0], 77), (still, cur1[1], 256), (np.full((Ho, Wo), 90, np.uint8), cur1[0], 128)):
        prev = (c8, p88, pyramid(c8, levels)[1:])
        want = sub_ref(grey(c8), cur, prev=prev, levels=levels, q8=q8)
        assert not want["mvf"].any() and not want["mv"].any()
        got = run(eng, grey(c8), cur, prev=prev, levels=levels, **device_kw(q8=q8))
        parent = run_pyr(eng, grey(c8), cur, prev=prev, levels=levels, **device_kw(q8=q8))
        assert equal(got, want) and np.array_equal(got["out88"], parent["out88"]) and same(got["dst"], parent["dst"])
        if q8 == 256:
            assert np.array_equal(got["out88"], p88)


def test_a_one_row_block_of_a_still_picture_takes_a_fraction_and_fetches_the_same_row(eng):
    """33 x 47 against itself: the blocks of the last block row hold row 32 alone, where SAD(1, 0) clamps to SAD(0, 0) = 0 < SAD(-1, 0), so
    the fit as stated gives (2, 0) there; r0 = r1 = 32 under that fraction, so the result is the whole-pixel path's all the same.  A flat
    frame of the same size has E = 0 in every block."""
    Ho, Wo = 33, 47
    src0, cur0, src1, cur1 = case((Ho, Wo, Ho, Wo))
    still = luma8(src0[0], Ho, Wo)
    prev = (still, to88(cur0[0]).astype(np.uint16), [])
    want = sub_ref(grey(still), cur1[0], prev=prev, q8=256)
    assert not want["mv"].any() and want["mvf"][2].tolist() == [[2, 0]] * 3 and not want["mvf"][:2].any()
    got = run(eng, grey(still), cur1[0], prev=prev, **device_kw(q8=256))
    parent = run_one_level(eng, grey(still), cur1[0], prev=prev[:2], **device_kw(q8=256))
    assert equal(got, want) and np.array_equal(got["out88"], parent["out88"]) and np.array_equal(got["out88"], prev[1])
    flat = np.full((Ho, Wo), 90, np.uint8)
    got = run(eng, grey(flat), cur1[0], prev=(flat, prev[1], []), **device_kw(q8=128))
    assert not got["mvf"].any() and equal(got, sub_ref(grey(flat), cur1[0], prev=(flat, prev[1], []), q8=128))


@pytest.mark.parametrize("shape", [(14, 30, 17, 33), (48, 64, 48, 64)], ids=ids)
def test_subpel_zero_is_the_existing_stage(eng, shape):
    """subpel = 0 through the new entry point: fs_temporal_pyr_f32 (and fs_temporal_f32 at one level) in every output, and a sentinel-filled
    mvf comes back untouched (a null one is taken too)."""
    src0, cur0, src1, cur1 = case(shape)
    Ho, Wo = shape[2:]
    for levels, kw in ((1, COMBOS[2]), (2, COMBOS[7]), (3, COMBOS[10])):
        c8 = luma8(src0[0], Ho, Wo, kw["matrix"], kw["bgr"])
        prev = (c8, to88(cur0[0]).astype(np.uint16), pyramid(c8, levels)[1:])
        for pv in (None, prev):
            got = lib_call(eng, src1[0], cur1[0], pv, levels, 0, **kw)
            assert np.all(got.pop("mvf").view(np.uint8) == MVF_FILL)
            assert equal(dict(got, mvf=None), pyr_ref(src1[0], cur1[0], prev=pv, levels=levels, **kw), mvf=False), (levels, kw)
            parent = run_pyr(eng, src1[0], cur1[0], prev=pv, levels=levels, **device_kw(**kw))
            assert equal(dict(got, mvf=None), parent, mvf=False)
            if levels == 1:
                one = run_one_level(eng, src1[0], cur1[0], prev=None if pv is None else pv[:2], **device_kw(**kw))
                assert equal(dict(got, mvf=None), dict(one, lumas=[], vs=[]), mvf=False)
            null = lib_call(eng, src1[0], cur1[0], pv, levels, 0, null_mvf=True, **kw)
            assert equal(dict(null, mvf=None), parent, mvf=False)


def lib_call(eng, src, cur, prev, levels, subpel, q8=256, K=16, R=7, matrix=0, bgr=False, null_mvf=False):
    """fs_temporal_sub_f32 itself on guarded buffers -> dict as run's"""
    mem = eng.mem
    Ho, Wo = cur.shape[:2]
    _, s, _ = placed(eng, src, 0, 0)
    _, c, _ = placed(eng, cur, 0, 0)
    dbuf, d, d0 = placed(eng, np.full(cur.shape, SENTINEL, np.float32), 0, GUARD)
    state, spyr, smvf = slot_buffers(eng, Ho, Wo), pyr_buffer(eng, Ho, Wo, levels) if levels > 1 else None, mvf_buffer(eng, Ho, Wo)
    before = slot_buffers(eng, Ho, Wo, fill=prev[:2]) if prev is not None else None
    bpyr = pyr_buffer(eng, Ho, Wo, levels, prev[2]) if prev is not None and levels > 1 else None
    eng._sync_stream()
    p8 = mem.ptr_u8
    rc = eng.lib.fs_temporal_sub_f32(eng.ctx, mem.ptr(s), src.shape[0], src.shape[1], mem.ptr(c), Ho, Wo, q8, K, R, levels, subpel, matrix, int(bgr),
                                     None if before is None else p8(before[0][1]), None if before is None else p8(before[1][1]),
                                     None if bpyr is None else p8(bpyr[1]), p8(state[0][1]), p8(state[1][1]), None if spyr is None else p8(spyr[1]),
                                     p8(state[2][1]), None if null_mvf else p8(smvf[1]), mem.ptr(d))
    assert rc == 0, eng.lib.fs_last_error()
    whole = np.array(mem.to_numpy(dbuf), copy=True).reshape(-1)
    assert np.all(whole[:d0] == SENTINEL) and np.all(whole[d0 + cur.size:] == SENTINEL)
    luma, out88, mv = read_slot(eng, state, Ho, Wo)
    lumas, vs = read_pyr(eng, spyr, Ho, Wo, levels) if levels > 1 else ([], [])
    return dict(luma=luma, mv=mv, mvf=read_mvf(eng, smvf, Ho, Wo), out88=out88, dst=whole[d0:d0 + cur.size].reshape(cur.shape), lumas=lumas, vs=vs)


@pytest.mark.parametrize("shift", [(-9, -9), (9, 9), (-9, 9), (9, -9)], ids=lambda s: "dy%d_dx%d" % s)
def test_vectors_that_point_out_of_the_frame_clamp_with_their_fractions(eng, shift):
    """A hand-written previous state: cur8[y][x] = prev8[clampy(y + dy)][clampx(x + dx)] by construction at two levels, so that the vectors of
    the blocks on two edges point out of the frame; the previous luma is smooth, so the refinement yields fractions there, and r0, r1, c0,
    c1 clamp under them.  40 x 52 has ragged blocks on the right and at the bottom."""
    Ho, Wo = 40, 52
    dy, dx = shift
    p8, o8 = texture_pair(Ho, Wo, 0, 0, 1, sigma=3.0)[0], texture_pair(Ho, Wo, 0, 0, 101, sigma=3.0)[0]      # (o8: another picture, a quarter of cur8)
    c8 = ((p8[np.clip(np.arange(Ho) + dy, 0, Ho - 1)][:, np.clip(np.arange(Wo) + dx, 0, Wo - 1)].astype(np.int64) * 3 + o8) >> 2).astype(np.uint8)
    p88 = np.random.RandomState(6).randint(0, 65281, (Ho, Wo, 3)).astype(np.uint16)
    cur = case((Ho, Wo, Ho, Wo))[3][0]
    prev = (p8, p88, pyramid(p8, 2)[1:])
    want = sub_ref(grey(c8), cur, prev=prev, levels=2, q8=200, K=4)
    y, x = np.indices((Ho, Wo))
    Y4 = 4 * (y + want["mv"].astype(np.int64)[y >> 4, x >> 4, 0]) + want["mvf"].astype(np.int64)[y >> 4, x >> 4, 0]
    X4 = 4 * (x + want["mv"].astype(np.int64)[y >> 4, x >> 4, 1]) + want["mvf"].astype(np.int64)[y >> 4, x >> 4, 1]
    out_y, out_x = ((Y4 >> 2) < 0) | ((Y4 >> 2) + 1 > Ho - 1), ((X4 >> 2) < 0) | ((X4 >> 2) + 1 > Wo - 1)
    assert (out_y & ((Y4 & 3) != 0)).any() and (out_x & ((X4 & 3) != 0)).any()                  # clamped rows and columns under a fraction
    got = run(eng, grey(c8), cur, prev=prev, levels=2, **device_kw(q8=200, K=4))
    assert equal(got, want)


@pytest.mark.parametrize("levels", [1, 2])
def test_the_destination_may_be_the_current_tensor(eng, levels):
    for shape in ((14, 30, 17, 33), (33, 47, 33, 47)):
        src0, cur0, src1, cur1 = slow_case(shape)
        Ho, Wo = shape[2:]
        for kw, S in ((dict(q8=77, K=1), 2), (dict(q8=256, K=16, R=3, matrix=1, bgr=True), 1)):
            c8 = luma8(src0[0], Ho, Wo, kw.get("matrix", 0), kw.get("bgr", False))
            prev = (c8, to88(cur0[0]).astype(np.uint16), pyramid(c8, levels)[1:])
            got = run(eng, src1[0], cur1[0], prev=prev, levels=levels, subpel=S, alias=True, **device_kw(**kw))
            assert equal(got, sub_ref(src1[0], cur1[0], prev=prev, levels=levels, subpel=S, **kw)), kw


def test_tensors_and_state_off_sixteen_byte_alignment_give_the_same_values(eng):
    shape = (33, 47, 33, 47)
    src0, cur0, src1, cur1 = slow_case(shape)
    c8 = luma8(src0[0], 33, 47)
    prev = (c8, to88(cur0[0]).astype(np.uint16), pyramid(c8, 3)[1:])
    want = sub_ref(src1[0], cur1[0], prev=prev, levels=3, q8=128, K=4)
    assert want["mvf"].any()
    for off, soff, poff, foff in (((1, 0, 0), 0, 0, 1), ((0, 1, 0), 0, 1, 0), ((0, 0, 1), 0, 7, 3), ((0, 0, 0), 2, 2, 2), ((3, 2, 1), 6, 13, 9)):
        got = run(eng, src1[0], cur1[0], prev=prev, levels=3, off=off, soff=soff, poff=poff, foff=foff, **device_kw(q8=128, K=4))
        assert equal(got, want), (off, soff, poff, foff)


def test_engine_slots(eng):
    """Engine.temporal_state / temporal_f32 with subpel on the engine's own buffers, two frames; mvf is the last buffer of a slot"""
    shape = (33, 47, 33, 47)
    src0, cur0, src1, cur1 = slow_case(shape)
    mem = eng.mem
    for levels, S in ((1, 2), (2, 1), (3, 2)):
        slots = [eng.temporal_state(33, 47, levels, S) for _ in range(2)]
        assert len(slots[0]) == (4 if levels == 1 else 5) and tuple(slots[0][-1].shape) == (3, 3, 2)
        d = mem.empty((33, 47, 3))
        eng.temporal_f32(mem.from_numpy(src0[0]), mem.from_numpy(cur0[0]), d, slots[0], levels=levels, subpel=S)
        first = sub_ref(src0[0], cur0[0], levels=levels, subpel=S)
        eng.temporal_f32(mem.from_numpy(src1[0]), mem.from_numpy(cur1[0]), d, slots[1], prev=slots[0], levels=levels, subpel=S)
        second = sub_ref(src1[0], cur1[0], prev=state_of(first), levels=levels, subpel=S)
        assert same(np.asarray(mem.to_numpy(d)), second["dst"])
        mvf = np.array(mem.to_numpy(slots[1][-1]), dtype=np.uint8, copy=True).view(np.int8)
        assert np.array_equal(mvf, second["mvf"]) and np.array_equal(np.asarray(mem.to_numpy(slots[1][2])).view(np.int8), second["mv"])
    assert len(eng.temporal_state(33, 47)) == 3 and len(eng.temporal_state(33, 47, 2)) == 4 and len(eng.temporal_state(33, 47, 2, 0)) == 4
    for bad in (dict(subpel=3), dict(subpel=-1), dict(subpel=1.5), dict(levels=4, subpel=1)):
        with pytest.raises(L.FaststyleError):
            eng.temporal_state(33, 47, **bad)


def test_refused_calls_return_their_code_and_launch_nothing(eng):
    mem, lib, ctx = eng.mem, eng.lib, eng.ctx
    H, W, Ho, Wo, levels = 14, 30, 17, 33, 3
    src0, cur0, src1, cur1 = case((H, W, Ho, Wo))
    _, s, _ = placed(eng, src1[0], 0, 0)
    _, c, _ = placed(eng, cur1[0], 0, 0)
    dbuf, d, d0 = placed(eng, np.full(cur1[0].shape, SENTINEL, np.float32), 0, GUARD)
    state, spyr, smvf = slot_buffers(eng, Ho, Wo), pyr_buffer(eng, Ho, Wo, levels), mvf_buffer(eng, Ho, Wo)
    c8 = luma8(src0[0], Ho, Wo)
    prevh = (c8, to88(cur0[0]).astype(np.uint16), pyramid(c8, levels)[1:])
    before, bpyr = slot_buffers(eng, Ho, Wo, fill=prevh[:2]), pyr_buffer(eng, Ho, Wo, levels, prevh[2])
    for _, view, _ in state + [spyr, smvf]:                     # (so that a launch of any of the kernels would show)
        if hasattr(view, "fill_"):
            view.fill_(FILL)
        else:
            view[...] = FILL
    ps, pc, pd = mem.ptr(s), mem.ptr(c), mem.ptr(d)
    pl, po, pm = (mem.ptr_u8(b[1]) for b in state)
    pp, qp, pf = mem.ptr_u8(spyr[1]), mem.ptr_u8(bpyr[1]), mem.ptr_u8(smvf[1])
    ql, qo = mem.ptr_u8(before[0][1]), mem.ptr_u8(before[1][1])
    eng._sync_stream()

    def call(src=ps, H=H, W=W, cur=pc, Ho=Ho, Wo=Wo, q8=128, K=16, R=7, levels=levels, subpel=2, matrix=0, bgr=0, prev_luma=ql, prev_out88=qo,
             prev_pyr=qp, luma=pl, out88=po, pyr=pp, mv=pm, mvf=pf, dst=pd):
        return lib.fs_temporal_sub_f32(ctx, src, H, W, cur, Ho, Wo, q8, K, R, levels, subpel, matrix, bgr, prev_luma, prev_out88, prev_pyr, luma,
                                       out88, pyr, mv, mvf, dst)

    refused = [(-1, dict(src=None)), (-1, dict(cur=None)), (-1, dict(luma=None)), (-1, dict(out88=None)), (-1, dict(mv=None)), (-1, dict(dst=None)),
               (-1, dict(prev_luma=None)), (-1, dict(prev_out88=None)), (-1, dict(prev_luma=pl)), (-1, dict(prev_out88=po)),
               (-1, dict(H=0)), (-1, dict(W=0)), (-1, dict(H=-3)), (-1, dict(Ho=H - 1)), (-1, dict(Ho=H + 4)), (-1, dict(Wo=W - 1)),
               (-1, dict(Wo=W + 4)), (-1, dict(H=2 ** 31 - 1)),
               (-2, dict(q8=-1)), (-2, dict(q8=257)), (-2, dict(K=0)), (-2, dict(K=257)), (-2, dict(R=-1)), (-2, dict(R=8)), (-2, dict(matrix=2)),
               (-2, dict(matrix=-1)), (-2, dict(bgr=2)), (-2, dict(bgr=-1)),
               (-5, dict(src=ps + 2)), (-5, dict(cur=pc + 1)), (-5, dict(dst=pd + 3)), (-5, dict(out88=po + 1)), (-5, dict(prev_out88=qo + 1)),
               (-2, dict(levels=0)), (-2, dict(levels=4)), (-2, dict(levels=-1)),
               (-1, dict(pyr=None)), (-1, dict(pyr=None, levels=2)), (-1, dict(prev_pyr=None)),
               (-1, dict(prev_luma=None, prev_out88=None)), (-1, dict(prev_pyr=pp)), (-1, dict(pyr=qp)),
               (-2, dict(subpel=-1)), (-2, dict(subpel=3)), (-2, dict(subpel=3, mvf=None)), (-1, dict(mvf=None)), (-1, dict(mvf=None, subpel=1)),
               (-2, dict(subpel=0, levels=4)), (-1, dict(subpel=0, pyr=None))]
    for code, kw in refused:
        assert call(**kw) == code, kw
        assert b"fs_temporal_sub_f32" in lib.fs_last_error()
    assert lib.fs_temporal_sub_f32(None, ps, H, W, pc, Ho, Wo, 128, 16, 7, levels, 2, 0, 0, ql, qo, qp, pl, po, pp, pm, pf, pd) == -1
    assert np.all(np.asarray(mem.to_numpy(dbuf)) == SENTINEL)                                 # nothing was launched
    assert all(np.all(np.asarray(mem.to_numpy(b[0])) == FILL) for b in state + [spyr, smvf])
    # the call they were variations of is taken, with and without a previous frame
    assert call() == 0
    got = np.asarray(mem.to_numpy(dbuf)).reshape(-1)[d0:d0 + cur1[0].size].reshape(cur1[0].shape)
    want = sub_ref(src1[0], cur1[0], prev=prevh, levels=levels, q8=128)
    luma, out88, mv = read_slot(eng, state, Ho, Wo)
    lumas, vs = read_pyr(eng, spyr, Ho, Wo, levels)
    assert equal(dict(luma=luma, mv=mv, mvf=read_mvf(eng, smvf, Ho, Wo), out88=out88, dst=got, lumas=lumas, vs=vs), want)
    assert call(prev_luma=None, prev_out88=None, prev_pyr=None) == 0
    assert np.array_equal(read_slot(eng, state, Ho, Wo)[1], to88(cur1[0])) and not read_mvf(eng, smvf, Ho, Wo).any()
    # the engine checks the slot's length and shapes for (levels, subpel)
    views = tuple(b[1] for b in state) + (spyr[1], smvf[1])
    for bad in (dict(cur=s), dict(state=eng.temporal_state(Ho, Wo - 1, levels, 2)), dict(prev=eng.temporal_state(Ho, Wo - 1, levels, 2)),
                dict(state=views[:4]), dict(state=views[:3] + views[4:]), dict(state=eng.temporal_state(Ho, Wo, 2, 2)),
                dict(prev=eng.temporal_state(Ho, Wo, levels)), dict(levels=0), dict(levels=4), dict(subpel=3), dict(subpel=-1), dict(subpel=1.5)):
        a = dict(dict(src=s, cur=c, dst=d, state=views, prev=None, levels=levels, subpel=2), **bad)
        with pytest.raises(L.FaststyleError):
            eng.temporal_f32(a["src"], a["cur"], a["dst"], a["state"], prev=a["prev"], levels=a["levels"], subpel=a["subpel"])
    with pytest.raises(L.FaststyleError):
        eng.temporal_f32(s, c, d, views, radius=8, levels=levels, subpel=2)
