"""Overlapped block vectors of the temporal stage (csrc/fs_temporal.hip: fs_temporal_obmc_f32) against its contract in
include/faststyle_io.h.  The first part of this file is an independent numpy restatement of that text (int64, >> and floor division), built on
the luma, the pyramid, the searches, the refinement and the whole-block blends of tests/test_temporal.py, tests/test_temporal_pyr.py and
tests/test_temporal_sub.py; every comparison of the device with the restatement -- luma, mv, mvf, the 8.8 state and the float result -- is
equality.  The same bodies run on the CPU emulator and, under -m gpu, on the MI355X.  tests/test_temporal_obmc_stream.py builds its expected
tensors with the restatement."""
import numpy as np
import pytest

from faststyle_amd import _lib as L
from tests import backends
from tests.test_compose import GUARD, SENTINEL, placed, same, to88
from tests.test_temporal import FILL, blend, blocks_of, case, device_kw, grey, luma8, read_slot, slot_buffers
from tests.test_temporal import run as run_one_level
from tests.test_temporal_pyr import COMBOS, ids, moved_pair, pyr_buffer, pyramid, read_pyr, search_pyr
from tests.test_temporal_pyr import run as run_pyr
from tests.test_temporal_sub import MVF_FILL, blend_sub, fetch, mvf_buffer, read_mvf, refine, texture_pair
from tests.test_temporal_sub import run as run_sub


# ================================================================ the restatement
def window(n, nb):
    """One axis of n pixels and nb blocks -> (block int64 [n,2], weight int64 [n,2]): the two candidate blocks of every pixel and their
    window weights, which sum to 32"""
    t = 2 * np.arange(n, dtype=np.int64) - 15
    j0, a = t >> 5, t & 31
    return np.stack([np.clip(j0, 0, nb - 1), np.clip(j0 + 1, 0, nb - 1)], axis=-1), np.stack([32 - a, a], axis=-1)


def fetch_q(prev8, prev88, Q):
    """Q int64 [Ho,Wo,2], a held vector in quarter pixels per pixel -> (pq int64 [Ho,Wo], P int64 [Ho,Wo,3]): the previous luma and output at
    4 p + Q quarter pixels, bilinear, every coordinate clamped"""
    Ho, Wo = prev8.shape
    y, x = np.indices((Ho, Wo))
    Y4, X4 = 4 * y + Q[..., 0], 4 * x + Q[..., 1]
    y0, ay, x0, ax = Y4 >> 2, Y4 & 3, X4 >> 2, X4 & 3
    r0, r1, c0, c1 = np.clip(y0, 0, Ho - 1), np.clip(y0 + 1, 0, Ho - 1), np.clip(x0, 0, Wo - 1), np.clip(x0 + 1, 0, Wo - 1)

    def bil(A, ay, ax):
        return ((4 - ay) * ((4 - ax) * A[r0, c0] + ax * A[r0, c1]) + ay * ((4 - ax) * A[r1, c0] + ax * A[r1, c1]) + 8) >> 4

    return bil(prev8.astype(np.int64), ay, ax), bil(prev88.astype(np.int64), ay[..., None], ax[..., None])


def blend_obmc(cur, cur8, prev8, prev88, mv, mvf, q8, K, bound):
    """-> (F int64 [Ho,Wo,3], info): info None without a previous frame, otherwise dict(cbar= [Ho,Wo], conf= [4,Ho,Wo] per candidate, blk=
    [4,Ho,Wo] the candidates' flat block indices, Q= [4,Ho,Wo,2] their held vectors in quarter pixels, D=)"""
    B = to88(cur)
    if prev8 is None:
        return B, None
    Ho, Wo = cur8.shape
    nby, nbx = blocks_of(Ho, Wo)
    q = 4 * np.clip(mv.astype(np.int64), -bound, bound) + np.clip(mvf.astype(np.int64), -2, 2)
    (bys, wys), (bxs, wxs) = window(Ho, nby), window(Wo, nbx)
    D, N, cmax = np.zeros((Ho, Wo), np.int64), np.zeros((Ho, Wo, 3), np.int64), np.zeros((Ho, Wo), np.int64)
    confs, blks, Qs, wsum = [], [], [], 0
    for a in (0, 1):
        for b in (0, 1):
            w = wys[:, a][:, None] * wxs[:, b][None, :]
            by, bx = np.broadcast_arrays(bys[:, a][:, None], bxs[:, b][None, :])
            Q = q[by, bx]
            pq, P = fetch_q(prev8, prev88, Q)
            conf = np.maximum(0, 256 - np.abs(cur8.astype(np.int64) - pq) * K)
            D += w * conf
            N += (w * conf)[..., None] * P
            cmax = np.maximum(cmax, conf)
            wsum = wsum + w
            confs.append(conf), blks.append(by * nbx + bx), Qs.append(Q)
    assert np.all(wsum == 1024) and D.max() <= 1 << 18 and N.max() < 1 << 34
    Dn = np.maximum(D, 1)[..., None]
    Pbar = (2 * N + Dn) // (2 * Dn)
    assert Pbar.min() >= 0 and Pbar.max() <= 65280
    cbar = np.minimum(cmax, D >> 8)
    w = q8 * cbar
    assert w.min() >= 0 and w.max() <= 65536
    F = np.where((D == 0)[..., None], B, B + (((Pbar - B) * w[..., None] + 32768) >> 16))
    assert F.min() >= 0 and F.max() <= 65280                    # still no clamp
    return F, dict(cbar=cbar, conf=np.stack(confs), blk=np.stack(blks), Q=np.stack(Qs), D=D)


def obmc_ref(src, cur, prev=None, levels=1, subpel=0, q8=256, K=16, R=7, matrix=0, bgr=False):
    """src [H,W,3], cur [Ho,Wo,3], prev (luma u8, out88 u16, [lumas of the levels 1 ..]) or None -> dict(luma=, mv=, mvf=, out88=, dst=,
    lumas=, vs=, F= the int64 result, info= blend_obmc's, whole= the int64 result of the whole-block blend of the same vectors, conf= the
    confidence that blend gave every pixel (None on a first frame))"""
    Ho, Wo = cur.shape[:2]
    cl = pyramid(luma8(src, Ho, Wo, matrix, bgr), levels)
    pl = None if prev is None else [prev[0]] + list(prev[2])
    vs = search_pyr(cl, pl, R)
    p8, p88 = (None, None) if prev is None else prev[:2]
    mvf = refine(cl[0], p8, vs[0], R, subpel)
    bound = R * ((1 << levels) - 1)
    F, info = blend_obmc(cur, cl[0], p8, p88, vs[0], mvf, q8, K, bound)
    whole, e = blend_sub(cur, cl[0], p8, p88, vs[0], mvf, q8, K, bound)
    return dict(luma=cl[0], mv=vs[0], mvf=mvf, out88=F.astype(np.uint16), dst=F.astype(np.float32) * np.float32(0.00390625), lumas=cl[1:],
                vs=vs[1:], F=F, info=info, whole=whole, conf=None if e is None else np.maximum(0, 256 - e * K))


def own_candidate(Ho, Wo):
    """-> int64 [Ho,Wo]: which of the four candidates (2 row + column) is the pixel's own block (y >> 4, x >> 4) -- the one with the larger
    window weight along either axis"""
    oy, ox = (window(Ho, 1)[1][:, 1] > 16).astype(np.int64), (window(Wo, 1)[1][:, 1] > 16).astype(np.int64)
    return 2 * oy[:, None] + ox[None, :]


def masks(ref):
    """The pixel masks of the consequences, from the restatement's own vectors and confidences: (equal: the four held vectors agree, alone:
    every candidate of another block than the pixel's own has confidence 0, rest: the four vectors are (0, 0))"""
    info = ref["info"]
    Ho, Wo = ref["luma"].shape
    equal = np.all(info["Q"] == info["Q"][:1], axis=(0, 3))
    y, x = np.indices((Ho, Wo))
    own = (y >> 4) * blocks_of(Ho, Wo)[1] + (x >> 4)
    assert np.array_equal(np.take_along_axis(info["blk"], own_candidate(Ho, Wo)[None], axis=0)[0], own)
    alone = np.all((info["blk"] == own[None]) | (info["conf"] == 0), axis=0)
    return equal, alone, np.all(info["Q"] == 0, axis=(0, 3))


def two_region(H, W, seed, axis=1, va=(0, 3), vb=(0, -3)):
    """(prev8, cur8) uint8 [H,W]: uniform noise whose first region -- the columns (axis 1) or rows (axis 0) before the edge -- shows what the
    previous frame shows at p + va and whose second region what it shows at p + vb (wrapped round); the edge lies in the middle of the block
    that holds the frame's centre: 40 of 80, 40 of 64 columns, 24 of 48 rows"""
    a = np.random.RandomState(seed).randint(0, 256, (H, W)).astype(np.uint8)
    n = (H, W)[axis]
    edge = (n // 32) * 16 + 8
    first = np.arange(n) < edge
    first = first[None, :] if axis == 1 else first[:, None]
    return a, np.where(first, np.roll(a, (-va[0], -va[1]), axis=(0, 1)), np.roll(a, (-vb[0], -vb[1]), axis=(0, 1)))


def two_textures(H, W, seed, axis=1, va=(3, -2), vb=(-5, 6)):
    """two_region on a smooth texture, the regions moved by different fractions (quarter pixels)"""
    p, ca = texture_pair(H, W, va[0], va[1], seed, sigma=4.0)
    p2, cb = texture_pair(H, W, vb[0], vb[1], seed, sigma=4.0)
    assert np.array_equal(p, p2)
    n = (H, W)[axis]
    first = np.arange(n) < (n // 32) * 16 + 8
    return p, np.where(first[None, :] if axis == 1 else first[:, None], ca, cb)


def weights_of(ref):
    """(the whole-block blend's confidence, the overlapped blend's) per pixel"""
    return ref["conf"], ref["info"]["cbar"]


# ================================================================ running the device call
@pytest.fixture(params=backends.engine_params())
def eng(request):
    return backends.get_engine(request.param)


def run(eng, src, cur, prev=None, levels=1, subpel=0, overlap=1, alias=False, off=(0, 0, 0), soff=0, poff=None, foff=None, **kw):
    """eng.temporal_f32(levels=, subpel=, overlap=) on host arrays -> dict as obmc_ref's device part (mvf None with subpel 0: such a slot has
    none); off: floats past a 16-byte boundary of src, cur, dst; soff / poff / foff: bytes of the state, pyramid and mvf buffers.  Every
    output lies between guards, which must come back untouched, and the previous state is read only."""
    poff, foff = soff if poff is None else poff, soff if foff is None else foff
    mem = eng.mem
    Ho, Wo = cur.shape[:2]
    _, s, _ = placed(eng, src, off[0], 0)
    cbuf, c, c0 = placed(eng, cur, off[1], GUARD)
    dbuf, d, d0 = (cbuf, c, c0) if alias else placed(eng, np.full(cur.shape, SENTINEL, np.float32), off[2], GUARD)
    state, spyr = slot_buffers(eng, Ho, Wo, off=soff), pyr_buffer(eng, Ho, Wo, levels, off=poff) if levels > 1 else None
    smvf = mvf_buffer(eng, Ho, Wo, foff) if subpel else None
    tail = lambda pyr, mvf: ((pyr[1],) if levels > 1 else ()) + ((mvf[1],) if subpel else ())
    before = bpyr = bmvf = pslot = None
    if prev is not None:
        before = slot_buffers(eng, Ho, Wo, fill=prev[:2], off=soff)
        bpyr = pyr_buffer(eng, Ho, Wo, levels, prev[2], off=poff) if levels > 1 else None
        bmvf = mvf_buffer(eng, Ho, Wo, foff) if subpel else None
        pslot = tuple(b[1] for b in before) + tail(bpyr, bmvf)
    eng.temporal_f32(s, c, d, tuple(b[1] for b in state) + tail(spyr, smvf), prev=pslot, levels=levels, subpel=subpel, overlap=overlap, **kw)
    whole = np.array(mem.to_numpy(dbuf), copy=True).reshape(-1)
    assert np.all(whole[:d0] == SENTINEL) and np.all(whole[d0 + cur.size:] == SENTINEL), "a write outside the destination"
    luma, out88, mv = read_slot(eng, state, Ho, Wo)
    lumas, vs = read_pyr(eng, spyr, Ho, Wo, levels) if levels > 1 else ([], [])
    if prev is not None:
        pl, po, _ = read_slot(eng, before, Ho, Wo)
        assert np.array_equal(pl, prev[0]) and np.array_equal(po, prev[1])
        assert levels == 1 or all(np.array_equal(a, b) for a, b in zip(read_pyr(eng, bpyr, Ho, Wo, levels)[0], prev[2]))
        assert not subpel or np.all(read_mvf(eng, bmvf, Ho, Wo).view(np.uint8) == MVF_FILL)
    return dict(luma=luma, mv=mv, mvf=read_mvf(eng, smvf, Ho, Wo) if subpel else None, out88=out88,
                dst=whole[d0:d0 + cur.size].reshape(cur.shape), lumas=lumas, vs=vs)


def equal(got, want):
    return all(np.array_equal(got[k], want[k]) for k in ("luma", "mv", "out88")) and same(got["dst"], want["dst"]) and \
        (got["mvf"] is None or (np.array_equal(got["mvf"], want["mvf"]) and got["mvf"].dtype == np.int8)) and \
        got["mv"].dtype == np.int8 and got["out88"].dtype.kind == "u" and len(got["lumas"]) == len(want["lumas"]) and \
        all(np.array_equal(a, b) for a, b in zip(got["lumas"], want["lumas"])) and all(np.array_equal(a, b) for a, b in zip(got["vs"], want["vs"]))


def state_of(res):
    return (res["luma"], res["out88"], res["lumas"])


SHAPES = [(1, 1, 1, 1), (16, 16, 16, 16), (14, 30, 17, 33), (33, 47, 33, 47), (48, 64, 48, 64), (64, 80, 64, 80)]      # H, W, Ho, Wo
_edges = {}


def edge_case(shape):
    """tests.test_temporal.case with sources whose blocks move differently: (src0, cur0, src1, cur1), src [4, H, W, 3], cur [3, Ho, Wo, 3],
    built once and read-only.  Source kind 0: the two-region noise frame, the edge between columns in mid-block; 1: case's source with NaN,
    infinities and values off the scale (moved by (2, -3)); 2: a smooth texture whose two regions, split between rows, move by different
    fractions; 3: independent noise.  cur0 and cur1 are case's, every kind."""
    if shape not in _edges:
        H, W = shape[:2]
        s0, cur0, s1, cur1 = case(shape)
        rs = np.random.RandomState(H * 131 + W)
        pa, ca = two_region(H, W, 5 + H)
        pt, ct = two_textures(H, W, 9 + W, axis=0)
        src0 = np.stack([grey(pa), s0[1], grey(pt), rs.uniform(0, 255, (H, W, 3)).astype(np.float32)])
        src1 = np.stack([grey(ca), s1[1], grey(ct) + rs.randint(-1, 2, (H, W, 3)).astype(np.float32),
                         rs.uniform(0, 255, (H, W, 3)).astype(np.float32)])
        for a in (src0, src1):
            a.setflags(write=False)
        _edges[shape] = (src0, cur0, src1, cur1)
    return _edges[shape]


REGIONS = [((64, 80), 1), ((64, 80), 0), ((48, 64), 1), ((48, 64), 0)]     # (Ho, Wo), the axis the edge cuts


def region_ref(size, axis, subpel=0, K=256, q8=256, levels=1):
    """The two-region noise frame against its previous frame, the previous output a third noise picture -> (cur8, prev, cur, obmc_ref's dict)"""
    Ho, Wo = size
    va, vb = ((0, 3), (0, -3)) if axis == 1 else ((3, 0), (-3, 0))
    p8, c8 = two_region(Ho, Wo, 3, axis, va, vb)
    p88 = np.random.RandomState(11).randint(0, 65281, (Ho, Wo, 3)).astype(np.uint16)
    cur = case((Ho, Wo, Ho, Wo))[3][0]
    prev = (p8, p88, pyramid(p8, levels)[1:])
    return c8, prev, cur, obmc_ref(grey(c8), cur, prev=prev, levels=levels, subpel=subpel, q8=q8, K=K)


# ================================================================ the restatement itself (CPU)
def test_restatement_window():
    blk, w = window(48, 3)
    assert np.all(w.sum(axis=1) == 32) and w.min() >= 1 and w.max() <= 31
    assert blk[:8].tolist() == [[0, 0]] * 8 and w[0].tolist() == [15, 17] and w[7].tolist() == [1, 31]      # j0 = -1: both clamp to block 0
    assert blk[8].tolist() == [0, 1] and w[8].tolist() == [31, 1] and blk[23].tolist() == [0, 1] and w[23].tolist() == [1, 31]
    assert blk[24].tolist() == [1, 2] and blk[39].tolist() == [1, 2] and blk[40:].tolist() == [[2, 2]] * 8
    own = np.arange(48) >> 4                                    # symmetric about the centres 16 b + 7.5; the own block weighs at least 17
    mine = np.where(blk[:, 0] == own, w[:, 0], 0) + np.where(blk[:, 1] == own, w[:, 1], 0)
    assert mine.min() == 17 and np.array_equal(mine, mine[::-1])
    assert window(1, 1)[0].tolist() == [[0, 0]] and window(17, 2)[0][16].tolist() == [0, 1]
    oc = own_candidate(33, 47)
    assert oc[0, 0] == 3 and oc[8, 8] == 0 and oc[7, 8] == 2 and oc[8, 7] == 1 and oc[32, 46] == 2


def test_restatement_fetch_q_is_the_whole_block_fetch_for_one_vector():
    rs = np.random.RandomState(2)
    p8, p88 = rs.randint(0, 256, (33, 47)).astype(np.uint8), rs.randint(0, 65281, (33, 47, 3)).astype(np.uint16)
    mv, mvf = rs.randint(-9, 10, (3, 3, 2)).astype(np.int8), rs.randint(-2, 3, (3, 3, 2)).astype(np.int8)
    y, x = np.indices((33, 47))
    Q = (4 * np.clip(mv.astype(np.int64), -7, 7) + mvf)[y >> 4, x >> 4]
    a, b = fetch_q(p8, p88, Q), fetch(p8, p88, mv, mvf, 7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_restatement_equal_vectors_are_the_whole_block_blends():
    """Consequence 1 on the restatement: uniform motion, a still picture, a frame of one block"""
    for (Ho, Wo), (dy, dx), S in (((48, 64), (0, 0), 0), ((48, 64), (2, -3), 0), ((33, 47), (0, 0), 2), ((16, 16), (1, 1), 2), ((1, 1), (0, 0), 2)):
        a, moved = moved_pair(Ho, Wo, dy, dx, 4)
        p88 = np.random.RandomState(8).randint(0, 65281, (Ho, Wo, 3)).astype(np.uint16)
        cur = case((Ho, Wo, Ho, Wo))[3][0]
        for K, q8 in ((1, 77), (256, 256)):
            ref = obmc_ref(grey(moved), cur, prev=(a, p88, []), subpel=S, K=K, q8=q8)
            eq = masks(ref)[0]
            assert np.array_equal(ref["F"][eq], ref["whole"][eq]) and np.array_equal(ref["info"]["cbar"][eq], ref["conf"][eq])
            if S == 0:
                assert np.array_equal(ref["whole"], blend(cur, moved, a, p88, ref["mv"], q8, K))
    a, moved = moved_pair(64, 80, 2, -3, 4)                     # wrapped noise: every block finds (2, -3), so every pixel is the whole-block one
    ref = obmc_ref(grey(moved), case((64, 80, 64, 80))[3][0], prev=(a, np.zeros((64, 80, 3), np.uint16), []), q8=200)
    assert masks(ref)[0].all() and np.array_equal(ref["F"], ref["whole"])


@pytest.mark.parametrize("size,axis", REGIONS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "axis%d" % v)
def test_restatement_two_regions(size, axis):
    """The known answers of the two-region frames at sensitivity 256 and strength 1: no pixel's weight falls, strictly fewer pixels have none
    and strictly more have all of it than under the whole-block blend of the same vectors; consequences 1 to 3; F in range"""
    for S in (0, 2):
        c8, prev, cur, ref = region_ref(size, axis, subpel=S)
        check_region(ref)
    lo, hi = weights_of(region_ref(size, axis)[3])
    if size == (64, 80) and axis == 1:                          # the frame of the issue: a tenth of the pixels are lost to the vote, all are won back
        assert np.count_nonzero(lo == 0) > 400 and np.count_nonzero(hi == 0) < 40


def check_region(ref, out88=None):
    """The known answers on a restatement dict of a frame whose blocks move differently; out88: the device's, held to them as well"""
    lo, hi = weights_of(ref)
    eq, alone, _ = masks(ref)
    assert np.all(hi >= lo)                                                                     # consequence 3
    assert np.count_nonzero(hi == 0) < np.count_nonzero(lo == 0) and np.count_nonzero(hi == 256) > np.count_nonzero(lo == 256)
    assert 0 < np.count_nonzero(eq) < eq.size and np.count_nonzero(alone & ~eq) > 0
    for F in (ref["F"],) + (() if out88 is None else (out88.astype(np.int64),)):
        assert np.array_equal(F[eq], ref["whole"][eq]) and np.array_equal(F[alone], ref["whole"][alone])     # consequences 1 and 2
        assert F.min() >= 0 and F.max() <= 65280
    assert np.array_equal(hi[eq], lo[eq]) and np.array_equal(hi[alone], lo[alone])


def test_restatement_smooth_regions_gain_weight():
    """Smooth two-region texture at sensitivity 16: the mean weight rises"""
    p8, c8 = two_textures(64, 80, 3, va=(0, 12), vb=(0, -12))
    ref = obmc_ref(grey(c8), grey(c8), prev=(p8, np.zeros((64, 80, 3), np.uint16), []), subpel=2, K=16)
    lo, hi = weights_of(ref)
    assert np.all(hi >= lo) and hi.mean() > lo.mean()


def test_restatement_rest_cases():
    """Consequences 4 and 5 on the restatement"""
    Ho, Wo = 48, 64
    src0, cur0, src1, cur1 = case((Ho, Wo, Ho, Wo))
    p8, c8 = two_region(Ho, Wo, 3)
    p88 = to88(cur0[0]).astype(np.uint16)
    for S in (0, 2):
        assert np.array_equal(obmc_ref(grey(c8), cur1[1], prev=(p8, p88, []), subpel=S, q8=0)["F"], to88(cur1[1]))
        assert np.array_equal(obmc_ref(grey(c8), cur1[1], subpel=S)["F"], to88(cur1[1]))
        far = obmc_ref(grey(150 + (c8 % 100)), cur1[0], prev=((p8 % 100).astype(np.uint8), p88, []), subpel=S, K=6)     # every e >= 50: e K >= 256
        assert not far["info"]["D"].any() and np.array_equal(far["F"], to88(cur1[0]))
        still = obmc_ref(grey(p8), cur1[0], prev=(p8, p88, []), subpel=S, q8=256)
        rest = masks(still)[2]
        assert rest.mean() > 0.9 and np.array_equal(still["out88"][rest], p88[rest])


# ================================================================ the device against the restatement
@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_two_frames_match_the_restatement(eng, shape, levels):
    """Both matrices, both channel orders and every radius, the nine pairs of sensitivity and strength going round, whole and quarter pixels
    alternating; the four source kinds of edge_case; a first frame (no previous state) and a second one fed with the first one's state."""
    src0, cur0, src1, cur1 = edge_case(shape)
    mixed = 0
    for i, kw in enumerate(COMBOS):
        kind, S = (i + i // 4) % 4, 2 * ((i + i // 3 + levels) % 2)
        first = run(eng, src0[kind], cur0[kind % 3], levels=levels, subpel=S, **device_kw(**kw))
        assert equal(first, obmc_ref(src0[kind], cur0[kind % 3], levels=levels, subpel=S, **kw)), ("first", kw, S)
        assert not first["mv"].any() and np.array_equal(first["out88"], to88(cur0[kind % 3]))
        second = run(eng, src1[kind], cur1[kind % 3], prev=state_of(first), levels=levels, subpel=S, **device_kw(**kw))
        want = obmc_ref(src1[kind], cur1[kind % 3], prev=state_of(first), levels=levels, subpel=S, **kw)
        assert equal(second, want), ("second", kw, S)
        if kw["q8"] == 0:
            assert np.array_equal(second["out88"], to88(cur1[kind % 3]))
        eq = masks(want)[0]
        mixed += int(np.count_nonzero(~eq & (want["info"]["D"] > 0)))
        assert np.array_equal(second["out88"][eq], want["whole"][eq])
    assert (mixed == 0) == (shape[2:] in ((1, 1), (16, 16)))    # (the cases do exercise the four-candidate path, except in a frame of one block)


@pytest.mark.parametrize("size,axis", REGIONS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "axis%d" % v)
def test_two_regions_on_the_device(eng, size, axis):
    for S, levels in ((0, 1), (2, 1), (2, 3)):
        c8, prev, cur, ref = region_ref(size, axis, subpel=S, levels=levels)
        got = run(eng, grey(c8), cur, prev=prev, levels=levels, subpel=S, **device_kw(K=256))
        assert equal(got, ref)
        check_region(ref, got["out88"])
        whole = (run_sub(eng, grey(c8), cur, prev=prev, levels=levels, subpel=S, **device_kw(K=256)) if S else
                 run_pyr(eng, grey(c8), cur, prev=prev, levels=levels, **device_kw(K=256)))["out88"]
        eq, alone, _ = masks(ref)                               # consequences 1 and 2 against the device's own whole-block blend
        assert np.array_equal(got["out88"][eq], whole[eq]) and np.array_equal(got["out88"][alone], whole[alone])
        assert np.array_equal(whole, ref["whole"])


def test_smooth_regions_on_the_device(eng):
    for axis, va, vb in ((1, (0, 12), (0, -12)), (0, (3, -2), (-5, 6))):
        p8, c8 = two_textures(64, 80, 3, axis, va, vb)
        prev = (p8, np.random.RandomState(5).randint(0, 65281, (64, 80, 3)).astype(np.uint16), [])
        cur = case((64, 80, 64, 80))[3][2]
        for S in (1, 2):
            ref = obmc_ref(grey(c8), cur, prev=prev, subpel=S, q8=200)
            lo, hi = weights_of(ref)
            assert np.all(hi >= lo) and hi.mean() > lo.mean()
            assert equal(run(eng, grey(c8), cur, prev=prev, subpel=S, **device_kw(q8=200)), ref)


def test_equal_vectors_are_the_whole_block_blends_on_the_device(eng):
    """Consequence 1: uniform motion (wrapped noise: every block finds the move), a frame of one block, one pixel"""
    for (Ho, Wo), (dy, dx), S, levels in (((64, 80), (2, -3), 0, 1), ((48, 64), (1, -2), 2, 2), ((16, 16), (1, 1), 2, 1), ((1, 1), (0, 0), 0, 1)):
        a, moved = moved_pair(Ho, Wo, dy, dx, 4)
        prev = (a, np.random.RandomState(8).randint(0, 65281, (Ho, Wo, 3)).astype(np.uint16), pyramid(a, levels)[1:])
        cur = case((Ho, Wo, Ho, Wo))[3][0]
        ref = obmc_ref(grey(moved), cur, prev=prev, levels=levels, subpel=S, q8=200, K=4)
        assert masks(ref)[0].all() and np.array_equal(ref["F"], ref["whole"])
        got = run(eng, grey(moved), cur, prev=prev, levels=levels, subpel=S, **device_kw(q8=200, K=4))
        whole = run_sub(eng, grey(moved), cur, prev=prev, levels=levels, subpel=S, **device_kw(q8=200, K=4)) if S else \
            run_pyr(eng, grey(moved), cur, prev=prev, levels=levels, **device_kw(q8=200, K=4))
        assert equal(got, ref) and np.array_equal(got["out88"], whole["out88"]) and same(got["dst"], whole["dst"])


def test_rest_cases_on_the_device(eng):
    """Consequences 4 and 5: strength 0, a first frame and e K >= 256 everywhere return to88(cur); strength 256 on a still picture returns
    the first frame wherever the four vectors are (0, 0)"""
    Ho, Wo = 48, 64
    src0, cur0, src1, cur1 = case((Ho, Wo, Ho, Wo))
    p8, c8 = two_region(Ho, Wo, 3)
    p88 = to88(cur0[0]).astype(np.uint16)
    for S in (0, 2):
        got = run(eng, grey(c8), cur1[1], prev=(p8, p88, []), subpel=S, **device_kw(q8=0))
        assert np.array_equal(got["out88"], to88(cur1[1])) and equal(got, obmc_ref(grey(c8), cur1[1], prev=(p8, p88, []), subpel=S, q8=0))
        got = run(eng, grey(c8), cur1[1], subpel=S)
        assert np.array_equal(got["out88"], to88(cur1[1])) and equal(got, obmc_ref(grey(c8), cur1[1], subpel=S))
        far8, near8 = (150 + (c8 % 100)).astype(np.uint8), (p8 % 100).astype(np.uint8)
        got = run(eng, grey(far8), cur1[0], prev=(near8, p88, []), subpel=S, **device_kw(K=6))
        assert np.array_equal(got["out88"], to88(cur1[0])) and equal(got, obmc_ref(grey(far8), cur1[0], prev=(near8, p88, []), subpel=S, K=6))
        ref = obmc_ref(grey(p8), cur1[0], prev=(p8, p88, []), subpel=S, q8=256)
        got = run(eng, grey(p8), cur1[0], prev=(p8, p88, []), subpel=S, **device_kw(q8=256))
        rest = masks(ref)[2]
        assert equal(got, ref) and rest.any() and np.array_equal(got["out88"][rest], p88[rest])


def lib_call(eng, src, cur, prev, levels, subpel, overlap, q8=256, K=16, R=7, matrix=0, bgr=False, null_mvf=False):
    """fs_temporal_obmc_f32 itself on guarded buffers -> dict as run's (mvf always read: untouched with subpel 0)"""
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
    rc = eng.lib.fs_temporal_obmc_f32(eng.ctx, mem.ptr(s), src.shape[0], src.shape[1], mem.ptr(c), Ho, Wo, q8, K, R, levels, subpel, overlap, matrix,
                                      int(bgr), None if before is None else p8(before[0][1]), None if before is None else p8(before[1][1]),
                                      None if bpyr is None else p8(bpyr[1]), p8(state[0][1]), p8(state[1][1]), None if spyr is None else p8(spyr[1]),
                                      p8(state[2][1]), None if null_mvf else p8(smvf[1]), mem.ptr(d))
    assert rc == 0, eng.lib.fs_last_error()
    whole = np.array(mem.to_numpy(dbuf), copy=True).reshape(-1)
    assert np.all(whole[:d0] == SENTINEL) and np.all(whole[d0 + cur.size:] == SENTINEL)
    luma, out88, mv = read_slot(eng, state, Ho, Wo)
    lumas, vs = read_pyr(eng, spyr, Ho, Wo, levels) if levels > 1 else ([], [])
    return dict(luma=luma, mv=mv, mvf=read_mvf(eng, smvf, Ho, Wo), out88=out88, dst=whole[d0:d0 + cur.size].reshape(cur.shape), lumas=lumas, vs=vs)


def bytes_equal(a, b, mvf=False):
    return all(np.array_equal(a[k], b[k]) for k in ("luma", "mv", "out88") + (("mvf",) if mvf else ())) and same(a["dst"], b["dst"]) and \
        len(a["lumas"]) == len(b["lumas"]) and all(np.array_equal(x, y) for x, y in zip(a["lumas"] + a["vs"], b["lumas"] + b["vs"]))


@pytest.mark.parametrize("shape", [(14, 30, 17, 33), (48, 64, 48, 64)], ids=ids)
def test_overlap_zero_is_the_existing_stage(eng, shape):
    """overlap = 0 through the new entry point: fs_temporal_sub_f32 in every output byte, fs_temporal_pyr_f32 at subpel 0 (a sentinel-filled
    mvf comes back untouched, a null one is taken) and fs_temporal_f32 at one level; overlap = 1 at subpel 0 leaves mvf alone as well."""
    src0, cur0, src1, cur1 = edge_case(shape)
    Ho, Wo = shape[2:]
    for levels, S, kw in ((1, 0, COMBOS[2]), (1, 2, COMBOS[5]), (2, 0, COMBOS[7]), (3, 1, COMBOS[10])):
        c8 = luma8(src0[0], Ho, Wo, kw["matrix"], kw["bgr"])
        prev = (c8, to88(cur0[0]).astype(np.uint16), pyramid(c8, levels)[1:])
        for pv in (None, prev):
            got = lib_call(eng, src1[0], cur1[0], pv, levels, S, 0, **kw)
            if S:
                assert bytes_equal(got, run_sub(eng, src1[0], cur1[0], prev=pv, levels=levels, subpel=S, **device_kw(**kw)), mvf=True), (levels, S)
            else:
                assert np.all(got["mvf"].view(np.uint8) == MVF_FILL)
                assert bytes_equal(got, run_pyr(eng, src1[0], cur1[0], prev=pv, levels=levels, **device_kw(**kw)))
                assert bytes_equal(lib_call(eng, src1[0], cur1[0], pv, levels, 0, 0, null_mvf=True, **kw), got)
                if levels == 1:
                    one = run_one_level(eng, src1[0], cur1[0], prev=None if pv is None else pv[:2], **device_kw(**kw))
                    assert bytes_equal(got, dict(one, lumas=[], vs=[]))
                over = lib_call(eng, src1[0], cur1[0], pv, levels, 0, 1, **kw)
                assert np.all(over["mvf"].view(np.uint8) == MVF_FILL)
                assert bytes_equal(lib_call(eng, src1[0], cur1[0], pv, levels, 0, 1, null_mvf=True, **kw), over)
                assert equal(dict(over, mvf=None), obmc_ref(src1[0], cur1[0], prev=pv, levels=levels, **kw))


@pytest.mark.parametrize("shift", [(-9, 9), (9, -9)], ids=lambda s: "dy%d_dx%d" % s)
def test_vectors_that_point_out_of_the_frame_clamp(eng, shift):
    """A hand-written previous state whose blocks on two edges find vectors that point out of the frame (tests/test_temporal_sub.py), here
    with an inner region that stays: the candidates' rows and columns clamp under their fractions.  40 x 52 has ragged blocks."""
    Ho, Wo = 40, 52
    dy, dx = shift
    p8, o8 = texture_pair(Ho, Wo, 0, 0, 1, sigma=3.0)[0], texture_pair(Ho, Wo, 0, 0, 101, sigma=3.0)[0]
    c8 = ((p8[np.clip(np.arange(Ho) + dy, 0, Ho - 1)][:, np.clip(np.arange(Wo) + dx, 0, Wo - 1)].astype(np.int64) * 3 + o8) >> 2).astype(np.uint8)
    c8[12:28, 20:36] = p8[12:28, 20:36]
    p88 = np.random.RandomState(6).randint(0, 65281, (Ho, Wo, 3)).astype(np.uint16)
    cur = case((Ho, Wo, Ho, Wo))[3][0]
    prev = (p8, p88, pyramid(p8, 2)[1:])
    want = obmc_ref(grey(c8), cur, prev=prev, levels=2, subpel=2, q8=200, K=4)
    Q = want["info"]["Q"]
    y, x = np.indices((Ho, Wo))
    Y, X = (4 * y + Q[..., 0]) >> 2, (4 * x + Q[..., 1]) >> 2
    assert ((Y < 0) | (Y + 1 > Ho - 1)).any() and ((X < 0) | (X + 1 > Wo - 1)).any() and not masks(want)[0].all()
    assert equal(run(eng, grey(c8), cur, prev=prev, levels=2, subpel=2, **device_kw(q8=200, K=4)), want)


@pytest.mark.parametrize("levels", [1, 2])
def test_the_destination_may_be_the_current_tensor(eng, levels):
    for shape in ((14, 30, 17, 33), (33, 47, 33, 47)):
        src0, cur0, src1, cur1 = edge_case(shape)
        Ho, Wo = shape[2:]
        for kind, kw, S in ((0, dict(q8=77, K=1), 2), (2, dict(q8=256, K=16, R=3, matrix=1, bgr=True), 0)):
            c8 = luma8(src0[kind], Ho, Wo, kw.get("matrix", 0), kw.get("bgr", False))
            prev = (c8, to88(cur0[0]).astype(np.uint16), pyramid(c8, levels)[1:])
            got = run(eng, src1[kind], cur1[0], prev=prev, levels=levels, subpel=S, alias=True, **device_kw(**kw))
            assert equal(got, obmc_ref(src1[kind], cur1[0], prev=prev, levels=levels, subpel=S, **kw)), kw


def test_tensors_and_state_off_sixteen_byte_alignment_give_the_same_values(eng):
    shape = (33, 47, 33, 47)
    src0, cur0, src1, cur1 = edge_case(shape)
    c8 = luma8(src0[0], 33, 47)
    prev = (c8, to88(cur0[0]).astype(np.uint16), pyramid(c8, 3)[1:])
    want = obmc_ref(src1[0], cur1[0], prev=prev, levels=3, subpel=2, q8=128, K=4)
    assert not masks(want)[0].all()
    for off, soff, poff, foff in (((1, 0, 0), 0, 0, 1), ((0, 1, 0), 0, 1, 0), ((0, 0, 1), 0, 7, 3), ((0, 0, 0), 2, 2, 2), ((3, 2, 1), 6, 13, 9)):
        got = run(eng, src1[0], cur1[0], prev=prev, levels=3, subpel=2, off=off, soff=soff, poff=poff, foff=foff, **device_kw(q8=128, K=4))
        assert equal(got, want), (off, soff, poff, foff)


def test_engine_slots(eng):
    """Engine.temporal_f32(overlap=1) on the engine's own slots, which are those of (levels, subpel) without it"""
    shape = (33, 47, 33, 47)
    src0, cur0, src1, cur1 = edge_case(shape)
    mem = eng.mem
    for levels, S in ((1, 0), (1, 2), (2, 0), (3, 2)):
        slots = [eng.temporal_state(33, 47, levels, S) for _ in range(2)]
        assert len(slots[0]) == 3 + (levels > 1) + (S > 0)
        d = mem.empty((33, 47, 3))
        eng.temporal_f32(mem.from_numpy(src0[0]), mem.from_numpy(cur0[0]), d, slots[0], levels=levels, subpel=S, overlap=1)
        first = obmc_ref(src0[0], cur0[0], levels=levels, subpel=S)
        eng.temporal_f32(mem.from_numpy(src1[0]), mem.from_numpy(cur1[0]), d, slots[1], prev=slots[0], levels=levels, subpel=S, overlap=1)
        second = obmc_ref(src1[0], cur1[0], prev=state_of(first), levels=levels, subpel=S)
        assert same(np.asarray(mem.to_numpy(d)), second["dst"])
        assert np.array_equal(np.asarray(mem.to_numpy(slots[1][2])).view(np.int8), second["mv"])
        eng.temporal_f32(mem.from_numpy(src1[0]), mem.from_numpy(cur1[0]), d, slots[1], prev=slots[0], levels=levels, subpel=S, overlap=0)
        assert same(np.asarray(mem.to_numpy(d)), second["whole"].astype(np.float32) * np.float32(0.00390625))


def test_refused_calls_return_their_code_and_launch_nothing(eng):
    mem, lib, ctx = eng.mem, eng.lib, eng.ctx
    H, W, Ho, Wo, levels = 14, 30, 17, 33, 3
    src0, cur0, src1, cur1 = edge_case((H, W, Ho, Wo))
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

    def call(src=ps, H=H, W=W, cur=pc, Ho=Ho, Wo=Wo, q8=128, K=16, R=7, levels=levels, subpel=2, overlap=1, matrix=0, bgr=0, prev_luma=ql,
             prev_out88=qo, prev_pyr=qp, luma=pl, out88=po, pyr=pp, mv=pm, mvf=pf, dst=pd):
        return lib.fs_temporal_obmc_f32(ctx, src, H, W, cur, Ho, Wo, q8, K, R, levels, subpel, overlap, matrix, bgr, prev_luma, prev_out88, prev_pyr,
                                        luma, out88, pyr, mv, mvf, dst)

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
               (-2, dict(subpel=0, levels=4)), (-1, dict(subpel=0, pyr=None)),
               (-2, dict(overlap=2)), (-2, dict(overlap=-1)), (-2, dict(overlap=2, subpel=0, mvf=None)), (-1, dict(overlap=0, mvf=None)),
               (-2, dict(overlap=0, subpel=3)), (-1, dict(overlap=0, src=None)), (-5, dict(overlap=0, dst=pd + 3))]
    for code, kw in refused:
        assert call(**kw) == code, kw
        assert b"fs_temporal_obmc_f32" in lib.fs_last_error()
    assert lib.fs_temporal_obmc_f32(None, ps, H, W, pc, Ho, Wo, 128, 16, 7, levels, 2, 1, 0, 0, ql, qo, qp, pl, po, pp, pm, pf, pd) == -1
    assert np.all(np.asarray(mem.to_numpy(dbuf)) == SENTINEL)                                 # nothing was launched
    assert all(np.all(np.asarray(mem.to_numpy(b[0])) == FILL) for b in state + [spyr, smvf])
    # the call they were variations of is taken, with and without a previous frame
    assert call() == 0
    got = np.asarray(mem.to_numpy(dbuf)).reshape(-1)[d0:d0 + cur1[0].size].reshape(cur1[0].shape)
    want = obmc_ref(src1[0], cur1[0], prev=prevh, levels=levels, subpel=2, q8=128)
    luma, out88, mv = read_slot(eng, state, Ho, Wo)
    lumas, vs = read_pyr(eng, spyr, Ho, Wo, levels)
    assert equal(dict(luma=luma, mv=mv, mvf=read_mvf(eng, smvf, Ho, Wo), out88=out88, dst=got, lumas=lumas, vs=vs), want)
    assert call(prev_luma=None, prev_out88=None, prev_pyr=None) == 0
    assert np.array_equal(read_slot(eng, state, Ho, Wo)[1], to88(cur1[0])) and not read_mvf(eng, smvf, Ho, Wo).any()
    # the engine checks overlap, and the slot's length and shapes for (levels, subpel)
    views = tuple(b[1] for b in state) + (spyr[1], smvf[1])
    for bad in (dict(cur=s), dict(state=eng.temporal_state(Ho, Wo - 1, levels, 2)), dict(prev=eng.temporal_state(Ho, Wo - 1, levels, 2)),
                dict(state=views[:4]), dict(state=views[:3] + views[4:]), dict(state=eng.temporal_state(Ho, Wo, 2, 2)),
                dict(prev=eng.temporal_state(Ho, Wo, levels)), dict(state=views, subpel=0), dict(levels=0), dict(levels=4), dict(subpel=3),
                dict(subpel=-1), dict(overlap=2), dict(overlap=-1), dict(overlap=1.0), dict(overlap=True)):
        a = dict(dict(src=s, cur=c, dst=d, state=views, prev=None, levels=levels, subpel=2, overlap=1), **bad)
        with pytest.raises(L.FaststyleError):
            eng.temporal_f32(a["src"], a["cur"], a["dst"], a["state"], prev=a["prev"], levels=a["levels"], subpel=a["subpel"], overlap=a["overlap"])
    with pytest.raises(L.FaststyleError):
        eng.temporal_f32(s, c, d, views, radius=8, levels=levels, subpel=2, overlap=1)
