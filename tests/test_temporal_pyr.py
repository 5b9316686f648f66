"""The coarse-to-fine block search of the temporal stage (csrc/fs_temporal.hip: fs_temporal_pyr_f32) against its contract in
include/faststyle_io.h.  The first part of this file is an independent numpy restatement of that text (int64 and >>), built on the luma and
the blend of tests/test_temporal.py; every comparison of the device with the restatement -- the pyramid lumas, every level's vectors, mv, the
8.8 state and the float result -- is equality.  The same bodies run on the CPU emulator and, under -m gpu, on the MI355X.
tests/test_temporal_pyr_stream.py builds its expected tensors with the restatement."""
import itertools

import numpy as np
import pytest

from faststyle_amd import _lib as L
from tests import backends
from tests.test_compose import GUARD, SENTINEL, placed, same, to88
from tests.test_temporal import FILL, blend, blocks_of, case, device_kw, grey, luma8, read_slot, search, slot_buffers, temporal_ref


# ================================================================ the restatement
def level_sizes(Ho, Wo, levels):
    out = [(Ho, Wo)]
    for _ in range(1, levels):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def layout(Ho, Wo, levels):
    """-> (sizes, luma offsets, vector offsets, bytes) of the extra state buffer: lumas of the levels 1 .., then their vectors, each part on a
    multiple of 16 (entry 0 of both offset lists is 0 and unused)"""
    sizes = level_sizes(Ho, Wo, levels)
    lo, vo, at = [0] * levels, [0] * levels, 0
    for l in range(1, levels):
        lo[l] = at
        at += (sizes[l][0] * sizes[l][1] + 15) // 16 * 16
    for l in range(1, levels):
        nby, nbx = blocks_of(*sizes[l])
        vo[l] = at
        at += (nby * nbx * 2 + 15) // 16 * 16
    return sizes, lo, vo, at


def halve(a):
    """uint8 [H,W] -> uint8 [ceil(H / 2), ceil(W / 2)]: the rounded mean of 2 x 2, the odd edge clamped"""
    H, W = a.shape
    a = a.astype(np.int64)
    y, x = np.arange((H + 1) // 2), np.arange((W + 1) // 2)
    ya, yb, xa, xb = np.minimum(2 * y, H - 1), np.minimum(2 * y + 1, H - 1), np.minimum(2 * x, W - 1), np.minimum(2 * x + 1, W - 1)
    return ((a[ya][:, xa] + a[ya][:, xb] + a[yb][:, xa] + a[yb][:, xb] + 2) >> 2).astype(np.uint8)


def pyramid(c8, levels):
    out = [c8]
    for _ in range(1, levels):
        out.append(halve(out[-1]))
    return out


def search_level(cur, prev, R, pred):
    """One level: cur, prev uint8 [H,W] (prev None: zeros), pred int64 [nby,nbx,2] -> v int64 [nby,nbx,2] = pred + the best refinement"""
    H, W = cur.shape
    nby, nbx = blocks_of(H, W)
    v = np.zeros((nby, nbx, 2), np.int64)
    if prev is None:
        return v
    c, p = cur.astype(np.int64), prev.astype(np.int64)
    r = np.arange(-R, R + 1)
    mag = np.abs(r)[:, None] + np.abs(r)[None, :]
    for by, bx in itertools.product(range(nby), range(nbx)):
        ys, xs = np.arange(by * 16, min(by * 16 + 16, H)), np.arange(bx * 16, min(bx * 16 + 16, W))
        py, px = pred[by, bx]
        Y = np.clip(ys[None, :] + py + r[:, None], 0, H - 1)                # [n, rows]
        X = np.clip(xs[None, :] + px + r[:, None], 0, W - 1)                # [n, cols]
        sad = np.abs(c[ys][:, xs][None, None] - p[Y[:, None, :, None], X[None, :, None, :]]).sum(axis=(2, 3))
        cost = sad + ((ys.size * xs.size) >> 5) * mag
        assert cost.max() < 1 << 17
        k = ((cost << 12) | (mag << 8) | ((r[:, None] + 7) << 4) | (r[None, :] + 7)).min()
        v[by, bx] = (py + ((k >> 4) & 15) - 7, px + (k & 15) - 7)
    return v


def search_pyr(cur_levels, prev_levels, R):
    """-> [v_0, v_1, ...] int8, v_0 = mv; from the coarsest level down, each block predicted by twice its parent's vector"""
    n = len(cur_levels)
    vs = [None] * n
    for l in range(n - 1, -1, -1):
        nby, nbx = blocks_of(*cur_levels[l].shape)
        by, bx = np.indices((nby, nbx))
        pred = np.zeros((nby, nbx, 2), np.int64) if l == n - 1 else 2 * vs[l + 1][by >> 1, bx >> 1]
        vs[l] = search_level(cur_levels[l], None if prev_levels is None else prev_levels[l], R, pred)
        assert np.abs(vs[l]).max() <= R * ((1 << (n - l)) - 1)
    return [v.astype(np.int8) for v in vs]


def pyr_ref(src, cur, prev=None, levels=2, q8=256, K=16, R=7, matrix=0, bgr=False):
    """src [H,W,3], cur [Ho,Wo,3], prev (luma u8, out88 u16, [lumas of the levels 1 ..]) or None -> dict(luma=, mv=, out88=, dst=, lumas=
    [levels 1 ..], vs= [levels 1 ..])"""
    Ho, Wo = cur.shape[:2]
    cl = pyramid(luma8(src, Ho, Wo, matrix, bgr), levels)
    pl = None if prev is None else [prev[0]] + list(prev[2])
    vs = search_pyr(cl, pl, R)
    F = blend(cur, cl[0], None if prev is None else prev[0], None if prev is None else prev[1], vs[0], q8, K)
    return dict(luma=cl[0], mv=vs[0], out88=F.astype(np.uint16), dst=F.astype(np.float32) * np.float32(0.00390625), lumas=cl[1:], vs=vs[1:])


def interior(Ho, Wo, dy, dx):
    """The blocks that lie wholly inside the frame together with their copy displaced by (dy, dx)"""
    nby, nbx = blocks_of(Ho, Wo)
    return [(by, bx) for by in range(nby) for bx in range(nbx)
            if min(by * 16, by * 16 + dy) >= 0 and max(by * 16, by * 16 + dy) + 15 <= Ho - 1 and
            min(bx * 16, bx * 16 + dx) >= 0 and max(bx * 16, bx * 16 + dx) + 15 <= Wo - 1]


def moved_pair(Ho, Wo, dy, dx, seed):
    """(a, moved): uniform u8 noise and the same moved so that moved[y][x] = a[y + dy][x + dx]"""
    a = np.random.RandomState(seed).randint(0, 256, (Ho, Wo)).astype(np.uint8)
    return a, np.roll(a, (-dy, -dx), axis=(0, 1))


# ================================================================ running the device call
@pytest.fixture(params=backends.engine_params())
def eng(request):
    return backends.get_engine(request.param)


def pyr_buffer(eng, Ho, Wo, levels, lumas=None, off=0):
    """A guarded extra state buffer (buffer, view, start); lumas: host lumas of the levels 1 .. to start from"""
    sizes, lo, _, total = layout(Ho, Wo, levels)
    host = np.zeros(total, np.uint8)
    if lumas is not None:
        for l in range(1, levels):
            host[lo[l]:lo[l] + lumas[l - 1].size] = lumas[l - 1].reshape(-1)
    return placed(eng, host, off, GUARD, u8=True)


def read_pyr(eng, buf, Ho, Wo, levels):
    """-> (lumas, vectors) of the levels 1 .., after checking that nothing outside the buffer was written"""
    sizes, lo, vo, total = layout(Ho, Wo, levels)
    whole = np.array(eng.mem.to_numpy(buf[0]), copy=True).reshape(-1)
    start = buf[2]
    assert np.all(whole[:start] == FILL) and np.all(whole[start + total:] == FILL), "a write outside the pyramid"
    raw = whole[start:start + total]
    lumas = [raw[lo[l]:lo[l] + sizes[l][0] * sizes[l][1]].reshape(sizes[l]) for l in range(1, levels)]
    vs = [raw[vo[l]:vo[l] + 2 * int(np.prod(blocks_of(*sizes[l])))].view(np.int8).reshape(blocks_of(*sizes[l]) + (2,)) for l in range(1, levels)]
    return lumas, vs


def run(eng, src, cur, prev=None, levels=2, alias=False, off=(0, 0, 0), soff=0, poff=None, **kw):
    """eng.temporal_f32(levels=) on host arrays -> dict as pyr_ref's; off: floats past a 16-byte boundary of src, cur, dst; soff: bytes of
    the state buffers, poff: of the pyramid buffers (soff).  Every output lies between guards, which must come back untouched, and the
    previous state is read only.  levels = 1 runs the slots of three buffers."""
    poff = soff if poff is None else poff
    mem = eng.mem
    Ho, Wo = cur.shape[:2]
    _, s, _ = placed(eng, src, off[0], 0)
    cbuf, c, c0 = placed(eng, cur, off[1], GUARD)
    dbuf, d, d0 = (cbuf, c, c0) if alias else placed(eng, np.full(cur.shape, SENTINEL, np.float32), off[2], GUARD)
    state, spyr = slot_buffers(eng, Ho, Wo, off=soff), pyr_buffer(eng, Ho, Wo, levels, off=poff) if levels > 1 else None
    before = bpyr = pslot = None
    if prev is not None:
        before = slot_buffers(eng, Ho, Wo, fill=prev[:2], off=soff)
        bpyr = pyr_buffer(eng, Ho, Wo, levels, prev[2], off=poff) if levels > 1 else None
        pslot = tuple(b[1] for b in before) + ((bpyr[1],) if levels > 1 else ())
    eng.temporal_f32(s, c, d, tuple(b[1] for b in state) + ((spyr[1],) if levels > 1 else ()), prev=pslot, levels=levels, **kw)
    whole = np.array(mem.to_numpy(dbuf), copy=True).reshape(-1)
    assert np.all(whole[:d0] == SENTINEL) and np.all(whole[d0 + cur.size:] == SENTINEL), "a write outside the destination"
    luma, out88, mv = read_slot(eng, state, Ho, Wo)
    lumas, vs = read_pyr(eng, spyr, Ho, Wo, levels) if levels > 1 else ([], [])
    if prev is not None:
        pl, po, _ = read_slot(eng, before, Ho, Wo)
        assert np.array_equal(pl, prev[0]) and np.array_equal(po, prev[1])
        assert levels == 1 or all(np.array_equal(a, b) for a, b in zip(read_pyr(eng, bpyr, Ho, Wo, levels)[0], prev[2]))
    return dict(luma=luma, mv=mv, out88=out88, dst=whole[d0:d0 + cur.size].reshape(cur.shape), lumas=lumas, vs=vs)


def equal(got, want):
    return all(np.array_equal(got[k], want[k]) for k in ("luma", "mv", "out88")) and same(got["dst"], want["dst"]) and \
        got["mv"].dtype == np.int8 and got["out88"].dtype.kind == "u" and len(got["lumas"]) == len(want["lumas"]) and \
        all(np.array_equal(a, b) for a, b in zip(got["lumas"], want["lumas"])) and all(np.array_equal(a, b) for a, b in zip(got["vs"], want["vs"]))


def state_of(res):
    return (res["luma"], res["out88"], res["lumas"])


SHAPES = [(1, 1, 1, 1), (16, 16, 16, 16), (14, 30, 17, 33), (33, 47, 33, 47), (48, 64, 48, 64), (64, 80, 64, 80), (96, 128, 96, 128)]   # H, W, Ho, Wo
RADII, SENSITIVITIES, STRENGTHS = (0, 3, 7), (1, 16, 256), (0, 77, 256)
COMBOS = [dict(matrix=m, bgr=b, R=R, K=SENSITIVITIES[i % 3], q8=STRENGTHS[(i // 3 + i) % 3])
          for i, (m, b, R) in enumerate(itertools.product((0, 1), (False, True), RADII))]
ZERO88 = lambda Ho, Wo: np.zeros((Ho, Wo, 3), np.uint16)
ids = lambda s: "%dx%d_to_%dx%d" % s


# ================================================================ the restatement itself (CPU)
def test_restatement_pyramid_and_layout():
    assert halve(np.array([[1, 2], [3, 4]], np.uint8)).tolist() == [[3]]                        # (10 + 2) >> 2
    assert halve(np.array([[1, 2, 9], [3, 4, 10], [7, 8, 11]], np.uint8)).tolist() == [[3, 10], [8, 11]]    # the odd edge: its last byte twice
    assert halve(np.array([[200]], np.uint8)).tolist() == [[200]]
    assert [a.shape for a in pyramid(np.zeros((33, 47), np.uint8), 3)] == [(33, 47), (17, 24), (9, 12)]
    assert layout(96, 128, 1)[3] == 0
    sizes, lo, vo, total = layout(33, 47, 3)
    assert (lo, vo, total) == ([0, 0, 416], [0, 528, 544], 560)                                 # 17 x 24 = 408 -> 416; 9 x 12 = 108 -> 112; 2 x 2 x 2, 1 x 1 x 2
    assert len(COMBOS) == 12 and len({(c["K"], c["q8"]) for c in COMBOS}) == 9


def test_restatement_with_one_level_is_the_existing_search():
    for shape in ((40, 52, 40, 52), (64, 48, 64, 48)):
        src0, cur0, src1, cur1 = case(shape)
        Ho, Wo = shape[2:]
        p8, c8 = luma8(src0[0], Ho, Wo), luma8(src1[0], Ho, Wo)
        for R in RADII:
            assert np.array_equal(search_pyr([c8], [p8], R)[0], search(c8, p8, R))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_known_moves(seed):
    """What the coarse levels are for: a move beyond 7 pixels is found exactly in every interior block, where one level finds it in none."""
    for (Ho, Wo), (dy, dx), levels, count in (((96, 128), (28, -28), 3, 24), ((48, 64), (12, 0), 2, 8)):
        a, moved = moved_pair(Ho, Wo, dy, dx, seed)
        inside = interior(Ho, Wo, dy, dx)
        assert len(inside) == count
        mv = search_pyr(pyramid(moved, levels), pyramid(a, levels), 7)[0]
        assert all(mv[b].tolist() == [dy, dx] for b in inside)
        one = search_pyr([moved], [a], 7)[0]
        assert not any(one[b].tolist() == [dy, dx] for b in inside)
    # identical frames: at rest on every level
    for levels in (2, 3):
        assert not any(v.any() for v in search_pyr(pyramid(a, levels), pyramid(a, levels), 7))
    # an odd move: the halved lumas do not line up, most blocks are found all the same (how many depends on the seed)
    a, moved = moved_pair(96, 128, -21, 21, seed)
    inside = interior(96, 128, -21, 21)
    mv = search_pyr(pyramid(moved, 3), pyramid(a, 3), 7)[0]
    assert len(inside) == 24 and 2 * sum(mv[b].tolist() == [-21, 21] for b in inside) >= len(inside)


# ================================================================ the device against the restatement
def test_the_layout_query_matches_the_restatement(eng):
    for (H, W, Ho, Wo), levels in itertools.product(SHAPES + [(720, 1280, 720, 1280)], (1, 2, 3)):
        info = eng.temporal_pyr_layout(Ho, Wo, levels)
        sizes, lo, vo, total = layout(Ho, Wo, levels)
        assert info.levels == levels and info.pyr_bytes == total and (levels > 1 or total == 0)
        for l in range(3):
            want = sizes[l] + blocks_of(*sizes[l]) + (lo[l], vo[l]) if l < levels else (0,) * 6
            assert (info.h[l], info.w[l], info.nby[l], info.nbx[l], info.luma_offset[l], info.mv_offset[l]) == want
            assert info.luma_offset[l] % 16 == 0 and info.mv_offset[l] % 16 == 0
        slot = eng.temporal_state(Ho, Wo, levels)
        assert len(slot) == (3 if levels == 1 else 4) and (levels == 1 or tuple(slot[3].shape) == (total,))
    assert tuple(tuple(b.shape) for b in eng.temporal_state(17, 33)) == ((17, 33), (17, 33, 3, 2), (2, 3, 2))
    import ctypes
    info = L.fs_temporal_pyr_info()
    for code, args in ((-1, (0, 8, 2)), (-1, (8, -1, 2)), (-2, (8, 8, 0)), (-2, (8, 8, 4))):
        assert eng.lib.fs_temporal_pyr_layout(*args, ctypes.byref(info)) == code and b"fs_temporal_pyr_layout" in eng.lib.fs_last_error()
    assert eng.lib.fs_temporal_pyr_layout(8, 8, 2, None) == -1
    for bad in (0, 4):
        with pytest.raises(L.FaststyleError):
            eng.temporal_state(17, 33, bad)


def lib_call(eng, src, cur, prev, levels, q8=256, K=16, R=7, matrix=0, bgr=False):
    """fs_temporal_pyr_f32 itself with levels = 1 and no pyramid buffers -> dict(luma=, mv=, out88=, dst=)"""
    mem = eng.mem
    Ho, Wo = cur.shape[:2]
    _, s, _ = placed(eng, src, 0, 0)
    _, c, _ = placed(eng, cur, 0, 0)
    dbuf, d, d0 = placed(eng, np.full(cur.shape, SENTINEL, np.float32), 0, GUARD)
    state = slot_buffers(eng, Ho, Wo)
    before = slot_buffers(eng, Ho, Wo, fill=prev) if prev is not None else None
    eng._sync_stream()
    p8 = mem.ptr_u8
    rc = eng.lib.fs_temporal_pyr_f32(eng.ctx, mem.ptr(s), src.shape[0], src.shape[1], mem.ptr(c), Ho, Wo, q8, K, R, levels, matrix, int(bgr),
                                     None if before is None else p8(before[0][1]), None if before is None else p8(before[1][1]), None,
                                     p8(state[0][1]), p8(state[1][1]), None, p8(state[2][1]), mem.ptr(d))
    assert rc == 0, eng.lib.fs_last_error()
    whole = np.array(mem.to_numpy(dbuf), copy=True).reshape(-1)
    assert np.all(whole[:d0] == SENTINEL) and np.all(whole[d0 + cur.size:] == SENTINEL)
    luma, out88, mv = read_slot(eng, state, Ho, Wo)
    return dict(luma=luma, mv=mv, out88=out88, dst=whole[d0:d0 + cur.size].reshape(cur.shape))


def equal1(got, want):
    return all(np.array_equal(got[k], want[k]) for k in ("luma", "mv", "out88")) and same(got["dst"], want["dst"])


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_one_level_is_the_existing_stage(eng, shape):
    """levels = 1 through the new entry point: temporal_ref and Engine.temporal_f32 without levels, in luma, vectors, state and result"""
    from tests.test_temporal import run as run1
    src0, cur0, src1, cur1 = case(shape)
    for i, kw in enumerate(COMBOS[::3]):
        kw = dict(kw, R=RADII[i % 3])
        kind = i % 3
        first = lib_call(eng, src0[kind], cur0[kind], None, 1, **kw)
        assert equal1(first, temporal_ref(src0[kind], cur0[kind], **kw)) and equal1(first, run1(eng, src0[kind], cur0[kind], **device_kw(**kw)))
        prev = (first["luma"], first["out88"])
        second = lib_call(eng, src1[kind], cur1[kind], prev, 1, **kw)
        assert equal1(second, temporal_ref(src1[kind], cur1[kind], prev=prev, **kw)), kw
        assert equal1(second, run1(eng, src1[kind], cur1[kind], prev=prev, **device_kw(**kw))), kw


@pytest.mark.parametrize("levels", [2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_two_frames_match_the_restatement(eng, shape, levels):
    """Both matrices, both channel orders and every radius, the nine pairs of sensitivity and strength going round; every data kind; a first
    frame (no previous state) and a second one fed with the first one's state.  The odd sizes clamp the pyramid's edge, and the small ones
    have a coarsest level of one ragged block."""
    src0, cur0, src1, cur1 = case(shape)
    for i, kw in enumerate(COMBOS):
        kind = i % 3
        first = run(eng, src0[kind], cur0[kind], levels=levels, **device_kw(**kw))
        assert equal(first, pyr_ref(src0[kind], cur0[kind], levels=levels, **kw)), ("first", kw)
        assert not first["mv"].any() and not any(v.any() for v in first["vs"])
        second = run(eng, src1[kind], cur1[kind], prev=state_of(first), levels=levels, **device_kw(**kw))
        assert equal(second, pyr_ref(src1[kind], cur1[kind], prev=state_of(first), levels=levels, **kw)), ("second", kw)
        if kw["R"] == 0:
            assert not second["mv"].any() and not any(v.any() for v in second["vs"])


def run_lumas(eng, cur8, prev8, levels, prev88=None, cur=None, **kw):
    """A grey frame of luma cur8 against the state of a grey frame of luma prev8"""
    Ho, Wo = cur8.shape
    prev = (prev8, ZERO88(Ho, Wo) if prev88 is None else prev88, pyramid(prev8, levels)[1:])
    got = run(eng, grey(cur8), grey(cur8) if cur is None else cur, prev=prev, levels=levels, **device_kw(**kw))
    assert np.array_equal(got["luma"], cur8)
    return got, prev


def test_known_moves_on_the_device(eng):
    for (Ho, Wo), (dy, dx), levels in (((96, 128), (28, -28), 3), ((48, 64), (12, 0), 2)):
        a, moved = moved_pair(Ho, Wo, dy, dx, 1)
        inside = interior(Ho, Wo, dy, dx)
        got, prev = run_lumas(eng, moved, a, levels)
        want = search_pyr(pyramid(moved, levels), pyramid(a, levels), 7)
        assert all(want[0][b].tolist() == [dy, dx] for b in inside) and all(got["mv"][b].tolist() == [dy, dx] for b in inside)
        assert np.array_equal(got["mv"], want[0]) and all(np.array_equal(g, w) for g, w in zip(got["vs"], want[1:]))
        one = run(eng, grey(moved), grey(moved), prev=(a, ZERO88(Ho, Wo), []), levels=1, **device_kw())
        assert np.array_equal(one["mv"], search(moved, a, 7)) and not any(one["mv"][b].tolist() == [dy, dx] for b in inside)
    # identical frames: at rest on every level
    a = np.random.RandomState(4).randint(0, 256, (48, 64)).astype(np.uint8)
    for levels in (2, 3):
        assert not any(v.any() for v in search_pyr(pyramid(a, levels), pyramid(a, levels), 7))
        got, _ = run_lumas(eng, a, a, levels)
        assert not got["mv"].any() and not any(v.any() for v in got["vs"])


def test_an_odd_move_is_mostly_found(eng):
    """(-21, 21) at three levels on 96 x 128: the halved lumas do not line up; the restatement finds at least half of the interior blocks, how
    many depends on the seed, and the device equals it."""
    a, moved = moved_pair(96, 128, -21, 21, 2)
    inside = interior(96, 128, -21, 21)
    want = search_pyr(pyramid(moved, 3), pyramid(a, 3), 7)
    assert 2 * sum(want[0][b].tolist() == [-21, 21] for b in inside) >= len(inside)
    got, _ = run_lumas(eng, moved, a, 3)
    assert np.array_equal(got["mv"], want[0]) and all(np.array_equal(g, w) for g, w in zip(got["vs"], want[1:]))


def test_full_strength_fetches_the_previous_output_along_the_vector(eng):
    """Strength 256 with sensitivity 256 on a moved pair: out88 == prev88[q] on the interior blocks"""
    for (Ho, Wo), (dy, dx), levels in (((48, 64), (12, 0), 2), ((96, 128), (28, -28), 3)):
        a, moved = moved_pair(Ho, Wo, dy, dx, 3)
        p88 = np.random.RandomState(6).randint(0, 65281, (Ho, Wo, 3)).astype(np.uint16)
        inside = interior(Ho, Wo, dy, dx)
        want = pyr_ref(grey(moved), np.zeros((Ho, Wo, 3), np.float32), prev=(a, p88, pyramid(a, levels)[1:]), levels=levels, q8=256, K=256)
        got, _ = run_lumas(eng, moved, a, levels, prev88=p88, cur=np.zeros((Ho, Wo, 3), np.float32), q8=256, K=256)
        assert equal(got, want)
        for res in (want, got):
            for by, bx in inside:
                y, x = by * 16, bx * 16
                assert np.array_equal(res["out88"][y:y + 16, x:x + 16], p88[y + dy:y + dy + 16, x + dx:x + dx + 16])


@pytest.mark.parametrize("shift", [(-12, -12), (12, 12), (-12, 12), (12, -12)], ids=lambda s: "dy%d_dx%d" % s)
def test_vectors_that_point_out_of_the_frame_follow_the_clamp(eng, shift):
    """cur8[y][x] = prev8[clampy(y + dy)][clampx(x + dx)] by construction, beyond the reach of one level; 56 x 68 has ragged blocks on the
    right and at the bottom on both levels.  Block (1, 1), where nothing clamps, yields the vector; everything equals the restatement,
    which clamps every displaced coordinate into its level, and some vectors do point out of the frame."""
    Ho, Wo = 56, 68
    dy, dx = shift
    p8 = np.random.RandomState(22).randint(0, 256, (Ho, Wo)).astype(np.uint8)
    c8 = p8[np.clip(np.arange(Ho) + dy, 0, Ho - 1)][:, np.clip(np.arange(Wo) + dx, 0, Wo - 1)]
    want = search_pyr(pyramid(c8, 2), pyramid(p8, 2), 7)
    assert want[0][1, 1].tolist() == [dy, dx]                   # rows 16 .. 31, columns 16 .. 31
    got, _ = run_lumas(eng, c8, p8, 2)
    assert np.array_equal(got["mv"], want[0]) and np.array_equal(got["vs"][0], want[1])
    y, x = np.indices((Ho, Wo))
    q = np.stack([y, x], axis=-1) + got["mv"].astype(np.int64)[y >> 4, x >> 4]
    assert ((q[..., 0] < 0) | (q[..., 0] >= Ho)).any() and ((q[..., 1] < 0) | (q[..., 1] >= Wo)).any()


@pytest.mark.parametrize("levels", [2, 3])
def test_the_destination_may_be_the_current_tensor(eng, levels):
    for shape in ((14, 30, 17, 33), (33, 47, 33, 47)):
        src0, cur0, src1, cur1 = case(shape)
        Ho, Wo = shape[2:]
        prev = (luma8(src0[0], Ho, Wo), to88(cur0[0]).astype(np.uint16), pyramid(luma8(src0[0], Ho, Wo), levels)[1:])
        for kw in (dict(q8=77, K=1), dict(q8=256, K=16, R=3, matrix=1, bgr=True)):
            got = run(eng, src1[0], cur1[0], prev=prev, levels=levels, alias=True, **device_kw(**kw))
            assert equal(got, pyr_ref(src1[0], cur1[0], prev=prev, levels=levels, **kw)), kw


def test_tensors_and_state_off_sixteen_byte_alignment_give_the_same_values(eng):
    shape = (33, 47, 33, 47)
    src0, cur0, src1, cur1 = case(shape)
    c8 = luma8(src0[0], 33, 47)
    prev = (c8, to88(cur0[0]).astype(np.uint16), pyramid(c8, 3)[1:])
    want = pyr_ref(src1[0], cur1[0], prev=prev, levels=3, q8=128, K=16)
    for off, soff, poff in (((1, 0, 0), 0, 0), ((0, 1, 0), 0, 1), ((0, 0, 1), 0, 7), ((0, 0, 0), 2, 2), ((3, 2, 1), 6, 13)):   # (out88 is u16: soff is even)
        assert equal(run(eng, src1[0], cur1[0], prev=prev, levels=3, off=off, soff=soff, poff=poff, **device_kw(q8=128, K=16)), want), (off, soff, poff)


def test_engine_pyramid_readback(eng):
    """Engine.temporal_state / temporal_f32 / temporal_pyramid on the engine's own buffers, two frames"""
    shape = (33, 47, 33, 47)
    src0, cur0, src1, cur1 = case(shape)
    mem = eng.mem
    for levels in (2, 3):
        slots = [eng.temporal_state(33, 47, levels) for _ in range(2)]
        d = mem.empty((33, 47, 3))
        eng.temporal_f32(mem.from_numpy(src0[0]), mem.from_numpy(cur0[0]), d, slots[0], levels=levels)
        first = pyr_ref(src0[0], cur0[0], levels=levels)
        eng.temporal_f32(mem.from_numpy(src1[0]), mem.from_numpy(cur1[0]), d, slots[1], prev=slots[0], levels=levels)
        second = pyr_ref(src1[0], cur1[0], prev=state_of(first), levels=levels)
        assert same(np.asarray(mem.to_numpy(d)), second["dst"])
        for slot, want in ((slots[0], first), (slots[1], second)):
            lumas, vs = eng.temporal_pyramid(slot, 33, 47, levels)
            assert len(lumas) == levels - 1 and all(np.array_equal(a, b) for a, b in zip(lumas, want["lumas"]))
            assert all(a.dtype == np.int8 and np.array_equal(a, b) for a, b in zip(vs, want["vs"]))
        assert eng.temporal_pyramid(eng.temporal_state(33, 47), 33, 47, 1) == ([], [])
        with pytest.raises(L.FaststyleError):
            eng.temporal_pyramid(slots[0][:3], 33, 47, levels)


def test_refused_calls_return_their_code_and_launch_nothing(eng):
    mem, lib, ctx = eng.mem, eng.lib, eng.ctx
    H, W, Ho, Wo, levels = 14, 30, 17, 33, 3
    src0, cur0, src1, cur1 = case((H, W, Ho, Wo))
    _, s, _ = placed(eng, src1[0], 0, 0)
    _, c, _ = placed(eng, cur1[0], 0, 0)
    dbuf, d, d0 = placed(eng, np.full(cur1[0].shape, SENTINEL, np.float32), 0, GUARD)
    state, spyr = slot_buffers(eng, Ho, Wo), pyr_buffer(eng, Ho, Wo, levels)
    c8 = luma8(src0[0], Ho, Wo)
    prevh = (c8, to88(cur0[0]).astype(np.uint16), pyramid(c8, levels)[1:])
    before, bpyr = slot_buffers(eng, Ho, Wo, fill=prevh[:2]), pyr_buffer(eng, Ho, Wo, levels, prevh[2])
    for _, view, _ in state + [spyr]:                           # (so that a launch of any of the kernels would show)
        if hasattr(view, "fill_"):
            view.fill_(FILL)
        else:
            view[...] = FILL
    ps, pc, pd = mem.ptr(s), mem.ptr(c), mem.ptr(d)
    pl, po, pm = (mem.ptr_u8(b[1]) for b in state)
    pp, qp = mem.ptr_u8(spyr[1]), mem.ptr_u8(bpyr[1])
    ql, qo = mem.ptr_u8(before[0][1]), mem.ptr_u8(before[1][1])
    eng._sync_stream()

    def call(src=ps, H=H, W=W, cur=pc, Ho=Ho, Wo=Wo, q8=128, K=16, R=7, levels=levels, matrix=0, bgr=0, prev_luma=ql, prev_out88=qo, prev_pyr=qp,
             luma=pl, out88=po, pyr=pp, mv=pm, dst=pd):
        return lib.fs_temporal_pyr_f32(ctx, src, H, W, cur, Ho, Wo, q8, K, R, levels, matrix, bgr, prev_luma, prev_out88, prev_pyr, luma, out88, pyr,
                                       mv, dst)

    refused = [(-1, dict(src=None)), (-1, dict(cur=None)), (-1, dict(luma=None)), (-1, dict(out88=None)), (-1, dict(mv=None)), (-1, dict(dst=None)),
               (-1, dict(prev_luma=None)), (-1, dict(prev_out88=None)), (-1, dict(prev_luma=pl)), (-1, dict(prev_out88=po)),
               (-1, dict(H=0)), (-1, dict(W=0)), (-1, dict(H=-3)), (-1, dict(Ho=H - 1)), (-1, dict(Ho=H + 4)), (-1, dict(Wo=W - 1)),
               (-1, dict(Wo=W + 4)), (-1, dict(H=2 ** 31 - 1)),
               (-2, dict(q8=-1)), (-2, dict(q8=257)), (-2, dict(K=0)), (-2, dict(K=257)), (-2, dict(R=-1)), (-2, dict(R=8)), (-2, dict(matrix=2)),
               (-2, dict(matrix=-1)), (-2, dict(bgr=2)), (-2, dict(bgr=-1)),
               (-5, dict(src=ps + 2)), (-5, dict(cur=pc + 1)), (-5, dict(dst=pd + 3)), (-5, dict(out88=po + 1)), (-5, dict(prev_out88=qo + 1)),
               (-2, dict(levels=0)), (-2, dict(levels=4)), (-2, dict(levels=-1)),
               (-1, dict(pyr=None)), (-1, dict(pyr=None, levels=2)), (-1, dict(prev_pyr=None)),
               (-1, dict(prev_luma=None, prev_out88=None)), (-1, dict(prev_pyr=pp)), (-1, dict(pyr=qp))]
    for code, kw in refused:
        assert call(**kw) == code, kw
        assert b"fs_temporal_pyr_f32" in lib.fs_last_error()
    assert lib.fs_temporal_pyr_f32(None, ps, H, W, pc, Ho, Wo, 128, 16, 7, levels, 0, 0, ql, qo, qp, pl, po, pp, pm, pd) == -1
    assert np.all(np.asarray(mem.to_numpy(dbuf)) == SENTINEL)                                 # nothing was launched
    assert all(np.all(np.asarray(mem.to_numpy(b[0])) == FILL) for b in state + [spyr])
    # the call they were variations of is taken, with and without a previous frame
    assert call() == 0
    got = np.asarray(mem.to_numpy(dbuf)).reshape(-1)[d0:d0 + cur1[0].size].reshape(cur1[0].shape)
    want = pyr_ref(src1[0], cur1[0], prev=prevh, levels=levels, q8=128)
    luma, out88, mv = read_slot(eng, state, Ho, Wo)
    lumas, vs = read_pyr(eng, spyr, Ho, Wo, levels)
    assert equal(dict(luma=luma, mv=mv, out88=out88, dst=got, lumas=lumas, vs=vs), want)
    assert call(prev_luma=None, prev_out88=None, prev_pyr=None) == 0
    assert np.array_equal(read_slot(eng, state, Ho, Wo)[1], to88(cur1[0]))
    # the engine checks the shapes against each other and the fourth buffer against the layout; one level keeps its own refusals
    views = tuple(b[1] for b in state) + (spyr[1],)
    for bad in (dict(cur=s), dict(state=eng.temporal_state(Ho, Wo - 1, levels)), dict(prev=eng.temporal_state(Ho, Wo - 1, levels)),
                dict(state=views[:3]), dict(state=eng.temporal_state(Ho, Wo, 2)), dict(prev=eng.temporal_state(Ho, Wo, 2)), dict(levels=0),
                dict(levels=4), dict(levels=2.5)):
        a = dict(dict(src=s, cur=c, dst=d, state=views, prev=None, levels=levels), **bad)
        with pytest.raises(L.FaststyleError):
            eng.temporal_f32(a["src"], a["cur"], a["dst"], a["state"], prev=a["prev"], levels=a["levels"])
    for lv in (1, 2):
        with pytest.raises(L.FaststyleError):
            eng.temporal_f32(s, c, d, views[:3] if lv == 1 else eng.temporal_state(Ho, Wo, 2), radius=8, levels=lv)
