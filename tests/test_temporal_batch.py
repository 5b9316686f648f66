"""Batches of consecutive frames in the temporal stage (csrc/fs_temporal.hip: fs_temporal_batch_f32) against the contract in
include/faststyle_io.h: one call over N frames writes bit for bit what N chained single-frame calls write -- every frame's stabilised tensor
and vectors, and the state the last frame leaves.  The chain runs on the same engine (Engine.temporal_f32) and, in one case, in the numpy
restatement of tests/test_temporal_obmc.py, which shows that the chain itself is the contract.  Every comparison is equality.  The frames
are the moving-apart noise of tests/test_temporal_obmc_stream.py, so that the four-candidate blend runs.  The same bodies run on the CPU
emulator and, under -m gpu, on the MI355X."""
import ctypes

import numpy as np
import pytest

from faststyle_amd import _lib as L
from tests import backends
from tests.test_compose import GUARD, SENTINEL, f32_of_F, placed, same, to88
from tests.test_temporal import FILL, blocks_of, case, device_kw, luma8, read_slot, slot_buffers
from tests.test_temporal_obmc import masks, obmc_ref, state_of
from tests.test_temporal_obmc import run as run_single
from tests.test_temporal_obmc_stream import sequence
from tests.test_temporal_pyr import SHAPES as PYR_SHAPES
from tests.test_temporal_pyr import ids, pyr_buffer, pyramid, read_pyr
from tests.test_temporal_sub import MVF_FILL, mvf_buffer, read_mvf


@pytest.fixture(params=backends.engine_params())
def eng(request):
    return backends.get_engine(request.param)


WORK_FILL = 0xA7                                                # what the work buffer holds before a call
FRAMES = [1, 2, 3, 5]                                           # 2: one intermediate frame; 3: the out88 pair wraps; 5: odd
MODES = [(1, 0, 0), (1, 0, 1), (2, 2, 0), (3, 2, 1)]            # levels, subpel, overlap
SHAPES = [(1, 1, 4, 4), (16, 16, 16, 16), (14, 30, 17, 33), (64, 48, 64, 48)]     # H, W, Ho, Wo
CASES = [(m, s) for m in MODES for s in (PYR_SHAPES if m[0] == 3 else SHAPES)]
_streams = {}


def stream_of(shape):
    """Seven consecutive frames of one shape, built once and read-only: (src float32 [7,H,W,3], cur float32 [6,Ho,Wo,3]) -- the sources are
    noise whose halves move apart (tests.test_temporal_obmc_stream.sequence), the current tensors tests.test_temporal.case's (NaN, infinities
    and values off the scale among them)"""
    if shape not in _streams:
        H, W, Ho, Wo = shape
        src = np.stack(sequence(H, W, 3 + H, 7)).astype(np.float32)
        c = case(shape)
        cur = np.concatenate([c[1], c[3]]).astype(np.float32)
        for a in (src, cur):
            a.setflags(write=False)
        _streams[shape] = (src, cur)
    return _streams[shape]


def run_batch(eng, src, cur, prev=None, levels=1, subpel=0, overlap=0, alias=False, off=(0, 0, 0), soff=0, woff=0, **kw):
    """eng.temporal_batch_f32 on host arrays src [N,H,W,3], cur [N,Ho,Wo,3] -> tests.test_temporal_obmc.run's dict for the last frame's state,
    dst [N,Ho,Wo,3], and mvs / mvfs: every frame's vectors.  off: floats past a 16-byte boundary of src, cur, dst; soff: bytes of the state
    buffers; woff: bytes of the work buffer (a multiple of 16).  Every output and the work buffer, which has exactly the layout's size, lie
    between guards that must come back untouched; the previous state is read only."""
    mem = eng.mem
    N, Ho, Wo = cur.shape[:3]
    _, s, _ = placed(eng, src, off[0], 0)
    cbuf, c, c0 = placed(eng, cur, off[1], GUARD)
    dbuf, d, d0 = (cbuf, c, c0) if alias else placed(eng, np.full(cur.shape, SENTINEL, np.float32), off[2], GUARD)
    state, spyr = slot_buffers(eng, Ho, Wo, off=soff), pyr_buffer(eng, Ho, Wo, levels, off=soff) if levels > 1 else None
    smvf = mvf_buffer(eng, Ho, Wo, soff) if subpel else None
    tail = lambda pyr, mvf: ((pyr[1],) if levels > 1 else ()) + ((mvf[1],) if subpel else ())
    before = bpyr = bmvf = pslot = None
    if prev is not None:
        before = slot_buffers(eng, Ho, Wo, fill=prev[:2], off=soff)
        bpyr = pyr_buffer(eng, Ho, Wo, levels, prev[2], off=soff) if levels > 1 else None
        bmvf = mvf_buffer(eng, Ho, Wo, soff) if subpel else None
        pslot = tuple(b[1] for b in before) + tail(bpyr, bmvf)
    need = int(eng.temporal_batch_layout(Ho, Wo, N, levels, subpel).work_bytes)
    assert (need == 0) == (N == 1)
    work = placed(eng, np.full(need, WORK_FILL, np.uint8), woff, GUARD, u8=True) if N > 1 else None
    slot = tuple(b[1] for b in state) + tail(spyr, smvf)
    eng.temporal_batch_f32(s, c, d, slot, None if work is None else work[1], prev=pslot, levels=levels, subpel=subpel, overlap=overlap, **kw)
    whole = np.array(mem.to_numpy(dbuf), copy=True).reshape(-1)
    assert np.all(whole[:d0] == SENTINEL) and np.all(whole[d0 + cur.size:] == SENTINEL), "a write outside the destination"
    if work is not None:
        w = np.array(mem.to_numpy(work[0]), copy=True).reshape(-1)
        assert np.all(w[:work[2]] == FILL) and np.all(w[work[2] + need:] == FILL), "a write outside the work buffer"
    luma, out88, mv = read_slot(eng, state, Ho, Wo)
    lumas, vs = read_pyr(eng, spyr, Ho, Wo, levels) if levels > 1 else ([], [])
    if prev is not None:
        pl, po, _ = read_slot(eng, before, Ho, Wo)
        assert np.array_equal(pl, prev[0]) and np.array_equal(po, prev[1])
        assert levels == 1 or all(np.array_equal(a, b) for a, b in zip(read_pyr(eng, bpyr, Ho, Wo, levels)[0], prev[2]))
        assert not subpel or np.all(read_mvf(eng, bmvf, Ho, Wo).view(np.uint8) == MVF_FILL)
    mvs, mvfs = eng.temporal_batch_vectors(None if work is None else work[1], slot, Ho, Wo, N, levels, subpel)
    assert mvs.dtype == np.int8 and mvs.shape == (N,) + blocks_of(Ho, Wo) + (2,) and (mvfs is None) == (subpel == 0)
    return dict(luma=luma, mv=mv, mvf=read_mvf(eng, smvf, Ho, Wo) if subpel else None, out88=out88,
                dst=whole[d0:d0 + cur.size].reshape(cur.shape), lumas=lumas, vs=vs, mvs=mvs, mvfs=mvfs)


def chain(eng, src, cur, prev=None, **kw):
    """The same frames through chained single-frame calls of the same engine -> one tests.test_temporal_obmc.run dict per frame"""
    outs = []
    for s, c in zip(src, cur):
        outs.append(run_single(eng, s, c, prev=prev, **kw))
        prev = state_of(outs[-1])
    return outs


def equal_chain(got, outs):
    """The batch's dict against the chain's: every frame's tensor and vectors, and the last frame's state"""
    last = outs[-1]
    return all(same(got["dst"][i], o["dst"]) and np.array_equal(got["mvs"][i], o["mv"]) and
               (o["mvf"] is None or np.array_equal(got["mvfs"][i], o["mvf"])) for i, o in enumerate(outs)) and \
        all(np.array_equal(got[k], last[k]) for k in ("luma", "mv", "out88")) and (last["mvf"] is None or np.array_equal(got["mvf"], last["mvf"])) and \
        len(got["lumas"]) == len(last["lumas"]) and all(np.array_equal(a, b) for a, b in zip(got["lumas"], last["lumas"])) and \
        all(np.array_equal(a, b) for a, b in zip(got["vs"], last["vs"]))


# ================================================================ the layout (host only)
def test_the_layout_is_monotone_and_holds_two_out88_frames(eng):
    for (Ho, Wo), levels, subpel in (((64, 48), 1, 0), ((48, 64), 2, 2), ((720, 1280), 3, 2), ((1080, 1920), 3, 0), ((45, 62), 3, 1)):
        lays = [eng.temporal_batch_layout(Ho, Wo, n, levels, subpel) for n in range(1, 65)]
        sizes = [int(l.work_bytes) for l in lays]
        assert sizes[0] == 0 and all(b > a for a, b in zip(sizes, sizes[1:]))
        assert all(l.frames == n + 1 and l.levels == levels and l.subpel == subpel and l.reserved == 0 for n, l in enumerate(lays))
        steps = {b - a for a, b in zip(sizes[2:], sizes[3:])}                                   # per extra frame beyond 3: no out88 frame
        assert len(steps) == 1 and 0 < steps.pop() < 6 * Ho * Wo
        assert sizes[2] - sizes[1] >= 6 * Ho * Wo and sizes[1] >= 6 * Ho * Wo                   # (the two that there are)
        nblk = 2 * int(np.prod(blocks_of(Ho, Wo)))
        for n, l in enumerate(lays[1:], 2):
            assert l.mv_offset % 16 == 0 and l.mv_stride % 16 == 0 and l.mv_stride >= Ho * Wo + nblk
            assert l.mv_offset + (n - 2) * l.mv_stride + nblk <= l.work_bytes
            if subpel:
                assert l.mvf_stride == l.mv_stride and l.mvf_offset >= l.mv_offset + nblk and l.mvf_offset + (n - 2) * l.mvf_stride + nblk <= l.work_bytes
            else:
                assert l.mvf_offset == 0 and l.mvf_stride == 0
    info = L.fs_temporal_batch_info()
    assert ctypes.sizeof(info) == 56
    for code, a in ((-1, (0, 8, 1, 0, 2)), (-1, (8, 0, 1, 0, 2)), (-1, (8, 8, 1, 0, 0)), (-1, (8, 8, 1, 0, 65)), (-2, (8, 8, 0, 0, 2)),
                    (-2, (8, 8, 4, 0, 2)), (-2, (8, 8, 1, 3, 2)), (-2, (8, 8, 1, -1, 2))):
        assert eng.lib.fs_temporal_batch_layout(*a, ctypes.byref(info)) == code and b"fs_temporal_batch_layout" in eng.lib.fs_last_error()
    assert eng.lib.fs_temporal_batch_layout(8, 8, 1, 0, 2, None) == -1


# ================================================================ the batch against chained single-frame calls
@pytest.mark.parametrize("frames", FRAMES)
@pytest.mark.parametrize("mode,shape", CASES, ids=lambda v: "x".join(map(str, v)) if len(v) == 4 else "L%dS%dO%d" % v)
def test_a_batch_is_the_chain_of_single_frame_calls(eng, mode, shape, frames):
    """Without a previous frame, then fed the state that call left: a first frame affects frame 0 alone"""
    levels, subpel, overlap = mode
    src, cur = stream_of(shape)
    kw = dict(levels=levels, subpel=subpel, overlap=overlap, **device_kw(q8=154, K=4, matrix=1))
    got = run_batch(eng, src[:frames], cur[:frames], **kw)
    outs = chain(eng, src[:frames], cur[:frames], **kw)
    assert equal_chain(got, outs)
    assert not got["mvs"][0].any() and same(got["dst"][0], f32_of_F(to88(cur[0])))              # frame 0 had no previous frame: F = B
    if frames > 1 and shape[:2] >= (33, 47):                                                    # ... and frame 1 had one
        assert got["mvs"][1].any() and not same(got["dst"][1], f32_of_F(to88(cur[1])))
    prev = state_of(outs[-1])
    got = run_batch(eng, src[2:2 + frames], cur[1:1 + frames], prev=prev, **kw)
    assert equal_chain(got, chain(eng, src[2:2 + frames], cur[1:1 + frames], prev=prev, **kw))


def test_the_chain_is_the_restatement_and_the_four_candidate_blend_runs(eng):
    """Three frames against tests.test_temporal_obmc.obmc_ref chained in numpy, with a previous state in front"""
    shape, levels, subpel = (64, 48, 64, 48), 2, 2
    src, cur = stream_of(shape)
    c8 = luma8(src[0], 64, 48, 1)
    prev = (c8, to88(cur[5]).astype(np.uint16), pyramid(c8, levels)[1:])
    got = run_batch(eng, src[1:4], cur[:3], prev=prev, levels=levels, subpel=subpel, overlap=1, **device_kw(q8=200, K=8, matrix=1))
    mixed = 0
    for i in range(3):
        want = obmc_ref(src[1 + i], cur[i], prev=prev, levels=levels, subpel=subpel, q8=200, K=8, matrix=1)
        assert same(got["dst"][i], want["dst"]) and np.array_equal(got["mvs"][i], want["mv"]) and np.array_equal(got["mvfs"][i], want["mvf"])
        mixed += int(np.count_nonzero(~masks(want)[0] & (want["info"]["D"] > 0)))
        prev = (want["luma"], want["out88"], want["lumas"])
    assert mixed                                                                                # (pixels blended along more than one vector)
    assert all(np.array_equal(got[k], want[k]) for k in ("luma", "mv", "mvf", "out88"))
    assert all(np.array_equal(a, b) for a, b in zip(got["lumas"], want["lumas"])) and all(np.array_equal(a, b) for a, b in zip(got["vs"], want["vs"]))


@pytest.mark.parametrize("mode", MODES[1:], ids=lambda v: "L%dS%dO%d" % v)
def test_the_destination_may_be_the_current_tensor(eng, mode):
    levels, subpel, overlap = mode
    src, cur = stream_of((14, 30, 17, 33))
    kw = dict(levels=levels, subpel=subpel, overlap=overlap, **device_kw(q8=128))
    a, b = run_batch(eng, src[:3], cur[:3], **kw), run_batch(eng, src[:3], cur[:3], alias=True, **kw)
    assert same(a["dst"], b["dst"]) and all(np.array_equal(a[k], b[k]) for k in ("luma", "mv", "out88", "mvs"))


def test_buffers_off_their_alignment_give_the_same_values(eng):
    """Tensors off 16 bytes, the state off by odd byte counts (out88 by even ones), the work buffer 16, 32 and 48 bytes further"""
    src, cur = stream_of((14, 30, 17, 33))
    kw = dict(levels=3, subpel=2, overlap=1, **device_kw(q8=200))
    first = run_batch(eng, src[:2], cur[:2], **kw)
    prev = state_of(first)
    want = run_batch(eng, src[2:5], cur[2:5], prev=prev, **kw)
    for off, soff, woff in (((1, 2, 3), 2, 16), ((3, 1, 2), 6, 32), ((2, 3, 1), 10, 48)):
        got = run_batch(eng, src[2:5], cur[2:5], prev=prev, off=off, soff=soff, woff=woff, **kw)
        assert same(got["dst"], want["dst"]) and all(np.array_equal(got[k], want[k]) for k in ("luma", "mv", "mvf", "out88", "mvs", "mvfs"))
        assert all(np.array_equal(a, b) for a, b in zip(got["lumas"] + got["vs"], want["lumas"] + want["vs"]))


# ================================================================ refusals
def test_refused_calls_return_their_code_and_launch_nothing(eng):
    mem, lib, ctx = eng.mem, eng.lib, eng.ctx
    H, W, Ho, Wo, levels, N = 14, 30, 17, 33, 3, 3
    src, cur = stream_of((H, W, Ho, Wo))
    _, s, _ = placed(eng, src[1:1 + N], 0, 0)
    _, c, _ = placed(eng, cur[:N], 0, 0)
    dbuf, d, d0 = placed(eng, np.full(cur[:N].shape, SENTINEL, np.float32), 0, GUARD)
    state, spyr, smvf = slot_buffers(eng, Ho, Wo), pyr_buffer(eng, Ho, Wo, levels), mvf_buffer(eng, Ho, Wo)
    c8 = luma8(src[0], Ho, Wo)
    prevh = (c8, to88(cur[5]).astype(np.uint16), pyramid(c8, levels)[1:])
    before, bpyr = slot_buffers(eng, Ho, Wo, fill=prevh[:2]), pyr_buffer(eng, Ho, Wo, levels, prevh[2])
    need = int(eng.temporal_batch_layout(Ho, Wo, N, levels, 2).work_bytes)
    work = placed(eng, np.full(need, FILL, np.uint8), 0, GUARD, u8=True)
    for _, view, _ in state + [spyr, smvf]:                     # (so that a launch of any of the kernels would show)
        if hasattr(view, "fill_"):
            view.fill_(FILL)
        else:
            view[...] = FILL
    ps, pc, pd = mem.ptr(s), mem.ptr(c), mem.ptr(d)
    pl, po, pm = (mem.ptr_u8(b[1]) for b in state)
    pp, qp, pf, pw = mem.ptr_u8(spyr[1]), mem.ptr_u8(bpyr[1]), mem.ptr_u8(smvf[1]), mem.ptr_u8(work[1])
    ql, qo = mem.ptr_u8(before[0][1]), mem.ptr_u8(before[1][1])
    eng._sync_stream()

    def call(src=ps, H=H, W=W, cur=pc, Ho=Ho, Wo=Wo, frames=N, q8=128, K=16, R=7, levels=levels, subpel=2, overlap=1, matrix=0, bgr=0, prev_luma=ql,
             prev_out88=qo, prev_pyr=qp, luma=pl, out88=po, pyr=pp, mv=pm, mvf=pf, work=pw, work_bytes=need, dst=pd):
        return lib.fs_temporal_batch_f32(ctx, src, H, W, cur, Ho, Wo, frames, q8, K, R, levels, subpel, overlap, matrix, bgr, prev_luma, prev_out88,
                                         prev_pyr, luma, out88, pyr, mv, mvf, work, work_bytes, dst)

    refused = [(-1, dict(src=None)), (-1, dict(cur=None)), (-1, dict(luma=None)), (-1, dict(out88=None)), (-1, dict(mv=None)), (-1, dict(dst=None)),
               (-1, dict(prev_luma=None)), (-1, dict(prev_out88=None)), (-1, dict(prev_luma=pl)), (-1, dict(prev_out88=po)),
               (-1, dict(H=0)), (-1, dict(W=0)), (-1, dict(H=-3)), (-1, dict(Ho=H - 1)), (-1, dict(Ho=H + 4)), (-1, dict(Wo=W - 1)),
               (-1, dict(Wo=W + 4)), (-1, dict(H=2 ** 31 - 1)),
               (-2, dict(q8=-1)), (-2, dict(q8=257)), (-2, dict(K=0)), (-2, dict(K=257)), (-2, dict(R=-1)), (-2, dict(R=8)), (-2, dict(matrix=2)),
               (-2, dict(matrix=-1)), (-2, dict(bgr=2)), (-2, dict(bgr=-1)),
               (-5, dict(src=ps + 2)), (-5, dict(cur=pc + 1)), (-5, dict(dst=pd + 3)), (-5, dict(out88=po + 1)), (-5, dict(prev_out88=qo + 1)),
               (-2, dict(levels=0)), (-2, dict(levels=4)), (-1, dict(pyr=None)), (-1, dict(prev_pyr=None)),
               (-1, dict(prev_luma=None, prev_out88=None)), (-1, dict(prev_pyr=pp)), (-1, dict(pyr=qp)),
               (-2, dict(subpel=-1)), (-2, dict(subpel=3)), (-1, dict(mvf=None)), (-2, dict(overlap=2)), (-2, dict(overlap=-1)),
               (-1, dict(frames=0)), (-1, dict(frames=-1)), (-1, dict(frames=65)), (-1, dict(work=None)), (-1, dict(work_bytes=need - 1)),
               (-1, dict(work_bytes=0)), (-1, dict(frames=N + 1)), (-5, dict(work=pw + 8)), (-5, dict(work=pw + 1)),
               (-1, dict(frames=1, work=None, work_bytes=0, src=None))]
    for code, kw in refused:
        assert call(**kw) == code, kw
        assert b"fs_temporal_batch_f32" in lib.fs_last_error()
    assert lib.fs_temporal_batch_f32(None, ps, H, W, pc, Ho, Wo, N, 128, 16, 7, levels, 2, 1, 0, 0, ql, qo, qp, pl, po, pp, pm, pf, pw, need, pd) == -1
    assert np.all(np.asarray(mem.to_numpy(dbuf)) == SENTINEL)                                 # nothing was launched
    assert all(np.all(np.asarray(mem.to_numpy(b[0])) == FILL) for b in state + [spyr, smvf, work])
    # the call they were variations of is taken, and so is one frame without a work buffer
    assert call() == 0
    got = np.asarray(mem.to_numpy(dbuf)).reshape(-1)[d0:d0 + cur[:N].size].reshape(cur[:N].shape)
    prev = prevh
    for i in range(N):
        want = obmc_ref(src[1 + i], cur[i], prev=prev, levels=levels, subpel=2, q8=128)
        assert same(got[i], want["dst"])
        prev = (want["luma"], want["out88"], want["lumas"])
    assert np.array_equal(read_slot(eng, state, Ho, Wo)[1], want["out88"]) and np.array_equal(read_mvf(eng, smvf, Ho, Wo), want["mvf"])
    assert call(frames=1, work=None, work_bytes=0) == 0
    assert np.array_equal(read_slot(eng, state, Ho, Wo)[1], obmc_ref(src[1], cur[0], prev=prevh, levels=levels, subpel=2, q8=128)["out88"])
    # the engine checks the shapes against each other, against the slots and against the work buffer
    views = tuple(b[1] for b in state) + (spyr[1], smvf[1])
    short = eng.temporal_batch_work(Ho, Wo, N - 1, levels, 2)
    for bad in (dict(cur=s), dict(src=mem.view(s, 0, (N - 1, H, W, 3))), dict(dst=mem.view(d, 0, (N - 1, Ho, Wo, 3))),
                dict(src=mem.view(s, 0, (H, W, 3)), cur=mem.view(c, 0, (Ho, Wo, 3)), dst=mem.view(d, 0, (Ho, Wo, 3))),
                dict(state=eng.temporal_state(Ho, Wo - 1, levels, 2)), dict(prev=eng.temporal_state(Ho, Wo - 1, levels, 2)), dict(state=views[:4]),
                dict(state=eng.temporal_state(Ho, Wo, 2, 2)), dict(prev=eng.temporal_state(Ho, Wo, levels)), dict(work=short), dict(work=None),
                dict(levels=0), dict(levels=4), dict(subpel=3), dict(subpel=1.5), dict(overlap=2), dict(overlap=True)):
        a = dict(dict(src=s, cur=c, dst=d, state=views, work=work[1], prev=None, levels=levels, subpel=2, overlap=1), **bad)
        with pytest.raises(L.FaststyleError):
            eng.temporal_batch_f32(a["src"], a["cur"], a["dst"], a["state"], a["work"], prev=a["prev"], levels=a["levels"], subpel=a["subpel"],
                                   overlap=a["overlap"])
    with pytest.raises(L.FaststyleError):
        eng.temporal_batch_f32(s, c, d, views, work[1], radius=8, levels=levels, subpel=2)
    assert int(np.prod(eng.temporal_batch_work(Ho, Wo, 1).shape)) >= 1 and int(np.prod(short.shape)) == eng.temporal_batch_layout(Ho, Wo, N - 1, levels, 2).work_bytes
