"""Batches of independent streams in the temporal stage (csrc/fs_temporal.hip: fs_temporal_streams_f32) against the contract in
include/faststyle_io.h: one call over S streams writes, for every stream that is not skipped, bit for bit what a single-frame call writes for
that stream's image -- the stabilised tensor and the whole slot --, with the previous frame taken from the stream's other slot where
FS_TS_PREV is set; a skipped stream is not touched.  The single-frame calls run on the same engine (tests.test_temporal_obmc.run) and, in one
case, in the numpy restatement of that file.  Every comparison is equality.  Every stream has its own frames, so a stream that read its
neighbour's state would show.  The same bodies run on the CPU emulator and, under -m gpu, on the MI355X."""
import ctypes

import numpy as np
import pytest

from faststyle_amd import _lib as L
from faststyle_amd._lib import FS_TS_PREV as PREV, FS_TS_SKIP as SKIP, FS_TS_SLOT as SLOT
from tests import backends
from tests.test_compose import GUARD, SENTINEL, f32_of_F, placed, same, to88
from tests.test_temporal import FILL, blocks_of, device_kw, luma8
from tests.test_temporal_batch import stream_of
from tests.test_temporal_obmc import obmc_ref, state_of
from tests.test_temporal_obmc import run as run_single
from tests.test_temporal_pyr import SHAPES as PYR_SHAPES
from tests.test_temporal_pyr import pyramid


@pytest.fixture(params=backends.engine_params())
def eng(request):
    return backends.get_engine(request.param)


STATE_FILL = 0x5C                                               # what the state buffer holds where no previous state was put
STREAMS = [1, 2, 3, 5]
MODES = [(1, 0, 0), (1, 0, 1), (2, 2, 0), (3, 2, 1)]            # levels, subpel, overlap
SHAPES = [(1, 1, 4, 4), (16, 16, 16, 16), (14, 30, 17, 33), (64, 48, 64, 48)]     # H, W, Ho, Wo
CASES = [(m, s) for m in MODES for s in (PYR_SHAPES if m[0] == 3 else SHAPES)]
case_id = lambda v: "x".join(map(str, v)) if len(v) == 4 else "L%dS%dO%d" % v


def slot_parts(eng, raw, Ho, Wo, levels, subpel):
    """The host bytes of one slot -> tests.test_temporal_obmc.run's dict without dst"""
    lay, pl = eng.temporal_streams_layout(Ho, Wo, 1, levels, subpel), eng.temporal_pyr_layout(Ho, Wo, levels)
    nb = blocks_of(Ho, Wo)
    part = lambda off, n: raw[int(off):int(off) + n]
    vec = lambda off, blocks: part(off, 2 * blocks[0] * blocks[1]).view(np.int8).reshape(blocks + (2,))
    pyr = int(lay.pyr_offset)
    return dict(luma=part(lay.luma_offset, Ho * Wo).reshape(Ho, Wo), out88=part(lay.out88_offset, Ho * Wo * 6).view("<u2").reshape(Ho, Wo, 3),
                mv=vec(lay.mv_offset, nb), mvf=vec(lay.mvf_offset, nb) if subpel else None,
                lumas=[part(pyr + pl.luma_offset[l], pl.h[l] * pl.w[l]).reshape(pl.h[l], pl.w[l]) for l in range(1, levels)],
                vs=[vec(pyr + pl.mv_offset[l], (pl.nby[l], pl.nbx[l])) for l in range(1, levels)])


def slot_range(lay, s, w):
    a = s * int(lay.stream_stride) + w * int(lay.slot_stride)
    return a, a + int(lay.slot_stride)


def put_previous(eng, image, s, w, prev, Ho, Wo, levels, subpel):
    """A previous frame's state (luma u8, out88 u16, [lumas of the levels 1 ..]) into slot w of stream s of the host image"""
    lay, pl = eng.temporal_streams_layout(Ho, Wo, 1, levels, subpel), eng.temporal_pyr_layout(Ho, Wo, levels)
    a = slot_range(lay, s, w)[0]
    image[a + int(lay.luma_offset):a + int(lay.luma_offset) + Ho * Wo] = np.ascontiguousarray(prev[0], np.uint8).reshape(-1)
    image[a + int(lay.out88_offset):a + int(lay.out88_offset) + Ho * Wo * 6] = np.ascontiguousarray(prev[1], "<u2").reshape(-1).view(np.uint8)
    for l in range(1, levels):
        at = a + int(lay.pyr_offset) + int(pl.luma_offset[l])
        image[at:at + prev[2][l - 1].size] = prev[2][l - 1].reshape(-1)


def run_streams(eng, src, cur, ctl, prevs=None, image=None, levels=1, subpel=0, overlap=0, alias=False, off=(0, 0, 0), coff=0, **kw):
    """eng.temporal_streams_f32 on host arrays src [S,H,W,3], cur [S,Ho,Wo,3] with the control words ctl -> (outs, image): per stream
    tests.test_temporal_obmc.run's dict from the slot the word names as written (None for a skipped stream), and the state buffer's bytes
    after the call.  The state starts as `image` (None: STATE_FILL everywhere) with prevs[s] (a previous frame's state, or None) put into
    the slot that stream s reads.  off: floats past a 16-byte boundary of src, cur, dst; coff: int32 words of ctl.  The state buffer has
    exactly the layout's size; it, the destination and the control words lie between guards that must come back untouched.  The control
    words come back unchanged, a stream's slot read comes back unchanged, and of a skipped stream both slots and its image of dst do."""
    mem = eng.mem
    S, Ho, Wo = cur.shape[:3]
    lay = eng.temporal_streams_layout(Ho, Wo, S, levels, subpel)
    need = int(lay.state_bytes)
    image = np.full(need, STATE_FILL, np.uint8) if image is None else np.array(image, copy=True)
    assert image.shape == (need,) and len(ctl) == S
    for s, prev in enumerate(prevs or ()):
        if prev is not None:
            put_previous(eng, image, s, (ctl[s] >> 1 & 1) ^ 1, prev, Ho, Wo, levels, subpel)
    _, sv, _ = placed(eng, src, off[0], 0)
    cbuf, c, c0 = placed(eng, cur, off[1], GUARD)
    dbuf, d, d0 = (cbuf, c, c0) if alias else placed(eng, np.full(cur.shape, SENTINEL, np.float32), off[2], GUARD)
    words = np.array(ctl, "<i4")
    kbuf, k, k0 = placed(eng, words.view(np.uint8), 4 * coff, GUARD, u8=True)
    tbuf, t, t0 = placed(eng, image, 0, GUARD, u8=True)
    eng.temporal_streams_f32(sv, c, d, k, t, levels=levels, subpel=subpel, overlap=overlap, **kw)
    whole = np.array(mem.to_numpy(dbuf), copy=True).reshape(-1)
    assert np.all(whole[:d0] == SENTINEL) and np.all(whole[d0 + cur.size:] == SENTINEL), "a write outside the destination"
    dst = whole[d0:d0 + cur.size].reshape(cur.shape)
    kw_ = np.array(mem.to_numpy(kbuf), copy=True).reshape(-1)
    assert np.all(kw_[:k0] == FILL) and np.all(kw_[k0 + 4 * S:] == FILL) and np.array_equal(kw_[k0:k0 + 4 * S].view("<i4"), words), "the control words changed"
    tw = np.array(mem.to_numpy(tbuf), copy=True).reshape(-1)
    assert np.all(tw[:t0] == FILL) and np.all(tw[t0 + need:] == FILL), "a write outside the state buffer"
    after = tw[t0:t0 + need]
    outs = []
    for s in range(S):
        w = ctl[s] >> 1 & 1
        (a, b), (ra, rb) = slot_range(lay, s, w), slot_range(lay, s, w ^ 1)
        assert np.array_equal(after[ra:rb], image[ra:rb]), "stream %d: the slot read changed" % s
        if ctl[s] & SKIP:
            assert np.array_equal(after[a:b], image[a:b]), "stream %d was skipped and its slot changed" % s
            assert same(dst[s], cur[s]) if alias else np.all(dst[s] == SENTINEL), "stream %d was skipped and its destination changed" % s
            outs.append(None)
            continue
        outs.append(dict(slot_parts(eng, after[a:b], Ho, Wo, levels, subpel), dst=dst[s]))
    mvs, mvfs = eng.temporal_streams_vectors(t, ctl, Ho, Wo, levels, subpel)
    assert mvs.dtype == np.int8 and mvs.shape == (S,) + blocks_of(Ho, Wo) + (2,) and (mvfs is None) == (subpel == 0)
    assert all(o is None or (np.array_equal(mvs[s], o["mv"]) and (mvfs is None or np.array_equal(mvfs[s], o["mvf"]))) for s, o in enumerate(outs))
    return outs, after


def equal_single(got, want):
    """One stream's dict against the single-frame call's: the tensor and every part of the slot"""
    return same(got["dst"], want["dst"]) and all(np.array_equal(got[k], want[k]) for k in ("luma", "out88", "mv")) and \
        (want["mvf"] is None) == (got["mvf"] is None) and (want["mvf"] is None or np.array_equal(got["mvf"], want["mvf"])) and \
        len(got["lumas"]) == len(want["lumas"]) and all(np.array_equal(a, b) for a, b in zip(got["lumas"], want["lumas"])) and \
        len(got["vs"]) == len(want["vs"]) and all(np.array_equal(a, b) for a, b in zip(got["vs"], want["vs"]))


# ================================================================ the layout (host only)
def test_the_layout_has_disjoint_aligned_parts_and_is_monotone(eng):
    for (Ho, Wo), levels, subpel in (((1, 1), 1, 0), ((64, 48), 1, 0), ((48, 64), 2, 2), ((720, 1280), 3, 2), ((1080, 1920), 3, 0), ((45, 62), 3, 1)):
        lays = [eng.temporal_streams_layout(Ho, Wo, n, levels, subpel) for n in range(1, 65)]
        pyr_bytes, nblk = int(eng.temporal_pyr_layout(Ho, Wo, levels).pyr_bytes), 2 * int(np.prod(blocks_of(Ho, Wo)))
        for n, l in enumerate(lays, 1):
            assert (l.streams, l.levels, l.subpel, l.reserved) == (n, levels, subpel, 0)
            parts = [(int(l.luma_offset), Ho * Wo), (int(l.out88_offset), Ho * Wo * 6), (int(l.pyr_offset), pyr_bytes), (int(l.mv_offset), nblk),
                     (int(l.mvf_offset), nblk if subpel else 0)]
            assert all(o % 16 == 0 for o, _ in parts) and l.slot_stride % 16 == 0 and l.stream_stride % 16 == 0
            assert parts[0][0] == 0 and all(a + n_ <= b for (a, n_), (b, _) in zip(parts, parts[1:])) and parts[-1][0] + parts[-1][1] <= l.slot_stride
            assert l.stream_stride == 2 * l.slot_stride and l.state_bytes == n * l.stream_stride
            assert all(getattr(l, f) == getattr(lays[0], f) for f in ("luma_offset", "out88_offset", "pyr_offset", "mv_offset", "mvf_offset",
                                                                      "slot_stride", "stream_stride"))
        sizes = [int(l.state_bytes) for l in lays]
        assert all(b > a for a, b in zip(sizes, sizes[1:]))
    info = L.fs_temporal_streams_info()
    assert ctypes.sizeof(info) == 80
    for code, a in ((-1, (0, 8, 1, 0, 2)), (-1, (8, 0, 1, 0, 2)), (-1, (8, 8, 1, 0, 0)), (-1, (8, 8, 1, 0, -1)), (-1, (8, 8, 1, 0, 65)),
                    (-2, (8, 8, 0, 0, 2)), (-2, (8, 8, 4, 0, 2)), (-2, (8, 8, 1, 3, 2)), (-2, (8, 8, 1, -1, 2))):
        assert eng.lib.fs_temporal_streams_layout(*a, ctypes.byref(info)) == code and b"fs_temporal_streams_layout" in eng.lib.fs_last_error()
    assert eng.lib.fs_temporal_streams_layout(8, 8, 1, 0, 2, None) == -1


# ================================================================ one call against single-frame calls
def frames_of(shape, S, step):
    """Stream s's frame number `step`: a different source and current tensor per stream and step"""
    src, cur = stream_of(shape)
    return np.stack([src[(s + step) % 7] for s in range(S)]), np.stack([cur[(s + 2 * step) % 6] for s in range(S)])


@pytest.mark.parametrize("streams", STREAMS)
@pytest.mark.parametrize("mode,shape", CASES, ids=case_id)
def test_a_call_is_the_single_frame_call_of_every_stream(eng, mode, shape, streams):
    """All first, the slot written mixed across the streams; then all continuing from the state that call left, in place"""
    levels, subpel, overlap = mode
    kw = dict(levels=levels, subpel=subpel, overlap=overlap, **device_kw(q8=154, K=4, matrix=1))
    src, cur = frames_of(shape, streams, 0)
    ctl = [SLOT * (s & 1) for s in range(streams)]
    first, image = run_streams(eng, src, cur, ctl, **kw)
    wants = [run_single(eng, src[s], cur[s], **kw) for s in range(streams)]
    assert all(equal_single(g, w) for g, w in zip(first, wants))
    assert all(not g["mv"].any() and same(g["dst"], f32_of_F(to88(cur[s]))) for s, g in enumerate(first))      # no previous frame: F = B
    src, cur = frames_of(shape, streams, 1)
    ctl = [PREV | (SLOT * (~s & 1)) for s in range(streams)]
    second, _ = run_streams(eng, src, cur, ctl, image=image, **kw)
    for s in range(streams):
        assert equal_single(second[s], run_single(eng, src[s], cur[s], prev=state_of(wants[s]), **kw)), s
    if shape[:2] >= (33, 47):                                                                   # ... and these had one (stream 0's frames show it)
        assert second[0]["mv"].any() and not same(second[0]["dst"], f32_of_F(to88(cur[0])))


def previous_states(shape, S, levels):
    """A previous frame's state per stream, every one different, from the restatement's parts"""
    src, cur = stream_of(shape)
    Ho, Wo = shape[2:]
    out = []
    for s in range(S):
        c8 = luma8(src[(s + 3) % 7], Ho, Wo, 1)
        out.append((c8, to88(cur[(s + 4) % 6]).astype(np.uint16), pyramid(c8, levels)[1:]))
    return out


@pytest.mark.parametrize("mode", MODES, ids=case_id)
@pytest.mark.parametrize("shape", [(14, 30, 17, 33), (64, 48, 64, 48)], ids=case_id)
def test_the_control_words_select_per_stream(eng, shape, mode):
    """Every slot holds a previous state; PREV and SLOT are mixed across the streams and the bits above 2 are ignored"""
    levels, subpel, overlap = mode
    if levels == 3:                                                                             # (three levels: their own ragged and large shape)
        shape = PYR_SHAPES[3] if shape[2] == 17 else PYR_SHAPES[-1]
    S = 5
    kw = dict(levels=levels, subpel=subpel, overlap=overlap, **device_kw(q8=200, K=8, matrix=1))
    src, cur = frames_of(shape, S, 2)
    prevs = previous_states(shape, S, levels)
    high = [0, 8, 0x7FFFFFF8, -8, 0x100]                                                        # (-8: every bit above 2)
    for ctl in ([PREV] * S, [PREV | SLOT] * S, [PREV, SLOT, PREV | SLOT, 0, PREV], [PREV | SLOT, PREV, 0, PREV, SLOT]):
        got, _ = run_streams(eng, src, cur, [c | h for c, h in zip(ctl, high)], prevs=prevs, **kw)
        for s in range(S):
            want = run_single(eng, src[s], cur[s], prev=prevs[s] if ctl[s] & PREV else None, **kw)
            assert equal_single(got[s], want), (ctl, s)
            assert bool(ctl[s] & PREV) or not got[s]["mv"].any()


# ================================================================ skipped streams
@pytest.mark.parametrize("mode", [MODES[0], MODES[3]], ids=case_id)
def test_a_skipped_stream_is_not_touched(eng, mode):
    """run_streams holds both slots and the destination rows of a skipped stream to what they were; its neighbours are exact"""
    levels, subpel, overlap = mode
    shape = PYR_SHAPES[-1] if levels == 3 else (14, 30, 17, 33)
    kw = dict(levels=levels, subpel=subpel, overlap=overlap, **device_kw(q8=154, K=4))
    src, cur = frames_of(shape, 3, 1)
    prevs = previous_states(shape, 3, levels)
    for ctl in ([PREV, SKIP | PREV | SLOT, PREV | SLOT], [SKIP, PREV, SKIP | SLOT], [PREV | SLOT, 0, SKIP | 8]):
        got, _ = run_streams(eng, src, cur, ctl, prevs=prevs, **kw)
        for s in range(3):
            if ctl[s] & SKIP:
                assert got[s] is None
            else:
                assert equal_single(got[s], run_single(eng, src[s], cur[s], prev=prevs[s] if ctl[s] & PREV else None, **kw)), (ctl, s)
    before = np.full(int(eng.temporal_streams_layout(shape[2], shape[3], 3, levels, subpel).state_bytes), STATE_FILL, np.uint8)
    for alias in (False, True):
        got, after = run_streams(eng, src, cur, [SKIP, SKIP | PREV, SKIP | SLOT | PREV], alias=alias, **kw)
        assert got == [None] * 3 and np.array_equal(after, before)                              # with every stream skipped nothing changes


# ================================================================ chained passes with per-stream control
SCHEDULE = [((1, 0, 1), None), ((1, 1, 1), None), ((1, 1, 0), None), ((1, 1, 1), 0)]            # (active per stream, the stream reset before the pass)


def chained(eng, shape, kw, single):
    """Four passes of three streams: stream 1 joins at pass 1, stream 2 skips pass 2, stream 0 is reset at pass 3.  Every stream's results
    against its own chain of `single` calls over the frames it actually took."""
    S = 3
    n, parity, prev, image = [0] * S, [0] * S, [None] * S, None
    for step, (active, reset) in enumerate(SCHEDULE):
        if reset is not None:
            n[reset] = 0
        src, cur = frames_of(shape, S, step)
        ctl = [(PREV if n[s] else 0) | (SLOT if parity[s] else 0) if active[s] else SKIP | (SLOT if parity[s] else 0) for s in range(S)]
        got, image = run_streams(eng, src, cur, ctl, image=image, **kw)
        for s in range(S):
            if not active[s]:
                assert got[s] is None
                continue
            want = single(src[s], cur[s], prev[s] if n[s] else None)
            assert equal_single(got[s], want), (step, s)
            prev[s], n[s], parity[s] = state_of(want), n[s] + 1, parity[s] ^ 1
    assert n == [1, 3, 3]


@pytest.mark.parametrize("mode", MODES, ids=case_id)
def test_four_chained_passes_are_every_streams_own_chain(eng, mode):
    levels, subpel, overlap = mode
    shape = PYR_SHAPES[-1] if levels == 3 else (64, 48, 64, 48)
    kw = dict(levels=levels, subpel=subpel, overlap=overlap, **device_kw(q8=154, K=4, matrix=1))
    chained(eng, shape, kw, lambda s, c, prev: run_single(eng, s, c, prev=prev, **kw))


def test_the_chained_passes_are_the_restatement(eng):
    kw = dict(levels=2, subpel=2, overlap=1, **device_kw(q8=200, K=8, matrix=1))
    chained(eng, (64, 48, 64, 48), kw, lambda s, c, prev: obmc_ref(s, c, prev=prev, levels=2, subpel=2, q8=200, K=8, matrix=1))


# ================================================================ placement
@pytest.mark.parametrize("mode", MODES[1:], ids=case_id)
def test_the_destination_may_be_the_current_tensor(eng, mode):
    levels, subpel, overlap = mode
    shape = (14, 30, 17, 33)
    kw = dict(levels=levels, subpel=subpel, overlap=overlap, **device_kw(q8=128))
    src, cur = frames_of(shape, 3, 0)
    prevs = previous_states(shape, 3, levels)
    ctl = [PREV, PREV | SLOT, 0]
    (a, ia), (b, ib) = run_streams(eng, src, cur, ctl, prevs=prevs, **kw), run_streams(eng, src, cur, ctl, prevs=prevs, alias=True, **kw)
    assert all(equal_single(x, y) for x, y in zip(a, b)) and np.array_equal(ia, ib)


def test_buffers_off_their_alignment_give_the_same_values(eng):
    """Tensors off 16 bytes and the control words 4, 8 and 12 bytes further; the state buffer has exactly the layout's size in every run"""
    shape = (14, 30, 17, 33)
    kw = dict(levels=3, subpel=2, overlap=1, **device_kw(q8=200))
    src, cur = frames_of(shape, 3, 0)
    prevs = previous_states(shape, 3, 3)
    ctl = [PREV | SLOT, PREV, PREV]
    want, iw = run_streams(eng, src, cur, ctl, prevs=prevs, **kw)
    for off, coff in (((1, 2, 3), 1), ((3, 1, 2), 2), ((2, 3, 1), 3)):
        got, ig = run_streams(eng, src, cur, ctl, prevs=prevs, off=off, coff=coff, **kw)
        assert all(equal_single(x, y) for x, y in zip(got, want)) and np.array_equal(ig, iw)


# ================================================================ refusals
def test_refused_calls_return_their_code_and_launch_nothing(eng):
    mem, lib, ctx = eng.mem, eng.lib, eng.ctx
    H, W, Ho, Wo, levels, S = 14, 30, 17, 33, 3, 3
    src, cur = frames_of((H, W, Ho, Wo), S, 1)
    prevs = previous_states((H, W, Ho, Wo), S, levels)
    _, s, _ = placed(eng, src, 0, 0)
    _, c, _ = placed(eng, cur, 0, 0)
    dbuf, d, d0 = placed(eng, np.full(cur.shape, SENTINEL, np.float32), 0, GUARD)
    need = int(eng.temporal_streams_layout(Ho, Wo, S, levels, 2).state_bytes)
    image = np.full(need, STATE_FILL, np.uint8)
    ctl = [PREV, PREV | SLOT, PREV]
    for i in range(S):
        put_previous(eng, image, i, (ctl[i] >> 1 & 1) ^ 1, prevs[i], Ho, Wo, levels, 2)
    tbuf, t, t0 = placed(eng, image, 0, GUARD, u8=True)
    _, k, _ = placed(eng, np.array(ctl, "<i4").view(np.uint8), 0, GUARD, u8=True)
    ps, pc, pd, pk, pt = mem.ptr(s), mem.ptr(c), mem.ptr(d), mem.ptr_u8(k), mem.ptr_u8(t)
    eng._sync_stream()

    def call(src=ps, H=H, W=W, cur=pc, Ho=Ho, Wo=Wo, streams=S, q8=128, K=16, R=7, levels=levels, subpel=2, overlap=1, matrix=0, bgr=0, ctl=pk,
             state=pt, state_bytes=need, dst=pd):
        return lib.fs_temporal_streams_f32(ctx, src, H, W, cur, Ho, Wo, streams, q8, K, R, levels, subpel, overlap, matrix, bgr, ctl, state,
                                           state_bytes, dst)

    refused = [(-1, dict(src=None)), (-1, dict(cur=None)), (-1, dict(dst=None)),
               (-1, dict(H=0)), (-1, dict(W=0)), (-1, dict(H=-3)), (-1, dict(Ho=H - 1)), (-1, dict(Ho=H + 4)), (-1, dict(Wo=W - 1)),
               (-1, dict(Wo=W + 4)), (-1, dict(H=2 ** 31 - 1)),
               (-2, dict(q8=-1)), (-2, dict(q8=257)), (-2, dict(K=0)), (-2, dict(K=257)), (-2, dict(R=-1)), (-2, dict(R=8)), (-2, dict(matrix=2)),
               (-2, dict(matrix=-1)), (-2, dict(bgr=2)), (-2, dict(bgr=-1)),
               (-5, dict(src=ps + 2)), (-5, dict(cur=pc + 1)), (-5, dict(dst=pd + 3)),
               (-2, dict(levels=0)), (-2, dict(levels=4)), (-2, dict(subpel=-1)), (-2, dict(subpel=3)), (-2, dict(overlap=2)), (-2, dict(overlap=-1)),
               (-1, dict(streams=0)), (-1, dict(streams=-1)), (-1, dict(streams=65)), (-1, dict(streams=S + 1)), (-1, dict(ctl=None)),
               (-1, dict(state=None)), (-1, dict(state_bytes=need - 1)), (-1, dict(state_bytes=0)), (-1, dict(streams=0, ctl=None, state=None)),
               (-5, dict(state=pt + 8, state_bytes=need + 16)), (-5, dict(state=pt + 1)), (-5, dict(ctl=pk + 2)), (-5, dict(ctl=pk + 1))]
    for code, kw in refused:
        assert call(**kw) == code, kw
        assert b"fs_temporal_streams_f32" in lib.fs_last_error()
    assert lib.fs_temporal_streams_f32(None, ps, H, W, pc, Ho, Wo, S, 128, 16, 7, levels, 2, 1, 0, 0, pk, pt, need, pd) == -1
    assert np.all(np.asarray(mem.to_numpy(dbuf)) == SENTINEL)                                 # nothing was launched
    assert np.array_equal(np.asarray(mem.to_numpy(tbuf)).reshape(-1)[t0:t0 + need], image)
    # the call they were variations of is taken
    assert call() == 0
    got = np.asarray(mem.to_numpy(dbuf)).reshape(-1)[d0:d0 + cur.size].reshape(cur.shape)
    for i in range(S):
        assert same(got[i], obmc_ref(src[i], cur[i], prev=prevs[i], levels=levels, subpel=2, q8=128)["dst"])
    # the engine checks the shapes against each other, against the state buffer and the control words
    short = eng.temporal_streams_state(Ho, Wo, S - 1, levels, 2)
    assert int(np.prod(short.shape)) == eng.temporal_streams_layout(Ho, Wo, S - 1, levels, 2).state_bytes
    for bad in (dict(cur=s), dict(src=mem.view(s, 0, (S - 1, H, W, 3))), dict(dst=mem.view(d, 0, (S - 1, Ho, Wo, 3))),
                dict(src=mem.view(s, 0, (H, W, 3)), cur=mem.view(c, 0, (Ho, Wo, 3)), dst=mem.view(d, 0, (Ho, Wo, 3))),
                dict(state=short), dict(ctl=mem.view(k, 0, (4 * (S - 1),))), dict(ctl=eng.i32_buffer([0] * (S + 1))),
                dict(levels=0), dict(levels=4), dict(subpel=3), dict(subpel=1.5), dict(overlap=2), dict(overlap=True)):
        a = dict(dict(src=s, cur=c, dst=d, ctl=k, state=t, levels=levels, subpel=2, overlap=1), **bad)
        with pytest.raises(L.FaststyleError):
            eng.temporal_streams_f32(a["src"], a["cur"], a["dst"], a["ctl"], a["state"], levels=a["levels"], subpel=a["subpel"], overlap=a["overlap"])
    with pytest.raises(L.FaststyleError):
        eng.temporal_streams_f32(s, c, d, k, t, radius=8, levels=levels, subpel=2)
