"""Overlapped block vectors in the frame lanes (faststyle_amd/stream.py, temporal=dict(..., overlap=)): the recursion over frames on the slots
of (levels, subpel), reset(), the three tail graphs and the pipelined lanes.  As in tests/test_temporal_sub_stream.py every comparison is exact
and independent of the net's numerics: the stabilised tensor, the vectors, the fractions and the pyramid are the numpy restatement's
(tests/test_temporal_obmc.py) of the same lane's own tensors, chained over the frames.  The frames are noise whose two halves move apart, the
edge in mid-block, so that the four-candidate path runs.  The net runs at 48 x 64 (45 x 62 for the lanes whose output is larger than their
input)."""
import numpy as np
import pytest

from faststyle_amd import _lib, stream
from tests.backends import engine_params, get_engine, on_emulator
from tests.test_compose import f32_of_F, same, to88
from tests.test_compose_stream import KINDS, expected_frame, graph_modes, restated, variables
from tests.test_temporal import blocks_of
from tests.test_temporal_obmc import masks, obmc_ref
from tests.test_temporal_stream import current


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


HO, WO = 48, 64
SIZE = {False: (HO, WO), True: (HO - 3, WO - 2)}               # by "the output is larger than the input"


def apart(a, axis, d=2):
    """uint8 [H,W,3] -> the same with the first region (the columns before 40 on axis 1, the rows before 24 on axis 0) showing what a shows
    d pixels further along the axis and the second what it shows d pixels back, wrapped round"""
    n = a.shape[axis]
    first = np.arange(n) < (n // 32) * 16 + 8
    first = first[None, :, None] if axis == 1 else first[:, None, None]
    return np.where(first, np.roll(a, -d, axis=axis), np.roll(a, d, axis=axis))


def sequence(H, W, seed, n=4):
    """A noise frame, its halves moved apart along the columns, moved apart again, another picture (and, beyond four, that picture's halves
    moved apart along the rows, the same again, and the first frame)"""
    rs = np.random.RandomState(seed)
    a, b = (rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(2))
    a1 = apart(a, 1)
    return [a, a1, apart(a1, 1, 1), b, apart(b, 0), apart(b, 0), a.copy()][:n]


def check_frame(st, kind, out, prev, levels, subpel):
    """One frame of a lane against the restatement -> (the state the next frame reads, the restatement's dict)"""
    t = st.temporal
    assert t["overlap"] == 1
    want = obmc_ref(st.net_input()[0], current(st), prev=prev, levels=levels, subpel=subpel, q8=t["strength_q8"], K=t["sensitivity"],
                    R=t["radius"], matrix=t["matrix"], bgr=t["source_bgr"])
    stab = st.stabilised_output()
    assert stab.shape == st.out_shape and same(stab[0], want["dst"])
    mv = st.motion_vectors()
    assert mv.dtype == np.int8 and mv.shape == blocks_of(HO, WO) + (2,) and np.array_equal(mv, want["mv"])
    if subpel:
        assert np.array_equal(st.motion_vectors_subpel(), 4 * want["mv"].astype(np.int16) + want["mvf"])
    if levels > 1:
        lumas, vs = st.eng.temporal_pyramid(st._tslots[(st._tn - 1) & 1][:4], HO, WO, levels)
        assert all(np.array_equal(a, b) for a, b in zip(lumas, want["lumas"])) and all(np.array_equal(a, b) for a, b in zip(vs, want["vs"]))
    frame = expected_frame(st, kind, stab[0])
    assert out == frame if kind == "jpeg" else (out.dtype == np.uint8 and np.array_equal(out, frame))
    return (want["luma"], want["out88"], want["lumas"]), want


def mixed_pixels(want):
    """How many pixels the four-candidate path blended: the vectors differ and some candidate matched"""
    return 0 if want["info"] is None else int(np.count_nonzero(~masks(want)[0] & (want["info"]["D"] > 0)))


@pytest.mark.parametrize("levels,subpel", [(1, 0), (2, 2)])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_sequence_is_the_chained_restatement(eng, kind, levels, subpel):
    kw, odd = KINDS[kind]
    H, W = SIZE[odd]
    frames = sequence(H, W, 3)
    for use_graph in graph_modes(eng):
        extra = dict(dict(levels=levels) if levels > 1 else {}, **(dict(subpel=subpel) if subpel else {}))
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, temporal=dict(strength=0.6, matrix="bt709", overlap=1, **extra),
                                  **kw)
        assert st.out_shape[1:3] == (HO, WO)
        assert st.temporal == dict(dict(strength_q8=154, sensitivity=16, radius=7, matrix=1, source_bgr=st.swap_rb, overlap=1), **extra)
        assert all(len(slot) == 3 + (levels > 1) + (subpel > 0) for slot in st._tslots)         # the slots of (levels, subpel): no buffer more
        prev, mixed = None, 0
        for k, f in enumerate(frames):
            out = st(f)
            assert same(st.net_input()[0], f.astype(np.float32))
            prev, want = check_frame(st, kind, out, prev, levels, subpel)
            B = f32_of_F(to88(current(st)))
            if k == 0:                                                                      # a first frame
                assert not st.motion_vectors().any() and same(st.stabilised_output()[0], B)
            elif k <= 2:                                                                    # (the stage did something)
                assert not same(st.stabilised_output()[0], B)
                assert not np.array_equal(want["F"], want["whole"])                         # (... that the whole-block blend does not)
            mixed += mixed_pixels(want)
        assert mixed                                                                        # (... along more than one vector per pixel)
        if use_graph:                                                                       # a first frame's tail and one per parity
            assert sorted(st._tail_graphs, key=str) == [0, 1, None]
        st.release()


@pytest.mark.parametrize("levels,subpel", [(1, 2), (3, 0)])
def test_reset_forgets_the_previous_frame_and_compose_comes_first(eng, levels, subpel):
    """Five frames around a reset(): frames 0 1 2 write slots 0 1 0, then 0 1 again -- both parities, and the first-frame path twice.  The
    lane also composes: the stage reads the composed tensor."""
    H, W = SIZE[True]
    frames = sequence(H, W, 4, 5)
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, compose=dict(strength=0.7, keep_color=True),
                                  temporal=dict(strength=0.6, sensitivity=4, radius=3, source_bgr=False, levels=levels, subpel=subpel, overlap=1))
        assert st.temporal == dict(dict(strength_q8=154, sensitivity=4, radius=3, matrix=0, source_bgr=False, overlap=1),
                                   **dict(dict(levels=levels) if levels > 1 else {}, **(dict(subpel=subpel) if subpel else {})))
        prev, mixed = None, 0
        for k, f in enumerate(frames):
            if k == 3:
                st.reset()
                prev = None
            out = st(f)
            assert same(st.composed_output(), restated(st))
            prev, want = check_frame(st, "u8", out, prev, levels, subpel)
            mixed += mixed_pixels(want)
            if k in (0, 3):
                assert same(st.stabilised_output(), f32_of_F(to88(st.composed_output())))
            else:
                assert not same(st.stabilised_output(), f32_of_F(to88(st.composed_output())))
        assert mixed
        st.release()


def test_overlap_zero_is_the_lane_without_the_key_and_strength_zero_the_lane_without_the_stage(eng):
    H, W = SIZE[True]
    g = not on_emulator(eng)
    frames = sequence(H, W, 5, 3)[:2] if on_emulator(eng) else sequence(H, W, 5, 3)         # (a pass takes seconds there: a frame and its move)
    plain = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, temporal=dict(strength=0.6))
    zero = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, temporal=dict(strength=0.6, overlap=0))
    assert zero.temporal == plain.temporal and "overlap" not in zero.temporal and all(len(slot) == 3 for slot in zero._tslots)
    for f in frames:
        a, b = plain(f), zero(f)
        assert np.array_equal(a, b) and same(plain.stabilised_output(), zero.stabilised_output())
        assert np.array_equal(plain.motion_vectors(), zero.motion_vectors())
    bare = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g)
    off = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, temporal=dict(strength=0.0, overlap=1))
    for f in frames[-2:]:
        assert np.array_equal(off(f), bare(f)) and same(off.stabilised_output(), f32_of_F(to88(off.net_output())))
    assert off.motion_vectors().any()                                                       # (the search ran all the same)
    for s in (plain, zero, bare, off):
        s.release()


@pytest.mark.gpu
def test_overlap_captures_the_graphs_of_the_lane_without_the_key():
    """overlap = 0 is the lane without the key in bytes and in graph node counts; overlap = 1 replaces the blend and adds no node"""
    from tests.test_generations import graph_node_types
    eng = get_engine("hip")
    H, W = SIZE[True]
    frames = sequence(H, W, 6, 3)
    stream.FrameStylizer.KEEP_GRAPH = True
    try:
        lanes = [stream.FrameStylizer(eng, variables(eng), H, W, temporal=t)
                 for t in (dict(strength=0.6), dict(strength=0.6, overlap=0), dict(strength=0.6, overlap=1), dict(strength=0.6, levels=3, subpel=2),
                           dict(strength=0.6, levels=3, subpel=2, overlap=0), dict(strength=0.6, levels=3, subpel=2, overlap=1))]
        outs = [[s(f) for f in frames] for s in lanes]
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1])) and all(np.array_equal(a, b) for a, b in zip(outs[3], outs[4]))
        assert not all(np.array_equal(a, b) for a, b in zip(outs[0], outs[2]))
        count = lambda s: [len(graph_node_types(s._graph))] + [len(graph_node_types(s._tail_graphs[k])) for k in (None, 0, 1)]
        n = [count(s) for s in lanes]
        assert n[0] == n[1] == n[2] and n[3] == n[4] == n[5], n
        for s in lanes:
            s.release()
    finally:
        stream.FrameStylizer.KEEP_GRAPH = False


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3])
def test_pipelined_lanes_keep_the_recursion_and_the_one_lane_results(depth):
    eng = get_engine("hip")
    H, W = SIZE[True]
    kw = dict(temporal=dict(strength=0.8, sensitivity=4, levels=depth - 1, subpel=depth - 1, overlap=1), compose=dict(strength=0.9))
    frames = sequence(H, W, 8, 7)
    single = stream.FrameStylizer(eng, variables(eng), H, W, **kw)
    ps = stream.PipelinedStylizer(eng, variables(eng), H, W, depth=depth, **kw)
    assert ps.temporal["overlap"] == 1
    want = [single(f) for f in frames]
    assert len({w.tobytes() for w in want}) == 7                                            # (a recursion: the same picture later is another frame)
    got = list(ps.run(frames))
    assert len(got) == 7 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert all(ln._tslots is ps.lanes[0]._tslots and len(ln._tslots[0]) == 2 + depth and ln._stab is not ps.lanes[0]._stab for ln in ps.lanes[1:])
    ps.reset()
    single.reset()
    want = [single(f) for f in frames[2:6]]
    assert all(np.array_equal(g, w) for g, w in zip(ps.run(frames[2:6]), want))
    for s in (single, ps):
        s.release()


def test_overlap_values_that_are_refused(eng):
    H, W = SIZE[False]
    for bad in (2, -1, 0.5, float("nan"), "yes", None):
        with pytest.raises(_lib.FaststyleError):
            stream.FrameStylizer(eng, variables(eng), H, W, use_graph=False, temporal=dict(strength=0.5, overlap=bad))
    with pytest.raises(_lib.FaststyleError):
        stream.FrameStylizer(eng, variables(eng), H, W, batch=2, use_graph=False, temporal=dict(strength=0.5, overlap=1))
    for more in (dict(levels=4), dict(subpel=3), dict(overlapped=1)):                       # the other keys keep their ranges beside it
        with pytest.raises(_lib.FaststyleError):
            stream.FrameStylizer(eng, variables(eng), H, W, use_graph=False, temporal=dict(strength=0.5, overlap=1, **more))
    st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=False, temporal=dict(strength=0.5, overlap=1.0, levels=2))
    assert st.temporal["overlap"] == 1 and len(st._tslots) == 2 and all(len(slot) == 4 for slot in st._tslots)
    with pytest.raises(_lib.FaststyleError):                                                # a lane without subpel has no fractions to show
        st.motion_vectors_subpel()
    st.release()
