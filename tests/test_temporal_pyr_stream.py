"""The coarse-to-fine search in the frame lanes (faststyle_amd/stream.py, temporal=dict(..., levels=)): the recursion over frames with the
fourth state buffer, reset(), the three tail graphs and the pipelined lanes.  As in tests/test_temporal_stream.py every comparison is exact and
independent of the net's numerics: the stabilised tensor, the vectors and the pyramid are the numpy restatement's (tests/test_temporal_pyr.py)
of the same lane's own tensors, chained over the frames.  The net runs at 48 x 64 (45 x 62 for the lanes whose output is larger than their
input): two levels end in a 24 x 32 level, three in one ragged 12 x 16 block."""
import numpy as np
import pytest

from faststyle_amd import _lib, stream
from tests.backends import engine_params, get_engine, on_emulator
from tests.test_compose import f32_of_F, same, to88
from tests.test_compose_stream import KINDS, expected_frame, graph_modes, restated, variables
from tests.test_temporal import blocks_of
from tests.test_temporal_pyr import pyr_ref
from tests.test_temporal_stream import current


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


HO, WO = 48, 64
SIZE = {False: (HO, WO), True: (HO - 3, WO - 2)}               # by "the output is larger than the input"


def sequence(H, W, seed, n=4):
    """A frame, the same frame, the frame moved by (10, -6) -- beyond the reach of one level --, unrelated noise (and, beyond four, that
    noise moved by (-4, 12) and again)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    frames = [a, a.copy(), np.roll(a, (-10, 6), axis=(0, 1)), b, np.roll(b, (4, -12), axis=(0, 1)), b.copy(), a.copy()]
    return frames[:n]


def check_frame(st, kind, out, prev, levels):
    """One frame of a lane against the restatement -> the state the next frame reads"""
    t = st.temporal
    want = pyr_ref(st.net_input()[0], current(st), prev=prev, levels=levels, q8=t["strength_q8"], K=t["sensitivity"], R=t["radius"],
                   matrix=t["matrix"], bgr=t["source_bgr"])
    stab = st.stabilised_output()
    assert stab.shape == st.out_shape and same(stab[0], want["dst"])
    mv = st.motion_vectors()
    assert mv.dtype == np.int8 and mv.shape == blocks_of(HO, WO) + (2,) and np.array_equal(mv, want["mv"])
    lumas, vs = st.eng.temporal_pyramid(st._tslots[(st._tn - 1) & 1], HO, WO, levels)
    assert len(lumas) == len(vs) == levels - 1
    assert all(np.array_equal(a, b) for a, b in zip(lumas, want["lumas"])) and all(np.array_equal(a, b) for a, b in zip(vs, want["vs"]))
    frame = expected_frame(st, kind, stab[0])
    assert out == frame if kind == "jpeg" else (out.dtype == np.uint8 and np.array_equal(out, frame))
    return want["luma"], want["out88"], want["lumas"]


@pytest.mark.parametrize("levels", [2, 3])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_sequence_is_the_chained_restatement(eng, kind, levels):
    kw, odd = KINDS[kind]
    H, W = SIZE[odd]
    frames = sequence(H, W, 3)
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, temporal=dict(strength=0.6, matrix="bt709", levels=levels), **kw)
        assert st.out_shape[1:3] == (HO, WO)
        assert st.temporal == dict(strength_q8=154, sensitivity=16, radius=7, matrix=1, source_bgr=st.swap_rb, levels=levels)
        assert all(len(slot) == 4 for slot in st._tslots)
        prev = None
        for k, f in enumerate(frames):
            out = st(f)
            assert same(st.net_input()[0], f.astype(np.float32))
            prev = check_frame(st, kind, out, prev, levels)
            B = f32_of_F(to88(current(st)))
            if k < 2:                                                                       # a first frame; the same frame again: at rest, P = B
                assert not st.motion_vectors().any() and same(st.stabilised_output()[0], B)
            else:                                                                           # (the stage did something)
                assert not same(st.stabilised_output()[0], B)
            if k == 2 and not odd and levels == 2:                                          # block (0, 1) and its copy lie inside, and the move
                assert st.motion_vectors()[0, 1].tolist() == [10, -6]                       # is whole on the coarsest level: (5, -3)
        if use_graph:                                                                       # a first frame's tail and one per parity
            assert sorted(st._tail_graphs, key=str) == [0, 1, None]
        st.release()


@pytest.mark.parametrize("levels", [2, 3])
def test_reset_forgets_the_previous_frame_and_compose_comes_first(eng, levels):
    """Five frames around a reset(): frames 0 1 2 write slots 0 1 0, then 0 1 again -- both parities, and the first-frame path twice.  The
    lane also composes: the stage reads the composed tensor."""
    H, W = SIZE[True]
    frames = sequence(H, W, 4, 5)
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, compose=dict(strength=0.7, keep_color=True),
                                  temporal=dict(strength=0.6, sensitivity=1, radius=3, source_bgr=False, levels=levels))
        assert st.temporal == dict(strength_q8=154, sensitivity=1, radius=3, matrix=0, source_bgr=False, levels=levels)
        prev = None
        for k, f in enumerate(frames):
            if k == 3:
                st.reset()
                prev = None
                with pytest.raises(_lib.FaststyleError):
                    st.motion_vectors()
            out = st(f)
            assert same(st.composed_output(), restated(st))
            prev = check_frame(st, "u8", out, prev, levels)
            if k in (0, 3):
                assert same(st.stabilised_output(), f32_of_F(to88(st.composed_output())))
            elif k != 1:
                assert not same(st.stabilised_output(), f32_of_F(to88(st.composed_output())))
        st.release()


def test_one_level_is_the_lane_without_the_key_and_strength_zero_the_lane_without_the_stage(eng):
    H, W = SIZE[True]
    g = not on_emulator(eng)
    frames = sequence(H, W, 5, 3)[1:] if on_emulator(eng) else sequence(H, W, 5, 3)         # (a pass takes seconds there: a frame and its move)
    plain = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, temporal=dict(strength=0.6))
    one = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, temporal=dict(strength=0.6, levels=1))
    assert one.temporal == plain.temporal and "levels" not in one.temporal and all(len(slot) == 3 for slot in one._tslots)
    for f in frames:
        a, b = plain(f), one(f)
        assert np.array_equal(a, b) and same(plain.stabilised_output(), one.stabilised_output())
        assert np.array_equal(plain.motion_vectors(), one.motion_vectors())
    bare = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g)
    for levels in (3,) if on_emulator(eng) else (2, 3):
        zero = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, temporal=dict(strength=0.0, levels=levels))
        for f in frames[-2:]:
            assert np.array_equal(zero(f), bare(f)) and same(zero.stabilised_output(), f32_of_F(to88(zero.net_output())))
        assert zero.motion_vectors().any()                                                  # (the search ran all the same)
        zero.release()
    for s in (plain, one, bare):
        s.release()


@pytest.mark.gpu
def test_one_level_captures_the_graphs_of_the_lane_without_the_key():
    from tests.test_generations import graph_node_types
    eng = get_engine("hip")
    H, W = SIZE[True]
    frames = sequence(H, W, 6, 3)
    stream.FrameStylizer.KEEP_GRAPH = True
    try:
        lanes = [stream.FrameStylizer(eng, variables(eng), H, W, temporal=t)
                 for t in (dict(strength=0.6), dict(strength=0.6, levels=1), dict(strength=0.6, levels=2), dict(strength=0.6, levels=3))]
        outs = [[s(f) for f in frames] for s in lanes]
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))
        count = lambda s: [len(graph_node_types(s._graph))] + [len(graph_node_types(s._tail_graphs[k])) for k in (None, 0, 1)]
        n = [count(s) for s in lanes]
        assert n[0] == n[1], n
        assert n[2] == [n[0][0]] + [c + 2 for c in n[0][1:]] and n[3] == [n[0][0]] + [c + 3 for c in n[0][1:]], n     # the pyramid, a search per level
        for s in lanes:
            s.release()
    finally:
        stream.FrameStylizer.KEEP_GRAPH = False


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3])
def test_pipelined_lanes_keep_the_recursion_and_the_one_lane_results(depth):
    eng = get_engine("hip")
    H, W = SIZE[True]
    kw = dict(temporal=dict(strength=0.8, sensitivity=4, levels=depth), compose=dict(strength=0.9))     # (two levels at depth 2, three at 3)
    frames = sequence(H, W, 8, 7)
    single = stream.FrameStylizer(eng, variables(eng), H, W, **kw)
    ps = stream.PipelinedStylizer(eng, variables(eng), H, W, depth=depth, **kw)
    want = [single(f) for f in frames]
    assert len({w.tobytes() for w in want[1:]}) == 6                                        # (a recursion: the same picture later is another frame)
    got = list(ps.run(frames))
    assert len(got) == 7 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert all(ln._tslots is ps.lanes[0]._tslots and len(ln._tslots[0]) == 4 and ln._stab is not ps.lanes[0]._stab for ln in ps.lanes[1:])
    ps.reset()
    single.reset()
    want = [single(f) for f in frames[2:6]]
    assert all(np.array_equal(g, w) for g, w in zip(ps.run(frames[2:6]), want))
    for s in (single, ps):
        s.release()


def test_levels_that_are_refused(eng):
    H, W = SIZE[False]
    for bad in (0, 4, -1, 2.5, float("nan"), "deep", None):
        with pytest.raises(_lib.FaststyleError):
            stream.FrameStylizer(eng, variables(eng), H, W, use_graph=False, temporal=dict(strength=0.5, levels=bad))
    with pytest.raises(_lib.FaststyleError):
        stream.FrameStylizer(eng, variables(eng), H, W, batch=2, use_graph=False, temporal=dict(strength=0.5, levels=2))
    with pytest.raises(_lib.FaststyleError):                                                # the radius keeps its range under more levels
        stream.FrameStylizer(eng, variables(eng), H, W, use_graph=False, temporal=dict(strength=0.5, levels=3, radius=8))
    st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=False, temporal=dict(strength=0.5, levels=2.0))
    assert st.temporal["levels"] == 2 and len(st._tslots) == 2 and all(len(slot) == 4 for slot in st._tslots)
    st.release()
