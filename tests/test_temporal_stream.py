"""The temporal stage in the frame lanes (faststyle_amd/stream.py, temporal=): the recursion over frames, its two state slots, reset(), the
split of the captured pass into a head and per-parity tails, and the ordering of the tails across pipelined lanes.  Every comparison is exact
and independent of the net's numerics: the stabilised tensor is the numpy restatement's (tests/test_temporal.py) of the same lane's
net_input() and net_output() / composed_output(), chained over the frames, and the frame that comes back is the existing conversion's
restatement of the stabilised tensor.  Sizes as tests/test_compose_stream.py."""
import numpy as np
import pytest

from faststyle_amd import _lib, stream
from tests.backends import engine_params, get_engine, on_emulator
from tests.test_compose import f32_of_F, same, to88
from tests.test_compose_stream import KINDS, expected_frame, graph_modes, odd_size, restated, variables
from tests.test_frame_source import net_size, plain_stylizer
from tests.test_temporal import blocks_of, temporal_ref


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


TEMPORAL = dict(strength=0.6, sensitivity=16, radius=7)


def sequence(H, W, seed, n=4):
    """A frame, the same frame, the frame moved by (3, -5), unrelated noise (and, beyond four, that noise moved and again)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    frames = [a, a.copy(), np.roll(a, (-3, 5), axis=(0, 1)), b, np.roll(b, (2, 1), axis=(0, 1)), b.copy(), a.copy()]
    return frames[:n]


def current(st):
    return (st.composed_output() if st.compose is not None else st.net_output())[0]


def step(st, prev):
    """The restatement of the lane's temporal stage on the tensors of its last pass, fed with the previous frame's restated state"""
    t = st.temporal
    return temporal_ref(st.net_input()[0], current(st), prev=prev, q8=t["strength_q8"], K=t["sensitivity"], R=t["radius"], matrix=t["matrix"],
                        bgr=t["source_bgr"])


def check_frame(st, kind, out, prev):
    """One frame of a lane against the restatement -> the state the next frame reads"""
    want = step(st, prev)
    stab = st.stabilised_output()
    assert stab.shape == st.out_shape and same(stab[0], want["dst"])
    mv = st.motion_vectors()
    assert mv.dtype == np.int8 and mv.shape == blocks_of(*st.out_shape[1:3]) + (2,) and np.array_equal(mv, want["mv"])
    frame = expected_frame(st, kind, stab[0])
    assert out == frame if kind == "jpeg" else (out.dtype == np.uint8 and np.array_equal(out, frame))
    return want["luma"], want["out88"]


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_sequence_is_the_chained_restatement(eng, kind):
    kw, odd = KINDS[kind]
    H, W = odd_size(eng) if odd else net_size(eng)
    frames = sequence(H, W, 3)
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, temporal=dict(TEMPORAL, matrix="bt709"), **kw)
        assert st.temporal == dict(strength_q8=154, sensitivity=16, radius=7, matrix=1, source_bgr=st.swap_rb)
        with pytest.raises(_lib.FaststyleError):
            st.stabilised_output()                                                          # nothing has run yet
        with pytest.raises(_lib.FaststyleError):
            st.motion_vectors()
        prev = None
        for k, f in enumerate(frames):
            out = st(f)
            assert same(st.net_input()[0], f.astype(np.float32))
            prev = check_frame(st, kind, out, prev)
            B = f32_of_F(to88(current(st)))
            if k < 2:                                                                       # a first frame; the same frame again: at rest, P = B
                assert not st.motion_vectors().any() and same(st.stabilised_output()[0], B)
            else:                                                                           # (the stage did something)
                assert not same(st.stabilised_output()[0], B)
            if k == 2:
                assert st.motion_vectors()[1, 1].tolist() == [3, -5]
        if use_graph:                                                                       # a first frame's tail and one per parity
            assert sorted(st._tail_graphs, key=str) == [0, 1, None]
        st.release()


def test_reset_forgets_the_previous_frame_and_compose_comes_first(eng):
    """Five frames around a reset(): frames 0 1 2 write slots 0 1 0, then 0 1 again -- both parities, and the first-frame path twice.  The
    lane also composes: the stage reads the composed tensor."""
    H, W = odd_size(eng)
    frames = sequence(H, W, 4, 5)
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, compose=dict(strength=0.7, keep_color=True),
                                  temporal=dict(strength=0.5, sensitivity=1, radius=3, source_bgr=False))
        assert st.temporal == dict(strength_q8=128, sensitivity=1, radius=3, matrix=0, source_bgr=False)
        prev = None
        for k, f in enumerate(frames):
            if k == 3:
                st.reset()
                prev = None
                with pytest.raises(_lib.FaststyleError):
                    st.motion_vectors()
            out = st(f)
            assert same(st.composed_output(), restated(st))
            prev = check_frame(st, "u8", out, prev)
            if k in (0, 3):
                assert same(st.stabilised_output(), f32_of_F(to88(st.composed_output())))
            elif k != 1:
                assert not same(st.stabilised_output(), f32_of_F(to88(st.composed_output())))
        st.release()


def test_strength_zero_reproduces_the_lane_without_the_stage(eng):
    """F = to88(cur), whose high byte is what fs_f32_to_u8 writes and whose 8.8 value is what the deep conversion reads: every kind of frame
    is that of the same lane built without temporal=, byte for byte, on first and later frames."""
    g = not on_emulator(eng)
    for kind in ("deep", "u8") if on_emulator(eng) else sorted(KINDS):                      # (jpeg and yuv8 read the u8 lane's bytes: GPU only)
        kw, odd = KINDS[kind]
        H, W = odd_size(eng) if odd else net_size(eng)
        frames = sequence(H, W, 5, 3)[1:]
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, temporal=dict(strength=0.0), **kw)
        ref = plain_stylizer(eng, H, W) if kind == "u8" else stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, **kw)
        for f in frames:
            got, want = st(f), ref(f)
            assert got == want if kind == "jpeg" else np.array_equal(got, want)
            assert same(st.stabilised_output(), f32_of_F(to88(st.net_output()))) and same(st.net_output(), ref.net_output())
        assert st.motion_vectors()[1, 1].tolist() == [3, -5]                                # (the search ran all the same)
        st.release()
        if kind != "u8":
            ref.release()


def test_a_lane_without_the_stage_has_none_of_it(eng):
    H, W = net_size(eng)
    st = plain_stylizer(eng, H, W)
    st(np.zeros((H, W, 3), np.uint8))
    assert st.temporal is None and st._stab is None and st._tslots is None and st._tail_graphs == {} and st._cur is None
    for call in (st.stabilised_output, st.motion_vectors, st.reset):
        with pytest.raises(_lib.FaststyleError):
            call()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3])
def test_pipelined_lanes_keep_the_recursion_and_the_one_lane_results(depth):
    eng = get_engine("hip")
    H, W = odd_size(eng)
    kw = dict(temporal=dict(strength=0.8, sensitivity=4), compose=dict(strength=0.9))
    frames = sequence(H, W, 8, 7)
    single = stream.FrameStylizer(eng, variables(eng), H, W, **kw)
    ps = stream.PipelinedStylizer(eng, variables(eng), H, W, depth=depth, **kw)
    want = [single(f) for f in frames]
    assert len({w.tobytes() for w in want[1:]}) == 6                                        # (a recursion: the same picture later is another frame)
    got = list(ps.run(frames))
    assert len(got) == 7 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert all(ln._tslots is ps.lanes[0]._tslots and ln._stab is not ps.lanes[0]._stab for ln in ps.lanes[1:])
    # reset: with nothing in flight only; the next frames are those of a one-lane run from its reset on
    ps.submit(frames[0])
    with pytest.raises(_lib.FaststyleError):
        ps.reset()
    ps.fetch()
    ps.reset()
    single.reset()
    want = [single(f) for f in frames[2:6]]
    assert all(np.array_equal(g, w) for g, w in zip(ps.run(frames[2:6]), want))
    for s in (single, ps):
        s.release()
    plain = stream.PipelinedStylizer(eng, variables(eng), H, W, depth=2)
    with pytest.raises(_lib.FaststyleError):
        plain.reset()
    assert plain.temporal is None and plain._tail_done is None
    plain.release()


def test_temporal_options_that_are_refused(eng):
    H, W = net_size(eng)
    nan = float("nan")
    for opt in (dict(strenght=0.5), dict(strength=0.5, keep_color=True), dict(strength=-0.1), dict(strength=1.5), dict(strength=nan),
                dict(strength="much"), dict(sensitivity=0), dict(sensitivity=257), dict(sensitivity=nan), dict(sensitivity=2.5),
                dict(sensitivity=None), dict(radius=-1), dict(radius=8), dict(radius=nan), dict(radius=1.5), dict(radius="far"),
                dict(matrix="bt2020"), dict(matrix=2)):
        with pytest.raises(_lib.FaststyleError):
            stream.FrameStylizer(eng, variables(eng), H, W, use_graph=False, temporal=opt)
    with pytest.raises(_lib.FaststyleError):
        stream.FrameStylizer(eng, variables(eng), H, W, batch=2, use_graph=False, temporal=dict(strength=0.5))
    # floor(s * 256 + 0.5), as compose; the defaults
    for s, q8 in ((0.0, 0), (0.001, 0), (0.002, 1), (0.3, 77), (0.5, 128), (0.998, 255), (0.9999, 256), (1, 256)):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=False, swap_rb=q8 & 1 == 0, temporal=dict(strength=s))
        assert st.temporal == dict(strength_q8=q8, sensitivity=16, radius=7, matrix=0, source_bgr=q8 & 1 == 0)
        assert tuple(st._stab.shape) == st.out_shape and len(st._tslots) == 2
        st.release()
