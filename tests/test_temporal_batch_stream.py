"""Consecutive frames per pass in the frame lanes (faststyle_amd/stream.py, temporal=dict(..., sequence=True) with batch=N): the recursion
over the frames of a pass and over passes, reset(), the three tail graphs by pass and the pipelined lanes.  As in
tests/test_temporal_obmc_stream.py every comparison is exact and independent of the net's numerics -- and so of which conv kernels a batch
selects: every frame of every pass is the numpy restatement's (tests/test_temporal_obmc.py) of the same lane's own net_input()[i] and current
tensor, chained over the frames.  The frames are that file's moving-apart noise; the net runs at 48 x 64 (45 x 62 for the lanes whose
output is larger than their input).  A stream's end is padded by the test itself, by repeating its last frame."""
import numpy as np
import pytest

from faststyle_amd import _lib, stream
from tests.backends import engine_params, get_engine, on_emulator
from tests.test_compose import f32_of_F, same, to88
from tests.test_compose_stream import KINDS, expected_frame, graph_modes, restated, variables
from tests.test_temporal import blocks_of
from tests.test_temporal_obmc import masks, obmc_ref
from tests.test_temporal_obmc_stream import HO, SIZE, WO, sequence


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


def passes_of(frames, n):
    """The frames in passes of n, the last one padded by repeating its last frame -> [(uint8 [n,H,W,3], how many are real), ...]"""
    out = []
    for k in range(0, len(frames), n):
        part = list(frames[k:k + n])
        out.append((np.stack(part + [part[-1]] * (n - len(part))), len(part)))
    return out


def check_pass(st, kind, out, prev, levels, subpel):
    """One pass of a sequence lane against the restatement chained over its frames -> (the state the next pass reads, the dicts)"""
    t = st.temporal
    N = st.shape[0]
    assert t["overlap"] == 1 and t["sequence"] is True
    src = st.net_input()
    cur = st.composed_output() if st.compose is not None else st.net_output()
    stab, mv = st.stabilised_output(), st.motion_vectors()
    assert stab.shape == st.out_shape == (N, HO, WO, 3) and mv.dtype == np.int8 and mv.shape == (N,) + blocks_of(HO, WO) + (2,)
    sub = st.motion_vectors_subpel() if subpel else None
    wants = []
    for i in range(N):
        want = obmc_ref(src[i], cur[i], prev=prev, levels=levels, subpel=subpel, q8=t["strength_q8"], K=t["sensitivity"], R=t["radius"],
                        matrix=t["matrix"], bgr=t["source_bgr"])
        assert same(stab[i], want["dst"]) and np.array_equal(mv[i], want["mv"])
        if subpel:
            assert np.array_equal(sub[i], 4 * want["mv"].astype(np.int16) + want["mvf"])
        assert out[i].dtype == np.uint8 and np.array_equal(out[i], expected_frame(st, kind, stab[i]))
        prev = (want["luma"], want["out88"], want["lumas"])
        wants.append(want)
    if levels > 1:                                                                          # the slot holds the last frame's pyramid
        lumas, vs = st.eng.temporal_pyramid(st._tslots[(st._tn - 1) & 1][:4], HO, WO, levels)
        assert all(np.array_equal(a, b) for a, b in zip(lumas, want["lumas"])) and all(np.array_equal(a, b) for a, b in zip(vs, want["vs"]))
    return prev, wants


def mixed_pixels(want):
    return 0 if want["info"] is None else int(np.count_nonzero(~masks(want)[0] & (want["info"]["D"] > 0)))


# kind -> (the lane kind of tests.test_compose_stream.KINDS, compose=, levels, subpel)
LANES = {"u8": ("u8", None, 2, 2), "yuv8": ("yuv8", None, 1, 0), "composed": ("u8", dict(strength=0.7, keep_color=True), 1, 2)}


@pytest.mark.parametrize("lane", sorted(LANES))
def test_a_sequence_lane_is_the_chained_restatement(eng, lane):
    """batch 3: seven frames in three passes, the last padded (on the emulator five frames in two passes: a pass takes seconds there)"""
    kind, compose, levels, subpel = LANES[lane]
    kw, odd = KINDS[kind]
    H, W = SIZE[odd]
    frames = sequence(H, W, 3, 7)[:5 if on_emulator(eng) else 7]
    extra = dict(dict(levels=levels) if levels > 1 else {}, **(dict(subpel=subpel) if subpel else {}))
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, variables(eng), H, W, batch=3, use_graph=use_graph, compose=compose,
                                  temporal=dict(strength=0.6, matrix="bt709", overlap=1, sequence=True, **extra), **kw)
        assert st.out_shape == (3, HO, WO, 3)
        assert st.temporal == dict(dict(strength_q8=154, sensitivity=16, radius=7, matrix=1, source_bgr=st.swap_rb, overlap=1, sequence=True), **extra)
        assert all(len(slot) == 3 + (levels > 1) + (subpel > 0) for slot in st._tslots) and len(st._tslots) == 2
        prev, mixed = None, 0
        for k, (batch, real) in enumerate(passes_of(frames, 3)):
            out = st(batch)
            assert same(st.net_input(), batch.astype(np.float32)) and st._tn == k + 1       # the counter goes by pass
            if compose is not None:
                assert same(st.composed_output(), restated(st))
            prev, wants = check_pass(st, kind, out, prev, levels, subpel)
            cur = st.composed_output() if compose is not None else st.net_output()
            if k == 0:                                                                      # a first frame, and only frame 0 of pass 0 is one
                assert not st.motion_vectors()[0].any() and same(st.stabilised_output()[0], f32_of_F(to88(cur[0])))
                assert st.motion_vectors()[1].any() and not same(st.stabilised_output()[1], f32_of_F(to88(cur[1])))
            else:
                assert not same(st.stabilised_output()[0], f32_of_F(to88(cur[0])))
            if real < 3:                                                                    # (the padding repeats a frame: it finds no motion)
                assert not st.motion_vectors()[real:].any()
            mixed += sum(mixed_pixels(w) for w in wants)
        assert mixed                                                                        # (the four-candidate path ran)
        if use_graph:                                                                       # a first pass's tail and one per parity
            assert sorted(st._tail_graphs, key=str) == [0, 1, None]
        st.release()


def test_reset_between_passes_forgets_the_previous_frame(eng):
    H, W = SIZE[True]
    frames = sequence(H, W, 4, 7)
    frames = frames[:5] + frames[6:]                                                        # (frames 4 and 5 of a sequence are one picture)
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, variables(eng), H, W, batch=2, use_graph=use_graph,
                                  temporal=dict(strength=0.6, sensitivity=4, radius=3, source_bgr=False, subpel=1, overlap=1, sequence=True))
        prev = None
        for k, (batch, _) in enumerate(passes_of(frames[:6], 2)):
            if k == 2 or (k == 1 and on_emulator(eng)):                                      # (two passes on the emulator: the reset before the second)
                st.reset()
                prev = None
                with pytest.raises(_lib.FaststyleError):
                    st.motion_vectors()
            out = st(batch)
            first = prev is None
            prev, _ = check_pass(st, "u8", out, prev, 1, 1)
            B = f32_of_F(to88(st.net_output()))
            assert same(st.stabilised_output()[0], B[0]) == first and not same(st.stabilised_output()[1], B[1])
            if on_emulator(eng) and k == 1:
                break
        st.release()


def test_sequence_at_batch_one_is_the_lane_without_the_key(eng):
    H, W = SIZE[True]
    g = not on_emulator(eng)
    frames = sequence(H, W, 5, 3)[:2 if on_emulator(eng) else 3]
    t = dict(strength=0.6, levels=2, subpel=2, overlap=1)
    stream.FrameStylizer.KEEP_GRAPH = g
    try:
        plain = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, temporal=t)
        seq = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, temporal=dict(t, sequence=True))
        off = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, temporal=dict(t, sequence=False))
        assert seq.temporal == plain.temporal == off.temporal and "sequence" not in seq.temporal and seq._twork is None
        assert [tuple(b.shape) for slot in seq._tslots for b in slot] == [tuple(b.shape) for slot in plain._tslots for b in slot]
        for f in frames:
            a, b = plain(f), seq(f)
            assert np.array_equal(a, b) and same(plain.stabilised_output(), seq.stabilised_output())
            assert seq.motion_vectors().shape == blocks_of(HO, WO) + (2,) and np.array_equal(plain.motion_vectors_subpel(), seq.motion_vectors_subpel())
        if g:
            from tests.test_generations import graph_node_types
            count = lambda s: [len(graph_node_types(s._graph))] + [len(graph_node_types(s._tail_graphs[k])) for k in (None, 0, 1)]
            assert count(plain) == count(seq)
        for s in (plain, seq, off):
            s.release()
    finally:
        stream.FrameStylizer.KEEP_GRAPH = False


def test_batches_without_the_key_and_other_values_are_still_refused(eng):
    H, W = SIZE[False]
    for t in (dict(strength=0.5), dict(strength=0.5, overlap=1), dict(strength=0.5, sequence=False)):
        with pytest.raises(_lib.FaststyleError, match="one frame per pass"):
            stream.FrameStylizer(eng, variables(eng), H, W, batch=2, use_graph=False, temporal=t)
    for bad in (1, 0, "yes", None, 1.0, 2):
        for batch in (1, 2):
            with pytest.raises(_lib.FaststyleError, match="sequence"):
                stream.FrameStylizer(eng, variables(eng), H, W, batch=batch, use_graph=False, temporal=dict(strength=0.5, sequence=bad))
    with pytest.raises(_lib.FaststyleError):
        stream.FrameStylizer(eng, variables(eng), H, W, batch=2, use_graph=False, temporal=dict(strength=0.5, sequence=True, levels=4))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3])
def test_pipelined_lanes_equal_the_one_lane_sequence_lane(depth):
    eng = get_engine("hip")
    H, W = SIZE[True]
    kw = dict(batch=3, temporal=dict(strength=0.8, sensitivity=4, levels=depth - 1, subpel=depth - 1, overlap=1, sequence=True),
              compose=dict(strength=0.9))
    batches = [b for b, _ in passes_of(sequence(H, W, 8, 7) + sequence(H, W, 9, 7), 3)]   # five passes
    single = stream.FrameStylizer(eng, variables(eng), H, W, **kw)
    ps = stream.PipelinedStylizer(eng, variables(eng), H, W, depth=depth, **kw)
    assert ps.temporal["sequence"] is True
    want = [single(b) for b in batches]
    assert len({w.tobytes() for w in want}) == len(batches) and want[0].shape == (3, HO, WO, 3)
    got = list(ps.run(batches))
    assert len(got) == len(batches) and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert all(ln._tslots is ps.lanes[0]._tslots and ln._twork is not ps.lanes[0]._twork and ln._stab is not ps.lanes[0]._stab for ln in ps.lanes[1:])
    ps.reset()
    single.reset()
    want = [single(b) for b in batches[1:4]]
    assert all(np.array_equal(g, w) for g, w in zip(ps.run(batches[1:4]), want))
    for s in (single, ps):
        s.release()


@pytest.mark.gpu
def test_a_batch_of_four_adds_three_blend_nodes_to_the_tail_graph():
    """A u8 lane's tail at batch 1 is luma, search, blend and the u8 conversion; at batch 4 the three launches in front of the blends and
    the conversion cover all frames, and only the blends are one per frame"""
    from tests.test_generations import HIP_NODE_KERNEL, graph_node_types
    eng = get_engine("hip")
    H, W = SIZE[False]
    stream.FrameStylizer.KEEP_GRAPH = True
    try:
        for t in (dict(strength=0.6), dict(strength=0.6, levels=3, subpel=2, overlap=1)):
            one = stream.FrameStylizer(eng, variables(eng), H, W, temporal=t)
            four = stream.FrameStylizer(eng, variables(eng), H, W, batch=4, temporal=dict(t, sequence=True))
            frames = sequence(H, W, 6, 7) + sequence(H, W, 7, 5)
            for f in frames[:3]:
                one(f)
            for b, _ in passes_of(frames, 4):
                four(b)
            for k in (None, 0, 1):
                a, b = graph_node_types(one._tail_graphs[k]), graph_node_types(four._tail_graphs[k])
                assert set(a) == set(b) == {HIP_NODE_KERNEL} and len(b) == len(a) + 3, (k, len(a), len(b))
            one.release()
            four.release()
    finally:
        stream.FrameStylizer.KEEP_GRAPH = False
