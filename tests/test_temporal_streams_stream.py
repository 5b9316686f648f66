"""Independent streams per pass in the frame lanes (faststyle_amd/stream.py, temporal=dict(..., streams=True) with batch=S): every row of a
pass is a stream of its own with its own previous frame, set_streams() leaves streams out of passes, reset(stream=) forgets one stream's
previous frame, and all of it replays one tail graph.  As in tests/test_temporal_batch_stream.py every comparison is exact and independent
of the net's numerics: every active row of every pass is the numpy restatement's (tests/test_temporal_obmc.py) of the same lane's own
net_input()[s] and current tensor, chained over the passes that stream took part in.  The frames are that file's moving-apart noise, another
seed per stream; the net runs at 48 x 64 (45 x 62 for the lanes whose output is larger than their input)."""
import numpy as np
import pytest

from faststyle_amd import _lib, stream
from tests.backends import engine_params, get_engine, on_emulator
from tests.test_compose import f32_of_F, same, to88
from tests.test_compose_stream import KINDS, expected_frame, graph_modes, restated, variables
from tests.test_temporal import blocks_of
from tests.test_temporal_batch_stream import LANES
from tests.test_temporal_obmc import obmc_ref
from tests.test_temporal_obmc_stream import HO, SIZE, WO, sequence


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


# (active per stream, the stream reset before the pass): stream 1 joins at pass 1, stream 2 skips pass 2, stream 0 is reset at pass 3
SCHEDULE = [((True, False, True), None), ((True, True, True), None), ((True, True, False), None), ((True, True, True), 0), ((True, True, True), None)]
# on the emulator, where a pass takes seconds, the same events in three passes
SHORT = [((True, False, True), None), ((True, True, True), 0), ((True, True, False), None)]


def passes(H, W, S, n):
    """n passes of S streams, another noise sequence per stream -> [uint8 [S,H,W,3], ...]"""
    per = [sequence(H, W, 3 + s, 7) for s in range(S)]
    return [np.stack([per[s][k % 7] for s in range(S)]) for k in range(n)]


class Chains(object):
    """The restatement chained per stream over the passes that stream took, beside a streams lane"""

    def __init__(self, S, levels, subpel):
        self.S, self.levels, self.subpel = S, levels, subpel
        self.prev, self.stab, self.mv = [None] * S, None, [None] * S

    def reset(self, s):
        self.prev[s] = None

    def check(self, st, kind, out, active):
        t = st.temporal
        assert t["overlap"] == 1 and t["streams"] is True
        src = st.net_input()
        cur = st.composed_output() if st.compose is not None else st.net_output()
        stab, mv = st.stabilised_output(), st.motion_vectors()
        assert stab.shape == st.out_shape == (self.S, HO, WO, 3) and mv.dtype == np.int8 and mv.shape == (self.S,) + blocks_of(HO, WO) + (2,)
        sub = st.motion_vectors_subpel() if self.subpel else None
        firsts = []
        for s in range(self.S):
            if not active[s]:                                                                   # its row and its vectors are what they were
                assert self.stab is None or same(stab[s], self.stab[s])
                assert self.mv[s] is None or np.array_equal(mv[s], self.mv[s])
                continue
            want = obmc_ref(src[s], cur[s], prev=self.prev[s], levels=self.levels, subpel=self.subpel, q8=t["strength_q8"], K=t["sensitivity"],
                            R=t["radius"], matrix=t["matrix"], bgr=t["source_bgr"])
            assert same(stab[s], want["dst"]) and np.array_equal(mv[s], want["mv"]), s
            if self.subpel:
                assert np.array_equal(sub[s], 4 * want["mv"].astype(np.int16) + want["mvf"])
            assert out[s].dtype == np.uint8 and np.array_equal(out[s], expected_frame(st, kind, stab[s]))
            if self.prev[s] is None:
                assert not mv[s].any() and same(stab[s], f32_of_F(to88(cur[s])))                # a first frame: F = B
                firsts.append(s)
            self.prev[s], self.mv[s] = (want["luma"], want["out88"], want["lumas"]), want["mv"]
        self.stab = stab
        return firsts


@pytest.mark.parametrize("lane", sorted(LANES))
def test_a_streams_lane_is_every_streams_own_chain(eng, lane):
    kind, compose, levels, subpel = LANES[lane]
    kw, odd = KINDS[kind]
    H, W = SIZE[odd]
    schedule = SHORT if on_emulator(eng) else SCHEDULE
    extra = dict(dict(levels=levels) if levels > 1 else {}, **(dict(subpel=subpel) if subpel else {}))
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, variables(eng), H, W, batch=3, use_graph=use_graph, compose=compose,
                                  temporal=dict(strength=0.6, matrix="bt709", overlap=1, streams=True, **extra), **kw)
        assert st.temporal == dict(dict(strength_q8=154, sensitivity=16, radius=7, matrix=1, source_bgr=st.swap_rb, overlap=1, streams=True), **extra)
        assert int(np.prod(st._tslots.shape)) == eng.temporal_streams_layout(HO, WO, 3, levels, subpel).state_bytes and st._twork is None
        chains, firsts = Chains(3, levels, subpel), []
        for k, (batch, (active, reset)) in enumerate(zip(passes(H, W, 3, len(schedule)), schedule)):
            if reset is not None:
                st.reset(reset)
                chains.reset(reset)
            st.set_streams(active)
            out = st(batch)
            assert same(st.net_input(), batch.astype(np.float32)) and st._tn == k + 1
            if compose is not None:
                assert same(st.composed_output(), restated(st))
            firsts.append(chains.check(st, kind, out, active))
        assert firsts == ([[0, 2], [0, 1], []] if schedule is SHORT else [[0, 2], [1], [], [0], []])
        if use_graph:                                                                           # whatever the passes, resets and activity were
            assert list(st._tail_graphs) == ["streams"]
        if not on_emulator(eng):                                                                # one more: all of them again, all forgotten
            st.set_streams()
            st.reset()
            out = st(passes(H, W, 3, 1)[0])
            for s in range(3):
                chains.reset(s)
            assert chains.check(st, kind, out, (True, True, True)) == [0, 1, 2] and len(st._tail_graphs) == (1 if use_graph else 0)
        st.release()


def test_streams_at_batch_one_gives_the_bytes_of_the_lane_without_the_key(eng):
    H, W = SIZE[True]
    n = 3 if on_emulator(eng) else 5
    frames = sequence(H, W, 5, 7)[:n]
    t = dict(strength=0.6, levels=2, subpel=2, overlap=1)
    for use_graph in graph_modes(eng):
        plain = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, temporal=t)
        one = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, temporal=dict(t, streams=True))
        off = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, temporal=dict(t, streams=False))
        assert off.temporal == plain.temporal and "streams" not in off.temporal and off._sh is None and len(off._tslots) == 2
        for k, f in enumerate(frames):
            if k == n - 2:
                plain.reset()
                one.reset()
            a, b = plain(f), one(f)
            assert a.shape == b.shape and np.array_equal(a, b) and same(plain.stabilised_output(), one.stabilised_output())
            assert np.array_equal(plain.motion_vectors_subpel(), one.motion_vectors_subpel()[0])
            assert plain.motion_vectors().any() == (k not in (0, n - 2))
        if use_graph:
            assert sorted(plain._tail_graphs, key=str) == [0, 1, None] and list(one._tail_graphs) == ["streams"]
        for s in (plain, one, off):
            s.release()


def test_the_lane_refusals(eng):
    H, W = SIZE[False]
    v = variables(eng)
    for bad in (1, 0, "yes", None, 1.0, 2):
        for batch in (1, 2):
            with pytest.raises(_lib.FaststyleError, match="streams"):
                stream.FrameStylizer(eng, v, H, W, batch=batch, use_graph=False, temporal=dict(strength=0.5, streams=bad))
    for batch in (1, 2):
        with pytest.raises(_lib.FaststyleError, match="mutually exclusive"):
            stream.FrameStylizer(eng, v, H, W, batch=batch, use_graph=False, temporal=dict(strength=0.5, streams=True, sequence=True))
    with pytest.raises(_lib.FaststyleError, match="one frame per pass"):
        stream.FrameStylizer(eng, v, H, W, batch=2, use_graph=False, temporal=dict(strength=0.5, streams=False))
    with pytest.raises(_lib.FaststyleError):
        stream.FrameStylizer(eng, v, H, W, batch=2, use_graph=False, temporal=dict(strength=0.5, streams=True, levels=4))
    st = stream.FrameStylizer(eng, v, H, W, batch=2, use_graph=False, temporal=dict(strength=0.5, streams=True))
    for bad in ([True], [True, False, True], [1, 0], [True, None], "ab", 1, [[True, True]], np.ones(2, np.int32)):
        with pytest.raises(_lib.FaststyleError, match="set_streams"):
            st.set_streams(bad)
    st.set_streams(np.array([True, False]))
    st.set_streams((False, True))
    for bad in (-1, 2, 1.0, "0", True, [0]):
        with pytest.raises(_lib.FaststyleError, match="reset"):
            st.reset(bad)
    st.reset(np.int64(1))
    with pytest.raises(_lib.FaststyleError):
        st.motion_vectors()                                                                     # (no pass yet)
    st.release()
    for other in (stream.FrameStylizer(eng, v, H, W, use_graph=False, temporal=dict(strength=0.5)),
                  stream.FrameStylizer(eng, v, H, W, use_graph=False)):
        with pytest.raises(_lib.FaststyleError, match="set_streams"):
            other.set_streams([True])
        with pytest.raises(_lib.FaststyleError, match="reset"):
            other.reset(0)
        other.release()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3])
def test_pipelined_lanes_equal_the_one_lane_streams_lane(depth):
    """The lanes share the state buffer, each has its own control words; set_streams and reset(stream=) apply to the next submitted pass"""
    eng = get_engine("hip")
    H, W = SIZE[True]
    kw = dict(batch=3, temporal=dict(strength=0.8, sensitivity=4, levels=depth - 1, subpel=depth - 1, overlap=1, streams=True),
              compose=dict(strength=0.9))
    schedule = SCHEDULE + SCHEDULE[1:3]                                                        # seven passes
    batches = passes(H, W, 3, len(schedule))

    def stepper(st):
        it = iter(schedule)

        def step():
            active, reset = next(it)
            if reset is not None:
                st.reset(reset)
            st.set_streams(active)
        return step

    single = stream.FrameStylizer(eng, variables(eng), H, W, **kw)
    step, want = stepper(single), []
    for b in batches:
        step()
        want.append(single(b))
    assert len({w.tobytes() for w in want}) == len(batches) and want[0].shape == (3, HO, WO, 3)
    ps = stream.PipelinedStylizer(eng, variables(eng), H, W, depth=depth, **kw)
    assert ps.temporal["streams"] is True
    got = list(ps.run(batches, before_submit=stepper(ps)))
    assert len(got) == len(batches)
    for g, w, (active, _) in zip(got, want, schedule):                                         # (an inactive row is whatever its lane held)
        assert all(np.array_equal(g[s], w[s]) for s in range(3) if active[s])
    assert np.array_equal(ps.lanes[(len(batches) - 1) % depth].motion_vectors(), single.motion_vectors())
    assert all(ln._tslots is ps.lanes[0]._tslots and ln._sh is ps.lanes[0]._sh and ln._sctl is not ps.lanes[0]._sctl and
               ln._stab is not ps.lanes[0]._stab for ln in ps.lanes[1:])
    assert all(list(ln._tail_graphs) == ["streams"] for ln in ps.lanes) and list(single._tail_graphs) == ["streams"]
    for s in (single, ps):
        s.release()


@pytest.mark.gpu
def test_a_batch_of_four_streams_adds_no_node_to_the_tail_graph():
    """A streams tail holds the kernel nodes of a batch-1 temporal tail of the same mode: every launch, the blend included, covers all
    streams"""
    from tests.test_generations import HIP_NODE_KERNEL, graph_node_types
    eng = get_engine("hip")
    H, W = SIZE[False]
    stream.FrameStylizer.KEEP_GRAPH = True
    try:
        for t in (dict(strength=0.6), dict(strength=0.6, levels=3, subpel=2, overlap=1)):
            one = stream.FrameStylizer(eng, variables(eng), H, W, temporal=t)
            four = stream.FrameStylizer(eng, variables(eng), H, W, batch=4, temporal=dict(t, streams=True))
            for b in passes(H, W, 4, 3):
                one(b[0])
                four(b)
            assert list(four._tail_graphs) == ["streams"]
            b = graph_node_types(four._tail_graphs["streams"])
            for k in (None, 0, 1):
                a = graph_node_types(one._tail_graphs[k])
                assert set(a) == set(b) == {HIP_NODE_KERNEL} and len(b) == len(a), (k, len(a), len(b))
            one.release()
            four.release()
    finally:
        stream.FrameStylizer.KEEP_GRAPH = False
