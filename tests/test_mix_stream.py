"""Two styles per stream in the frame lanes (faststyle_amd/stream.py, mix=): a second forward pass into a workspace of its own and fs_mix_f32
ahead of compose, the temporal stage and every output conversion.  Every comparison is exact: the two nets' outputs are those of two
one-model lanes bit for bit (the frozen-filter test), the mixed tensor is the numpy restatement's (tests/test_mix.py) of the lane's own two
outputs, and the frame that comes back is the existing conversion's restatement of it.  starry + candy; 48 x 56 eager on the emulator,
96 x 136 on the GPU through the captured graphs and eagerly, two frames there so that the second replays."""
import os

import numpy as np
import pytest

from faststyle_amd import _lib, ckpt, stream
from oracle import tnet
from tests.backends import engine_params, get_engine, on_emulator
from tests.test_compose import compose_ref, f32_of_F, same, to88
from tests.test_compose_stream import KINDS, expected_frame, graph_modes, noise_mask, odd_size
from tests.test_frame_source import n_frames, net_size
from tests.test_jpeg_encode import starry
from tests.test_mix import mix_ref
from tests.test_temporal_batch_stream import passes_of
from tests.test_temporal_obmc import obmc_ref
from tests.test_temporal_obmc_stream import HO, SIZE, WO, sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


def candy(eng):
    P = tnet.strip_scope(ckpt.load_checkpoint(os.path.join(ROOT, "models", "candy_final.ckpt")))
    return P, eng.mem.from_numpy(eng.flatten_params(P, scope=""))


_vars = {}


def models(eng):
    """(starry, candy) on the engine's device, once per engine"""
    if id(eng) not in _vars:
        _vars[id(eng)] = (starry(eng)[1], candy(eng)[1])
    return _vars[id(eng)]


def q8_of(t):
    return int(np.floor(t * 256.0 + 0.5))


def restated(st, weights, mask=None):
    """The restatement of the lane's mix stage on the two outputs of its last pass; a model the pass did not run lends the other's"""
    live = st.last_forwards()
    a = st.net_output() if "a" in live else st.net_output2()
    b = st.net_output2() if "b" in live else st.net_output()
    return mix_ref(a, b, t=[q8_of(t) for t in np.broadcast_to(weights, (st.shape[0],))], mask=mask, in_hw=st.shape[1:3])


def frames_of(H, W, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(n)]


def same_frame(got, want):
    return got == want if isinstance(want, bytes) else (got.dtype == np.uint8 and np.array_equal(got, want))


# ================================================================ 1. the two forwards are the one-model lanes'
def test_both_outputs_equal_the_one_model_lanes_bit_for_bit(eng):
    """Three lanes on one context, their calls interleaved: the mixed lane alternates two (parameters, workspace) pairs under
    FS_FLAG_PARAMS_FROZEN, the one-model lanes come in between.  A filter re-layout reused for the wrong model would show here."""
    H, W = net_size(eng)
    A, B = models(eng)
    for use_graph in graph_modes(eng):
        mixed = stream.FrameStylizer(eng, A, H, W, use_graph=use_graph, mix=dict(variables=B, weight=0.5))
        one_a = stream.FrameStylizer(eng, A, H, W, use_graph=use_graph)
        one_b = stream.FrameStylizer(eng, B, H, W, use_graph=use_graph)
        for f in frames_of(H, W, n_frames(eng), 21):
            mixed(f)
            ya, yb = mixed.net_output(), mixed.net_output2()
            one_b(f)
            one_a(f)
            assert mixed.last_forwards() == ("a", "b")
            assert same(ya, one_a.net_output()) and same(yb, one_b.net_output()) and not same(ya, yb)
            assert same(mixed.mixed_output(), restated(mixed, 0.5))
        for s in (mixed, one_a, one_b):
            s.release()


# ================================================================ 2. the mixed tensor and the frame are the restatements
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_mixed_tensor_and_frame_are_the_restatements(eng, kind):
    """u8 and deep at the odd input size, whose output is larger than the input; jpeg and deep with a mask"""
    kw, odd = KINDS[kind]
    H, W = odd_size(eng) if odd else net_size(eng)
    mask = noise_mask(H, W) if kind in ("jpeg", "deep") else None
    A, B = models(eng)
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, A, H, W, use_graph=use_graph, mix=dict(variables=B, weight=0.3, mask=mask), **kw)
        assert st.mix == dict(mask=mask is not None) and st.out_shape[1:3] == net_size(eng) and st._mix_q8 == (77,)
        with pytest.raises(_lib.FaststyleError):
            st.mixed_output()                                                               # nothing has run yet
        for f in frames_of(H, W, n_frames(eng), 3):
            out = st(f)
            assert same(st.net_input()[0], f.astype(np.float32)) and st.last_forwards() == ("a", "b")
            m = st.mixed_output()
            assert m.shape == st.out_shape and same(m, restated(st, 0.3, mask))
            assert not same(m, f32_of_F(to88(st.net_output()))) and not same(m, f32_of_F(to88(st.net_output2())))
            assert same_frame(out, expected_frame(st, kind, m[0]))
        st.release()


# ================================================================ 3. weight 0 and weight 1 are the one-model lanes, byte for byte
@pytest.mark.parametrize("kind", ["u8", "jpeg", "yuv8"])
def test_weight_zero_and_one_return_the_one_model_lanes_bytes(eng, kind):
    kw = KINDS[kind][0]
    H, W = net_size(eng)
    A, B = models(eng)
    g = not on_emulator(eng)
    frames = frames_of(H, W, n_frames(eng), 5)
    ref = {"a": stream.FrameStylizer(eng, A, H, W, use_graph=g, **kw), "b": stream.FrameStylizer(eng, B, H, W, use_graph=g, **kw)}
    want = {k: [s(f) for f in frames] for k, s in ref.items()}
    assert not same_frame(want["a"][0], want["b"][0])
    for t, live in ((0.0, "a"), (1.0, "b")):
        st = stream.FrameStylizer(eng, A, H, W, use_graph=g, mix=dict(variables=B, weight=t), **kw)
        for f, w in zip(frames, want[live]):
            assert same_frame(st(f), w) and st.last_forwards() == (live,)
        with pytest.raises(_lib.FaststyleError):
            st.net_output2() if live == "a" else st.net_output()                            # (the model that did not run has no output)
        assert sorted(st._mix_graphs) == ([(live, False)] if g else [])
        st.release()
    # a mask keeps model A live at weight 1, a weight in between both; a mask at weight 0 runs A alone and returns its bytes
    mask = noise_mask(H, W)
    if kind == "u8":
        for opt, live in ((dict(weight=1.0, mask=mask), ("a", "b")), (dict(weight=0.004), ("a", "b")), (dict(weight=0.0, mask=mask), ("a",))):
            st = stream.FrameStylizer(eng, A, H, W, use_graph=g, mix=dict(variables=B, **opt), **kw)
            out = st(frames[0])
            assert st.last_forwards() == live and same(st.mixed_output(), restated(st, opt["weight"], opt.get("mask")))
            assert same_frame(out, want["a"][0]) == (live == ("a",))
            st.release()
    for s in ref.values():
        s.release()


# ================================================================ 4. a fade through one lane
def test_set_mix_through_one_lane_changes_weights_and_liveness(eng):
    H, W = net_size(eng)
    A, B = models(eng)
    plan = [(0.0, ("a",)), (0.0, ("a",)), (0.5, ("a", "b")), (1.0, ("b",)), (1.0, ("b",)), (0.0, ("a",))]
    frames = frames_of(H, W, len(plan), 7)
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, A, H, W, use_graph=use_graph, mix=dict(variables=B, weight=0.25))
        for f, (t, live) in zip(frames, plan):
            st.set_mix(t)
            out = st(f)
            assert st.last_forwards() == live
            m = st.mixed_output()
            assert same(m, restated(st, t)) and same_frame(out, expected_frame(st, "u8", m[0]))
            if len(live) == 1:                                                              # weight 0 and 1: to88 of the live model's output
                assert same(m, f32_of_F(to88(st.net_output() if live == ("a",) else st.net_output2())))
        if use_graph:                                                                       # one head per kind, each captured when it first occurred
            assert sorted(st._mix_graphs) == [("a", False), ("ab", False), ("b", False)] and st._graph is None
        st.release()


def test_jpeg_frames_take_the_heads_of_their_own(eng):
    """A lane fed JPEG files captures its heads ahead of the upload, one per liveness kind: the frames are those of the same lane fed the
    decoded pixels"""
    import io
    from PIL import Image
    from tests.test_jpeg import encode, picture
    H, W = 44, 52                                                                           # (no multiple of the 16 x 16 MCU)
    A, B = models(eng)
    g = not on_emulator(eng)
    plan = [(0.5, ("a", "b"))] if on_emulator(eng) else [(0.5, ("a", "b")), (0.0, ("a",)), (1.0, ("b",)), (0.5, ("a", "b"))]
    files = [encode(picture("smooth", H, W, False, seed=35 + k), quality=90) for k in range(len(plan))]
    st = stream.FrameStylizer(eng, A, H, W, use_graph=g, mix=dict(variables=B), source=stream.jpeg_source(eng, files[0]))
    pix = stream.FrameStylizer(eng, A, H, W, use_graph=g, mix=dict(variables=B))
    for data, (t, live) in zip(files, plan):
        for s in (st, pix):
            s.set_mix(t)
        got, want = st(data), pix(np.array(Image.open(io.BytesIO(data)).convert("RGB")))
        assert np.array_equal(got, want) and st.last_forwards() == live and same(st.mixed_output(), restated(st, t))
    if g:
        assert sorted(st._mix_graphs) == [("a", True), ("ab", True), ("b", True)] and sorted(pix._mix_graphs) == [("a", False), ("ab", False), ("b", False)]
    for s in (st, pix):
        s.release()


# ================================================================ 5. with compose= and temporal=
def test_compose_and_temporal_read_the_mixed_tensor(eng):
    """Five frames, four of them around a reset(): the composed tensor is compose's restatement of the mixed one, and the stabilised tensor the temporal
    restatement chained over the composed ones"""
    H, W = SIZE[True]
    A, B = models(eng)
    frames = sequence(H, W, 4, 5)
    weights = (0.5, 0.75, 0.75, 0.2, 0.2)
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, A, H, W, use_graph=use_graph, mix=dict(variables=B, weight=0.5), compose=dict(strength=0.7, keep_color=True),
                                  temporal=dict(strength=0.6, sensitivity=4, radius=3, source_bgr=False, overlap=1))
        t, c = st.temporal, st.compose
        prev = None
        for k, f in enumerate(frames):
            if k == 3:
                st.reset()
                prev = None
            st.set_mix(weights[k])
            out = st(f)
            m = st.mixed_output()
            assert st.last_forwards() == ("a", "b") and same(m, restated(st, weights[k]))
            composed = st.composed_output()
            assert same(composed, compose_ref(st.net_input(), m, q8=c["strength_q8"], keep=True, matrix=c["matrix"], bgr=st.swap_rb))
            want = obmc_ref(st.net_input()[0], composed[0], prev=prev, q8=t["strength_q8"], K=t["sensitivity"], R=t["radius"], matrix=t["matrix"],
                            bgr=t["source_bgr"])
            stab = st.stabilised_output()
            assert same(stab[0], want["dst"]) and same_frame(out, expected_frame(st, "u8", stab[0]))
            assert same(stab, f32_of_F(to88(composed))) == (k in (0, 3))
            prev = (want["luma"], want["out88"], want["lumas"])
        st.release()


# ================================================================ 6. consecutive frames per pass, a weight per frame
def test_a_sequence_lane_takes_a_weight_per_frame(eng):
    H, W = SIZE[False]
    A, B = models(eng)
    frames = sequence(H, W, 6, 7) + sequence(H, W, 7, 1)
    plan = [((0.0, 0.0, 0.0, 0.0), ("a",)), ((0.0, 0.25, 0.5, 1.0), ("a", "b"))]
    if not on_emulator(eng):
        plan.append(((1.0, 1.0, 1.0, 1.0), ("b",)))
        frames = frames + frames[:4]
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, A, H, W, batch=4, use_graph=use_graph, mix=dict(variables=B),
                                  temporal=dict(strength=0.6, overlap=1, sequence=True))
        t = st.temporal
        prev = None
        for (batch, _), (ws, live) in zip(passes_of(frames, 4), plan):
            st.set_mix(ws)
            out = st(batch)
            m = st.mixed_output()
            assert st.last_forwards() == live and m.shape == (4, HO, WO, 3) and same(m, restated(st, ws))
            stab = st.stabilised_output()
            for i in range(4):
                want = obmc_ref(st.net_input()[i], m[i], prev=prev, q8=t["strength_q8"], K=t["sensitivity"], R=t["radius"], matrix=t["matrix"],
                                bgr=t["source_bgr"])
                assert same(stab[i], want["dst"]) and same_frame(out[i], expected_frame(st, "u8", stab[i]))
                prev = (want["luma"], want["out88"], want["lumas"])
        st.release()


# ================================================================ 7. pipelined lanes
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3])
def test_pipelined_lanes_equal_the_one_lane_results_with_weights_changing_per_frame(depth):
    eng = get_engine("hip")
    A, B = models(eng)
    weights = [0.0, 0.0, 0.3, 0.6, 1.0, 1.0, 0.1]
    # plain lanes: a weight per frame
    H, W = odd_size(eng)
    kw = dict(mix=dict(variables=B, weight=0.5, mask=noise_mask(H, W, 11) if depth == 3 else None))
    frames = frames_of(H, W, len(weights), 8)
    single = stream.FrameStylizer(eng, A, H, W, **kw)
    ps = stream.PipelinedStylizer(eng, A, H, W, depth=depth, **kw)
    want = []
    for f, t in zip(frames, weights):
        single.set_mix(t)
        want.append(single(f))
    assert len({w.tobytes() for w in want}) == len(want)                                    # distinct frames: an order mix-up cannot pass
    got = []
    for f, t in zip(frames, weights):
        if ps.in_flight >= depth:
            got.append(ps.fetch())
        ps.set_mix(t)
        ps.submit(f)
    while ps.in_flight:
        got.append(ps.fetch())
    assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert all(ln._ws2 is not ps.lanes[0]._ws2 and ln._mixed is not ps.lanes[0]._mixed and ln._mix_w is not ps.lanes[0]._mix_w and
               ln._mix_stage[1] is not ps.lanes[0]._mix_stage[1] for ln in ps.lanes[1:])
    for s in (single, ps):
        s.release()
    # temporal=, and a sequence lane with the weights of two consecutive frames per pass
    H, W = SIZE[True]
    frames = sequence(H, W, 8, 7)
    for extra, items, ws in ((dict(temporal=dict(strength=0.8, sensitivity=4)), frames, weights),
                             (dict(batch=2, temporal=dict(strength=0.8, sensitivity=4, sequence=True)), [b for b, _ in passes_of(frames, 2)],
                              [(0.0, 0.0), (0.0, 0.5), (1.0, 1.0), (1.0, 0.2)])):
        kw = dict(mix=dict(variables=B), **extra)
        single = stream.FrameStylizer(eng, A, H, W, **kw)
        ps = stream.PipelinedStylizer(eng, A, H, W, depth=depth, **kw)
        want, got = [], []
        for f, t in zip(items, ws):
            single.set_mix(t)
            want.append(single(f))
            if ps.in_flight >= depth:
                got.append(ps.fetch())
            ps.set_mix(t)
            ps.submit(f)
        while ps.in_flight:
            got.append(ps.fetch())
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
        for s in (single, ps):
            s.release()


# ================================================================ 8. what a lane refuses, and a lane without the stage
def test_mix_options_that_are_refused(eng):
    H, W = net_size(eng)
    A, B = models(eng)
    ok = np.zeros((H, W), np.uint8)
    for opt in (dict(variables=B, wieght=0.5), dict(variables=B, strength=0.5), dict(weight=0.5), dict(variables=None), dict(variables=B, weight=-0.1),
                dict(variables=B, weight=1.5), dict(variables=B, weight=float("nan")), dict(variables=B, weight="much"),
                dict(variables=B, weight=(0.5, 0.5)), dict(variables=B, weight=()), dict(variables=B, mask=np.zeros((H, W + 1), np.uint8)),
                dict(variables=B, mask=np.zeros((W, H), np.uint8)), dict(variables=B, mask=np.zeros((H, W, 1), np.uint8)),
                dict(variables=B, mask=ok.astype(np.float32)), dict(variables=B, mask=ok.astype(bool))):
        with pytest.raises(_lib.FaststyleError):
            stream.FrameStylizer(eng, A, H, W, use_graph=False, mix=opt)
    # floor(t * 256 + 0.5), per frame of a batch
    st = stream.FrameStylizer(eng, A, H, W, batch=2, use_graph=False, mix=dict(variables=B, weight=(0.3, 1), mask=ok))
    assert st._mix_q8 == (77, 256) and st.mix == dict(mask=True) and tuple(st._mixed.shape) == st.out_shape
    for t, q8 in ((0.0, (0, 0)), (0.002, (1, 1)), ((0.5, 0.998), (128, 255)), ([0.9999, 0.001], (256, 0))):
        st.set_mix(t)
        assert st._mix_q8 == q8
    for bad in (-0.1, 1.5, float("nan"), "much", (0.5,), (0.1, 0.2, 0.3), [[0.1, 0.2]], (0.5, 2.0), (0.5, float("nan"))):
        with pytest.raises(_lib.FaststyleError):
            st.set_mix(bad)
    assert st._mix_q8 == (256, 0)                                                           # (a refused call changes nothing)
    with pytest.raises(_lib.FaststyleError):
        st.last_forwards()                                                                  # nothing has run yet
    st.release()


def test_a_lane_without_the_stage_has_none_of_it(eng):
    from tests.test_frame_source import plain_stylizer
    H, W = net_size(eng)
    st = plain_stylizer(eng, H, W)
    st(np.zeros((H, W, 3), np.uint8))
    assert st.mix is None and st._mixed is None and not hasattr(st, "_ws2") and not hasattr(st, "_mix_graphs")
    assert (st._graph is not None) == (not on_emulator(eng))
    for call in (st.mixed_output, st.net_output2, st.last_forwards, lambda: st.set_mix(0.5)):
        with pytest.raises(_lib.FaststyleError):
            call()
