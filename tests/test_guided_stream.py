"""Guided delivery in the frame lanes (faststyle_amd/stream.py, deliver=dict(guided=)): fs_guided_f32 between the tensor the output
conversions would read and every output conversion, guided by the source at its own size.  Every comparison is exact and independent of the
net's numerics: the delivery tensor is the numpy restatement's (tests/test_guided.py) of the lane's own tensors -- net_input(), the tensor
the stage received and the buffer the lane holds the full-size source in -- and the frame that comes back is the existing conversion's
restatement of the delivery tensor.  A 48 x 64 net from a 96 x 128 source, the smallest the net's reflection padding takes."""
import io

import numpy as np
import pytest
from PIL import Image

from faststyle_amd import _lib, stream
from tests.backends import engine_params, get_engine, on_emulator
from tests.test_compose import same, to88
from tests.test_compose_stream import expected_frame, graph_modes, restated, variables
from tests.test_frame_source import n_frames
from tests.test_guided import box, guided_ref, hi88, luma_of
from tests.test_video_deep import DEEP, EIGHT, ref_args
from tests.test_yuv import rgb_to_frame
from tests.test_yuv_deep import f32_to_frame

H, W, HS, WS = 48, 64, 96, 128
GUIDED = dict(radius=2, smoothness=4, matrix=0)                 # what a lane's guided dict holds beside lo_bgr, by default


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


def coloured(seed, dy=0, dx=0):
    """A 96 x 128 uint8 picture with edges whose channel 0 and channel 2 lie far apart (200..255 against 0..55), so that a luma that weighs
    the wrong one of them is another picture"""
    rng = np.random.default_rng(seed)
    y, x = np.indices((HS, WS))
    y, x = y + dy, x + dx
    step = (((x // 11 + y // 9) % 2) * 40).astype(np.int64)
    c0 = 200 + step // 2 + rng.integers(0, 16, (HS, WS))
    c1 = 60 + 2 * step + ((x + y) // 17 % 2) * 60 + rng.integers(0, 16, (HS, WS))
    c2 = 35 - step // 2 + rng.integers(0, 16, (HS, WS))
    return np.stack([c0, c1, c2], axis=-1).astype(np.uint8)


def jpeg_of(frame):
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=90, subsampling=2)
    return buf.getvalue()


DEEP10 = DEEP["420p10"]
# source kind -> (lane options, the frame the lane takes for a picture, hi_kind, lo_bgr, hi_bgr): the flags as they follow from where R and B
# are exchanged -- for the u8 buffers in the resize behind them, for the deep fp32 source in the conversion in front of it
SOURCES = {
    "pixels": (dict(source=dict(height=HS, width=WS)), lambda eng, p: p, 0, True, True),
    "pixels_swapped": (dict(source=dict(height=HS, width=WS, swap_rb=True)), lambda eng, p: p, 0, True, False),
    "yuv8": (dict(swap_rb=False, source=dict(height=HS, width=WS, swap_rb=True, yuv=EIGHT)),
             lambda eng, p: rgb_to_frame(p, **ref_args(EIGHT)), 1, True, False),
    "jpeg": (dict(), lambda eng, p: jpeg_of(p), 1, True, False),
    "deep": (dict(swap_rb=False, source=dict(height=HS, width=WS, swap_rb=True, yuv=DEEP10, resample="bicubic")),
             lambda eng, p: f32_to_frame(p.astype(np.float32), **ref_args(DEEP10)), 2, True, True),
}
OUTPUTS = {"u8": dict(), "jpeg": dict(jpeg=dict(quality=90, subsampling=2)), "yuv8": dict(yuv_out=EIGHT), "deep": dict(yuv_out=DEEP10)}


def lane(eng, skind, okind="u8", use_graph=False, guided=None, **more):
    kw = dict(SOURCES[skind][0])
    if skind == "jpeg":
        kw["source"] = stream.jpeg_source(eng, jpeg_of(coloured(0)), swap_rb=True)
    g = dict(guided or {})
    if "swap_rb" in kw:                                         # (the lanes of the command line: the net is fed B,G,R, the output not swapped)
        g.setdefault("source_bgr", True)
    kw.update(OUTPUTS[okind])
    kw.update(more)
    return stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, deliver=dict(height=HS, width=WS, guided=g), **kw)


def guide_of(st, jpeg_in=False):
    """A host copy of the buffer the lane holds the full-size source in"""
    return np.array(st.eng.mem.to_numpy(st._guided_src[jpeg_in][0]), copy=True)


def delivered_ref(st, tensor, skind):
    """The restatement of the lane's stage on a host copy [1, Ho, Wo, 3] of the tensor it read; the channel flags are SOURCES', not the lane's"""
    _, _, kind, lo_bgr, hi_bgr = SOURCES[skind]
    hi = guide_of(st, skind == "jpeg")
    assert hi.shape == (1, HS, WS, (3, 4, 3)[kind]) and hi.dtype == (np.float32 if kind == 2 else np.uint8)
    g = st._guided
    # both lumas weigh the same physical channel: the guide's luma, box-averaged to the net's grid, is the net input's luma (the resize apart);
    # with either flag wrong the two differ by the distance between channel 0 and channel 2
    lo = luma_of(to88(st.net_input()[0]), g["matrix"], lo_bgr)
    up = luma_of(hi88(hi[0]), g["matrix"], hi_bgr).reshape(H, 2, W, 2).mean(axis=(1, 3))
    wrong = luma_of(hi88(hi[0]), g["matrix"], not hi_bgr).reshape(H, 2, W, 2).mean(axis=(1, 3))
    assert np.abs(lo - up).mean() < 8 * 256 and np.abs(lo - wrong).mean() > 24 * 256
    return guided_ref(st.net_input(), tensor, hi, r=g["radius"], E=g["smoothness"], matrix=g["matrix"], lo_bgr=lo_bgr, hi_bgr=hi_bgr)["dst"]


def check(st, skind, okind, out, tensor):
    got = st.delivered_output()
    assert got.shape == (1, HS, WS, 3) and same(got, delivered_ref(st, tensor, skind))
    want = expected_frame(st, okind, got[0])
    assert out == want if okind == "jpeg" else (out.dtype == np.uint8 and np.array_equal(out, want))
    return got


PAIRS = [("pixels", "u8"), ("pixels", "deep"), ("pixels_swapped", "jpeg"), ("yuv8", "yuv8"), ("yuv8", "u8"), ("jpeg", "u8"), ("jpeg", "yuv8"),
         ("deep", "deep"), ("deep", "jpeg")]


@pytest.mark.parametrize("skind,okind", PAIRS)
def test_every_source_and_every_output(eng, skind, okind):
    for use_graph in graph_modes(eng):
        st = lane(eng, skind, okind, use_graph)
        assert st.deliver == dict(height=HS, width=WS, guided=dict(GUIDED, lo_bgr=True)) and st.delivery_shape == (1, HS, WS, 3)
        assert st._deliver_plan is None and st.out_shape[1:3] == (H, W) and st._guided_src[skind == "jpeg"][1] == SOURCES[skind][4]
        for k in range(n_frames(eng)):
            out = st(SOURCES[skind][1](eng, coloured(20 + k)))
            got = check(st, skind, okind, out, st.net_output())
            assert not same(got[0, ::2, ::2], st.net_output()[0])                              # (the stage did something)
        st.release()


def test_pixel_frames_into_a_jpeg_lane_take_the_pixel_buffer(eng):
    """a lane built for JPEG files also takes pixels (a file the decoder does not take): their guide is the pixel buffer, kind 0"""
    st = lane(eng, "jpeg", "u8", False)                         # (eagerly: net_output() is then the pass just run, whichever kind it was)
    outs = []
    for k in range(n_frames(eng)):
        outs.append(st(jpeg_of(coloured(30 + k))))
        check(st, "jpeg", "u8", outs[-1], st.net_output())
        outs.append(st(coloured(32 + k)))
        got = st.delivered_output()
        assert guide_of(st).shape == (1, HS, WS, 3) and np.array_equal(guide_of(st)[0], coloured(32 + k))
        want = guided_ref(st.net_input(), st.net_output(), guide_of(st), r=2, E=4, lo_bgr=True, hi_bgr=False)["dst"]
        assert same(got, want) and np.array_equal(outs[-1], expected_frame(st, "u8", got[0]))
    st.release()
    if not on_emulator(eng):                                    # through the two graphs of such a lane: the same frames
        st = lane(eng, "jpeg", "u8", True)
        for k in range(n_frames(eng)):
            assert np.array_equal(st(jpeg_of(coloured(30 + k))), outs[2 * k]) and np.array_equal(st(coloured(32 + k)), outs[2 * k + 1])
        st.release()


def test_parameters_reach_the_launch(eng):
    st = lane(eng, "pixels", "u8", not on_emulator(eng), guided=dict(radius=8, smoothness=64, matrix="bt709", source_bgr=False), swap_rb=False)
    assert st._guided == dict(radius=8, smoothness=64, matrix=1, lo_bgr=False) and st._guided_src[False][1] is False
    out = st(coloured(40)[..., ::-1])
    got = st.delivered_output()
    want = guided_ref(st.net_input(), st.net_output(), guide_of(st), r=8, E=64, matrix=1, lo_bgr=False, hi_bgr=False)["dst"]
    assert same(got, want) and np.array_equal(out, expected_frame(st, "u8", got[0]))
    st.release()


def test_the_stage_reads_the_composed_tensor(eng):
    for use_graph in graph_modes(eng):
        st = lane(eng, "pixels", "u8", use_graph, compose=dict(strength=0.6, keep_color=True))
        for k in range(n_frames(eng)):
            out = st(coloured(50 + k))
            composed = st.composed_output()
            assert same(composed, restated(st))                                                # compose stays on the net's grid
            got = check(st, "pixels", "u8", out, composed)
            assert not same(got, delivered_ref(st, st.net_output(), "pixels"))
        st.release()


def test_behind_temporal_over_a_sequence_around_a_reset(eng):
    """Four frames, reset() before the third: the stage sits in the tail, reads the stabilised tensor and the source of the same frame"""
    frames = [coloured(60), coloured(60), coloured(60, 2, -3), coloured(61)]
    for use_graph in graph_modes(eng):
        st = lane(eng, "yuv8", "yuv8", use_graph, temporal=dict(strength=0.6, source_bgr=True))
        ref = None if on_emulator(eng) else stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph,        # (the emulator: a forward less a frame)
                                                                 temporal=dict(strength=0.6, source_bgr=True), **SOURCES["yuv8"][0])
        for k, f in enumerate(frames):
            if k == 2:
                st.reset()
            planes = SOURCES["yuv8"][1](eng, f)
            out = st(planes)
            stab = st.stabilised_output()
            if ref is not None:                                                                # the stage and its state stay on the net's grid
                if k == 2:
                    ref.reset()
                ref(planes)
                assert same(stab, ref.stabilised_output())
            check(st, "yuv8", "yuv8", out, stab)
        if use_graph:
            assert sorted(st._tail_graphs, key=str) == [1, None]
        for s in (st, ref):
            if s is not None:
                s.release()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3])
def test_pipelined_lanes_equal_one_lane_in_order(depth):
    eng = get_engine("hip")
    kw = dict(SOURCES["pixels"][0], temporal=dict(strength=0.8, sensitivity=4), compose=dict(strength=0.9),
              deliver=dict(height=HS, width=WS, guided=dict(radius=1)))
    frames = [coloured(70 + k // 2, k, -k) for k in range(7)]
    single = stream.FrameStylizer(eng, variables(eng), H, W, **kw)
    ps = stream.PipelinedStylizer(eng, variables(eng), H, W, depth=depth, **kw)
    want = [single(f) for f in frames]
    assert want[0].shape == (HS, WS, 3) and len({w.tobytes() for w in want}) == 7
    got = list(ps.run(frames))
    assert len(got) == 7 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert all(ln._guided_work is not ps.lanes[0]._guided_work and ln._delivered is not ps.lanes[0]._delivered for ln in ps.lanes[1:])
    for s in (single, ps):
        s.release()


def test_a_lane_without_the_key_has_none_of_it(eng):
    g = not on_emulator(eng)
    frame = coloured(80)
    plain = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, source=dict(height=HS, width=WS))
    resampled = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, source=dict(height=HS, width=WS), deliver=dict(height=HS, width=WS))
    for st in (plain, resampled):
        assert st._guided is None and st._guided_work is None and st._guided_src is None and "guided" not in (st.deliver or {})
    assert plain.deliver is None and resampled.deliver == dict(height=HS, width=WS, filter="bicubic") and resampled._deliver_plan is not None
    out = plain(frame)
    from tests.test_video_deep import u8_of
    assert np.array_equal(out, u8_of(plain.net_output()[0], True))
    resampled(frame)
    from tests.test_resample import restate, same_bits
    assert same_bits(resampled.delivered_output(), restate(resampled.net_output()[:, :H, :W], HS, WS, "bicubic"))
    for st in (plain, resampled):
        st.release()


@pytest.mark.gpu
def test_the_graph_of_a_guided_lane_has_two_nodes_more_than_a_resampling_one():
    from tests.test_generations import graph_node_types
    eng = get_engine("hip")
    frame = coloured(81)
    src = dict(source=dict(height=HS, width=WS))
    stream.FrameStylizer.KEEP_GRAPH = True
    try:
        plain = stream.FrameStylizer(eng, variables(eng), H, W, **src)
        again = stream.FrameStylizer(eng, variables(eng), H, W, deliver=None, **src)
        resampled = stream.FrameStylizer(eng, variables(eng), H, W, deliver=dict(height=HS, width=WS, filter="bilinear"), **src)
        guided = stream.FrameStylizer(eng, variables(eng), H, W, deliver=dict(height=HS, width=WS, guided=dict()), **src)
        outs = [s(frame) for s in (plain, again, resampled, guided)]
        n = [len(graph_node_types(s._graph)) for s in (plain, again, resampled, guided)]
        assert n[0] == n[1] and n[2] == n[0] + 1 and n[3] == n[2] + 2, n
        assert np.array_equal(outs[0], outs[1]) and outs[2].shape == outs[3].shape == (HS, WS, 3)
        for s in (plain, again, resampled, guided):
            s.release()
    finally:
        stream.FrameStylizer.KEEP_GRAPH = False


def test_lane_refusals(eng):
    v = variables(eng)
    src = dict(height=HS, width=WS)

    def refused(deliver, **kw):
        with pytest.raises(_lib.FaststyleError):
            stream.FrameStylizer(eng, v, H, W, use_graph=False, deliver=deliver, **kw)

    ok = dict(height=HS, width=WS)
    for g in (dict(radios=2), dict(radius=0), dict(radius=9), dict(radius=2.5), dict(radius=float("nan")), dict(radius="two"), dict(radius=None),
              dict(smoothness=0), dict(smoothness=65), dict(smoothness=4.5), dict(smoothness=float("nan")), dict(smoothness=float("inf")),
              dict(matrix="bt2020"), dict(matrix=2), dict(strength=1.0)):
        refused(dict(ok, guided=g), source=src)
    refused(dict(ok, guided=dict(), filter="bicubic"), source=src)                             # guided together with filter
    refused(dict(ok, guided=dict(), size=3), source=src)                                       # an unknown key beside it
    refused(dict(ok, guided=dict()))                                                           # no source
    refused(dict(height=HS + 2, width=WS, guided=dict()), source=src)                          # a source of another size than the delivery
    refused(dict(height=HS, width=WS - 2, guided=dict()), source=src)
    refused(dict(height=H, width=W, guided=dict()), source=dict(height=H, width=W))            # ... of the net's size: nothing to upsample
    refused(dict(height=H, width=W, guided=dict()), source=dict(height=H, width=W, swap_rb=True))
    refused(dict(height=H - 2, width=W - 2, guided=dict()), source=dict(height=H - 2, width=W - 2))   # delivery below the net's size
    refused(dict(width=WS, guided=dict()), source=src)                                         # the refusals that were there before
    refused(dict(height=0, width=WS, guided=dict()), source=src)
    refused(dict(ok, guided=dict()), source=dict(height=HS, width=WS, yuv=DEEP10))             # (a deep source that is not resampled: refused before)
    st = lane(eng, "pixels", guided=dict(radius=1.0, smoothness=64.0))                         # whole numbers given as floats are taken
    assert st._guided == dict(radius=1, smoothness=64, matrix=0, lo_bgr=True)
    st.release()
