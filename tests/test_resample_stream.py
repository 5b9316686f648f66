"""The fp32 resampler in the frame lanes (faststyle_amd/stream.py): deliver= between the tensor the output conversions would read and every
output conversion, and source resample= between a deep source's fp32 image and the net's input.  Every comparison is exact and independent
of the net's numerics: the delivery tensor is the numpy restatement's (tests/test_resample.py) of the top-left H x W of the same lane's
net_output() / composed_output() / stabilised_output(), and the frame that comes back is the existing conversion's restatement of the delivery
tensor.  Sizes as tests/test_compose_stream.py."""
import numpy as np
import pytest

from faststyle_amd import _lib, stream
from tests.backends import engine_params, get_engine, on_emulator
from tests.test_compose_stream import KINDS, expected_frame, graph_modes, odd_size, restated, variables
from tests.test_frame_source import n_frames, net_size, plain_stylizer
from tests.test_resample import restate, same_bits
from tests.test_temporal_stream import sequence
from tests.test_video_deep import DEEP, EIGHT, ref_args, samples_of, u8_of
from tests.test_yuv_deep import frame_to_f32


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


def delivery(eng, which):
    """(Hd, Wd): even sizes (the 4:2:0 outputs), larger or smaller than the net's 48 x 56 / 96 x 136 on both axes, by factors that are no ratio
    of small numbers"""
    H, W = net_size(eng)
    return (H * 3 // 2 - 2, W * 3 // 2 + 6) if which == "larger" else (H * 2 // 3, W * 3 // 4 - 2)


def delivered_ref(st, tensor):
    """The restatement of the lane's delivery stage on a host copy [B, Ho, Wo, 3] of the tensor it read"""
    H, W = st.shape[1:3]
    d = st.deliver
    return restate(tensor[:, :H, :W], d["height"], d["width"], d["filter"])


@pytest.mark.parametrize("which,filt", [("larger", "bicubic"), ("smaller", "lanczos")])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_deliver_through_every_output(eng, kind, which, filt):
    kw, odd = KINDS[kind]
    H, W = odd_size(eng) if odd else net_size(eng)
    Hd, Wd = delivery(eng, which)
    rng = np.random.default_rng(13)
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, deliver=dict(height=Hd, width=Wd, filter=filt), **kw)
        assert st.deliver == dict(height=Hd, width=Wd, filter=filt) and st.delivery_shape == (1, Hd, Wd, 3)
        assert st.out_shape[1:3] == net_size(eng) and st._deliver_plan.src_shape == (H, W)
        if st.yuv_out_desc is not None:
            assert (st.yuv_out_desc.height, st.yuv_out_desc.width) == (Hd, Wd)
        with pytest.raises(_lib.FaststyleError):
            st.delivered_output()                                                           # nothing has run yet
        for _ in range(n_frames(eng)):
            out = st(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
            got = st.delivered_output()
            assert got.shape == st.delivery_shape and same_bits(got, delivered_ref(st, st.net_output()))
            want = expected_frame(st, kind, got[0])
            assert out == want if kind == "jpeg" else (out.dtype == np.uint8 and np.array_equal(out, want))
            if kind == "u8":
                assert out.shape == (Hd, Wd, 3)
        st.release()


def test_deliver_default_filter_is_bicubic_and_equal_size_copies_the_crop(eng):
    H, W = odd_size(eng)
    st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=not on_emulator(eng), deliver=dict(height=H, width=W))
    assert st.deliver["filter"] == "bicubic" and st.delivery_shape == (1, H, W, 3) and st.out_shape[1:3] == net_size(eng)
    out = st(np.random.default_rng(14).integers(0, 256, (H, W, 3), dtype=np.uint8))
    y = st.net_output()
    assert same_bits(st.delivered_output(), y[:, :H, :W]) and np.array_equal(out, u8_of(y[0, :H, :W], True))
    st.release()


def test_deliver_reads_the_composed_tensor(eng):
    H, W = odd_size(eng)
    Hd, Wd = delivery(eng, "larger")
    rng = np.random.default_rng(15)
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, compose=dict(strength=0.6, keep_color=True),
                                  deliver=dict(height=Hd, width=Wd, filter="bilinear"))
        for _ in range(n_frames(eng)):
            out = st(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
            composed = st.composed_output()
            assert composed.shape == st.out_shape and same_bits(composed, restated(st))     # compose stays on the net's grid
            got = st.delivered_output()
            assert same_bits(got, delivered_ref(st, composed)) and not same_bits(got, delivered_ref(st, st.net_output()))
            assert np.array_equal(out, u8_of(got[0], True))
        st.release()


def test_deliver_behind_temporal_over_a_sequence_around_a_reset(eng):
    """Four frames, reset() before the third: the first-frame tail twice and one parity's (GPU: each a graph of its own that carries the stage)."""
    H, W = odd_size(eng)
    Hd, Wd = delivery(eng, "smaller")
    frames = sequence(H, W, 16, 4)
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, temporal=dict(strength=0.6),
                                  deliver=dict(height=Hd, width=Wd, filter="box"))
        ref = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, temporal=dict(strength=0.6))
        for k, f in enumerate(frames):
            if k == 2:
                st.reset()
                ref.reset()
            out = st(f)
            ref(f)
            stab = st.stabilised_output()
            assert stab.shape == st.out_shape and same_bits(stab, ref.stabilised_output())  # the stage and its state stay on the net's grid
            got = st.delivered_output()
            assert same_bits(got, delivered_ref(st, stab)) and np.array_equal(out, u8_of(got[0], True))
        if use_graph:
            assert sorted(st._tail_graphs, key=str) == [1, None]
        for s in (st, ref):
            s.release()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [2, 3])
def test_pipelined_lanes_equal_one_lane_in_order(depth):
    eng = get_engine("hip")
    H, W = odd_size(eng)
    Hd, Wd = delivery(eng, "larger")
    kw = dict(temporal=dict(strength=0.8, sensitivity=4), compose=dict(strength=0.9), deliver=dict(height=Hd, width=Wd, filter="lanczos"))
    frames = sequence(H, W, 17, 7)
    single = stream.FrameStylizer(eng, variables(eng), H, W, **kw)
    ps = stream.PipelinedStylizer(eng, variables(eng), H, W, depth=depth, **kw)
    want = [single(f) for f in frames]
    assert want[0].shape == (Hd, Wd, 3) and len({w.tobytes() for w in want[1:]}) == 6
    got = list(ps.run(frames))
    assert len(got) == 7 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert all(ln.delivery_shape == (1, Hd, Wd, 3) and ln._delivered is not ps.lanes[0]._delivered for ln in ps.lanes[1:])
    for s in (single, ps):
        s.release()


def test_a_lane_without_the_keys_has_none_of_it(eng):
    H, W = net_size(eng)
    st = plain_stylizer(eng, H, W)
    frame = np.random.default_rng(18).integers(0, 256, (H, W, 3), dtype=np.uint8)
    out = st(frame)
    assert st.deliver is None and st._deliver_plan is None and st._delivered is None and st.delivery_shape == st.out_shape
    assert st._src_rplan is None and st._src_f32 is None
    assert np.array_equal(out, u8_of(st.net_output()[0], True))
    with pytest.raises(_lib.FaststyleError):
        st.delivered_output()
    none = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=not on_emulator(eng), deliver=None)
    assert none.deliver is None and none._delivered is None and np.array_equal(none(frame), out)
    none.release()


@pytest.mark.gpu
def test_the_graph_of_a_lane_without_the_key_has_one_node_less():
    from tests.test_generations import graph_node_types
    eng = get_engine("hip")
    H, W = net_size(eng)
    frame = np.random.default_rng(19).integers(0, 256, (H, W, 3), dtype=np.uint8)
    stream.FrameStylizer.KEEP_GRAPH = True
    try:
        plain = stream.FrameStylizer(eng, variables(eng), H, W)
        again = stream.FrameStylizer(eng, variables(eng), H, W, deliver=None)
        with_stage = stream.FrameStylizer(eng, variables(eng), H, W, deliver=dict(height=H + 10, width=W + 10))
        outs = [s(frame) for s in (plain, again, with_stage)]
        n = [len(graph_node_types(s._graph)) for s in (plain, again, with_stage)]
        assert n[0] == n[1] and n[2] == n[0] + 1, n
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], plain_stylizer(eng, H, W)(frame))
        for s in (plain, again, with_stage):
            s.release()
    finally:
        stream.FrameStylizer.KEEP_GRAPH = False


def test_a_deep_source_of_another_size_with_resample(eng):
    H, W = net_size(eng)
    Hs, Ws = 2 * H, 2 * W
    opt = DEEP["420p10"]
    a = ref_args(opt)
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph, swap_rb=False,
                                  source=dict(height=Hs, width=Ws, swap_rb=True, yuv=opt, resample="bicubic"))
        assert st.source["resample"] == "bicubic" and st._src_deep and st._src_plan is None and st._src_rplan.src_shape == (Hs, Ws)
        assert st.in_shape == (1, int(st._src_yuv.frame_bytes)) and tuple(st._src_f32.shape) == (1, Hs, Ws, 3)
        for k in range(n_frames(eng)):
            s = samples_of(opt, Ws, Hs, 60 + k)
            out = st(s)
            want = restate(frame_to_f32(s, Ws, Hs, swap=True, **a), H, W, "bicubic")
            assert same_bits(st.net_input()[0], want)
            assert np.array_equal(out, u8_of(st.net_output()[0], False))
        st.release()
    with pytest.raises(_lib.FaststyleError):                                                # without the key: refused as before
        stream.FrameStylizer(eng, variables(eng), H, W, use_graph=False, source=dict(height=Hs, width=Ws, swap_rb=True, yuv=opt))
    # the key with a source of the net's size: the lane it is without it
    st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=False, source=dict(height=H, width=W, yuv=opt, resample="lanczos"))
    assert st._src_rplan is None and st._src_f32 is None and st._src_deep
    st.release()


def test_a_small_deep_source_into_a_small_net(eng):
    """10-bit 48 x 64 into a 24 x 32 net -- where the net takes that size"""
    try:
        eng.tnet_out_shape(24, 32)
    except _lib.FaststyleError:
        H, W, Hs, Ws = 48, 64, 96, 128                                                      # (REFLECT padding needs a larger input: the same factor)
    else:
        H, W, Hs, Ws = 24, 32, 48, 64
    opt = DEEP["420p10"]
    st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=not on_emulator(eng), source=dict(height=Hs, width=Ws, yuv=opt, resample="bilinear"))
    s = samples_of(opt, Ws, Hs, 70)
    st(s)
    assert same_bits(st.net_input()[0], restate(frame_to_f32(s, Ws, Hs, **ref_args(opt)), H, W, "bilinear"))
    st.release()


def test_lane_refusals(eng):
    H, W = net_size(eng)
    v = variables(eng)
    for opt in (dict(height=60), dict(width=60), dict(height=60, width=70, size=3), dict(height=60, width=70, filter="nearest"),
                dict(height=60, width=70, filter=2), dict(height=0, width=70), dict(height=60, width=-1), dict(height=60.0, width=70),
                dict(height="60", width=70), dict(height=True, width=70), dict(height=60, width=None), dict(height=40000, width=70)):
        with pytest.raises(_lib.FaststyleError):
            stream.FrameStylizer(eng, v, H, W, use_graph=False, deliver=opt)
    with pytest.raises(_lib.FaststyleError):                                                # a plan the library refuses: 96 rows into one
        stream.FrameStylizer(eng, v, 96, 56, use_graph=False, deliver=dict(height=1, width=56, filter="lanczos"))
    deep = DEEP["420p10"]
    for src in (dict(height=2 * H, width=2 * W, resample="bicubic"),                                    # 8-bit pixel frames
                dict(height=2 * H, width=2 * W, yuv=EIGHT, resample="bicubic"),                         # 8-bit planes
                dict(height=H, width=W, yuv=dict(EIGHT, bits=8), resample="bicubic"),
                dict(height=2 * H, width=2 * W, yuv=deep, resample="nearest"),
                dict(height=2 * H, width=2 * W, yuv=deep, resample=None),
                dict(height=2 * H, width=2 * W, yuv=deep, resampel="bicubic"),
                dict(height=2 * H, width=2 * W, yuv=deep)):                                             # the refusal that was there before
        with pytest.raises(_lib.FaststyleError):
            stream.FrameStylizer(eng, v, H, W, use_graph=False, source=src)
    with pytest.raises(_lib.FaststyleError) as e:
        stream.FrameStylizer(eng, v, H, W, use_graph=False, source=dict(height=2 * H, width=2 * W, yuv=EIGHT, resample="bicubic"))
    assert "8-bit" in str(e.value) and "interpolation" in str(e.value)
