"""The compose stage in the frame lanes (faststyle_amd/stream.py, compose=): strength, colour preservation and a region mask between the
forward pass and every output conversion.  Every comparison is exact and independent of the net's numerics: the composed tensor is the
numpy restatement's (tests/test_compose.py) of the same lane's net_input() and net_output(), and the frame that comes back is the existing
conversion's restatement of the composed tensor.  Shapes as tests/test_video_deep.py: 48 x 56 eager on the emulator, 96 x 136 on the GPU,
through the captured graph and eagerly, two frames there so that the second replays; plus 45 x 54 / 93 x 134, whose net output (48 x 56 /
96 x 136) is larger than the input."""
import numpy as np
import pytest

from faststyle_amd import _lib, stream
from tests.backends import engine_params, get_engine, on_emulator
from tests.test_compose import compose_ref, f32_of_F, same, to88
from tests.test_frame_source import n_frames, net_size, plain_stylizer
from tests.test_jpeg_encode import pil_encode, starry
from tests.test_video_deep import DEEP, EIGHT, ref_args, samples_of, u8_of
from tests.test_yuv import rgb_to_frame
from tests.test_yuv_deep import f32_to_frame


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


_vars = {}


def variables(eng):
    if id(eng) not in _vars:
        _vars[id(eng)] = starry(eng)[1]
    return _vars[id(eng)]


def odd_size(eng):
    """A net input whose output is 3 rows and 2 columns larger"""
    H, W = net_size(eng)
    return H - 3, W - 2


def graph_modes(eng):
    return (False,) if on_emulator(eng) else (True, False)


def replicated(a, Ho, Wo):
    """[..., H, W, 3] -> [..., Ho, Wo, 3]: the last row and column again"""
    H, W = a.shape[-3:-1]
    return a[..., np.minimum(np.arange(Ho), H - 1), :, :][..., np.minimum(np.arange(Wo), W - 1), :]


def noise_mask(H, W, seed=9):
    m = np.random.RandomState(seed).randint(0, 256, (H, W)).astype(np.uint8)
    m[0, :4] = (0, 127, 128, 255)
    return m


def restated(st, mask=None):
    """The restatement of the lane's compose stage applied to the tensors of its last pass"""
    c = st.compose
    return compose_ref(st.net_input(), st.net_output(), q8=c["strength_q8"], keep=c["keep_color"], matrix=c["matrix"], bgr=st.swap_rb,
                       mask=mask, src_swapped=c["source_swapped"])


# kind -> (lane options, odd-sized input)
KINDS = {"u8": (dict(), True), "jpeg": (dict(jpeg=dict(quality=90, subsampling=2)), False), "yuv8": (dict(yuv_out=EIGHT, swap_rb=False), False),
         "deep": (dict(yuv_out=DEEP["420p10"], swap_rb=False), True)}


def expected_frame(st, kind, composed):
    if kind == "u8":
        return u8_of(composed, st.swap_rb)
    if kind == "jpeg":
        return pil_encode(u8_of(composed, st.swap_rb), 90, 2)
    if kind == "yuv8":
        return rgb_to_frame(u8_of(composed, st.swap_rb), **ref_args(EIGHT))
    return f32_to_frame(composed, swap=st.swap_rb, **ref_args(DEEP["420p10"])).view(np.uint8)


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_composed_tensor_and_frame_are_the_restatements(eng, kind):
    kw, odd = KINDS[kind]
    H, W = odd_size(eng) if odd else net_size(eng)
    mask = noise_mask(H, W)
    rng = np.random.default_rng(3)
    for use_graph in graph_modes(eng):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=use_graph,
                                  compose=dict(strength=0.6, keep_color=kind in ("u8", "deep"), matrix="bt709", mask=mask), **kw)
        assert st.compose == dict(strength_q8=154, keep_color=kind in ("u8", "deep"), matrix=1, mask=True, source_swapped=False)
        assert st.out_shape[1:3] == net_size(eng)
        with pytest.raises(_lib.FaststyleError):
            st.composed_output()                                                            # nothing has run yet
        for _ in range(n_frames(eng)):
            frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            out = st(frame)
            assert same(st.net_input()[0], frame.astype(np.float32))
            composed = st.composed_output()
            assert composed.shape == st.out_shape and same(composed, restated(st, mask))
            assert not same(composed, f32_of_F(to88(st.net_output())))                      # (the stage did something)
            want = expected_frame(st, kind, composed[0])
            assert out == want if kind == "jpeg" else (out.dtype == np.uint8 and np.array_equal(out, want))
        st.release()


def test_a_swapped_source_is_read_with_r_and_b_exchanged(eng):
    """The lanes of the command line: a deep source written B,G,R, an output conversion that does not swap, source_swapped"""
    H, W = net_size(eng)
    opt = DEEP["420p10"]
    st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=not on_emulator(eng), swap_rb=False,
                              source=dict(height=H, width=W, swap_rb=True, yuv=opt), yuv_out=opt,
                              compose=dict(strength=0.5, keep_color=True, source_swapped=True))
    assert st.compose == dict(strength_q8=128, keep_color=True, matrix=0, mask=False, source_swapped=True)
    for k in range(n_frames(eng)):
        got = st(samples_of(opt, W, H, 80 + k))
        composed = st.composed_output()
        assert same(composed, compose_ref(st.net_input(), st.net_output(), q8=128, keep=True, matrix=0, bgr=False, src_swapped=True))
        assert np.array_equal(got.view("<u2"), f32_to_frame(composed[0], **ref_args(opt)))
    st.release()


def test_full_strength_reproduces_the_lane_without_the_stage(eng):
    """Plain mode, strength 1, no mask: F = B, and F >> 8 is what fs_f32_to_u8 writes -- the u8 frame, the JPEG bytes and the 8-bit planes
    are those of the same lane built without compose=, byte for byte."""
    H, W = net_size(eng)
    g = not on_emulator(eng)
    frame = np.random.default_rng(5).integers(0, 256, (H, W, 3), dtype=np.uint8)
    for kw in (dict(), dict(jpeg=dict(quality=90, subsampling=2)), dict(yuv_out=EIGHT, swap_rb=False)):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, compose=dict(strength=1.0), **kw)
        ref = plain_stylizer(eng, H, W) if not kw else stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, **kw)
        for _ in range(n_frames(eng)):
            got, want = st(frame), ref(frame)
            assert got == want if "jpeg" in kw else np.array_equal(got, want)
        assert same(st.composed_output(), f32_of_F(to88(st.net_output()))) and same(st.net_output(), ref.net_output())
        st.release()
        if kw:
            ref.release()


def test_strength_zero_returns_the_source(eng):
    H, W = odd_size(eng)
    Ho, Wo = net_size(eng)
    g = not on_emulator(eng)
    frame = np.random.default_rng(6).integers(0, 256, (H, W, 3), dtype=np.uint8)
    # a u8 lane: the source frame, replicated into the extra rows and columns (through the lane's own swap, if it swaps)
    for swap in (False, True):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, swap_rb=swap, compose=dict(strength=0.0, keep_color=swap))
        want = replicated(frame, Ho, Wo)
        assert np.array_equal(st(frame), want[:, :, ::-1] if swap else want)
        st.release()
        if on_emulator(eng):
            break
    # a deep lane: to88 of its input
    H, W = net_size(eng)
    opt = DEEP["420p10"]
    st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=g, swap_rb=False, source=dict(height=H, width=W, swap_rb=True, yuv=opt),
                              yuv_out=opt, compose=dict(strength=0.0))
    got = st(samples_of(opt, W, H, 90))
    A = f32_of_F(to88(st.net_input()))
    assert same(st.composed_output(), A) and same(A, st.net_input())                        # (a deep source writes 8.8 values)
    assert np.array_equal(got.view("<u2"), f32_to_frame(A[0], **ref_args(opt)))
    st.release()


def test_a_half_mask_keeps_the_source_on_the_left(eng):
    H, W = net_size(eng)
    mask = np.zeros((H, W), np.uint8)
    mask[:, W // 2:] = 255
    frame = np.random.default_rng(7).integers(0, 256, (H, W, 3), dtype=np.uint8)
    plain = plain_stylizer(eng, H, W)
    for keep in (False,) if on_emulator(eng) else (False, True):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=not on_emulator(eng), compose=dict(keep_color=keep, mask=mask))
        if keep:
            unmasked = stream.FrameStylizer(eng, variables(eng), H, W, compose=dict(keep_color=True))
            free = unmasked(frame)
            unmasked.release()
        else:
            free = plain(frame)
        got = st(frame)
        assert np.array_equal(got[:, :W // 2], frame[:, :W // 2, ::-1])                     # (the lane's own BGR -> RGB of the source)
        assert np.array_equal(got[:, W // 2:], free[:, W // 2:]) and not np.array_equal(got[:, :W // 2], free[:, :W // 2])
        st.release()


@pytest.mark.gpu
def test_pipelined_lanes_keep_the_order_and_the_one_lane_results():
    eng = get_engine("hip")
    H, W = odd_size(eng)
    mask = noise_mask(H, W, 11)
    kw = dict(compose=dict(strength=0.7, keep_color=True, mask=mask))
    rng = np.random.default_rng(8)
    frames = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(5)]
    single = stream.FrameStylizer(eng, variables(eng), H, W, **kw)
    ps = stream.PipelinedStylizer(eng, variables(eng), H, W, depth=2, **kw)
    want = [single(f) for f in frames]
    assert len({w.tobytes() for w in want}) == 5                                            # five distinct frames: an order mix-up cannot pass
    assert np.array_equal(want[4], u8_of(restated(single, mask)[0], True))
    got = list(ps.run(frames))
    assert len(got) == 5 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert all(ln.compose == single.compose and ln._mask is not None for ln in ps.lanes) and ps.lanes[0]._mask is not ps.lanes[1]._mask
    for s in (single, ps):
        s.release()


def test_a_lane_without_the_stage_has_none_of_it(eng):
    H, W = net_size(eng)
    st = plain_stylizer(eng, H, W)
    st(np.zeros((H, W, 3), np.uint8))
    assert st.compose is None and st._composed is None and st._mask is None
    with pytest.raises(_lib.FaststyleError):
        st.composed_output()


def test_compose_options_that_are_refused(eng):
    H, W = net_size(eng)
    ok = np.zeros((H, W), np.uint8)
    for opt in (dict(strenght=0.5), dict(strength=0.5, bgr=True), dict(strength=-0.1), dict(strength=1.5), dict(strength=float("nan")),
                dict(strength="much"), dict(matrix="bt2020"), dict(matrix=2), dict(mask=np.zeros((H, W + 1), np.uint8)),
                dict(mask=np.zeros((W, H), np.uint8)), dict(mask=np.zeros((H, W, 1), np.uint8)), dict(mask=ok.astype(np.float32)),
                dict(mask=ok.astype(bool))):
        with pytest.raises(_lib.FaststyleError):
            stream.FrameStylizer(eng, variables(eng), H, W, use_graph=False, compose=opt)
    # floor(s * 256 + 0.5)
    for s, q8 in ((0.0, 0), (0.001, 0), (0.002, 1), (0.3, 77), (0.5, 128), (0.998, 255), (0.9999, 256), (1, 256)):
        st = stream.FrameStylizer(eng, variables(eng), H, W, use_graph=False, compose=dict(strength=s, mask=ok))
        assert st.compose["strength_q8"] == q8 and st._composed is not None and tuple(st._composed.shape) == st.out_shape
        st.release()
