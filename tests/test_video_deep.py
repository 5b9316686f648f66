"""Deep video through the frame lanes (faststyle_amd/stream.py: source yuv= / yuv_out= with bits=) and the command line (stylize_webcam.py
--video_depth / --video_out_depth).  Every comparison is exact: the fp32 image that reaches the net is the numpy restatement's
(tests/test_yuv_deep.py), read back with FrameStylizer.net_input(); the net behind it is the existing launch sequence, held by a grey frame
whose fp32 image is that of a u8 frame; and what comes back is the restatement's of FrameStylizer.net_output().  Shapes as
tests/test_frame_source.py: 48 x 56 eager on the emulator, 96 x 136 through the captured graph on the GPU, two frames there so that the
second replays."""
import os

import numpy as np
import pytest
from PIL import Image

from faststyle_amd import _lib, stream, y4m
from tests.backends import engine_params, get_engine, on_emulator
from tests.test_frame_source import n_frames, net_size, plain_stylizer
from tests.test_jpeg_encode import starry
from tests.test_yuv import frame_to_rgb, geometry, rgb_to_frame
from tests.test_yuv_deep import F_of_f32, f32_to_frame, frame_to_F, frame_to_f32, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = ["--model_path", os.path.join(ROOT, "models", "starry_final.ckpt")]

# name -> the yuv= dict
DEEP = {
    "420p10": dict(sampling=(2, 2), siting=0, matrix=0, full_range=False, bits=10),
    "422p12": dict(sampling=(2, 1), siting=1, matrix=1, full_range=False, bits=12),
    "444p16": dict(sampling=(1, 1), siting=0, matrix=1, full_range=True, bits=16),
    "mono12": dict(sampling=(1, 1), siting=0, matrix=0, full_range=True, components=1, bits=12),
}
EIGHT = dict(sampling=(2, 2), siting=1, matrix=1, full_range=True)


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


def graph(eng):
    return not on_emulator(eng)


def ref_args(opt):
    """The restatements' arguments of a yuv= dict"""
    a = dict(hs=opt["sampling"][0], vs=opt["sampling"][1], ncomp=opt.get("components", 3), siting=opt["siting"], matrix=opt["matrix"],
             full_range=int(opt["full_range"]))
    if opt.get("bits", 8) != 8:
        a["bits"] = opt["bits"]
    return a


def samples_of(opt, W, H, seed):
    """One frame of a ramp plus noise over the depth's whole range: its samples (uint16 for a deep layout, uint8 otherwise)"""
    a = ref_args(opt)
    n = geometry(W, H, a["hs"], a["vs"], a["ncomp"])[2]
    top = 2 ** opt.get("bits", 8)
    rng = np.random.default_rng(seed)
    ramp = (np.arange(n) * (top // 85) + seed * 17) % top
    return ((ramp + rng.integers(0, top // 4, n)) % top).astype(np.uint16 if top > 256 else np.uint8)


def u8_of(y, swap):
    """fs_f32_to_u8's rule on a host tensor: clamp, truncate, optionally exchange R and B"""
    u = (F_of_f32(y) >> 8).astype(np.uint8)
    return np.ascontiguousarray(u[..., ::-1]) if swap else u


@pytest.mark.parametrize("name", ["420p10", "444p16", "mono12"])
def test_deep_frames_reach_the_net_as_the_restatement_converts_them(eng, name):
    H, W = net_size(eng)
    opt = DEEP[name]
    variables = starry(eng)[1]
    st = stream.FrameStylizer(eng, variables, H, W, use_graph=graph(eng), source=dict(height=H, width=W, yuv=opt))
    a = ref_args(opt)
    n = geometry(W, H, a["hs"], a["vs"], a["ncomp"])[2]
    assert st.in_shape == (1, 2 * n) and st.source["yuv"] == opt and st._src_plan is None and st._src_deep and not st._out_deep
    with pytest.raises(_lib.FaststyleError):
        st.net_output()                                                                     # nothing has run yet
    sw = stream.FrameStylizer(eng, variables, H, W, use_graph=graph(eng), swap_rb=False, source=dict(height=H, width=W, swap_rb=True, yuv=opt)) \
        if name == "420p10" else None
    for k in range(n_frames(eng)):
        s = samples_of(opt, W, H, 20 + k)
        out = st(s.view(np.uint8))
        assert same(st.net_input()[0], frame_to_f32(s, W, H, **a))
        y = st.net_output()
        assert y.shape == st.out_shape and y.dtype == np.float32
        assert out.dtype == np.uint8 and np.array_equal(out, u8_of(y[0], True))             # (a lane swaps R and B on the way out by default)
        if sw is not None:
            out = sw(s)                                                                     # (the samples themselves are taken as well)
            assert same(sw.net_input()[0], frame_to_f32(s, W, H, swap=True, **a))
            assert np.array_equal(out, u8_of(sw.net_output()[0], False))
    assert np.array_equal(st(s.view(np.uint8)[np.newaxis]), u8_of(y, True))                 # a batch of one keeps its axis
    with pytest.raises(_lib.FaststyleError):
        st(np.zeros((H, W, 3), np.uint8))                                                   # such a stylizer takes planes only
    with pytest.raises(_lib.FaststyleError):
        st(s.view(np.uint8)[:-2])
    with pytest.raises(_lib.FaststyleError):
        st(s.view(np.uint8)[:n])                                                            # the 8-bit size of such a frame
    for s_ in (st, sw):
        if s_ is not None:
            s_.release()


def test_the_net_behind_a_deep_source_is_the_existing_launch_sequence(eng):
    """A grey 16-bit full-range frame with Y = 257 v and chroma 2^15 has F = 256 v exactly, so the net's input is the float of the u8 grey frame
    v: the lane returns byte for byte what the existing stylizer returns for that frame -- as pixels, and as the JPEG file of a lane with jpeg=."""
    H, W = net_size(eng)
    opt = dict(sampling=(2, 2), siting=0, matrix=1, full_range=True, bits=16)
    rng = np.random.default_rng(5)
    cw, ch, n = geometry(W, H, 2, 2, 3)
    variables = starry(eng)[1]
    st = stream.FrameStylizer(eng, variables, H, W, use_graph=graph(eng), source=dict(height=H, width=W, yuv=opt))
    plain = plain_stylizer(eng, H, W)
    for k in range(n_frames(eng)):
        v = ((np.arange(H * W).reshape(H, W) * 3 // 7 + rng.integers(0, 32, (H, W)) + 40 * k) % 256).astype(np.int64)
        s = np.concatenate([(257 * v).reshape(-1), np.full(2 * cw * ch, 2 ** 15)]).astype(np.uint16)
        assert np.array_equal(frame_to_F(s, W, H, **ref_args(opt)), np.repeat((256 * v)[:, :, None], 3, axis=2))
        grey = np.repeat(v.astype(np.uint8)[:, :, None], 3, axis=2)
        out = st(s.view(np.uint8))
        assert same(st.net_input()[0], grey.astype(np.float32))
        assert np.array_equal(out, plain(grey))
    st.release()
    if on_emulator(eng):                                                                    # (two more passes of the net: on the GPU only)
        return
    jp = dict(quality=90, subsampling=2)
    sj = stream.FrameStylizer(eng, variables, H, W, use_graph=graph(eng), jpeg=jp, source=dict(height=H, width=W, yuv=opt))
    pj = stream.FrameStylizer(eng, variables, H, W, use_graph=graph(eng), jpeg=jp)
    data = sj(s.view(np.uint8))
    assert isinstance(data, bytes) and data[:2] == b"\xff\xd8" and data == pj(grey)
    for s_ in (sj, pj):
        s_.release()


@pytest.mark.parametrize("name", ["420p10", "422p12"])
def test_deep_yuv_out_returns_the_planes_of_the_net_output(eng, name):
    H, W = net_size(eng)
    opt = DEEP[name]
    plain = plain_stylizer(eng, H, W)
    st = stream.FrameStylizer(eng, starry(eng)[1], H, W, use_graph=graph(eng), yuv_out=opt)
    Ho, Wo = st.out_shape[1:3]
    a = ref_args(opt)
    assert st.yuv_out == opt and st.jpeg is None and st._out_deep and not st._src_deep
    assert int(st.yuv_out_desc.frame_bytes) == 2 * geometry(Wo, Ho, a["hs"], a["vs"], a["ncomp"])[2] and st.yuv_out_desc.reserved[0] == opt["bits"]
    rng = np.random.default_rng(31)
    for _ in range(n_frames(eng)):
        frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        got = st(frame)
        y = st.net_output()[0]
        assert got.dtype == np.uint8 and got.shape == (int(st.yuv_out_desc.frame_bytes),)
        assert np.array_equal(got.view("<u2"), f32_to_frame(y, swap=True, **a))              # (the lane's default swap, made by the conversion)
        assert np.array_equal(plain(frame), u8_of(y, True)) and same(plain.net_output()[0], y)     # the same net output as the existing lane's
    st.release()


def test_one_deep_end_with_the_eight_bit_kernels_on_the_other(eng):
    H, W = net_size(eng)
    variables = starry(eng)[1]
    deep = DEEP["420p10"]
    # 8-bit in, deep out, the channel options of the command line
    st = stream.FrameStylizer(eng, variables, H, W, use_graph=graph(eng), swap_rb=False, source=dict(height=H, width=W, swap_rb=True, yuv=EIGHT),
                              yuv_out=deep)
    planes = samples_of(EIGHT, W, H, 41)
    got = st(planes)
    bgr = np.ascontiguousarray(frame_to_rgb(planes, W, H, **ref_args(EIGHT))[:, :, ::-1])
    assert same(st.net_input()[0], bgr.astype(np.float32))
    assert np.array_equal(got.view("<u2"), f32_to_frame(st.net_output()[0], **ref_args(deep)))
    st.release()
    # deep in, 8-bit out
    st = stream.FrameStylizer(eng, variables, H, W, use_graph=graph(eng), swap_rb=False, source=dict(height=H, width=W, swap_rb=True, yuv=deep),
                              yuv_out=EIGHT)
    s = samples_of(deep, W, H, 42)
    got = st(s)
    assert same(st.net_input()[0], frame_to_f32(s, W, H, swap=True, **ref_args(deep)))
    assert np.array_equal(got, rgb_to_frame(u8_of(st.net_output()[0], False), **ref_args(EIGHT)))
    st.release()


def test_deep_options_that_are_refused(eng):
    H, W = net_size(eng)
    variables = starry(eng)[1]
    deep = DEEP["420p10"]
    for kw in (dict(source=dict(height=H + 2, width=W, yuv=deep)), dict(source=dict(height=H // 2, width=W // 2, yuv=deep)),     # the resize is u8 only
               dict(source=dict(height=H, width=W, yuv=dict(deep, bits=17))), dict(source=dict(height=H, width=W, yuv=dict(deep, bits=7))),
               dict(yuv_out=dict(deep, bits=17)), dict(yuv_out=dict(deep, depth=10)), dict(source=dict(height=H, width=W, yuv=dict(deep, depth=10))),
               dict(yuv_out=deep, jpeg=dict(quality=90)),
               dict(source=dict(height=H, width=W, yuv=deep, jpeg=dict(width=W, height=H, components=3, sampling=(2, 2))))):
        with pytest.raises(_lib.FaststyleError):
            stream.FrameStylizer(eng, variables, H, W, use_graph=False, **kw)
    # bits=8 is the lane it is without the key
    st = stream.FrameStylizer(eng, variables, H, W, use_graph=False, source=dict(height=H, width=W, yuv=dict(EIGHT, bits=8)), yuv_out=dict(EIGHT, bits=8))
    assert not st._src_deep and not st._out_deep and st.in_shape == (1, geometry(W, H, 2, 2, 3)[2]) and st.yuv_out_desc.reserved[0] == 0
    st.release()


@pytest.mark.gpu
def test_pipelined_deep_frames_come_back_in_order():
    eng = get_engine("hip")
    H, W = 96, 136
    opt = DEEP["420p10"]
    variables = starry(eng)[1]
    kw = dict(swap_rb=False, source=dict(height=H, width=W, swap_rb=True, yuv=opt), yuv_out=opt)
    frames = [samples_of(opt, W, H, 50 + k).view(np.uint8) for k in range(5)]
    single = stream.FrameStylizer(eng, variables, H, W, **kw)
    ps = stream.PipelinedStylizer(eng, variables, H, W, depth=2, **kw)
    want = [single(f) for f in frames]
    assert len({w.tobytes() for w in want}) == 5                                            # five distinct frames: an order mix-up cannot pass
    assert np.array_equal(want[4].view("<u2"), f32_to_frame(single.net_output()[0], **ref_args(opt)))
    got = list(ps.run(frames))
    assert len(got) == 5 and all(np.array_equal(g, w) for g, w in zip(got, want))
    # the reader's way in: the next lane's pinned buffer, sized from frame_bytes, filled in place, then submitted
    got = []
    for f in frames:
        if ps.in_flight >= ps.depth:
            got.append(ps.fetch())
        buf = ps.next_input()
        assert buf.shape == (1, f.size) == (1, int(single._src_yuv.frame_bytes)) and buf.ctypes.data == ps.host_in[ps._n % 2].data_ptr()
        buf[0] = f
        ps.submit(buf[0])
    while ps.in_flight:
        got.append(ps.fetch())
    assert len(got) == 5 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert tuple(ps.host_out[0].shape) == (1, int(ps.yuv_out_desc.frame_bytes)) and ps.yuv_out_desc.reserved[0] == 10
    for s in (single, ps):
        s.release()


def write_stream(path, opt, W, H, frames, rate=(30000, 1001), aspect=(1, 1)):
    a = ref_args(opt)
    with open(path, "wb") as f:
        f.write(y4m.header(W, H, (a["hs"], a["vs"]), a["siting"], a["ncomp"], bool(a["full_range"]), rate, aspect, bits=opt.get("bits", 8)))
        for fr in frames:
            f.write(b"FRAME\n" + fr.tobytes())


def read_stream(path):
    with open(path, "rb") as f:
        head = f.readline()
        f.seek(0)
        r = y4m.Reader(f, deep=True)
        out = []
        buf = np.zeros(r.format.frame_bytes, np.uint8)
        while r.read_frame_into(buf):
            out.append(buf.copy())
    return head, r.format, out


@pytest.mark.gpu
def test_deep_video_in_video_out_files(tmp_path):
    import stylize_webcam
    eng = get_engine("hip")
    parser = stylize_webcam.setup_parser()
    default = parser.parse_args(MODEL)
    assert (default.video_depth, default.video_out_depth) == ("8", None)
    W, H = 72, 56
    opt = dict(sampling=(2, 2), siting=0, matrix=1, full_range=True, bits=10)              # C420p10, full range, --video_matrix bt709
    frames = [samples_of(opt, W, H, 60 + k) for k in range(3)]
    src = str(tmp_path / "f.y4m")
    write_stream(src, opt, W, H, frames)
    common = MODEL + ["--video_in", src, "--video_matrix", "bt709", "--video_depth", "stream"]
    stylize_webcam.run_video(parser.parse_args(common + ["--video_out", str(tmp_path / "g.y4m")]))
    head, fmt, got = read_stream(str(tmp_path / "g.y4m"))
    Ho, Wo = eng.tnet_out_shape(H, W)
    assert b" C420p10 " in head and b" F30000:1001 " in head and b" A1:1 " in head and b"XCOLORRANGE=FULL" in head
    assert (fmt.width, fmt.height, fmt.rate, fmt.aspect, fmt.sampling, fmt.siting, fmt.full_range, fmt.components, fmt.bits) == \
        (Wo, Ho, (30000, 1001), (1, 1), (2, 2), 0, True, 3, 10)
    lane = stream.FrameStylizer(eng, starry(eng)[1], H, W, swap_rb=False, source=dict(height=H, width=W, swap_rb=True, yuv=opt), yuv_out=opt)
    want = [lane(f) for f in frames]
    assert len(got) == 3 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert np.array_equal(want[2].view("<u2"), f32_to_frame(lane.net_output()[0], **ref_args(opt)))
    lane.release()
    # --video_out_depth 8 from the 10-bit input: an 8-bit stream of the same layout
    stylize_webcam.run_video(parser.parse_args(common + ["--video_out", str(tmp_path / "g8.y4m"), "--video_out_depth", "8"]))
    head, fmt, got = read_stream(str(tmp_path / "g8.y4m"))
    opt8 = {k: v for k, v in opt.items() if k != "bits"}
    assert b" C420jpeg " in head and fmt.bits == 8 and fmt.frame_bytes == geometry(Wo, Ho, 2, 2, 3)[2]
    lane = stream.FrameStylizer(eng, starry(eng)[1], H, W, swap_rb=False, source=dict(height=H, width=W, swap_rb=True, yuv=opt), yuv_out=opt8)
    assert len(got) == 3 and all(np.array_equal(g, lane(f)) for g, f in zip(got, frames))
    lane.release()
    # 8-bit in, --video_out_depth 12 out; --video_depth stream with an 8-bit stream runs as without it
    frames8 = [samples_of(opt8, W, H, 70 + k) for k in range(2)]
    write_stream(str(tmp_path / "e.y4m"), opt8, W, H, frames8)
    eight = MODEL + ["--video_in", str(tmp_path / "e.y4m"), "--video_matrix", "bt709"]
    stylize_webcam.run_video(parser.parse_args(eight + ["--video_out", str(tmp_path / "h12.y4m"), "--video_out_depth", "12"]))
    head, fmt, got = read_stream(str(tmp_path / "h12.y4m"))
    lane = stream.FrameStylizer(eng, starry(eng)[1], H, W, swap_rb=False, source=dict(height=H, width=W, swap_rb=True, yuv=opt8), yuv_out=dict(opt8, bits=12))
    assert b" C420p12 " in head and len(got) == 2 and all(np.array_equal(g, lane(f)) for g, f in zip(got, frames8))
    lane.release()
    stylize_webcam.run_video(parser.parse_args(eight + ["--video_out", str(tmp_path / "h_a.y4m")]))
    stylize_webcam.run_video(parser.parse_args(eight + ["--video_out", str(tmp_path / "h_b.y4m"), "--video_depth", "stream"]))
    assert open(str(tmp_path / "h_a.y4m"), "rb").read() == open(str(tmp_path / "h_b.y4m"), "rb").read()
    # a deep input with --output_dir: the .png files of the lane's u8 frames
    stylize_webcam.run_video(parser.parse_args(common + ["--output_dir", str(tmp_path / "png")]))
    lane = stream.FrameStylizer(eng, starry(eng)[1], H, W, source=dict(height=H, width=W, swap_rb=True, yuv=opt))
    assert sorted(os.listdir(str(tmp_path / "png"))) == ["%06d.png" % k for k in range(3)]
    for k, f in enumerate(frames):
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / "png" / ("%06d.png" % k)))), lane(f)[:, :, ::-1])
    lane.release()


def test_deep_flags_that_exit_before_the_model_loads(tmp_path):
    import stylize_webcam
    parser = stylize_webcam.setup_parser()
    W, H = 64, 48
    opt = DEEP["420p10"]
    src = str(tmp_path / "f.y4m")
    write_stream(src, opt, W, H, [samples_of(opt, W, H, 1)])
    out = tmp_path / "g.y4m"
    # (no --model_path in any of these: a run that got as far as loading the model would fail otherwise)
    with pytest.raises(SystemExit) as e:                                                    # the existing behaviour, asserted again
        stylize_webcam.run_video(parser.parse_args(["--video_in", src, "--video_out", str(out)]))
    assert "C420p10" in str(e.value) and "--video_depth stream" in str(e.value) and not out.exists()
    with pytest.raises(SystemExit) as e:
        stylize_webcam.run_video(parser.parse_args(["--video_in", src, "--video_out", str(out), "--video_depth", "8"]))
    assert "C420p10" in str(e.value) and not out.exists()
    with pytest.raises(SystemExit) as e:
        stylize_webcam.run_video(parser.parse_args(["--video_in", src, "--video_out", str(out), "--video_depth", "stream", "--frame_size", "32", "24"]))
    assert "--frame_size" in str(e.value) and "10 bits" in str(e.value) and not out.exists()
    # a co-sited 4:2:0 stream has no deep tag to be written with
    write_stream(str(tmp_path / "m.y4m"), EIGHT, W, H, [samples_of(EIGHT, W, H, 2)])
    with pytest.raises(SystemExit) as e:
        stylize_webcam.run_video(parser.parse_args(["--video_in", str(tmp_path / "m.y4m"), "--video_out", str(out), "--video_out_depth", "10"]))
    assert "no Y4M colour space" in str(e.value) and not out.exists()
    for flags in (["--video_depth", "10"], ["--video_out_depth", "7"], ["--video_out_depth", "17"]):
        with pytest.raises(SystemExit):
            parser.parse_args(flags)
