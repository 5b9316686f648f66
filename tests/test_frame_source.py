"""The frame loop's input side on the device (faststyle_amd/stream.py, source=): pixel frames of another size resized with cv2.resize's
resampling ahead of the net, JPEG frames decoded natively, both inside the lane's captured graph.  Every comparison is exact: the resized /
decoded frame that reaches the net is bit-identical to cvresize.py's / PIL's, and the net behind it is the same launch sequence.  Shapes as
the precedent's (tests/test_jpeg_encode.py): 48 x 56 eager on the emulator, 96 x 136 through the captured graph on the GPU, two frames there
so that the second replays."""
import io
import os

import numpy as np
import pytest
from PIL import Image

from faststyle_amd import _lib, cvresize, stream
from tests.backends import engine_params, get_engine, on_emulator
from tests.test_jpeg import encode, picture
from tests.test_jpeg_encode import pil_encode, starry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


def net_size(eng):
    return (48, 56) if on_emulator(eng) else (96, 136)


def n_frames(eng):
    return 1 if on_emulator(eng) else 2


def cv_resized(frame, H, W):
    """The frame as the lane's resize must deliver it: fx = W / Ws, fy = H / Hs, area when shrinking, cubic otherwise."""
    Hs, Ws = frame.shape[:2]
    fx, fy = W / float(Ws), H / float(Hs)
    fn = cvresize.resize_area_u8 if (fx <= 1 and fy <= 1 and (fx < 1 or fy < 1)) else cvresize.resize_cubic_u8
    out = fn(frame, fx, fy)
    assert out.shape == (H, W, 3)
    return out


_plain = {}


def plain_stylizer(eng, H, W, **kw):
    """One stylizer of the existing path per engine, size and options: the reference of every case here."""
    key = (id(eng), H, W, tuple(sorted(kw.items())))
    if key not in _plain:
        _plain[key] = stream.FrameStylizer(eng, starry(eng)[1], H, W, use_graph=not on_emulator(eng), **kw)
    return _plain[key]


@pytest.mark.parametrize("which", ["enlarging", "shrinking"])
def test_pixel_frames_of_another_size_are_resized_on_the_device(eng, which):
    H, W = net_size(eng)
    Hs, Ws = (H * 37 // 48, W * 45 // 56) if which == "enlarging" else (H * 61 // 48 + 1, W * 83 // 56 + 1)
    variables = starry(eng)[1]
    rng = np.random.default_rng(11)
    plain = plain_stylizer(eng, H, W)
    st = stream.FrameStylizer(eng, variables, H, W, use_graph=not on_emulator(eng), source=dict(height=Hs, width=Ws))
    assert st.in_shape == (1, Hs, Ws, 3) and st.source["swap_rb"] is False and plain.source is None
    # R and B exchanged on the way: once (the enlarging source), the kernel's own swap is held per path in tests/test_cvresize_device.py
    sw = stream.FrameStylizer(eng, variables, H, W, use_graph=not on_emulator(eng), source=dict(height=Hs, width=Ws, swap_rb=True)) \
        if which == "enlarging" else None
    for _ in range(n_frames(eng)):
        frame = rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
        resized = cv_resized(frame, H, W)
        assert np.array_equal(st(frame), plain(resized))
        if sw is not None:
            assert np.array_equal(sw(frame), plain(np.ascontiguousarray(resized[:, :, ::-1])))
    with pytest.raises(_lib.FaststyleError):
        st(np.zeros((H, W, 3), np.uint8))                          # the net's size is no longer the frame's
    for s in (st, sw):
        if s is not None:
            s.release()


def test_source_of_the_same_size_launches_no_resize(eng):
    H, W = net_size(eng)
    st = stream.FrameStylizer(eng, starry(eng)[1], H, W, use_graph=not on_emulator(eng), source=dict(height=H, width=W))
    assert st._src_plan is None and st._pix_dst is st._in_u8
    frame = np.random.default_rng(12).integers(0, 256, (H, W, 3), dtype=np.uint8)
    assert np.array_equal(st(frame), plain_stylizer(eng, H, W)(frame))
    with pytest.raises(_lib.FaststyleError):
        stream.FrameStylizer(eng, starry(eng)[1], H, W, source=dict(height=H, width=W, colour="bgr"))
    with pytest.raises(stream.FrameNotTaken):
        st(encode(frame, quality=90))                              # built without jpeg=: pixel frames only
    st.release()


JPEG_KINDS = [("420", dict(subsampling=2), False), ("444", dict(subsampling=0), False), ("gray", dict(), True)]


@pytest.mark.parametrize("name,opts,gray", [pytest.param(*k, id=k[0]) for k in JPEG_KINDS])
def test_jpeg_frames_are_decoded_and_resized_on_the_device(eng, name, opts, gray):
    H, W = net_size(eng)
    Hs, Ws = H * 61 // 48 + 1, W * 83 // 56 + 1                    # (62 x 84 / 123 x 202: no multiple of the MCU)
    assert Hs % 8 and Ws % 8
    variables = starry(eng)[1]
    files = [encode(picture("smooth" if k else "random", Hs, Ws, gray, seed=30 + k), quality=90, **opts) for k in range(n_frames(eng))]
    source = stream.jpeg_source(eng, files[0])
    assert source["height"] == Hs and source["width"] == Ws
    assert source["jpeg"] == dict(width=Ws, height=Hs, components=1 if gray else 3, sampling={"420": (2, 2), "444": (1, 1), "gray": (1, 1)}[name])
    plain = plain_stylizer(eng, H, W)
    st = stream.FrameStylizer(eng, variables, H, W, use_graph=not on_emulator(eng), source=source)
    out = stream.FrameStylizer(eng, variables, H, W, use_graph=not on_emulator(eng), source=source, swap_rb=False, jpeg=dict(quality=90, subsampling=1))
    for data in files:
        pixels = np.array(Image.open(io.BytesIO(data)).convert("RGB"))
        want = plain(cv_resized(pixels, H, W))
        assert np.array_equal(st(data), want)
        if name == "420":
            assert np.array_equal(st(pixels), want)                # the same stylizer takes the frame as pixels too
        got = out(data)
        assert isinstance(got, bytes) and got == pil_encode(np.ascontiguousarray(want[:, :, ::-1]), 90, 1)       # (swap_rb=False: the frame before the output swap)
    for s in (st, out):
        s.release()


def test_jpeg_frames_of_the_net_size_go_straight_in(eng):
    """Nothing to resize or swap: the decoder writes packed RGB into the net's input buffer, no resize is launched."""
    H, W = 44, 52                                                  # (no multiple of the 16 x 16 MCU)
    files = [encode(picture("smooth", H, W, False, seed=35 + k), quality=90) for k in range(n_frames(eng))]
    st = stream.FrameStylizer(eng, starry(eng)[1], H, W, use_graph=not on_emulator(eng), source=stream.jpeg_source(eng, files[0]))
    assert st._src_plan is None and st._src_rgbx is None
    plain = plain_stylizer(eng, H, W)
    for data in files:
        assert np.array_equal(st(data), plain(np.array(Image.open(io.BytesIO(data)).convert("RGB"))))
    st.release()


def progressive(arr):
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", quality=90, progressive=True)
    return buf.getvalue()


def test_frames_that_do_not_fit_raise_and_the_next_frame_is_right(eng):
    H, W = net_size(eng)
    Hs, Ws = H * 61 // 48 + 1, W * 83 // 56 + 1
    good = [encode(picture("smooth", Hs, Ws, False, seed=40 + k), quality=90) for k in range(2)]
    assert stream.jpeg_source(eng, progressive(picture("smooth", Hs, Ws, False, seed=1))) is None
    assert stream.jpeg_source(eng, b"not a jpeg at all") is None
    st = stream.FrameStylizer(eng, starry(eng)[1], H, W, use_graph=not on_emulator(eng), source=stream.jpeg_source(eng, good[0]))
    plain = plain_stylizer(eng, H, W)
    want = plain(cv_resized(np.asarray(Image.open(io.BytesIO(good[1])).convert("RGB")), H, W))
    if not on_emulator(eng):
        st(good[0])                                                # (the graph is captured and has run before the first refusal)
    bad = [progressive(picture("smooth", Hs, Ws, False, seed=41)),                         # the parser answers 1
           encode(picture("smooth", Hs + 8, Ws, False, seed=42), quality=90),              # another geometry
           encode(picture("smooth", Hs, Ws, False, seed=43), quality=90, subsampling=0),   # ... in its sampling only
           good[1][:len(good[1]) * 2 // 3],                                                # truncated in the scan
           good[1][:40]]                                                                   # truncated in the headers
    for data in bad:
        with pytest.raises(stream.FrameNotTaken):
            st(data)
        if not on_emulator(eng) or data is bad[-2]:                # the next good frame is right (emulator: after the refusal that came furthest)
            assert np.array_equal(st(good[1]), want)
    assert issubclass(stream.FrameNotTaken, _lib.FaststyleError)
    st.release()


@pytest.mark.gpu
def test_pipelined_jpeg_frames_come_back_in_order():
    eng = get_engine("hip")
    H, W = 96, 136
    Hs, Ws = 123, 202
    variables = starry(eng)[1]
    files = [encode(picture("smooth", Hs, Ws, False, seed=50 + k), quality=90) for k in range(5)]
    source = stream.jpeg_source(eng, files[0], swap_rb=True)
    single = stream.FrameStylizer(eng, variables, H, W, source=source)
    ps = stream.PipelinedStylizer(eng, variables, H, W, depth=2, jpeg_threads=2, source=source)
    want = [single(d) for d in files]
    got = list(ps.run(files))
    assert len(got) == 5 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert len({g.tobytes() for g in got}) == 5                    # five distinct frames: an order mix-up cannot pass
    plain = plain_stylizer(eng, H, W)
    pixels = np.asarray(Image.open(io.BytesIO(files[0])).convert("RGB"))
    assert np.array_equal(want[0], plain(np.ascontiguousarray(cv_resized(pixels, H, W)[:, :, ::-1])))
    # a frame that is not taken in the middle: through the driver's fallback, still in order; without one, the exception
    mixed = files[:2] + [progressive(pixels)] + files[3:]
    taken = []

    def not_taken(data):
        taken.append(data)
        return np.array(Image.open(io.BytesIO(data)).convert("RGB"))

    got = list(ps.run(mixed, not_taken=not_taken))
    assert taken == [mixed[2]] and len(got) == 5
    assert all(np.array_equal(got[k], want[k]) for k in (0, 1, 3, 4)) and np.array_equal(got[2], single(not_taken(mixed[2])))
    ps.submit(files[1])                                            # submit(bytes) on its own decodes on the calling thread
    assert np.array_equal(ps.fetch(), want[1])
    with pytest.raises(stream.FrameNotTaken):
        ps.submit(mixed[2])
    ps.submit(files[4])
    assert np.array_equal(ps.fetch(), want[4])
    for s in (single, ps):
        s.release()


@pytest.mark.gpu
def test_frames_dir_native_decode_and_frame_size(tmp_path):
    import stylize_webcam
    eng = get_engine("hip")
    parser = stylize_webcam.setup_parser()
    model = ["--model_path", os.path.join(ROOT, "models", "starry_final.ckpt")]
    default = parser.parse_args(model + ["--frames_dir", "x"])
    assert (default.input_decode, default.frame_size) == ("pil", None)
    fd = tmp_path / "frames"
    fd.mkdir()
    for k in range(3):
        with open(str(fd / ("f%02d.jpg" % k)), "wb") as f:
            f.write(encode(picture("smooth", 56, 72, False, seed=60 + k), quality=92))
    with open(str(fd / "f03.jpg"), "wb") as f:                     # a frame the library does not take rides along through PIL
        f.write(progressive(picture("smooth", 56, 72, False, seed=63)))
    common = model + ["--frames_dir", str(fd)]
    stylize_webcam.run_frames_dir(parser.parse_args(common + ["--output_dir", str(tmp_path / "pil")]))
    stylize_webcam.run_frames_dir(parser.parse_args(common + ["--output_dir", str(tmp_path / "native"), "--input_decode", "native"]))
    names = ["f%02d.png" % k for k in range(4)]
    assert sorted(os.listdir(str(tmp_path / "pil"))) == names and sorted(os.listdir(str(tmp_path / "native"))) == names
    for n in names:
        assert open(str(tmp_path / "native" / n), "rb").read() == open(str(tmp_path / "pil" / n), "rb").read()
    # --frame_size 72 56 on 112 x 144 frames, both decoders, against stylizing cvresize's result
    big = tmp_path / "big"
    big.mkdir()
    pics = [picture("smooth", 112, 144, False, seed=70 + k) for k in range(3)]
    for k, p in enumerate(pics):
        with open(str(big / ("g%02d.jpg" % k)), "wb") as f:
            f.write(encode(p, quality=92))
    common = model + ["--frames_dir", str(big), "--frame_size", "72", "56"]
    stylize_webcam.run_frames_dir(parser.parse_args(common + ["--output_dir", str(tmp_path / "rs_pil")]))
    stylize_webcam.run_frames_dir(parser.parse_args(common + ["--output_dir", str(tmp_path / "rs_native"), "--input_decode", "native"]))
    plain = plain_stylizer(eng, 56, 72)
    for k in range(3):
        decoded = np.asarray(Image.open(str(big / ("g%02d.jpg" % k))).convert("RGB"))
        want = plain(np.ascontiguousarray(cv_resized(decoded, 56, 72)[:, :, ::-1]))[:, :, ::-1]       # BGR in, the saved frame swapped back
        for d in ("rs_pil", "rs_native"):
            assert np.array_equal(np.asarray(Image.open(str(tmp_path / d / ("g%02d.png" % k)))), want), (d, k)
    with pytest.raises(SystemExit):
        stylize_webcam.run_frames_dir(parser.parse_args(common + ["--resolution", "72", "56"]))
