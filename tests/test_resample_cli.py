"""--output_size / --output_filter / --frame_filter of stylize_webcam.py, run in-process with main(argv) (tests/test_resample_stream.py holds
the lanes against the restatement): the files and streams are those of the lanes and carry the delivery size, --frame_filter lifts the deep
--frame_size refusal and nothing else does, and bad flags exit before the model loads."""
import os

import numpy as np
import pytest
from PIL import Image

from faststyle_amd import stream
from tests.backends import get_engine
from tests.test_compose_cli import H, OPT, W, files, frames_dir, main, pngs, video
from tests.test_compose_stream import variables
from tests.test_video_deep import MODEL, read_stream, samples_of, write_stream

DEEP10 = dict(OPT, bits=10)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["png", "jpg"])
def test_frames_dir_delivers_at_a_given_size_and_at_the_source_size(tmp_path, fmt):
    eng = get_engine("hip")
    rng = np.random.default_rng(21)
    Hs, Ws = 80, 100
    images = [rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8) for _ in range(3)]
    out = lambda name: str(tmp_path / name)
    more = ["--output_format", "jpg", "--output_quality", "90"] if fmt == "jpg" else []
    lane_kw = dict(swap_rb=False, jpeg=dict(quality=90, subsampling=2)) if fmt == "jpg" else {}

    def check(d, lane, size):
        assert sorted(os.listdir(d)) == ["%03d.%s" % (k, fmt) for k in range(3)]
        for k, im in enumerate(images):
            want = lane(np.ascontiguousarray(im[:, :, ::-1]))
            if fmt == "jpg":
                assert files(d)[k] == want
                assert Image.open(os.path.join(d, "%03d.jpg" % k)).size == size
            else:
                got = pngs(d)[k]
                assert got.shape == (size[1], size[0], 3) and np.array_equal(got, want[:, :, ::-1])
        lane.release()

    # the net at 72 x 56, the files at the frames' own 100 x 80
    main(frames_dir(tmp_path, images, "a") + ["--output_dir", out("src"), "--frame_size", str(W), str(H), "--output_size", "source"] + more)
    check(out("src"), stream.FrameStylizer(eng, variables(eng), H, W, source=dict(height=Hs, width=Ws),
                                           deliver=dict(height=Hs, width=Ws, filter="bicubic"), **lane_kw), (Ws, Hs))
    # the net at the frames' size, the files smaller, another filter
    main(frames_dir(tmp_path, images, "b") + ["--output_dir", out("num"), "--output_size", "66", "52", "--output_filter", "lanczos"] + more)
    check(out("num"), stream.FrameStylizer(eng, variables(eng), Hs, Ws, deliver=dict(height=52, width=66, filter="lanczos"), **lane_kw), (66, 52))


@pytest.mark.gpu
def test_video_streams_carry_the_delivery_size_at_8_and_10_bits(tmp_path):
    eng = get_engine("hip")
    out = lambda name: str(tmp_path / name)
    # 8 bits: the net at the stream's 72 x 56, delivered at 108 x 84
    frames = [samples_of(OPT, W, H, 30 + k) for k in range(3)]
    main(video(tmp_path, frames) + ["--video_out", out("g.y4m"), "--output_size", "108", "84", "--output_filter", "bilinear"])
    head, fmt, got = read_stream(out("g.y4m"))
    assert b" W108 " in head and b" H84 " in head and (fmt.width, fmt.height, fmt.bits) == (108, 84, 8)
    lane = stream.FrameStylizer(eng, variables(eng), H, W, swap_rb=False, source=dict(height=H, width=W, swap_rb=True, yuv=OPT), yuv_out=OPT,
                                deliver=dict(height=84, width=108, filter="bilinear"))
    assert len(got) == 3 and all(np.array_equal(g, lane(f)) for g, f in zip(got, frames))
    lane.release()
    # 10 bits: a 144 x 112 stream, the net at 72 x 56 through --frame_filter, delivered at the stream's size
    Ws, Hs = 2 * W, 2 * H
    deep = [samples_of(DEEP10, Ws, Hs, 40 + k) for k in range(3)]
    src = out("d.y4m")
    write_stream(src, DEEP10, Ws, Hs, deep)
    run = MODEL + ["--video_in", src, "--video_matrix", "bt709", "--video_depth", "stream", "--frame_size", str(W), str(H)]
    main(run + ["--frame_filter", "bicubic", "--output_size", "source", "--video_out", out("h.y4m")])
    head, fmt, got = read_stream(out("h.y4m"))
    assert b" W144 " in head and b" H112 " in head and (fmt.width, fmt.height, fmt.bits) == (Ws, Hs, 10)
    lane = stream.FrameStylizer(eng, variables(eng), H, W, swap_rb=False,
                                source=dict(height=Hs, width=Ws, swap_rb=True, yuv=DEEP10, resample="bicubic"), yuv_out=DEEP10,
                                deliver=dict(height=Hs, width=Ws, filter="bicubic"))
    assert len(got) == 3 and all(np.array_equal(g, lane(f)) for g, f in zip(got, deep))
    lane.release()
    # --frame_filter alone lifts the refusal: the stream comes back at the net's size
    main(run + ["--frame_filter", "lanczos", "--video_out", out("i.y4m")])
    head, fmt, got = read_stream(out("i.y4m"))
    assert (fmt.width, fmt.height, fmt.bits) == (W, H, 10) and len(got) == 3
    lane = stream.FrameStylizer(eng, variables(eng), H, W, swap_rb=False,
                                source=dict(height=Hs, width=Ws, swap_rb=True, yuv=DEEP10, resample="lanczos"), yuv_out=DEEP10)
    assert all(np.array_equal(g, lane(f)) for g, f in zip(got, deep))
    lane.release()
    # and without it the refusal stands
    with pytest.raises(SystemExit) as e:
        main(run + ["--video_out", out("j.y4m")])
    assert "--frame_size does not take a stream of 10 bits" in str(e.value) and not os.path.exists(out("j.y4m"))


def test_new_refusals_fire_before_the_model_loads_and_create_nothing(tmp_path):
    # (no usable --model_path in any of these: a run that got as far as loading the model would fail otherwise)
    nomodel = ["--model_path", str(tmp_path / "none.ckpt")]
    write_stream(str(tmp_path / "f.y4m"), OPT, W, H, [samples_of(OPT, W, H, 1)])
    write_stream(str(tmp_path / "d.y4m"), DEEP10, W, H, [samples_of(DEEP10, W, H, 2)])
    vid = nomodel + ["--video_in", str(tmp_path / "f.y4m"), "--video_out", str(tmp_path / "g.y4m")]
    deep = nomodel + ["--video_in", str(tmp_path / "d.y4m"), "--video_out", str(tmp_path / "g.y4m"), "--video_depth", "stream"]
    d = tmp_path / "in"
    d.mkdir()
    Image.fromarray(np.zeros((H, W, 3), np.uint8)).save(str(d / "000.png"))
    pix = nomodel + ["--frames_dir", str(d), "--output_dir", str(tmp_path / "out")]
    for run in (vid, deep, pix):
        for flags, word in ((["--output_filter", "lanczos"], "--output_filter needs --output_size"),
                            (["--output_size", "5"], "--output_size"), (["--output_size", "wide", "tall"], "--output_size"),
                            (["--output_size", "0", "10"], "--output_size"), (["--output_size", "64", "-2"], "--output_size"),
                            (["--output_size", "source", "3"], "--output_size"), (["--output_size", "64", "48", "32"], "--output_size"),
                            (["--output_size", "40000", "10"], "--output_size"), (["--output_size", "10", "32768"], "--output_size")):
            with pytest.raises(SystemExit) as e:
                main(run + flags)
            assert word in str(e.value), (flags, str(e.value))
        with pytest.raises(SystemExit):
            main(run + ["--output_size", "64", "48", "--output_filter", "nearest"])           # (argparse: not one of the four)
        with pytest.raises(SystemExit):
            main(run + ["--frame_size", "36", "28", "--frame_filter", "nearest"])
    # --frame_filter: a deep --video_in under --video_depth stream with --frame_size, nothing else
    for run in (deep + ["--frame_filter", "bicubic"],                                          # no --frame_size
                vid + ["--frame_size", "36", "28", "--frame_filter", "bicubic"],               # --video_depth 8
                vid + ["--video_depth", "stream", "--frame_size", "36", "28", "--frame_filter", "bicubic"],      # an 8-bit stream
                pix + ["--frame_size", "36", "28", "--frame_filter", "bicubic"]):              # no --video_in
        with pytest.raises(SystemExit) as e:
            main(run)
        assert "--frame_filter" in str(e.value), str(e.value)
    # the refusal that was there before, in its own words
    with pytest.raises(SystemExit) as e:
        main(deep + ["--frame_size", "36", "28"])
    assert "--frame_size does not take a stream of 10 bits per sample: the resize is 8-bit only" in str(e.value)
    assert not (tmp_path / "g.y4m").exists() and not (tmp_path / "out").exists()
    # what is taken gets as far as the model
    for run in (deep + ["--frame_size", "36", "28", "--frame_filter", "box", "--output_size", "source"], vid + ["--output_size", "90", "70"],
                pix + ["--output_size", "source", "--output_filter", "box"]):
        with pytest.raises(Exception) as e:
            main(run)
        assert not isinstance(e.value, SystemExit), str(e.value)
    assert not (tmp_path / "g.y4m").exists()


def test_flags_are_absent_unless_given_and_what_the_lanes_are_given():
    import stylize_webcam
    parse = stylize_webcam.setup_parser().parse_args
    assert not {"output_size", "output_filter", "frame_filter"} & set(vars(parse([])))
    assert stylize_webcam.delivery_options(parse([])) is None
    assert stylize_webcam.delivery_options(parse(["--output_size", "source"])) == ("source", "bicubic")
    assert stylize_webcam.delivery_options(parse(["--output_size", "3840", "2160", "--output_filter", "lanczos"])) == ((3840, 2160), "lanczos")
    assert parse(["--frame_filter", "box"]).frame_filter == "box"
    assert stylize_webcam.deliver_dict(("source", "box"), (100, 80), (72, 56)) == dict(height=80, width=100, filter="box")
    assert stylize_webcam.deliver_dict(((64, 48), "bicubic"), (100, 80), (72, 56)) == dict(height=48, width=64, filter="bicubic")
