"""--output_guided / --guided_radius / --guided_smoothness of stylize_webcam.py, run in-process with main(argv) (tests/test_guided_stream.py
holds the lanes against the restatement): the streams and files are those of the lanes, the flags are absent unless given, and bad flags
exit before the model loads, with nothing created."""
import os

import numpy as np
import pytest
from PIL import Image

from faststyle_amd import stream
from tests.backends import get_engine
from tests.test_compose_cli import H, OPT, W, frames_dir, main, pngs
from tests.test_compose_stream import variables
from tests.test_video_deep import MODEL, read_stream, samples_of, write_stream

WS, HS = 2 * W, 2 * H                                           # the streams and frames: 144 x 112, the net at 72 x 56


@pytest.mark.gpu
def test_a_video_run_writes_the_stream_of_the_guided_lane(tmp_path):
    eng = get_engine("hip")
    frames = [samples_of(OPT, WS, HS, 30 + k) for k in range(3)]
    src, dst = str(tmp_path / "f.y4m"), str(tmp_path / "g.y4m")
    write_stream(src, OPT, WS, HS, frames)
    main(MODEL + ["--video_in", src, "--video_matrix", "bt709", "--video_out", dst, "--frame_size", str(W), str(H), "--output_size", "source",
                  "--output_guided", "--guided_radius", "1", "--guided_smoothness", "8"])
    head, fmt, got = read_stream(dst)
    assert b" W144 " in head and b" H112 " in head and (fmt.width, fmt.height, fmt.bits) == (WS, HS, 8)
    # the lanes of such a run: the net is fed B,G,R, the output conversion does not swap, the luma weights are --video_matrix's
    lane = stream.FrameStylizer(eng, variables(eng), H, W, swap_rb=False, source=dict(height=HS, width=WS, swap_rb=True, yuv=OPT), yuv_out=OPT,
                                deliver=dict(height=HS, width=WS, guided=dict(radius=1, smoothness=8, matrix="bt709", source_bgr=True)))
    assert lane._guided_src[False][1] is False                  # (the RGBX of the stream's frames against a net fed B,G,R)
    assert len(got) == 3 and all(np.array_equal(g, lane(f)) for g, f in zip(got, frames))
    lane.release()
    # and not the resampled stream
    other = stream.FrameStylizer(eng, variables(eng), H, W, swap_rb=False, source=dict(height=HS, width=WS, swap_rb=True, yuv=OPT), yuv_out=OPT,
                                 deliver=dict(height=HS, width=WS))
    assert not np.array_equal(got[0], other(frames[0]))
    other.release()


@pytest.mark.gpu
def test_a_frames_dir_run_writes_the_files_of_the_guided_lane(tmp_path):
    eng = get_engine("hip")
    rng = np.random.default_rng(22)
    images = [rng.integers(0, 256, (HS, WS, 3), dtype=np.uint8) for _ in range(3)]
    out = str(tmp_path / "out")
    main(frames_dir(tmp_path, images) + ["--output_dir", out, "--frame_size", str(W), str(H), "--output_size", str(WS), str(HS), "--output_guided"])
    lane = stream.FrameStylizer(eng, variables(eng), H, W, source=dict(height=HS, width=WS),
                                deliver=dict(height=HS, width=WS, guided=dict(source_bgr=True)))
    got = pngs(out)
    assert len(got) == 3
    for g, im in zip(got, images):
        assert g.shape == (HS, WS, 3) and np.array_equal(g, lane(np.ascontiguousarray(im[:, :, ::-1]))[:, :, ::-1])
    lane.release()


def test_flags_are_absent_unless_given_and_what_the_lanes_are_given():
    import stylize_webcam
    parse = stylize_webcam.setup_parser().parse_args
    assert not {"output_guided", "guided_radius", "guided_smoothness"} & set(vars(parse([])))
    assert stylize_webcam.guided_options(parse([])) is None
    on = ["--frame_size", "72", "56", "--output_size", "source", "--output_guided"]
    assert stylize_webcam.guided_options(parse(on)) == dict(radius=2, smoothness=4, matrix="bt601", source_bgr=True)
    assert stylize_webcam.guided_options(parse(on + ["--guided_radius", "8", "--guided_smoothness", "64", "--color_matrix", "bt709"])) == \
        dict(radius=8, smoothness=64, matrix="bt709", source_bgr=True)
    assert stylize_webcam.guided_options(parse(on), "bt709")["matrix"] == "bt709"              # (--video_matrix, as temporal's)
    g = dict(radius=2, smoothness=4, matrix="bt601", source_bgr=True)
    assert stylize_webcam.deliver_dict(("source", "bicubic"), (144, 112), (72, 56), g) == dict(height=112, width=144, guided=g)
    assert stylize_webcam.deliver_dict(((144, 112), "bicubic"), (144, 112), (144, 56), g) == dict(height=112, width=144, guided=g)
    assert stylize_webcam.deliver_dict(("source", "box"), (100, 80), (72, 56)) == dict(height=80, width=100, filter="box")     # as it was


def test_refusals_fire_before_the_model_loads_and_create_nothing(tmp_path):
    # (no usable --model_path in any of these: a run that got as far as loading the model would fail otherwise)
    nomodel = ["--model_path", str(tmp_path / "none.ckpt")]
    write_stream(str(tmp_path / "f.y4m"), OPT, WS, HS, [samples_of(OPT, WS, HS, 1)])
    vid = nomodel + ["--video_in", str(tmp_path / "f.y4m"), "--video_out", str(tmp_path / "g.y4m")]
    d = tmp_path / "in"
    d.mkdir()
    Image.fromarray(np.zeros((HS, WS, 3), np.uint8)).save(str(d / "000.png"))
    pix = nomodel + ["--frames_dir", str(d), "--output_dir", str(tmp_path / "out")]
    size, net = ["--output_size", "source"], ["--frame_size", str(W), str(H)]
    for run in (vid, pix):
        for flags, word in ((net + size + ["--guided_radius", "2"], "--guided_radius needs --output_guided"),
                            (net + size + ["--guided_smoothness", "4"], "--guided_smoothness needs --output_guided"),
                            (net + ["--output_guided"], "--output_guided needs --output_size"),
                            (net + size + ["--output_guided", "--output_filter", "bicubic"], "--output_filter"),
                            (size + ["--output_guided"], "--output_guided needs --frame_size"),
                            (net + ["--output_size", "150", "112", "--output_guided"], "--output_guided: the delivery is 150 by 112"),
                            (net + ["--output_size", "72", "56", "--output_guided"], "--output_guided: the delivery is 72 by 56"),
                            (["--frame_size", str(WS), str(HS)] + size + ["--output_guided"], "--output_guided upsamples"),
                            (["--frame_size", str(WS + 8), str(HS)] + size + ["--output_guided"], "--output_guided upsamples"),
                            (net + size + ["--output_guided", "--guided_radius", "0"], "--guided_radius 0 is outside [1, 8]"),
                            (net + size + ["--output_guided", "--guided_radius", "9"], "--guided_radius 9 is outside [1, 8]"),
                            (net + size + ["--output_guided", "--guided_smoothness", "0"], "--guided_smoothness 0 is outside [1, 64]"),
                            (net + size + ["--output_guided", "--guided_smoothness", "65"], "--guided_smoothness 65 is outside [1, 64]")):
            with pytest.raises(SystemExit) as e:
                main(run + flags)
            assert word in str(e.value), (flags, str(e.value))
        with pytest.raises(SystemExit):
            main(run + net + size + ["--output_guided", "--guided_radius", "2.5"])             # (argparse: not a whole number)
    assert not (tmp_path / "g.y4m").exists() and not (tmp_path / "out").exists()
    # what is taken gets as far as the model
    for run in (vid + net + size + ["--output_guided"], pix + net + size + ["--output_guided", "--guided_radius", "8"],
                pix + ["--frame_size", str(WS), str(H)] + size + ["--output_guided"]):
        with pytest.raises(Exception) as e:
            main(run)
        assert not isinstance(e.value, SystemExit), str(e.value)
    assert not (tmp_path / "g.y4m").exists()
