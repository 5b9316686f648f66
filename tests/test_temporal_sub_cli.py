"""--temporal_subpel of stylize_webcam.py, run in-process with main(argv) (tests/test_temporal_sub_stream.py holds the lanes against the
restatement): absent from the namespace unless given, refused before the model loads when out of range or without --temporal_strength, and
file to file the bytes of a lane built with the same options, alone and with --temporal_levels."""
import numpy as np
import pytest
from PIL import Image

from tests.test_compose_cli import H, OPT, W, main, video
from tests.test_video_deep import read_stream, samples_of, write_stream


def test_the_flag_and_what_the_lanes_are_given():
    import stylize_webcam
    parse = stylize_webcam.setup_parser().parse_args
    assert "temporal_subpel" not in vars(parse([])) and "temporal_subpel" not in vars(parse(["--temporal_strength", "0.6"]))
    assert "temporal_subpel" not in vars(parse(["--temporal_strength", "0.6", "--temporal_levels", "2"]))
    assert vars(parse(["--temporal_subpel", "2"]))["temporal_subpel"] == 2
    base = dict(strength=0.6, sensitivity=16, radius=7, matrix="bt601", source_bgr=True)
    assert stylize_webcam.temporal_options(parse(["--temporal_strength", "0.6"])) == base       # (without the flag: the dict it always was)
    for n in (0, 1, 2):
        assert stylize_webcam.temporal_options(parse(["--temporal_strength", "0.6", "--temporal_subpel", str(n)])) == dict(base, subpel=n)
    both = parse(["--temporal_strength", "0.6", "--temporal_subpel", "2", "--temporal_levels", "3"])
    assert stylize_webcam.temporal_options(both) == dict(base, levels=3, subpel=2)


def test_bad_flags_exit_before_the_model_loads(tmp_path):
    # (no usable --model_path in any of these: a run that got as far as loading the model would fail otherwise)
    nomodel = ["--model_path", str(tmp_path / "none.ckpt")]
    write_stream(str(tmp_path / "f.y4m"), OPT, W, H, [samples_of(OPT, W, H, 1)])
    vid = nomodel + ["--video_in", str(tmp_path / "f.y4m"), "--video_out", str(tmp_path / "g.y4m")]
    d = tmp_path / "in"
    d.mkdir()
    Image.fromarray(np.zeros((H, W, 3), np.uint8)).save(str(d / "000.png"))
    pix = nomodel + ["--frames_dir", str(d), "--output_dir", str(tmp_path / "out")]
    for run in (vid, pix):
        for v in ("3", "-1"):
            with pytest.raises(SystemExit) as e:
                main(run + ["--temporal_strength", "0.5", "--temporal_subpel", v])
            assert "--temporal_subpel" in str(e.value) and "[0, 2]" in str(e.value)
        with pytest.raises(SystemExit) as e:                                                # without the stage
            main(run + ["--temporal_subpel", "2"])
        assert "--temporal_subpel" in str(e.value) and "--temporal_strength" in str(e.value)
        with pytest.raises(SystemExit) as e:                                                # ... also beside --temporal_levels
            main(run + ["--temporal_subpel", "2", "--temporal_levels", "2"])
        assert "--temporal_strength" in str(e.value)
        with pytest.raises(SystemExit):
            main(run + ["--temporal_subpel", "1.5", "--temporal_strength", "0.5"])          # (argparse: not a whole number)
        with pytest.raises(SystemExit) as e:                                                # the levels keep their range and their message
            main(run + ["--temporal_strength", "0.5", "--temporal_subpel", "2", "--temporal_levels", "4"])
        assert "--temporal_levels 4 is outside [1, 3]" in str(e.value)
    assert not (tmp_path / "g.y4m").exists() and not (tmp_path / "out").exists()


def drifting(n, step=3):
    """n frames of one smooth picture that drifts by `step` quarter pixels per frame, as C420jpeg planes"""
    from tests.test_temporal_sub import texture_pair
    from tests.test_yuv import rgb_to_frame
    rgb = [np.ascontiguousarray(np.stack([texture_pair(H, W, step * k, -step * k, 20 + c, sigma=4.0)[1] for c in range(3)], axis=-1))
           for k in range(n)]
    return [rgb_to_frame(f, matrix=1, full_range=1) for f in rgb]


@pytest.mark.gpu
def test_video_runs_write_the_files_of_the_lanes(tmp_path):
    """File to file against the lane: a run with --temporal_subpel (alone and with --temporal_levels) writes the frames of a FrameStylizer
    built as the script builds its lanes, with the dict temporal_options returns; they differ from the run without the flag from the first
    blended frame on."""
    import stylize_webcam
    from faststyle_amd import stream
    from tests.backends import get_engine
    from tests.test_compose_stream import variables
    eng = get_engine("hip")
    out = lambda name: str(tmp_path / name)
    frames = drifting(4)
    common = video(tmp_path, frames) + ["--temporal_strength", "0.8"]
    main(common + ["--video_out", out("whole.y4m")])
    whole = read_stream(out("whole.y4m"))[2]
    parse = stylize_webcam.setup_parser().parse_args
    kw = dict(swap_rb=False, yuv_out=OPT, source=dict(height=H, width=W, swap_rb=True, yuv=OPT))
    for name, more in (("sub.y4m", ["--temporal_subpel", "2"]), ("both.y4m", ["--temporal_subpel", "1", "--temporal_levels", "2"])):
        argv = common + ["--video_out", out(name)] + more
        main(argv)
        got = read_stream(out(name))[2]
        assert len(got) == len(whole) == 4 and np.array_equal(got[0], whole[0]) and any(not np.array_equal(g, w) for g, w in zip(got[1:], whole[1:]))
        temporal = stylize_webcam.temporal_options(parse(argv), "bt709")
        assert temporal["subpel"] == int(more[1]) and temporal["matrix"] == "bt709"
        lane = stream.FrameStylizer(eng, variables(eng), H, W, temporal=temporal, **kw)
        assert all(np.array_equal(g, lane(f)) for g, f in zip(got, frames))
        assert (lane.motion_vectors_subpel() & 3).any()                                     # (fractions were found)
        lane.release()


@pytest.mark.gpu
def test_subpel_zero_writes_the_bytes_of_the_run_without_it_and_a_moving_video_runs_with_levels(tmp_path):
    still = samples_of(OPT, W, H, 50)
    out = lambda name: str(tmp_path / name)
    main(video(tmp_path, [still] * 4) + ["--video_out", out("a.y4m"), "--temporal_strength", "0.5"])
    main(video(tmp_path, [still] * 4) + ["--video_out", out("b.y4m"), "--temporal_strength", "0.5", "--temporal_subpel", "0"])
    assert open(out("a.y4m"), "rb").read() == open(out("b.y4m"), "rb").read()
    moving = [samples_of(OPT, W, H, 60 + (k >> 1)) for k in range(4)]
    main(video(tmp_path, moving, "m.y4m") + ["--video_out", out("mplain.y4m")])
    main(video(tmp_path, moving, "m.y4m") + ["--video_out", out("msub.y4m"), "--temporal_strength", "0.5", "--temporal_subpel", "2", "--temporal_levels", "2"])
    a, b = read_stream(out("mplain.y4m"))[2], read_stream(out("msub.y4m"))[2]
    assert len(a) == len(b) == 4 and np.array_equal(a[0], b[0]) and not np.array_equal(a[2], b[2])
