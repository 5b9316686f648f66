"""--temporal_levels of stylize_webcam.py, run in-process with main(argv) (tests/test_temporal_pyr_stream.py holds the lanes against the
restatement): absent from the namespace unless given, refused before the model loads when out of range or without --temporal_strength, a
still picture stays the first frame at full strength with three levels, and a moving sequence runs end to end with two, on a video stream
and on a directory of frames."""
import numpy as np
import pytest
from PIL import Image

from tests.test_compose_cli import H, OPT, W, files, frames_dir, main, video
from tests.test_video_deep import read_stream, samples_of, write_stream


def test_the_flag_and_what_the_lanes_are_given():
    import stylize_webcam
    parse = stylize_webcam.setup_parser().parse_args
    assert "temporal_levels" not in vars(parse([])) and "temporal_levels" not in vars(parse(["--temporal_strength", "0.6"]))
    assert vars(parse(["--temporal_levels", "3"]))["temporal_levels"] == 3
    base = dict(strength=0.6, sensitivity=16, radius=7, matrix="bt601", source_bgr=True)
    assert stylize_webcam.temporal_options(parse(["--temporal_strength", "0.6"])) == base       # (without the flag: the dict it always was)
    for n in (1, 2, 3):
        assert stylize_webcam.temporal_options(parse(["--temporal_strength", "0.6", "--temporal_levels", str(n)])) == dict(base, levels=n)


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
        for v in ("0", "4", "-1"):
            with pytest.raises(SystemExit) as e:
                main(run + ["--temporal_strength", "0.5", "--temporal_levels", v])
            assert "--temporal_levels" in str(e.value) and "[1, 3]" in str(e.value)
        with pytest.raises(SystemExit) as e:                                                # without the stage
            main(run + ["--temporal_levels", "2"])
        assert "--temporal_levels" in str(e.value) and "--temporal_strength" in str(e.value)
        with pytest.raises(SystemExit):
            main(run + ["--temporal_levels", "2.5", "--temporal_strength", "0.5"])          # (argparse: not a whole number)
        with pytest.raises(SystemExit) as e:                                                # the radius keeps its range and its message
            main(run + ["--temporal_strength", "0.5", "--temporal_levels", "3", "--temporal_radius", "8"])
        assert "--temporal_radius 8 is outside [0, 7]" in str(e.value)
    assert not (tmp_path / "g.y4m").exists() and not (tmp_path / "out").exists()


@pytest.mark.gpu
def test_a_still_video_stays_its_first_frame_with_three_levels(tmp_path):
    still = samples_of(OPT, W, H, 50)
    out = lambda name: str(tmp_path / name)
    main(video(tmp_path, [still] * 5) + ["--video_out", out("plain.y4m")])
    main(video(tmp_path, [still] * 5) + ["--video_out", out("full.y4m"), "--temporal_strength", "1", "--temporal_sensitivity", "256",
                                         "--temporal_levels", "3"])
    got = read_stream(out("full.y4m"))[2]
    assert len(got) == 5 and all(np.array_equal(g, got[0]) for g in got[1:])
    assert np.array_equal(got[0], read_stream(out("plain.y4m"))[2][0])                      # (a first frame is not blended)
    # one level by the flag: the bytes of the run without it
    main(video(tmp_path, [still] * 5) + ["--video_out", out("a.y4m"), "--temporal_strength", "0.5"])
    main(video(tmp_path, [still] * 5) + ["--video_out", out("b.y4m"), "--temporal_strength", "0.5", "--temporal_levels", "1"])
    assert open(out("a.y4m"), "rb").read() == open(out("b.y4m"), "rb").read()


@pytest.mark.gpu
def test_a_moving_sequence_runs_end_to_end_with_two_levels(tmp_path):
    out = lambda name: str(tmp_path / name)
    moving = [samples_of(OPT, W, H, 60 + (k >> 1)) for k in range(5)]
    main(video(tmp_path, moving, "m.y4m") + ["--video_out", out("mplain.y4m")])
    main(video(tmp_path, moving, "m.y4m") + ["--video_out", out("mhalf.y4m"), "--temporal_strength", "0.5", "--temporal_levels", "2"])
    a, b = read_stream(out("mplain.y4m"))[2], read_stream(out("mhalf.y4m"))[2]
    assert len(a) == len(b) == 5 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[2], b[2])
    # a directory of frames: a picture that moves by 10 pixels per frame; the first frame is the plain one, the others are blended
    rng = np.random.default_rng(8)
    wide = rng.integers(0, 256, (H, W + 40, 3), dtype=np.uint8)
    frames = [np.ascontiguousarray(wide[:, 10 * k:10 * k + W]) for k in range(4)]
    main(frames_dir(tmp_path, frames, "a") + ["--output_dir", out("plain")])
    main(frames_dir(tmp_path, frames, "b") + ["--output_dir", out("pyr"), "--temporal_strength", "0.8", "--temporal_levels", "2"])
    got, plain = files(out("pyr")), files(out("plain"))
    assert len(got) == len(plain) == 4 and got[0] == plain[0] and all(g != p for g, p in zip(got[1:], plain[1:]))
