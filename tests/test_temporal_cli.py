"""--temporal_strength / --temporal_radius / --temporal_sensitivity of stylize_webcam.py, run in-process with main(argv)
(tests/test_temporal_stream.py holds the lanes against the restatement): a still picture stays the first frame at full strength, strength 0
reproduces the run without the flag byte for byte, on a video stream and on a directory of frames, and bad flags exit before the model
loads."""
import numpy as np
import pytest
from PIL import Image

from tests.test_compose_cli import H, OPT, W, files, frames_dir, main, video
from tests.test_video_deep import read_stream, samples_of, write_stream


@pytest.mark.gpu
def test_a_still_video_stays_its_first_frame_and_strength_zero_changes_nothing(tmp_path):
    still = samples_of(OPT, W, H, 50)
    out = lambda name: str(tmp_path / name)
    main(video(tmp_path, [still] * 5) + ["--video_out", out("plain.y4m")])
    main(video(tmp_path, [still] * 5) + ["--video_out", out("zero.y4m"), "--temporal_strength", "0"])
    main(video(tmp_path, [still] * 5) + ["--video_out", out("full.y4m"), "--temporal_strength", "1", "--temporal_sensitivity", "256"])
    assert open(out("plain.y4m"), "rb").read() == open(out("zero.y4m"), "rb").read()
    got = read_stream(out("full.y4m"))[2]
    assert len(got) == 5 and all(np.array_equal(g, got[0]) for g in got[1:])
    assert np.array_equal(got[0], read_stream(out("plain.y4m"))[2][0])                      # (a first frame is not blended)
    # moving frames at an in-between strength: another stream than the plain one, of as many frames
    moving = [samples_of(OPT, W, H, 60 + (k >> 1)) for k in range(5)]
    main(video(tmp_path, moving, "m.y4m") + ["--video_out", out("mplain.y4m")])
    main(video(tmp_path, moving, "m.y4m") + ["--video_out", out("mhalf.y4m"), "--temporal_strength", "0.5", "--temporal_radius", "3"])
    a, b = read_stream(out("mplain.y4m"))[2], read_stream(out("mhalf.y4m"))[2]
    assert len(a) == len(b) == 5 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[2], b[2])


@pytest.mark.gpu
def test_a_still_directory_stays_its_first_frame_and_strength_zero_changes_nothing(tmp_path):
    rng = np.random.default_rng(6)
    still = rng.integers(0, 256, (H - 3, W - 2, 3), dtype=np.uint8)                          # (53 x 70: the output is larger)
    out = lambda name: str(tmp_path / name)
    main(frames_dir(tmp_path, [still] * 5, "a") + ["--output_dir", out("plain")])
    main(frames_dir(tmp_path, [still] * 5, "b") + ["--output_dir", out("zero"), "--temporal_strength", "0"])
    main(frames_dir(tmp_path, [still] * 5, "c") + ["--output_dir", out("full"), "--temporal_strength", "1"])
    assert len(files(out("plain"))) == 5 and files(out("plain")) == files(out("zero"))
    got = files(out("full"))
    assert len(got) == 5 and all(g == got[0] for g in got[1:]) and got[0] == files(out("plain"))[0]
    # the same through the encoder, and a frame of another size in the middle starts over: its first frame is the plain one
    other = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mixed = [still, still, other, other, still]
    jpg = ["--output_format", "jpg", "--temporal_strength", "1"]
    main(frames_dir(tmp_path, mixed, "d") + ["--output_dir", out("mixed")] + jpg)
    main(frames_dir(tmp_path, mixed, "e") + ["--output_dir", out("mixed_plain"), "--output_format", "jpg"])
    got, plain = files(out("mixed")), files(out("mixed_plain"))
    assert len(got) == 5 and got[0] == got[1] == plain[0] and got[2] == got[3] == plain[2] and got[4] == plain[4]


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
        for flag, values in (("--temporal_strength", ("1.5", "-0.25", "nan")), ("--temporal_radius", ("-1", "8")),
                             ("--temporal_sensitivity", ("0", "257"))):
            for v in values:
                with pytest.raises(SystemExit) as e:
                    main(run + ["--temporal_strength", "0.5"] * (flag != "--temporal_strength") + [flag, v])
                assert flag in str(e.value)
        with pytest.raises(SystemExit) as e:                                                # a bad radius is refused without the stage, too
            main(run + ["--temporal_radius", "9"])
        assert "--temporal_radius" in str(e.value)
        with pytest.raises(SystemExit):
            main(run + ["--temporal_radius", "2.5", "--temporal_strength", "0.5"])          # (argparse: not a whole number)
    assert not (tmp_path / "g.y4m").exists() and not (tmp_path / "out").exists()


def test_flags_and_what_the_lanes_are_given():
    import stylize_webcam
    parse = stylize_webcam.setup_parser().parse_args
    assert not any(k.startswith("temporal") for k in vars(parse([])))                       # absent unless given: the defaults of the others stand
    assert stylize_webcam.temporal_options(parse([])) is None                               # no flag: no stage
    assert stylize_webcam.temporal_options(parse(["--temporal_radius", "3"])) is None
    for flags, matrix, want in ((["--temporal_strength", "0.6"], "bt601", dict(strength=0.6, sensitivity=16, radius=7, matrix="bt601", source_bgr=True)),
                                (["--temporal_strength", "1", "--temporal_radius", "0", "--temporal_sensitivity", "256"], "bt709",
                                 dict(strength=1.0, sensitivity=256, radius=0, matrix="bt709", source_bgr=True)),
                                (["--temporal_strength", "0", "--color_matrix", "bt601"], "bt709",
                                 dict(strength=0.0, sensitivity=16, radius=7, matrix="bt601", source_bgr=True))):
        assert stylize_webcam.temporal_options(parse(flags), matrix) == want
