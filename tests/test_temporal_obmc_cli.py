"""--temporal_overlap of stylize_webcam.py, run in-process with main(argv) (tests/test_temporal_obmc_stream.py holds the lanes against the
restatement): absent from the namespace unless given, refused before the model loads when out of range or without --temporal_strength, and
file to file the bytes of a lane built with the same options, alone and with --temporal_levels and --temporal_subpel."""
import numpy as np
import pytest
from PIL import Image

from tests.test_compose_cli import H, OPT, W, main, video
from tests.test_video_deep import read_stream, samples_of, write_stream


def test_the_flag_and_what_the_lanes_are_given():
    import stylize_webcam
    parse = stylize_webcam.setup_parser().parse_args
    assert "temporal_overlap" not in vars(parse([])) and "temporal_overlap" not in vars(parse(["--temporal_strength", "0.6"]))
    assert "temporal_overlap" not in vars(parse(["--temporal_strength", "0.6", "--temporal_levels", "2", "--temporal_subpel", "2"]))
    assert vars(parse(["--temporal_overlap", "1"]))["temporal_overlap"] == 1
    base = dict(strength=0.6, sensitivity=16, radius=7, matrix="bt601", source_bgr=True)
    assert stylize_webcam.temporal_options(parse(["--temporal_strength", "0.6"])) == base       # (without the flag: the dict it always was)
    for n in (0, 1):
        assert stylize_webcam.temporal_options(parse(["--temporal_strength", "0.6", "--temporal_overlap", str(n)])) == dict(base, overlap=n)
    every = parse(["--temporal_strength", "0.6", "--temporal_overlap", "1", "--temporal_subpel", "2", "--temporal_levels", "3"])
    assert stylize_webcam.temporal_options(every) == dict(base, levels=3, subpel=2, overlap=1)


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
        for v in ("2", "-1"):
            with pytest.raises(SystemExit) as e:
                main(run + ["--temporal_strength", "0.5", "--temporal_overlap", v])
            assert "--temporal_overlap" in str(e.value) and "[0, 1]" in str(e.value)
        with pytest.raises(SystemExit) as e:                                                # without the stage
            main(run + ["--temporal_overlap", "1"])
        assert "--temporal_overlap" in str(e.value) and "--temporal_strength" in str(e.value)
        with pytest.raises(SystemExit) as e:                                                # ... also beside the other two
            main(run + ["--temporal_overlap", "1", "--temporal_levels", "2", "--temporal_subpel", "2"])
        assert "--temporal_strength" in str(e.value)
        with pytest.raises(SystemExit):
            main(run + ["--temporal_overlap", "0.5", "--temporal_strength", "0.5"])         # (argparse: not a whole number)
        with pytest.raises(SystemExit) as e:                                                # the others keep their ranges and their messages
            main(run + ["--temporal_strength", "0.5", "--temporal_overlap", "1", "--temporal_subpel", "3"])
        assert "--temporal_subpel 3 is outside [0, 2]" in str(e.value)
    assert not (tmp_path / "g.y4m").exists() and not (tmp_path / "out").exists()


def parting(n):
    """n frames of one noise picture whose halves move apart by two pixels per frame, the edge in mid-block, as C420jpeg planes"""
    from tests.test_temporal_obmc_stream import apart
    from tests.test_yuv import rgb_to_frame
    rgb = [np.repeat(np.repeat(np.random.RandomState(30).randint(0, 256, (H // 2, W // 2, 3)).astype(np.uint8), 2, axis=0), 2, axis=1)]
    for _ in range(n - 1):
        rgb.append(apart(rgb[-1], 1))
    return [rgb_to_frame(np.ascontiguousarray(f), matrix=1, full_range=1) for f in rgb]


@pytest.mark.gpu
def test_video_runs_write_the_files_of_the_lanes(tmp_path):
    """File to file against the lane: a run with --temporal_overlap 1 (alone and with the other two flags) writes the frames of a
    FrameStylizer built as the script builds its lanes, with the dict temporal_options returns; they differ from the run without the flag
    from the first blended frame on, and --temporal_overlap 0 writes the bytes of the run without it."""
    import stylize_webcam
    from faststyle_amd import stream
    from tests.backends import get_engine
    from tests.test_compose_stream import variables
    eng = get_engine("hip")
    out = lambda name: str(tmp_path / name)
    frames = parting(4)
    common = video(tmp_path, frames) + ["--temporal_strength", "0.8"]
    main(common + ["--video_out", out("whole.y4m")])
    main(common + ["--video_out", out("zero.y4m"), "--temporal_overlap", "0"])
    assert open(out("whole.y4m"), "rb").read() == open(out("zero.y4m"), "rb").read()
    whole = read_stream(out("whole.y4m"))[2]
    parse = stylize_webcam.setup_parser().parse_args
    kw = dict(swap_rb=False, yuv_out=OPT, source=dict(height=H, width=W, swap_rb=True, yuv=OPT))
    for name, more in (("over.y4m", ["--temporal_overlap", "1"]), ("every.y4m", ["--temporal_overlap", "1", "--temporal_subpel", "2", "--temporal_levels", "2"])):
        argv = common + ["--video_out", out(name)] + more
        main(argv)
        got = read_stream(out(name))[2]
        assert len(got) == len(whole) == 4 and np.array_equal(got[0], whole[0]) and any(not np.array_equal(g, w) for g, w in zip(got[1:], whole[1:]))
        temporal = stylize_webcam.temporal_options(parse(argv), "bt709")
        assert temporal["overlap"] == 1 and temporal["matrix"] == "bt709"
        lane = stream.FrameStylizer(eng, variables(eng), H, W, temporal=temporal, **kw)
        assert all(np.array_equal(g, lane(f)) for g, f in zip(got, frames))
        assert len({tuple(v) for v in lane.motion_vectors().reshape(-1, 2).tolist()}) > 1    # (the blocks did move differently)
        lane.release()
