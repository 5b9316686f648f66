"""--video_batch and --precision of stylize_webcam.py, run in-process with main(argv) (tests/test_temporal_batch_stream.py holds the
sequence lanes against the restatement): absent from the namespace unless given, refused before the model loads when out of range or in a
combination that is not taken, and file to file the bytes of a lane built as the script builds its lanes and fed the same padded batches."""
import os

import numpy as np
import pytest
from PIL import Image

from tests.test_compose_cli import H, OPT, W, main, video
from tests.test_temporal_obmc_cli import parting
from tests.test_video_deep import read_stream, samples_of, write_stream

STAGE = ["--temporal_strength", "0.8", "--temporal_levels", "2", "--temporal_subpel", "2", "--temporal_overlap", "1"]


def test_the_flags_and_what_they_give():
    import stylize_webcam
    parse = stylize_webcam.setup_parser().parse_args
    for argv in ([], ["--temporal_strength", "0.6"], ["--video_in", "x.y4m"]):
        assert "video_batch" not in vars(parse(argv)) and "precision" not in vars(parse(argv))
    assert vars(parse(["--video_batch", "8"]))["video_batch"] == 8 and "precision" not in vars(parse(["--video_batch", "8"]))
    assert vars(parse(["--precision", "bf16"]))["precision"] == "bf16" and "video_batch" not in vars(parse(["--precision", "bf16"]))
    assert stylize_webcam.batch_options(parse([])) == (1, False)
    assert stylize_webcam.batch_options(parse(["--precision", "fp32"])) == (1, False)
    assert stylize_webcam.batch_options(parse(["--video_in", "x", "--video_batch", "1"])) == (1, False)
    assert stylize_webcam.batch_options(parse(["--video_in", "x", "--video_batch", "64", "--precision", "bf16"])) == (64, True)
    assert stylize_webcam.batch_options(parse(["--frames_dir", "d", "--precision", "bf16"])) == (1, True)
    text = stylize_webcam.setup_parser().format_help()
    assert "--video_batch" in text and "latency" in text and "--precision" in text


def test_bad_flags_exit_before_the_model_loads(tmp_path):
    # (no usable --model_path in any of these: a run that got as far as loading the model would fail otherwise)
    nomodel = ["--model_path", str(tmp_path / "none.ckpt")]
    write_stream(str(tmp_path / "f.y4m"), OPT, W, H, [samples_of(OPT, W, H, 1)])
    vid = nomodel + ["--video_in", str(tmp_path / "f.y4m"), "--video_out", str(tmp_path / "g.y4m")]
    d = tmp_path / "in"
    d.mkdir()
    Image.fromarray(np.zeros((H, W, 3), np.uint8)).save(str(d / "000.png"))
    pix = nomodel + ["--frames_dir", str(d), "--output_dir", str(tmp_path / "out")]
    for v in ("0", "-1", "65"):
        with pytest.raises(SystemExit) as e:
            main(vid + ["--video_batch", v])
        assert "--video_batch" in str(e.value) and "[1, 64]" in str(e.value)
    with pytest.raises(SystemExit):
        main(vid + ["--video_batch", "2.5"])                                                # (argparse: not a whole number)
    for run in (pix, nomodel):                                                              # a directory of frames, the camera
        with pytest.raises(SystemExit) as e:
            main(run + ["--video_batch", "2"])
        assert "--video_batch" in str(e.value) and "--video_in" in str(e.value)
    for run in (vid, pix, nomodel, vid + ["--video_batch", "2"]):
        with pytest.raises(SystemExit) as e:
            main(run + ["--precision", "bf16", "--upsample_method", "deconv"])
        assert "--precision" in str(e.value) and "deconv" in str(e.value)
        with pytest.raises(SystemExit):
            main(run + ["--precision", "fp16"])                                             # (argparse: not a choice)
    with pytest.raises(SystemExit) as e:                                                    # the other flags keep their messages beside them
        main(vid + ["--video_batch", "2", "--temporal_overlap", "1"])
    assert "--temporal_strength" in str(e.value)
    assert not (tmp_path / "g.y4m").exists() and not (tmp_path / "out").exists()


def padded(frames, n):
    """The frames in batches of n, the last one padded by repeating its last frame -> [(uint8 [n, frame_bytes], how many are real), ...]"""
    out = []
    for k in range(0, len(frames), n):
        part = list(frames[k:k + n])
        out.append((np.stack(part + [part[-1]] * (n - len(part))), len(part)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("stage", [False, True], ids=["plain", "temporal"])
def test_a_batched_run_writes_the_frames_of_the_lane(tmp_path, stage):
    """Seven 4:2:0 frames, three per pass: seven frames come out, those of a lane built as the script builds its lanes (with sequence=True
    when the stage is on) and fed the same padded batches."""
    import stylize_webcam
    from faststyle_amd import stream
    from tests.backends import get_engine
    from tests.test_compose_stream import variables
    eng = get_engine("hip")
    frames = parting(7)
    argv = video(tmp_path, frames) + ["--video_out", str(tmp_path / "g.y4m"), "--video_batch", "3"] + (STAGE if stage else [])
    main(argv)
    got = read_stream(str(tmp_path / "g.y4m"))[2]
    assert len(got) == 7
    kw = dict(batch=3, swap_rb=False, yuv_out=OPT, source=dict(height=H, width=W, swap_rb=True, yuv=OPT))
    if stage:
        temporal = stylize_webcam.temporal_options(stylize_webcam.setup_parser().parse_args(argv), "bt709")
        assert temporal == dict(strength=0.8, sensitivity=16, radius=7, matrix="bt709", source_bgr=True, levels=2, subpel=2, overlap=1)
        kw["temporal"] = dict(temporal, sequence=True)
    lane = stream.FrameStylizer(eng, variables(eng), H, W, **kw)
    want = []
    for batch, real in padded(frames, 3):
        want += list(lane(batch)[:real])
    assert len(want) == 7 and all(np.array_equal(g, w) for g, w in zip(got, want))
    if stage:                                                                               # (the recursion ran: the run without the stage differs)
        main(video(tmp_path, frames, "p.y4m") + ["--video_out", str(tmp_path / "p_out.y4m"), "--video_batch", "3"])
        plain = read_stream(str(tmp_path / "p_out.y4m"))[2]
        assert np.array_equal(plain[0], got[0]) and any(not np.array_equal(a, b) for a, b in zip(plain[1:], got[1:]))
    lane.release()


@pytest.mark.gpu
def test_batch_one_and_fp32_are_the_run_without_them_and_bf16_is_the_bf16_lane(tmp_path):
    from faststyle_amd import stream
    from tests.backends import get_engine
    from tests.test_compose_stream import variables
    eng = get_engine("hip")
    out = lambda name: str(tmp_path / name)
    frames = parting(3)
    common = video(tmp_path, frames) + ["--temporal_strength", "0.8"]
    main(common + ["--video_out", out("a.y4m")])
    main(common + ["--video_out", out("b.y4m"), "--video_batch", "1", "--precision", "fp32"])
    assert open(out("a.y4m"), "rb").read() == open(out("b.y4m"), "rb").read()
    main(common + ["--video_out", out("c.y4m"), "--precision", "bf16"])
    got = read_stream(out("c.y4m"))[2]
    lane = stream.FrameStylizer(eng, variables(eng), H, W, bf16=True, swap_rb=False, yuv_out=OPT, source=dict(height=H, width=W, swap_rb=True, yuv=OPT),
                                temporal=dict(strength=0.8, sensitivity=16, radius=7, matrix="bt709", source_bgr=True))
    assert len(got) == 3 and all(np.array_equal(g, lane(f)) for g, f in zip(got, frames))
    assert any(not np.array_equal(g, a) for g, a in zip(got, read_stream(out("a.y4m"))[2]))     # (another arithmetic than fp32's)
    lane.release()


@pytest.mark.gpu
def test_a_truncated_stream_writes_what_was_read(tmp_path, capsys):
    """Five frames, the fifth cut in half, three per pass: the second pass has one real frame; four frames are written, the count says
    four, and the run ends with the reader's message"""
    frames = parting(5)
    argv = video(tmp_path, frames)
    src = argv[argv.index("--video_in") + 1]
    raw = open(src, "rb").read()
    with open(src, "wb") as f:
        f.write(raw[:len(raw) - frames[0].size // 2])
    main(video(tmp_path, frames[:4], "whole.y4m") + ["--video_out", str(tmp_path / "w.y4m"), "--video_batch", "3"])
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        main(argv + ["--video_out", str(tmp_path / "g.y4m"), "--video_batch", "3"])
    assert "--video_in" in str(e.value) and "the stream ends after" in str(e.value)
    assert "\n4 frames\n" in capsys.readouterr().out                                        # (the real frames, not the padded pass)
    got, want = read_stream(str(tmp_path / "g.y4m"))[2], read_stream(str(tmp_path / "w.y4m"))[2]
    assert len(got) == 4 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert os.path.getsize(str(tmp_path / "g.y4m")) == os.path.getsize(str(tmp_path / "w.y4m"))
