"""--video_also of stylize_webcam.py, run in-process with main(argv) (tests/test_temporal_streams_stream.py holds the lanes against the
restatement): absent from the namespace unless given, every refusal before the model loads -- a stream whose header differs from the first
one's is named with the field --, and file to file every stream's output is its input's frames through a lane fed the same rows and
activity: with --temporal_strength a streams lane, without it a plain batch lane.  A stream that breaks off leaves the others complete."""
import numpy as np
import pytest

from tests.test_compose_cli import H, MODEL, OPT, W, main
from tests.test_video_deep import DEEP, read_stream, samples_of, write_stream


def test_the_flag_is_absent_unless_given():
    import stylize_webcam
    parse = stylize_webcam.setup_parser().parse_args
    assert "video_also" not in vars(parse([])) and "video_also" not in vars(parse(["--video_in", "a", "--video_out", "b", "--temporal_strength", "0.5"]))
    got = vars(parse(["--video_also", "a", "b", "--video_in", "x", "--video_also", "c", "d"]))["video_also"]
    assert got == [["a", "b"], ["c", "d"]]
    assert stylize_webcam.also_options(parse(["--video_in", "x", "--video_out", "y"])) == []
    assert stylize_webcam.also_options(parse(["--video_in", "x", "--video_out", "y", "--video_also", "a", "b"])) == [("a", "b")]
    assert stylize_webcam.also_options(parse(["--video_in", "-", "--video_out", "-", "--video_also", "a", "b"])) == [("a", "b")]
    assert stylize_webcam.also_options(parse(["--video_in", "x", "--video_out", "y", "--video_also", "-", "-"])) == [("-", "-")]


def test_bad_flags_exit_before_the_model_loads(tmp_path):
    # (no usable --model_path in any of these: a run that got as far as loading the model would fail otherwise)
    nomodel = ["--model_path", str(tmp_path / "none.ckpt")]
    p = lambda name: str(tmp_path / name)
    for name in ("a.y4m", "b.y4m"):
        write_stream(p(name), OPT, W, H, [samples_of(OPT, W, H, 1)])
    vid = nomodel + ["--video_in", p("a.y4m"), "--video_out", p("ao.y4m")]
    also = ["--video_also", p("b.y4m"), p("bo.y4m")]

    def refused(argv, *words):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert all(w in str(e.value) for w in words), str(e.value)

    refused(nomodel + also, "--video_also", "--video_in")
    refused(nomodel + ["--video_in", p("a.y4m")] + also, "--video_also", "--video_out")
    refused(nomodel + ["--frames_dir", p("."), "--output_dir", p("out")] + also, "--video_also", "--video_in")
    refused(vid + also + ["--video_batch", "2"], "--video_also", "--video_batch")
    refused(vid + also + ["--video_batch", "1"], "--video_also", "--video_batch")
    many = [w for k in range(64) for w in ("--video_also", p("i%d.y4m" % k), p("o%d.y4m" % k))]
    refused(vid + many, "64 times", "63")
    refused(nomodel + ["--video_in", "-", "--video_out", p("ao.y4m"), "--video_also", "-", p("bo.y4m")], "-", "input")
    refused(vid + ["--video_also", "-", p("bo.y4m"), "--video_also", "-", p("co.y4m")], "-", "input")
    refused(nomodel + ["--video_in", p("a.y4m"), "--video_out", "-", "--video_also", p("b.y4m"), "-"], "-", "output")
    refused(vid + ["--video_also", p("a.y4m"), p("bo.y4m")], "a.y4m", "more than once")
    refused(vid + ["--video_also", p("b.y4m"), p("ao.y4m")], "ao.y4m", "more than once")
    refused(vid + ["--video_also", p("b.y4m"), p("b.y4m")], "b.y4m", "more than once")
    refused(vid + also + ["--video_also", p("b.y4m"), p("co.y4m")], "b.y4m", "more than once")
    with pytest.raises(SystemExit):
        main(vid + ["--video_also", p("b.y4m")])                                                # (argparse: two names)
    # a further stream whose header is not the first one's: named with the field
    other = dict(OPT, sampling=(1, 1))
    for name, opt, w, h, field in (("wide.y4m", OPT, W + 2, H, "width"), ("tall.y4m", OPT, W, H + 2, "height"), ("444.y4m", other, W, H, "sampling"),
                                   ("sited.y4m", dict(OPT, sampling=(2, 2), siting=1), W, H, "siting"), ("limited.y4m", dict(OPT, full_range=False), W, H, "range"),
                                   ("mono.y4m", dict(OPT, sampling=(1, 1), components=1), W, H, "components")):
        write_stream(p(name), opt, w, h, [samples_of(opt, w, h, 2)])
        refused(vid + also + ["--video_also", p(name), p("x.y4m")], "--video_also", name, field)
    deep = DEEP["420p10"]
    write_stream(p("deep.y4m"), deep, W, H, [samples_of(deep, W, H, 2)])
    write_stream(p("full.y4m"), dict(OPT, full_range=False), W, H, [samples_of(OPT, W, H, 2)])
    refused(nomodel + ["--video_in", p("full.y4m"), "--video_out", p("ao.y4m"), "--video_depth", "stream", "--video_also", p("deep.y4m"), p("x.y4m")],
            "--video_also", "deep.y4m", "bits")
    open(p("junk.y4m"), "wb").write(b"not a stream\n")
    refused(vid + ["--video_also", p("junk.y4m"), p("x.y4m")], "--video_also", "junk.y4m")
    assert not any((tmp_path / n).exists() for n in ("ao.y4m", "bo.y4m", "co.y4m", "x.y4m", "out"))


def moving(n, seed):
    """n frames of one noise picture whose halves move apart by two pixels per frame, as C420jpeg planes; another picture per seed"""
    from tests.test_temporal_obmc_stream import apart
    from tests.test_yuv import rgb_to_frame
    rgb = [np.repeat(np.repeat(np.random.RandomState(seed).randint(0, 256, (H // 2, W // 2, 3)).astype(np.uint8), 2, axis=0), 2, axis=1)]
    for _ in range(n - 1):
        rgb.append(apart(rgb[-1], 1))
    return [rgb_to_frame(np.ascontiguousarray(f), matrix=1, full_range=1) for f in rgb]


def lane_outputs(lane, streams, temporal):
    """The frames of every stream through a batch lane fed as the script feeds it: one frame of every open stream per pass, a row of a
    stream that has ended left as it is, and (temporal) that stream inactive -> per stream its output frames"""
    S = len(streams)
    buf = np.zeros((S,) + streams[0][0].shape, np.uint8)
    outs = [[] for _ in streams]
    for k in range(max(len(s) for s in streams)):
        is_open = [k < len(s) for s in streams]
        for s in range(S):
            if is_open[s]:
                buf[s] = streams[s][k]
        if temporal:
            lane.set_streams(is_open)
        got = lane(buf)
        for s in range(S):
            if is_open[s]:
                outs[s].append(got[s])
    return outs


@pytest.mark.gpu
def test_three_streams_write_the_files_of_the_lanes(tmp_path):
    import stylize_webcam
    from faststyle_amd import stream
    from tests.backends import get_engine
    from tests.test_compose_stream import variables
    eng = get_engine("hip")
    p = lambda name: str(tmp_path / name)
    streams = [moving(5, 31), moving(3, 32), moving(4, 33)]
    for k, frames in enumerate(streams):
        write_stream(p("in%d.y4m" % k), OPT, W, H, frames, rate=(25 + k, 1))
    parse = stylize_webcam.setup_parser().parse_args
    kw = dict(swap_rb=False, yuv_out=OPT, source=dict(height=H, width=W, swap_rb=True, yuv=OPT))
    results = {}
    for tag, more in (("plain", []), ("stab", ["--temporal_strength", "0.8", "--temporal_overlap", "1", "--temporal_subpel", "2"])):
        argv = MODEL + ["--video_matrix", "bt709", "--video_in", p("in0.y4m"), "--video_out", p(tag + "0.y4m"),
                        "--video_also", p("in1.y4m"), p(tag + "1.y4m"), "--video_also", p("in2.y4m"), p(tag + "2.y4m")] + more
        main(argv)
        temporal = stylize_webcam.temporal_options(parse(argv), "bt709")
        assert (temporal is not None) == bool(more)
        lane = stream.FrameStylizer(eng, variables(eng), H, W, batch=3, temporal=None if temporal is None else dict(temporal, streams=True), **kw)
        want = lane_outputs(lane, streams, temporal is not None)
        lane.release()
        for k, frames in enumerate(streams):
            head, fmt, got = read_stream(p("%s%d.y4m" % (tag, k)))
            assert fmt.rate == (25 + k, 1) and (fmt.width, fmt.height) == (W, H)                # (every output carries its own input's rate)
            assert len(got) == len(frames) and all(np.array_equal(g, w) for g, w in zip(got, want[k])), (tag, k)
        results[tag] = want
    # the stage did something, from every stream's second frame on
    assert all(np.array_equal(a[0], b[0]) and not np.array_equal(a[1], b[1]) for a, b in zip(results["plain"], results["stab"]))


@pytest.mark.gpu
def test_a_truncated_stream_leaves_the_others_complete(tmp_path):
    p = lambda name: str(tmp_path / name)
    streams = [moving(4, 41), moving(4, 42), moving(3, 43)]
    for k, frames in enumerate(streams):
        write_stream(p("in%d.y4m" % k), OPT, W, H, frames)
    whole = open(p("in1.y4m"), "rb").read()
    open(p("in1.y4m"), "wb").write(whole[:len(whole) - streams[1][0].size // 2])                # the fourth frame breaks off
    argv = MODEL + ["--video_matrix", "bt709", "--video_in", p("in0.y4m"), "--video_out", p("out0.y4m"), "--video_also", p("in1.y4m"), p("out1.y4m"),
                    "--video_also", p("in2.y4m"), p("out2.y4m"), "--temporal_strength", "0.6"]
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert "--video_also" in str(e.value) and "in1.y4m" in str(e.value) and "in0.y4m" not in str(e.value) and "in2.y4m" not in str(e.value)
    assert [len(read_stream(p("out%d.y4m" % k))[2]) for k in range(3)] == [4, 3, 3]
    # the complete streams' files are those of the run in which the second stream simply ends after three frames
    write_stream(p("in1.y4m"), OPT, W, H, streams[1][:3])
    main([p("ref" + a[-5:]) if a.startswith(p("out")) else a for a in argv])
    for k in range(3):
        assert open(p("out%d.y4m" % k), "rb").read() == open(p("ref%d.y4m" % k), "rb").read()
