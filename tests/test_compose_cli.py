"""--style_strength / --preserve_color / --color_matrix / --mask_path of stylize_webcam.py, run in-process with main(argv): the files are
those of the lanes (tests/test_compose_stream.py holds the lanes against the restatement), full strength alone reproduces the run without
the flag byte for byte, the source shows through in its own colours on every output kind, and bad flags exit before the model loads."""
import os

import numpy as np
import pytest
from PIL import Image

from faststyle_amd import stream
from tests.backends import get_engine
from tests.test_compose_stream import replicated, variables
from tests.test_video_deep import MODEL, read_stream, ref_args, samples_of, write_stream
from tests.test_yuv import frame_to_rgb, rgb_to_frame

OPT = dict(sampling=(2, 2), siting=0, matrix=1, full_range=True)                            # C420jpeg, full range, --video_matrix bt709
W, H = 72, 56                                                                               # (the net's output has this size too)


def main(argv):
    import stylize_webcam
    stylize_webcam.main(argv)


def video(tmp_path, frames, name="f.y4m"):
    src = str(tmp_path / name)
    write_stream(src, OPT, W, H, frames)
    return MODEL + ["--video_in", src, "--video_matrix", "bt709"]


def frames_dir(tmp_path, images, name="in"):
    d = tmp_path / name
    d.mkdir()
    for k, im in enumerate(images):
        Image.fromarray(im).save(str(d / ("%03d.png" % k)))
    return MODEL + ["--frames_dir", str(d)]


def pngs(d):
    return [np.asarray(Image.open(os.path.join(str(d), n))) for n in sorted(os.listdir(str(d)))]


def files(d):
    return [open(os.path.join(str(d), n), "rb").read() for n in sorted(os.listdir(str(d)))]


@pytest.mark.gpu
def test_video_runs_write_the_files_of_the_lanes(tmp_path):
    eng = get_engine("hip")
    frames = [samples_of(OPT, W, H, 30 + k) for k in range(3)]
    common = video(tmp_path, frames) + ["--style_strength", "0.5", "--preserve_color"]
    # the lanes of such a run: the net is fed B,G,R, the output conversion does not swap, the luma weights are --video_matrix's
    kw = dict(swap_rb=False, source=dict(height=H, width=W, swap_rb=True, yuv=OPT))
    compose = dict(strength=0.5, keep_color=True, matrix="bt709", source_swapped=True)

    main(common + ["--video_out", str(tmp_path / "g.y4m")])
    lane = stream.FrameStylizer(eng, variables(eng), H, W, yuv_out=OPT, compose=compose, **kw)
    got = read_stream(str(tmp_path / "g.y4m"))[2]
    assert len(got) == 3 and all(np.array_equal(g, lane(f)) for g, f in zip(got, frames))
    lane.release()
    # --color_matrix overrides the default
    main(common + ["--video_out", str(tmp_path / "g601.y4m"), "--color_matrix", "bt601"])
    lane = stream.FrameStylizer(eng, variables(eng), H, W, yuv_out=OPT, compose=dict(compose, matrix="bt601"), **kw)
    got601 = read_stream(str(tmp_path / "g601.y4m"))[2]
    assert all(np.array_equal(g, lane(f)) for g, f in zip(got601, frames)) and not np.array_equal(got601[0], got[0])
    lane.release()

    main(common + ["--output_dir", str(tmp_path / "png")])
    lane = stream.FrameStylizer(eng, variables(eng), H, W, compose=compose, **kw)
    assert sorted(os.listdir(str(tmp_path / "png"))) == ["%06d.png" % k for k in range(3)]
    assert all(np.array_equal(g, lane(f)) for g, f in zip(pngs(tmp_path / "png"), frames))
    lane.release()

    main(common + ["--output_dir", str(tmp_path / "jpg"), "--output_format", "jpg", "--output_quality", "90"])
    lane = stream.FrameStylizer(eng, variables(eng), H, W, jpeg=dict(quality=90, subsampling=2), compose=compose, **kw)
    assert sorted(os.listdir(str(tmp_path / "jpg"))) == ["%06d.jpg" % k for k in range(3)]
    assert all(g == lane(f) for g, f in zip(files(tmp_path / "jpg"), frames))
    lane.release()


@pytest.mark.gpu
def test_full_strength_alone_reproduces_the_run_without_the_flag(tmp_path):
    frames = [samples_of(OPT, W, H, 40 + k) for k in range(2)]
    rng = np.random.default_rng(2)
    images = [rng.integers(0, 256, (H - 3, W - 2, 3), dtype=np.uint8) for _ in range(2)]     # (53 x 70: the output is larger)
    vid, pix = video(tmp_path, frames), frames_dir(tmp_path, images)
    for k, flags in enumerate((vid + ["--video_out", "{}.y4m"], vid + ["--output_dir", "{}"], pix + ["--output_dir", "{}"],
                               pix + ["--output_dir", "{}", "--output_format", "jpg"])):
        a, b = (str(tmp_path / ("%s%d" % (tag, k))) for tag in "ab")
        main([f.format(a) for f in flags])
        main([f.format(b) for f in flags] + ["--style_strength", "1"])
        if k == 0:
            assert open(a + ".y4m", "rb").read() == open(b + ".y4m", "rb").read()
        else:
            assert len(files(a)) == 2 and sorted(os.listdir(a)) == sorted(os.listdir(b)) and files(a) == files(b)


@pytest.mark.gpu
def test_the_source_shows_through_in_its_own_colours(tmp_path):
    """A red and a blue source frame under --preserve_color come out with the R - G and B - G of the source: every path of the script feeds
    the net B,G,R and shows its output as R,G,B, and the stage reads the source accordingly.  The two frames are the primary on a grey
    floor, (200, 56, 56) and (56, 56, 200), at strength 0.25: the luma delta then lies within [-25, 39] of 255 and no channel clamps, so the
    property holds at every pixel.  A .png holds the truncated 8.8 values, whose differences are exact (the source's are multiples of 256).
    A .jpg and 8-bit 4:2:0 planes round: two colour conversions of at most ~1.3 levels each and a chroma that is constant over the
    frame -- the frame means are held to 2 levels, 144 away from what exchanged channels would give."""
    red, blue = np.array([200, 56, 56], np.uint8), np.array([56, 56, 200], np.uint8)
    images = [np.broadcast_to(c, (H, W, 3)).copy() for c in (red, blue)]
    flags = ["--preserve_color", "--style_strength", "0.25"]

    def diffs(rgb):
        rgb = rgb.astype(np.int64)
        return rgb[..., 0] - rgb[..., 1], rgb[..., 2] - rgb[..., 1]

    # .png: exact at every pixel, and the luma did move
    main(frames_dir(tmp_path, images) + flags + ["--output_dir", str(tmp_path / "png")])
    for out, src in zip(pngs(tmp_path / "png"), images):
        assert out.shape == src.shape and out.min() > 0 and out.max() < 255
        for got, want in zip(diffs(out), diffs(src)):
            assert np.array_equal(got, want)
        assert len(np.unique(out[..., 1])) > 4
    # .jpg and .y4m: the frame means
    main(frames_dir(tmp_path, images, "in2") + flags + ["--output_dir", str(tmp_path / "jpg"), "--output_format", "jpg"])
    decoded = [np.asarray(Image.open(os.path.join(str(tmp_path / "jpg"), n)).convert("RGB")) for n in sorted(os.listdir(str(tmp_path / "jpg")))]
    planes = [rgb_to_frame(im, **ref_args(OPT)) for im in images]
    main(video(tmp_path, planes) + flags + ["--video_out", str(tmp_path / "g.y4m")])
    shown = [frame_to_rgb(p, W, H, **ref_args(OPT)) for p in read_stream(str(tmp_path / "g.y4m"))[2]]
    for outs in (decoded, shown):
        assert len(outs) == 2
        for out, src in zip(outs, images):
            for got, want in zip(diffs(out), diffs(src)):
                assert abs(got.mean() - want.mean()) <= 2.0, (got.mean(), want.mean())


@pytest.mark.gpu
def test_strength_zero_and_a_mask_give_the_source_back(tmp_path):
    rng = np.random.default_rng(4)
    images = [rng.integers(0, 256, (H - 3, W - 2, 3), dtype=np.uint8) for _ in range(2)]     # (53 x 70 -> 56 x 72)
    main(frames_dir(tmp_path, images) + ["--style_strength", "0", "--output_dir", str(tmp_path / "zero")])
    assert all(np.array_equal(g, replicated(im, H, W)) for g, im in zip(pngs(tmp_path / "zero"), images))
    mask = np.zeros((H - 3, W - 2), np.uint8)
    mask[:, 35:] = 255
    Image.fromarray(mask).save(str(tmp_path / "mask.png"))
    main(frames_dir(tmp_path, images, "in2") + ["--mask_path", str(tmp_path / "mask.png"), "--output_dir", str(tmp_path / "masked")])
    main(frames_dir(tmp_path, images, "in3") + ["--output_dir", str(tmp_path / "plain")])
    for g, p, im in zip(pngs(tmp_path / "masked"), pngs(tmp_path / "plain"), images):
        assert np.array_equal(g[:, :35], replicated(im, H, W)[:, :35]) and np.array_equal(g[:, 35:], p[:, 35:])


def test_bad_flags_exit_before_the_model_loads(tmp_path):
    # (no usable --model_path in any of these: a run that got as far as loading the model would fail otherwise)
    nomodel = ["--model_path", str(tmp_path / "none.ckpt")]
    write_stream(str(tmp_path / "f.y4m"), OPT, W, H, [samples_of(OPT, W, H, 1)])
    vid = nomodel + ["--video_in", str(tmp_path / "f.y4m"), "--video_out", str(tmp_path / "g.y4m")]
    d = tmp_path / "in"
    d.mkdir()
    Image.fromarray(np.zeros((H, W, 3), np.uint8)).save(str(d / "000.png"))
    pix = nomodel + ["--frames_dir", str(d), "--output_dir", str(tmp_path / "out")]
    Image.fromarray(np.zeros((H, W + 1), np.uint8)).save(str(tmp_path / "wide.png"))
    Image.fromarray(np.zeros((H, W), np.uint8)).save(str(tmp_path / "fits.png"))
    for run in (vid, pix):
        for s in ("1.5", "-0.25", "nan"):
            with pytest.raises(SystemExit) as e:
                main(run + ["--style_strength", s])
            assert "--style_strength" in str(e.value)
        with pytest.raises(SystemExit) as e:
            main(run + ["--mask_path", str(tmp_path / "wide.png")])
        assert "--mask_path" in str(e.value) and "%d by %d" % (W + 1, H) in str(e.value) and "%d by %d" % (W, H) in str(e.value)
        with pytest.raises(SystemExit) as e:                                                # the mask's size is the net's, after --frame_size
            main(run + ["--mask_path", str(tmp_path / "fits.png"), "--frame_size", "64", "48"])
        assert "--mask_path" in str(e.value) and "64 by 48" in str(e.value)
        with pytest.raises(SystemExit) as e:
            main(run + ["--mask_path", str(tmp_path / "missing.png")])
        assert "--mask_path" in str(e.value)
    assert not (tmp_path / "g.y4m").exists() and not (tmp_path / "out").exists()
    with pytest.raises(SystemExit):
        main(vid + ["--color_matrix", "bt2020"])


def test_parser_defaults_of_the_existing_flags_are_unchanged():
    import stylize_webcam
    args = vars(stylize_webcam.setup_parser().parse_args([]))
    new = dict(style_strength=None, preserve_color=False, color_matrix=None, mask_path=None)
    old = dict(model_path="./models/starry_final.ckpt", upsample_method="resize", resolution=None, frames_dir=None, output_dir="./frames_out",
               output_format="png", output_quality=95, frame_size=None, input_decode="pil", video_in=None, video_out=None, video_matrix="bt601",
               video_depth="8", video_out_depth=None)
    assert args == dict(old, **new)
    assert stylize_webcam.compose_options(stylize_webcam.setup_parser().parse_args([])) is None         # no flag: no stage
    for flags, want in ((["--preserve_color"], dict(strength=1.0, keep_color=True, matrix="bt601", source_swapped=True)),
                        (["--style_strength", "0.3"], dict(strength=0.3, keep_color=False, matrix="bt601", source_swapped=True)),
                        (["--color_matrix", "bt709"], dict(strength=1.0, keep_color=False, matrix="bt709", source_swapped=True))):
        assert stylize_webcam.compose_options(stylize_webcam.setup_parser().parse_args(flags)) == want
    assert stylize_webcam.compose_options(stylize_webcam.setup_parser().parse_args(["--preserve_color"]), "bt709")["matrix"] == "bt709"
