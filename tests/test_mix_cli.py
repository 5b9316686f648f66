"""--model_path2 / --style_mix / --mix_mask / --mix_fade of stylize_webcam.py, run in-process with main(argv), file to file on small YUV4MPEG2
streams: weight 0 writes the bytes of the run without the flags and weight 1 those of the second model's run, a fade does so before and after
its frames, also in passes of two frames, a mask shows one model on either side, and bad flags exit before a checkpoint is opened.
tests/test_mix_stream.py holds the lanes against the restatement.  On the emulator the script's engine is the emulator's (one lane, eager)
and the frames are the smallest the net takes."""
import os

import numpy as np
import pytest
from PIL import Image

from tests.backends import engine_params, get_engine, on_emulator
from tests.test_video_deep import MODEL, ROOT, read_stream, samples_of, write_stream

OPT = dict(sampling=(2, 2), siting=0, matrix=1, full_range=True)                            # C420jpeg, full range, --video_matrix bt709
CANDY = os.path.join(ROOT, "models", "candy_final.ckpt")
MODEL2 = ["--model_path2", CANDY]
N = 5


@pytest.fixture(params=engine_params())
def eng(request, monkeypatch):
    """The engine the script will make: the GPU's own, or -- with faststyle_amd.engine.Engine patched -- the emulator's"""
    e = get_engine(request.param)
    if on_emulator(e):
        from faststyle_amd import engine
        monkeypatch.setattr(engine, "Engine", lambda: e)
    return e


def size(eng):
    """W, H of the streams: 44 x 42 on the emulator (the net's output is 44 x 44), 72 x 56 on the GPU"""
    return (44, 42) if on_emulator(eng) else (72, 56)


def main(argv):
    import stylize_webcam
    stylize_webcam.main(argv)


def run(tmp_path, eng, name, flags, model=MODEL):
    """One file-to-file run over the N-frame stream -> the frames written"""
    W, H = size(eng)
    src = str(tmp_path / "in.y4m")
    if not os.path.exists(src):
        write_stream(src, OPT, W, H, [samples_of(OPT, W, H, 60 + k) for k in range(N)])
    out = str(tmp_path / (name + ".y4m"))
    main(model + ["--video_in", src, "--video_matrix", "bt709", "--video_out", out] + flags)
    frames = read_stream(out)[2]
    assert len(frames) == N
    return [f.tobytes() for f in frames]


def test_weight_zero_and_one_write_the_one_model_runs(eng, tmp_path):
    starry, candy = run(tmp_path, eng, "a", []), run(tmp_path, eng, "b", [], ["--model_path", CANDY])
    assert all(a != b for a, b in zip(starry, candy)) and len(set(starry)) == N
    assert run(tmp_path, eng, "w0", MODEL2 + ["--style_mix", "0"]) == starry
    assert run(tmp_path, eng, "w1", MODEL2 + ["--style_mix", "1"]) == candy


@pytest.mark.parametrize("batch", [1, 2])
def test_a_fade_is_the_first_model_before_and_the_second_after(eng, tmp_path, batch):
    """--mix_fade 1 3 over five frames: weights 0, 0, 128, 256, 256 of 256.  Under --video_batch 2 the passes are (0, 1), (2, 3) and (4 and
    its repeat): the one-model runs are batched alike, so the net's batch numerics are the same on both sides."""
    more = ["--video_batch", "2"] if batch == 2 else []
    starry, candy = run(tmp_path, eng, "a", more), run(tmp_path, eng, "b", more, ["--model_path", CANDY])
    fade = run(tmp_path, eng, "f", more + MODEL2 + ["--mix_fade", "1", "3"])
    assert fade[:2] == starry[:2] and fade[3:] == candy[3:]
    assert fade[2] != starry[2] and fade[2] != candy[2]


def test_a_frames_directory_with_a_mask_shows_one_model_on_either_side(eng, tmp_path):
    W, H = size(eng)
    Ho, Wo = eng.tnet_out_shape(H, W)
    d = tmp_path / "in"
    d.mkdir()
    Image.fromarray(np.random.default_rng(4).integers(0, 256, (H, W, 3), dtype=np.uint8)).save(str(d / "000.png"))
    mask = np.zeros((H, W), np.uint8)
    mask[:, W // 2:] = 255
    Image.fromarray(mask).save(str(tmp_path / "mask.png"))
    pix = ["--frames_dir", str(d)]
    main(MODEL + pix + ["--output_dir", str(tmp_path / "a")])
    main(["--model_path", CANDY] + pix + ["--output_dir", str(tmp_path / "b")])
    main(MODEL + pix + MODEL2 + ["--mix_mask", str(tmp_path / "mask.png"), "--output_dir", str(tmp_path / "m")])
    a, b, m = (np.asarray(Image.open(str(tmp_path / k / "000.png"))) for k in "abm")
    assert m.shape == (Ho, Wo, 3) and not np.array_equal(a, b)
    assert np.array_equal(m[:, :W // 2], a[:, :W // 2]) and np.array_equal(m[:, W // 2:], b[:, W // 2:])


def test_bad_flags_exit_before_a_checkpoint_is_opened(tmp_path):
    # (no usable --model_path or --model_path2 in any of these: a run that got as far as loading a model would fail otherwise)
    W, H = 72, 56
    nomodel = ["--model_path", str(tmp_path / "none.ckpt")]
    second = ["--model_path2", str(tmp_path / "none2.ckpt")]
    write_stream(str(tmp_path / "f.y4m"), OPT, W, H, [samples_of(OPT, W, H, 1)])
    vid = nomodel + ["--video_in", str(tmp_path / "f.y4m"), "--video_out", str(tmp_path / "g.y4m")]
    d = tmp_path / "in"
    d.mkdir()
    Image.fromarray(np.zeros((H, W, 3), np.uint8)).save(str(d / "000.png"))
    pix = nomodel + ["--frames_dir", str(d), "--output_dir", str(tmp_path / "out")]
    Image.fromarray(np.zeros((H, W + 1), np.uint8)).save(str(tmp_path / "wide.png"))
    Image.fromarray(np.zeros((H, W), np.uint8)).save(str(tmp_path / "fits.png"))
    (tmp_path / "text.png").write_bytes(b"not a picture")

    def refused(argv, *words):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert all(w in str(e.value) for w in words), (argv, str(e.value))

    for base in (vid, pix, nomodel):                                                        # (nomodel alone: the camera loop)
        refused(base + second, "--model_path2", "--style_mix")                              # the second model without a way to mix
        for flags in (["--style_mix", "0.5"], ["--mix_mask", str(tmp_path / "fits.png")], ["--mix_fade", "1", "3"]):
            refused(base + flags, flags[0], "--model_path2")                                # ... and each way without the second model
        for t in ("1.5", "-0.25", "nan"):
            refused(base + second + ["--style_mix", t], "--style_mix")
        for f0, f1 in (("3", "3"), ("4", "2"), ("-1", "2")):
            refused(base + second + ["--mix_fade", f0, f1], "--mix_fade")
        refused(base + second + ["--mix_mask", str(tmp_path / "missing.png")], "--mix_mask")
        refused(base + second + ["--mix_mask", str(tmp_path / "text.png")], "--mix_mask")
    for base in (vid, pix):
        refused(base + second + ["--mix_mask", str(tmp_path / "wide.png")], "--mix_mask", "%d by %d" % (W + 1, H), "%d by %d" % (W, H))
        refused(base + second + ["--mix_mask", str(tmp_path / "fits.png"), "--frame_size", "64", "48"], "--mix_mask", "64 by 48")
    refused(nomodel + second + ["--mix_fade", "1", "3"], "--mix_fade", "camera")            # a fade needs frame numbers
    assert not (tmp_path / "g.y4m").exists() and not (tmp_path / "out").exists()


def test_the_flags_are_absent_unless_given_and_the_weights_are_integers():
    import stylize_webcam
    parser = stylize_webcam.setup_parser()
    args = vars(parser.parse_args([]))
    assert not {"model_path2", "style_mix", "mix_mask", "mix_fade"} & set(args)
    assert stylize_webcam.mix_options(parser.parse_args([])) is None                        # no flag: no stage
    got = parser.parse_args(MODEL2 + ["--mix_fade", "1", "3", "--style_mix", "0.3"])
    assert (got.model_path2, got.style_mix, got.mix_fade) == (CANDY, 0.3, [1, 3])
    mix = stylize_webcam.mix_options(got)
    assert mix == dict(model_path2=CANDY, weight=0.3, mask=None, fade=(1, 3))
    # q8_n = (2 T_q8 k + d) // (2 d) with T_q8 = 77: 0, 0, 38.5 rounded half up, 77, 77
    assert [stylize_webcam.fade_weight(mix, n) for n in range(5)] == [0, 0, 39, 77, 77]
    full = dict(mix, weight=1.0, fade=(10, 17))
    assert [stylize_webcam.fade_weight(full, n) for n in (0, 10, 11, 13, 16, 17, 400)] == [0, 0, 37, 110, 219, 256, 256]
    assert stylize_webcam.fade_weight(dict(mix, fade=None), 123) == 77
