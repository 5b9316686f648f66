"""The two-stream forms of the split-bf16 VGG16 section (fs_vgg.hip: W6Chains, w6_half, w6_chain_launch_ok; fs_wino6.hip: the two-chunk pipeline of
wino6_launch) at the smallest shapes that engage them, against the same call on one stream (FS_WINO6_OVERLAP=0), BIT FOR BIT: a tile's value does not
depend on which launch or stream carries it, so any difference is a missing join or a wrong half offset.  The single-stream arithmetic itself is held to
float64 at 256 x 256, batch 4, by test_hip_train_step_256_b4_real_style_image_all_48_gradients_tight.

By themselves the chains run from 1024 tiles per half batch (conv4_x at batch 32).  A launch goes out as two halves when, besides the threshold
FS_WINO6_CHAIN_MINTILES, (a) EACH HALF is a launch the pipeline takes -- at least FS_WINO6_MINTILES = 256 tiles -- and (b) the pipeline's scratch holds
both halves padded to 128 tiles each: w6ws_floats >= 2 * wino6_ws_floats(N / 2, ...).  Hence the cases (conv4_x has H / 32 * W / 32 tiles per sample):
  n4_256x512   FS_WINO6_CHAIN_MINTILES=128 alone: 2 samples = 256 tiles per half, the smallest batch-4 shape that engages with only the threshold lowered
  n4_256x256   + FS_WINO6_MINTILES=128: 2 samples = 128 tiles per half (the per-GPU batch of the 8-GPU configuration)
  n2_256x512   + FS_WINO6_MINTILES=128: one sample per half
  n6_256x256   + FS_WINO6_MINTILES=128 FS_WINO6_MINCC=0: 3 samples = 192 tiles per half, padded to 256.  Two padded halves (512 tiles) do not fit the
               scratch of the 384-tile launch, so (b) fails while conv4_x alone sizes it; with FS_WINO6_MINCC=0 conv2_1 of the 12-image forward
               sizes it, and conv3_x / conv2_2 take the pipeline too: their input gradients join the chains, with joins at the pooling layers between
  n3_256x256   + FS_WINO6_MINTILES=128: odd batch, the chains must stay off
  n4_256x256_whole  FS_WINO6_CHAIN_MINTILES=128 alone: the halves (128 tiles) fall below FS_WINO6_MINTILES, W6Chains::launch sends the whole launch
               out on the caller's stream
fs_vgg_dgrad hands its launches no side stream and offers its input gradients no split-bf16 layout (fs_vgg.hip, vgg_dgrad): it runs on one stream
under every setting, which its debug lines must show; its result is compared all the same.

Measured on the MI355X: the chains engaged at n4_256x512, n4_256x256, n2_256x512 and n6_256x256 and stayed off at the other two; the two-chunk
pipeline ran in all 15 launches; every compared tensor was bit-identical on both runs of each call.  Wall time per test as it prints it (input
generation included): 0.45 s for the first (n4_256x512, with the engine's start), 0.02 .. 0.15 s for each of the others."""
import re
import time
from collections import Counter

import numpy as np
import pytest

from faststyle_amd import engine
from oracle import perceptual
from tests.backends import get_engine

pytestmark = pytest.mark.gpu

CV_WINO6 = 12        # ConvVariant of the split-bf16 pipeline (fs_kernels.h), as FS_CONV_DEBUG prints it
DGRAD_LAYERS = ("conv3_3", "conv4_3")
CONV_LINE = re.compile(r"^conv N(\d+) (\d+)x(\d+)x(\d+) -> \d+x\d+x(\d+) k3x3 s1 src\d+: variant (\d+) ", re.M)
WINO6_LINE = re.compile(r"^wino6 N(\d+) (\d+)x(\d+)x(\d+) -> \d+x\d+x(\d+): (\d+) tiles in (\d+) chunks over (one stream|two streams)$", re.M)

_weights = []


def vgg_weights():
    if not _weights:
        _weights.append(perceptual.synthetic_vgg_weights(3))
    return _weights[0]


@pytest.fixture
def vgg():
    """(engine, set_knob) with the pattern of test_path_parity.py's knob_hip; afterwards the engine again holds a buffer prepared under the default knobs
    (FS_WINO6_MINCC decides which layers' bf16 pieces fs_vgg_prepare builds)."""
    e = get_engine("hip")
    mp = pytest.MonkeyPatch()

    def set_knob(name, value):
        mp.setenv(name, str(value))
        e.lib.fs_debug_reload_env()
        e.reset_workspaces()
    yield e, set_knob
    mp.undo()
    e.lib.fs_debug_reload_env()
    e.reset_workspaces()
    e.vgg_load(vgg_weights())


_problems = {}


def problem(N, H, W):
    if (N, H, W) not in _problems:
        rng = np.random.default_rng(8)
        pb = dict(style=rng.uniform(0, 255, (1, 64, 64, 3)).astype(np.float32),
                  y=rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32), xc=rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32))
        for name, div, C in (("conv3_3", 4, 256), ("conv4_3", 8, 512)):
            shape = (N, H // div, W // div, C)
            pb[name] = (rng.standard_normal(shape, dtype=np.float32) / np.sqrt(np.prod(shape[1:]))).astype(np.float32)
        _problems[(N, H, W)] = pb
    return _problems[(N, H, W)]


def w6_convs(err):
    """{(N, H, W, Cin, Cout): launches} of the conv launches that took the split-bf16 pipeline, from FS_CONV_DEBUG's lines."""
    return Counter(tuple(int(v) for v in m.groups()[:5]) for m in CONV_LINE.finditer(err) if int(m.group(6)) == CV_WINO6)


def expected_w6(N, H, W, mincc0, loss):
    """The split-bf16 launches of one call on one stream, from VGG16's layer table.  loss: fs_perceptual_loss under the default loss configuration
    (2 N images up to conv3_3, the backward from conv4_3 down); else fs_vgg_dgrad (N images, forward only: see the module docstring).
    FS_WINO6_MINCC at its default keeps the pipeline to Cin * Cout >= 512 * 256, conv4_x; 0 adds every layer with Cin % 32 == 0 and Cout % 128 == 0."""
    c = Counter()
    nb = 2 * N if loss else N
    (h2, w2), (h4, w4), (h8, w8) = ((H // d, W // d) for d in (2, 4, 8))
    c[(N, h8, w8, 256, 512)] += 1                 # conv4_1
    c[(N, h8, w8, 512, 512)] += 2                 # conv4_2, conv4_3
    if mincc0:
        c[(nb, h2, w2, 64, 128)] += 1             # conv2_1
        c[(nb, h2, w2, 128, 128)] += 1            # conv2_2
        c[(nb, h4, w4, 128, 256)] += 1            # conv3_1
        c[(nb, h4, w4, 256, 256)] += 2            # conv3_2, conv3_3
    if loss:
        c[(N, h8, w8, 512, 512)] += 2             # input gradients of conv4_3, conv4_2
        c[(N, h8, w8, 512, 256)] += 1             # ... conv4_1
        if mincc0:
            c[(N, h4, w4, 256, 256)] += 2         # ... conv3_3, conv3_2
            c[(N, h4, w4, 256, 128)] += 1         # ... conv3_1
            c[(N, h2, w2, 128, 128)] += 1         # ... conv2_2 (conv2_1's has 64 output channels)
    return c


def halved(c, N):
    """The same launches with every batch-N one as two of N / 2 (the 2 N forward launches below the content layer never chain)."""
    out = Counter()
    for (n, h, w, ci, co), k in c.items():
        if n == N:
            out[(N // 2, h, w, ci, co)] += 2 * k
        else:
            out[(n, h, w, ci, co)] += k
    return out


def run_calls(e, pb, capfd):
    """fs_perceptual_loss twice, fs_vgg_dgrad twice (the second run of each finds the workspace as the first left it: a join missing at the end of a
    call shows as a difference) -> host copies of every result and the debug lines of the FIRST run of each call."""
    up = e.mem.from_numpy
    cfg = engine.default_loss_cfg()
    cfg["beta"] = 1e-4
    tg = e.style_targets(up(pb["style"]), cfg)
    y, xc = up(pb["y"]), up(pb["xc"])
    dfe = [up(pb[n]) for n in DGRAD_LAYERS]
    out = {}
    capfd.readouterr()
    for run in (1, 2):
        losses, dy = e.perceptual_loss(y, xc, tg, cfg)
        out["losses%d" % run], out["dy%d" % run] = e.mem.to_numpy(losses).copy(), e.mem.to_numpy(dy).copy()
        if run == 1:
            out["loss_lines"] = capfd.readouterr().err
    capfd.readouterr()
    for run in (1, 2):
        out["dx%d" % run] = e.mem.to_numpy(e.vgg_dgrad(y, list(DGRAD_LAYERS), dfe)).copy()
        if run == 1:
            out["dgrad_lines"] = capfd.readouterr().err
    capfd.readouterr()
    for k in ("losses1", "dy1", "dx1"):
        assert np.isfinite(out[k]).all()
    return out


def assert_same_bits(got, ref):
    for k in ("losses", "dy", "dx"):
        assert np.array_equal(ref[k + "2"], ref[k + "1"]), "single stream: second %s differs from the first" % k
        for run in ("1", "2"):
            assert np.array_equal(got[k + run], ref[k + "1"]), "%s of run %s differs from the single-stream result (%d elements, max %g)" % (
                k, run, np.count_nonzero(got[k + run] != ref[k + "1"]), np.abs(got[k + run] - ref[k + "1"]).max())


CHAIN_CASES = {
    # id: (N, H, W, knobs besides FS_WINO6_CHAIN_MINTILES=128, the chains engage)
    "n4_256x512": (4, 256, 512, {}, True),
    "n4_256x256": (4, 256, 256, {"FS_WINO6_MINTILES": 128}, True),
    "n2_256x512": (2, 256, 512, {"FS_WINO6_MINTILES": 128}, True),
    "n6_256x256": (6, 256, 256, {"FS_WINO6_MINTILES": 128, "FS_WINO6_MINCC": 0}, True),
    "n3_256x256": (3, 256, 256, {"FS_WINO6_MINTILES": 128}, False),
    "n4_256x256_whole": (4, 256, 256, {}, False),
}


@pytest.mark.parametrize("case", list(CHAIN_CASES))
def test_half_batch_chains_on_two_streams_change_no_bit(vgg, capfd, case):
    """FS_WINO6_OVERLAP=1 with the threshold lowered to 128 tiles against FS_WINO6_OVERLAP=0: losses[4], dL/dy and fs_vgg_dgrad's dL/dx bit for bit, on
    both runs of each call.  The debug lines prove what ran: on one stream every split-bf16 launch once with the full batch; with the chains the three
    conv4_x forward launches and every split-bf16 input-gradient launch of fs_perceptual_loss twice with half the batch (cases that must NOT engage:
    the single-stream lines again); fs_vgg_dgrad the single-stream lines under both settings."""
    e, knob = vgg
    N, H, W, extra, engages = CHAIN_CASES[case]
    t0 = time.perf_counter()
    pb = problem(N, H, W)
    knob("FS_CONV_DEBUG", 1)
    knob("FS_WINO6_CHAIN_MINTILES", 128)
    for k, v in extra.items():
        knob(k, v)
    e.vgg_load(vgg_weights())             # (prepared under the knobs of the case)
    mincc0 = extra.get("FS_WINO6_MINCC") == 0
    one_loss, one_dgrad = expected_w6(N, H, W, mincc0, True), expected_w6(N, H, W, mincc0, False)
    knob("FS_WINO6_OVERLAP", 0)
    ref = run_calls(e, pb, capfd)
    assert w6_convs(ref["loss_lines"]) == one_loss, ref["loss_lines"]
    assert w6_convs(ref["dgrad_lines"]) == one_dgrad, ref["dgrad_lines"]
    knob("FS_WINO6_OVERLAP", 1)
    got = run_calls(e, pb, capfd)
    assert w6_convs(got["loss_lines"]) == (halved(one_loss, N) if engages else one_loss), got["loss_lines"]
    assert w6_convs(got["dgrad_lines"]) == one_dgrad, got["dgrad_lines"]
    assert_same_bits(got, ref)
    print("two half-batch chains, %s: %s, bit-identical, %.2f s" % (case, "engaged" if engages else "not engaged (as it must)", time.perf_counter() - t0))


def test_chains_without_a_side_stream_fall_back_to_one_stream(vgg, capfd):
    """FS_NO_SIDE_STREAM=1 is read when a context is created: a context made under it has no second stream, and the same forced settings run every
    launch whole.  A fresh engine (its own context), the shared engine's single-stream result as the reference."""
    e, knob = vgg
    t0 = time.perf_counter()
    N, H, W = 4, 256, 256
    pb = problem(N, H, W)
    knob("FS_CONV_DEBUG", 1)
    knob("FS_WINO6_CHAIN_MINTILES", 128)
    knob("FS_WINO6_MINTILES", 128)
    e.vgg_load(vgg_weights())
    knob("FS_WINO6_OVERLAP", 0)
    ref = run_calls(e, pb, capfd)
    knob("FS_WINO6_OVERLAP", 1)
    knob("FS_NO_SIDE_STREAM", 1)
    e2 = engine.Engine()
    e2.vgg_load(vgg_weights())
    got = run_calls(e2, pb, capfd)
    assert w6_convs(got["loss_lines"]) == expected_w6(N, H, W, False, True), got["loss_lines"]
    assert_same_bits(got, ref)
    print("chains forced without a side stream: one stream, bit-identical, %.2f s" % (time.perf_counter() - t0))


def w6_launches(err):
    """[(N, H, W, Cin, Cout, tiles, chunks, two streams)] of wino6_launch's debug lines."""
    return [tuple(int(v) for v in m.groups()[:7]) + (m.group(8) == "two streams",) for m in WINO6_LINE.finditer(err)]


@pytest.mark.parametrize("form", ["pipelined", "pipe_off", "chunk128"])
def test_two_chunk_pipeline_of_a_launch_changes_no_bit(vgg, capfd, form):
    """FS_WINO6_OVERLAP=2 at N = 4, 256 x 256 with FS_WINO6_MINCC=0 FS_WINO6_MINTILES=1 (conv2_1 ... conv4_3 and seven input gradients take the
    pipeline, 256 ... 32768 tiles each): every launch of fs_perceptual_loss as two tile chunks software-pipelined over the two streams -- wino6_launch's
    debug line says so --, against the single-stream result bit for bit.  pipe_off: FS_WINO6_PIPE=0 on top, the launches must fall back to the chunk
    loop (one chunk: the scratch holds a launch).  chunk128: FS_WINO6_CHUNK=128 on top, two chunks do not fit any more: tiles / 128 chunks on one stream."""
    e, knob = vgg
    t0 = time.perf_counter()
    N, H, W = 4, 256, 256
    pb = problem(N, H, W)
    knob("FS_CONV_DEBUG", 1)
    knob("FS_WINO6_MINCC", 0)
    knob("FS_WINO6_MINTILES", 1)
    e.vgg_load(vgg_weights())
    one_loss, one_dgrad = expected_w6(N, H, W, True, True), expected_w6(N, H, W, True, False)
    knob("FS_WINO6_OVERLAP", 0)
    ref = run_calls(e, pb, capfd)
    assert w6_convs(ref["loss_lines"]) == one_loss, ref["loss_lines"]
    ref_launches = w6_launches(ref["loss_lines"])
    assert len(ref_launches) == 15 and all(chunks == 1 and not two for *_, chunks, two in ref_launches), ref["loss_lines"]
    knob("FS_WINO6_OVERLAP", 2)
    if form == "pipe_off":
        knob("FS_WINO6_PIPE", 0)
    elif form == "chunk128":
        knob("FS_WINO6_CHUNK", 128)
    got = run_calls(e, pb, capfd)
    assert w6_convs(got["loss_lines"]) == one_loss, got["loss_lines"]           # whole launches: the chunks are cut inside wino6_launch
    assert w6_convs(got["dgrad_lines"]) == one_dgrad, got["dgrad_lines"]
    launches = w6_launches(got["loss_lines"])
    assert Counter(l[:5] for l in launches) == one_loss, got["loss_lines"]
    for n, h, w, ci, co, tiles, chunks, two in launches:
        assert tiles == n * (h // 4) * (w // 4)
        want = {"pipelined": (2, True), "pipe_off": (1, False), "chunk128": (tiles // 128, False)}[form]
        assert (chunks, two) == want, got["loss_lines"]
    assert all(not two for *_, two in w6_launches(got["dgrad_lines"])), got["dgrad_lines"]      # (fs_vgg_dgrad has no side stream)
    assert_same_bits(got, ref)
    print("two chunks per launch, %s: 15 launches as told, bit-identical, %.2f s" % (form, time.perf_counter() - t0))
