"""Composite-call parity: fs_tnet_forward / fs_tnet_backward / fs_perceptual_loss /
fs_style_targets / fs_adam_tf_step against the numpy oracle (float64 oracle, float32 kernels).
Tolerances: forward pixels 1e-3 relative of the 0..255 range is the north-star budget -- we
hold 2e-5; gradients 2e-4 of each tensor's max magnitude."""
import os

import numpy as np
import pytest

from faststyle_amd import ckpt, engine
from oracle import perceptual, tnet
from tests.backends import engine_params, get_engine, on_emulator
from tests.imgutil import jpeg_roundtrip, load_rgb, psnr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=engine_params())
def eng(request):
    return get_engine(request.param)


@pytest.fixture
def knob(monkeypatch, eng):
    """Set an FS_* tuning knob for one test: the library caches the environment at first use, so it is told to re-read
    it now and again once monkeypatch has restored the environment."""
    def set_knob(name, value):
        monkeypatch.setenv(name, str(value))
        eng.lib.fs_debug_reload_env()
        eng.reset_workspaces()
    yield set_knob
    monkeypatch.undo()
    eng.lib.fs_debug_reload_env()
    eng.reset_workspaces()


@pytest.fixture
def knob_hip(monkeypatch):
    """The same for the product library only (GPU-only tests that are not parametrised over the engines)."""
    e = get_engine("hip")

    def set_knob(name, value):
        monkeypatch.setenv(name, str(value))
        e.lib.fs_debug_reload_env()
        e.reset_workspaces()
    yield set_knob
    monkeypatch.undo()
    e.lib.fs_debug_reload_env()
    e.reset_workspaces()


def f64(d):
    return {k: np.asarray(v, np.float64) for k, v in d.items()}


def starry():
    return ckpt.load_checkpoint(os.path.join(ROOT, "models", "starry_final.ckpt"))


def grads_close(e, g, want, tol, method="resize"):
    bad = []
    # some gradients are exactly 0 by symmetry (INshift1 feeds a VALID conv + instance norm):
    # their float32 value is summation noise, so errors are measured against a global floor
    floor = 5e-2 * max(np.abs(w).max() for w in want.values())
    for name, off, shape in e.param_table_for(method):
        n = int(np.prod(shape))
        a = g[off:off + n].reshape(shape)
        err = np.abs(a - want[name]).max() / max(np.abs(want[name]).max(), floor)
        if not err < tol:
            bad.append((name, err))
    return bad


def flat_close(got, want, tight=1e-4, l2=2e-3, cos_min=0.99999):
    """Tight max-abs agreement, or -- when a ReLU / max-pool kink flipped between float32 and
    float64 -- agreement of the whole gradient vector in direction and norm."""
    got = np.asarray(got, np.float64).ravel()
    want = np.asarray(want, np.float64).ravel()
    if np.abs(got - want).max() / np.abs(want).max() < tight:
        return True
    cos = np.dot(got, want) / (np.linalg.norm(got) * np.linalg.norm(want))
    return cos > cos_min and np.linalg.norm(got - want) / np.linalg.norm(want) < l2


def test_param_table_is_checkpoint_order(eng):
    names = [n for n, _, _ in eng.param_table()]
    assert ["img_t_net/" + n for n in names] == list(starry())
    assert eng.param_table()[2] == ("initconv_0/W", 32, (9, 9, 3, 16))       # byte offset 128 in .data
    assert eng.param_table()[-1][1] * 4 == 1680856
    flat = eng.flatten_params(starry())
    rt = eng.unflatten_params(flat)
    assert all(np.array_equal(rt[k], v) for k, v in starry().items())


def kink_free_params(seed=0, method="resize"):
    """Random-init parameters whose ReLU inputs stay positive (INscale~0.25, INshift~+6 on every ReLU'd unit):
    the loss is then smooth in float32 noise, so ALL 48 gradients can be held to a tight
    tolerance.  (With real masks a single pre-activation within ~1e-7 of zero flips its ReLU
    derivative between the float32 kernel and the float64 oracle and moves upstream gradient
    sums by ~1/sqrt(#pixels) -- a property of the kink, not of the kernels.)"""
    rng = np.random.default_rng(seed)
    P = tnet.init_params(seed=seed, upsample_method=method)
    for k in P:
        leaf = k.split("/")[1]
        if leaf.startswith("INscale"):
            P[k] = (0.25 + 0.05 * rng.standard_normal(P[k].shape)).astype(np.float32)
        elif leaf in ("INshift", "INshift1") and not k.startswith("upsample_2"):
            P[k] = (6.0 + 0.1 * rng.standard_normal(P[k].shape)).astype(np.float32)
        elif leaf.startswith("INshift"):
            P[k] = (0.1 * rng.standard_normal(P[k].shape)).astype(np.float32)
    return P


def run_fwd_bwd(eng, P_named, shape, seed, method="resize"):
    rng = np.random.default_rng(seed)
    flat = eng.mem.from_numpy(eng.flatten_params(P_named, scope="", upsample_method=method))
    x = rng.uniform(0, 255, shape + (3,)).astype(np.float32)
    xd = eng.mem.from_numpy(x)
    y = eng.mem.to_numpy(eng.tnet_forward(flat, xd, save_for_bwd=True, upsample_method=method))
    yo, cache = tnet.create_net(x.astype(np.float64), f64(P_named), upsample_method=method, keep=True)
    assert y.shape == yo.shape == (shape[0],) + eng.tnet_out_shape(shape[1], shape[2]) + (3,)
    dy = rng.standard_normal(y.shape).astype(np.float32)
    g = eng.mem.to_numpy(eng.tnet_backward(flat, xd, eng.mem.from_numpy(dy), upsample_method=method))
    assert np.isfinite(g).all()
    want = tnet.create_net_bwd(dy.astype(np.float64), f64(P_named), cache)
    return y, yo, g, want


def test_tnet_forward_with_two_level_statistics_merge(eng, knob):
    """Large images pre-reduce the per-tile instance-norm records (in_prereduce_kernel); force that path at a
    small size: T > 1 tiles -> 64 ranges -> finalize."""
    knob("FS_FINALIZE_MIN_T", 1)
    rng = np.random.default_rng(6)
    P = tnet.strip_scope(starry())
    flat = eng.mem.from_numpy(eng.flatten_params(P, scope=""))
    x = rng.uniform(0, 255, (2, 60, 72, 3)).astype(np.float32)
    y = eng.mem.to_numpy(eng.tnet_forward(flat, eng.mem.from_numpy(x)))
    yo = tnet.create_net(x.astype(np.float64), f64(P))
    assert np.abs(y - yo).max() / 255.0 < 2e-5


@pytest.mark.parametrize("shape,wgs", [((1, 45, 67), 0), ((2, 48, 56), 6), ((3, 52, 44), 10)])
def test_tnet_residual_convs_through_the_winograd_kernel(eng, shape, wgs, knob):
    """FS_TNET_WINO=2 forces what 720p / 1080p frames (and large training batches) select by themselves: the ten 3x3
    VALID residual convs through wino_conv_kernel -- producer instance norm + ReLU on load, per-block statistics --
    forward against the oracle with the shipped weights, and the backward pass on top of that forward.
    wgs > 0: a persistent grid of that many workgroups, chosen so that the launches end in a PARTIAL round -- the remainder
    split of fs_wino2.hip (leftover items split over their input-channel chunks across all workgroups, partial tiles summed
    by wino2_rem_epilogue_kernel: statistics records in the forward, the residual-gradient addend in the backward)."""
    knob("FS_TNET_WINO", 2)
    if wgs:
        knob("FS_WINO2_WGS", wgs)
    rng = np.random.default_rng(9)
    P = tnet.strip_scope(starry())
    flat = eng.mem.from_numpy(eng.flatten_params(P, scope=""))
    x = rng.uniform(0, 255, shape + (3,)).astype(np.float32)
    y = eng.mem.to_numpy(eng.tnet_forward(flat, eng.mem.from_numpy(x)))
    yo = tnet.create_net(x.astype(np.float64), f64(P))
    assert np.abs(y - yo).max() / 255.0 < 2e-5
    yk, yok, g, want = run_fwd_bwd(eng, kink_free_params(), shape, seed=0)
    assert np.abs(yk - yok).max() / 255.0 < 2e-5
    assert grads_close(eng, g, want, 2e-4) == []


@pytest.mark.parametrize("shape,wgs", [((1, 45, 67), 0), ((3, 52, 44), 3), ((2, 56, 44), -5)])   # (wgs < 0: the flattened form, grid of -wgs)
def test_tnet_residual_convs_through_the_16tile_f4x4_kernel(eng, shape, wgs, knob):
    """fs_wino4t.hip: what 720p frames and the training batches select by themselves (>= 64 items of 16x16 pixels) -- the ten
    residual convs and their ten input gradients through the 16-tile Winograd F(4x4,3x3) kernel (instance norm + ReLU on load,
    per-item statistics; 'full' padding + the residual gradient in the backward).  FS_TNET_WINO4=2 selects it at test sizes,
    FS_WINO4T_WGS=3 makes workgroups walk several items.  Same oracle, same tolerances as every other path (measured: 2.5e-6 .. 4.4e-6
    of the pixel range with the shipped weights -- 64-channel reductions keep F(4x4)'s larger transform constants harmless)."""
    knob("FS_TNET_WINO4", 2)
    if wgs < 0:      # round 5: items over the flattened per-sample tile lists (what a batch of 32 selects by itself: a round of the persistent grid less)
        knob("FS_WINO4T_FLAT", 2)
        wgs = -wgs
    if wgs:
        knob("FS_WINO4T_WGS", wgs)
    rng = np.random.default_rng(9)
    P = tnet.strip_scope(starry())
    flat = eng.mem.from_numpy(eng.flatten_params(P, scope=""))
    x = rng.uniform(0, 255, shape + (3,)).astype(np.float32)
    y = eng.mem.to_numpy(eng.tnet_forward(flat, eng.mem.from_numpy(x)))
    yo = tnet.create_net(x.astype(np.float64), f64(P))
    print("F(4x4) residual convs, shipped weights: max pixel error %.2e of the range" % (np.abs(y - yo).max() / 255.0))
    assert np.abs(y - yo).max() / 255.0 < 2e-5
    yk, yok, g, want = run_fwd_bwd(eng, kink_free_params(), shape, seed=0)
    print("   kink-free weights: %.2e" % (np.abs(yk - yok).max() / 255.0))
    assert np.abs(yk - yok).max() / 255.0 < 2e-5
    assert grads_close(eng, g, want, 2e-4) == []


@pytest.mark.parametrize("shape,block", [((1, 45, 67), 1), ((3, 52, 44), 2), ((2, 56, 72), -1)])   # (a fallback path since round 4: below 64 items of 16x16 pixels)
def test_tnet_residual_convs_through_the_half_item_winograd_kernel(eng, shape, block, knob):
    """fs_wino2h.hip: what a batch of 4 at 256x256 selects by itself (100..252 items on 256 CUs) -- the ten residual convs and
    their ten input gradients through the half-item Winograd kernel (<= 32 tiles x 64 channels, waves split by channel block
    x position-row pair, output-row shares exchanged through LDS).  FS_WINO2H_MIN_ITEMS=1 selects it at test sizes;
    FS_WINO2H_SHAPE pins a block shape (4x8, 5x6, 6x5 tiles; -1: the planner's pick among those and 8x4) so that ragged edge blocks, blocks
    with 30 of 32 tiles and several items per workgroup (FS_WINO2_WGS=3: the cross-item pipeline) are all visited.  Same
    oracle, same tolerances as every other path."""
    knob("FS_WINO2H_MIN_ITEMS", 1)
    knob("FS_WINO2_WGS", 3)
    if block >= 0:
        knob("FS_WINO2H_SHAPE", block)
    if block in (1, 2):      # ... and the (off-by-default) fused instance-norm finalize: the launch's last workgroup merges the records
        knob("FS_FUSED_FINALIZE", 1)
    rng = np.random.default_rng(9)
    P = tnet.strip_scope(starry())
    flat = eng.mem.from_numpy(eng.flatten_params(P, scope=""))
    x = rng.uniform(0, 255, shape + (3,)).astype(np.float32)
    y = eng.mem.to_numpy(eng.tnet_forward(flat, eng.mem.from_numpy(x)))
    yo = tnet.create_net(x.astype(np.float64), f64(P))
    assert np.abs(y - yo).max() / 255.0 < 2e-5
    yk, yok, g, want = run_fwd_bwd(eng, kink_free_params(), shape, seed=0)
    assert np.abs(yk - yok).max() / 255.0 < 2e-5
    assert grads_close(eng, g, want, 2e-4) == []


def test_frozen_params_forward_reuses_the_relaid_filters_and_rebuilds_them_for_other_params(eng, knob):
    """FS_FLAG_PARAMS_FROZEN (stylize_image.py / stylize_webcam.py: one checkpoint, many frames): the second call of a sequence
    skips the filter re-layouts inside the workspace -- same pixels, bit for bit --, a call with another parameter buffer
    rebuilds them (the promise is about ONE buffer's contents)."""
    knob("FS_TNET_WINO4", 2)         # the residual convs through a Winograd kernel: its transformed filters are part of what is kept
    rng = np.random.default_rng(5)
    P1, P2 = tnet.strip_scope(starry()), tnet.init_params(seed=3)
    f1, f2 = (eng.mem.from_numpy(eng.flatten_params(P, scope="")) for P in (P1, P2))
    x = eng.mem.from_numpy(rng.uniform(0, 255, (1, 45, 67, 3)).astype(np.float32))
    ref1, ref2 = (eng.mem.to_numpy(eng.tnet_forward(f, x)) for f in (f1, f2))
    a = eng.mem.to_numpy(eng.tnet_forward(f1, x, frozen=True))
    b = eng.mem.to_numpy(eng.tnet_forward(f1, x, frozen=True))     # re-layouts skipped
    c = eng.mem.to_numpy(eng.tnet_forward(f2, x, frozen=True))     # other buffer: rebuilt
    d = eng.mem.to_numpy(eng.tnet_forward(f2, x, frozen=True))
    assert np.array_equal(a, ref1) and np.array_equal(b, ref1)
    assert np.array_equal(c, ref2) and np.array_equal(d, ref2) and not np.array_equal(ref1, ref2)


@pytest.mark.parametrize("shape", [(2, 48, 56), (1, 41, 41), (1, 45, 67)])
def test_tnet_forward_matches_oracle_and_backward_tight_when_kink_free(eng, shape):
    """Smallest legal size (41: REFLECT needs pad < dim), odd sizes (asymmetric SAME padding of
    the stride-2 convs, 45 -> 125 -> 63 -> 32) and a batch of 2."""
    y, yo, g, want = run_fwd_bwd(eng, kink_free_params(), shape, seed=0)
    assert np.abs(y - yo).max() / 255.0 < 2e-5
    assert grads_close(eng, g, want, 2e-4) == []


@pytest.mark.parametrize("shape", [(2, 48, 56), (1, 45, 67)])
def test_tnet_narrow_layers_through_the_streaming_kernel(eng, shape, knob):
    """fs_cstream.hip takes the 16/32-channel stride-2 and resize-conv units and their input gradients once a launch has a few
    tiles per workgroup (training batches, 720p frames); FS_CSTREAM_MIN_TILES=1 sends these small shapes through it: odd
    extents (ragged tiles, clipped pixel-shuffle stores), instance-norm partials per tile, several tiles per workgroup
    (FS_CSTREAM_WGS=3 makes the persistent loop run).  Same oracle, same tolerances as the one-tile kernel."""
    knob("FS_CSTREAM_MIN_TILES", 1)
    knob("FS_CSTREAM_MASK", 31)     # + the 64 -> 64 3x3 instance (residual convs and both forms of their input gradient), off by default
    knob("FS_CSTREAM_WGS", 3)
    y, yo, g, want = run_fwd_bwd(eng, kink_free_params(), shape, seed=0)
    assert np.abs(y - yo).max() / 255.0 < 2e-5
    assert grads_close(eng, g, want, 2e-4) == []


@pytest.mark.parametrize("shape", [(2, 48, 56), (1, 45, 67)])
def test_tnet_sixteen_channel_layers_through_the_streaming_kernel(eng, knob, shape):
    """conv_s16_kernel (fs_s16.hip) takes the 9x9 image layer (REFLECT-40 fused), the kw-folded output layer and the input
    gradient of the output layer once a launch has 64 tiles of 16 x 16 pixels -- every training / inference shape; the small
    shapes of this suite only reach that in the image layer, so the threshold is lowered here: forward against the oracle,
    then all 48 gradients on top of that forward (odd sizes: partial edge tiles, mirrored borders inside a patch)."""
    knob("FS_S16_MIN_TILES", 1)
    y, yo, g, want = run_fwd_bwd(eng, kink_free_params(), shape, seed=5)
    assert np.abs(y - yo).max() / 255.0 < 2e-5
    assert grads_close(eng, g, want, 2e-4) == []
    P = tnet.strip_scope(starry())
    rng = np.random.default_rng(11)
    x = rng.uniform(0, 255, shape + (3,)).astype(np.float32)
    ys = eng.mem.to_numpy(eng.tnet_forward(eng.mem.from_numpy(eng.flatten_params(P, scope="")), eng.mem.from_numpy(x)))
    assert np.abs(ys - tnet.create_net(x.astype(np.float64), f64(P))).max() / 255.0 < 2e-5


@pytest.mark.parametrize("wgs,shape", [(2, (1, 48, 56)), (12, (1, 48, 48))])
def test_tnet_backward_filter_gradients_on_the_batch4_tiles(eng, knob, wgs, shape):
    """The filter gradients of the two 9x9 layers run wgrad2_kernel instances with STATIC tile geometry (operand reads by
    immediate offsets): 16 x 32 / 16 x 24-pixel tiles at batch 32 -- which the small shapes above happen to pick too -- and
    16 x 16 tiles at batch 4 per GPU.  The workgroup budget steers the planner to the 16 x 16 tiles at these sizes: 2 for the
    output layer (patch 21 wide), 12 for the image layer (patch 24 wide)."""
    knob("FS_WGRAD2_WGS", wgs)
    y, yo, g, want = run_fwd_bwd(eng, kink_free_params(), shape, seed=3)
    assert np.abs(y - yo).max() / 255.0 < 2e-5
    assert grads_close(eng, g, want, 2e-4) == []


@pytest.mark.parametrize("shape", [(2, 48, 56), (1, 45, 67)])
def test_tnet_deconv_method_forward_and_backward(eng, shape):
    """--upsample_method deconv (im_transf_net.py:57-63): conv2d_transpose 3x3 s2 x2 and 9x9 s1 with
    filters stored [k,k,Cout,Cin]; forward 2e-5 of the pixel range, all 48 gradients 2e-4."""
    y, yo, g, want = run_fwd_bwd(eng, kink_free_params(1, "deconv"), shape, seed=1, method="deconv")
    assert np.abs(y - yo).max() / 255.0 < 2e-5
    assert grads_close(eng, g, want, 2e-4, "deconv") == []
    # a resize-layout checkpoint must be refused, not silently reinterpreted
    with pytest.raises(Exception):
        eng.flatten_params(kink_free_params(1, "resize"), scope="", upsample_method="deconv")


def test_tnet_shipped_weights_forward_tight_backward_with_real_relu_masks(eng):
    y, yo, g, want = run_fwd_bwd(eng, tnet.strip_scope(starry()), (2, 48, 56), seed=0)
    assert np.abs(y - yo).max() / 255.0 < 2e-5
    wflat = np.concatenate([want[n].ravel() for n, _, _ in eng.param_table()])
    cos = np.dot(g, wflat) / (np.linalg.norm(g) * np.linalg.norm(wflat))
    assert cos > 0.99999
    assert np.linalg.norm(g - wflat) / np.linalg.norm(wflat) < 2e-3
    # SURVEY.md §8a invariant: dL/dINshift2 is the same vector for every residual block
    tab = {n: (o, s) for n, o, s in eng.param_table()}
    ref = g[tab["resblock_0/INshift2"][0]:][:64]
    for k in range(1, 5):
        np.testing.assert_allclose(g[tab["resblock_%d/INshift2" % k][0]:][:64], ref, rtol=2e-3, atol=2e-4 * np.abs(ref).max())


@pytest.mark.parametrize("mode,shape", [(0, (2, 13, 11, 16)), (1, (2, 13, 11, 16)), (2, (2, 13, 11, 16)),
                                        (1, (4, 37, 41, 16)),     # 24 chunks per sample, 4 lanes per sample in the final reduce
                                        (1, (3, 29, 23, 8)),      # batch size that does not divide 16: per-sample final + dparams
                                        (2, (2, 19, 17, 3))])     # C % 4 != 0: the scalar kernels (the 3-channel output layer)
def test_instnorm_backward_modes(eng, mode, shape):
    """IN backward with the three activations; pre-activations are nudged away from the ReLU kink."""
    from oracle import nnops
    rng = np.random.default_rng(3)
    N, H, W, C = shape
    z = rng.standard_normal((N, H, W, C)).astype(np.float32) * 2 + 0.5
    gamma = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(C)).astype(np.float32)
    n64, cache = nnops.inst_norm(z.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64))
    near = np.abs(n64) < 1e-3
    z[near] += 0.05
    n64, cache = nnops.inst_norm(z.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64))
    xhat, rstd, _ = cache
    mean = z.astype(np.float64).mean(axis=(1, 2))
    a = gamma * rstd[:, 0, 0, :]
    b = beta - mean * a
    gin = rng.standard_normal(z.shape).astype(np.float32)
    if mode == 1:
        dn = gin * (n64 > 0)
    elif mode == 2:
        dn = nnops.scaled_tanh_bwd(gin.astype(np.float64), n64)
    else:
        dn = gin.astype(np.float64)
    dz_o, dg_o, db_o = nnops.inst_norm_bwd(dn, cache)
    up = eng.mem.from_numpy
    dz, dg, db = eng.instnorm_bwd(up(gin), up(z), up(mean), up(rstd[:, 0, 0, :]), up(a), up(b), mode)
    for got, wnt in ((dz, dz_o), (dg, dg_o), (db, db_o)):
        assert np.abs(eng.mem.to_numpy(got) - wnt).max() / np.abs(wnt).max() < 5e-5


@pytest.mark.parametrize("force_ksplit", [0, 3, "big_items"])
def test_perceptual_loss_and_gradient_match_oracle(eng, knob, force_ksplit):
    """force_ksplit=3 drives every eligible VGG conv (forward and dgrad) through the split-K kernel path +
    splitk_epilogue_kernel (bias/ReLU, tap add + ReLU mask), which otherwise only triggers at 256x256.
    "big_items": the item forms the batch-32 step takes by itself -- FS_WINO4T_TB=2 selects 32-tile items for the 64-channel
    layers and the 128-channel form (two channel blocks per wave, filter layout of wt_wino4u) for every layer that has them."""
    if force_ksplit == "big_items":
        knob("FS_WINO4T_TB", 2)
    elif force_ksplit:
        knob("FS_CONV_FORCE_KSPLIT", force_ksplit)
    rng = np.random.default_rng(1)
    Wv = perceptual.synthetic_vgg_weights(seed=3)
    eng.vgg_load(Wv)
    cfg = engine.default_loss_cfg()
    cfg["beta"] = 1e-4
    style = rng.uniform(0, 255, (1, 37, 45, 3)).astype(np.float32)      # odd sizes: SAME max-pool padding
    tg = eng.style_targets(eng.mem.from_numpy(style), cfg)
    tgo = perceptual.target_grams(style.astype(np.float64), f64(Wv), cfg["style_layers"])
    for a, b in zip(tg, tgo):
        assert np.abs(eng.mem.to_numpy(a) - b).max() / np.abs(b).max() < 2e-5
    y = rng.uniform(0, 255, (2, 32, 40, 3)).astype(np.float32)
    xc = rng.uniform(0, 255, (2, 32, 40, 3)).astype(np.float32)
    losses, dy = eng.perceptual_loss(eng.mem.from_numpy(y), eng.mem.from_numpy(xc), tg, cfg)
    feats = perceptual.vgg16(xc.astype(np.float64), f64(Wv), upto="conv3_3")
    lo, dyo = perceptual.perceptual_loss(y.astype(np.float64), [feats["conv3_3"]], tgo, f64(Wv), beta=1e-4)
    got = eng.mem.to_numpy(losses)
    want = [lo[k] for k in ("loss", "content_loss", "style_loss", "tv_loss")]
    np.testing.assert_allclose(got, want, rtol=2e-5)
    assert flat_close(eng.mem.to_numpy(dy), dyo)


@pytest.mark.parametrize("chunk", [0, 128])
def test_perceptual_loss_through_the_split_bf16_pipeline(eng, knob, chunk):
    """FS_WINO_V=6 (round 6, fs_wino6.hip): the VGG16 convs with Cin % 32 == 0 and Cout % 128 == 0 and their input gradients as input transform + 36 GEMMs on the
    bf16 matrix cores (six exact products of bf16 pieces, fp32 accumulation) + output transform with the bias / ReLU / pool / consumer-mask epilogues
    (libs/vgg16.py:83-173 behind train.py:203).  The thresholds that keep the path to conv4_x at training sizes are lowered so that every eligible layer of
    this small problem takes it (conv2_1 ... conv4_3 forward, conv4_3 ... conv2_2 input gradients); chunk = 128: the launches run in tile chunks.
    Unchanged tolerances: losses 2e-5, the gradient as in test_perceptual_loss_and_gradient_match_oracle."""
    knob("FS_WINO_V", 6)
    knob("FS_WINO6_MINCC", 0)
    knob("FS_WINO6_MINTILES", 1)
    if chunk:
        knob("FS_WINO6_CHUNK", chunk)
    rng = np.random.default_rng(1)
    Wv = perceptual.synthetic_vgg_weights(seed=3)
    eng.vgg_load(Wv)                     # (prepared under the knob: the buffer carries the bf16 pieces)
    cfg = engine.default_loss_cfg()
    cfg["beta"] = 1e-4
    style = rng.uniform(0, 255, (1, 37, 45, 3)).astype(np.float32)
    tg = eng.style_targets(eng.mem.from_numpy(style), cfg)
    tgo = perceptual.target_grams(style.astype(np.float64), f64(Wv), cfg["style_layers"])
    y = rng.uniform(0, 255, (2, 32, 40, 3)).astype(np.float32)
    xc = rng.uniform(0, 255, (2, 32, 40, 3)).astype(np.float32)
    losses, dy = eng.perceptual_loss(eng.mem.from_numpy(y), eng.mem.from_numpy(xc), tg, cfg)
    losses, dy = eng.mem.to_numpy(losses).copy(), eng.mem.to_numpy(dy).copy()
    feats = perceptual.vgg16(xc.astype(np.float64), f64(Wv), upto="conv3_3")
    lo, dyo = perceptual.perceptual_loss(y.astype(np.float64), [feats["conv3_3"]], tgo, f64(Wv), beta=1e-4)
    np.testing.assert_allclose(losses, [lo[k] for k in ("loss", "content_loss", "style_loss", "tv_loss")], rtol=2e-5)
    assert flat_close(dy, dyo)
    knob("FS_WINO_V", 5)                 # the same buffer under the default knob: the fp32 F(4x4) kernels -- another algorithm, the same answer
    l5, dy5 = eng.perceptual_loss(eng.mem.from_numpy(y), eng.mem.from_numpy(xc), tg, cfg)
    l5, dy5 = eng.mem.to_numpy(l5), eng.mem.to_numpy(dy5)
    assert not np.array_equal(dy5, dy)
    np.testing.assert_allclose(l5, losses, rtol=2e-5)
    eng.vgg_load(Wv)                     # (leave the engine with a buffer prepared under the default knobs)


@pytest.mark.parametrize("content_layers", [("conv1_2", "conv3_3"), ("conv2_2", "conv3_3", "conv4_3")])
def test_perceptual_loss_with_several_content_layers(eng, knob, content_layers):
    """train.py:56-60: --loss_content_layers takes several names.  A content term BELOW the last content layer reads the content half of a pooled
    layer's full-resolution activation -- the store the pooling epilogue of the big-item kernel skips for the content half when nothing reads it
    (ConvArgs::y_keep_n; round-5 advisor finding: the skip looked at the LAST content layer only).  FS_WINO4T_TB=2 selects the item forms that skip."""
    knob("FS_WINO4T_TB", 2)
    rng = np.random.default_rng(11)
    Wv = perceptual.synthetic_vgg_weights(seed=3)
    eng.vgg_load(Wv)
    cfg = engine.default_loss_cfg()
    cfg["content_layers"] = list(content_layers)
    cfg["content_weights"] = [0.7, 1.3, 0.4][:len(content_layers)]
    style = rng.uniform(0, 255, (1, 40, 36, 3)).astype(np.float32)
    tg = eng.style_targets(eng.mem.from_numpy(style), cfg)
    tgo = perceptual.target_grams(style.astype(np.float64), f64(Wv), cfg["style_layers"])
    shape = (2, 32, 32, 3) if on_emulator(eng) else (2, 32, 64, 3)       # (one 32-tile item column on the emulator: same item forms, half the time)
    y = rng.uniform(0, 255, shape).astype(np.float32)
    xc = rng.uniform(0, 255, shape).astype(np.float32)
    # poison the workspace first: a skipped store would otherwise find the previous call's (correct) values
    eng.perceptual_loss(eng.mem.from_numpy(xc[::-1].copy()), eng.mem.from_numpy(y), tg, cfg)
    losses, dy = eng.perceptual_loss(eng.mem.from_numpy(y), eng.mem.from_numpy(xc), tg, cfg)
    losses, dy = eng.mem.to_numpy(losses).copy(), eng.mem.to_numpy(dy).copy()
    feats = perceptual.vgg16(xc.astype(np.float64), f64(Wv), upto=max(content_layers))
    lo, dyo = perceptual.perceptual_loss(y.astype(np.float64), [feats[n] for n in content_layers], tgo, f64(Wv), content_layers=tuple(content_layers),
                                         content_weights=tuple(cfg["content_weights"]))
    np.testing.assert_allclose(losses[:3], [lo[k] for k in ("loss", "content_loss", "style_loss")], rtol=2e-5)
    # (this seed has ReLU / pooling ties that flip between float32 and float64 -- the default configuration measures the same 3.5e-3 here --
    # so the gradient is held to direction + norm against the oracle and BIT FOR BIT against the path that stores everything)
    assert flat_close(dy, dyo, l2=1e-2, cos_min=0.9999)
    knob("FS_VGG_SKIP_CONTENT_Y", 0)
    l0, dy0 = eng.perceptual_loss(eng.mem.from_numpy(y), eng.mem.from_numpy(xc), tg, cfg)
    assert np.array_equal(eng.mem.to_numpy(l0), losses) and np.array_equal(eng.mem.to_numpy(dy0), dy)


@pytest.mark.parametrize("hw", [(35, 45)])   # (odd sizes: partial pooling windows; an even case ran here too until the suite grew past 11 minutes)
def test_pool_gradient_routing_fused_into_the_gram_gradient_conv(eng, knob, hw):
    """The backward of max-pool + ReLU behind conv1_2 / conv2_2 (first-maximum routing, SAME padding for odd extents) runs
    in the epilogue of the Gram-gradient conv (ConvArgs::route_src) with FS_VGG_ROUTE_FUSED=1; by default the separate
    vgg_bwd_route pass does it.  Same arithmetic in the same order: the two must agree bit for bit, and with the oracle."""
    rng = np.random.default_rng(5)
    Wv = perceptual.synthetic_vgg_weights(seed=3)
    eng.vgg_load(Wv)
    cfg = engine.default_loss_cfg()
    style = rng.uniform(0, 255, (1, 40, 36, 3)).astype(np.float32)
    tg = eng.style_targets(eng.mem.from_numpy(style), cfg)
    y = rng.uniform(0, 255, (2,) + hw + (3,)).astype(np.float32)
    xc = rng.uniform(0, 255, (2,) + hw + (3,)).astype(np.float32)
    knob("FS_VGG_ROUTE_FUSED", 1)
    l1, dy1 = eng.perceptual_loss(eng.mem.from_numpy(y), eng.mem.from_numpy(xc), tg, cfg)
    l1, dy1 = eng.mem.to_numpy(l1).copy(), eng.mem.to_numpy(dy1).copy()
    knob("FS_VGG_ROUTE_FUSED", 0)
    l0, dy0 = eng.perceptual_loss(eng.mem.from_numpy(y), eng.mem.from_numpy(xc), tg, cfg)
    l0, dy0 = eng.mem.to_numpy(l0), eng.mem.to_numpy(dy0)
    assert np.array_equal(l0, l1) and np.array_equal(dy0, dy1)
    tgo = perceptual.target_grams(style.astype(np.float64), f64(Wv), cfg["style_layers"])
    feats = perceptual.vgg16(xc.astype(np.float64), f64(Wv), upto="conv3_3")
    _, dyo = perceptual.perceptual_loss(y.astype(np.float64), [feats["conv3_3"]], tgo, f64(Wv), beta=0.0)
    assert flat_close(dy1, dyo)


def test_pool_gradient_routing_in_the_streaming_gram_gradient_kernel(eng, knob):
    """Round 5: where the three pooled style layers tile into row pairs (every 256-wide input: relu1_2 8 x 256, relu2_2 4 x 128, relu3_3 2 x 64 here;
    relu3_3 also carries the content term) the streaming Gram-gradient kernel itself routes the max-pool gradient, applies the ReLU mask
    (gram_bwd_kernel<.., RT>) and forms the content-loss gradient and partial sums from its own operand; vgg_bwd_route and the sqdiff pass do not run.
    Against the three-launch result (FS_GRAM_ROUTE_FUSED=0) and the oracle."""
    rng = np.random.default_rng(6)
    Wv = perceptual.synthetic_vgg_weights(seed=3)
    eng.vgg_load(Wv)
    cfg = engine.default_loss_cfg()
    style = rng.uniform(0, 255, (1, 40, 36, 3)).astype(np.float32)
    tg = eng.style_targets(eng.mem.from_numpy(style), cfg)
    y = rng.uniform(0, 255, (1, 8, 256, 3)).astype(np.float32)
    xc = rng.uniform(0, 255, (1, 8, 256, 3)).astype(np.float32)
    l1, dy1 = eng.perceptual_loss(eng.mem.from_numpy(y), eng.mem.from_numpy(xc), tg, cfg)
    l1, dy1 = eng.mem.to_numpy(l1).copy(), eng.mem.to_numpy(dy1).copy()
    knob("FS_GRAM_ROUTE_FUSED", 0)
    l0, dy0 = eng.perceptual_loss(eng.mem.from_numpy(y), eng.mem.from_numpy(xc), tg, cfg)
    l0, dy0 = eng.mem.to_numpy(l0).copy(), eng.mem.to_numpy(dy0).copy()
    # the gradient bit for bit; the content loss is summed per workgroup of the Gram-gradient launch instead of per block of the sqdiff pass
    assert np.array_equal(dy0, dy1) and np.array_equal(l0[2:], l1[2:]) and abs(l0[1] - l1[1]) <= 2e-6 * abs(l0[1])
    knob("FS_GRAM_ROUTE_FUSED", 1)
    knob("FS_GRAM_CONTENT_FUSED", 0)      # routing in the kernel, content term from the sqdiff pass: every loss bit for bit too
    l2, dy2 = eng.perceptual_loss(eng.mem.from_numpy(y), eng.mem.from_numpy(xc), tg, cfg)
    assert np.array_equal(eng.mem.to_numpy(l2), l0) and np.array_equal(eng.mem.to_numpy(dy2), dy0)
    tgo = perceptual.target_grams(style.astype(np.float64), f64(Wv), cfg["style_layers"])
    feats = perceptual.vgg16(xc.astype(np.float64), f64(Wv), upto="conv3_3")
    lo, dyo = perceptual.perceptual_loss(y.astype(np.float64), [feats["conv3_3"]], tgo, f64(Wv), beta=0.0)
    np.testing.assert_allclose(l1[:3], [lo[k] for k in ("loss", "content_loss", "style_loss")], rtol=2e-5)
    assert flat_close(dy1, dyo)


@pytest.mark.parametrize("layers,prepared", [(("conv1_2", "conv2_2", "conv3_3", "conv4_3"), True), (("conv2_1", "conv3_2"), True), (("conv3_3",), False)])
def test_vgg_dgrad_named_export_matches_oracle(eng, layers, prepared):
    """fs_vgg_dgrad (round 6): upstream gradients of ANY subset of VGG16 layers -> dL/d(images) (libs/vgg16.py:36-173 behind tf.gradients, train.py:203): the
    adjoint of fs_vgg_features as a named entry point -- pooled and unpooled tap layers, the last layer tapped or not, with the prepared Winograd filters and
    with the direct kernels.  Oracle: perceptual.vgg16_bwd in float64 with random upstream gradients."""
    rng = np.random.default_rng(4)      # (seed 3 has a ReLU / pooling tie that flips between float32 and float64: 2e-3 instead of 4e-6)
    Wv = perceptual.synthetic_vgg_weights(seed=3)
    eng.vgg_load(Wv)
    x = rng.uniform(0, 255, (2, 24, 40, 3)).astype(np.float32)
    upto = max(layers)
    feats, cache = perceptual.vgg16(x.astype(np.float64), f64(Wv), upto=upto, keep=True)
    dfe = {n: (rng.standard_normal(feats[n].shape) / np.sqrt(feats[n][0].size)).astype(np.float32) for n in layers}
    got_feats = eng.vgg_features(eng.mem.from_numpy(x), list(layers))
    for n, t in zip(layers, got_feats):
        assert np.abs(eng.mem.to_numpy(t) - feats[n]).max() < 2e-5 * np.abs(feats[n]).max()
    dx = eng.mem.to_numpy(eng.vgg_dgrad(eng.mem.from_numpy(x), list(layers), [eng.mem.from_numpy(dfe[n]) for n in layers], use_prepared=prepared))
    want = perceptual.vgg16_bwd({n: dfe[n].astype(np.float64) for n in layers}, feats, f64(Wv), cache, upto=upto)
    assert dx.shape == want.shape == x.shape
    assert flat_close(dx, want)


# ----------------------------------------------------------------------------- which kernels a VGG16 launch is handed, per Winograd generation
# The prepared buffer is built under `prepare`, the calls run under `run` (a buffer prepared under other knobs must fall to the direct kernels).
SELECTION_SETTINGS = {
    "v1": ({"FS_WINO_V": 1}, {}),
    "v2": ({"FS_WINO_V": 2}, {}),
    "v4": ({"FS_WINO_V": 4}, {}),
    "v5": ({"FS_WINO_V": 5}, {}),
    "v6": ({"FS_WINO_V": 6, "FS_WINO6_MINCC": 0, "FS_WINO6_MINTILES": 1}, {}),
    "wino_off": ({"FS_CONV_WINO": 0}, {}),
    "prepared_v6_run_v4": ({"FS_WINO_V": 6, "FS_WINO6_MINCC": 0, "FS_WINO6_MINTILES": 1}, {"FS_WINO_V": 4}),
}
SELECTION_DGRAD_LAYERS = ("conv1_2", "conv2_2", "conv3_3", "conv4_3")
# profiler rows (fs_profile_family_name) the tables below speak of
I22, I21, I41, I12, I11 = ("conv_igemm_kernel<%s>" % t for t in ("32,2,2", "32,2,1", "16,4,1", "32,1,2", "32,1,1"))
WINO, WINO2, WINO4, WINO4T = "wino_conv_kernel", "wino2_conv_kernel (VGG16 convs)", "wino4_conv_kernel", "wino4t_conv_kernel (VGG16 convs)"
WINO6 = "wino6 pipeline (VGG16 convs: input transform + split-bf16 GEMMs + output transform)"
C3, GSTREAM, GWGRAD, GBWD, GBWD_I = ("conv3x3_to3_kernel", "gram_stream_kernel", "conv_wgrad_kernel (Gram forward)", "gram_bwd_kernel",
                                     "conv_igemm_kernel (Gram backward, 1x1 per-sample filters)")
# Launch counts per profiler row of one fs_perceptual_loss call and one fs_vgg_dgrad call, RECORDED ON THE PARENT COMMIT of the change that gave the VGG16
# launches one args builder (this test uses existing exports only and ran there unchanged; the tables were pasted from its printed output -- never taken
# from the code under test).  Recorded with the parent's sources on the emulator at 1 x 20 x 28 AND at 2 x 36 x 44: the same counts at both shapes.  Which
# kernel a launch takes is decided by host code that asks the device nothing, so the product library on the GPU plans the same launches at 2 x 36 x 44:
# the "hip" entries are those tables.
SELECTION_LAUNCHES = {
    ("emu", "v1"): {"perceptual_loss": {I22: 1, WINO: 18, C3: 1, GSTREAM: 4, GBWD: 3, GBWD_I: 1},
        "vgg_dgrad": {I22: 1, WINO: 18, C3: 1}},
    ("emu", "v2"): {"perceptual_loss": {I22: 1, WINO: 11, WINO2: 7, C3: 1, GSTREAM: 4, GBWD: 3, GBWD_I: 1},
        "vgg_dgrad": {I22: 1, WINO: 11, WINO2: 7, C3: 1}},
    ("emu", "v4"): {"perceptual_loss": {I22: 1, C3: 1, GSTREAM: 4, GBWD: 3, GBWD_I: 1, WINO4: 18},
        "vgg_dgrad": {I22: 1, C3: 1, WINO4: 18}},
    ("emu", "v5"): {"perceptual_loss": {I22: 1, C3: 1, GSTREAM: 4, GBWD: 3, GBWD_I: 1, WINO4T: 18},
        "vgg_dgrad": {I22: 1, C3: 1, WINO4T: 18}},
    ("emu", "v6"): {"perceptual_loss": {I22: 1, C3: 1, GSTREAM: 4, GBWD: 3, GBWD_I: 1, WINO4T: 3, WINO6: 15},
        "vgg_dgrad": {I22: 1, C3: 1, WINO4T: 10, WINO6: 8}},
    ("emu", "wino_off"): {"perceptual_loss": {I22: 1, I11: 18, C3: 1, GSTREAM: 4, GBWD: 3, GBWD_I: 1},
        "vgg_dgrad": {I22: 1, I11: 18, C3: 1}},
    ("emu", "prepared_v6_run_v4"): {"perceptual_loss": {I22: 1, I11: 18, C3: 1, GSTREAM: 4, GBWD: 3, GBWD_I: 1},
        "vgg_dgrad": {I22: 1, I11: 18, C3: 1}},
}
SELECTION_LAUNCHES.update({("hip", setting): table for (_, setting), table in list(SELECTION_LAUNCHES.items())})


def profiled_launches(eng, call):
    """call() under fs_profile_begin / fs_profile_end -> (its result, {row name: launches} of the rows that saw a launch)."""
    import ctypes
    from faststyle_amd import _lib
    assert eng.lib.fs_profile_begin(eng.ctx) == 0
    try:
        out = call()
    finally:
        buf = (ctypes.c_double * (3 * _lib.FS_PROFILE_FAMILIES))()
        rc = eng.lib.fs_profile_end(eng.ctx, ctypes.byref(buf))
    assert rc == 0
    names = _lib.profile_family_names(eng.lib)
    return out, {names[f]: int(buf[3 * f]) for f in range(_lib.FS_PROFILE_FAMILIES) if buf[3 * f]}


_selection_problem = {}


def selection_problem(shape):
    """Inputs and the float64 oracle of the selection test, computed once per shape and shared (read-only) by every setting."""
    if shape not in _selection_problem:
        rng = np.random.default_rng(1)
        Wv = perceptual.synthetic_vgg_weights(seed=3)
        style = rng.uniform(0, 255, (1, 23, 27, 3)).astype(np.float32)
        y = rng.uniform(0, 255, shape + (3,)).astype(np.float32)
        xc = rng.uniform(0, 255, shape + (3,)).astype(np.float32)
        tgo = perceptual.target_grams(style.astype(np.float64), f64(Wv), engine.default_loss_cfg()["style_layers"])
        feats = perceptual.vgg16(xc.astype(np.float64), f64(Wv), upto="conv3_3")
        lo, dyo = perceptual.perceptual_loss(y.astype(np.float64), [feats["conv3_3"]], tgo, f64(Wv), beta=1e-4)
        upto = max(SELECTION_DGRAD_LAYERS)
        fy, cache = perceptual.vgg16(y.astype(np.float64), f64(Wv), upto=upto, keep=True)
        dfe = {n: (rng.standard_normal(fy[n].shape) / np.sqrt(fy[n][0].size)).astype(np.float32) for n in SELECTION_DGRAD_LAYERS}
        dxo = perceptual.vgg16_bwd({n: dfe[n].astype(np.float64) for n in SELECTION_DGRAD_LAYERS}, fy, f64(Wv), cache, upto=upto)
        _selection_problem[shape] = dict(Wv=Wv, style=style, y=y, xc=xc, dfe=dfe, dxo=dxo, dyo=dyo,
                                         losses=[lo[k] for k in ("loss", "content_loss", "style_loss", "tv_loss")])
    return _selection_problem[shape]


@pytest.mark.parametrize("setting", list(SELECTION_SETTINGS))
def test_vgg_filter_selection_per_generation(eng, knob, setting):
    """Which prepared filter layouts fs_perceptual_loss and fs_vgg_dgrad hand their 3x3 launches: FS_WINO_V 1, 2, 4, 5, 6 with the buffer prepared under the
    same knob, FS_CONV_WINO=0, and a buffer prepared under FS_WINO_V=6 that runs under FS_WINO_V=4 (no layout both the buffer and the knobs agree on: the
    direct kernels).  2 x 36 x 44 (emulator: 1 x 20 x 28): the maps behind conv1_2 and conv2_2 have even extents -- the pool comes from the Winograd
    epilogue --, the one behind conv3_3 is odd -- the separate maxpool --, every tile grid is ragged.  Per setting: the launches per profiler row equal the
    table recorded on the parent commit, the losses are within 2e-5 of the float64 oracle and both gradients flat_close to it (the assertions of
    test_perceptual_loss_and_gradient_match_oracle)."""
    prepare, run = SELECTION_SETTINGS[setting]
    backend = "emu" if on_emulator(eng) else "hip"
    pb = selection_problem((1, 20, 28) if backend == "emu" else (2, 36, 44))
    for k, v in prepare.items():
        knob(k, v)
    eng.vgg_load(pb["Wv"])
    for k, v in run.items():
        knob(k, v)
    cfg = engine.default_loss_cfg()
    cfg["beta"] = 1e-4
    up = eng.mem.from_numpy
    tg = eng.style_targets(up(pb["style"]), cfg)
    (losses, dy), n_loss = profiled_launches(eng, lambda: eng.perceptual_loss(up(pb["y"]), up(pb["xc"]), tg, cfg))
    losses, dy = eng.mem.to_numpy(losses).copy(), eng.mem.to_numpy(dy).copy()
    dx, n_dgrad = profiled_launches(eng, lambda: eng.vgg_dgrad(up(pb["y"]), list(SELECTION_DGRAD_LAYERS), [up(pb["dfe"][n]) for n in SELECTION_DGRAD_LAYERS]))
    dx = eng.mem.to_numpy(dx).copy()
    print("(%r, %r): {\"perceptual_loss\": %r,\n    \"vgg_dgrad\": %r}," % (backend, setting, n_loss, n_dgrad))
    print("   loss error %.2e   dy %.2e   dx %.2e (max-abs, relative to the largest element)" % (
        np.abs(losses / np.asarray(pb["losses"]) - 1).max(), np.abs(dy - pb["dyo"]).max() / np.abs(pb["dyo"]).max(), np.abs(dx - pb["dxo"]).max() / np.abs(pb["dxo"]).max()))
    want = SELECTION_LAUNCHES[(backend, setting)]
    assert n_loss == want["perceptual_loss"]
    assert n_dgrad == want["vgg_dgrad"]
    np.testing.assert_allclose(losses, pb["losses"], rtol=2e-5)
    assert flat_close(dy, pb["dyo"])
    assert flat_close(dx, pb["dxo"])


def test_adam_tf_step_matches_oracle(eng):
    rng = np.random.default_rng(2)
    n = 5000
    p = rng.standard_normal(n).astype(np.float32)
    m = np.zeros(n, np.float32)
    v = np.zeros(n, np.float32)
    po, mo, vo = {"a": p.astype(np.float64)}, {"a": m.astype(np.float64)}, {"a": v.astype(np.float64)}
    pd, md, vd = (eng.mem.from_numpy(t) for t in (p, m, v))
    for t in (1, 2, 3):
        g = rng.standard_normal(n).astype(np.float32)
        eng.adam_tf_step(pd, eng.mem.from_numpy(g), md, vd, t)
        perceptual.adam_tf(po, {"a": g.astype(np.float64)}, mo, vo, t)
    np.testing.assert_allclose(eng.mem.to_numpy(pd), po["a"], rtol=0, atol=2e-6)
    # float32(0.999) != 0.999: (1-beta2) carries a 1.3e-5 relative rounding, exactly as in TF's float32 ApplyAdam
    np.testing.assert_allclose(eng.mem.to_numpy(vd), vo["a"], rtol=1e-4, atol=1e-12)


# ----------------------------------------------------------------------------- GPU-only: the differentiable builder-level API (torch tensors)
@pytest.mark.gpu
def test_loss_composed_from_the_differentiable_pieces_matches_the_fused_call_and_the_oracle():
    """Round 6: a script composes the objective from the reference's own helper names -- vgg16(...).layers / utils.get_layers, utils.get_grams,
    losses.content_loss / style_loss / tv_loss -- on a tensor that requires grad and calls .backward(), as train.py:157-204 and slow_style.py:140-176 do
    with tf.gradients.  Every node is one C-ABI call behind a torch.autograd.Function (fs_vgg_features / fs_vgg_dgrad, fs_gram_fwd / fs_gram_bwd,
    fs_loss_sqdiff_grad, fs_loss_tv_grad).  Against fs_perceptual_loss (the fused fixed-form path) and the float64 oracle: losses 2e-5, dL/dY as tight as the
    fused path is held."""
    import torch
    from faststyle_amd import losses, utils, vgg16
    e = get_engine("hip")
    rng = np.random.default_rng(1)
    Wv = perceptual.synthetic_vgg_weights(seed=3)
    e.vgg_load(Wv)
    cfg = engine.default_loss_cfg()
    cfg["beta"] = 1e-4
    style = rng.uniform(0, 255, (1, 37, 45, 3)).astype(np.float32)
    tg = e.style_targets(e.mem.from_numpy(style), cfg)
    y = rng.uniform(0, 255, (2, 32, 40, 3)).astype(np.float32)
    xc = rng.uniform(0, 255, (2, 32, 40, 3)).astype(np.float32)
    lf, dyf = e.perceptual_loss(e.mem.from_numpy(y), e.mem.from_numpy(xc), tg, cfg)
    lf, dyf = e.mem.to_numpy(lf).copy(), e.mem.to_numpy(dyf).copy()
    # the same objective, node by node
    Y = e.mem.from_numpy(y).requires_grad_(True)
    net = vgg16.vgg16(Y, engine=e)                                             # (the weights are loaded: vgg_load above)
    tnet = vgg16.vgg16(e.mem.from_numpy(xc), engine=e)
    content = utils.get_layers(["vgg/conv3_3:0"], net)                         # (the reference's tensor names, utils.py:55-63)
    targets = utils.get_layers(["vgg/conv3_3:0"], tnet)
    grams = utils.get_grams(["vgg/%s:0" % n for n in cfg["style_layers"]], net)
    closs = losses.content_loss(content, targets, cfg["content_weights"], engine=e)
    sloss = losses.style_loss(grams, tg, cfg["style_weights"], engine=e)
    tv = losses.tv_loss(Y, engine=e)
    loss = closs + sloss + cfg["beta"] * tv                                     # train.py:184
    assert loss.requires_grad
    loss.backward()
    got = np.array([loss.item(), closs.item(), sloss.item(), cfg["beta"] * tv.item()])
    np.testing.assert_allclose(got, lf, rtol=2e-5)
    dy = Y.grad.detach().cpu().numpy()
    assert flat_close(dy, dyf, tight=2e-5)                                      # two launch sequences of the same library: rounding apart
    tgo = perceptual.target_grams(style.astype(np.float64), f64(Wv), cfg["style_layers"])
    feats = perceptual.vgg16(xc.astype(np.float64), f64(Wv), upto="conv3_3")
    lo, dyo = perceptual.perceptual_loss(y.astype(np.float64), [feats["conv3_3"]], tgo, f64(Wv), beta=1e-4)
    np.testing.assert_allclose(got, [lo[k] for k in ("loss", "content_loss", "style_loss", "tv_loss")], rtol=2e-5)
    assert flat_close(dy, dyo)
    # value-only use (no grad required) keeps returning plain device scalars
    v = losses.tv_loss(e.mem.from_numpy(y), engine=e)
    assert not getattr(v, "requires_grad", False) and abs(float(e.mem.to_numpy(v)[0]) - tv.item()) <= 1e-6 * abs(tv.item())


# ----------------------------------------------------------------------------- GPU-only, full sizes
@pytest.mark.gpu
@pytest.mark.parametrize("style", ["starry", "candy"])
def test_hip_reproduces_shipped_golden_jpeg(style):
    """The reference's own known answer (README.md:5-18) through the HIP path, full 474x712."""
    e = get_engine("hip")
    assets = os.path.join(ROOT, "tests", "golden", "ref_assets")
    x = load_rgb(os.path.join(assets, "chicago.jpg")).astype(np.float32)[None]
    W = ckpt.load_checkpoint(os.path.join(ROOT, "models", style + "_final.ckpt"))
    y = e.mem.to_numpy(e.tnet_forward(e.mem.from_numpy(e.flatten_params(W)), e.mem.from_numpy(x)))
    assert y.shape == (1, 476, 712, 3)
    dec = jpeg_roundtrip(y[0])
    gold = load_rgb(os.path.join(assets, style + "_chicago.jpg"))
    assert psnr(dec, gold) >= 63.0
    assert (dec == gold).mean() >= 0.985
    yo = tnet.create_net(x, tnet.strip_scope(W))               # float32 oracle, same input
    assert np.abs(y - yo).max() / 255.0 < 1e-4


@pytest.mark.gpu
def test_hip_720p_forward_matches_oracle():
    """BASELINE config 2: 720p frame, batch 1, fp32, starry weights, rng(0) uniform[0,255)."""
    e = get_engine("hip")
    W = starry()
    x = np.random.default_rng(0).uniform(0, 255, (1, 720, 1280, 3)).astype(np.float32)
    y = e.mem.to_numpy(e.tnet_forward(e.mem.from_numpy(e.flatten_params(W)), e.mem.from_numpy(x)))
    assert y.shape == (1, 720, 1280, 3) and np.isfinite(y).all() and y.min() >= 0 and y.max() <= 255
    yo = tnet.create_net(x, tnet.strip_scope(W))
    assert np.abs(y - yo).max() <= 0.255        # 1e-3 * 255, the north-star tolerance


@pytest.mark.gpu
def test_hip_train_step_256_matches_oracle_and_batch_sum_property(knob_hip):
    """BASELINE config 3 shape (256x256): losses + all 48 gradients vs the float32 oracle on a
    batch of 2, and the data-parallel identity grads(batch) == sum of per-sample grads (losses are
    batch-summed, losses.py:32,63; instance norm is per sample) that the 8-GPU SUM all-reduce
    relies on.  (The identity is held to 3e-4 of the largest gradient with the SAME conv kernels on both
    sides -- a different summation order in a FORWARD conv flips ReLU ties: the half-item Winograd kernel a batch of 2
    selects for the residual convs is therefore also selected for the single samples, and the VGG Winograd convs run
    without split-K, which a batch of 1 and a batch of 2 would otherwise take with different factors on conv3_x / conv4_x;
    tools/w4_slp_repro.py shows the F(4x4) kernel bit-identical per sample whatever batch it rides in.  What remains differs by
    construction with the batch size: the pixel chunks of the instance-norm backward's partial sums and the slab partition
    of the filter gradients -- last-bit differences that the mean subtraction of sixteen instance-norm backwards amplifies
    to ~1e-4 of the largest gradient.)"""
    e = get_engine("hip")
    knob_hip("FS_WINO2H_MIN_ITEMS", 32)
    knob_hip("FS_WINO_KSPLIT", 1)
    rng = np.random.default_rng(1)
    Wv = perceptual.synthetic_vgg_weights(seed=3)
    e.vgg_load(Wv)
    cfg = engine.default_loss_cfg()
    P = tnet.init_params(seed=0)
    flat = e.mem.from_numpy(e.flatten_params(P, scope=""))
    style = rng.uniform(0, 255, (1, 96, 128, 3)).astype(np.float32)
    tg = e.style_targets(e.mem.from_numpy(style), cfg)
    x = rng.uniform(0, 255, (2, 256, 256, 3)).astype(np.float32)

    def step(xb):
        xd = e.mem.from_numpy(xb)
        y = e.tnet_forward(flat, xd, save_for_bwd=True)
        losses, dy = e.perceptual_loss(y, xd, tg, cfg)
        g = e.tnet_backward(flat, xd, dy)
        return e.mem.to_numpy(losses).copy(), e.mem.to_numpy(g).copy()

    l2, g2 = step(x)
    la, ga = step(x[:1])
    lb, gb = step(x[1:])
    np.testing.assert_allclose(l2, la + lb, rtol=1e-4)
    dp_err = np.abs(g2 - (ga + gb)).max() / np.abs(g2).max()
    print("data-parallel identity 2 x 256 x 256: max |g(batch) - sum g(sample)| / max |g| = %.2e (tolerance 3e-4)" % dp_err)   # (recorded in DESIGN.md section 2)
    assert dp_err < 3e-4
    tgo = perceptual.target_grams(style, Wv, cfg["style_layers"])
    lo, go, _ = perceptual.train_step(P, x, tgo, Wv)
    np.testing.assert_allclose(l2[:3], [lo["loss"], lo["content_loss"], lo["style_loss"]], rtol=1e-3)
    assert flat_close(g2, np.concatenate([go[n].ravel() for n, _, _ in e.param_table()]), l2=5e-3, cos_min=0.9999)


# ------------------------------------------------------------------ bf16 mixed-precision inference (BASELINE config 5)
def test_bf16_rounding_helper_known_answers():
    x = np.array([1.0, 1.00390625, 1.005859375, 1.01171875, 255.0, 0.1, -3.1415927], np.float32)
    # 1 + 2^-8 is a tie -> even (1.0); 1 + 1.5*2^-8 -> 1 + 2^-7; 1 + 3*2^-8 is a tie -> even (1 + 2^-6)
    want = np.array([1.0, 1.0, 1.0078125, 1.015625, 255.0, 0.10009765625, -3.140625], np.float32)
    assert np.array_equal(tnet.bf16_round(x), want)


@pytest.mark.parametrize("shape,grid_cap", [((2, 48, 56), None), ((1, 45, 67), None), ((2, 48, 56), 3)])
def test_tnet_bf16_forward_against_bf16_restatement_and_fp32_oracle(eng, shape, grid_cap, knob):
    """FS_FLAG_BF16 against (a) the numpy restatement with the same rounding points -- differences are
    accumulation-order noise flipping an occasional bf16 rounding -- and (b) the fp32/fp64 oracle, where
    the error is the precision of bfloat16 itself (~1e-2 of the range; reported, not held to 1e-3)."""
    if grid_cap:      # persistent workgroups: 3 workgroups walk all the tiles of a layer (crossing images): the pipeline of
        knob("FS_BF16_GRID", grid_cap)          # fs_bstream.hip (every layer behind the image layer) and of the image layer's kernel
        knob("FS_BSTREAM_WGS", grid_cap)
        knob("FS_BSTREAM_WGS64", grid_cap)
    rng = np.random.default_rng(4)
    P = tnet.strip_scope(starry())
    flat = eng.mem.from_numpy(eng.flatten_params(P, scope=""))
    x = rng.integers(0, 256, shape + (3,)).astype(np.float32)
    y = eng.mem.to_numpy(eng.tnet_forward(flat, eng.mem.from_numpy(x), bf16=True))
    yb = tnet.create_net_bf16(x, P)
    yo = tnet.create_net(x.astype(np.float64), f64(P))
    assert y.shape == yo.shape and np.isfinite(y).all()
    e_b = np.abs(y - yb)
    e_o = np.abs(y - yo)
    print("bf16 path: vs bf16 restatement max %.3f mean %.4f psnr %.1f dB | vs fp32 oracle max %.2f mean %.3f psnr %.1f dB"
          % (e_b.max(), e_b.mean(), psnr(y, yb), e_o.max(), e_o.mean(), psnr(y, yo)))
    assert psnr(y, yb) > 45 and e_b.mean() < 1.0
    assert psnr(y, yo) > 40 and e_o.mean() / 255.0 < 1e-2


@pytest.mark.gpu
def test_hip_1080p_batch_consistency_and_bf16_agreement():
    """BASELINE config 5 size (1080p): no CPU oracle at this size, so (a) samples of a batch are independent --
    a batch holding the same frame twice gives two identical outputs equal to the batch-1 result (instance
    norm is per sample; exercises persistent workgroups crossing the image boundary), (b) the bf16 path stays
    within its accuracy envelope of the fp32 path on a natural image (the shipped chicago.jpg, upscaled)."""
    from PIL import Image
    e = get_engine("hip")
    flat = e.mem.from_numpy(e.flatten_params(starry()))
    img = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "ref_assets", "chicago.jpg")).convert("RGB")
                     .resize((1920, 1080), Image.BICUBIC), dtype=np.float32)
    x1 = e.mem.from_numpy(img[None])
    x2 = e.mem.from_numpy(np.stack([img, img]))
    for bf16 in (False, True):
        y1 = e.mem.to_numpy(e.tnet_forward(flat, x1, bf16=bf16))
        y2 = e.mem.to_numpy(e.tnet_forward(flat, x2, bf16=bf16))
        assert y1.shape == (1, 1080, 1920, 3) and np.isfinite(y2).all()
        # (the two copies are the same to summation order, not to the bit: the remainder split of the residual Winograd
        # launches sums the input channels of the launch's LAST items in rem_ks partial sums -- fs_wino2.hip)
        assert np.abs(y2[0] - y2[1]).max() < (1e-3 * 255 if not bf16 else 3.0)
        # same arithmetic, different tiling walk: fp32 summation-order noise (measured 1.2e-4); in the bf16 path that
        # noise flips an occasional bfloat16 rounding, so there the bound is a few bf16 steps of the 0..255 range
        d = np.abs(y2[0] - y1[0])
        assert d.max() < (1e-3 * 255 if not bf16 else 3.0) and d.mean() < (1e-4 if not bf16 else 0.2)
        if not bf16:
            ref = y1
    assert psnr(y1, ref) > 40 and np.abs(y1 - ref).mean() / 255.0 < 1e-2


@pytest.mark.gpu
def test_hip_1080p_batch8_bf16_is_the_configured_batch():
    """BASELINE config 5 AS CONFIGURED: bf16, 1080p, batch 8 per GPU -- the shape bench.py times (persistent workgroups
    walk 8 images; item lists 8x the batch-1 case).  Eight different frames; every output must equal the batch-1 result
    of its own frame within the bf16 tiling-walk envelope, and the batch must stay inside the bf16-vs-fp32 accuracy
    envelope measured at batch 1."""
    import torch
    from PIL import Image
    e = get_engine("hip")
    flat = e.mem.from_numpy(e.flatten_params(starry()))
    img = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "ref_assets", "chicago.jpg")).convert("RGB")
                     .resize((1920, 1080), Image.BICUBIC), dtype=np.float32)
    frames = np.stack([np.roll(img, (37 * k, 101 * k), axis=(0, 1)) if k % 2 == 0 else np.ascontiguousarray(np.roll(img, 53 * k, axis=1)[::-1])
                       for k in range(8)])
    x8 = e.mem.from_numpy(frames)
    y8 = e.tnet_forward(flat, x8, bf16=True)
    assert tuple(y8.shape) == (8, 1080, 1920, 3) and bool(torch.isfinite(y8).all())
    for k in (0, 3, 7):
        y1 = e.tnet_forward(flat, x8[k:k + 1].contiguous(), bf16=True)
        d = (y8[k] - y1[0]).abs()
        assert float(d.max()) < 3.0 and float(d.mean()) < 0.2, (k, float(d.max()), float(d.mean()))
    yf = e.tnet_forward(flat, x8[5:6].contiguous())                       # fp32 path, one frame
    err = (y8[5] - yf[0]).abs()
    mse = float((err.double() ** 2).mean())
    assert 10 * np.log10(255.0 ** 2 / mse) > 40 and float(err.mean()) / 255.0 < 1e-2


@pytest.mark.gpu
def test_hip_1080p_forward_matches_the_float64_restatement():
    """BASELINE config 5 size with an ORACLE (round 6): one 1080p frame through the fp32 HIP path against the float64 restatement of create_net
    (im_transf_net.py:14-75 as written: REFLECT-40, materialised x4 nearest-neighbour upsample + stride-2 conv) -- oracle/torch_ref.py on the host's
    cores, itself held to the numpy oracle at 1e-8 (tests/test_oracle_backward.py), which is pinned on the reference's golden JPEGs.  Tolerances:
    5e-6 of the pixel range on the mean, 1e-4 of it on the worst of 6.2 M values (persistent workgroups over
    135 x 240-pixel residual maps, 33,750-tile instance-norm merges); the bf16 mode of the same frame inside its envelope against the SAME oracle."""
    import torch
    from PIL import Image
    from oracle import torch_ref
    e = get_engine("hip")
    W = starry()
    flat = e.mem.from_numpy(e.flatten_params(W))
    img = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "ref_assets", "chicago.jpg")).convert("RGB")
                     .resize((1920, 1080), Image.BICUBIC), dtype=np.float32)
    nt = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 8))       # (oneDNN float64 convs stop scaling early on a many-core host)
    try:
        with torch.no_grad():
            P = {k: torch.tensor(v, dtype=torch.float64) for k, v in tnet.strip_scope(W).items()}
            want = torch_ref.tnet(torch.tensor(img[None], dtype=torch.float64), P).numpy()
    finally:
        torch.set_num_threads(nt)
    assert want.shape == (1, 1080, 1920, 3)
    y = e.mem.to_numpy(e.tnet_forward(flat, e.mem.from_numpy(img[None])))
    d = np.abs(y - want)
    print("1080p fp32 against float64: max %.3e mean %.3e of the pixel range" % (d.max() / 255.0, d.mean() / 255.0))
    assert d.max() < 1e-4 * 255 and d.mean() < 5e-6 * 255      # measured: 4.9e-5 / 9.6e-7
    yb = e.mem.to_numpy(e.tnet_forward(flat, e.mem.from_numpy(img[None]), bf16=True))
    db = np.abs(yb - want)
    print("1080p bf16 against float64: PSNR %.1f dB, mean %.3e of the pixel range" % (psnr(yb, want), db.mean() / 255.0))
    assert psnr(yb, want) > 40 and db.mean() / 255.0 < 1e-2              # measured: 51.1 dB / 1.9e-3


# ------------------------------------------------------------------ the metric's own workload: 256x256, batch 32
@pytest.mark.gpu
def test_hip_train_step_b32_256_kernel_paths_and_data_parallel_identity(knob_hip):
    """BASELINE.json's metric shape, 32 x 256 x 256 (reference train.py:158-160 with --batch_size 32), the step bench.py
    times.  At this size the persistent item lists run several rounds, the transform net's residual convs switch to the
    Winograd kernel (>= 200 items), the filter-gradient slabs and the Gram pixel ranges split differently than at batch 4
    -- paths no smaller test takes.  The CPU oracle cannot run 32 images in test time, so:
      (a) the default kernels against the direct-convolution kernels (FS_CONV_WINO=0, FS_TNET_WINO=0) on the same inputs:
          forward pixels 2e-5 of the range, the four losses 2e-5, gradient direction;
      (b) the data-parallel identity the RCCL SUM all-reduce relies on: the gradient of the batch equals the sum of
          the gradients of its eight batch-4 shards (= the 8 x b4 shape of BASELINE configs[3]), losses likewise;
      (c) the float64 oracle on shard 0: the batch-32 run's y[0:4] and that shard's loss contribution."""
    import torch
    from faststyle_amd import utils
    e = get_engine("hip")
    style = utils.imread(os.path.join(ROOT, "style_images", "starry_night_crop.jpg")).astype(np.float32)[None]
    Wv = perceptual.synthetic_vgg_weights(seed=3)
    cfg = engine.default_loss_cfg()
    P = tnet.init_params(seed=0)
    gen = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.rand((32, 256, 256, 3), device="cuda", generator=gen) * 255.0

    def run(xb):
        e.vgg_load(Wv)
        flat = e.mem.from_numpy(e.flatten_params(P, scope=""))
        tg = e.style_targets(e.mem.from_numpy(style), cfg)
        y = e.tnet_forward(flat, xb, save_for_bwd=True)
        losses, dy = e.perceptual_loss(y, xb, tg, cfg)
        g = e.tnet_backward(flat, xb, dy)
        return y.double(), losses.double().clone(), g.double().clone()

    y_new, l_new, g_new = run(x)
    shard_l, shard_g = torch.zeros(4, device="cuda", dtype=torch.float64), torch.zeros_like(g_new)
    l_shard0 = None
    for r in range(8):
        _, l_r, g_r = run(x[4 * r:4 * r + 4].contiguous())
        if r == 0:
            l_shard0 = l_r.clone()
        shard_l += l_r
        shard_g += g_r
    # (c) one oracle-checked sample AT this shape: the float64 oracle on shard 0 (4 images) of the batch.  The batch-32 run's
    # own outputs y[0:4] are held to it at the forward tolerance; the shard's loss contribution twice: as the batch-4 HIP run of
    # that shard (2e-5) and as what the batch-32 run's batch-summed losses leave once the other seven shards are taken out
    # (a difference of eight near-equal terms: 2e-4).
    f64 = lambda d: dict((k, np.asarray(v, np.float64)) for k, v in d.items())
    x0 = x[0:4].cpu().numpy().astype(np.float64)
    y_o = tnet.create_net(x0, f64(P))
    assert np.abs(y_new[0:4].cpu().numpy() - y_o).max() < 2e-5 * 255
    W64 = f64(Wv)
    tgo = perceptual.target_grams(style.astype(np.float64), W64, cfg["style_layers"])
    ct = perceptual.vgg16(x0, W64, upto="conv3_3")
    fy = perceptual.vgg16(y_o, W64, upto="conv4_3")
    closs, _ = perceptual.content_loss([fy[n] for n in cfg["content_layers"]], [ct[n] for n in cfg["content_layers"]], cfg["content_weights"])
    sloss, _ = perceptual.style_loss([perceptual.gram(fy[n]) for n in cfg["style_layers"]], tgo, cfg["style_weights"])
    want0 = np.array([closs + sloss, closs, sloss])
    np.testing.assert_allclose(l_shard0.cpu().numpy()[:3], want0, rtol=2e-5)
    np.testing.assert_allclose((l_new - (shard_l - l_shard0)).cpu().numpy()[:3], want0, rtol=2e-4)
    knob_hip("FS_CONV_WINO", 0)
    knob_hip("FS_TNET_WINO", 0)
    y_dir, l_dir, g_dir = run(x)

    def cos_l2(a, b):
        return float(torch.dot(a, b) / (a.norm() * b.norm())), float((a - b).norm() / b.norm())
    assert bool(torch.isfinite(g_new).all()) and float(g_new.norm()) > 0
    # two float32 paths against each other: each is held to the float64 oracle at 2e-5 of the range (above, and test_tnet_forward_...), so their
    # difference has a budget of 4e-5; measured 1.2e-5 .. 1.6e-5 with 16 x 16-pixel items, 2.03e-5 since the residual convs of this shape take
    # the flattened tile lists (round 5: the statistics records partition the pixels differently)
    dy_paths = float((y_new - y_dir).abs().max())
    print("b32 256x256: forward pixels, default vs direct kernels: %.2e of the range" % (dy_paths / 255))
    assert dy_paths < 3e-5 * 255
    assert float(((l_new - l_dir).abs() / l_dir.abs().clamp_min(1e-30))[:3].max()) < 2e-5, (l_new, l_dir)
    c1, e1 = cos_l2(g_new, g_dir)
    # (b): losses are batch sums (losses.py:32,63), instance norm / Grams are per sample
    assert float(((shard_l - l_new).abs() / l_new.abs().clamp_min(1e-30))[:3].max()) < 2e-5, (shard_l, l_new)
    c2, e2 = cos_l2(shard_g, g_new)
    print("b32 256x256: default vs direct kernels cos %.8f relL2 %.2e; sum of 8 b4 shards vs b32 cos %.8f relL2 %.2e" % (c1, e1, c2, e2))
    assert c1 > 0.99999 and c2 > 0.99999 and e1 < 1e-3 and e2 < 1e-3, (c1, e1, c2, e2)


# ------------------------------------------------------------------ gradients to rounding: the oracle with the HIP path's masks
def maskinject_units():
    from tests import maskinject
    return maskinject.RELU_UNITS.values()


def test_train_step_gradients_to_rounding_with_injected_masks(eng):
    """Shipped weights (real ReLU sign patterns, not the kink-free construction), synthetic VGG: with the HIP path's own
    ReLU masks and pooling arg-max fed to the float64 oracle's backward, ALL 48 gradients are held to the per-tensor 2e-4
    that test_tnet_..._kink_free needs special parameters for."""
    rng = np.random.default_rng(21)
    P = tnet.strip_scope(starry())
    x = rng.uniform(0, 255, (2, 48, 56, 3)).astype(np.float32)
    style = rng.uniform(0, 255, (1, 40, 52, 3)).astype(np.float32)
    cfg = engine.default_loss_cfg()
    cfg["beta"] = 1e-4
    from tests import maskinject
    lh, lo, g, go, masks = maskinject.step_with_injected_masks(eng, P, x, style, perceptual.synthetic_vgg_weights(3), cfg)
    np.testing.assert_allclose(lh[:3], [lo["loss"], lo["content_loss"], lo["style_loss"]], rtol=2e-5)
    assert grads_close(eng, g, go, 2e-4) == []
    assert set(masks["tnet"]) == set(maskinject_units()) and "pool3/idx" in masks["vgg"]
