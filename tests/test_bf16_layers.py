"""The bf16 inference path (FS_FLAG_BF16: fs_bstream.hip, fs_bf16.hip) held LAYER BY LAYER against float64.

One forward per (kernel selection, shape) leaves every intermediate in the caller's workspace (fs_tnet_bf16_ws_tensor); each unit is then
recomputed in float64 from what HIP stored for the unit before it (teacher forcing: oracle.tnet.bf16_unit), so one layer's rounding flips
cannot leak into the next layer's comparison, and a wrong element of ONE layer is a failure of that layer instead of -50 dB in the picture.

The bounds are derived, not measured:
  * packed filters, instance-norm scale a, residual sums (off rounding ties): to the bit;
  * conv outputs: |bf2f(z_hip) - z_ref| <= ulp_bf16(|z_ref| + E) / 2 + E with E = 2 K 2^-24 S, K the terms per output as executed and S the
    same conv of |x| with |w|: bf16 x bf16 products are exact in fp32, any-order fp32 accumulation errs by at most K u S, the factor 2 lets the
    matrix unit's internal adds truncate instead of rounding; the stored value is the accumulator rounded once to bfloat16;
  * statistics: the 2e-5 the fp32 kernels' tile statistics are held to (tests/test_kernels_parity.py);
  * the output end: the project's forward bar, 2e-5 of the pixel range (tests/test_path_parity.py).
Set BF16_LAYER_PARITY_JSON=<file> to have the measured maxima of err / bound written there (profiles/bf16_layer_parity.json is such a GPU run)."""
import contextlib
import json
import os

import numpy as np
import pytest

from faststyle_amd import _lib as L, ckpt
from oracle import nnops, tnet
from tests.backends import engine_params, get_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_STATS = 2e-5          # tests/test_kernels_parity.py: TOL, as test_conv_producer_instnorm_folded_into_load_and_stats holds mean and rstd
TOL_PIXELS = 2e-5 * 255   # tests/test_path_parity.py: forward pixels

SHAPES = {"41x43": (2, 41, 43),    # the minimum size: odd extents, stride-2 layers with odd inputs, partial 16x16 tiles everywhere
          "48x56": (1, 48, 56),
          "45x67": (3, 45, 67)}    # the grid-capped cases: three workgroups walk three images
SELECTIONS = {
    "default": {},
    "round2": {"FS_BSTREAM": 0},                                             # the kernels of fs_bf16.hip everywhere
    "round2_wm1": {"FS_BSTREAM": 0, "FS_BF16_WM": 1},                        # ... with the 128-pixel tile
    "mixed": {"FS_BSTREAM_MASK": 4},                                         # only the residual instance streams: both families in one forward
    "walk": {"FS_BSTREAM_WGS": 3, "FS_BSTREAM_WGS64": 3, "FS_BF16_GRID": 3},
    "round2_walk": {"FS_BSTREAM": 0, "FS_BF16_GRID": 3},
}
# the emulator is ~10^3 x slower than the GPU: the default selection at every shape and the round-2 kernels at the smallest
EMU_CASES = [("default", "41x43"), ("default", "48x56"), ("default", "45x67"), ("round2", "41x43")]
HIP_CASES = [(s, g) for s in ("default", "round2", "mixed") for g in ("41x43", "48x56")] + \
            [("round2_wm1", "41x43"), ("default", "45x67"), ("walk", "45x67"), ("round2_walk", "45x67")]
CASES = [pytest.param(e.values[0], s, g, id="%s-%s-%s" % (e.id, s, g), marks=e.marks)
         for e in engine_params() for s, g in (EMU_CASES if e.values[0] == "emu" else HIP_CASES)]

K_TERMS = [243] + [9 * 16, 9 * 32] + [9 * 64] * 10 + [4 * 64, 4 * 32, 18 * 16]   # taps x Cin per output as executed
BS_DEFAULT = [7, 1, 2] + [3] * 10 + [4, 5, 6]
CIN = [3, 16, 32] + [64] * 10 + [64, 32, 16]

_params = {}
_snaps = {}
_refs = {}
_figures = {}


def starry():
    if not _params:
        _params["P"] = tnet.strip_scope(ckpt.load_checkpoint(os.path.join(ROOT, "models", "starry_final.ckpt")))
    return _params["P"]


@contextlib.contextmanager
def knobs(eng, env):
    """FS_* tuning knobs for one forward: the library caches the environment, so it is told to re-read it now and again afterwards."""
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            os.environ[k] = str(v)
        eng.lib.fs_debug_reload_env()
        eng.reset_workspaces()
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        eng.lib.fs_debug_reload_env()
        eng.reset_workspaces()


def snapshot(kind, sel, shape_id):
    """ONE forward of this selection and shape; everything it left in the workspace, on the host."""
    key = (kind, sel, shape_id)
    if key in _snaps:
        return _snaps[key]
    eng = get_engine(kind)
    N, H, W = SHAPES[shape_id]
    P = starry()
    x = np.random.default_rng(7).integers(0, 256, (N, H, W, 3)).astype(np.float32)
    s = {"N": N, "H": H, "W": W, "x": x, "sel": sel}
    with knobs(eng, SELECTIONS[sel]):
        s["plan"] = [eng.tnet_bf16_plan(N, H, W, i) for i in range(16)]
        ws = eng.new_tnet_workspace(N, H, W, bf16=True)
        flat = eng.mem.from_numpy(eng.flatten_params(P, scope=""))
        s["y"] = np.array(eng.mem.to_numpy(eng.tnet_forward(flat, eng.mem.from_numpy(x), bf16=True, workspace=ws)))
        get = lambda unit, what: eng.tnet_bf16_saved(ws, N, H, W, unit, what)
        for name, what in (("z", L.FS_TNET_BWS_Z), ("a", L.FS_TNET_BWS_A), ("b", L.FS_TNET_BWS_B), ("mean", L.FS_TNET_BWS_MEAN),
                           ("rstd", L.FS_TNET_BWS_RSTD), ("wpk", L.FS_TNET_BWS_WPK)):
            s[name] = [get(i, what) for i in range(16)]
        s["h"] = [get(k, L.FS_TNET_BWS_H) for k in range(5)]
        s["zfold"] = get(15, L.FS_TNET_BWS_ZFOLD)
    _snaps[key] = s
    return s


def unit_input(s, i):
    """What unit i read, as HIP stored it: (tensor values, a, b)."""
    val = tnet.bf16_from_bits
    if i == 0:
        return s["x"], None, None
    if i in (5, 7, 9, 11, 13):                     # first conv of residual block k >= 1, and the first resize-conv: a residual sum
        return val(s["h"][(i - 5) // 2]), None, None
    return val(s["z"][i - 1]), s["a"][i - 1], s["b"][i - 1]


def reference(kind, sel, shape_id):
    """Per unit (z_ref, S) of oracle.tnet.bf16_unit on HIP's own stored input; computed once per forward, shared by the tests, never modified."""
    key = (kind, sel, shape_id)
    if key not in _refs:
        s = snapshot(*key)
        out = []
        for i in range(16):
            src, a, b = unit_input(s, i)
            _, z_ref, S = tnet.bf16_unit(i, src, starry(), a, b)
            z_ref.setflags(write=False)
            S.setflags(write=False)
            out.append((z_ref, S))
        _refs[key] = out
    return _refs[key]


def record(kind, sel, shape_id, name, values):
    _figures.setdefault("%s/%s/%s" % (kind, sel, shape_id), {})[name] = values
    path = os.environ.get("BF16_LAYER_PARITY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump(_figures, f, indent=1, sort_keys=True)


def ulp_bf16(v):
    """Spacing of bfloat16 (8 significant bits) at magnitude v; 0 at 0."""
    v = np.abs(np.asarray(v, np.float64))
    _, ex = np.frexp(v)
    return np.where(v > 0, np.ldexp(1.0, np.maximum(ex - 1, -126) - 7), 0.0)


def rel(got, want):
    return np.abs(np.asarray(got, np.float64) - want).max() / (np.abs(want).max() + 1e-30)


def where_worst(err_over_bound, n=6):
    idx = np.argsort(err_over_bound, axis=None)[::-1][:n]
    return [tuple(int(v) for v in np.unravel_index(j, err_over_bound.shape)) for j in idx]


# ------------------------------------------------------------------------------------------------------------------ kernel selection
@pytest.mark.parametrize("kind,sel,shape_id", CASES)
def test_kernel_selection_is_what_the_case_is_about(kind, sel, shape_id):
    """The PLAN query, not an assumption: which kernel family runs every unit, with which tile, and that the shapes do reach the ragged paths."""
    s = snapshot(kind, sel, shape_id)
    plan, N = s["plan"], s["N"]
    bs = [p["bs"] for p in plan]
    if sel in ("default", "walk"):
        assert bs == BS_DEFAULT
    elif sel == "mixed":
        assert bs == [0, 0, 0] + [3] * 10 + [0, 0, 0]
    else:
        assert bs == [0] * 16
    assert [p["c4"] for p in plan] == [1] + [0] * 15
    if sel.startswith("round2"):
        # both round-2 kernels occur: the resident one (the whole Cin in one staged chunk) and the chunked one
        resident = [i for i in range(1, 16) if plan[i]["CC"] == CIN[i]]
        chunked = [i for i in range(1, 16) if plan[i]["CC"] < CIN[i]]
        assert resident and chunked, (resident, chunked)
        assert all(i in resident for i in (1, 15)) and all(i in chunked for i in range(3, 13))
    if sel.startswith("round2"):
        # conv_bf16_plan keeps the 256-pixel tile (WM = 2) only for a launch of >= 512 workgroups, i.e. >= 131072 output pixels per channel block:
        # no shape a float64 reference covers in seconds reaches it in any layer behind the image layer, so FS_BF16_WM=1 pins what these shapes plan
        # anyway and the WM = 2 instances of the round-2 kernels stay with the 1080p whole-network tests
        assert all(p["WM"] == 1 for p in plan)
    for i, p in enumerate(plan):
        if p["bs"]:
            assert p["CC"] == (4 if i == 0 else CIN[i]) and p["BN"] == (64 if i in range(2, 15) else 32)
    # layers whose channel block is padded: the image layer (16 of 32) and the folded output layer (15 real columns of 16, of 32)
    assert plan[0]["cout_pad"] == 32 and plan[15]["cout_pad"] == 32
    if sel in ("default", "walk", "mixed"):       # 16 x 16-pixel tiles: a partial last tile row AND column in every streamed unit but the odd exact fit
        dims = [s["z"][i].shape if i < 15 else s["zfold"].shape for i in range(16)]
        conv_hw = [(d[1] // 2, d[2] // 2) if i in (13, 14) else (d[1], d[2]) for i, d in enumerate(dims)]
        partial = [i for i in range(16) if plan[i]["bs"] and conv_hw[i][0] % 16 and conv_hw[i][1] % 16]
        assert all(plan[i]["tiles_y"] == -(-conv_hw[i][0] // 16) and plan[i]["tiles_x"] == -(-conv_hw[i][1] // 16) for i in range(16) if plan[i]["bs"])
        assert 2 * len(partial) >= sum(1 for p in plan if p["bs"]), partial
    if sel.endswith("walk"):                      # three workgroups per channel block walk every tile of all three images
        assert N == 3 and all(N * p["tiles_y"] * p["tiles_x"] > 3 for p in plan)


# ------------------------------------------------------------------------------------------------------------------ packed filters
@pytest.mark.parametrize("kind,sel,shape_id", CASES)
def test_packed_filters_to_the_bit(kind, sel, shape_id):
    """pack_bf16_kernel's four layouts (PK_C4, PK_CONV, PK_UP, PK_FOLD) of the shipped checkpoint against their numpy restatement, zero padding
    included: co >= Cout, kw >= 9 and the 4th channel of the image layer, j >= 15 of the fold.  PK_UP's float32 sums run in kh, kw order."""
    s = snapshot(kind, sel, shape_id)
    for i in range(16):
        want = tnet.bf16_packed_filter(i, starry(), s["plan"][i]["cout_pad"])
        got = s["wpk"][i]
        assert got.shape == want.shape, (i, got.shape, want.shape)
        bad = np.argwhere(got != want)
        assert not len(bad), "unit %d: %d packed filter elements differ, first at [tap, co, ci] = %s" % (i, len(bad), bad[:4].tolist())
    wq = tnet.bf16_packed_filter(15, starry(), 32)
    assert not wq[:, 15:].any() and not wq[1::2, 12:15].any() and wq[0::2, :15].any()        # j >= 15; kw = 5 + 4 does not exist
    w0 = tnet.bf16_packed_filter(0, starry(), 32).reshape(9, 32, 12, 4)
    assert not w0[:, 16:].any() and not w0[:, :, 9:].any() and not w0[..., 3].any()


# ------------------------------------------------------------------------------------------------------------------ conv outputs
@pytest.mark.parametrize("kind,sel,shape_id", CASES)
def test_every_conv_output_element_within_the_accumulation_bound(kind, sel, shape_id):
    """Every stored element of every unit (both pixel-shuffle stores in their stored [N,2H,2W,C] order, the folded output layer's zfold with
    its unread border columns) against the float64 conv of HIP's own stored input: the bound of the module docstring, no element excluded."""
    s = snapshot(kind, sel, shape_id)
    ref = reference(kind, sel, shape_id)
    worst, fails = [], []
    for i in range(16):
        z_ref, S = ref[i]
        got = tnet.bf16_from_bits(s["z"][i] if i < 15 else s["zfold"])
        assert got.shape == z_ref.shape, (i, got.shape, z_ref.shape)
        assert np.isfinite(got).all(), i
        E = 2.0 * K_TERMS[i] * 2.0 ** -24 * S
        bound = 0.5 * ulp_bf16(np.abs(z_ref) + E) + E
        err = np.abs(got - z_ref)
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        worst.append(float(ratio.max()))
        print("unit %2d (%s): max err/bound %.4f, %d elements" % (i, s["plan"][i], ratio.max(), ratio.size))
        if not (err <= bound).all():
            fails.append("unit %d plan %s: %d of %d elements outside the bound, worst err/bound %.3g at [n, y, x, c] = %s"
                         % (i, s["plan"][i], int((err > bound).sum()), err.size, ratio.max(), where_worst(ratio)))
    record(kind, sel, shape_id, "conv_err_over_bound", worst)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("kind,sel,shape_id", CASES)
def test_instance_norm_statistics_of_every_unit(kind, sel, shape_id):
    """mean and rstd per (n, c) against float64 statistics of the UNROUNDED reference conv (what the fp32 accumulators approximate; unit 15: of
    the float64 fold of HIP's zfold), at the tolerance test_conv_producer_instnorm_folded_into_load_and_stats holds the fp32 kernels' tile
    statistics to: max |got - want| / max |want| < 2e-5 (tests/test_kernels_parity.py TOL).  The shapes leave partial last tile rows and columns
    and padded channel blocks (asserted with the selection): a masked pixel or a padded channel that entered a sum fails here.  Then a == gamma *
    rstd to the bit and b == beta - mean * a within one fp32 rounding of each of its two operations, both from HIP's OWN mean and rstd."""
    s = snapshot(kind, sel, shape_id)
    ref = reference(kind, sel, shape_id)
    P = starry()
    fig = {"mean": [], "rstd": []}
    fails = []
    for i in range(16):
        z_ref = ref[i][0] if i < 15 else tnet.bf16_fold5(tnet.bf16_from_bits(s["zfold"]))
        _, gkey, bkey = tnet.BF16_UNITS[i][:3]
        gamma, beta = np.asarray(P[gkey], np.float32), np.asarray(P[bkey], np.float32)
        mean, rstd, _, _ = tnet.bf16_norm_consts(z_ref, gamma.astype(np.float64), beta.astype(np.float64))
        mean, rstd = mean[:, 0, 0, :], rstd[:, 0, 0, :]
        assert s["mean"][i].shape == mean.shape == (s["N"], len(gamma))
        em, er = rel(s["mean"][i], mean), rel(s["rstd"][i], rstd)
        fig["mean"].append(float(em))
        fig["rstd"].append(float(er))
        print("unit %2d: mean %.2e rstd %.2e of the largest" % (i, em, er))
        if not (em < TOL_STATS and er < TOL_STATS):
            d = np.abs(s["mean"][i] - mean)
            fails.append("unit %d plan %s: mean %.3g rstd %.3g, worst mean at [n, c] = %s" % (i, s["plan"][i], em, er, where_worst(d, 3)))
        a_want = gamma[None, :] * s["rstd"][i]                                                                  # float32 product: one rounding
        if not np.array_equal(s["a"][i], a_want):
            fails.append("unit %d: a != gamma * rstd at %s" % (i, np.argwhere(s["a"][i] != a_want)[:3].tolist()))
        prod = s["mean"][i].astype(np.float64) * s["a"][i].astype(np.float64)
        b_want = beta.astype(np.float64)[None, :] - prod
        b_tol = 2.0 ** -23 * (np.abs(beta.astype(np.float64))[None, :] + np.abs(prod))                         # fused or not: <= 1/2 ulp twice
        if not (np.abs(s["b"][i] - b_want) <= b_tol).all():
            fails.append("unit %d: b != beta - mean * a, worst %.3g of its tolerance" % (i, (np.abs(s["b"][i] - b_want) / b_tol).max()))
    record(kind, sel, shape_id, "stats_rel_err", fig)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------------ residual sums
TIE_WINDOW = 2.0 ** -22   # distance of the float64 value from a bfloat16 rounding tie, relative to the largest fp32 intermediate, inside which it is not compared


@pytest.mark.parametrize("kind,sel,shape_id", CASES)
def test_residual_sums_to_the_bit(kind, sel, shape_id):
    """apply_res_bf16_kernel: h[k] == bf16(fmaf(z, a, b) + T(skip)[y+2, x+2]) evaluated in float64 from HIP's stored operands and rounded once
    (block 0: T = the on-load affine + ReLU of the raw initconv_2 output).  To the bit, except next to a rounding tie: the kernel rounds three
    fp32 intermediates -- t = fmaf(z, a, b), T(skip) in block 0, and their sum -- each by at most 2^-24 of its own magnitude, so its pre-rounding
    value is within 3 x 2^-24 < 2^-22 of the LARGEST of |t|, |T(skip)|, |sum| from the float64 one.  An element whose float64 value lies within
    2^-22 of a tie on that scale is decided from the reference alone and skipped; the skipped share is asserted <= 1 % (measured: below 5e-4 on every input here).
    (Relative to |sum| alone the window is too narrow exactly where t and the skip cancel: emulator, 41x43, default selection, block 0, element
    [0, 5, 25, 17]: t = -0.712111915, skip = 0.712133999, sum 2.208e-05 lies 1.4e-3 of itself from the tie but only 4.2e-8 = 0.7 x 2^-24 of |t|;
    1 to 4 such elements of ~10^5 per case, every one with |sum| < |t| / 90.)"""
    s = snapshot(kind, sel, shape_id)
    val = tnet.bf16_from_bits
    skipped = []
    for k in range(5):
        i = 4 + 2 * k
        z = val(s["z"][i])
        if k == 0:
            skip, sa, sb = val(s["z"][2]), s["a"][2], s["b"][2]
        else:
            skip, sa, sb = val(s["h"][k - 1]), None, None
        v = tnet.bf16_residual(z, s["a"][i], s["b"][i], skip, sa, sb)
        assert v.shape == s["h"][k].shape
        t = tnet.bf16_residual(z, s["a"][i], s["b"][i], np.zeros_like(skip))                  # fmaf(z, a, b) alone
        scale = np.maximum(np.abs(v), np.maximum(np.abs(t), np.abs(v - t)))
        u = ulp_bf16(v)
        frac = np.where(u > 0, np.abs(v) / np.where(u > 0, u, 1.0), 0.0) % 1.0
        near_tie = np.abs(frac - 0.5) * u <= TIE_WINDOW * scale
        skipped.append(float(near_tie.mean()))
        want = tnet.bf16_bits(v)
        bad = np.argwhere((s["h"][k] != want) & ~near_tie)
        print("block %d: %d of %d elements near a tie, %d differ" % (k, int(near_tie.sum()), v.size, len(bad)))
        assert near_tie.mean() <= 0.01, (k, near_tie.mean())
        assert not len(bad), "block %d: %d elements differ, first at [n, y, x, c] = %s" % (k, len(bad), bad[:6].tolist())
    record(kind, sel, shape_id, "residual_skipped_share", skipped)


# ------------------------------------------------------------------------------------------------------------------ output end
@pytest.mark.parametrize("kind,sel,shape_id", CASES)
def test_fold_last_instance_norm_and_tanh(kind, sel, shape_id):
    """The fp32 end of the path from HIP's zfold: the 5-term fold (fp32 sums of five bfloat16 values: within 5 x 2^-24 of their absolute sum), then
    the last instance norm and the scaled tanh in float64 against y at the project's forward bar, 2e-5 of the pixel range."""
    s = snapshot(kind, sel, shape_id)
    P = starry()
    Z = tnet.bf16_from_bits(s["zfold"])
    z = tnet.bf16_fold5(Z)
    assert s["z"][15].shape == z.shape and s["y"].shape == z.shape
    e_fold = np.abs(s["z"][15] - z)
    assert (e_fold <= 5 * 2.0 ** -24 * tnet.bf16_fold5(np.abs(Z))).all(), where_worst(e_fold)
    n, _ = nnops.inst_norm(z, np.asarray(P["upsample_2/INscale"], np.float64), np.asarray(P["upsample_2/INshift"], np.float64))
    want = nnops.scaled_tanh(n)
    err = np.abs(s["y"] - want)
    print("output end: max %.3e of the pixel range" % (err.max() / 255.0))
    record(kind, sel, shape_id, "output_end_max_err_of_range", float(err.max() / 255.0))
    assert np.isfinite(s["y"]).all() and err.max() < TOL_PIXELS, where_worst(err)
