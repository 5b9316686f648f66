"""The instance-norm kernels of fs_elem.hip in every form a knob or a size selects, against float64.

The train step's backward (in_bwd_rec: in_bwd_partial4_kernel<8> -> in_bwd_apply_rec_kernel -> in_bwd_params_kernel) walks its software-pipelined
loop more than once only when HW * C / 4 > 1024 * max(1, FS_INBWD_APPLY_WGS / N) -- by itself at batch 32 --, and the three-launch vector form
(in_bwd_partial4_kernel<4>, in_bwd_final_all_kernel / in_bwd_final_kernel, in_bwd_apply4_kernel) runs only under FS_INBWD_REC=0: the FS_INBWD_* knobs
send both through shapes of a few hundred pixels here.  fs_instnorm_finalize is fed synthetic records instead of a conv's.

Worst errors measured with these very cases (relative to each output's largest magnitude; the bounds are 5e-5 and 2e-5):
  backward, emulator   defaults 8.0e-07  rec0 8.0e-07  rec0_chunk64 3.9e-07  maxt2_punr4 8.0e-07  apply_wgs1 8.0e-07   (flat channel + spike: 2.2e-07 each)
  backward, MI355X     defaults 7.4e-07  rec0 7.4e-07  rec0_chunk64 4.6e-07  maxt2_punr4 7.4e-07  apply_wgs1 7.4e-07   (flat channel + spike: 2.2e-07, 1.7e-07 rec0_chunk64)
  finalize, emulator   FS_FINALIZE_MIN_T default 1.9e-07, 1: 1.9e-07
  finalize, MI355X     FS_FINALIZE_MIN_T default 1.4e-07, 1: 1.4e-07
On the MI355X every test of this file takes under 0.1 s."""
import numpy as np
import pytest

from oracle import nnops
from tests.test_path_parity import eng, grads_close, kink_free_params, knob, run_fwd_bwd   # noqa: F401  (eng, knob: fixtures)

BWD_TOL = 5e-5       # of each output's largest magnitude: the bound of test_instnorm_backward_modes
FIN_TOL = 2e-5       # TOL of test_kernels_parity.py

# (N, H, W, C) and the boundary each stands for
BWD_SHAPES = [
    (1, 3, 5, 4),        # one thread per pixel
    (2, 13, 11, 16),
    (3, 9, 7, 24),       # C not a power of two and 1024 % C != 0: no fixed channel quad per thread, cmask = -1
    (5, 17, 9, 32),
    (2, 12, 11, 64),
    (1, 9, 15, 96),
    (2, 5, 13, 128),
    (1, 4, 9, 256),      # C at the limit: two record lanes, one lane per channel in in_bwd_params_kernel
    (16, 5, 7, 16),      # one lane per sample in in_bwd_final_all_kernel
    (17, 5, 7, 8),       # N > 16: the per-sample final reduce + the nparams tail of the apply kernel
    (2, 37, 41, 16),     # 12 chunks per sample, ragged last chunk
    (1, 1, 130, 12),     # a one-pixel tail chunk
    (2, 19, 17, 3),      # C % 4 != 0: the scalar kernels
    (17, 6, 5, 3),
    (1, 67, 64, 64),     # with FS_INBWD_APPLY_WGS=1: the 64-channel width walks 67 batches of 1024 float4
]
BWD_KNOBS = {
    "defaults": {},
    "rec0": {"FS_INBWD_REC": 0},
    "rec0_chunk64": {"FS_INBWD_REC": 0, "FS_INBWD_CHUNK": 64},
    "maxt2_punr4": {"FS_INBWD_REC_MAXT": 2, "FS_INBWD_PUNR": 4},
    "apply_wgs1": {"FS_INBWD_APPLY_WGS": 1},     # one workgroup per sample: (2, 37, 41, 16) walks six batches of 1024 float4, the last one ragged
}

_bwd_problems = {}


def bwd_problem(shape, edge=False):
    """Inputs and the float64 results of one shape, all three modes; computed once, shared read-only.  edge: channel 0 of z almost flat around 200
    (std 1e-3: rstd ~ 1 / sqrt(eps)), channel 1 with one spike of 1e3.
    The activation derivative is taken at v = z * a + b with the float32 a, b that are passed, evaluated in float64 -- the operation the kernel is given
    (for the rectifier v > 0 is then the kernel's own decision: fmaf rounds once and keeps the sign) --, with z nudged off the ReLU kink first."""
    key = (shape, edge)
    if key in _bwd_problems:
        return _bwd_problems[key]
    rng = np.random.default_rng(3)
    N, H, W, C = shape
    z = rng.standard_normal(shape).astype(np.float32) * 2 + 0.5
    if edge:
        z[..., 0] = (200.0 + 1e-3 * rng.standard_normal((N, H, W))).astype(np.float32)
        z[0, H // 2, W // 3, 1] = 1e3
    gamma = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(C)).astype(np.float32)
    g64, b64 = gamma.astype(np.float64), beta.astype(np.float64)
    n64, _ = nnops.inst_norm(z.astype(np.float64), g64, b64)
    sd = z.astype(np.float64).std(axis=(1, 2), keepdims=True)
    z = np.where(np.abs(n64) < 1e-3, z + 0.025 * sd, z).astype(np.float32)     # (0.025 of the channel's spread: the statistics barely move)
    z64 = z.astype(np.float64)
    _, cache = nnops.inst_norm(z64, g64, b64)
    rstd = cache[1][:, 0, 0, :]
    mean = z64.mean(axis=(1, 2))
    a64 = g64 * rstd
    a, b = a64.astype(np.float32), (b64 - mean * a64).astype(np.float32)
    v = z64 * a.astype(np.float64)[:, None, None, :] + b.astype(np.float64)[:, None, None, :]
    assert np.abs(v).min() > 1e-6, "a pre-activation sits on the ReLU kink: pick another seed"
    gin = rng.standard_normal(shape).astype(np.float32)
    # xhat likewise from the float32 mean and rstd that are passed: they are inputs of the operation, and around 200 a float32 mean is only good to
    # 7.6e-6 -- times rstd ~ 31.6 a common shift of 2.4e-4 in the flat channel's xhat, 7e-5 of the largest dgamma, which no kernel could take back
    mean32, rstd32 = mean.astype(np.float32), rstd.astype(np.float32)
    cache = ((z64 - mean32.astype(np.float64)[:, None, None, :]) * rstd32.astype(np.float64)[:, None, None, :], rstd32.astype(np.float64)[:, None, None, :], g64)
    want = {}
    for mode in (0, 1, 2):
        dn = gin.astype(np.float64)
        if mode == 1:
            dn = dn * (v > 0)
        elif mode == 2:
            dn = nnops.scaled_tanh_bwd(dn, v)
        want[mode] = nnops.inst_norm_bwd(dn, cache)
    pb = dict(z=z, gin=gin, mean=mean32, rstd=rstd32, a=a, b=b, want=want)
    _bwd_problems[key] = pb
    return pb


def run_bwd(eng, pb, mode):
    up = eng.mem.from_numpy
    out = eng.instnorm_bwd(up(pb["gin"]), up(pb["z"]), up(pb["mean"]), up(pb["rstd"]), up(pb["a"]), up(pb["b"]), mode)
    return [np.array(eng.mem.to_numpy(t)) for t in out]


def bwd_errors(got, want):
    return [np.abs(g - w).max() / np.abs(w).max() for g, w in zip(got, want)]


@pytest.mark.parametrize("knobs", list(BWD_KNOBS))
def test_instnorm_backward_every_form_against_float64(eng, knob, knobs):
    """fs_instnorm_bwd over BWD_SHAPES x {linear, ReLU, scaled tanh} under one knob set: dz, dgamma and dbeta within 5e-5 of each output's largest
    magnitude of oracle.nnops.inst_norm_bwd in float64 (HW = 1 is left out: its exact result is identically zero).  Measured: the module docstring."""
    for k, v in BWD_KNOBS[knobs].items():
        knob(k, v)
    worst, bad = 0.0, []
    for shape in BWD_SHAPES:
        pb = bwd_problem(shape)
        for mode in (0, 1, 2):
            errs = bwd_errors(run_bwd(eng, pb, mode), pb["want"][mode])
            worst = max(worst, max(errs))
            if not max(errs) < BWD_TOL:      # (not <: a NaN fails)
                bad.append((shape, mode, errs))
    print("instance-norm backward, %s: worst error %.2e of the output's largest magnitude over %d shapes x 3 modes" % (knobs, worst, len(BWD_SHAPES)))
    assert bad == []


@pytest.mark.parametrize("knobs", list(BWD_KNOBS))
def test_instnorm_backward_flat_channel_and_spike(eng, knob, knobs):
    """(2, 12, 11, 64) with channel 0 almost flat around 200 (std 1e-3: rstd ~ 31, b ~ -6000, z * a + b cancels six digits) and one spike of 1e3 in
    channel 1: the same bound."""
    for k, v in BWD_KNOBS[knobs].items():
        knob(k, v)
    pb = bwd_problem((2, 12, 11, 64), edge=True)
    assert pb["rstd"][:, 0].min() > 30 and np.abs(pb["z"][..., 1]).max() == 1e3
    worst, bad = 0.0, []
    for mode in (0, 1, 2):
        errs = bwd_errors(run_bwd(eng, pb, mode), pb["want"][mode])
        worst = max(worst, max(errs))
        if not max(errs) < BWD_TOL:
            bad.append((mode, errs))
    print("instance-norm backward, flat channel + spike, %s: worst error %.2e" % (knobs, worst))
    assert bad == []


def test_instnorm_backward_span_of_a_workgroup_changes_no_bit(eng, knob):
    """FS_INBWD_APPLY_WGS=1 (one workgroup walks a whole sample in batches) against the default (one batch per workgroup at these sizes): the record
    order and the per-element arithmetic do not depend on the span, so dz, dgamma and dbeta are the same bits."""
    ref = {(shape, mode): run_bwd(eng, bwd_problem(shape), mode) for shape in BWD_SHAPES for mode in (0, 1, 2)}
    knob("FS_INBWD_APPLY_WGS", 1)
    bad = []
    for (shape, mode), want in ref.items():
        got = run_bwd(eng, bwd_problem(shape), mode)
        if not all(np.array_equal(g, w) for g, w in zip(got, want)):
            bad.append((shape, mode))
    assert bad == []


@pytest.mark.parametrize("knobs", [{"FS_INBWD_REC": 0},
                                   {"FS_INBWD_FUSED": 0},                                   # the records come from in_bwd_partial4_kernel, not from the Winograd epilogue
                                   {"FS_INBWD_APPLY_WGS": 1, "FS_INBWD_REC_MAXT": 2}],
                         ids=["rec0", "fused0", "apply_wgs1_maxt2"])
def test_tnet_backward_through_the_other_instnorm_backward_forms(eng, knob, knobs):
    """The whole net at (1, 45, 67) with the instance-norm backward in its three-launch form, with records from a pass of its own, and with one apply
    workgroup per sample over two records: the unchanged tolerances of test_path_parity.py (forward 2e-5 of the pixel range, 2e-4 per gradient tensor)."""
    for k, v in knobs.items():
        knob(k, v)
    y, yo, g, want = run_fwd_bwd(eng, kink_free_params(), (1, 45, 67), seed=0)
    assert np.abs(y - yo).max() / 255.0 < 2e-5
    assert grads_close(eng, g, want, 2e-4) == []


# ----------------------------------------------------------------------------- fs_instnorm_finalize on synthetic records
# (N, T, C, groups): one tile; a few; T around kFinalizeSplit = 64 (63 / 65, 64 with four groups); the 256-lane instance (N * C <= 512 and
# T * groups >= 256: (1, 300, 16, 1), (1, 64, 32, 4), (2, 67, 16, 4), (1, 257, 64, 1), (1, 1030, 8, 1), (1, 66, 128, 4)); the scalar-width C = 3;
# four groups with Cv = 256 and with Cv = 512 (beyond what the pre-reduction takes)
FIN_CASES = [(1, 1, 3, 1), (2, 5, 16, 1), (3, 63, 64, 1), (2, 65, 64, 1), (1, 300, 16, 1), (1, 64, 32, 4), (2, 67, 16, 4), (1, 257, 64, 1),
             (5, 70, 3, 1), (1, 1030, 8, 1), (2, 130, 64, 4), (1, 66, 128, 4)]


def finalize_problem(case, zeros, offset):
    """Records [N][T][C * groups][3] = {mean, M2, count} and the pooled float64 result.  Counts are integers 1..256, one per (tile, group) as a conv
    writes them (ragged between the groups); zeros: every third record (t * groups + q = 1 mod 3) has count 0 and must be skipped."""
    N, T, C, groups = case
    rng = np.random.default_rng(7)
    cnt = rng.integers(1, 257, (N, T, groups)).astype(np.float64)
    if zeros:
        cnt[:, (np.arange(T * groups) % 3 == 1).reshape(T, groups)] = 0
    cnt = np.repeat(cnt[:, :, :, None], C, axis=3)                                  # [N][T][groups][C]
    mu = (offset + 3 * rng.standard_normal((N, T, groups, C))).astype(np.float32)
    m2 = (2 * cnt * np.abs(rng.standard_normal((N, T, groups, C)))).astype(np.float32)
    stats = np.stack([mu, m2, cnt.astype(np.float32)], axis=-1).reshape(N, T, groups * C, 3)    # record (t, q) of channel c at q * C + c
    gamma = (1 + 0.3 * rng.standard_normal(C)).astype(np.float32)
    beta = (0.3 * rng.standard_normal(C)).astype(np.float32)
    mu64, m264 = mu.astype(np.float64), m2.astype(np.float64)
    total = cnt.sum(axis=(1, 2))
    mean = (cnt * mu64).sum(axis=(1, 2)) / total
    var = (m264 * (cnt > 0) + cnt * np.square(mu64 - mean[:, None, None, :])).sum(axis=(1, 2)) / total
    rstd = 1.0 / np.sqrt(var + 1e-3)
    a = gamma.astype(np.float64) * rstd
    return stats, gamma, beta, (mean, rstd, a, beta.astype(np.float64) - mean * a)


@pytest.mark.parametrize("min_t", [None, 1], ids=["min_t_default", "min_t_1"])
def test_instnorm_finalize_on_synthetic_records(eng, knob, min_t):
    """fs_instnorm_finalize over FIN_CASES x {no empty records, every third one empty} x {means around 0, around 1000}: mean, rstd, a and b within 2e-5
    of each output's largest magnitude of the pooled mean / biased variance in float64.  Both values of FS_FINALIZE_MIN_T run; the entry point hands
    in_finalize no scratch, so its pre-reduction launch stays with the whole-net test (test_tnet_forward_with_two_level_statistics_merge) and what the
    knob must show here is that it changes nothing.  Measured: the module docstring."""
    if min_t is not None:
        knob("FS_FINALIZE_MIN_T", min_t)
    up = eng.mem.from_numpy
    worst, bad = 0.0, []
    for case in FIN_CASES:
        for zeros in (False, True):
            for offset in (0.0, 1000.0):
                stats, gamma, beta, want = finalize_problem(case, zeros, offset)
                N, T, C, groups = case
                got = eng.instnorm_finalize(up(stats), T, C, groups, up(gamma), up(beta))
                errs = [np.abs(eng.mem.to_numpy(g) - w).max() / np.abs(w).max() for g, w in zip(got, want)]
                worst = max(worst, max(errs))
                if not max(errs) < FIN_TOL:
                    bad.append((case, zeros, offset, errs))
    print("instance-norm finalize, FS_FINALIZE_MIN_T %s: worst error %.2e of the output's largest magnitude over %d record sets" % (
        "default" if min_t is None else min_t, worst, 4 * len(FIN_CASES)))
    assert bad == []
