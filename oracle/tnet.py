"""Image-transform net: numpy restatement of reference im_transf_net.py (test oracle).

``create_net`` follows im_transf_net.py:14-75 line by line in the AS-WRITTEN form
(materialised x4 nearest upsample followed by a 3x3 stride-2 conv, unfused instance norm).
Parameters are a dict keyed like the checkpoint minus the ``img_t_net/`` scope prefix:
``initconv_0/W``, ``resblock_3/INscale2`` ....
"""
from collections import OrderedDict

import numpy as np

from . import nnops as F

# (name, kind, k, cin, cout) in network order -- im_transf_net.py:37-70
LAYERS = [("initconv_0", "conv", 9, 3, 16), ("initconv_1", "conv", 3, 16, 32),
          ("initconv_2", "conv", 3, 32, 64)] + \
         [("resblock_%d" % i, "res", 3, 64, 64) for i in range(5)] + \
         [("upsample_0", "up", 3, 64, 32), ("upsample_1", "up", 3, 32, 16),
          ("upsample_2", "conv", 9, 16, 3)]


def param_shapes(upsample_method="resize"):
    """name -> shape for the 48 variables, in sorted (= checkpoint) order."""
    out = {}
    for name, kind, k, ci, co in LAYERS:
        if kind == "res":
            for s in ("1", "2"):
                out[name + "/INscale" + s] = (co,)
                out[name + "/INshift" + s] = (co,)
                out[name + "/W" + s] = (k, k, ci, co)
        else:
            out[name + "/INscale"] = (co,)
            out[name + "/INshift"] = (co,)
            # deconv2d stores its filter as [k,k,Cout,Cin] (im_transf_net.py:174)
            tr = upsample_method == "deconv" and name.startswith("upsample")
            out[name + "/W"] = (k, k, co, ci) if tr else (k, k, ci, co)
    return OrderedDict(sorted(out.items()))


def init_params(seed=0, upsample_method="resize", dtype=np.float32):
    """Initialisers of the reference: conv2d N(0,0.1) (im_transf_net.py:114), upconv2d /
    deconv2d N(0,1) (:149,:180), INscale=1, INshift=0 (:233-236).  (Distribution only --
    TF's RNG stream is not reproducible outside TF.)"""
    rng = np.random.default_rng(seed)
    p = OrderedDict()
    for name, shape in param_shapes(upsample_method).items():
        leaf = name.split("/")[1]
        if leaf.startswith("INscale"):
            p[name] = np.ones(shape, dtype)
        elif leaf.startswith("INshift"):
            p[name] = np.zeros(shape, dtype)
        else:
            layer = name.split("/")[0]
            std = 1.0 if layer in ("upsample_0", "upsample_1") else 0.1
            if upsample_method == "deconv" and layer == "upsample_2":
                std = 1.0
            p[name] = (rng.standard_normal(shape) * std).astype(dtype)
    return p


def out_shape(H, W):
    """Output H,W of create_net for an HxW input:
    4*(ceil(ceil((H+80)/2)/2) - 20)."""
    f = lambda s: 4 * (-(-(-(-(s + 80) // 2)) // 2) - 20)
    return f(H), f(W)


def upconv2d(x, w):
    """im_transf_net.py:122-155: resize x(stride**2)=x4 NEAREST, then conv3x3 stride 2 SAME."""
    return F.conv2d(F.resize_nearest(x, 4), w, stride=2, padding="SAME")


def create_net(x, params, upsample_method="resize", keep=False):
    """Forward of im_transf_net.create_net (im_transf_net.py:14-75).

    x: [N,H,W,3] float (RGB 0..255, not mean-subtracted).  Returns y, or (y, cache) with
    everything the backward needs when ``keep``.
    """
    assert upsample_method in ("deconv", "resize")       # im_transf_net.py:28
    P = params
    c = {"x_shape": x.shape, "method": upsample_method}
    acts = {}                                            # named intermediates (for tests)
    h = F.reflect_pad(x, 40)                             # :34
    strides = {"initconv_0": 1, "initconv_1": 2, "initconv_2": 2}
    for name in ("initconv_0", "initconv_1", "initconv_2"):   # :37-42
        c[name + "/in"] = h
        z = F.conv2d(h, P[name + "/W"], strides[name], "SAME")
        n, c[name + "/in_cache"] = F.inst_norm(z, P[name + "/INscale"], P[name + "/INshift"])
        c[name + "/n"] = n
        h = F.relu(n)
        acts[name] = h
    for i in range(5):                                   # :45-54, res_layer :250-276
        name = "resblock_%d" % i
        c[name + "/in"] = h
        z1 = F.conv2d(h, P[name + "/W1"], 1, "VALID")
        n1, c[name + "/in_cache1"] = F.inst_norm(z1, P[name + "/INscale1"], P[name + "/INshift1"])
        c[name + "/n1"] = n1
        a1 = F.relu(n1)
        c[name + "/a1"] = a1
        z2 = F.conv2d(a1, P[name + "/W2"], 1, "VALID")
        n2, c[name + "/in_cache2"] = F.inst_norm(z2, P[name + "/INscale2"], P[name + "/INshift2"])
        h = n2 + h[:, 2:-2, 2:-2, :]                      # :268-274 (no ReLU after the add)
        acts[name] = h
    for name in ("upsample_0", "upsample_1"):            # :57-68
        c[name + "/in"] = h
        if upsample_method == "resize":
            z = upconv2d(h, P[name + "/W"])
        else:
            z = F.conv2d_transpose(h, P[name + "/W"], 2)
        n, c[name + "/in_cache"] = F.inst_norm(z, P[name + "/INscale"], P[name + "/INshift"])
        c[name + "/n"] = n
        h = F.relu(n)
        acts[name] = h
    name = "upsample_2"                                  # :62-63 / :69-70
    c[name + "/in"] = h
    if upsample_method == "resize":
        z = F.conv2d(h, P[name + "/W"], 1, "SAME")
    else:
        z = F.conv2d_transpose(h, P[name + "/W"], 1)
    n, c[name + "/in_cache"] = F.inst_norm(z, P[name + "/INscale"], P[name + "/INshift"])
    c[name + "/n"] = n
    y = F.scaled_tanh(n)                                 # :202-215
    acts[name] = y
    c["acts"] = acts
    return (y, c) if keep else y


def create_net_bwd(dy, params, cache, masks=None):
    """Gradients of create_net wrt its 48 parameters, given dL/dy.  Returns a dict with
    the same keys as ``params`` (the input image gets no gradient in train.py).

    ``masks`` (tests only): boolean ReLU masks of the ten rectified units taken from another evaluation of the same forward
    (keys ``initconv_0..2``, ``resblock_k`` for the ReLU between a block's two convs, ``upsample_0..1``) instead of this
    evaluation's own sign pattern -- see perceptual.vgg16_bwd."""
    P, c = params, cache
    masks = masks or {}
    deconv = c["method"] == "deconv"
    g = {}
    name = "upsample_2"
    dn = F.scaled_tanh_bwd(dy, c[name + "/n"])
    dz, g[name + "/INscale"], g[name + "/INshift"] = F.inst_norm_bwd(dn, c[name + "/in_cache"])
    if deconv:
        # y = conv2d_transpose(x, W) is the input-gradient of conv2d(., W): its adjoints are
        # dx = conv2d(dy, W) and dW = conv2d_bwd_filter(input=dy, grad=x)
        g[name + "/W"] = F.conv2d_bwd_filter(dz, c[name + "/in"], 9, 1, "SAME")
        dh = F.conv2d(dz, P[name + "/W"], 1, "SAME")
    else:
        g[name + "/W"] = F.conv2d_bwd_filter(c[name + "/in"], dz, 9, 1, "SAME")
        dh = F.conv2d_bwd_input(dz, P[name + "/W"], c[name + "/in"].shape[1:3], 1, "SAME")
    for name in ("upsample_1", "upsample_0"):
        dn = dh * masks.get(name, c[name + "/n"] > 0)
        dz, g[name + "/INscale"], g[name + "/INshift"] = F.inst_norm_bwd(dn, c[name + "/in_cache"])
        if deconv:
            g[name + "/W"] = F.conv2d_bwd_filter(dz, c[name + "/in"], 3, 2, "SAME")
            dh = F.conv2d(dz, P[name + "/W"], 2, "SAME")
            continue
        up = F.resize_nearest(c[name + "/in"], 4)
        g[name + "/W"] = F.conv2d_bwd_filter(up, dz, 3, 2, "SAME")
        dup = F.conv2d_bwd_input(dz, P[name + "/W"], up.shape[1:3], 2, "SAME")
        dh = F.resize_nearest_bwd(dup, 4)
    for i in reversed(range(5)):
        name = "resblock_%d" % i
        dz2, g[name + "/INscale2"], g[name + "/INshift2"] = F.inst_norm_bwd(dh, c[name + "/in_cache2"])
        g[name + "/W2"] = F.conv2d_bwd_filter(c[name + "/a1"], dz2, 3, 1, "VALID")
        da1 = F.conv2d_bwd_input(dz2, P[name + "/W2"], c[name + "/a1"].shape[1:3], 1, "VALID")
        dn1 = da1 * masks.get(name, c[name + "/n1"] > 0)
        dz1, g[name + "/INscale1"], g[name + "/INshift1"] = F.inst_norm_bwd(dn1, c[name + "/in_cache1"])
        g[name + "/W1"] = F.conv2d_bwd_filter(c[name + "/in"], dz1, 3, 1, "VALID")
        dskip = np.pad(dh, ((0, 0), (2, 2), (2, 2), (0, 0)))
        dh = F.conv2d_bwd_input(dz1, P[name + "/W1"], c[name + "/in"].shape[1:3], 1, "VALID") + dskip
    strides = {"initconv_0": 1, "initconv_1": 2, "initconv_2": 2}
    for name in ("initconv_2", "initconv_1", "initconv_0"):
        k = 9 if name == "initconv_0" else 3
        dn = dh * masks.get(name, c[name + "/n"] > 0)
        dz, g[name + "/INscale"], g[name + "/INshift"] = F.inst_norm_bwd(dn, c[name + "/in_cache"])
        g[name + "/W"] = F.conv2d_bwd_filter(c[name + "/in"], dz, k, strides[name], "SAME")
        if name != "initconv_0":
            dh = F.conv2d_bwd_input(dz, P[name + "/W"], c[name + "/in"].shape[1:3], strides[name], "SAME")
    return OrderedDict((k, g[k]) for k in params)


def strip_scope(tensors, scope="img_t_net/"):
    """Checkpoint names -> oracle names (drops the variable_scope prefix used at
    stylize_image.py:63 / train.py:159)."""
    return OrderedDict((k[len(scope):], v) for k, v in tensors.items() if k.startswith(scope))


# ---------------------------------------------------------------------- bf16 mixed-precision restatement
def bf16_round(x):
    """float -> nearest bfloat16 (ties to even), returned as float32/float64 of the same shape."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(a.shape)


def bf16_bits(x):
    """float -> the 16-bit pattern of the nearest bfloat16 (uint16)."""
    return (bf16_round(x).view(np.uint32) >> 16).astype(np.uint16)


def bf16_from_bits(u):
    """uint16 bfloat16 patterns -> float64 values."""
    return (np.ascontiguousarray(u, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _r(t):
    return bf16_round(t).astype(np.float64)


# The sixteen conv + instance-norm units of the HIP path (fs_tnet.h: Unit) in launch order:
# (filter, INscale, INshift, kind, stride, padding); kind "up" = phase-collapsed resize-conv, "fold" = kw-folded output layer.
BF16_UNITS = [("initconv_0/W", "initconv_0/INscale", "initconv_0/INshift", "conv", 1, "SAME"),
              ("initconv_1/W", "initconv_1/INscale", "initconv_1/INshift", "conv", 2, "SAME"),
              ("initconv_2/W", "initconv_2/INscale", "initconv_2/INshift", "conv", 2, "SAME")] + \
             [("resblock_%d/W%s" % (k, s), "resblock_%d/INscale%s" % (k, s), "resblock_%d/INshift%s" % (k, s), "conv", 1, "VALID")
              for k in range(5) for s in ("1", "2")] + \
             [("upsample_0/W", "upsample_0/INscale", "upsample_0/INshift", "up", 1, None),
              ("upsample_1/W", "upsample_1/INscale", "upsample_1/INshift", "up", 1, None),
              ("upsample_2/W", "upsample_2/INscale", "upsample_2/INshift", "fold", 1, None)]

_UP_R = {(0, 0): (0, 1, 2), (0, 1): (), (1, 0): (0, 1), (1, 1): (2,)}      # (phase, tap) -> source rows/cols of the 3x3 filter


def bf16_upconv_weff(w):
    """The phase-collapsed resize-conv filter [2,2,Ci,4,Co] (tap dy, dx; phase q = 2a + b) as pack_bf16_kernel forms it (PK_UP): float32 sums of the
    3x3 filter's terms in kh, kw order, NOT yet rounded to bfloat16."""
    w = np.asarray(w).astype(np.float32)
    ci, co = w.shape[2], w.shape[3]
    weff = np.zeros((2, 2, ci, 4, co), np.float32)
    for pa in range(2):
        for dy in range(2):
            for pb in range(2):
                for dx in range(2):
                    acc = np.zeros((ci, co), np.float32)
                    for kh in range(3):
                        for kw in range(3):
                            if kh in _UP_R[(pa, dy)] and kw in _UP_R[(pb, dx)]:
                                acc = acc + w[kh, kw]
                    weff[dy, dx, :, pa * 2 + pb, :] = acc
    return weff


def bf16_fold_filter(w):
    """The kw-folded form of the 9x9, Ci -> 3 output layer (fs_fold.hip: kw = 5b + v): [9,2,Ci,16], column j = 3v + co, zero for j = 15 and kw >= 9."""
    w = np.asarray(w)
    wf = np.zeros((9, 2, w.shape[2], 16), w.dtype)
    for b in range(2):
        for v in range(5):
            if 5 * b + v < 9:
                wf[:, b, :, 3 * v:3 * v + 3] = w[:, 5 * b + v]
    return wf


def bf16_packed_filter(i, params, cout_pad):
    """uint16 restatement of what pack_bf16_kernel (fs_bf16.hip) writes for unit i: PK_C4 [9][cout_pad][48] (k = 4 kw + ci) for the image layer, PK_UP
    [4][cout_pad][Ci], PK_FOLD [18][cout_pad][Ci], PK_CONV [KH*KW][cout_pad][Ci]; zero wherever the layout pads."""
    wkey, _, _, kind, _, _ = BF16_UNITS[i]
    w = np.asarray(params[wkey]).astype(np.float32)
    if i == 0:
        kh, kw, ci, co = w.shape
        out = np.zeros((kh, cout_pad, 12, 4), np.float32)
        out[:, :co, :kw, :ci] = w.transpose(0, 3, 1, 2)
        return bf16_bits(out.reshape(kh, cout_pad, 48))
    if kind == "up":
        weff = bf16_upconv_weff(w)                                     # [2,2,ci,4,co]
        g = weff.reshape(4, w.shape[2], 4 * w.shape[3])
    elif kind == "fold":
        g = bf16_fold_filter(w).reshape(18, w.shape[2], 16)
    else:
        g = w.reshape(w.shape[0] * w.shape[1], w.shape[2], w.shape[3])
    out = np.zeros((g.shape[0], cout_pad, g.shape[1]), np.float32)
    out[:, :g.shape[2], :] = g.transpose(0, 2, 1)
    return bf16_bits(out)


def bf16_stage(src, a=None, b=None, relu=True):
    """What a conv kernel of the bf16 path stages for a stored tensor `src` (bfloat16 values): relu(fmaf(x, a, b)) in float32, then bfloat16 -- or
    `src` itself where the producer left no instance norm to apply (a is None: the image, a residual sum).  a, b: per-sample constants [N,C] or
    [N,1,1,C].  (Evaluated in float64 and rounded to float32: with float32 a, b the product is exact and the sum is rounded twice, which differs from
    the fused multiply-add only on a 2^-29 tie.)"""
    x = np.asarray(src, np.float64)
    if a is None:
        return _r(x)
    a, b = (np.asarray(t, np.float64).reshape(x.shape[0], 1, 1, x.shape[3]) for t in (a, b))
    v = a * x + b
    return _r(np.maximum(v, 0.0) if relu else v)


def bf16_unit(i, src, params, a=None, b=None, want_S=True):
    """Unit i of the bf16 path on a TEACHER-FORCED input: `src` is the stored tensor the unit reads (the image for unit 0, otherwise bfloat16 values: a
    raw conv output z with its per-sample a, b, or a residual sum with a = b = None).  Returns
      xs     the staged conv input (bf16_stage; unit 0: the REFLECT-40 padded image rounded to bfloat16),
      z_ref  the float64, unrounded conv of xs with the bfloat16 filter, in the order the unit STORES it: [N,Ho,Wo,C]; the resize-convs pixel-shuffled
             [N,2H,2W,C]; the output layer as its 16 kw-folded virtual channels [N,Ho,Wo+4,16] (fs_fold.hip),
      S      the same conv of |xs| with |filter| (None unless want_S): the scale of the accumulation error."""
    wkey, _, _, kind, stride, padding = BF16_UNITS[i]
    w = np.asarray(params[wkey], np.float64)
    if i == 0:
        xs = _r(F.reflect_pad(np.asarray(src, np.float64), 40))                  # image pixels -> bf16
    else:
        xs = bf16_stage(src, a, b)
    if kind == "conv":
        wq = _r(w)
        conv = lambda t, f: F.conv2d(t, f, stride, padding)
    elif kind == "up":
        ci, co = w.shape[2], w.shape[3]
        wq = _r(bf16_upconv_weff(w).reshape(2, 2, ci, 4 * co))

        def conv(t, f):
            zc = F.conv2d(np.pad(t, ((0, 0), (0, 1), (0, 1), (0, 0))), f, 1, "VALID")     # [N,H,W,4*co]
            N, Hh, Ww, _ = zc.shape
            return zc.reshape(N, Hh, Ww, 2, 2, co).transpose(0, 1, 3, 2, 4, 5).reshape(N, 2 * Hh, 2 * Ww, co)
    else:
        # Z[q,(v,co)] = sum_{kh,b,ci} X[q + (kh, 5b) - 4, ci] W[kh, 5b+v, ci, co] for q in [0, Wo+4): as a 9x9 conv whose filter holds, for virtual
        # channel (v, co), the taps kw in {v, 5+v} only, evaluated at p = q - v
        wf = _r(w)
        wq = np.zeros(wf.shape[:3] + (15,), np.float64)
        for v in range(5):
            for kw in (v, 5 + v):
                if kw < 9:
                    wq[:, kw, :, 3 * v:3 * v + 3] = wf[:, kw]

        def conv(t, f):
            o = F.conv2d(np.pad(t, ((0, 0), (0, 0), (4, 4), (0, 0))), f, 1, "SAME")        # [N,H,W+8,15], column p + 4
            N, Hh, W8, _ = o.shape
            Z = np.zeros((N, Hh, W8 - 4, 16), np.float64)
            for v in range(5):
                Z[..., 3 * v:3 * v + 3] = o[:, :, 4 - v:W8 - v, 3 * v:3 * v + 3]
            return Z
    z_ref = conv(xs, wq)
    S = conv(np.abs(xs), np.abs(wq)) if want_S else None
    return xs, z_ref, S


def bf16_fold5(Z):
    """z[n,y,x,co] = sum_v Z[n,y,x+v,(v,co)] (fs_fold.hip) of the STORED (bfloat16) virtual channels, v ascending."""
    Wo = Z.shape[2] - 4
    z = 0.0
    for v in range(5):
        z = z + Z[:, :, v:v + Wo, 3 * v:3 * v + 3]
    return z


def bf16_norm_consts(z, gamma, beta):
    """float64 (mean, rstd, a, b), each [N,1,1,C], of an instance norm over z: a = gamma * rstd, b = beta - mean * a (im_transf_net.py:238-245)."""
    mean = z.mean(axis=(1, 2), keepdims=True)
    var = z.var(axis=(1, 2), keepdims=True)
    a = gamma / np.sqrt(var + 1e-3)
    return mean, 1.0 / np.sqrt(var + 1e-3), a, beta - mean * a


def bf16_residual(z, a, b, skip, sa=None, sb=None):
    """What apply_res_bf16_kernel rounds to bfloat16: fmaf(z, a, b) + T(skip)[y+2, x+2] in float64, UNROUNDED; T = relu(sa * skip + sb) for block 0
    (the skip is the raw third conv output) and the identity behind it.  z, skip: stored bfloat16 values."""
    z, skip = np.asarray(z, np.float64), np.asarray(skip, np.float64)
    shp = (z.shape[0], 1, 1, z.shape[3])
    if sa is not None:
        skip = np.maximum(np.asarray(sa, np.float64).reshape(shp) * skip + np.asarray(sb, np.float64).reshape(shp), 0.0)
    return np.asarray(a, np.float64).reshape(shp) * z + np.asarray(b, np.float64).reshape(shp) + skip[:, 2:-2, 2:-2, :]


def create_net_bf16(x, params):
    """create_net ('resize') with the rounding points of the HIP mixed-precision inference path
    (fs_bf16.hip, FS_FLAG_BF16): weights, the image, every conv input (after the producer's
    instance-norm + ReLU) and every stored activation are bfloat16; accumulation, instance-norm
    statistics (taken before the output is rounded), the last instance norm and the tanh are full
    precision.  The resize-conv is evaluated in its phase-collapsed form because
    the kernel rounds the COLLAPSED filter.  Composed of the per-unit pieces above, each fed the restatement's own previous result.
    Test infrastructure for the config-5 path only: the
    parity bar of the project (1e-3 of the pixel range) applies to the fp32 path, not to this one."""
    P = {k: np.asarray(v, np.float64) for k, v in params.items()}
    src, a, b = x, None, None
    skip = None
    for i in range(15):
        _, z, _ = bf16_unit(i, src, P, a, b, want_S=False)
        _, _, a, b = bf16_norm_consts(z, P[BF16_UNITS[i][1]], P[BF16_UNITS[i][2]])
        src = _r(z)                                                            # stored bf16
        if i == 2:
            skip = (src, a, b)                                                 # block 0 reads the raw initconv_2 output
        if 4 <= i <= 12 and i % 2 == 0:                                        # second conv of a residual block: h_k stored bf16
            src = _r(bf16_residual(src, a, b, *skip))
            skip = (src, None, None)
            a = b = None
    _, Z, _ = bf16_unit(15, src, P, a, b, want_S=False)
    z = bf16_fold5(_r(Z))                                                      # five partial sums, each stored as bf16
    n, _ = F.inst_norm(z, P["upsample_2/INscale"], P["upsample_2/INshift"])
    return F.scaled_tanh(n)
