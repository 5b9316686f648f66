#!/usr/bin/env python
"""Drop-in for the reference's stylize_webcam.py (same flags): filters an OpenCV webcam feed through
a trained model and writes output.avi, with the network on the MI355X (faststyle_amd/stream.py).

OpenCV (camera capture, window, XVID writer) is a host-side dependency of the reference that this
image does not ship; without it the script can still filter a *directory of frames*:
    python stylize_webcam.py --model_path models/starry_final.ckpt --frames_dir in/ --output_dir out/
(frames are read RGB with PIL and converted to the BGR order a cv2 capture would deliver, so the
reference's channel handling -- BGR fed as is, output swapped -- is reproduced bit for bit).
``--output_format jpg [--output_quality 95]`` writes <name>.jpg instead of <name>.png, encoded by the
library (faststyle_amd/stream.py, jpeg=): the bytes PIL would write for the pixels of the .png at that
quality, 4:2:0.  ``--frame_size W H`` resizes every frame on the device with cv2.resize's resampling (INTER_AREA shrinking,
INTER_CUBIC otherwise), and ``--input_decode native`` hands baseline .jpg frames to the library's decoder (Huffman pass on host
threads, reconstruction on the GPU) instead of PIL; the results are the same files.

Video without OpenCV: ``--video_in`` / ``--video_out`` read and write YUV4MPEG2 streams (faststyle_amd/y4m.py), the raw format ffmpeg, x264 and mpv
speak on pipes; ``-`` is standard input / output:
    ffmpeg -i in.mp4 -f yuv4mpegpipe - | python stylize_webcam.py --model_path m.ckpt --video_in - --video_out - | ffmpeg -i - out.mp4
    ffmpeg -f v4l2 -i /dev/video0 -f yuv4mpegpipe - | python stylize_webcam.py --model_path m.ckpt --video_in - --video_out - | ffplay -
Chroma resampling and the YCbCr <-> RGB matrix (``--video_matrix``, BT.601 by default) run on the device inside each lane's graph; the host reads a
frame's planes into pinned memory and writes the result's planes, nothing else.  The output stream has the input's frame rate, aspect, sampling,
siting and range at the net's output size.  ``--video_in`` without ``--video_out`` writes 000000.png, 000001.png ... (or .jpg) to --output_dir.
Deep video: ``--video_depth stream`` takes the stream at its own depth (C420p10, C422p10, C444p12 ... up to 16 bits; the default ``8`` refuses
them) and ``--video_out_depth N`` writes N bits (default: the input's); above 8 bits the planes go straight to and from the net's fp32 tensors,
without a u8 stage on that side.  ``--frame_size`` takes a deep input only with ``--frame_filter`` (below).

How much of the style lands: ``--style_strength S`` (0 the source, 1 the net's output) blends every stylized frame back towards its source,
``--preserve_color`` keeps the source's colours under the stylized luminance (``--color_matrix`` names the luma weights; the default is
--video_matrix with --video_in, else bt601), and ``--mask_path FILE`` (a grey image of the net's input size: 0 keeps the source pixel, 255
stylizes it) restricts either to a region -- one more launch inside each lane's graph, on the net's fp32 tensors (faststyle_amd/stream.py,
compose=), with every input and output flag above.  Without any of the four nothing changes; ``--style_strength 1`` alone writes the same bytes.

Less flicker: ``--temporal_strength S`` (0 nothing, 1 all of it) blends every frame towards the previous stabilised frame, fetched along
16 x 16 block motion vectors found between the two source frames (``--temporal_radius R``, 0..7 pixels) and only where the source matched
there (``--temporal_sensitivity K``, 1..256: nothing is blended at a luma difference of 256 / K) -- three more launches per frame, on the
net's fp32 tensors, behind the stage above (faststyle_amd/stream.py, temporal=).  The luma weights follow --color_matrix / --video_matrix.
With --frames_dir a change of frame size starts over.  Without the flag nothing changes; ``--temporal_strength 0`` writes the same bytes.
``--temporal_levels L`` (1..3, default 1) searches coarse to fine over L halved lumas for fast motion: vectors up to R (2^L - 1) pixels, found
reliably up to about R 2^(L-1) -- 14 at L = 2, 28 at L = 3 --, for one more launch and one more search launch per level.
``--temporal_subpel S`` (0..2, default 0) gives the vectors in whole, half or quarter pixels for slow motion -- a pan, a drifting handheld shot,
a zoom --: a fraction per block and a bilinear fetch of the previous frame, for one more launch; it combines with ``--temporal_levels``.
``--temporal_overlap 1`` (0..1, default 0) blends every pixel along the vectors of the four blocks whose centres surround it, weighted by a
bilinear window and by how well the source matched along each, so that a block that straddles a motion edge -- the outline of every moving
subject -- keeps its match on both sides; the same launches with another blend; it combines with ``--temporal_levels`` and ``--temporal_subpel``.

Deliver at any size: ``--output_size W H`` (or ``--output_size source``: the stream's or the first frame's own size) resamples every result
from the net's size to that size on the device -- Pillow's mode-F arithmetic on the net's fp32 output (or the blended / stabilised tensor),
``--output_filter`` box, bilinear, bicubic (default) or lanczos, one launch ahead of the output conversions (faststyle_amd/stream.py,
deliver=) -- so ``--frame_size 1280 720 --output_size source`` runs the net at 720p on a 2160p stream and writes 2160p.  The .png / .jpg
files, the YUV4MPEG2 header and deep outputs carry that size.  ``--frame_filter F`` lets ``--frame_size`` take a ``--video_depth stream`` input
of 9 to 16 bits: its fp32 frames are resampled to the net's size the same way (source resample=), with no u8 stage.

Edge-aware delivery: ``--output_guided`` (with ``--frame_size W H`` and an ``--output_size`` that is the source's, ``source`` for one) takes
the place of the resampling filter: a guided filter fits the stylized picture to the source's luma on the net's grid (``--guided_radius R``,
1..8, default 2: the window; ``--guided_smoothness E``, 1..64 8-bit levels, default 4) and applies the fit to the full-size source, which the
lane still holds, so that the source's edges return at the delivery resolution -- three launches in the place of one
(faststyle_amd/stream.py, deliver guided=).  The luma weights follow --color_matrix / --video_matrix.  Without the flag nothing changes.

Throughput: ``--video_batch N`` (1..64, with --video_in) sends N consecutive frames through the net per pass; with ``--temporal_strength`` the
stage runs over the N frames in order (faststyle_amd/stream.py, temporal sequence=), so the results are those of the same lanes fed one
frame at a time up to the net's own batch numerics.  A stream's last pass is padded by repeating its last frame and only the frames read
are written.  Latency grows by N frames, so live pipes keep 1.  ``--precision bf16`` runs the net's mixed-precision path (resize-conv models
only: not with --upsample_method deconv) with --frames_dir, --video_in and the camera.  Without the flags, or with ``--video_batch 1`` /
``--precision fp32``, nothing changes.

Several streams: ``--video_also IN OUT`` (repeatable, up to 63 times, with --video_in and --video_out) names one more YUV4MPEG2 stream of the
first one's size and format; every pass takes one frame of every open stream, so the net runs a batch without a frame of latency: eight
cameras or eight files in one process.  With ``--temporal_strength`` every stream is stabilised on its own, against its own previous frame
(faststyle_amd/stream.py, temporal streams=), in the launches of one stream.  A stream that ends or breaks off leaves the passes, its file
is closed complete and the others go on; the run ends with the last stream, and a stream that broke off is reported then.  Every other flag
applies to all streams alike (one mask, one --mix_fade weight per pass).  A pass waits for every open stream: live sources are not paced
against each other.  Not with --video_batch, --frames_dir or the camera; without the flag nothing changes.

Two styles: ``--model_path2 CKPT`` names a second model of the same --upsample_method; every frame goes through both nets and their fp32
outputs are mixed on the device, one launch ahead of every stage above (faststyle_amd/stream.py, mix=).  ``--style_mix T`` (0..1, default 1)
is the share of the second model, ``--mix_mask FILE`` (a grey image of the net's input size: 0 shows --model_path, 255 the mix) puts one style
on a region and the other around it, and ``--mix_fade F0 F1`` cross-fades over the 0-based frames F0..F1 of --frames_dir or --video_in: frame
n has the weight T min(max(n - F0, 0), F1 - F0) / (F1 - F0), in 256ths, rounded half up.  A model nobody will see is not run: before and
after a fade the frames cost one forward pass and are, byte for byte, those of the run with that model alone (8-bit outputs; deep outputs
are that model's on the 8.8 grid).  --model_path2 needs one of the three, and each of them needs it.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def setup_parser():
    """The reference flag surface (stylize_webcam.py:17-39) plus --frames_dir/--output_dir, in faststyle_amd/cli.py."""
    from faststyle_amd import cli
    return cli.stylize_webcam_parser()


def _load(args):
    from faststyle_amd import ckpt, engine
    eng = engine.Engine()
    variables = eng.mem.from_numpy(eng.flatten_params(ckpt.load_checkpoint(args.model_path),
                                                      upsample_method=args.upsample_method))
    return eng, variables


def compose_options(args, matrix='bt601'):
    """--style_strength / --preserve_color / --color_matrix / --mask_path -> the compose= dict of the lanes (faststyle_amd/stream.py), None when
    none of them is given; matrix: what --color_matrix defaults to.  A strength outside [0, 1] or an unreadable mask is a SystemExit here,
    before anything is loaded.  Every path of this script feeds the net B,G,R and shows its output as R,G,B (the reference's channel
    handling, kept as it is): the stage is told so (source_swapped) and the source shows through in its own colours; the lanes of a run with
    the stage do not swap on the way out, and the host swaps where a lane without it would have."""
    if args.style_strength is None and not args.preserve_color and args.color_matrix is None and args.mask_path is None:
        return None
    s = 1.0 if args.style_strength is None else args.style_strength
    if not 0.0 <= s <= 1.0:
        raise SystemExit('--style_strength %r is outside [0, 1]' % s)
    opt = dict(strength=s, keep_color=args.preserve_color, matrix=args.color_matrix or matrix, source_swapped=True)
    if args.mask_path is not None:
        from PIL import Image
        try:
            opt['mask'] = np.array(Image.open(args.mask_path).convert('L'), dtype=np.uint8)
        except (IOError, OSError) as e:
            raise SystemExit('--mask_path %s: %s' % (args.mask_path, e))
    return opt


def temporal_options(args, matrix='bt601'):
    """--temporal_strength / --temporal_radius / --temporal_sensitivity / --temporal_levels / --temporal_subpel / --temporal_overlap -> the
    temporal= dict of the lanes (faststyle_amd/stream.py), None without --temporal_strength; matrix: what --color_matrix defaults to.  A value
    outside its range, or --temporal_levels, --temporal_subpel or --temporal_overlap without --temporal_strength, is a SystemExit here, before
    anything is loaded.  Every path of this script feeds the net B,G,R: the stage is told so (source_bgr)."""
    s = getattr(args, 'temporal_strength', None)                # (the six flags are absent from the namespace unless given)
    radius, sensitivity = getattr(args, 'temporal_radius', 7), getattr(args, 'temporal_sensitivity', 16)
    levels = getattr(args, 'temporal_levels', None)
    if levels is not None and not 1 <= levels <= 3:
        raise SystemExit('--temporal_levels %d is outside [1, 3]' % levels)
    if levels is not None and s is None:
        raise SystemExit('--temporal_levels needs --temporal_strength')
    subpel = getattr(args, 'temporal_subpel', None)
    if subpel is not None and not 0 <= subpel <= 2:
        raise SystemExit('--temporal_subpel %d is outside [0, 2]' % subpel)
    if subpel is not None and s is None:
        raise SystemExit('--temporal_subpel needs --temporal_strength')
    overlap = getattr(args, 'temporal_overlap', None)
    if overlap is not None and not 0 <= overlap <= 1:
        raise SystemExit('--temporal_overlap %d is outside [0, 1]' % overlap)
    if overlap is not None and s is None:
        raise SystemExit('--temporal_overlap needs --temporal_strength')
    if not 0 <= radius <= 7:
        raise SystemExit('--temporal_radius %d is outside [0, 7]' % radius)
    if not 1 <= sensitivity <= 256:
        raise SystemExit('--temporal_sensitivity %d is outside [1, 256]' % sensitivity)
    if s is None:
        return None
    if not 0.0 <= s <= 1.0:
        raise SystemExit('--temporal_strength %r is outside [0, 1]' % s)
    opt = dict(strength=s, sensitivity=sensitivity, radius=radius, matrix=args.color_matrix or matrix, source_bgr=True)
    if levels is not None:
        opt = dict(opt, levels=levels)
    if subpel is not None:
        opt = dict(opt, subpel=subpel)
    return opt if overlap is None else dict(opt, overlap=overlap)


def batch_options(args):
    """--video_batch / --precision -> (frames per pass, the lanes' bf16=).  The flags are absent from the namespace unless given.  A batch
    outside [1, 64] or without --video_in, or bf16 for a deconv model, is a SystemExit here, before anything is loaded."""
    batch = getattr(args, 'video_batch', None)
    if batch is not None and not 1 <= batch <= 64:
        raise SystemExit('--video_batch %d is outside [1, 64]' % batch)
    if batch is not None and args.video_in is None:
        raise SystemExit('--video_batch needs --video_in: it batches the consecutive frames of that stream')
    bf16 = getattr(args, 'precision', 'fp32') == 'bf16'
    if bf16 and args.upsample_method == 'deconv':
        raise SystemExit('--precision bf16 does not take --upsample_method deconv: the mixed-precision path is for resize-conv models')
    return batch or 1, bf16


def also_options(args):
    """--video_also IN OUT, repeatable -> [(IN, OUT), ...] of the further streams, [] without the flag (absent from the namespace unless
    given).  Without both --video_in and --video_out, with --video_batch, more than 63 pairs, '-' for more than one input or more than one
    output, or a file named twice: a SystemExit here, before anything is loaded."""
    also = getattr(args, 'video_also', None)
    if also is None:
        return []
    if args.video_in is None or args.video_out is None:
        raise SystemExit('--video_also needs --video_in and --video_out: it names further streams beside that one')
    if getattr(args, 'video_batch', None) is not None:
        raise SystemExit('--video_also and --video_batch are mutually exclusive: a batch is one frame of every stream or consecutive frames of one')
    if len(also) > 63:
        raise SystemExit('--video_also was given %d times: at most 63 (64 streams per pass)' % len(also))
    ins, outs = [args.video_in] + [a for a, _ in also], [args.video_out] + [b for _, b in also]
    for flag, names in (('input', ins), ('output', outs)):
        if names.count('-') > 1:
            raise SystemExit('--video_also: - names more than one %s: the standard %s serves one stream' % (flag, flag))
    files = [os.path.abspath(n) for n in ins + outs if n != '-']
    for n in files:
        if files.count(n) > 1:
            raise SystemExit('--video_also: %s is named more than once: every stream has its own input and output' % n)
    return [(a, b) for a, b in also]


def delivery_options(args):
    """--output_size / --output_filter -> (size, filter) with size (W, H) or 'source', None without --output_size.  The flags are absent from
    the namespace unless given.  A malformed size, or --output_filter alone, is a SystemExit here, before anything is loaded."""
    size, filt = getattr(args, 'output_size', None), getattr(args, 'output_filter', None)
    if size is None:
        if filt is not None:
            raise SystemExit('--output_filter needs --output_size')
        return None
    if list(size) == ['source']:
        return 'source', filt or 'bicubic'
    try:
        if len(size) != 2:
            raise ValueError
        W, H = (int(v) for v in size)
    except ValueError:
        raise SystemExit("--output_size takes W H or 'source', got %s" % ' '.join(size))
    if W < 1 or H < 1:
        raise SystemExit('--output_size %d %d: both sides must be at least 1' % (W, H))
    return (W, H), filt or 'bicubic'


def guided_options(args, matrix='bt601'):
    """--output_guided / --guided_radius / --guided_smoothness -> the guided= dict of the lanes' deliver= (faststyle_amd/stream.py), None
    without --output_guided; matrix: what --color_matrix defaults to.  The flags are absent from the namespace unless given.  A value flag
    without --output_guided, a value outside its range, --output_guided without --output_size or --frame_size or together with
    --output_filter is a SystemExit here, before anything is loaded.  Every path of this script feeds the net B,G,R: the stage is told so
    (source_bgr)."""
    on = getattr(args, 'output_guided', False)
    for flag in ('guided_radius', 'guided_smoothness'):
        if hasattr(args, flag) and not on:
            raise SystemExit('--%s needs --output_guided' % flag)
    if not on:
        return None
    radius, smoothness = getattr(args, 'guided_radius', 2), getattr(args, 'guided_smoothness', 4)
    if not 1 <= radius <= 8:
        raise SystemExit('--guided_radius %d is outside [1, 8]' % radius)
    if not 1 <= smoothness <= 64:
        raise SystemExit('--guided_smoothness %d is outside [1, 64]' % smoothness)
    if getattr(args, 'output_size', None) is None:
        raise SystemExit("--output_guided needs --output_size: the source's own size ('source')")
    if getattr(args, 'output_filter', None) is not None:
        raise SystemExit('--output_guided and --output_filter are mutually exclusive: the delivery is guided or resampled')
    if args.frame_size is None:
        raise SystemExit("--output_guided needs --frame_size W H: the net runs below the source's size and the full-size source guides the delivery")
    return dict(radius=radius, smoothness=smoothness, matrix=args.color_matrix or matrix, source_bgr=True)


def deliver_dict(delivery, source_size, net_size, guided=None):
    """The deliver= dict of the lanes for delivery_options' answer (source_size, net_size: (W, H)); the resampling plan is checked here, on the
    host: a size the kernel does not take is a SystemExit.  guided: guided_options' answer; the delivery then has the source's size, which
    is no smaller than the net's and not the net's."""
    from faststyle_amd import _lib, engine
    W, H = source_size if delivery[0] == 'source' else delivery[0]
    if guided is not None:
        if (W, H) != tuple(source_size):
            raise SystemExit("--output_guided: the delivery is %d by %d, the source %d by %d: the full-size source guides the delivery, so "
                             "--output_size is the source's size ('source')" % ((W, H) + tuple(source_size)))
        if W < net_size[0] or H < net_size[1] or (W, H) == tuple(net_size) or max(W, H) > 32767:
            raise SystemExit('--output_guided upsamples: a source of %d by %d with the net at %d by %d (--frame_size no larger than the source '
                             'on both sides, smaller on one)' % ((W, H) + tuple(net_size)))
        return dict(height=H, width=W, guided=guided)
    try:
        engine.ResampleHost().resample_plan(net_size[1], net_size[0], H, W, delivery[1])
    except _lib.FaststyleError as e:
        raise SystemExit('--output_size %d %d: %s' % (W, H, e))
    return dict(height=H, width=W, filter=delivery[1])


def mix_options(args, camera=False):
    """--model_path2 / --style_mix / --mix_mask / --mix_fade -> dict(model_path2=, weight=, mask= uint8 [H,W] or None, fade= (F0, F1) or None),
    None when none of them is given.  The flags are absent from the namespace unless given.  --model_path2 without one of the other three,
    one of them without it, a value outside its range, an unreadable mask or --mix_fade with the camera loop is a SystemExit here, before
    anything is loaded."""
    given = [f for f in ('style_mix', 'mix_mask', 'mix_fade') if hasattr(args, f)]
    if not hasattr(args, 'model_path2'):
        if given:
            raise SystemExit('--%s needs --model_path2: it mixes two models' % given[0])
        return None
    if not given:
        raise SystemExit('--model_path2 needs --style_mix, --mix_mask or --mix_fade: they say how the two models are mixed')
    t = getattr(args, 'style_mix', 1.0)
    if not 0.0 <= t <= 1.0:                                      # (NaN fails both comparisons)
        raise SystemExit('--style_mix %r is outside [0, 1]' % t)
    fade = getattr(args, 'mix_fade', None)
    if fade is not None:
        if camera:
            raise SystemExit('--mix_fade counts the frames of --frames_dir or --video_in: the camera loop has no frame numbers to fade between')
        if not 0 <= fade[0] < fade[1]:
            raise SystemExit('--mix_fade %d %d: 0-based frame numbers with 0 <= F0 < F1' % tuple(fade))
        fade = tuple(fade)
    mask = None
    if hasattr(args, 'mix_mask'):
        from PIL import Image
        try:
            mask = np.array(Image.open(args.mix_mask).convert('L'), dtype=np.uint8)
        except (IOError, OSError) as e:
            raise SystemExit('--mix_mask %s: %s' % (args.mix_mask, e))
    return dict(model_path2=args.model_path2, weight=t, mask=mask, fade=fade)


def check_mix_mask_size(args, mix, W, H):
    """SystemExit unless the --mix_mask (if any) has the net's input size W x H."""
    if mix is not None and mix['mask'] is not None and mix['mask'].shape != (H, W):
        raise SystemExit('--mix_mask %s is %d by %d, the net takes frames of %d by %d' % ((args.mix_mask,) + mix['mask'].shape[::-1] + (W, H)))


def fade_weight(mix, n):
    """The share of the second model in frame n (0-based) by 256, an integer computed on the host: T_q8 = floor(T * 256 + 0.5) without
    --mix_fade; with it d = F1 - F0, k = min(max(n - F0, 0), d) and (2 T_q8 k + d) // (2 d), T_q8 k / d rounded half up."""
    t_q8 = int(np.floor(mix['weight'] * 256.0 + 0.5))
    if mix['fade'] is None:
        return t_q8
    f0, f1 = mix['fade']
    d = f1 - f0
    k = min(max(n - f0, 0), d)
    return (2 * t_q8 * k + d) // (2 * d)


def mix_dict(eng, args, mix):
    """The mix= dict of the lanes (faststyle_amd/stream.py) for mix_options' answer: loads the second checkpoint.  A fade starts at frame 0's
    weight; the driver sets every later frame's (set_mix takes shares of 1, and q8 / 256 is quantised back to q8 exactly)."""
    from faststyle_amd import ckpt
    variables2 = eng.mem.from_numpy(eng.flatten_params(ckpt.load_checkpoint(mix['model_path2']), upsample_method=args.upsample_method))
    return dict(variables=variables2, weight=fade_weight(mix, 0) / 256.0, mask=mix['mask'])


def check_mask_size(args, compose, W, H):
    """SystemExit unless the mask (if any) has the net's input size W x H."""
    if compose is not None and 'mask' in compose and compose['mask'].shape != (H, W):
        raise SystemExit('--mask_path %s is %d by %d, the net takes frames of %d by %d' %
                         ((args.mask_path,) + compose['mask'].shape[::-1] + (W, H)))


def run_frames_dir(args):
    from PIL import Image
    from faststyle_amd import stream
    if args.frame_size is not None and args.resolution is not None:
        raise SystemExit('--frame_size (device resize) and --resolution (PIL resize) are mutually exclusive')
    names = sorted(f for f in os.listdir(args.frames_dir) if f.lower().endswith(('.jpg', '.jpeg', '.png')))
    if not names:
        raise SystemExit('no frames under %s' % args.frames_dir)
    compose = compose_options(args)
    temporal = temporal_options(args)
    delivery = delivery_options(args)
    guided = guided_options(args)
    bf16 = batch_options(args)[1]
    mix = mix_options(args)
    first_size = None
    if delivery is not None or (((compose is not None and 'mask' in compose) or (mix is not None and mix['mask'] is not None)) and
                                (args.frame_size or args.resolution) is None):
        try:
            with Image.open(os.path.join(args.frames_dir, names[0])) as im:
                first_size = im.size
        except (IOError, OSError) as e:
            raise SystemExit('%s: %s' % (os.path.join(args.frames_dir, names[0]), e))
    if compose is not None and 'mask' in compose:                # (the first frame's size, before the model is loaded; later sizes: build())
        check_mask_size(args, compose, *(args.frame_size or args.resolution or first_size))
    if mix is not None and mix['mask'] is not None:
        check_mix_mask_size(args, mix, *(args.frame_size or args.resolution or first_size))
    if delivery is not None:                                     # ('source': the first frame's own size, for every frame; checked before the model is loaded)
        delivery = (tuple(first_size) if delivery[0] == 'source' else delivery[0], delivery[1])
        deliver_dict(delivery, first_size, tuple(args.frame_size or args.resolution or first_size), guided)
    eng, variables = _load(args)
    if not os.path.isdir(args.output_dir):
        os.makedirs(args.output_dir)
    # On the GPU the frames of a directory are independent work: two of them in flight on two streams (stream.PipelinedStylizer: 720p 1277 -> 1890 frames/s;
    # FS_FRAMES_IN_FLIGHT=1 for one at a time).  The results -- and their order -- are the same.
    import collections
    depth = int(os.environ.get('FS_FRAMES_IN_FLIGHT', '2')) if hasattr(eng.mem, 'torch') else 1
    pend = collections.deque()

    # --output_format jpg: the lanes encode.  The .png holds img_out[:, :, ::-1], the lane's frame with R and B swapped back -- which is the frame
    # of a lane that does not swap, so the encoder is given that one (swap_rb=False) and its bytes go to disk as they are.
    jpg = args.output_format == 'jpg'
    kw = dict(swap_rb=False, jpeg=dict(quality=args.output_quality, subsampling=2)) if jpg else {}
    if compose is not None:                                      # (compose_options: such lanes do not swap; the .png is then the frame as it comes)
        kw = dict(kw, swap_rb=False, compose=compose)
    if temporal is not None:                                     # (a run of frames of another size builds a new stylizer: it starts over)
        kw = dict(kw, temporal=temporal)
    if bf16:
        kw = dict(kw, bf16=True)
    count = [0]                                                  # frames handed to a stylizer so far: --mix_fade goes by it
    before = None
    if mix is not None:                                          # (both nets are fed and shown alike: the channel handling does not change)
        kw = dict(kw, mix=mix_dict(eng, args, mix))
        if mix['fade'] is not None:
            def before(st):
                st.set_mix(fade_weight(mix, count[0]) / 256.0)
                count[0] += 1

    def save(n, img_out):
        if jpg:
            with open(os.path.join(args.output_dir, os.path.splitext(n)[0] + '.jpg'), 'wb') as f:
                f.write(img_out)
            return
        # cv2.imshow / VideoWriter interpret that array as BGR; save exactly what they would show
        Image.fromarray(img_out if compose is not None else img_out[:, :, ::-1]).save(os.path.join(args.output_dir, os.path.splitext(n)[0] + '.png'))

    # --frame_size W H: every frame is resized to W x H on the device, with cv2.resize's resampling (stream.py, source=).  --input_decode native: the
    # .jpg / .jpeg frames the library's decoder takes go in as file bytes (RGB; the lane swaps R and B on the device, source swap_rb: the BGR of a
    # cv2 capture, as the PIL path below delivers it from the host); the others, and whatever fails to decode, go through PIL.  --resolution is a
    # PIL resize and therefore keeps the PIL decode.
    native = args.input_decode == 'native' and args.resolution is None

    def pil_rgb(src):
        im = Image.open(src).convert('RGB')
        if args.resolution is not None:
            im = im.resize(tuple(args.resolution))
        return np.asarray(im, np.uint8)

    def frames():
        """(name, key, frame): key tells which stylizer takes the frame -- ('pix', Hs, Ws) for BGR pixels, ('jpeg', source dict) for file bytes"""
        for n in names:
            path = os.path.join(args.frames_dir, n)
            if native and n.lower().endswith(('.jpg', '.jpeg')):
                with open(path, 'rb') as f:
                    data = f.read()
                src = stream.jpeg_source(eng, data, swap_rb=True)
                if src is not None:
                    yield n, ('jpeg', src), data
                    continue
            frame = np.ascontiguousarray(pil_rgb(path)[:, :, ::-1])          # what cap.read() returns: BGR
            yield n, ('pix',) + frame.shape[:2], frame

    def build(key):
        if key[0] == 'jpeg':
            source = key[1]
            Hs, Ws = source['height'], source['width']
        else:
            Hs, Ws = key[1:]
            source = dict(height=Hs, width=Ws) if args.frame_size is not None else None
        W, H = args.frame_size if args.frame_size is not None else (Ws, Hs)
        print('Resolution is: {0} by {1}'.format(W, H))
        check_mask_size(args, compose, W, H)
        check_mix_mask_size(args, mix, W, H)
        more = dict(kw, source=source) if source is not None else kw
        if delivery is not None:
            more = dict(more, deliver=deliver_dict(delivery, (Ws, Hs), (W, H), guided))
            print('Output size is: {0} by {1}'.format(*delivery[0]))
        if depth > 1:
            return stream.PipelinedStylizer(eng, variables, H, W, depth=depth, upsample_method=args.upsample_method, **more)
        return stream.FrameStylizer(eng, variables, H, W, args.upsample_method, **more)

    def not_taken(data):
        import io
        return np.array(pil_rgb(io.BytesIO(data)))                           # (RGB: a stylizer of JPEG frames swaps on the device)

    it = frames()
    cur = next(it, None)
    while cur is not None:                                                  # one stylizer per run of frames of the same source
        key, nxt = cur[1], [None]
        st = build(key)

        def segment(item=cur):
            while item is not None and item[1] == key:
                pend.append(item[0])
                yield item[2]
                item = next(it, None)
            nxt[0] = item

        if depth > 1:
            for out in st.run(segment(), not_taken=not_taken, before_submit=None if before is None else (lambda st=st: before(st))):
                save(pend.popleft(), out)
        else:
            for frame in segment():
                if before is not None:
                    before(st)
                try:
                    out = st(frame)                                          # = cvtColor(astype(uint8)(Y), BGR2RGB)
                except stream.FrameNotTaken:
                    out = st(not_taken(frame))
                save(pend.popleft(), out)
        st.release()
        cur = nxt[0]


def check_video_flags(args):
    """The flag combinations --video_in / --video_out do not take: SystemExit with the reason, before anything is loaded."""
    if args.video_out is not None and args.video_in is None:
        raise SystemExit('--video_out needs --video_in: it writes the stylized frames of that stream')
    if args.video_in is not None and args.frames_dir is not None:
        raise SystemExit('--video_in and --frames_dir are mutually exclusive: frames come from one place')
    if args.video_in is not None and args.resolution is not None:
        raise SystemExit('--video_in and --resolution are mutually exclusive: --resolution is a PIL resize of image files; use --frame_size W H')
    if getattr(args, 'frame_filter', None) is not None:
        if args.video_in is None or args.video_depth != 'stream':
            raise SystemExit('--frame_filter resamples the fp32 frames of a deep stream: it needs --video_in and --video_depth stream')
        if args.frame_size is None:
            raise SystemExit('--frame_filter needs --frame_size W H: it is the filter of that resize')
    also_options(args)


def run_video(args):
    """--video_in [--video_out]: a YUV4MPEG2 stream through the pipelined lanes.  The driver reads frame i + 1 into the next lane's pinned buffer
    while frame i is on the device."""
    import collections
    from faststyle_amd import _lib, engine, stream, y4m
    check_video_flags(args)
    compose = compose_options(args, args.video_matrix)
    temporal = temporal_options(args, args.video_matrix)
    delivery = delivery_options(args)
    guided = guided_options(args, args.video_matrix)
    batch, bf16 = batch_options(args)
    also = also_options(args)
    mix = mix_options(args)
    frame_filter = getattr(args, 'frame_filter', None)
    to_stdout = args.video_out == '-'
    log = sys.stderr if to_stdout or any(b == '-' for _, b in also) else sys.stdout

    def say(text):
        print(text, file=log)
        log.flush()

    fin = sys.stdin.buffer if args.video_in == '-' else open(args.video_in, 'rb')
    fout = None
    more_in, more_out = [], []                                               # --video_also: the further streams' files
    try:
        try:
            reader = y4m.Reader(fin, deep=args.video_depth == 'stream')
        except y4m.Y4MError as e:
            raise SystemExit('--video_in %s: %s' % (args.video_in, e))
        fmt = reader.format
        readers = [reader]
        for name, _ in also:                                                 # every further stream has the first one's frames
            more_in.append(sys.stdin.buffer if name == '-' else open(name, 'rb'))
            try:
                readers.append(y4m.Reader(more_in[-1], deep=args.video_depth == 'stream'))
            except y4m.Y4MError as e:
                raise SystemExit('--video_also %s: %s' % (name, e))
            other = readers[-1].format
            for field, what in (('width', 'width'), ('height', 'height'), ('components', 'components'), ('sampling', 'sampling'),
                                ('siting', 'siting'), ('full_range', 'range'), ('bits', 'bits')):
                if getattr(other, field) != getattr(fmt, field):
                    raise SystemExit('--video_also %s: its %s %r is not that of --video_in %s, %r: the streams of a pass have one size and '
                                     'format' % (name, what, getattr(other, field), args.video_in, getattr(fmt, field)))
        Ws, Hs = fmt.width, fmt.height
        colour = dict(sampling=fmt.sampling, siting=fmt.siting, matrix=args.video_matrix, full_range=fmt.full_range, components=fmt.components)
        colour_in = dict(colour, bits=fmt.bits) if fmt.bits != 8 else colour       # (an 8-bit stream runs exactly as without --video_depth)
        out_bits = fmt.bits if args.video_out_depth is None else args.video_out_depth
        colour_out = dict(colour, bits=out_bits) if out_bits != 8 else colour
        if frame_filter is not None and fmt.bits == 8:
            raise SystemExit('--video_in %s: --frame_filter takes a stream of 9 to 16 bits per sample, this one has 8: --frame_size resizes it '
                             'with cv2.resize\'s resampling' % args.video_in)
        if fmt.bits != 8 and args.frame_size is not None and frame_filter is None:
            raise SystemExit('--video_in %s: --frame_size does not take a stream of %d bits per sample: the resize is 8-bit only' %
                             (args.video_in, fmt.bits))
        try:
            engine.YuvHost().yuv_plan(Ws, Hs, **colour_in)                   # (a frame the kernels do not take: said before the model is loaded)
            if args.video_out is not None and out_bits != 8:
                y4m.header(Ws, Hs, fmt.sampling, fmt.siting, fmt.components, fmt.full_range, bits=out_bits)    # (a layout without a deep tag)
        except (_lib.FaststyleError, y4m.Y4MError) as e:
            raise SystemExit('--video_in %s: %s' % (args.video_in, e))
        W, H = args.frame_size if args.frame_size is not None else (Ws, Hs)
        check_mask_size(args, compose, W, H)
        check_mix_mask_size(args, mix, W, H)
        deliver = None
        if delivery is not None:                                             # (a size the kernel or the output layout does not take: said before the model is loaded)
            deliver = deliver_dict(delivery, (Ws, Hs), (W, H), guided)
            try:
                if args.video_out is not None:
                    engine.YuvHost().yuv_plan(deliver['width'], deliver['height'], **colour_out)
                if frame_filter is not None and (W, H) != (Ws, Hs):
                    engine.ResampleHost().resample_plan(Hs, Ws, H, W, frame_filter)
            except _lib.FaststyleError as e:
                raise SystemExit('--output_size %d %d: %s' % (deliver['width'], deliver['height'], e))
        elif frame_filter is not None and (W, H) != (Ws, Hs):
            try:
                engine.ResampleHost().resample_plan(Hs, Ws, H, W, frame_filter)
            except _lib.FaststyleError as e:
                raise SystemExit('--frame_size %d %d: %s' % (W, H, e))
        say('Resolution is: {0} by {1}'.format(W, H))
        if deliver is not None:
            say('Output size is: {0} by {1}'.format(deliver['width'], deliver['height']))
        say('Loading up model...')
        eng, variables = _load(args)
        # The channel quirk as in run_frames_dir: the net sees B,G,R (source swap_rb, what a cv2 capture delivers) and the output is swapped back --
        # which is the frame of a lane that does not swap, so the lanes of a video or .jpg output are built with swap_rb=False.
        kw = dict(source=dict(height=Hs, width=Ws, swap_rb=True, yuv=colour_in))
        if frame_filter is not None:                                         # (a deep stream: fp32 at its own size, resampled to the net's)
            kw['source']['resample'] = frame_filter
        if deliver is not None:
            kw.update(deliver=deliver)
        jpg = args.video_out is None and args.output_format == 'jpg'
        if args.video_out is not None:
            kw.update(swap_rb=False, yuv_out=colour_out)
        elif jpg:
            kw.update(swap_rb=False, jpeg=dict(quality=args.output_quality, subsampling=2))
        if compose is not None:                                              # (compose_options: such lanes do not swap; the .png is then the frame as it comes)
            kw.update(swap_rb=False, compose=compose)
        if temporal is not None:
            kw.update(temporal=temporal)
        if bf16:
            kw.update(bf16=True)
        if batch > 1:                                                        # (the batch's images are consecutive frames: the stage is told so)
            kw.update(batch=batch)
            if temporal is not None:
                kw.update(temporal=dict(temporal, sequence=True))
        if also:                                                             # (the batch's images are one frame of every stream: likewise)
            kw.update(batch=len(readers))
            if temporal is not None:
                kw.update(temporal=dict(temporal, streams=True))
        if mix is not None:
            kw.update(mix=mix_dict(eng, args, mix))
        fading = mix is not None and mix['fade'] is not None
        sent = [0]                                                           # frames handed to the lanes so far: --mix_fade goes by it

        def set_weights(n):
            """The weights of the next pass of n consecutive frames (a last pass's padding counts on: it is never written)"""
            ws = [fade_weight(mix, sent[0] + i) / 256.0 for i in range(n)]
            st.set_mix(ws if batch > 1 else ws[0])                           # (--video_also: one pass is one frame number, one weight for all)
            sent[0] += n
        depth = int(os.environ.get('FS_FRAMES_IN_FLIGHT', '2')) if hasattr(eng.mem, 'torch') else 1
        if depth > 1:
            st = stream.PipelinedStylizer(eng, variables, H, W, depth=depth, upsample_method=args.upsample_method, **kw)
        else:
            st = stream.FrameStylizer(eng, variables, H, W, args.upsample_method, **kw)
        writer = None
        if args.video_out is not None:
            fout = sys.stdout.buffer if to_stdout else open(args.video_out, 'wb')
            writer = y4m.Writer(fout, st.yuv_out_desc, rate=fmt.rate, aspect=fmt.aspect)
            writers = [writer]
            for (_, name), r in zip(also, readers[1:]):
                more_out.append(sys.stdout.buffer if name == '-' else open(name, 'wb'))
                writers.append(y4m.Writer(more_out[-1], st.yuv_out_desc, rate=r.format.rate, aspect=r.format.aspect))
        elif not os.path.isdir(args.output_dir):
            os.makedirs(args.output_dir)
        say('Begin filtering...')
        done = [0]

        def emit(out):
            if writer is not None:
                writer.write_frame(out)
            elif jpg:
                with open(os.path.join(args.output_dir, '%06d.jpg' % done[0]), 'wb') as f:
                    f.write(out)
            else:
                from PIL import Image
                Image.fromarray(out if compose is not None else out[:, :, ::-1]).save(os.path.join(args.output_dir, '%06d.png' % done[0]))
            done[0] += 1

        failed = None                                                        # a stream that breaks off: what was read is still written
        try:
            if also:
                # one frame of every open stream per pass: the readers fill their rows of the [S, frame_bytes] buffer; a stream that has ended
                # or broken off is inactive from then on, its row stays as it is and is not written
                S = len(readers)
                names = [args.video_in] + [a for a, _ in also]
                outs_of = [args.video_out] + [b for _, b in also]
                is_open, broke = [True] * S, []
                took = collections.deque()

                def close_out(s):
                    writers[s].flush()
                    if s > 0 and outs_of[s] != '-':
                        more_out[s - 1].close()

                def emit_rows(outs):
                    for s in took.popleft():
                        writers[s].write_frame(outs[s])
                        done[0] += 1

                buf = None if depth > 1 else np.zeros((S, fmt.frame_bytes), np.uint8)
                while any(is_open):
                    if depth > 1:
                        if st.in_flight >= depth:
                            emit_rows(st.fetch())
                        buf = st.next_input()                                # [S, frame_bytes], pinned
                    ended = []
                    for s in range(S):
                        if not is_open[s]:
                            continue
                        try:
                            is_open[s] = bool(readers[s].read_frame_into(buf[s]))
                        except y4m.Y4MError as e:
                            is_open[s] = False
                            broke.append('%s %s: %s' % ('--video_in' if s == 0 else '--video_also', names[s], e))
                        if not is_open[s]:
                            ended.append(s)
                    if any(is_open):
                        if temporal is not None:
                            st.set_streams(list(is_open))
                        took.append([s for s in range(S) if is_open[s]])
                        if fading:
                            set_weights(1)
                        if depth > 1:
                            st.submit(buf)
                        else:
                            emit_rows(st(buf))
                    if ended:                                                # (their last frames may still be in flight: written first)
                        while depth > 1 and st.in_flight:
                            emit_rows(st.fetch())
                        for s in ended:
                            close_out(s)
                if broke:
                    failed = '; '.join(broke)
            elif batch > 1:
                # N frames per pass: the reader fills the [N, frame_bytes] buffer row by row; a last pass is padded with the last frame read
                # and only its real frames are written
                real = collections.deque()

                def emit_pass(outs):
                    for i in range(real.popleft()):
                        emit(outs[i])

                buf = None if depth > 1 else np.zeros((batch, fmt.frame_bytes), np.uint8)
                more = True
                while more:
                    if depth > 1:
                        if st.in_flight >= depth:
                            emit_pass(st.fetch())
                        buf = st.next_input()                                # [N, frame_bytes], pinned
                    got = 0
                    try:
                        while got < batch and reader.read_frame_into(buf[got]):
                            got += 1
                    except y4m.Y4MError as e:
                        failed = e
                    more = got == batch
                    if got == 0:
                        break
                    buf[got:] = buf[got - 1]
                    real.append(got)
                    if fading:
                        set_weights(batch)
                    if depth > 1:
                        st.submit(buf)
                    else:
                        emit_pass(st(buf))
                while depth > 1 and st.in_flight:
                    emit_pass(st.fetch())
            elif depth > 1:
                while failed is None:
                    if st.in_flight >= depth:
                        emit(st.fetch())
                    buf = st.next_input()                                    # [1, frame_bytes], pinned
                    try:
                        if not reader.read_frame_into(buf):
                            break
                    except y4m.Y4MError as e:
                        failed = e
                        break
                    if fading:
                        set_weights(1)
                    st.submit(buf[0])
                while st.in_flight:
                    emit(st.fetch())
            else:
                buf = np.zeros(fmt.frame_bytes, np.uint8)
                while failed is None:
                    try:
                        if not reader.read_frame_into(buf):
                            break
                    except y4m.Y4MError as e:
                        failed = e
                        break
                    if fading:
                        set_weights(1)
                    emit(st(buf))
        finally:
            st.release()
        if writer is not None:
            writer.flush()
        say('%d frames' % done[0])
        if failed is not None:
            raise SystemExit(str(failed) if also else '--video_in %s: %s' % (args.video_in, failed))
    finally:
        if args.video_in != '-':
            fin.close()
        if fout is not None and not to_stdout:
            fout.close()
        for (a, b), fa, fb in zip(also, more_in, more_out + [None] * len(also)):
            for name, f in ((a, fa), (b, fb)):
                if f is not None and name != '-' and not f.closed:
                    f.close()


def run_webcam(args):
    mix = mix_options(args, camera=True)
    try:
        import cv2
    except ImportError:
        raise SystemExit('stylize_webcam.py needs OpenCV (cv2) for camera capture and display, as the reference does; '
                         'it is not installed here.  Use --frames_dir to filter a directory of frames.')
    from faststyle_amd import stream
    compose = compose_options(args)
    temporal = temporal_options(args)
    delivery = delivery_options(args)
    guided = guided_options(args)
    bf16 = batch_options(args)[1]
    cap = cv2.VideoCapture(0)
    if args.resolution is not None:
        x_length, y_length = args.resolution
        cap.set(cv2.CAP_PROP_FRAME_WIDTH, x_length)      # (the reference passes the raw property ids 3 and 4: stylize_webcam.py:52-53)
        cap.set(cv2.CAP_PROP_FRAME_HEIGHT, y_length)
    x_new, y_new = int(cap.get(cv2.CAP_PROP_FRAME_WIDTH)), int(cap.get(cv2.CAP_PROP_FRAME_HEIGHT))
    x_cam, y_cam = x_new, y_new
    if guided is not None:                                   # (the one case in which the camera's frames are resized on the device: to --frame_size)
        x_new, y_new = args.frame_size
        deliver_dict(delivery, (x_cam, y_cam), (x_new, y_new), guided)
    print('Resolution is: {0} by {1}'.format(x_new, y_new))
    check_mask_size(args, compose, x_new, y_new)
    check_mix_mask_size(args, mix, x_new, y_new)
    print('Loading up model...')
    eng, variables = _load(args)
    more = dict(temporal=temporal) if temporal is not None else {}
    if mix is not None:
        more['mix'] = mix_dict(eng, args, mix)
    if bf16:
        more['bf16'] = True
    if guided is not None:
        more['source'] = dict(height=y_cam, width=x_cam)
    x_out, y_out = x_new, y_new
    if delivery is not None:
        more['deliver'] = deliver_dict(delivery, (x_cam, y_cam), (x_new, y_new), guided)
        x_out, y_out = more['deliver']['width'], more['deliver']['height']
        print('Output size is: {0} by {1}'.format(x_out, y_out))
    if compose is not None:                                  # (compose_options: the lane does not swap, the loop below does)
        st = stream.FrameStylizer(eng, variables, y_new, x_new, args.upsample_method, swap_rb=False, compose=compose, **more)
    else:
        st = stream.FrameStylizer(eng, variables, y_new, x_new, args.upsample_method, **more)
    fourcc = cv2.VideoWriter_fourcc(*'XVID')
    out = cv2.VideoWriter('output.avi', fourcc, 15.0, (x_out, y_out))
    print('Begin filtering...')
    while True:
        ret, frame = cap.read()
        img_out = st(np.ascontiguousarray(frame))
        if compose is not None:
            img_out = np.ascontiguousarray(img_out[:, :, ::-1])
        out.write(img_out)
        cv2.imshow('frame', img_out)
        if cv2.waitKey(1) & 0xFF == ord('q'):
            break
    cap.release()
    out.release()
    cv2.destroyAllWindows()


def main(argv=None):
    args = setup_parser().parse_args(argv)
    check_video_flags(args)
    batch_options(args)
    if args.video_in is not None:
        run_video(args)
    elif args.frames_dir is not None:
        run_frames_dir(args)
    else:
        run_webcam(args)


if __name__ == '__main__':
    main()
