#!/usr/bin/env python
"""Throughput of the TFRecord input pipeline alone (decode threads + GPU resize + HBM shuffle queue) on
synthetic COCO-like shards (640x480 JPEG quality 90).  usage: pipe_bench.py [n_images] [threads] [host | host_native | host_encode | frames_in | video [out.json [depth | batch]] | resample [out.json]]
"frames_in": the frames-dir loop end to end (stylize_webcam.run_frames_dir, two frames in flight, --output_format jpg) at 720p over a directory of
n JPEG frames: PIL decode against --input_decode native, and from 1080p sources PIL decode + PIL resize (--resolution) against native decode +
device resize (--frame_size).  Every leg runs on the same device, legs alternate over the repeats, and a leg's rate is taken from the DIFFERENCE
between its run over n frames and its run over n / 4 frames, so that engine start-up, checkpoint load and graph capture drop out; written to
profiles/frames_in.json (or to the file named as a fourth argument).
"video": the frames_in legs and, beside them in the same run with the same repeat and median scheme, the raw-video loop (stylize_webcam.run_video:
--video_in / --video_out, 720p 4:2:0 YUV4MPEG2 from a file to a file, the same 16 frames as planes, the same frame counts); written to profiles/video_stream.json.  The video loop is several times faster than the
others: give it enough frames (1280) that its timed difference is about a second.
"video" with a depth as the fifth argument (pipe_bench.py 1280 4 video profiles/video_deep.json 10): only the raw-video loop, as two legs that
alternate in the one run -- the 8-bit stream above and the same frames as a stream of that many bits per sample (C420p10 ..., --video_depth
stream, two bytes per sample in and out) -- plus the device time of one 720p launch of the two deep kernels and of the 8-bit kernel pairs they
replace (HIP events around the replay of a graph of 200 launches each); written to profiles/video_deep.json with the digest of the kernel sources.
"video" with "compose" as the fifth argument (pipe_bench.py 1280 4 video profiles/video_compose.json compose): only the raw-video loop, as two legs
that alternate in the one run -- the 8-bit stream above without and with --style_strength 0.7 --preserve_color -- plus the device time of one 720p
launch of compose_kernel (the same graph-of-200 scheme; wide path, with and without a mask, and the narrow path); written to
profiles/video_compose.json with the digest of the kernel sources.
"video" with "temporal" as the fifth argument (pipe_bench.py 1280 4 video profiles/video_temporal.json temporal): the same two-leg scheme without and
with --temporal_strength 0.6, plus the device time of one 720p call of fs_temporal_f32 (its three launches back to back, the graph-of-200 scheme:
with a previous frame at radius 7 and 3, and a first frame); written to profiles/video_temporal.json.  "temporal_kernels" as the third argument runs
those graphs alone: under a kernel trace that run gives the time of each of the three kernels back to back.
"video" with "temporal_levels" as the fifth argument (pipe_bench.py 1280 4 video profiles/video_temporal_pyr.json temporal_levels): the two legs are
--temporal_strength 0.6 alone and with --temporal_levels 3, plus the device time of one 720p call of the stage at one level (fs_temporal_f32), two and
three levels (fs_temporal_pyr_f32: the pyramid launch and one search launch per level more) on a frame moved by (20, -12), the graph-of-200 scheme;
written to profiles/video_temporal_pyr.json.  "temporal_pyr_kernels" as the third argument runs those graphs alone.
"video" with "temporal_subpel" as the fifth argument (pipe_bench.py 1280 4 video profiles/video_temporal_subpel.json temporal_subpel): the two legs
are --temporal_strength 0.6 alone and with --temporal_subpel 2, plus the device time of one 720p call of the stage at radius 7 on a frame moved by
(2, -1) quarter pixels: subpel 0 (fs_temporal_f32, the path without the key), 1 and 2 at one level and subpel 2 at three levels (fs_temporal_sub_f32:
the refinement launch more, the bilinear blend), the graph-of-200 scheme; written to profiles/video_temporal_subpel.json.
"temporal_subpel_kernels" as the third argument runs those graphs alone.
"video" with "temporal_overlap" as the fifth argument (pipe_bench.py 1280 4 video profiles/video_temporal_overlap.json temporal_overlap): the two legs
are --temporal_strength 0.6 alone and with --temporal_overlap 1, plus the device time of one 720p call of the stage at radius 7 with overlap 0
(the path without the key) and 1 (fs_temporal_obmc_f32), at subpel 0 and 2, on three frames: one moved as a whole (every thread of the
overlapped blend takes its one-vector shortcut), one whose neighbouring blocks alternate between two vectors (none does) and one whose two halves
move apart; three alternating repeats of the graph-of-200 scheme, with the share of threads on the shortcut read back from the vectors; written
to profiles/video_temporal_overlap.json.  "temporal_overlap_kernels" as the third argument runs those graphs alone.
"resample" (pipe_bench.py 96 4 resample): the fp32 resampler.  The kernel alone (the graph-of-200 scheme, data resident): 720 x 1280 -> 2160 x 3840
bicubic and lanczos, 2160 x 3840 -> 720 x 1280 bicubic; and the raw-video loop over a 2160p 4:2:0 file with --frame_size 1280 720, without and
with --output_size source, as two legs that alternate in the one run (rates from the difference between n and n / 4 frames); written to
profiles/video_resample.json with the digest of the kernel sources.
"guided" (pipe_bench.py 96 4 guided): guided delivery.  One call of fs_guided_f32 alone (its three launches back to back, the graph-of-200
scheme, data resident): 720 x 1280 -> 2160 x 3840 at radius 2 for an RGBX and an fp32 source, at radius 8, and the bicubic fs_resample_f32 of
the same enlargement in the same run; and the 2160p raw-video loop with --frame_size 1280 720 --output_size source, resampled (bicubic) and
with --output_guided, alternating in the one run; written to profiles/video_guided.json with the digest of the kernel sources.
"video" with "batch" as the fifth argument (pipe_bench.py 1280 4 video profiles/video_batch.json batch): consecutive frames per pass.  (a) the
device time per frame of one fs_temporal_batch_f32 call over 8 frames against 8 chained single-frame calls (Engine.temporal_f32, the path of a
lane without sequence=), at 720p and 1080p for (levels, subpel, overlap) = (1, 0, 0) and (3, 2, 1): the graph-of-200 scheme with the data
resident, the two alternating over three repeats.  (b) the raw-video loop over a 1080p 4:2:0 file at --video_batch 1 and 8, --precision fp32
and bf16, without and with --temporal_strength 0.6: eight legs that alternate in the one run, rates from the difference between n and n / 4
frames; written to profiles/video_batch.json with the digest of the kernel sources.  "video_batch_kernels" as the third argument runs the
720p (3, 2, 1) graphs of (a) alone: under a kernel trace that run gives the kernels' shares.
"video" with "mix" as the fifth argument (pipe_bench.py 1280 4 video profiles/video_mix.json mix): two styles per stream.  (a) the device time
of one 720p launch of mix_kernel (fs_mix_f32; the graph-of-200 scheme, data resident): without and with a mask, wide and narrow path, with the
weight as an argument and from device memory, and compose_kernel in plain mode the same way in the same run, three alternating repeats; the
device time of one 720p forward pass of one model and of two models alternating (what a mixed lane captures: both filter re-layouts rebuilt
per pass), whose difference is the second forward's.  (b) the 720p raw-video loop with one model and with --model_path2 ... --style_mix 0.5,
and (c) with --mix_fade over the middle tenth of the frames: three legs that alternate in the one run, rates from the difference between n
and n / 4 frames; written to profiles/video_mix.json with the digest of the kernel sources.  "mix_kernels" as the third argument runs (a) alone.
"video" with "streams" as the fifth argument (pipe_bench.py 1280 4 video profiles/video_streams.json streams): independent streams per pass.
(a) the device time per frame of one fs_temporal_streams_f32 call over 8 streams against 8 single-frame calls on the same data
(Engine.temporal_f32: what eight batch-1 lanes run), at 720p and 1080p for (levels, subpel, overlap) = (1, 0, 0) and (3, 2, 1): the
graph-of-200 scheme with the data resident, the two alternating over three repeats.  (b) the raw-video loop over 1080p 4:2:0 files: 8 inputs
of n / 8 frames through --video_also against one input of n frames at --video_batch 8, --precision fp32 and bf16, without and with
--temporal_strength 0.6: eight legs that alternate in the one run, rates from the difference between n and n / 4 frames; written to
profiles/video_streams.json with the digest of the kernel sources.  "video_streams_kernels" as the third argument runs the 720p (3, 2, 1)
graphs of (a) alone: under a kernel trace that run gives the kernels' shares.
"host_encode": the host half of the native JPEG OUTPUT path (fs_jpeg_write: Huffman coding of ready coefficient buffers) against PIL's
Image.save(JPEG) of the same 1280x720 frames (quality 95, 4:2:0) at the same thread count, host only; the coefficient buffers are those of PIL's
files, read back with fs_jpeg_parse + fs_jpeg_decode (the buffer fs_jpeg_forward_many leaves on the GPU: tests/test_jpeg_encode.py).
"host_native": the host half of the native JPEG path (fs_jpeg_parse + fs_jpeg_decode: the Huffman pass, coefficients dropped) and then the PIL
host half, at the same thread count, one after the other over the same shards.
"host": the host half only -- record framing, Example parsing and the JPEG decode pool, decoded images dropped (no engine, no GPU): what a rank's
cores sustain when eight pools run side by side on one box whose single GPU would otherwise be shared by all eight (tools/pipe_bench8.sh)."""
import io
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from faststyle_amd import datapipe, engine, tfrecord  # noqa: E402


def host_encode(n, th):
    """-> dict of the two rates (frames/s); prints them."""
    import ctypes
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    host = engine.JpegHost()
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (90, 160, 3), dtype=np.uint8)
    frames, coefs, sizes = [], [], []
    for k in range(16):      # 16 distinct natural-ish frames (upsampled noise), reused
        im = Image.fromarray(np.roll(base, 5 * k, axis=1)).resize((1280, 720), Image.BICUBIC)
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=95, subsampling=2)
        data = buf.getvalue()
        rc, info = host.jpeg_parse(data)
        coef = np.zeros(int(info.coef_bytes), dtype=np.uint8)
        assert rc == 0 and host.jpeg_decode(data, info, coef.ctypes.data, coef.nbytes) == 0
        rc, plan = host.jpeg_encode_plan(1280, 720, 3, 2, 2)
        assert rc == 0 and host.jpeg_write_bytes(plan, coef) == data          # the same file, byte for byte
        frames.append(im)
        coefs.append(coef)
        sizes.append(len(data))
    bound = host.jpeg_write_bound(plan)
    import threading
    local = threading.local()

    def native(k):
        if not hasattr(local, "out"):
            local.out = ctypes.create_string_buffer(bound)
        c = coefs[k % 16]
        rc, m = host.jpeg_write(plan, c.ctypes.data, c.nbytes, ctypes.addressof(local.out), bound)
        assert rc == 0
        return len(ctypes.string_at(local.out, m))

    def pil(k):
        buf = io.BytesIO()
        frames[k % 16].save(buf, "JPEG", quality=95, subsampling=2)
        return len(buf.getvalue())

    res = {"frames": n, "threads": th, "host_cores": os.cpu_count(), "size": [720, 1280], "quality": 95, "subsampling": "4:2:0",
           "mean_file_bytes": float(np.mean(sizes))}
    for name, fn in (("fs_jpeg_write", native), ("pil_save_jpeg", pil)):
        with ThreadPoolExecutor(th) as ex:
            list(ex.map(fn, range(2 * th)))       # warm-up
            t0 = time.time()
            total = sum(ex.map(fn, range(n)))
            dt = time.time() - t0
        res[name + "_frames_per_s"] = n / dt
        print("host_encode: %.0f frames/s %s (%d 720p frames, %.1f KB/file, in %.2f s, %d threads, %d host cores)"
              % (n / dt, name, n, total / n / 1e3, dt, th, os.cpu_count()))
    return res


def kernel_timed(fn, launches=200):
    """Device microseconds per call of fn: the launches are captured into one graph and the replay is timed with HIP events, after a warm-up --
    launched one by one from Python they would measure the interpreter."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        for _ in range(launches):
            fn()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches


def kernel_times(bits, W=1280, H=720, launches=200):
    """-> dict of device microseconds per 720p 4:2:0 launch (HIP events around the replay of a graph that holds `launches` of them, after a warm-up): the two deep
    kernels, and the 8-bit conversions with the u8 <-> f32 launches of a lane beside them."""
    eng = engine.Engine()
    mem = eng.mem
    d8, dd = eng.yuv_plan(W, H, full_range=True), eng.yuv_plan(W, H, full_range=True, bits=bits)
    rng = np.random.default_rng(1)
    p8 = mem.upload_u8(rng.integers(0, 256, (1, int(d8.frame_bytes)), dtype=np.uint8))
    pd = mem.upload_u8(rng.integers(0, 2 ** bits, (1, int(dd.frame_bytes) // 2)).astype("<u2").view(np.uint8))
    u8 = mem.upload_u8(np.zeros((1, H, W, 3), np.uint8))
    f32 = mem.from_numpy(rng.uniform(0, 255, (1, H, W, 3)).astype(np.float32))

    timed = lambda fn: kernel_timed(fn, launches)
    res = {"yuv_deep_to_f32": timed(lambda: eng.yuv_deep_to_f32(pd, dd, f32, swap_rb=True)),
           "yuv_to_rgb_u8_then_u8_to_f32": timed(lambda: (eng.yuv_to_rgb_u8(p8, d8, u8, swap_rb=True), eng.u8_to_f32(u8, f32))),
           "f32_to_yuv_deep": timed(lambda: eng.f32_to_yuv_deep(f32, dd, pd)),
           "f32_to_u8_then_rgb_to_yuv_u8": timed(lambda: (eng.f32_to_u8(f32, u8), eng.rgb_to_yuv_u8(u8, d8, p8)))}
    for k, v in res.items():
        print("video: %8.1f us per 720p launch: %s" % (v, k))
    return res


def compose_kernel_times(W=1280, H=720, launches=200):
    """-> dict of device microseconds per 720p launch of compose_kernel (fs_compose_f32), timed as kernel_times does: keep_color at strength 0.7 on
    the wide path without and with a mask, plain mode, and the narrow path (the source one float off 16-byte alignment)."""
    eng = engine.Engine()
    mem = eng.mem
    rng = np.random.default_rng(2)
    src = mem.from_numpy(rng.uniform(0, 255, (1, H, W, 3)).astype(np.float32))
    net = mem.from_numpy(rng.uniform(0, 255, (1, H, W, 3)).astype(np.float32))
    dst = mem.empty((1, H, W, 3))
    mask = mem.upload_u8(rng.integers(0, 256, (H, W), dtype=np.uint8))
    off = mem.view(mem.from_numpy(np.zeros(H * W * 3 + 4, np.float32)), 1, (1, H, W, 3))
    kw = dict(strength_q8=179, keep_color=True, bgr=False, src_swapped=True)
    res = {"compose_keep_color": kernel_timed(lambda: eng.compose_f32(src, net, dst, **kw)),
           "compose_keep_color_mask": kernel_timed(lambda: eng.compose_f32(src, net, dst, mask=mask, **kw)),
           "compose_plain": kernel_timed(lambda: eng.compose_f32(src, net, dst, strength_q8=179)),
           "compose_keep_color_narrow_path": kernel_timed(lambda: eng.compose_f32(off, net, dst, **kw))}
    for k, v in res.items():
        print("video: %8.1f us per 720p launch: %s" % (v, k))
    return res


def mix_kernel_times(W=1280, H=720, launches=200, repeats=3):
    """-> dict: device microseconds per 720p launch of mix_kernel (fs_mix_f32) and of compose_kernel in plain mode, timed as kernel_times
    does and alternating over the repeats (the median and every repeat); and per 720p forward pass of one model and of two models
    alternating on workspaces of their own under frozen=True, as a mixed lane runs them."""
    from faststyle_amd import ckpt
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    eng = engine.Engine()
    mem = eng.mem
    rng = np.random.default_rng(2)
    a = mem.from_numpy(rng.uniform(0, 255, (1, H, W, 3)).astype(np.float32))
    b = mem.from_numpy(rng.uniform(0, 255, (1, H, W, 3)).astype(np.float32))
    dst = mem.empty((1, H, W, 3))
    mask = mem.upload_u8(rng.integers(0, 256, (H, W), dtype=np.uint8))
    off = mem.view(mem.from_numpy(np.zeros(H * W * 3 + 4, np.float32)), 1, (1, H, W, 3))
    moff = mem.view(mem.upload_u8(np.zeros(H * W + 4, np.uint8)), 1, (H, W))
    wdev = eng.i32_buffer([128])
    cases = [("mix", lambda: eng.mix_f32(a, b, dst, weight_q8=128)),
             ("mix_weight_from_memory", lambda: eng.mix_f32(a, b, dst, weights=wdev)),
             ("mix_mask", lambda: eng.mix_f32(a, b, dst, weights=wdev, mask=mask)),
             ("mix_narrow_path", lambda: eng.mix_f32(off, b, dst, weight_q8=128)),
             ("mix_mask_narrow_path", lambda: eng.mix_f32(off, b, dst, weight_q8=128, mask=moff)),
             ("compose_plain", lambda: eng.compose_f32(a, b, dst, strength_q8=128)),
             ("compose_plain_mask", lambda: eng.compose_f32(a, b, dst, strength_q8=128, mask=mask))]
    times = {name: [] for name, _ in cases}
    for _ in range(repeats):
        for name, fn in cases:
            times[name].append(kernel_timed(fn, launches))
    res = {name: {"us": sorted(v)[len(v) // 2], "all_repeats": v} for name, v in times.items()}
    res["bytes_moved"] = 3 * H * W * 3 * 4
    # the forward passes: one model alone (its filters re-laid out once, outside the graph), and two models one behind the other
    models = [mem.from_numpy(eng.flatten_params(ckpt.load_checkpoint(os.path.join(root, "models", m + "_final.ckpt")))) for m in ("starry", "candy")]
    ws = [eng.new_tnet_workspace(1, H, W) for _ in models]
    ys = [mem.empty((1,) + tuple(eng.tnet_out_shape(H, W)) + (3,)) for _ in models]
    fwd = lambda k: eng.tnet_forward(models[k], a, frozen=True, workspace=ws[k], out=ys[k])
    ftimes = {"forward_one_model": [], "forward_two_models_alternating": []}
    for _ in range(repeats):
        eng.invalidate_frozen()
        ftimes["forward_one_model"].append(kernel_timed(lambda: fwd(0), 20))
        eng.invalidate_frozen()
        ftimes["forward_two_models_alternating"].append(kernel_timed(lambda: (fwd(0), fwd(1)), 20))
    for name, v in ftimes.items():
        res[name] = {"us": sorted(v)[len(v) // 2], "all_repeats": v}
    res["second_forward_us"] = res["forward_two_models_alternating"]["us"] - res["forward_one_model"]["us"]
    res["filter_relayouts_us_per_frame"] = res["forward_two_models_alternating"]["us"] - 2 * res["forward_one_model"]["us"]
    for k, v in res.items():
        if isinstance(v, dict):
            print("mix: %8.1f us per 720p launch: %s (repeats: %s)" % (v["us"], k, ", ".join("%.1f" % t for t in v["all_repeats"])))
    print("mix: %8.1f us per 720p frame: the second forward; of it %.1f us the two filter re-layouts" %
          (res["second_forward_us"], res["filter_relayouts_us_per_frame"]))
    return res


def video_mix(n, repeats=3, out_json=None):
    """-> dict: mix_kernel_times and the three legs of the 720p raw-video loop (one model, two models at --style_mix 0.5, a --mix_fade over
    the middle tenth of the frames); prints them and writes profiles/video_mix.json (after the kernel times and after every repeat)."""
    import contextlib
    import json
    import shutil
    from PIL import Image
    from faststyle_amd import build as fsbuild
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import stylize_webcam
    n = max(40, n // 40 * 40)
    w, h = 1280, 720
    dst = out_json or os.path.join(root, "profiles", "video_mix.json")
    res = {"frames": n, "frames_in_flight": 2, "host_threads": "1 driver", "host_cores": os.cpu_count(), "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
           "video": "720p 4:2:0 YUV4MPEG2 (full range, BT.601), file to file of 8-bit 4:2:0",
           "method": "rate = (n - n/4) / (t(n) - t(n/4)), median of %d alternating repeats" % repeats, "source_digest": fsbuild.source_digest()}

    def save():
        with open(dst, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    res["kernel_us_per_720p_launch"] = mix_kernel_times()
    save()
    d = tempfile.mkdtemp()
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (90, 160, 3), dtype=np.uint8)
    planes = []
    for k in range(16):      # 16 distinct natural-ish frames (upsampled noise), reused; PIL's matrix, box-averaged chroma
        ycc = np.asarray(Image.fromarray(np.roll(base, 5 * k, axis=1)).resize((w, h), Image.BICUBIC).convert("YCbCr"), np.uint16)
        sub = (ycc[0::2, 0::2, 1:] + ycc[0::2, 1::2, 1:] + ycc[1::2, 0::2, 1:] + ycc[1::2, 1::2, 1:] + 2) >> 2
        planes.append(b"FRAME\n" + ycc[:, :, 0].astype(np.uint8).tobytes() + sub[:, :, 0].astype(np.uint8).tobytes() + sub[:, :, 1].astype(np.uint8).tobytes())
    for count in (n, n // 4):
        with open(os.path.join(d, "720p_%d.y4m" % count), "wb") as f:
            f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n" % (w, h))
            for k in range(count):
                f.write(planes[k % 16])
    parser = stylize_webcam.setup_parser()
    out = os.path.join(d, "out.y4m")
    second = ["--model_path2", os.path.join(root, "models", "candy_final.ckpt")]
    # (the fade covers the middle tenth of each run's own frames: nine tenths of either run cost one forward pass)
    legs = [("video_y4m_720p_one_model", lambda count: []),
            ("video_y4m_720p_two_models_style_mix_0.5", lambda count: second + ["--style_mix", "0.5"]),
            ("video_y4m_720p_two_models_mix_fade_middle_tenth", lambda count: second + ["--mix_fade", str(count * 9 // 20), str(count * 11 // 20)])]

    def run(count, flags):
        args = parser.parse_args(["--model_path", os.path.join(root, "models", "starry_final.ckpt"), "--video_in", os.path.join(d, "720p_%d.y4m" % count),
                                  "--video_out", out] + flags)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.time()
            stylize_webcam.run_video(args)
            dt = time.time() - t0
        assert os.path.getsize(out) > count * w * h * 3 // 2
        os.remove(out)
        return dt

    run(n // 4, [])                                               # warm-up: library load, first kernels
    times = {name: [] for name, _ in legs}
    res["legs"] = {}
    try:
        for _ in range(repeats):                                  # legs alternate: a drifting clock touches all of them alike
            for name, flags in legs:
                times[name].append((run(n, flags(n)), run(n // 4, flags(n // 4))))
                print("video_mix: %s: %.2f s for %d frames, %.2f s for %d" % ((name,) + (times[name][-1][0], n, times[name][-1][1], n // 4)), flush=True)
            for name, _ in legs:
                rates = sorted((n - n // 4) / (a - b) for a, b in times[name])
                res["legs"][name] = {"frames_per_s": rates[len(rates) // 2], "all_repeats": rates, "seconds_n_and_quarter": times[name]}
            save()
    finally:
        shutil.rmtree(d)
    for name, _ in legs:
        r = res["legs"][name]
        print("video_mix: %7.0f frames/s %s (repeats: %s)" % (r["frames_per_s"], name, ", ".join("%.0f" % v for v in r["all_repeats"])))
    return res


def temporal_kernel_times(W=1280, H=720, launches=200):
    """-> dict of device microseconds per 720p call of fs_temporal_f32 (luma, search and blend kernel back to back), timed as kernel_times does:
    a frame moved by (2, -3) against its predecessor at radius 7 and 3, and a first frame (no search, no blend)."""
    eng = engine.Engine()
    mem = eng.mem
    rng = np.random.default_rng(3)
    small = rng.uniform(0, 255, (H // 8, W // 8, 3)).astype(np.float32)
    a = np.ascontiguousarray(np.kron(small, np.ones((8, 8, 1), np.float32)) + rng.uniform(-4, 4, (H, W, 3)).astype(np.float32))
    src0, src1 = mem.from_numpy(a[None]), mem.from_numpy(np.roll(a, (2, -3), axis=(0, 1))[None])
    cur = mem.from_numpy(rng.uniform(0, 255, (1, H, W, 3)).astype(np.float32))
    dst = mem.empty((1, H, W, 3))
    s0, s1 = eng.temporal_state(H, W), eng.temporal_state(H, W)
    eng.temporal_f32(src0, cur, dst, s0)                          # the previous frame's state
    kw = dict(strength_q8=154, sensitivity=16, src_bgr=True)
    res = {"temporal_radius_7": kernel_timed(lambda: eng.temporal_f32(src1, cur, dst, s1, prev=s0, radius=7, **kw), launches),
           "temporal_radius_3": kernel_timed(lambda: eng.temporal_f32(src1, cur, dst, s1, prev=s0, radius=3, **kw), launches),
           "temporal_first_frame": kernel_timed(lambda: eng.temporal_f32(src1, cur, dst, s1, radius=7, **kw), launches)}
    for k, v in res.items():
        print("video: %8.1f us per 720p call (three launches): %s" % (v, k))
    return res


def temporal_pyr_kernel_times(W=1280, H=720, launches=200):
    """-> dict of device microseconds per 720p call of the temporal stage by level count, timed as kernel_times does: a frame moved by (20, -12)
    against its predecessor at radius 7 -- one level is fs_temporal_f32's three launches, two and three levels are fs_temporal_pyr_f32's 5 and 6
    -- and the share of interior blocks whose vector is the move."""
    eng = engine.Engine()
    mem = eng.mem
    rng = np.random.default_rng(3)
    small = rng.uniform(0, 255, (H // 8, W // 8, 3)).astype(np.float32)
    a = np.ascontiguousarray(np.kron(small, np.ones((8, 8, 1), np.float32)) + rng.uniform(-4, 4, (H, W, 3)).astype(np.float32))
    src0, src1 = mem.from_numpy(a[None]), mem.from_numpy(np.roll(a, (-20, 12), axis=(0, 1))[None])
    cur = mem.from_numpy(rng.uniform(0, 255, (1, H, W, 3)).astype(np.float32))
    dst = mem.empty((1, H, W, 3))
    kw = dict(strength_q8=154, sensitivity=16, src_bgr=True, radius=7)
    res = {}
    for levels in (1, 2, 3):
        s0, s1 = eng.temporal_state(H, W, levels), eng.temporal_state(H, W, levels)
        eng.temporal_f32(src0, cur, dst, s0, levels=levels, **kw)                 # the previous frame's state
        us = kernel_timed(lambda: eng.temporal_f32(src1, cur, dst, s1, prev=s0, levels=levels, **kw), launches)
        mv = np.array(mem.to_numpy(s1[2]), dtype=np.uint8, copy=True).view(np.int8)[2:-3, 1:-2]
        found = float(np.mean((mv[..., 0] == 20) & (mv[..., 1] == -12)))
        res["temporal_levels_%d" % levels] = {"us": us, "launches": 3 if levels == 1 else 3 + levels, "interior_blocks_at_20_-12": found}
        print("video: %8.1f us per 720p call, %3.0f %% of the interior blocks at (20, -12): %d level(s)" % (us, 100 * found, levels))
    return res


def temporal_subpel_kernel_times(W=1280, H=720, launches=200):
    """-> dict of device microseconds per 720p call of the temporal stage by (levels, subpel), timed as kernel_times does: a smooth frame moved
    by (2, -1) quarter pixels (bilinearly) against its predecessor at radius 7 -- subpel 0 at one level is fs_temporal_f32's three launches,
    the others are fs_temporal_sub_f32's -- and the share of interior blocks whose vector 4 mv + mvf is within one quarter unit of the move."""
    eng = engine.Engine()
    mem = eng.mem
    rng = np.random.default_rng(3)
    small = rng.uniform(0, 255, (H // 8, W // 8, 3)).astype(np.float32)
    a = np.kron(small, np.ones((8, 8, 1), np.float32))
    for axis in (0, 1):                                           # (smooth: the blocks of 8 x 8 under a box of 9)
        a = sum(np.roll(a, k, axis=axis) for k in range(-4, 5)) / np.float32(9)
    half = (a + np.roll(a, -1, axis=0)) * np.float32(0.5)         # moved[y][x] = a[y + 1/2][x - 1/4]
    moved = half * np.float32(0.75) + np.roll(half, 1, axis=1) * np.float32(0.25)
    noise = lambda: rng.uniform(-1, 1, (H, W, 3)).astype(np.float32)
    src0, src1 = mem.from_numpy(np.ascontiguousarray(a + noise())[None]), mem.from_numpy(np.ascontiguousarray(moved + noise())[None])
    cur = mem.from_numpy(rng.uniform(0, 255, (1, H, W, 3)).astype(np.float32))
    dst = mem.empty((1, H, W, 3))
    kw = dict(strength_q8=154, sensitivity=16, src_bgr=True, radius=7)
    res = {}
    for levels, subpel in ((1, 0), (1, 1), (1, 2), (3, 2)):
        more = dict(levels=levels, subpel=subpel) if subpel else dict(levels=levels)      # (subpel 0: the call of a lane without the key)
        s0, s1 = (eng.temporal_state(H, W, **more) for _ in range(2))
        eng.temporal_f32(src0, cur, dst, s0, **more, **kw)                            # the previous frame's state
        us = kernel_timed(lambda: eng.temporal_f32(src1, cur, dst, s1, prev=s0, **more, **kw), launches)
        q = 4 * np.array(mem.to_numpy(s1[2]), dtype=np.uint8, copy=True).view(np.int8).astype(np.int16)
        if subpel:
            q = q + np.array(mem.to_numpy(s1[-1]), dtype=np.uint8, copy=True).view(np.int8)
        q = q[1:-1, 1:-1]
        found = float(np.mean((np.abs(q[..., 0] - 2) <= 1) & (np.abs(q[..., 1] + 1) <= 1)))
        launches_per_call = (3 if levels == 1 else 3 + levels) + (1 if subpel else 0)
        res["temporal_levels_%d_subpel_%d" % (levels, subpel)] = {"us": us, "launches": launches_per_call, "interior_blocks_within_a_quarter_of_2_-1": found}
        print("video: %8.1f us per 720p call, %3.0f %% of the interior blocks within a quarter of (2, -1): %d level(s), subpel %d" %
              (us, 100 * found, levels, subpel))
    return res


def shortcut_share(mv, mvf, H, W):
    """The share of the overlapped blend's threads (four pixels of a row) whose four candidate blocks hold one vector 4 mv + mvf"""
    q = 4 * mv.astype(np.int64) + mvf
    nby, nbx = q.shape[:2]
    j0, i0 = (2 * np.arange(H) - 15) >> 5, (2 * np.arange(0, W, 4) - 15) >> 5
    rows, cols = [np.clip(j0 + k, 0, nby - 1) for k in (0, 1)], [np.clip(i0 + k, 0, nbx - 1) for k in (0, 1)]
    first = q[rows[0][:, None], cols[0][None, :]]
    return float(np.mean(np.all([np.all(q[r[:, None], c[None, :]] == first, axis=-1) for r in rows for c in cols], axis=0)))


def temporal_overlap_kernel_times(W=1280, H=720, launches=200, repeats=3):
    """-> dict of device microseconds per 720p call of the temporal stage at radius 7 and one level by (frame, subpel, overlap), timed as
    kernel_times does, `repeats` times with the twelve alternating: overlap 0 is the call of a lane without the key, the yardstick of the same
    run.  Frames: 'uniform' moved by (2, -3) as a whole, 'alternating' with the blocks of even and odd row + column moved by (0, 3) and (0, -3),
    'two_region' with the columns before 648 (mid-block) moved by (0, 3) and the others by (0, -3)."""
    eng = engine.Engine()
    mem = eng.mem
    rng = np.random.default_rng(3)
    small = rng.uniform(0, 255, (H // 8, W // 8, 3)).astype(np.float32)
    a = np.ascontiguousarray(np.kron(small, np.ones((8, 8, 1), np.float32)) + rng.uniform(-4, 4, (H, W, 3)).astype(np.float32))
    y, x = np.indices((H, W))
    left, right = np.roll(a, -3, axis=1), np.roll(a, 3, axis=1)       # what a shows at (y, x + 3) and at (y, x - 3)
    moved = {"uniform": np.roll(a, (-2, 3), axis=(0, 1)),
             "alternating": np.where(((((y >> 4) + (x >> 4)) & 1) == 0)[..., None], left, right),
             "two_region": np.where((x < 648)[..., None], left, right)}
    src0 = mem.from_numpy(a[None])
    cur = mem.from_numpy(rng.uniform(0, 255, (1, H, W, 3)).astype(np.float32))
    dst = mem.empty((1, H, W, 3))
    kw = dict(strength_q8=154, sensitivity=16, src_bgr=True, radius=7)
    runs = []
    for frame, pic in moved.items():
        src1 = mem.from_numpy(np.ascontiguousarray(pic)[None])
        for subpel in (0, 2):
            more = dict(subpel=subpel) if subpel else {}                                  # (subpel 0: the call of a lane without the key)
            s0, s1 = (eng.temporal_state(H, W, **more) for _ in range(2))
            eng.temporal_f32(src0, cur, dst, s0, **more, **kw)                            # the previous frame's state
            for overlap in (0, 1):
                over = dict(more, overlap=1) if overlap else more
                runs.append(("%s_subpel_%d_overlap_%d" % (frame, subpel, overlap), subpel,
                             lambda src1=src1, s0=s0, s1=s1, over=over: eng.temporal_f32(src1, cur, dst, s1, prev=s0, **over, **kw), s1))
    res = {name: {"us_repeats": [], "launches": 4 if subpel else 3} for name, subpel, _, _ in runs}
    for _ in range(repeats):
        for name, subpel, fn, s1 in runs:
            res[name]["us_repeats"].append(kernel_timed(fn, launches))
            if "shortcut_share" not in res[name]:
                mv = np.array(mem.to_numpy(s1[2]), dtype=np.uint8, copy=True).view(np.int8)
                mvf = np.array(mem.to_numpy(s1[-1]), dtype=np.uint8, copy=True).view(np.int8) if subpel else np.zeros_like(mv)
                res[name]["shortcut_share"] = shortcut_share(mv, mvf, H, W)
    for name, r in res.items():
        r["us"] = sorted(r["us_repeats"])[len(r["us_repeats"]) // 2]
        print("video: %8.1f us per 720p call (repeats: %s), %3.0f %% of the threads see one vector: %s" %
              (r["us"], ", ".join("%.1f" % u for u in r["us_repeats"]), 100 * r["shortcut_share"], name))
    return res


def temporal_batch_kernel_times(sizes=((720, 1280), (1080, 1920)), modes=((1, 0, 0), (3, 2, 1)), N=8, launches=200, repeats=3):
    """-> dict of device microseconds per frame of the temporal stage over N consecutive frames at radius 7 by (size, levels, subpel, overlap):
    'chained' N single-frame calls on two alternating slots (what a lane without sequence= runs), 'batched' one fs_temporal_batch_f32 call,
    both reading the state a previous frame left; timed as kernel_times does (a graph of `launches` repetitions of the N frames), `repeats`
    times with the two alternating.  The frames are one picture drifting by (1, -2) pixels per frame."""
    eng = engine.Engine()
    mem = eng.mem
    res = {}
    for H, W in sizes:
        rng = np.random.default_rng(3)
        small = rng.uniform(0, 255, (H // 8, W // 8, 3)).astype(np.float32)
        a = np.ascontiguousarray(np.kron(small, np.ones((8, 8, 1), np.float32)) + rng.uniform(-4, 4, (H, W, 3)).astype(np.float32))
        src = mem.from_numpy(np.stack([np.roll(a, (k, -2 * k), axis=(0, 1)) for k in range(1, N + 1)]))
        first = mem.from_numpy(a[None])
        cur = mem.from_numpy(rng.uniform(0, 255, (N, H, W, 3)).astype(np.float32))
        dst = mem.empty((N, H, W, 3))
        one = lambda t, i: mem.view(t, i * H * W * 3, (1, H, W, 3))
        for levels, subpel, overlap in modes:
            more = dict(dict(levels=levels), **dict(dict(subpel=subpel) if subpel else {}, **(dict(overlap=overlap) if overlap else {})))
            kw = dict(more, strength_q8=154, sensitivity=16, src_bgr=True, radius=7)
            slots = [eng.temporal_state(H, W, levels, subpel) for _ in range(2)]
            work = eng.temporal_batch_work(H, W, N, levels, subpel)
            eng.temporal_f32(first, one(cur, 0), one(dst, 0), slots[1], **kw)             # the state in front of frame 0 (N is even: slot 1 again)

            def chained():
                for i in range(N):
                    eng.temporal_f32(one(src, i), one(cur, i), one(dst, i), slots[i & 1], prev=slots[(i - 1) & 1], **kw)

            def batched():
                eng.temporal_batch_f32(src, cur, dst, slots[0], work, prev=slots[1], **kw)

            name = "%dp_levels_%d_subpel_%d_overlap_%d" % (H, levels, subpel, overlap)
            per_call = (2 + levels + (levels > 1) + (subpel > 0))
            r = res[name] = {"frames": N, "launches": {"chained": N * per_call, "batched": per_call - 1 + N},
                             "chained_us_per_frame_repeats": [], "batched_us_per_frame_repeats": []}
            for _ in range(repeats):
                r["chained_us_per_frame_repeats"].append(kernel_timed(chained, launches) / N)
                r["batched_us_per_frame_repeats"].append(kernel_timed(batched, launches) / N)
            for k in ("chained", "batched"):
                r[k + "_us_per_frame"] = sorted(r[k + "_us_per_frame_repeats"])[repeats // 2]
            print("video_batch: %7.1f us per frame chained (%s), %7.1f batched (%s): %s" %
                  (r["chained_us_per_frame"], ", ".join("%.1f" % u for u in r["chained_us_per_frame_repeats"]), r["batched_us_per_frame"],
                   ", ".join("%.1f" % u for u in r["batched_us_per_frame_repeats"]), name), flush=True)
    return res


def temporal_streams_kernel_times(sizes=((720, 1280), (1080, 1920)), modes=((1, 0, 0), (3, 2, 1)), S=8, launches=200, repeats=3):
    """-> dict of device microseconds per frame of the temporal stage over one frame of each of S independent streams at radius 7 by (size,
    levels, subpel, overlap): 'single' S single-frame calls, every stream on two slots of its own (what S batch-1 lanes run), 'streams' one
    fs_temporal_streams_f32 call on the one state buffer, both reading the state a previous frame of every stream left; timed as kernel_times
    does (a graph of `launches` repetitions of the S frames), `repeats` times with the two alternating.  Stream k's picture is the batch
    measurement's, drifting by (1, -2) pixels per frame, k frames further."""
    from faststyle_amd import _lib
    eng = engine.Engine()
    mem = eng.mem
    res = {}
    for H, W in sizes:
        rng = np.random.default_rng(3)
        small = rng.uniform(0, 255, (H // 8, W // 8, 3)).astype(np.float32)
        a = np.ascontiguousarray(np.kron(small, np.ones((8, 8, 1), np.float32)) + rng.uniform(-4, 4, (H, W, 3)).astype(np.float32))
        before = mem.from_numpy(np.stack([np.roll(a, (k, -2 * k), axis=(0, 1)) for k in range(S)]))
        src = mem.from_numpy(np.stack([np.roll(a, (k, -2 * k), axis=(0, 1)) for k in range(1, S + 1)]))
        cur = mem.from_numpy(rng.uniform(0, 255, (S, H, W, 3)).astype(np.float32))
        dst = mem.empty((S, H, W, 3))
        one = lambda t, i: mem.view(t, i * H * W * 3, (1, H, W, 3))
        for levels, subpel, overlap in modes:
            more = dict(dict(levels=levels), **dict(dict(subpel=subpel) if subpel else {}, **(dict(overlap=overlap) if overlap else {})))
            kw = dict(more, strength_q8=154, sensitivity=16, src_bgr=True, radius=7)
            slots = [[eng.temporal_state(H, W, levels, subpel) for _ in range(2)] for _ in range(S)]
            state = eng.temporal_streams_state(H, W, S, levels, subpel)
            first, then = eng.i32_buffer([_lib.FS_TS_SLOT] * S), eng.i32_buffer([_lib.FS_TS_PREV] * S)
            for i in range(S):                                                              # the state in front of every stream's frame: slot 1
                eng.temporal_f32(one(before, i), one(cur, i), one(dst, i), slots[i][1], **kw)
            eng.temporal_streams_f32(before, cur, dst, first, state, **kw)

            def single():
                for i in range(S):
                    eng.temporal_f32(one(src, i), one(cur, i), one(dst, i), slots[i][0], prev=slots[i][1], **kw)

            def streams():
                eng.temporal_streams_f32(src, cur, dst, then, state, **kw)

            name = "%dp_levels_%d_subpel_%d_overlap_%d" % (H, levels, subpel, overlap)
            per_call = (2 + levels + (levels > 1) + (subpel > 0))
            r = res[name] = {"streams": S, "launches": {"single": S * per_call, "streams": per_call},
                             "single_us_per_frame_repeats": [], "streams_us_per_frame_repeats": []}
            for _ in range(repeats):
                r["single_us_per_frame_repeats"].append(kernel_timed(single, launches) / S)
                r["streams_us_per_frame_repeats"].append(kernel_timed(streams, launches) / S)
            for k in ("single", "streams"):
                r[k + "_us_per_frame"] = sorted(r[k + "_us_per_frame_repeats"])[repeats // 2]
            print("video_streams: %7.1f us per frame single (%s), %7.1f streams (%s): %s" %
                  (r["single_us_per_frame"], ", ".join("%.1f" % u for u in r["single_us_per_frame_repeats"]), r["streams_us_per_frame"],
                   ", ".join("%.1f" % u for u in r["streams_us_per_frame_repeats"]), name), flush=True)
    return res


def video_streams(n, repeats=3, out_json=None):
    """-> dict: temporal_streams_kernel_times and the eight legs of the 1080p raw-video loop; prints them and writes
    profiles/video_streams.json (after the kernel times and after every repeat, so that a run that is cut short leaves what it measured)."""
    import contextlib
    import json
    import shutil
    from PIL import Image
    from faststyle_amd import build as fsbuild
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import stylize_webcam
    n = max(32, n // 32 * 32)
    w, h, S = 1920, 1080, 8
    dst = out_json or os.path.join(root, "profiles", "video_streams.json")
    res = {"frames": n, "streams": S, "frames_in_flight": 2, "host_threads": "1 driver", "host_cores": os.cpu_count(),
           "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
           "video": "1080p 4:2:0 YUV4MPEG2 (full range, BT.601), file to file of 8-bit 4:2:0; --video_also: 8 inputs of n / 8 frames, 8 outputs",
           "method": "rate = (n - n/4) / (t(n) - t(n/4)) over all streams' frames, median of %d alternating repeats" % repeats,
           "source_digest": fsbuild.source_digest(),
           "launch_count_estimate": {"streams": S, "levels": 3, "subpel": 2, "single": 56, "streams_call": 7,
                                     "note": "arithmetic of the launch counts, not a measurement: see stage_us_per_frame for the measurement"}}

    def save():
        with open(dst, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    res["stage_us_per_frame"] = temporal_streams_kernel_times()
    save()
    d = tempfile.mkdtemp()
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (135, 240, 3), dtype=np.uint8)
    planes = []
    for k in range(16):      # 16 distinct natural-ish frames (upsampled noise), reused; PIL's matrix, box-averaged chroma
        ycc = np.asarray(Image.fromarray(np.roll(base, 5 * k, axis=1)).resize((w, h), Image.BICUBIC).convert("YCbCr"), np.uint16)
        sub = (ycc[0::2, 0::2, 1:] + ycc[0::2, 1::2, 1:] + ycc[1::2, 0::2, 1:] + ycc[1::2, 1::2, 1:] + 2) >> 2
        planes.append(b"FRAME\n" + ycc[:, :, 0].astype(np.uint8).tobytes() + sub[:, :, 0].astype(np.uint8).tobytes() + sub[:, :, 1].astype(np.uint8).tobytes())

    def write(name, count, start=0):
        with open(os.path.join(d, name), "wb") as f:
            f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n" % (w, h))
            for k in range(count):
                f.write(planes[(start + k) % 16])

    for count in (n, n // 4):
        write("1080p_%d.y4m" % count, count)
        for s in range(S):                                        # (stream s starts s frames into the same pictures)
            write("1080p_%d_of_%d.y4m" % (s, count), count // S, s)
    parser = stylize_webcam.setup_parser()
    outs = [os.path.join(d, "out%d.y4m" % s) for s in range(S)]
    legs = [("video_y4m_1080p_%s_%s%s" % (kind, p, "_temporal_strength_0.6" if t else ""), kind, ["--precision", p] + (["--temporal_strength", "0.6"] if t else []))
            for t in (False, True) for p in ("fp32", "bf16") for kind in ("batch_8", "also_8")]

    def run(count, kind, flags):
        model = ["--model_path", os.path.join(root, "models", "starry_final.ckpt")]
        if kind == "also_8":
            io_ = ["--video_in", os.path.join(d, "1080p_0_of_%d.y4m" % count), "--video_out", outs[0]]
            for s in range(1, S):
                io_ += ["--video_also", os.path.join(d, "1080p_%d_of_%d.y4m" % (s, count)), outs[s]]
            written = outs
        else:
            io_ = ["--video_in", os.path.join(d, "1080p_%d.y4m" % count), "--video_out", outs[0], "--video_batch", "8"]
            written = outs[:1]
        args = parser.parse_args(model + io_ + flags)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.time()
            stylize_webcam.run_video(args)
            dt = time.time() - t0
        assert sum(os.path.getsize(o) for o in written) > count * w * h * 3 // 2
        for o in written:
            os.remove(o)
        return dt

    run(n // 4, "batch_8", [])                                    # warm-up: library load, first kernels
    times = {name: [] for name, _, _ in legs}
    res["legs"] = {}
    try:
        for _ in range(repeats):                                  # legs alternate: a drifting clock touches all of them alike
            for name, kind, flags in legs:
                times[name].append((run(n, kind, flags), run(n // 4, kind, flags)))
                print("video_streams: %s: %.2f s for %d frames, %.2f s for %d" % ((name,) + (times[name][-1][0], n, times[name][-1][1], n // 4)), flush=True)
            for name, _, _ in legs:
                rates = sorted((n - n // 4) / (a - b) for a, b in times[name])
                res["legs"][name] = {"frames_per_s": rates[len(rates) // 2], "all_repeats": rates, "seconds_n_and_quarter": times[name]}
            save()
    finally:
        shutil.rmtree(d)
    for name, _, _ in legs:
        r = res["legs"][name]
        print("video_streams: %7.0f frames/s %s (repeats: %s)" % (r["frames_per_s"], name, ", ".join("%.0f" % v for v in r["all_repeats"])))
    return res


def video_batch(n, repeats=3, out_json=None):
    """-> dict: temporal_batch_kernel_times and the eight legs of the 1080p raw-video loop; prints them and writes profiles/video_batch.json
    (after the kernel times and after every repeat, so that a run that is cut short leaves what it measured)."""
    import contextlib
    import json
    import shutil
    from PIL import Image
    from faststyle_amd import build as fsbuild
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import stylize_webcam
    n = max(32, n // 32 * 32)
    w, h = 1920, 1080
    dst = out_json or os.path.join(root, "profiles", "video_batch.json")
    res = {"frames": n, "frames_in_flight": 2, "host_threads": "1 driver", "host_cores": os.cpu_count(), "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
           "video": "1080p 4:2:0 YUV4MPEG2 (full range, BT.601), file to file of 8-bit 4:2:0",
           "method": "rate = (n - n/4) / (t(n) - t(n/4)), median of %d alternating repeats" % repeats, "source_digest": fsbuild.source_digest(),
           "launch_count_estimate": {"N": 8, "levels": 3, "subpel": 2, "chained": 56, "batched": 14,
                                     "note": "arithmetic of the launch counts, not a measurement: see stage_us_per_frame for the measurement"}}

    def save():
        with open(dst, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    res["stage_us_per_frame"] = temporal_batch_kernel_times()
    save()
    d = tempfile.mkdtemp()
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (135, 240, 3), dtype=np.uint8)
    planes = []
    for k in range(16):      # 16 distinct natural-ish frames (upsampled noise), reused; PIL's matrix, box-averaged chroma
        ycc = np.asarray(Image.fromarray(np.roll(base, 5 * k, axis=1)).resize((w, h), Image.BICUBIC).convert("YCbCr"), np.uint16)
        sub = (ycc[0::2, 0::2, 1:] + ycc[0::2, 1::2, 1:] + ycc[1::2, 0::2, 1:] + ycc[1::2, 1::2, 1:] + 2) >> 2
        planes.append(b"FRAME\n" + ycc[:, :, 0].astype(np.uint8).tobytes() + sub[:, :, 0].astype(np.uint8).tobytes() + sub[:, :, 1].astype(np.uint8).tobytes())
    for count in (n, n // 4):
        with open(os.path.join(d, "1080p_%d.y4m" % count), "wb") as f:
            f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n" % (w, h))
            for k in range(count):
                f.write(planes[k % 16])
    parser = stylize_webcam.setup_parser()
    out = os.path.join(d, "out.y4m")
    legs = [("video_y4m_1080p_batch_%d_%s%s" % (b, p, "_temporal_strength_0.6" if t else ""),
             ["--video_batch", str(b), "--precision", p] + (["--temporal_strength", "0.6"] if t else []))
            for t in (False, True) for p in ("fp32", "bf16") for b in (1, 8)]

    def run(count, flags):
        args = parser.parse_args(["--model_path", os.path.join(root, "models", "starry_final.ckpt"), "--video_in", os.path.join(d, "1080p_%d.y4m" % count),
                                  "--video_out", out] + flags)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.time()
            stylize_webcam.run_video(args)
            dt = time.time() - t0
        assert os.path.getsize(out) > count * w * h * 3 // 2
        os.remove(out)
        return dt

    run(n // 4, [])                                               # warm-up: library load, first kernels
    times = {name: [] for name, _ in legs}
    res["legs"] = {}
    try:
        for _ in range(repeats):                                  # legs alternate: a drifting clock touches all of them alike
            for name, flags in legs:
                times[name].append((run(n, flags), run(n // 4, flags)))
                print("video_batch: %s: %.2f s for %d frames, %.2f s for %d" % ((name,) + (times[name][-1][0], n, times[name][-1][1], n // 4)), flush=True)
            for name, _ in legs:
                rates = sorted((n - n // 4) / (a - b) for a, b in times[name])
                res["legs"][name] = {"frames_per_s": rates[len(rates) // 2], "all_repeats": rates, "seconds_n_and_quarter": times[name]}
            save()
    finally:
        shutil.rmtree(d)
    for name, _ in legs:
        r = res["legs"][name]
        print("video_batch: %7.0f frames/s %s (repeats: %s)" % (r["frames_per_s"], name, ", ".join("%.0f" % v for v in r["all_repeats"])))
    return res


def resample_kernel_times(launches=200):
    """-> dict of device microseconds per call of fs_resample_f32, timed as kernel_times does, with the bytes each call reads and writes."""
    eng = engine.Engine()
    mem = eng.mem
    rng = np.random.default_rng(4)
    small = mem.from_numpy(rng.uniform(0, 255, (1, 720, 1280, 3)).astype(np.float32))
    big = mem.from_numpy(rng.uniform(0, 255, (1, 2160, 3840, 3)).astype(np.float32))
    res = {}
    for name, src, dst, filt in (("720p_to_2160p_bicubic", small, big, "bicubic"), ("720p_to_2160p_lanczos", small, big, "lanczos"),
                                 ("2160p_to_720p_bicubic", big, small, "bicubic")):
        plan = eng.resample_plan(src.shape[1], src.shape[2], dst.shape[1], dst.shape[2], filt)
        out = mem.empty(tuple(dst.shape))
        us = kernel_timed(lambda: eng.resample_f32(src, plan, out), launches)
        nbytes = 4 * (int(np.prod(src.shape)) + int(np.prod(dst.shape)))
        res[name] = {"us": us, "bytes_read_and_written": nbytes, "GB_per_s": nbytes / us / 1e3, "tile_h": plan.tile_h,
                     "tile_rows": int(plan.info.tile_rows), "lds_rows": int(plan.info.lds_rows)}
        print("resample: %8.1f us per call, %6.0f GB/s of source + destination: %s" % (us, nbytes / us / 1e3, name))
    return res


def guided_kernel_times(launches=200):
    """-> dict of device microseconds per call of fs_guided_f32 (coef, mean and apply back to back), timed as kernel_times does, and of the
    bicubic fs_resample_f32 of the same enlargement, with the bytes each call reads and writes at least once."""
    eng = engine.Engine()
    mem = eng.mem
    rng = np.random.default_rng(5)
    H, W, Hd, Wd = 720, 1280, 2160, 3840
    lo_src = mem.from_numpy(rng.uniform(0, 255, (1, H, W, 3)).astype(np.float32))
    lo_out = mem.from_numpy(rng.uniform(0, 255, (1, H, W, 3)).astype(np.float32))
    hi = {"rgbx_u8": mem.upload_u8(rng.integers(0, 256, (1, Hd, Wd, 4), dtype=np.uint8)),
          "fp32": mem.from_numpy(rng.uniform(0, 255, (1, Hd, Wd, 3)).astype(np.float32))}
    out = mem.empty((1, Hd, Wd, 3))
    work = eng.guided_workspace(H, W, 1)
    res = {}
    for name, kind, radius in (("720p_to_2160p_radius2_rgbx_u8", "rgbx_u8", 2), ("720p_to_2160p_radius2_fp32", "fp32", 2),
                               ("720p_to_2160p_radius8_rgbx_u8", "rgbx_u8", 8)):
        us = kernel_timed(lambda: eng.guided_f32(lo_src, lo_out, hi[kind], out, work, radius=radius, smoothness=4), launches)
        low = 2 * 4 * H * W * 3 + 3 * H * W * 24                 # coef: the two tensors in, coef out; mean: coef in, mean out
        high = H * W * 24 + Hd * Wd * (4 if kind == "rgbx_u8" else 12) + Hd * Wd * 12      # apply: mean and the source in, the result out
        res[name] = {"us": us, "bytes_low_resolution_launches": low, "bytes_apply_launch": high, "GB_per_s_of_all": (low + high) / us / 1e3}
        print("guided: %8.1f us per call (three launches), %6.0f GB/s of everything read and written once: %s" % (us, (low + high) / us / 1e3, name))
    plan = eng.resample_plan(H, W, Hd, Wd, "bicubic")
    us = kernel_timed(lambda: eng.resample_f32(lo_out, plan, out), launches)
    nbytes = 4 * (H * W * 3 + Hd * Wd * 3)
    res["resample_720p_to_2160p_bicubic"] = {"us": us, "bytes_read_and_written": nbytes, "GB_per_s": nbytes / us / 1e3}
    print("guided: %8.1f us per call, %6.0f GB/s: fs_resample_f32 bicubic, the same enlargement" % (us, nbytes / us / 1e3))
    return res


def guided(n, repeats=3, out_json=None):
    """-> dict: guided_kernel_times and the two video legs; prints them and writes profiles/video_guided.json."""
    w, h = 3840, 2160
    legs = [("video_y4m_2160p_net_720p_out_2160p_bicubic", ["--output_size", "source"], w * h),
            ("video_y4m_2160p_net_720p_out_2160p_guided", ["--output_size", "source", "--output_guided"], w * h)]
    return resample(n, repeats, out_json, legs=legs, kernels=guided_kernel_times, tag="guided", default_json="video_guided.json")


def resample(n, repeats=3, out_json=None, legs=None, kernels=None, tag="resample", default_json="video_resample.json"):
    """-> dict: resample_kernel_times and the two video legs; prints them and writes profiles/video_resample.json (guided(): its own legs and
    kernel times, to profiles/video_guided.json)."""
    import contextlib
    import json
    import shutil
    from PIL import Image
    from faststyle_amd import build as fsbuild
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import stylize_webcam
    n = max(16, n // 4 * 4)
    w, h = 3840, 2160
    d = tempfile.mkdtemp()
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (135, 240, 3), dtype=np.uint8)
    planes = []
    for k in range(16):      # 16 distinct natural-ish frames (upsampled noise), reused; PIL's matrix, box-averaged chroma
        ycc = np.asarray(Image.fromarray(np.roll(base, 5 * k, axis=1)).resize((w, h), Image.BICUBIC).convert("YCbCr"), np.uint16)
        sub = (ycc[0::2, 0::2, 1:] + ycc[0::2, 1::2, 1:] + ycc[1::2, 0::2, 1:] + ycc[1::2, 1::2, 1:] + 2) >> 2
        planes.append(b"FRAME\n" + ycc[:, :, 0].astype(np.uint8).tobytes() + sub[:, :, 0].astype(np.uint8).tobytes() + sub[:, :, 1].astype(np.uint8).tobytes())
    for count in (n, n // 4):
        with open(os.path.join(d, "2160p_%d.y4m" % count), "wb") as f:
            f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n" % (w, h))
            for k in range(count):
                f.write(planes[k % 16])
    parser = stylize_webcam.setup_parser()
    out = os.path.join(d, "out.y4m")
    legs = legs or [("video_y4m_2160p_net_720p_out_720p", [], 1280 * 720), ("video_y4m_2160p_net_720p_out_2160p_bicubic", ["--output_size", "source"], w * h)]

    def run(count, flags, pixels):
        args = parser.parse_args(["--model_path", os.path.join(root, "models", "starry_final.ckpt"), "--video_in", os.path.join(d, "2160p_%d.y4m" % count),
                                  "--video_out", out, "--frame_size", "1280", "720"] + flags)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.time()
            stylize_webcam.run_video(args)
            dt = time.time() - t0
        assert os.path.getsize(out) > count * pixels * 3 // 2
        os.remove(out)
        return dt

    run(n // 4, [], 1280 * 720)                                   # warm-up: library load, first kernels
    times = {name: [] for name, _, _ in legs}
    for _ in range(repeats):                                      # legs alternate: a drifting clock touches both alike
        for name, flags, pixels in legs:
            times[name].append((run(n, flags, pixels), run(n // 4, flags, pixels)))
            print("%s: %s: %.2f s for %d frames, %.2f s for %d" % ((tag, name) + (times[name][-1][0], n, times[name][-1][1], n // 4)), flush=True)
    shutil.rmtree(d)
    res = {"frames": n, "frames_in_flight": 2, "host_threads": "1 driver", "host_cores": os.cpu_count(), "omp_num_threads": os.environ.get("OMP_NUM_THREADS"),
           "video": "2160p 4:2:0 YUV4MPEG2 (full range, BT.601) from a file, --frame_size 1280 720, to a file of 8-bit 4:2:0",
           "method": "rate = (n - n/4) / (t(n) - t(n/4)), median of %d alternating repeats" % repeats, "source_digest": fsbuild.source_digest(), "legs": {}}
    for name, _, _ in legs:
        rates = sorted((n - n // 4) / (a - b) for a, b in times[name])
        res["legs"][name] = {"frames_per_s": rates[len(rates) // 2], "all_repeats": rates, "seconds_n_and_quarter": times[name]}
        print("%s: %7.0f frames/s %s (repeats: %s)" % (tag, rates[len(rates) // 2], name, ", ".join("%.0f" % r for r in rates)))
    res["kernel_per_call"] = (kernels or resample_kernel_times)()
    with open(out_json or os.path.join(root, "profiles", default_json), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


def frames_in(n, repeats=3, out_json=None, video=False, depth=None, compose=False, temporal=False, temporal_levels=False, temporal_subpel=False,
              temporal_overlap=False):
    """-> dict of the legs' rates (frames/s); prints them and writes profiles/frames_in.json (video: with the raw-video leg, to
    profiles/video_stream.json; video with a depth: the 8-bit and the deep raw-video legs alone, to profiles/video_deep.json; video with
    compose / temporal: the 8-bit raw-video leg without and with that stage, to profiles/video_compose.json / video_temporal.json)."""
    compose_flag, compose = compose, compose or temporal or temporal_levels or temporal_subpel or temporal_overlap      # (the stages share the two-leg scheme)
    import contextlib
    import json
    import shutil
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import stylize_webcam
    n = max(16, n // 4 * 4)
    d = tempfile.mkdtemp()
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, (135, 240, 3), dtype=np.uint8)
    dirs = {}
    for tag, (w, h) in (("720p", (1280, 720)), ("1080p", (1920, 1080))):
        if (depth or compose) and tag != "720p":          # (the two video legs alone: no 1080p sources, no directories of JPEG frames)
            continue
        files = []
        planes = []
        deep_planes = []
        for k in range(16):      # 16 distinct natural-ish frames (upsampled noise), reused
            buf = io.BytesIO()
            im = Image.fromarray(np.roll(base, 5 * k, axis=1)).resize((w, h), Image.BICUBIC)
            im.save(buf, "JPEG", quality=90)
            files.append(buf.getvalue())
            if video and tag == "720p":      # the same frame as 4:2:0 planes (PIL's matrix, box-averaged chroma: the content only has to be plausible)
                ycc = np.asarray(im.convert("YCbCr"), np.uint16)
                sub = (ycc[0::2, 0::2, 1:] + ycc[0::2, 1::2, 1:] + ycc[1::2, 0::2, 1:] + ycc[1::2, 1::2, 1:] + 2) >> 2
                planes.append(b"FRAME\n" + ycc[:, :, 0].astype(np.uint8).tobytes() + sub[:, :, 0].astype(np.uint8).tobytes() +
                              sub[:, :, 1].astype(np.uint8).tobytes())
                if depth:                    # ... and as samples of `depth` bits: the 8-bit value's bits repeated below it, so that the low bits are used
                    deep = [((p.astype(np.uint32) * 257) >> (16 - depth)).astype("<u2") for p in (ycc[:, :, 0], sub[:, :, 0], sub[:, :, 1])]
                    deep_planes.append(b"FRAME\n" + b"".join(p.tobytes() for p in deep))
        for count in () if depth or compose else (n, n // 4):
            p = os.path.join(d, "%s_%d" % (tag, count))
            os.makedirs(p)
            for k in range(count):
                with open(os.path.join(p, "f%05d.jpg" % k), "wb") as f:
                    f.write(files[k % 16])
            dirs[tag, count] = p
        for count in (n, n // 4) if planes else ():
            with open(os.path.join(d, "%s_%d.y4m" % (tag, count)), "wb") as f:
                f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n" % (w, h))
                for k in range(count):
                    f.write(planes[k % 16])
            if deep_planes:
                with open(os.path.join(d, "%s_%d_p%d.y4m" % (tag, count, depth)), "wb") as f:
                    f.write(b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C420p%d XCOLORRANGE=FULL\n" % (w, h, depth))
                    for k in range(count):
                        f.write(deep_planes[k % 16])
        print("frames_in: %s sources, %.0f KB/file" % (tag, np.mean([len(f) for f in files]) / 1e3))
    legs = [("pil_decode_720p", "720p", []),
            ("native_decode_720p", "720p", ["--input_decode", "native"]),
            ("pil_decode_pil_resize_1080p_to_720p", "1080p", ["--resolution", "1280", "720"]),
            ("native_decode_device_resize_1080p_to_720p", "1080p", ["--input_decode", "native", "--frame_size", "1280", "720"]),
            ("pil_decode_device_resize_1080p_to_720p", "1080p", ["--frame_size", "1280", "720"])]
    if video:
        legs.append(("video_y4m_720p", "720p", None))
    if depth:
        legs = [("video_y4m_720p", "720p", None), ("video_y4m_720p_%dbit" % depth, "720p", depth)]
    if compose:
        legs = [("video_y4m_720p", "720p", None), ("video_y4m_720p_strength_0.7_preserve_color", "720p", ("--style_strength", "0.7", "--preserve_color"))]
    if temporal:
        legs = [("video_y4m_720p", "720p", None), ("video_y4m_720p_temporal_strength_0.6", "720p", ("--temporal_strength", "0.6"))]
    if temporal_levels:
        legs = [("video_y4m_720p_temporal_strength_0.6", "720p", ("--temporal_strength", "0.6")),
                ("video_y4m_720p_temporal_strength_0.6_levels_3", "720p", ("--temporal_strength", "0.6", "--temporal_levels", "3"))]
    if temporal_subpel:
        legs = [("video_y4m_720p_temporal_strength_0.6", "720p", ("--temporal_strength", "0.6")),
                ("video_y4m_720p_temporal_strength_0.6_subpel_2", "720p", ("--temporal_strength", "0.6", "--temporal_subpel", "2"))]
    if temporal_overlap:
        legs = [("video_y4m_720p_temporal_strength_0.6", "720p", ("--temporal_strength", "0.6")),
                ("video_y4m_720p_temporal_strength_0.6_overlap_1", "720p", ("--temporal_strength", "0.6", "--temporal_overlap", "1"))]
    parser = stylize_webcam.setup_parser()
    out = os.path.join(d, "out")

    def run_stream(tag, count, bits=None, extra=()):
        """the raw-video loop over count frames, file to file (bits: the deep stream, taken and written at its own depth; extra: more flags)"""
        src = "%s_%d_p%d.y4m" % (tag, count, bits) if bits else "%s_%d.y4m" % (tag, count)
        args = parser.parse_args(["--model_path", os.path.join(root, "models", "starry_final.ckpt"), "--video_in", os.path.join(d, src),
                                  "--video_out", out + ".y4m"] + (["--video_depth", "stream"] if bits else []) + list(extra))
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.time()
            stylize_webcam.run_video(args)
            dt = time.time() - t0
        assert os.path.getsize(out + ".y4m") > count * 1280 * 720 * 3 // 2 * (2 if bits else 1)
        os.remove(out + ".y4m")
        return dt

    def run(tag, count, flags):
        if flags is None or isinstance(flags, int):
            return run_stream(tag, count, flags)
        if isinstance(flags, tuple):
            return run_stream(tag, count, extra=flags)
        args = parser.parse_args(["--model_path", os.path.join(root, "models", "starry_final.ckpt"), "--frames_dir", dirs[tag, count],
                                  "--output_dir", out, "--output_format", "jpg"] + flags)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.time()
            stylize_webcam.run_frames_dir(args)
            dt = time.time() - t0
        assert len(os.listdir(out)) == count
        shutil.rmtree(out)
        return dt

    run("720p", n // 4, None if depth or compose else [])                    # warm-up: library load, first kernels
    times = {name: [] for name, _, _ in legs}
    for _ in range(repeats):                                      # legs alternate: a drifting clock touches all of them alike
        for name, tag, flags in legs:
            times[name].append((run(tag, n, flags), run(tag, n // 4, flags)))
            print("frames_in: %s: %.2f s for %d frames, %.2f s for %d" % ((name,) + (times[name][-1][0], n, times[name][-1][1], n // 4)), flush=True)
    res = {"frames": n, "frames_in_flight": 2, "host_threads": "1 driver + 4 decode / encode",
           "host_cores": os.cpu_count(), "omp_num_threads": os.environ.get("OMP_NUM_THREADS"), "output": "jpg quality 95 4:2:0",
           "method": "rate = (n - n/4) / (t(n) - t(n/4)), median of %d alternating repeats" % repeats, "legs": {}}
    if video:
        res["video"] = "720p 4:2:0 YUV4MPEG2 (full range, BT.601), file to file; 1 driver thread, no decode / encode threads"
    if depth:
        res["output"] = "YUV4MPEG2 at the input's depth"
        res["host_threads"] = "1 driver"
        res["deep_bits"] = depth
        res["bytes_per_frame_in_and_out"] = {"video_y4m_720p": 1280 * 720 * 3 // 2, "video_y4m_720p_%dbit" % depth: 1280 * 720 * 3}
        from faststyle_amd import build as fsbuild
        res["source_digest"] = fsbuild.source_digest()
    if compose:
        res["output"] = "YUV4MPEG2, 8 bits"
        res["host_threads"] = "1 driver"
        from faststyle_amd import build as fsbuild
        res["source_digest"] = fsbuild.source_digest()
    for name, _, _ in legs:
        rates = sorted((n - n // 4) / (a - b) for a, b in times[name])
        res["legs"][name] = {"frames_per_s": rates[len(rates) // 2], "all_repeats": rates, "seconds_n_and_quarter": times[name]}
        print("frames_in: %7.0f frames/s %s (repeats: %s)" % (rates[len(rates) // 2], name, ", ".join("%.0f" % r for r in rates)))
    shutil.rmtree(d)
    if depth:
        res["kernel_us_per_720p_launch"] = kernel_times(depth)
    if compose_flag:
        res["kernel_us_per_720p_launch"] = compose_kernel_times()
    if temporal:
        res["kernel_us_per_720p_call_of_three_launches"] = temporal_kernel_times()
    if temporal_levels:
        res["kernel_us_per_720p_call_by_levels"] = temporal_pyr_kernel_times()
    if temporal_subpel:
        res["kernel_us_per_720p_call_by_levels_and_subpel"] = temporal_subpel_kernel_times()
    if temporal_overlap:
        res["kernel_us_per_720p_call_by_frame_subpel_and_overlap"] = temporal_overlap_kernel_times()
    dst = out_json or os.path.join(root, "profiles", "video_temporal_overlap.json" if temporal_overlap else "video_temporal_subpel.json" if temporal_subpel else "video_temporal_pyr.json" if temporal_levels else "video_temporal.json" if temporal else "video_compose.json" if compose else "video_deep.json" if depth else "video_stream.json" if video else "frames_in.json")
    with open(dst, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


def main():
    from PIL import Image
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    threads = int(sys.argv[2]) if len(sys.argv) > 2 else None
    if len(sys.argv) > 5 and sys.argv[3] == "video" and sys.argv[5] == "batch":
        video_batch(n, out_json=sys.argv[4])
        return
    if len(sys.argv) > 5 and sys.argv[3] == "video" and sys.argv[5] == "streams":
        video_streams(n, out_json=sys.argv[4])
        return
    if len(sys.argv) > 3 and sys.argv[3] == "video_streams_kernels":
        temporal_streams_kernel_times(sizes=((720, 1280),), modes=((3, 2, 1),), repeats=1)
        return
    if len(sys.argv) > 5 and sys.argv[3] == "video" and sys.argv[5] == "mix":
        video_mix(n, out_json=sys.argv[4])
        return
    if len(sys.argv) > 3 and sys.argv[3] == "mix_kernels":
        mix_kernel_times()
        return
    if len(sys.argv) > 3 and sys.argv[3] == "video_batch_kernels":
        temporal_batch_kernel_times(sizes=((720, 1280),), modes=((3, 2, 1),), repeats=1)
        return
    if len(sys.argv) > 3 and sys.argv[3] in ("frames_in", "video"):
        fifth = sys.argv[5] if len(sys.argv) > 5 and sys.argv[3] == "video" else None
        frames_in(n, out_json=sys.argv[4] if len(sys.argv) > 4 else None, video=sys.argv[3] == "video",
                  depth=int(fifth) if fifth not in (None, "compose", "temporal", "temporal_levels", "temporal_subpel", "temporal_overlap") else None,
                  compose=fifth == "compose", temporal=fifth == "temporal", temporal_levels=fifth == "temporal_levels",
                  temporal_subpel=fifth == "temporal_subpel", temporal_overlap=fifth == "temporal_overlap")
        return
    if len(sys.argv) > 3 and sys.argv[3] == "temporal_overlap_kernels":
        temporal_overlap_kernel_times()
        return
    if len(sys.argv) > 3 and sys.argv[3] == "temporal_subpel_kernels":
        temporal_subpel_kernel_times()
        return
    if len(sys.argv) > 3 and sys.argv[3] == "temporal_pyr_kernels":
        temporal_pyr_kernel_times()
        return
    if len(sys.argv) > 3 and sys.argv[3] == "resample":
        resample(n, out_json=sys.argv[4] if len(sys.argv) > 4 else None)
        return
    if len(sys.argv) > 3 and sys.argv[3] == "guided":
        guided(n, out_json=sys.argv[4] if len(sys.argv) > 4 else None)
        return
    if len(sys.argv) > 3 and sys.argv[3] == "guided_kernels":
        guided_kernel_times()
        return
    if len(sys.argv) > 3 and sys.argv[3] == "temporal_kernels":
        temporal_kernel_times()
        return
    if len(sys.argv) > 3 and sys.argv[3] == "host_encode":
        host_encode(n, threads or 4)
        return
    rng = np.random.default_rng(0)
    d = tempfile.mkdtemp()
    base = rng.integers(0, 256, (60, 80, 3), dtype=np.uint8)
    jpegs = []
    for k in range(16):      # 16 distinct natural-ish images (upsampled noise + gradient), reused
        im = Image.fromarray(np.roll(base, k, axis=1)).resize((640, 480), Image.BICUBIC)
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=90)
        jpegs.append(buf.getvalue())
    files = []
    for s in range(4):
        p = os.path.join(d, "train-%05d-of-00004" % s)
        with tfrecord.RecordWriter(p) as w:
            for k in range(n // 4):
                w.write(tfrecord.encode_example({"image/encoded": jpegs[k % 16], "image/height": 480, "image/width": 640,
                                                 "image/channels": 3}))
        files.append(p)
    print("shards: %d images, %.1f KB/jpeg" % (n, np.mean([len(j) for j in jpegs]) / 1e3))
    if len(sys.argv) > 3 and sys.argv[3] == "host_native":
        th = threads or 24
        host, arena = engine.JpegHost(), datapipe.CoefArena(None, False)
        t0 = time.time()
        k = fallback = 0
        for r in datapipe._prefetch_map(lambda job: datapipe._native_decode(host, job),
                                        datapipe._native_jobs(host, arena, datapipe._examples(files, 1, np.random.default_rng(0))), th, window=4 * th):
            slot = r if isinstance(r, datapipe.CoefSlot) else r[1]
            fallback += not isinstance(r, datapipe.CoefSlot)
            if slot is not None:
                slot.release()
            k += 1
        dt = time.time() - t0
        print("pipeline: %.0f images/s host half only, native entropy decode (%d images, %d of them through PIL, in %.2f s, %d decode threads, %d host cores)"
              % (k / dt, k, fallback, dt, th, os.cpu_count()))
        it = datapipe._prefetch_map(lambda d: datapipe.decode_jpeg(d, packed=False), datapipe._examples(files, 1, np.random.default_rng(0)), th, window=4 * th)
        t0 = time.time()
        k = sum(1 for _ in it)
        dt = time.time() - t0
        print("pipeline: %.0f images/s host half only, PIL decode (%d images in %.2f s, %d decode threads, %d host cores)" % (k / dt, k, dt, th, os.cpu_count()))
        return
    if len(sys.argv) > 3 and sys.argv[3] == "host":
        th = threads or 24
        it = datapipe._prefetch_map(datapipe.decode_jpeg, datapipe._examples(files, 1, np.random.default_rng(0)), th, window=4 * th)
        t0 = time.time()
        k = sum(1 for _ in it)
        dt = time.time() - t0
        print("pipeline: %.0f images/s host half only (%d images decoded in %.2f s, %d decode threads, %d host cores)" % (k / dt, k, dt, th, os.cpu_count()))
        return
    eng = engine.Engine()
    import torch
    it = datapipe.batcher(files, 4, (256, 256), num_epochs=1, min_after_dequeue=256, engine=eng, num_threads=threads)
    next(it)
    torch.cuda.synchronize()
    t0 = time.time()
    nb = 0
    for b in it:
        nb += 1
    torch.cuda.synchronize()
    dt = time.time() - t0
    print("pipeline: %.0f images/s (%d batches of 4 in %.2f s, %s decode threads, %d host cores)" %
          (nb * 4 / dt, nb, dt, threads or "auto", os.cpu_count()))


if __name__ == "__main__":
    main()
