#!/usr/bin/env python
"""Throughput of the TFRecord input pipeline alone (decode threads + GPU resize + HBM shuffle queue) on
synthetic COCO-like shards (640x480 JPEG quality 90).  usage: pipe_bench.py [n_images] [threads] [host | host_native | host_encode | frames_in | video]
"frames_in": the frames-dir loop end to end (stylize_webcam.run_frames_dir, two frames in flight, --output_format jpg) at 720p over a directory of
n JPEG frames: PIL decode against --input_decode native, and from 1080p sources PIL decode + PIL resize (--resolution) against native decode +
device resize (--frame_size).  Every leg runs on the same device, legs alternate over the repeats, and a leg's rate is taken from the DIFFERENCE
between its run over n frames and its run over n / 4 frames, so that engine start-up, checkpoint load and graph capture drop out; written to
profiles/frames_in.json (or to the file named as a fourth argument).
"video": the frames_in legs and, beside them in the same run with the same repeat and median scheme, the raw-video loop (stylize_webcam.run_video:
--video_in / --video_out, 720p 4:2:0 YUV4MPEG2 from a file to a file, the same 16 frames as planes, the same frame counts); written to profiles/video_stream.json.  The video loop is several times faster than the
others: give it enough frames (1280) that its timed difference is about a second.
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


def frames_in(n, repeats=3, out_json=None, video=False):
    """-> dict of the legs' rates (frames/s); prints them and writes profiles/frames_in.json (video: with the raw-video leg, to
    profiles/video_stream.json)."""
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
        files = []
        planes = []
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
        for count in (n, n // 4):
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
        print("frames_in: %s sources, %.0f KB/file" % (tag, np.mean([len(f) for f in files]) / 1e3))
    legs = [("pil_decode_720p", "720p", []),
            ("native_decode_720p", "720p", ["--input_decode", "native"]),
            ("pil_decode_pil_resize_1080p_to_720p", "1080p", ["--resolution", "1280", "720"]),
            ("native_decode_device_resize_1080p_to_720p", "1080p", ["--input_decode", "native", "--frame_size", "1280", "720"]),
            ("pil_decode_device_resize_1080p_to_720p", "1080p", ["--frame_size", "1280", "720"])]
    if video:
        legs.append(("video_y4m_720p", "720p", None))
    parser = stylize_webcam.setup_parser()
    out = os.path.join(d, "out")

    def run_stream(tag, count):
        """the raw-video loop over count frames, file to file"""
        args = parser.parse_args(["--model_path", os.path.join(root, "models", "starry_final.ckpt"), "--video_in", os.path.join(d, "%s_%d.y4m" % (tag, count)),
                                  "--video_out", out + ".y4m"])
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.time()
            stylize_webcam.run_video(args)
            dt = time.time() - t0
        assert os.path.getsize(out + ".y4m") > count * 1280 * 720 * 3 // 2
        os.remove(out + ".y4m")
        return dt

    def run(tag, count, flags):
        if flags is None:
            return run_stream(tag, count)
        args = parser.parse_args(["--model_path", os.path.join(root, "models", "starry_final.ckpt"), "--frames_dir", dirs[tag, count],
                                  "--output_dir", out, "--output_format", "jpg"] + flags)
        with contextlib.redirect_stdout(io.StringIO()):
            t0 = time.time()
            stylize_webcam.run_frames_dir(args)
            dt = time.time() - t0
        assert len(os.listdir(out)) == count
        shutil.rmtree(out)
        return dt

    run("720p", n // 4, [])                                       # warm-up: library load, first kernels
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
    for name, _, _ in legs:
        rates = sorted((n - n // 4) / (a - b) for a, b in times[name])
        res["legs"][name] = {"frames_per_s": rates[len(rates) // 2], "all_repeats": rates, "seconds_n_and_quarter": times[name]}
        print("frames_in: %7.0f frames/s %s (repeats: %s)" % (rates[len(rates) // 2], name, ", ".join("%.0f" % r for r in rates)))
    shutil.rmtree(d)
    dst = out_json or os.path.join(root, "profiles", "video_stream.json" if video else "frames_in.json")
    with open(dst, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


def main():
    from PIL import Image
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    threads = int(sys.argv[2]) if len(sys.argv) > 2 else None
    if len(sys.argv) > 3 and sys.argv[3] in ("frames_in", "video"):
        frames_in(n, out_json=sys.argv[4] if len(sys.argv) > 4 else None, video=sys.argv[3] == "video")
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
