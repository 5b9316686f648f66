#!/usr/bin/env python
"""What train.py reaches end to end, against what bench.py times (profiles/train_e2e.json).

Legs, each at batch 4 and batch 32, 256 x 256, every one a child process of its own under ``timeout -k 10`` (a leg that fails ends the run:
nothing is started on the GPU after it):
  pool           Trainer.step over a pool of device-resident batches, the way bench.py feeds it -- the yardstick
  synth_device   train.main --train_dir synthetic:device
  synth_host     train.main --train_dir synthetic (fewer steps: the host draws each batch with numpy)
  shards         train.main over generated TFRecord shards (640 x 480 JPEGs), FS_FEED_DEPTH at its default
  shards_sync    the same with FS_FEED_DEPTH=0
  shards_jpeg    the same as shards with FS_FEED_JPEG=1: the library's JPEG decoder (Huffman pass on the decode threads, the rest on the GPU)
plus ``decode`` (host only: the JPEG decode rate of the pool of threads that bounds the shard legs), ``decode_native`` (the same pool running the
library's Huffman pass instead of PIL) and ``kernels`` (HIP-event time per launch
of the three kernels of csrc/fs_feed.hip at the batch-32 training shapes).

A train.main leg is timed from inside: Trainer.step is wrapped, the clock starts at a device synchronise before step ``warmup`` and stops at one
before step ``warmup + steps`` -- so the interval holds ``steps`` whole iterations of the script's loop (input path, step, the loss read-back every
tenth step).  Rates on a shared machine are recorded, not gated.

    python tools/train_e2e.py --out profiles/train_e2e.json
    python tools/train_e2e.py --only shards,shards_jpeg --out somewhere.json      (the pool leg and the named train.main legs only)
"""
import argparse
import io
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STYLE = os.path.join(ROOT, "style_images", "starry_night_crop.jpg")
SIZE = 256


def make_shards(directory, n_images, n_shards, seed=0):
    """The recipe of tests/test_datapipe.py::make_shards at MS-COCO-like sizes: smooth colour fields with low-pass texture, 640 x 480 and
    480 x 640, JPEG quality 90."""
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from faststyle_amd import tfrecord
    rng = np.random.default_rng(seed)
    seeds = rng.integers(0, 2 ** 31, n_images)

    def encode(k):
        r = np.random.default_rng(int(seeds[k]))
        h, w = ((480, 640), (640, 480), (427, 640), (480, 500))[k % 4]
        low = Image.fromarray(r.integers(0, 256, (h // 8, w // 8, 3), dtype=np.uint8)).resize((w, h), Image.BICUBIC)
        arr = np.asarray(low, dtype=np.float32) * 0.7 + r.uniform(0, 255, (1, 1, 3)) * np.linspace(0.3, 1, w)[None, :, None] * 0.3
        arr = np.clip(arr + r.normal(0, 6, (h, w, 1)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(arr).save(buf, "JPEG", quality=90)
        return tfrecord.encode_example({"image/encoded": buf.getvalue(), "image/height": h, "image/width": w, "image/channels": 3,
                                        "image/colorspace": b"RGB", "image/format": b"JPEG", "image/filename": b"%d.jpg" % k})
    with ThreadPoolExecutor(max_workers=16) as ex:
        records = list(ex.map(encode, range(n_images)))
    for s in range(n_shards):
        with tfrecord.RecordWriter(os.path.join(directory, "train-%05d-of-%05d" % (s, n_shards))) as w:
            for rec in records[s::n_shards]:
                w.write(rec)
    return sum(len(r) for r in records) / float(n_images)


def timed_main(argv, warmup, steps, batch):
    """train.main(argv) with Trainer.step wrapped: images/s over steps [warmup, warmup + steps)."""
    import torch
    import train
    from faststyle_amd import trainer
    mark = {"n": 0, "t0": None, "t1": None}
    real = trainer.Trainer.step

    def step(self, b):
        if mark["n"] == warmup:
            torch.cuda.synchronize()
            mark["t0"] = time.perf_counter()
        elif mark["n"] == warmup + steps:
            torch.cuda.synchronize()
            mark["t1"] = time.perf_counter()
        mark["n"] += 1
        return real(self, b)
    trainer.Trainer.step = step
    try:
        train.main(train.setup_parser().parse_args(argv + ["--num_steps_break", str(warmup + steps)]))
    finally:
        trainer.Trainer.step = real
    if mark["t1"] is None:
        raise SystemExit("the run ended after %d steps, before the %d timed ones were done" % (mark["n"], steps))
    dt = mark["t1"] - mark["t0"]
    return {"images_per_s": steps * batch / dt, "ms_per_step": 1e3 * dt / steps, "steps": steps, "warmup": warmup}


def leg_pool(batch, steps, warmup):
    import torch
    from faststyle_amd import engine, im_transf_net, trainer, utils, vgg16
    eng = engine.Engine()
    g = torch.Generator(device="cuda")
    g.manual_seed(100)
    style = utils.imread(STYLE).astype(np.float32)[None]
    tr = trainer.Trainer(eng, eng.flatten_params(im_transf_net.initial_variables(seed=0), scope=""), vgg16.synthetic_weights(seed=3), style,
                         use_graph=True)
    pool = [torch.rand((batch, SIZE, SIZE, 3), device="cuda", generator=g) * 255.0 for _ in range(4)]
    for i in range(max(warmup, 2)):
        tr.step(pool[i % 4])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        tr.step(pool[i % 4])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"images_per_s": steps * batch / dt, "ms_per_step": 1e3 * dt / steps, "steps": steps, "warmup": max(warmup, 2)}


def leg_train(kind, batch, steps, warmup, shard_dir):
    from faststyle_amd import vgg16
    work = tempfile.mkdtemp(prefix="train_e2e_")
    os.makedirs(os.path.join(work, "libs"))
    np.savez(os.path.join(work, "libs", "vgg16_weights.npz"), **vgg16.synthetic_weights(3))
    os.chdir(work)
    argv = ["--model_name", "e2e", "--style_img_path", STYLE, "--preprocess_size", str(SIZE), str(SIZE), "--batch_size", str(batch),
            "--num_steps_ckpt", "1000000"]
    if kind in ("shards", "shards_sync", "shards_jpeg"):
        argv += ["--train_dir", shard_dir, "--n_epochs", "1000", "--num_pipe_buffer", "512"]
    else:
        argv += ["--train_dir", "synthetic:device" if kind == "synth_device" else "synthetic"]
    return timed_main(argv, warmup, steps, batch)


def leg_decode(shard_dir, threads, seconds=4.0):
    import glob
    from faststyle_amd import datapipe
    files = sorted(glob.glob(os.path.join(shard_dir, "train-*")))
    rng = np.random.default_rng(0)
    it = datapipe._prefetch_map(lambda d: datapipe.decode_jpeg(d, packed=False), datapipe._examples(files, None, rng), threads, window=4 * threads)
    for _ in range(2 * threads):
        next(it)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        next(it)
        n += 1
    dt = time.perf_counter() - t0
    it.close()
    return {"images_per_s": n / dt, "threads": threads, "note": "framing + Example lookup + PIL decode on the batcher's own thread pool, no GPU"}


def leg_decode_native(shard_dir, threads, seconds=4.0):
    """leg_decode with fs_jpeg_parse + fs_jpeg_decode in place of PIL: the host half of the native path, at the same thread count."""
    import glob
    from faststyle_amd import datapipe, engine
    files = sorted(glob.glob(os.path.join(shard_dir, "train-*")))
    rng = np.random.default_rng(0)
    host = engine.JpegHost()
    arena = datapipe.CoefArena(None, False)
    state = {"handled": 0, "other": 0}

    def results():
        for r in datapipe._prefetch_map(lambda job: datapipe._native_decode(host, job),
                                        datapipe._native_jobs(host, arena, datapipe._examples(files, None, rng)), threads, window=4 * threads):
            if isinstance(r, datapipe.CoefSlot):
                state["handled"] += 1
                r.release()
            else:
                state["other"] += 1
                if r[1] is not None:
                    r[1].release()
            yield r
    it = results()
    for _ in range(2 * threads):
        next(it)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        next(it)
        n += 1
    dt = time.perf_counter() - t0
    it.close()
    return {"images_per_s": n / dt, "threads": threads, "handled": state["handled"], "fallback": state["other"],
            "note": "framing + Example lookup + fs_jpeg_parse + fs_jpeg_decode into arena chunks (pageable here) on the batcher's own thread pool, no GPU"}


def leg_kernels(reps=20):
    import torch
    from faststyle_amd import engine
    eng = engine.Engine()
    mem = eng.mem
    out = {}

    def per_launch(fn):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / reps            # us
    for B in (4, 32):
        rng = np.random.default_rng(B)
        store = mem.empty((3 * B, SIZE, SIZE, 3))
        store.normal_()
        batch = mem.empty((B, SIZE, SIZE, 3))
        imgs = [rng.integers(0, 256, (480, 640, 4), dtype=np.uint8) for _ in range(B)]
        items = np.zeros(B, dtype=eng.RESIZE_ITEM)
        for k, im in enumerate(imgs):
            items[k] = (k * im.nbytes, 480, 640, 4, k)
        staged = mem.upload_u8(np.concatenate([im.reshape(-1) for im in imgs]))
        tables = torch.from_numpy(np.concatenate([np.arange(B), np.arange(2 * B, 3 * B), np.arange(B)]).astype(np.int32).view(np.uint8).copy()).to(mem.device)
        idev = mem.upload_u8(items.view(np.uint8))
        row_bytes = SIZE * SIZE * 3 * 4
        us = per_launch(lambda: eng.queue_take(store, np.arange(B), np.arange(2 * B, 3 * B), np.arange(B), batch, tables_dev=(tables, 0)))
        out["batch%d" % B] = {
            "fs_queue_take_us": us, "fs_queue_take_GBps": 4 * B * row_bytes / us * 1e-3,       # B rows gathered + B rows moved, read + written
            "fs_resize_bicubic_u8x_many_us": per_launch(lambda: eng.resize_bicubic_u8_many(staged, items, store, items_dev=(idev, 0))),
            "fs_synth_uniform_us": per_launch(lambda: eng.synth_uniform(batch, 1234, 0, 5)),
            "note": "HIP events around %d back-to-back launches (host wrapper included); take: B rows gathered and B rows back-filled; "
                    "resize: B RGBX 640x480 sources" % reps}
    return out


def child(args):
    if args.leg == "pool":
        r = leg_pool(args.batch, args.steps, args.warmup)
    elif args.leg == "decode":
        r = leg_decode(args.shard_dir, args.threads)
    elif args.leg == "decode_native":
        r = leg_decode_native(args.shard_dir, args.threads)
    elif args.leg == "kernels":
        r = leg_kernels()
    else:
        r = leg_train(args.leg, args.batch, args.steps, args.warmup, args.shard_dir)
    print("TRAIN_E2E " + json.dumps(r), flush=True)


def verdict(doc):
    """The targets (each against the pool leg of the same run), met or missed, with what bounds a leg beside a miss."""
    out = {}
    decode = doc["legs"]["decode"]["images_per_s"]
    for batch, legs in ((4, doc["legs"].get("batch4", {})), (32, doc["legs"].get("batch32", {}))):
        for leg in ("synth_device", "shards", "shards_jpeg"):
            if leg not in legs:
                continue
            r = legs[leg]["ratio_to_pool"]
            row = {"ratio_to_pool": round(r, 4), "target": 0.97 if (leg, batch) != ("shards", 32) else None}
            if row["target"] is not None:
                row["met"] = bool(r >= row["target"])
            if leg == "shards_jpeg":
                native = doc["legs"].get("decode_native", {}).get("images_per_s")
                if native:
                    row["decode_native_images_per_s"] = round(native, 1)
            elif leg == "shards":
                row["decode_images_per_s"] = round(decode, 1)
                row["decode_over_pool_rate"] = round(decode / legs["pool"]["images_per_s"], 3)
                row["bound"] = ("inferred from the legs, not isolated further -- the host: the training thread shares the interpreter lock and the CPUs with the decode pool (its Python halves), and copies "
                                "each batch's decoded pixels into pinned memory itself; the device side (one copy, two launches, on the side stream) is "
                                "hidden -- compare shards_sync, where it is not")
            elif not row.get("met", True):
                row["bound"] = "inferred: the loop of train.py itself: the loss read-back every tenth step drains the device queue"
            out["%s_batch%d" % (leg, batch)] = row
    return out


def parent(args):
    from faststyle_amd import build as fsbuild
    shard_dir = tempfile.mkdtemp(prefix="train_e2e_shards_")
    t0 = time.perf_counter()
    mean_bytes = make_shards(shard_dir, args.images, 8)
    doc = {"csrc_sha16": fsbuild.source_digest(), "size": SIZE, "shards": {"images": args.images, "files": 8, "mean_jpeg_bytes": mean_bytes,
                                                                              "seconds_to_write": time.perf_counter() - t0}, "legs": {}}

    def run(leg, batch, steps, limit, env=None):
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--batch", str(batch), "--steps", str(steps),
               "--warmup", str(args.warmup), "--shard_dir", shard_dir, "--threads", str(args.threads)]
        e = dict(os.environ)
        e.pop("FS_FEED_DEPTH", None)
        e.pop("FS_FEED_JPEG", None)
        e.update(env or {})
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e)
        lines = [l for l in p.stdout.decode(errors="replace").splitlines() if l.startswith("TRAIN_E2E ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stderr.decode(errors="replace")[-4000:])
            raise SystemExit("leg %s batch %s ended with status %d: nothing more is started" % (leg, batch, p.returncode))
        return json.loads(lines[-1][len("TRAIN_E2E "):])

    def flush():
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1, sort_keys=True)
            f.write("\n")
    doc["legs"]["decode"] = run("decode", 0, 0, 120)
    flush()
    doc["legs"]["decode_native"] = run("decode_native", 0, 0, 120)
    flush()
    only = [l for l in (args.only or "").split(",") if l]
    if not only:
        doc["legs"]["kernels"] = run("kernels", 0, 0, 180)
        flush()
    for batch in (32, 4):
        legs = doc["legs"]["batch%d" % batch] = {}
        legs["pool"] = run("pool", batch, args.steps, 240)
        flush()
        for leg, steps, env in (("synth_device", args.steps, None), ("synth_host", max(20, args.steps // 5), None), ("shards", args.steps, None),
                                ("shards_sync", args.steps, {"FS_FEED_DEPTH": "0"}), ("shards_jpeg", args.steps, {"FS_FEED_JPEG": "1"})):
            if only and leg not in only:
                continue
            legs[leg] = run(leg, batch, steps, 420, env)
            legs[leg]["ratio_to_pool"] = legs[leg]["images_per_s"] / legs["pool"]["images_per_s"]
            flush()
    doc["targets"] = verdict(doc)
    flush()
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_e2e.json"))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--threads", type=int, default=16, help="decode threads of the two host-only legs (a fixed count, not the machine's CPU count)")
    ap.add_argument("--only", default=None, help="comma-separated train.main legs to run beside the pool leg (default: all)")
    ap.add_argument("--leg", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--shard_dir", default=None)
    a = ap.parse_args()
    child(a) if a.leg else parent(a)
