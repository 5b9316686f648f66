"""Input pipeline of train.py (drop-in for the reference's datapipe.py): TFRecord shards of
tf.train.Example protos -> JPEG decode -> TF1 bicubic resize -> shuffle queue -> batches.

Where each stage runs:
  * shard reading / record framing / Example lookup: native host code over an mmap (csrc/fs_io.hip);
  * JPEG decode: libjpeg via PIL on ``num_threads`` host threads (PIL drops the GIL), running
    ahead of the training loop through a bounded prefetch window; with ``batcher(..., jpeg="device")`` the
    library's own decoder instead (csrc/fs_jpeg.hip): the threads run only its Huffman pass, straight into
    pinned memory, and the GPU reconstructs the pixels (CoefArena, FedQueue._issue) -- the same pixels;
  * resize (tf.image.resize_images(method=2), datapipe.py:24): HIP kernel, fed with the u8 pixels
    (a quarter of the fp32 bytes over PCIe), writing straight into
  * the shuffle queue (tf.train.shuffle_batch, datapipe.py:74-77): ONE [capacity,H,W,3] fp32 tensor
    resident in HBM (4000 x 256x256 images = 3.1 GB of the 288 GB); a batch is a device-side gather.

Data-parallel: rank r reads shards ``files[r::world]`` (no exchange).

Two ways from the decoded pixels to a batch:
  * ``batcher(...)`` (``prefetch=0``): ShuffleQueue -- one upload and one resize launch per image, a gather and up to batch_size row copies
    per batch, all on the caller's stream;
  * ``batcher(..., prefetch=D)``: the device-fed path (DeviceRing + FedQueue, kernels in csrc/fs_feed.hip) -- the same batches, bit for bit
    and in the same order, but every image enqueued since the last take crosses in ONE pinned copy with ONE resize launch, the take is ONE
    launch, and all of it runs on a side stream into a ring of D batches, ahead of the step.
"""
import io
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib as L
from . import tfrecord

FEATURE_KEYS = ("image/encoded", "image/height", "image/channels", "image/width")     # datapipe.py:42-45


def decode_jpeg(data, packed=True):
    """tf.image.decode_jpeg(contents, channels=3) (datapipe.py:46): uint8 [H,W,3] RGB.
    packed=False (the batcher's decode threads): the decoder's own RGBX storage [H,W,4] as a zero-copy view (Arrow C data interface of
    Pillow >= 11.2 + pyarrow) when both are there -- np.asarray(im) repacks RGBX -> RGB through im.tobytes() under the interpreter lock, 0.3 ms
    per 640 x 480 image and the largest serialised piece of a decode thread's work; fs_resize_bicubic_u8x reads the RGBX pixels as they are."""
    from PIL import Image
    im = Image.open(io.BytesIO(bytes(data)))
    if im.mode != "RGB":
        im = im.convert("RGB")
    if not packed and _ARROW_OK:
        im.load()
        try:
            flat = _pa.array(im).flatten().to_numpy(zero_copy_only=True)     # (keeps the image's memory alive through the Arrow buffer)
            if flat.size == im.height * im.width * 4:
                return flat.reshape(im.height, im.width, 4)
        except Exception:
            pass
    return np.asarray(im, dtype=np.uint8)


try:
    import pyarrow as _pa
    from PIL import Image as _Image
    _ARROW_OK = hasattr(_Image.Image, "__arrow_c_array__") and os.environ.get("FS_DATAPIPE_RGBX", "1") != "0"
except Exception:      # (no pyarrow / an older Pillow: the packed path)
    _pa = None
    _ARROW_OK = False


def count_records(filenames):
    n = 0
    for f in filenames:
        rf = tfrecord.RecordFile(f, verify_crc=False)
        n += len(rf)
        rf.close()
    return n


def _examples(files, num_epochs, rng):
    """tf.train.string_input_producer(files, num_epochs, shuffle=True) + TFRecordReader +
    parse_single_example (datapipe.py:38-46): yields the 'image/encoded' bytes, shard order
    reshuffled every epoch."""
    epoch = 0
    while num_epochs is None or epoch < num_epochs:
        for fi in rng.permutation(len(files)):
            rf = tfrecord.RecordFile(files[fi])
            try:
                for i in range(len(rf)):
                    for key in FEATURE_KEYS[1:]:        # FixedLenFeature: a missing key is an error, as in TF
                        rf.feature_int64(i, key)
                    yield bytes(rf.feature_bytes(i, "image/encoded"))
            finally:
                rf.close()
        epoch += 1


def _prefetch_map(fn, it, num_threads, window):
    """Ordered map over ``it`` on a thread pool, at most ``window`` items in flight."""
    pool = ThreadPoolExecutor(max_workers=num_threads)
    pending = deque()
    try:
        for item in it:
            pending.append(pool.submit(fn, item))
            if len(pending) >= window:
                yield pending.popleft().result()
        while pending:
            yield pending.popleft().result()
    finally:
        pool.shutdown(wait=False, cancel_futures=True)


class ShuffleQueue(object):
    """tf.RandomShuffleQueue as used by tf.train.shuffle_batch: elements live in one HBM tensor;
    dequeue_many draws uniformly without replacement and back-fills the holes from the tail."""

    def __init__(self, engine, capacity, shape, rng):
        self.eng = engine
        self.capacity = int(capacity)
        self.shape = tuple(int(s) for s in shape)
        self.store = engine.mem.empty((self.capacity,) + self.shape)
        self.size = 0
        self.rng = rng

    def enqueue_resized(self, img_u8):
        assert self.size < self.capacity
        slot = self.eng.mem.view(self.store, self.size * int(np.prod(self.shape)), self.shape)
        self.eng.resize_bicubic_u8(img_u8, slot)
        self.size += 1

    def dequeue_many(self, n):
        idx = self.rng.choice(self.size, size=n, replace=False)
        batch = self.eng.mem.gather_rows(self.store, idx)
        # swap-remove, highest index first so the tail elements moved in are never ones being removed
        for i in sorted((int(v) for v in idx), reverse=True):
            last = self.size - 1
            if i != last:
                self.eng.mem.copy_row(self.store, last, i)
            self.size -= 1
        return batch


class DeviceRing(object):
    """``depth`` pre-allocated device batches that producers fill on a side stream while the consumer's stream works on earlier ones.

    Per slot two events: ``ready`` (recorded on the side stream behind the producer's last launch; the consumer's stream waits on it before
    it reads the batch) and ``free`` (recorded on the consumer's stream once the consumer has enqueued everything that reads the batch; the
    side stream waits on it before the slot is written again).  The host never waits for either.  ONE host thread issues everything -- the
    overlap is between streams on the device -- so nothing is launched concurrently with a hipGraph capture on the consumer's side and the
    (not thread-safe) engine context is only ever used from its own thread.

    A memory provider without streams (the emulator's host arrays) runs the same producers synchronously."""

    def __init__(self, engine, shape, depth):
        self.eng = engine
        mem = self.mem = engine.mem
        self.depth = max(1, int(depth))
        self.slots = [mem.empty(shape) for _ in range(self.depth)]
        self.side = None
        if all(getattr(mem, n, None) is not None for n in ("new_stream", "new_event", "on_stream", "current_stream")):
            self.side = mem.new_stream()
            self.side.wait_stream(mem.current_stream())        # (the slots, and whatever the caller allocated before, exist for the side stream)
            self.ready = [mem.new_event() for _ in range(self.depth)]
            self.free = [mem.new_event() for _ in range(self.depth)]
        self._free_recorded = [False] * self.depth
        self._next = 0

    def run(self, fn):
        """fn() with the side stream current (no slot involved: e.g. a resize launch between two takes)."""
        if self.side is None:
            return fn()
        with self.mem.on_stream(self.side):
            return fn()

    def produce(self, fn):
        """Enqueue fn(slot tensor) on the side stream for the next slot of the ring; returns the slot number."""
        s = self._next
        self._next = (s + 1) % self.depth
        if self.side is None:
            fn(self.slots[s])
            return s
        with self.mem.on_stream(self.side):
            if self._free_recorded[s]:
                self.side.wait_event(self.free[s])
            fn(self.slots[s])
            self.ready[s].record(self.side)
        return s

    def hand_over(self, s):
        if self.side is not None:
            self.mem.current_stream().wait_event(self.ready[s])
        return self.slots[s]

    def release(self, s):
        if self.side is not None:
            self.free[s].record(self.mem.current_stream())
            self._free_recorded[s] = True

    def close(self):
        """Drain: nothing of this ring is queued or running afterwards."""
        if self.side is not None:
            self.side.synchronize()

    def feed(self, producers):
        """Generator of device batches: producers yields callables fn(out) that fill ``out``.  Up to depth - 1 batches are produced ahead of
        the one the consumer holds; a batch is the consumer's until it asks for the next one."""
        pending = deque()
        try:
            for fn in producers:
                pending.append(self.produce(fn))
                if len(pending) == self.depth:
                    s = pending.popleft()
                    yield self.hand_over(s)
                    self.release(s)
            while pending:
                s = pending.popleft()
                yield self.hand_over(s)
                self.release(s)
        finally:
            try:
                close = getattr(producers, "close", None)
                if close is not None:
                    close()
            finally:
                self.close()


def _align16(n):
    return (n + 15) & ~15


class CoefSlot(object):
    """Where one handled JPEG's coefficients go: ``nbytes`` bytes at byte ``off`` of an arena chunk (host address ``addr``)."""
    __slots__ = ("arena", "chunk", "off", "nbytes", "addr", "info")

    def release(self):
        self.arena.done(self)


class _CoefChunk(object):
    __slots__ = ("host", "pinned", "dev", "size", "head", "live", "retired", "event")


class CoefArena(object):
    """Pinned host memory the decode threads write JPEG coefficients into (fs_jpeg_decode), in chunks that each have a device twin.

    Slots are handed out by ONE thread in the order the images will be enqueued, bump-allocated: the images one FedQueue._issue stages are
    neighbours in a chunk and cross in one copy (two when they straddle a chunk boundary).  A chunk is refilled only when every slot of it has
    been issued or dropped and the copy that last read it has completed (its event); the device twin needs no event of its own -- the copy
    that refills it is queued on the stream behind the kernels that read it.  Without pinned staging (the emulator's host arrays) a chunk is a
    plain array and the "copy" is upload_u8."""

    CHUNK_BYTES = 32 << 20

    def __init__(self, mem, pinned):
        self.mem = mem
        self.pinned = pinned
        self.cur = None
        self.free = []
        self.n_chunks = 0

    def _chunk(self, n):
        for i, c in enumerate(self.free):
            if c.size >= n:
                del self.free[i]
                if c.event is not None:
                    c.event.synchronize()
                c.head, c.retired = 0, False
                return c
        c = _CoefChunk()
        c.size = max(self.CHUNK_BYTES, n)
        if self.pinned:
            c.host, c.pinned, c.dev = self.mem.staging_u8(("jpeg_coef", self.n_chunks), c.size)
        else:
            c.host, c.pinned, c.dev = np.empty(c.size, dtype=np.uint8), None, None
        self.n_chunks += 1
        c.head, c.live, c.retired, c.event = 0, 0, False, None
        return c

    def reserve(self, info):
        n = _align16(int(info.coef_bytes))
        c = self.cur
        if c is None or c.head + n > c.size:
            if c is not None:
                c.retired = True
                if c.live == 0:
                    self.free.append(c)
            c = self.cur = self._chunk(n)
        slot = CoefSlot()
        slot.arena, slot.chunk, slot.off, slot.nbytes, slot.info = self, c, c.head, int(info.coef_bytes), info
        slot.addr = c.host.ctypes.data + c.head
        c.head += n
        c.live += 1
        return slot

    def done(self, slot):
        """The slot's content has been copied to the device, or is not wanted any more."""
        c = slot.chunk
        c.live -= 1
        if c.live == 0 and c.retired:
            self.free.append(c)

    def upload(self, chunk, a, b):
        """Bytes [a, b) of a chunk on the device (asynchronous on the current stream where the chunk is pinned)."""
        if chunk.pinned is None:
            return self.mem.upload_u8(chunk.host[a:b])
        dev = chunk.dev[a:b]
        self.mem.upload_u8_pinned(dev, chunk.pinned[a:b], b - a)
        if chunk.event is None:
            chunk.event = self.mem.new_event()
        chunk.event.record(self.mem.current_stream())
        return dev


class FedQueue(object):
    """ShuffleQueue's logic with the device work regrouped: the host keeps the very sequence of ShuffleQueue (slot = size, size += 1 per image;
    rng.choice + swap-remove, highest index first, per batch) on plain integers, and per batch issues one staging copy (descriptor table, index
    tables and the pixels of every image enqueued since the last take), one fs_resize_bicubic_u8x_many launch and one fs_queue_take launch
    through ``ring``.  The swap-remove is resolved on the host: each hole below the new size gets the ORIGINAL row that ends up in it (size 5,
    remove {2,3}: row 4 -> 3 -> 2 becomes the one move 4 -> 2).

    An enqueued image is either decoded pixels (a uint8 array, staged as above) or a CoefSlot: a JPEG whose coefficients a decode thread has
    written into the pinned CoefArena.  Those are not copied by the host at all: _issue sends the slots' stretch of the arena as it lies, one
    fs_jpeg_reconstruct_many turns it into RGBX pixels in a device buffer, and a second fs_resize_bicubic_u8x_many launch reads that."""

    STAGE_CAP_BYTES = 64 << 20      # images waiting for a take are flushed (copy + resize, no take) beyond this: the fill phase stages in pieces

    def __init__(self, engine, capacity, shape, rng, ring):
        self.eng = engine
        self.mem = engine.mem
        self.ring = ring
        self.capacity = int(capacity)
        self.shape = tuple(int(s) for s in shape)
        self.store = self.mem.empty((self.capacity,) + self.shape)
        if ring.side is not None:
            ring.side.wait_stream(self.mem.current_stream())
        self.size = 0
        self.rng = rng
        self._pending = []          # [(image, row)]
        self._pending_bytes = 0
        self._pinned = getattr(self.mem, "staging_u8", None) is not None and getattr(self.mem, "upload_u8_pinned", None) is not None and ring.side is not None
        self._n_stage = ring.depth + 1
        self._stage_next = 0
        self._stage_event = [None] * self._n_stage
        self.copies = 0             # staging copies issued (tests: O(1) per batch)
        self.coef_copies = 0        # ... and copies of arena stretches (the native JPEG path)
        self._rgb = None            # device u8 buffer the reconstructed pixels of one _issue live in

    def enqueue(self, img_u8):
        assert self.size < self.capacity
        if not isinstance(img_u8, CoefSlot):
            img_u8 = np.ascontiguousarray(img_u8, dtype=np.uint8)
        if self._pending and self._pending_bytes + img_u8.nbytes > self.STAGE_CAP_BYTES:
            self.ring.run(lambda: self._issue(None, None))
        self._pending.append((img_u8, self.size))
        self._pending_bytes += _align16(img_u8.nbytes)
        self.size += 1

    def take(self, n):
        """The host half of dequeue_many (rng draw, swap-remove on integers); returns fn(out) that issues the device half."""
        idx = self.rng.choice(self.size, size=n, replace=False)
        at = {}                      # position -> original row now standing there (positions that changed only)
        size = self.size
        for i in sorted((int(v) for v in idx), reverse=True):
            last = size - 1
            src = at.pop(last, last)
            if i != last:
                at[i] = src
            size -= 1
        self.size = size
        dst = sorted(at)
        tables = np.concatenate([np.asarray(idx, dtype=np.int32), np.asarray([at[d] for d in dst], dtype=np.int32),
                                 np.asarray(dst, dtype=np.int32)]).astype(np.int32)
        return lambda out: self._issue(tables, out)

    def _staging(self, nbytes):
        """(host array to fill, commit() -> device u8 buffer)."""
        if not self._pinned:
            host = np.empty(nbytes, dtype=np.uint8)
            return host, lambda: self.mem.upload_u8(host)
        k = self._stage_next
        self._stage_next = (k + 1) % self._n_stage
        if self._stage_event[k] is not None:
            self._stage_event[k].synchronize()         # the copy that last read this pinned buffer: depth + 1 batches back, long done
        host, pinned, dev = self.mem.staging_u8(k, nbytes)

        def commit():
            self.mem.upload_u8_pinned(dev, pinned, nbytes)
            if self._stage_event[k] is None:
                self._stage_event[k] = self.mem.new_event()
            self._stage_event[k].record(self.mem.current_stream())
            return dev
        return host, commit

    def _rgb_buffer(self, nbytes):
        if self._rgb is None or int(self._rgb.shape[0]) < nbytes:
            have = 0 if self._rgb is None else int(self._rgb.shape[0])
            self._rgb = self.mem.upload_u8(np.zeros(max(nbytes, (have * 3) // 2, 1 << 20), dtype=np.uint8))
        return self._rgb

    def _issue(self, tables, out):
        """One staging copy; the resize of the pending images; the take when ``tables`` is given.  Runs with the ring's side stream current.
        Staged: the resize descriptors (decoded images first, then the JPEG slots), the reconstruct descriptors, the take's tables, the decoded
        images' pixels.  The slots' coefficients go from the arena as they lie."""
        pending, self._pending, self._pending_bytes = self._pending, [], 0
        plain = [p for p in pending if not isinstance(p[0], CoefSlot)]
        slots = [p for p in pending if isinstance(p[0], CoefSlot)]
        K, Kp, Kj = len(pending), len(plain), len(slots)
        n_tab = 0 if tables is None else int(tables.size)
        jit_off = _align16(K * self.eng.RESIZE_ITEM.itemsize)
        tab_off = _align16(jit_off + Kj * self.eng.JPEG_ITEM.itemsize)
        off = _align16(tab_off + 4 * n_tab)
        items = np.zeros(K, dtype=self.eng.RESIZE_ITEM)
        for k, (img, row) in enumerate(plain):
            items[k] = (off, img.shape[0], img.shape[1], img.shape[2], row)
            off += _align16(img.nbytes)
        # the slots: consecutive ones of one chunk form a group = one copy + one reconstruct; all write RGBX into one device buffer
        jitems = np.zeros(Kj, dtype=self.eng.JPEG_ITEM)
        groups, rgb_bytes = [], 0
        for j, (slot, row) in enumerate(slots):
            if not groups or groups[-1][0] is not slot.chunk:
                groups.append([slot.chunk, slot.off, slot.off, j, j])
            g = groups[-1]
            g[1], g[2], g[4] = min(g[1], slot.off), max(g[2], slot.off + _align16(slot.nbytes)), j + 1
            items[Kp + j] = (rgb_bytes, slot.info.height, slot.info.width, 4, row)
            rgb_bytes += _align16(slot.info.height * slot.info.width * 4)
        for chunk, a, b, j0, j1 in groups:
            for j in range(j0, j1):
                slot = slots[j][0]
                jitems[j] = self.eng.jpeg_item(slot.info, slot.off - a, int(items[Kp + j]["src_offset"]), 4)
        host, commit = self._staging(off)
        host[:K * items.itemsize] = items.view(np.uint8)
        if Kj:
            host[jit_off:jit_off + Kj * jitems.itemsize] = jitems.view(np.uint8)
        if n_tab:
            host[tab_off:tab_off + 4 * n_tab] = tables.view(np.uint8)
        for it, (img, _) in zip(items, plain):
            o = int(it["src_offset"])
            host[o:o + img.nbytes] = img.reshape(-1)
        dev = commit()
        self.copies += 1
        if Kp:
            self.eng.resize_bicubic_u8_many(dev, items[:Kp], self.store, items_dev=(dev, 0))
        if Kj:
            rgb = self._rgb_buffer(rgb_bytes)
            for chunk, a, b, j0, j1 in groups:
                coef = slots[j0][0].arena.upload(chunk, a, b)
                self.coef_copies += 1
                self.eng.jpeg_reconstruct_many(coef, jitems[j0:j1], rgb, items_dev=(dev, jit_off + j0 * jitems.itemsize))
            for slot, _ in slots:
                slot.release()
            self.eng.resize_bicubic_u8_many(rgb, items[Kp:], self.store, items_dev=(dev, Kp * items.itemsize))
        if tables is not None:
            B = int(out.shape[0])
            M = (n_tab - B) // 2
            self.eng.queue_take(self.store, tables[:B], tables[B:B + M], tables[B + M:], out, tables_dev=(dev, tab_off))


def _fed_producers(queue, decoded, batch_size, min_after_dequeue, max_batches):
    """batcher's loop with the device work handed out as callables (DeviceRing.feed runs them, up to depth - 1 batches ahead)."""
    produced = 0
    try:
        for img in decoded:
            queue.enqueue(img)
            while queue.size - batch_size >= min_after_dequeue:
                yield queue.take(batch_size)
                produced += 1
                if max_batches is not None and produced >= max_batches:
                    return
        while queue.size >= batch_size:
            yield queue.take(batch_size)
            produced += 1
            if max_batches is not None and produced >= max_batches:
                return
    finally:
        decoded.close()


def synthetic_device_batches(engine, batch_size, resize_shape, seed, rank, first, count, depth):
    """``count`` batches [batch_size,H,W,3] of uniform [0,255) images generated on the device (fs_synth_uniform), batch indices first,
    first + 1, ...: batch k is a function of (seed, rank, k) alone, so a resumed run continues the stream at its step."""
    H, W = (int(v) for v in resize_shape)
    ring = DeviceRing(engine, (batch_size, H, W, 3), depth)
    return ring.feed((lambda out, k=k: engine.synth_uniform(out, seed, rank, k)) for k in range(first, first + count))


def host_batches(engine, arrays, depth):
    """Host float32 batches (all of one shape) -> device batches through pinned staging and the ring: the copy of batch k + 1 is asynchronous
    and runs on the side stream under step k.  The values are the host's, untouched."""
    arrays = iter(arrays)
    try:
        head = next(arrays)
    except StopIteration:
        return iter(())
    mem = engine.mem
    ring = DeviceRing(engine, head.shape, depth)
    pinned_ok = ring.side is not None and getattr(mem, "staging_u8", None) is not None
    events = [None] * (ring.depth + 1)
    state = {"k": 0}

    def producer(a):
        a = np.ascontiguousarray(a, dtype=np.float32)

        def fn(out):
            if not pinned_ok:
                out[...] = mem.from_numpy(a)
                return
            k = state["k"]
            state["k"] = (k + 1) % len(events)
            if events[k] is not None:
                events[k].synchronize()
            host, pinned, _ = mem.staging_u8(("host_batches", k), a.nbytes)
            host[:a.nbytes] = a.reshape(-1).view(np.uint8)
            mem.upload_u8_pinned(mem.as_u8(out), pinned, a.nbytes)
            if events[k] is None:
                events[k] = mem.new_event()
            events[k].record(mem.current_stream())
        return fn
    import itertools
    return ring.feed(producer(a) for a in itertools.chain([head], arrays))


class Batches(object):
    """What batcher returns: an iterator of device batches (next / for / close, as the generator it wraps) that also counts, on the native
    JPEG path, the images the library decoded (``jpeg_handled``) and those that went to PIL (``jpeg_fallback``)."""

    def __init__(self, *args, **kw):
        self.jpeg_handled = 0
        self.jpeg_fallback = 0
        self._gen = _batches(self, *args, **kw)

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._gen)

    def close(self):
        self._gen.close()


def batcher(filenames, batch_size, resize_shape=None, num_epochs=None, min_after_dequeue=4000, engine=None,
            seed=0, rank=0, world=1, num_threads=None, max_batches=None, prefetch=0, jpeg=None):
    """Iterator of device tensors [batch_size,H,W,3] float32 (RGB 0..255, TF1-bicubic resized).

    Same arguments as the reference's ``batcher`` (datapipe.py:55-78) plus the engine that owns the
    device, the shard partition and a seed.  Like tf.train.shuffle_batch it fills the queue to
    ``min_after_dequeue`` before the first batch (capacity = min_after_dequeue + 3*batch_size), and when the
    epochs are exhausted it drains the queue and drops the last partial batch.

    prefetch=D > 0: the device-fed path -- the same batches, produced on a side stream into a ring of D device batches (DeviceRing, FedQueue).
    A yielded batch is the caller's until it asks for the next one; closing the generator drains the side stream.

    jpeg="device" (needs prefetch > 0): baseline JPEGs are decoded by the library -- the decode threads run fs_jpeg_decode (the Huffman pass)
    into pinned memory, the GPU reconstructs the pixels (fs_jpeg_reconstruct_many), bit-identical to PIL's.  A JPEG the library does not take, or
    finds malformed, goes through PIL as before; the returned object counts both kinds (jpeg_handled, jpeg_fallback).  The batches are the same.
    """
    return Batches(filenames, batch_size, resize_shape, num_epochs, min_after_dequeue, engine, seed, rank, world, num_threads, max_batches,
                   prefetch, jpeg)


def _native_jobs(engine, arena, examples):
    """(file bytes, CoefSlot or None) in enqueue order: the slot is reserved here, by the one thread that also issues the copies, because its
    place in the arena is what makes an _issue's images neighbours (the parse is the file's header, microseconds)."""
    try:
        for data in examples:
            rc, info = engine.jpeg_parse(data)
            yield data, (arena.reserve(info) if rc == 0 else None)
    finally:
        examples.close()


def _native_decode(engine, job):
    """On a decode thread: the Huffman pass into the reserved slot (no interpreter lock held, no Python work on the pixels); PIL for what the
    library does not take -- a file it finds malformed included, so that such a file fares as it did before."""
    data, slot = job
    if slot is not None and engine.jpeg_decode(data, slot.info, slot.addr, slot.nbytes) == 0:
        return slot
    return decode_jpeg(data, packed=False), slot


def _native_results(stats, results):
    try:
        for r in results:
            if isinstance(r, CoefSlot):
                stats.jpeg_handled += 1
                yield r
            else:
                img, slot = r
                if slot is not None:
                    slot.release()
                stats.jpeg_fallback += 1
                yield img
    finally:
        results.close()


def _batches(stats, filenames, batch_size, resize_shape, num_epochs, min_after_dequeue, engine, seed, rank, world, num_threads, max_batches,
             prefetch, jpeg):
    if engine is None:
        raise L.FaststyleError("datapipe.batcher needs the Engine that owns the device (no CPU resize path)")
    if resize_shape is None:
        raise L.FaststyleError("batching needs a static image shape: pass resize_shape (train.py --preprocess_size)")
    if jpeg not in (None, "host", "device"):
        raise L.FaststyleError("batcher: jpeg must be None / 'host' (PIL) or 'device' (the library's decoder), got %r" % (jpeg,))
    native = jpeg == "device"
    if native and not (prefetch and prefetch > 0):
        raise L.FaststyleError("batcher(jpeg='device') runs on the device-fed path only: it needs prefetch > 0 (train.py: FS_FEED_JPEG=1 with "
                               "FS_FEED_DEPTH=0 is refused, not silently decoded by PIL)")
    if max_batches is not None and max_batches <= 0:       # (checked before anything is read: a zero cap yields nothing)
        return
    files = sorted(filenames)[rank::world]
    if not files:
        raise L.FaststyleError("rank %d of %d has no TFRecord shard (%d files)" % (rank, world, len(filenames)))
    H, W = (int(v) for v in resize_shape)
    rng = np.random.default_rng(seed + 7919 * rank)
    capacity = min_after_dequeue + 3 * batch_size                      # datapipe.py:73
    threads = num_threads or min(32, max(4, (os.cpu_count() or 8) // max(1, world)))
    if prefetch and prefetch > 0:
        ring = DeviceRing(engine, (batch_size, H, W, 3), prefetch)
        queue = FedQueue(engine, capacity, (H, W, 3), rng, ring)
        if native:
            arena = CoefArena(engine.mem, queue._pinned)
            decoded = _native_results(stats, _prefetch_map(lambda job: _native_decode(engine, job),
                                                           _native_jobs(engine, arena, _examples(files, num_epochs, rng)), threads, window=4 * threads))
        else:
            decoded = _prefetch_map(lambda d: decode_jpeg(d, packed=False), _examples(files, num_epochs, rng), threads, window=4 * threads)
        fed = ring.feed(_fed_producers(queue, decoded, batch_size, min_after_dequeue, max_batches))
        try:
            for batch in fed:
                yield batch
        finally:
            fed.close()          # (also when the caller stops early: drains the side stream)
        return
    decoded = _prefetch_map(lambda d: decode_jpeg(d, packed=False), _examples(files, num_epochs, rng), threads, window=4 * threads)
    queue = ShuffleQueue(engine, capacity, (H, W, 3), rng)
    produced = 0
    for img in decoded:
        queue.enqueue_resized(img)
        while queue.size - batch_size >= min_after_dequeue:            # RandomShuffleQueue.dequeue_many's condition
            yield queue.dequeue_many(batch_size)
            produced += 1
            if max_batches is not None and produced >= max_batches:
                decoded.close()
                return
    while queue.size >= batch_size:                                    # queue closed: drain, drop the remainder
        yield queue.dequeue_many(batch_size)
        produced += 1
        if max_batches is not None and produced >= max_batches:
            return
