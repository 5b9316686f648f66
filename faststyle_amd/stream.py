"""Frame-streaming stylizer: the loop body of the reference's stylize_webcam.py (:84-96) on the HIP
engine -- u8 frame in, u8 frame out, everything in between on the GPU.

Per frame: upload u8 (3 B/pixel over PCIe instead of 12) -> fs_u8_to_f32 -> fs_tnet_forward ->
fs_f32_to_u8 (``astype(np.uint8)`` truncation + the BGR<->RGB swap of cv2.cvtColor) -> download u8.
The device part is captured ONCE into a hipGraph (fixed frame size, fixed weights) and replayed per
frame: a batch-1 frame is ~45 short launches, so replay removes the per-launch host latency from
the frame time.  Reference quirk kept: the webcam frame is BGR but is fed to the RGB-trained net
as is, and the *output* channels are swapped before display (stylize_webcam.py:88-95).

With ``jpeg=dict(quality=95, subsampling=2)`` a stylizer returns the frame as the bytes of a baseline JPEG
file instead of the u8 array (the bytes PIL writes for that array, quality and subsampling): the device
pass ends with fs_jpeg_forward_many on the u8 frame, inside the graph, the int16 coefficients come down
instead of the pixels, and fs_jpeg_write entropy-codes them on host threads (csrc/fs_jpegenc.hip).
"""
import ctypes

import numpy as np

from . import _lib as L


class FrameStylizer(object):
    KEEP_GRAPH = False     # tests: keep the captured hipGraph_t so that its node types can be inspected

    def __init__(self, eng, variables, height, width, upsample_method="resize", batch=1, swap_rb=True, use_graph=True,
                 bf16=False, jpeg=None, jpeg_threads=4):
        self.eng = eng
        self.variables = variables
        self.method = upsample_method
        self.bf16 = bf16                 # FS_FLAG_BF16 mixed-precision path (~2x the frame rate, ~52 dB vs fp32)
        self.shape = (int(batch), int(height), int(width), 3)
        self.swap_rb = swap_rb
        mem = eng.mem
        Ho, Wo = eng.tnet_out_shape(height, width)
        self.out_shape = (int(batch), Ho, Wo, 3)
        self._in_u8 = mem.upload_u8(np.zeros(self.shape, np.uint8))
        self._in_f32 = mem.empty(self.shape)
        self._out_u8 = mem.upload_u8(np.zeros(self.out_shape, np.uint8))
        self._graph = None
        # A workspace of this stylizer's OWN: with frozen=True the re-laid-out filters of self.variables live inside it and the captured
        # graph no longer rebuilds them -- nobody else may write there (the engine's shared per-shape workspace would be rewritten by any
        # other same-shape forward, and every later replay would silently mix two models).
        self._ws = eng.new_tnet_workspace(self.shape[0], self.shape[1], self.shape[2], bf16)
        self._use_graph = use_graph and hasattr(mem, "torch")
        self._y = None
        self.jpeg = None
        self._pool = None
        if jpeg is not None:
            self._jpeg_setup(dict(jpeg), int(jpeg_threads))

    # luma sampling factors of PIL's ``subsampling`` values
    SUBSAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2), "4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}

    def _jpeg_setup(self, opt, threads):
        """The encoder's fixed parts: the plan of one output frame, the descriptor table (on the device once: the graph replays its address),
        the device coefficient buffer of the batch and one output buffer per image that surely holds its file."""
        quality, sub = int(opt.pop("quality", 95)), opt.pop("subsampling", 2)
        if opt or sub not in self.SUBSAMPLING or not 1 <= quality <= 100:
            raise L.FaststyleError("jpeg takes quality (1..100) and subsampling (0, 1, 2), got %r" % dict(opt, quality=quality, subsampling=sub))
        e, mem = self.eng, self.eng.mem
        B, Ho, Wo, _ = self.out_shape
        rc, info = e.jpeg_encode_plan(Wo, Ho, 3, *self.SUBSAMPLING[sub])
        L.check(e.lib, rc, "fs_jpeg_encode_plan")
        self.jpeg = dict(quality=quality, subsampling=sub)
        self._jinfo = info
        self._jstride = int(info.coef_bytes)                     # (a multiple of 16)
        self._jitems = np.zeros(B, dtype=e.JPEGENC_ITEM)
        for b in range(B):
            self._jitems[b] = e.jpegenc_item(info, b * Ho * Wo * 3, b * self._jstride, 3, quality)
        self._jitems_dev = mem.upload_u8(self._jitems.view(np.uint8).reshape(-1))
        self._coef = mem.upload_u8(np.zeros(B * self._jstride, np.uint8))
        self._jbound = e.jpeg_write_bound(info)
        self._jout = [ctypes.create_string_buffer(self._jbound) for _ in range(B)]
        self._jthreads = max(1, threads)

    def _write_one(self, coef_addr, b):
        """fs_jpeg_write of image b of a downloaded coefficient buffer (host address of the batch's first byte) -> bytes."""
        e = self.eng
        rc, n = e.jpeg_write(self._jinfo, coef_addr + b * self._jstride, self._jstride, ctypes.addressof(self._jout[b]), self._jbound)
        L.check(e.lib, rc, "fs_jpeg_write")
        return ctypes.string_at(self._jout[b], n)

    def _write_all(self, coef_addr, pool=None):
        """The files of the batch, in order; on ``pool`` (a ThreadPoolExecutor) when there is more than one."""
        B = self.out_shape[0]
        if B == 1 or pool is None:
            return [self._write_one(coef_addr, b) for b in range(B)]
        return list(pool.map(lambda b: self._write_one(coef_addr, b), range(B)))

    def _device_pass(self):
        e = self.eng
        e.u8_to_f32(self._in_u8, self._in_f32)
        self._y = e.tnet_forward(self.variables, self._in_f32, upsample_method=self.method, bf16=self.bf16, frozen=True,   # one checkpoint, many frames
                                 workspace=self._ws)
        e.f32_to_u8(self._y, self._out_u8, swap_rb=self.swap_rb)
        if self.jpeg is not None:
            e.jpeg_forward_many(self._out_u8, self._jitems, self._coef, items_dev=(self._jitems_dev, 0))

    def _capture(self):
        torch = self.eng.mem.torch
        self.eng.invalidate_frozen()                       # the warm-up below rebuilds the filters in self._ws whatever the library remembers
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # warm-up outside capture (one-time initialisation)
            self._device_pass()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph(keep_graph=True) if self.KEEP_GRAPH else torch.cuda.CUDAGraph()
        # thread_local: calls made by OTHER threads (e.g. the RCCL watchdog of a data-parallel run) must not
        # invalidate this thread's capture
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            self._device_pass()
        self._graph = g                                    # (replays raw pointers into self._ws, which lives as long as this object)

    def release(self):
        """Drop the captured graph (and the encode threads)."""
        self._graph = None
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def __call__(self, frames_u8):
        """frames_u8: host uint8 [H,W,3] (or [B,H,W,3]) -> host uint8 stylized frame(s) of the net's output size; with jpeg=: the bytes of
        its JPEG file (a list of them for a batch)."""
        a = np.asarray(frames_u8)
        single = a.ndim == 3
        if single:
            a = a[np.newaxis]
        if a.shape != self.shape or a.dtype != np.uint8:
            raise L.FaststyleError("frame shape %s dtype %s, stylizer was built for uint8 %s" % (a.shape, a.dtype, self.shape))
        mem = self.eng.mem
        if hasattr(mem, "torch"):
            self._in_u8.copy_(mem.torch.from_numpy(np.ascontiguousarray(a)), non_blocking=True)
        else:
            self._in_u8[...] = a
        if self._use_graph:
            if self._graph is None:
                self._capture()
            self._graph.replay()
        else:
            self._device_pass()
        if self.jpeg is not None:
            coef = np.ascontiguousarray(mem.to_numpy(self._coef))  # (synchronises)
            if self._pool is None and self.out_shape[0] > 1 and self._jthreads > 1:
                from concurrent.futures import ThreadPoolExecutor
                self._pool = ThreadPoolExecutor(self._jthreads)
            files = self._write_all(coef.ctypes.data, self._pool)
            return files[0] if single else files
        out = np.array(mem.to_numpy(self._out_u8), copy=True)     # (synchronises; the device buffer is reused next frame)
        return out[0] if single else out


class PipelinedStylizer(object):
    """`depth` FrameStylizer lanes on streams of their own (round 6): frame i + 1 is uploaded and stylized while frame i is still on the device.

    A batch-1 frame is ~45 DEPENDENT launches, 28 of them statistics / residual-add kernels of a few microseconds each: one frame at a time leaves the chip
    idle between them.  Independent frames need no collective and no shared state (BASELINE: "inference shards independent frames") -- two frame graphs on two
    streams fill each other's gaps: 720p 1277 -> 1890 frames/s on one MI355X (bench.py: stylize_720p.two_frames_in_flight), for one frame of latency.  Every
    lane owns its buffers, its workspace (the re-laid-out filters live inside it) and its captured graph; results are bit-identical to FrameStylizer's.

        ps = PipelinedStylizer(eng, variables, H, W)            # same arguments as FrameStylizer, + depth
        for out in ps.run(frames):                              # any iterable of uint8 [H,W,3] frames, results in order
            ...
    or submit(frame) / fetch() by hand (at most `depth` frames between them).

    With jpeg=dict(quality=, subsampling=) every lane ends in the encoder's device half and downloads coefficients into a pinned buffer of its
    own; a pool of `jpeg_threads` host threads (default 4) waits for a lane's event and entropy-codes its frame while the next frames are on the
    device (fs_jpeg_write holds no interpreter lock).  fetch() / run() then give bytes, in submission order."""

    def __init__(self, eng, variables, height, width, depth=2, jpeg_threads=4, **kw):
        if not hasattr(eng.mem, "torch"):
            raise L.FaststyleError("PipelinedStylizer needs the GPU engine (streams); use FrameStylizer on the emulator")
        import collections
        torch = eng.mem.torch
        self.torch = torch
        self.depth = int(depth)
        self.lanes = [FrameStylizer(eng, variables, height, width, **kw) for _ in range(self.depth)]
        self.streams = [torch.cuda.Stream() for _ in self.lanes]
        self.events = [torch.cuda.Event() for _ in self.lanes]
        self.host_in = [torch.empty(ln.shape, dtype=torch.uint8, pin_memory=True) for ln in self.lanes]
        self.host_out = [torch.empty(ln.out_shape, dtype=torch.uint8, pin_memory=True) for ln in self.lanes]
        self.jpeg = self.lanes[0].jpeg
        self._pool = None
        if self.jpeg is not None:
            from concurrent.futures import ThreadPoolExecutor
            self.host_coef = [torch.empty(ln._coef.shape, dtype=torch.uint8, pin_memory=True) for ln in self.lanes]
            self._pool = ThreadPoolExecutor(max(1, int(jpeg_threads)))
        self._pending = collections.deque()
        self._n = 0
        self._single = collections.deque()

    def submit(self, frames_u8):
        if len(self._pending) >= self.depth:
            raise L.FaststyleError("PipelinedStylizer: %d frames in flight already -- fetch() one first" % self.depth)
        a = np.asarray(frames_u8)
        single = a.ndim == 3
        if single:
            a = a[np.newaxis]
        k = self._n % self.depth
        ln, st, torch = self.lanes[k], self.streams[k], self.torch
        if a.shape != ln.shape or a.dtype != np.uint8:
            raise L.FaststyleError("frame shape %s dtype %s, stylizer was built for uint8 %s" % (a.shape, a.dtype, ln.shape))
        self.host_in[k].copy_(torch.from_numpy(np.ascontiguousarray(a)))       # (host -> pinned host; the lane's previous frame was fetched: its buffers are free)
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            ln._in_u8.copy_(self.host_in[k], non_blocking=True)
            if ln._use_graph:
                if ln._graph is None:
                    ln._capture()
                ln._graph.replay()
            else:
                ln._device_pass()
            if self.jpeg is not None:
                self.host_coef[k].copy_(ln._coef, non_blocking=True)
            else:
                self.host_out[k].copy_(ln._out_u8, non_blocking=True)
            self.events[k].record(st)
        if self.jpeg is not None:
            k = (k, self._pool.submit(self._encode, k))           # (the lane is reused only after fetch() has taken this result)
        self._pending.append(k)
        self._single.append(single)
        self._n += 1

    def _encode(self, k):
        """On an encode thread: wait for lane k's download, then Huffman-code its frame(s)."""
        self.events[k].synchronize()
        return self.lanes[k]._write_all(self.host_coef[k].data_ptr())

    def fetch(self):
        """The oldest submitted frame's result (host uint8; bytes with jpeg=), waiting for its lane only."""
        k = self._pending.popleft()
        single = self._single.popleft()
        if self.jpeg is not None:
            files = k[1].result()
            return files[0] if single else files
        self.events[k].synchronize()
        out = self.host_out[k].numpy().copy()
        return out[0] if single else out

    def run(self, frames):
        for f in frames:
            if len(self._pending) >= self.depth:
                yield self.fetch()
            self.submit(f)
        while self._pending:
            yield self.fetch()

    def release(self):
        for ln in self.lanes:
            ln.release()
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
