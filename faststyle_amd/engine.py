"""Thin Python driver over the C ABI: owns a context, workspaces and the pointer plumbing.

Device memory, streams and (in ``trainer.py``) ``torch.distributed`` come from PyTorch-ROCm --
plumbing only; every FLOP of the path runs in libfaststyle_hip.so.  The memory provider is
injectable (``mem``) so the parity tests can drive the very same code with host arrays against
the kernel emulator build; the product always uses ``TorchMem`` on a ROCm device.
"""
import ctypes
from collections import OrderedDict

import numpy as np

from . import _lib as L


class TorchMem(object):
    """Device tensors from PyTorch-ROCm on the current HIP stream."""

    supports_graphs = True     # hipGraph capture of a step (trainer.py); host-array providers of the tests have none

    def __init__(self, device="cuda:0"):
        import torch
        if not torch.cuda.is_available():
            raise L.FaststyleError("no ROCm/HIP device visible: the faststyle engine has no CPU path")
        self.torch = torch
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)

    def empty(self, shape):
        return self.torch.empty(tuple(int(s) for s in shape), dtype=self.torch.float32, device=self.device)

    def zeros(self, shape):
        return self.torch.zeros(tuple(int(s) for s in shape), dtype=self.torch.float32, device=self.device)

    def from_numpy(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(self.device)

    def to_numpy(self, t):
        return t.detach().cpu().numpy()

    def ptr(self, t):
        if t is None:
            return None
        assert t.is_contiguous() and t.dtype == self.torch.float32 and t.is_cuda
        return t.data_ptr()

    def stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def device_index(self):
        return self.device.index or 0

    def view(self, t, offset, shape):
        n = int(np.prod(shape))
        return t.view(-1)[offset:offset + n].view(*shape)

    # ---- input pipeline (datapipe.py): u8 uploads and the HBM-resident shuffle queue
    def upload_u8(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(self.device, non_blocking=True)

    def ptr_u8(self, t):
        assert t.is_contiguous() and t.dtype == self.torch.uint8 and t.is_cuda
        return t.data_ptr()

    def gather_rows(self, store, idx):
        return store.index_select(0, self.torch.as_tensor(np.asarray(idx, dtype=np.int64), device=self.device))

    def copy_row(self, store, src, dst):
        store[dst].copy_(store[src])

    # ---- device-fed input path (datapipe.DeviceRing): a side stream, events, pinned staging
    def new_stream(self):
        return self.torch.cuda.Stream(self.device)

    def new_event(self):
        return self.torch.cuda.Event()

    def current_stream(self):
        return self.torch.cuda.current_stream(self.device)

    def on_stream(self, stream):
        return self.torch.cuda.stream(stream)

    def staging_u8(self, slot, nbytes):
        """Staging pair number ``slot``: (numpy view of a pinned host buffer, that buffer, a device buffer), each of at least nbytes bytes.  The
        pair is kept and reused; it grows (by half again at least) when a request does not fit.  The caller owns the ordering: a pinned buffer
        is refilled only after the event behind its last copy has completed."""
        pool = self.__dict__.setdefault("_staging", {})
        have = pool.get(slot)
        if have is None or have[1].numel() < nbytes:
            n = max(int(nbytes), (have[1].numel() * 3) // 2 if have else 0, 1 << 20)
            pinned = self.torch.empty(n, dtype=self.torch.uint8, pin_memory=True)
            have = pool[slot] = (pinned.numpy(), pinned, self.torch.empty(n, dtype=self.torch.uint8, device=self.device))
        return have

    def upload_u8_pinned(self, dst_device, pinned, nbytes):
        """Asynchronous host-to-device copy on the current stream: pinned[:nbytes] -> dst_device[:nbytes] (both flat uint8).  The host does not
        wait for the stream, unlike upload_u8 from pageable memory."""
        dst_device[:nbytes].copy_(pinned[:nbytes], non_blocking=True)
        return dst_device

    def as_u8(self, t):
        """Flat uint8 view of a contiguous device tensor (the destination of upload_u8_pinned for float data)."""
        return t.view(-1).view(self.torch.uint8)


def default_loss_cfg():
    """train.py:52-70 defaults: content conv3_3 x1.0; style conv1_2/2_2/3_3/4_3 x5.0."""
    return dict(content_layers=["conv3_3"], content_weights=[1.0],
                style_layers=["conv1_2", "conv2_2", "conv3_3", "conv4_3"], style_weights=[5.0] * 4, beta=0.0)


class JpegHost(object):
    """The host calls of the JPEG decoder (csrc/fs_jpeg.hip) and encoder (csrc/fs_jpegenc.hip).  They need the library and no device: the engine
    has them through this class, and a tool that measures the host half alone makes a JpegHost of its own."""

    def __init__(self, lib=None):
        self.lib = lib if lib is not None else L.load()

    def jpeg_parse(self, data):
        """(answer, info) of fs_jpeg_parse for the bytes of a JPEG file: 0 handled (info: an fs_jpeg_info), 1 not taken by this decoder
        (PIL's), negative malformed; info is None unless handled.  Host code: needs no device, may be called from any thread."""
        info = L.fs_jpeg_info()
        rc = self.lib.fs_jpeg_parse(data, len(data), ctypes.byref(info))
        return rc, (info if rc == 0 else None)

    def jpeg_decode(self, data, info, out_addr, out_bytes):
        """fs_jpeg_decode: the Huffman pass of a handled JPEG into info.coef_bytes bytes at host address out_addr; returns its answer
        (0, or what makes the caller decode the file with PIL).  Releases the interpreter lock; any number of threads at once."""
        return self.lib.fs_jpeg_decode(data, len(data), ctypes.byref(info), ctypes.c_void_p(out_addr), out_bytes)

    # ---- the encoder's host half (csrc/fs_jpegenc.hip)
    def jpeg_encode_plan(self, width, height, ncomp=3, hs=2, vs=2):
        """(answer, info) of fs_jpeg_encode_plan: the fs_jpeg_info of the file jpeg_write writes for this geometry (hs x vs: the luma sampling,
        2x2 = 4:2:0, 2x1 = 4:2:2, 1x1 = 4:4:4); info is None unless the answer is 0."""
        info = L.fs_jpeg_info()
        rc = self.lib.fs_jpeg_encode_plan(int(width), int(height), int(ncomp), int(hs), int(vs), ctypes.byref(info))
        return rc, (info if rc == 0 else None)

    def jpeg_write_bound(self, info):
        """fs_jpeg_write_bound: a buffer size that surely holds the file of this info."""
        return int(self.lib.fs_jpeg_write_bound(ctypes.byref(info)))

    def jpeg_write(self, info, coef_addr, coef_bytes, out_addr, cap):
        """fs_jpeg_write: Huffman-codes the coefficient buffer at host address coef_addr (what jpeg_forward_many left, downloaded) into the cap
        bytes at host address out_addr; returns (answer, file length).  Releases the interpreter lock; any number of threads at once."""
        n = ctypes.c_size_t(0)
        rc = self.lib.fs_jpeg_write(ctypes.byref(info), ctypes.c_void_p(coef_addr), int(coef_bytes), ctypes.c_void_p(out_addr), int(cap), ctypes.byref(n))
        return rc, int(n.value)

    def jpeg_write_bytes(self, info, coef):
        """The file of one image as bytes; coef: host uint8 array holding its coefficient buffer."""
        coef = np.ascontiguousarray(coef, dtype=np.uint8)
        out = np.empty(self.jpeg_write_bound(info), dtype=np.uint8)
        rc, n = self.jpeg_write(info, coef.ctypes.data, coef.nbytes, out.ctypes.data, out.nbytes)
        L.check(self.lib, rc, "fs_jpeg_write")
        return out[:n].tobytes()


class CvResizePlan(object):
    """One planned cv2.resize (fs_cvresize_plan): ``info`` the library's fs_cvresize_info, ``tables`` its per-axis tables on the host (uint8),
    and -- once an engine has run it -- the device copy of the tables, uploaded once per plan."""

    def __init__(self, info, tables):
        self.info = info
        self.tables = tables
        self.tables_dev = None
        self.src_shape = (int(info.src_h), int(info.src_w))
        self.dst_shape = (int(info.dst_h), int(info.dst_w))
        self.path = int(info.path)

    def axis_table(self, axis):
        """The entries of one axis table ('x' or 'y') as cvresize.py states them: cubic -> (idx [n_dst,4], w [n_dst,4]); area -> the list of
        (dst index, src index, float32 weight) of _area_tab; the area fast path has none (None)."""
        i = self.info
        n_dst, off, taps = (i.dst_w, i.x_offset, i.x_taps) if axis == "x" else (i.dst_h, i.y_offset, i.y_taps)
        if self.path == L.FS_CVRESIZE_PATH_AREA_FAST:
            return None
        if self.path == L.FS_CVRESIZE_PATH_CUBIC:
            t = self.tables[off:off + n_dst * 32].view("<i4").reshape(n_dst, 8)
            return t[:, :4].astype(np.int64), t[:, 4:].astype(np.int64)
        ofs = self.tables[off:off + (n_dst + 1) * 4].view("<i4")
        start = off + ((n_dst + 1) * 4 + 7) // 8 * 8
        rows = self.tables[start:start + taps * 8].view(np.dtype([("si", "<i4"), ("alpha", "<f4")]))
        return [(d, int(rows["si"][k]), rows["alpha"][k]) for d in range(n_dst) for k in range(int(ofs[d]), int(ofs[d + 1]))]


class CvResizeHost(object):
    """The host calls of the cv2.resize kernels (csrc/fs_cvresize.hip): plan and tables.  They need the library and no device."""

    def __init__(self, lib=None):
        self.lib = lib if lib is not None else L.load()

    def cvresize_plan(self, H, W, fx, fy, interpolation=None):
        """fs_cvresize_plan + fs_cvresize_tables of cv2.resize(img [H,W,3] u8, None, fx=fx, fy=fy, interpolation): a CvResizePlan.
        interpolation: L.FS_CV_INTER_CUBIC / L.FS_CV_INTER_AREA; None: the dispatch of the reference's utils.imresize on two axes -- area when
        both axes shrink or stay and at least one shrinks, otherwise cubic.  A refused request raises FaststyleError."""
        fx, fy = float(fx), float(fy)
        if interpolation is None:
            interpolation = L.FS_CV_INTER_AREA if (fx <= 1.0 and fy <= 1.0 and (fx < 1.0 or fy < 1.0)) else L.FS_CV_INTER_CUBIC
        info = L.fs_cvresize_info()
        L.check(self.lib, self.lib.fs_cvresize_plan(int(H), int(W), fx, fy, int(interpolation), ctypes.byref(info)), "fs_cvresize_plan")
        tables = np.zeros(int(info.table_bytes), np.uint8)
        L.check(self.lib, self.lib.fs_cvresize_tables(ctypes.byref(info), ctypes.c_void_p(tables.ctypes.data) if tables.size else None,
                                                      tables.nbytes), "fs_cvresize_tables")
        return CvResizePlan(info, tables)


class ResamplePlan(object):
    """One planned fp32 resampling (fs_resample_plan): ``info`` the library's fs_resample_info, ``tables`` its per-axis tables on the host
    (uint8), and -- once an engine has run it -- the device copy of the tables, uploaded once per plan."""

    def __init__(self, info, tables, filter):
        self.info = info
        self.tables = tables
        self.tables_dev = None
        self.filter = filter
        self.src_shape = (int(info.src_h), int(info.src_w))
        self.dst_shape = (int(info.dst_h), int(info.dst_w))
        self.tile_h = int(info.tile_h)

    def axis_table(self, axis):
        """One axis table ('x' or 'y') as (xmin [n_dst] int32, cnt [n_dst] int32, w [n_dst, ksize] float64); None for an axis that keeps
        its length."""
        i = self.info
        n_dst, off, ksize = (i.dst_w, i.x_offset, i.x_ksize) if axis == "x" else (i.dst_h, i.y_offset, i.y_ksize)
        if ksize == 0:
            return None
        rows = self.tables[off:off + n_dst * (8 + 8 * ksize)].view(np.dtype([("xmin", "<i4"), ("cnt", "<i4"), ("w", "<f8", (ksize,))]))
        return rows["xmin"].copy(), rows["cnt"].copy(), rows["w"].copy()


class ResampleHost(object):
    """The host calls of the fp32 resampler (csrc/fs_resample.hip): plan and tables.  They need the library and no device."""

    def __init__(self, lib=None):
        self.lib = lib if lib is not None else L.load()

    def resample_plan(self, Hs, Ws, Hd, Wd, filter="bicubic"):
        """fs_resample_plan + fs_resample_tables of Pillow's Image.resize((Wd, Hd), filter) on mode-F images of Hs x Ws: a ResamplePlan.
        filter: 'box', 'bilinear', 'bicubic' or 'lanczos'.  A refused request raises FaststyleError."""
        code = L.FS_RESAMPLE_FILTERS.get(filter)
        if code is None:
            raise L.FaststyleError("resample filter is one of %s, got %r" % (", ".join(sorted(L.FS_RESAMPLE_FILTERS)), filter))
        try:
            sizes = [int(v) for v in (Hs, Ws, Hd, Wd)]
            if any(a != b for a, b in zip(sizes, (Hs, Ws, Hd, Wd))):
                raise ValueError
        except (TypeError, ValueError):
            raise L.FaststyleError("resample sizes must be whole numbers, got %r" % ((Hs, Ws, Hd, Wd),))
        info = L.fs_resample_info()
        L.check(self.lib, self.lib.fs_resample_plan(sizes[0], sizes[1], sizes[2], sizes[3], code, ctypes.byref(info)), "fs_resample_plan")
        tables = np.zeros(int(info.table_bytes) // 8, np.float64).view(np.uint8)          # (8-byte aligned)
        L.check(self.lib, self.lib.fs_resample_tables(ctypes.byref(info), ctypes.c_void_p(tables.ctypes.data) if tables.size else None,
                                                      tables.nbytes), "fs_resample_tables")
        return ResamplePlan(info, tables, filter)


class YuvHost(object):
    """The host call of the planar YCbCr kernels (csrc/fs_yuv.hip): the frame geometry.  It needs the library and no device."""

    def __init__(self, lib=None):
        self.lib = lib if lib is not None else L.load()

    def yuv_plan(self, width, height, sampling=(2, 2), siting=0, matrix=0, full_range=False, components=3, bits=8):
        """fs_yuv_plan: the fs_yuv_desc of width x height frames -- sampling (hs, vs) of luma against chroma, siting 0 centre / 1 co-sited,
        matrix 0 BT.601 / 1 BT.709 (or 'bt601' / 'bt709'), components 3 or 1 (mono).  bits other than 8: fs_yuv_plan_deep, the frames of 9 to
        16 bits per sample in 16-bit words (desc.reserved[0] = bits).  A refused geometry raises FaststyleError."""
        hs, vs = (int(v) for v in sampling)
        matrix = {"bt601": 0, "bt709": 1}.get(matrix, matrix)
        desc = L.fs_yuv_desc()
        if int(bits) != 8:
            L.check(self.lib, self.lib.fs_yuv_plan_deep(int(width), int(height), hs, vs, int(components), int(siting), int(matrix), int(full_range),
                                                        int(bits), ctypes.byref(desc)), "fs_yuv_plan_deep")
            return desc
        L.check(self.lib, self.lib.fs_yuv_plan(int(width), int(height), hs, vs, int(components), int(siting), int(matrix), int(full_range),
                                               ctypes.byref(desc)), "fs_yuv_plan")
        return desc


class Engine(JpegHost, CvResizeHost, ResampleHost, YuvHost):
    # Workspaces are cached per shape (a backward must find the workspace its forward filled; a captured hipGraph replays raw
    # pointers into its own).  The cache is bounded by BYTES, least recently used first: stylizing a directory of mixed
    # resolutions must not pile up one multi-GB workspace per size.  Entries a live hipGraph replays into are pinned by
    # their trainer (pin_workspaces) and are never evicted while pinned.
    MAX_CACHED_BYTES = 24 << 30    # of 288 GB; the largest single shape of the BASELINE configs (1080p batch 8 fp32) needs 17 GB
    MAX_CACHED_SHAPES = 8

    def __init__(self, mem=None, lib=None):
        self.mem = mem if mem is not None else TorchMem()      # initialises the HIP runtime PyTorch ships
        self.lib = lib if lib is not None else L.load()
        ctx = ctypes.c_void_p()
        L.check(self.lib, self.lib.fs_ctx_create(self.mem.device_index(), ctypes.c_void_p(self.mem.stream()),
                                                 ctypes.byref(ctx)), "fs_ctx_create")
        self.ctx = ctx
        self._tnet_ws = {}
        self._perc_ws = {}
        self._pinned = {}          # id(workspace tensor) -> pin count
        self._tnet_nbytes = {}     # (N, H, W, bf16) -> fs_tnet_workspace_bytes, see _tnet_key
        self._perc_io = {}         # perceptual workspace key -> (y offset, content offset), see perceptual_inputs
        self._private = []         # [(weakref to a new_tnet_workspace() tensor, nbytes)]: counted in the byte budget while alive
        self._keep = []

    def close(self):
        if self.ctx:
            self.lib.fs_ctx_destroy(self.ctx)
            self.ctx = None

    def _sync_stream(self):
        self.lib.fs_ctx_set_stream(self.ctx, ctypes.c_void_p(self.mem.stream()))

    # ------------------------------------------------------------------ parameters
    def param_table(self):
        """[(name, offset, shape)] of the 48 tensors in the flat parameter buffer (ckpt order)."""
        out = []
        for i in range(L.FS_TNET_NTENSORS):
            name = ctypes.c_char_p()
            off = ctypes.c_int()
            nd = ctypes.c_int()
            dims = (ctypes.c_int * 4)()
            L.check(self.lib, self.lib.fs_tnet_param_info(i, ctypes.byref(name), ctypes.byref(off), ctypes.byref(nd),
                                                          ctypes.byref(dims)), "fs_tnet_param_info")
            out.append((name.value.decode(), off.value, tuple(dims[k] for k in range(nd.value))))
        return out

    def param_table_for(self, upsample_method="resize"):
        """param_table() with the conv2d_transpose filter shapes [K,K,Cout,Cin] of --upsample_method
        deconv (im_transf_net.py:174) -- same element counts, so the flat offsets are identical."""
        tab = self.param_table()
        if upsample_method == "deconv":
            tab = [(n, o, (s[0], s[1], s[3], s[2]) if n.startswith("upsample_") and len(s) == 4 else s) for n, o, s in tab]
        return tab

    def flatten_params(self, tensors, scope="img_t_net/", upsample_method="resize"):
        """dict name->ndarray (checkpoint names) -> flat float32 vector in table order."""
        flat = np.empty(L.FS_TNET_NPARAMS, dtype=np.float32)
        for name, off, shape in self.param_table_for(upsample_method):
            a = tensors.get(scope + name, tensors.get(name))
            if a is None:
                raise L.FaststyleError("checkpoint lacks tensor %s%s" % (scope, name))
            if tuple(a.shape) != shape:
                raise L.FaststyleError("tensor %s has shape %s, expected %s (wrong --upsample_method?)"
                                       % (name, a.shape, shape))
            flat[off:off + a.size] = np.asarray(a, dtype=np.float32).ravel()
        return flat

    def unflatten_params(self, flat, scope="img_t_net/", upsample_method="resize"):
        flat = np.asarray(flat)
        return OrderedDict((scope + name, flat[off:off + int(np.prod(shape))].reshape(shape).copy())
                           for name, off, shape in self.param_table_for(upsample_method))

    # ------------------------------------------------------------------ transform net
    def tnet_out_shape(self, H, W):
        ho, wo = ctypes.c_int(), ctypes.c_int()
        L.check(self.lib, self.lib.fs_tnet_out_shape(H, W, ctypes.byref(ho), ctypes.byref(wo)), "fs_tnet_out_shape")
        return ho.value, wo.value

    def _evict(self, cache, incoming_bytes):
        """Drop least-recently-used, unpinned entries of `cache` until `incoming_bytes` more fit the budget."""
        def total():
            self._private = [(r, nb) for r, nb in self._private if r() is not None]
            return sum(nb for _, nb in self._tnet_ws.values()) + sum(nb for _, nb in self._perc_ws.values()) + sum(nb for _, nb in self._private)
        dropped = False
        for key in list(cache):
            if len(cache) < self.MAX_CACHED_SHAPES and total() + incoming_bytes <= self.MAX_CACHED_BYTES:
                break
            if self._pinned.get(id(cache[key][0]), 0) == 0:
                cache.pop(key)
                dropped = True
        if dropped:
            self.invalidate_frozen()

    def invalidate_frozen(self):
        """A workspace (or a parameter buffer) the library may remember by ADDRESS went away: the caching allocator can hand the same address
        out again, so FS_FLAG_PARAMS_FROZEN must not trust pointer identity across this point (fs_tnet_invalidate)."""
        if self.ctx:
            self.lib.fs_tnet_invalidate(self.ctx)

    def pin_workspaces(self, entries, on=True):
        """entries: workspace tensors a captured hipGraph replays into; pinned entries survive cache eviction."""
        for t in entries:
            n = self._pinned.get(id(t), 0) + (1 if on else -1)
            if n > 0:
                self._pinned[id(t)] = n
            else:
                self._pinned.pop(id(t), None)

    def pin_last_used(self, tnet=True, perceptual=False):
        """The capture contract: whoever captures engine calls into a hipGraph calls this right after the capture and keeps the
        returned list (the workspace tensors the captured calls used = the most recently used entry of each cache, now
        pinned against eviction AND kept alive by the list) for as long as the graph lives; release_pins() afterwards."""
        held = []
        if tnet and self._tnet_ws:
            held.append(next(reversed(self._tnet_ws.values()))[0])
        if perceptual and self._perc_ws:
            held.append(next(reversed(self._perc_ws.values()))[0])
        self.pin_workspaces(held, True)
        return held

    def release_pins(self, held):
        if held:
            self.pin_workspaces(held, False)
            del held[:]

    def _tnet_key(self, N, H, W, bf16=False):
        # the layout (and with it the size) depends on the library's FS_TNET_WINO knob as the LIBRARY sees it (read once and
        # cached there): ask the library, not os.environ
        # (memoised: the C entry point rebuilds the whole layout, 40-65 us of host time -- per frame in an eager loop;
        # reset_workspaces(), which every knob flip is followed by, drops the memo)
        nbytes = self._tnet_nbytes.get((N, H, W, bf16))
        if nbytes is None:
            nbytes = self.lib.fs_tnet_workspace_bytes(N, H, W, L.FS_FLAG_BF16 if bf16 else L.FS_FLAG_SAVE_FOR_BWD)
            if nbytes == 0:
                raise L.FaststyleError("bad transform-net shape %s" % ((N, H, W, bf16),))
            self._tnet_nbytes[(N, H, W, bf16)] = nbytes
        return (N, H, W, bf16, nbytes)

    def _tnet_workspace(self, N, H, W, bf16=False):
        key = self._tnet_key(N, H, W, bf16)
        if key not in self._tnet_ws:
            self._evict(self._tnet_ws, key[4])
            self._tnet_ws[key] = (self.mem.empty((key[4] // 4,)), key[4])
        else:
            self._tnet_ws[key] = self._tnet_ws.pop(key)                      # mark as most recently used
        return self._tnet_ws[key]

    def reset_workspaces(self):
        """Drop every cached workspace (their sizes were planned under the tuning knobs of the time; tests that flip FS_*
        knobs with fs_debug_reload_env call this, production code never needs to)."""
        self._sync_stream()
        self._tnet_ws.clear()
        self._perc_ws.clear()
        self._pinned.clear()
        self._tnet_nbytes.clear()
        self._perc_io.clear()
        self.invalidate_frozen()

    def new_tnet_workspace(self, N, H, W, bf16=False):
        """A transform-net workspace of the caller's own (not in the shape cache): what a hipGraph capturer with frozen=True replays into --
        the re-laid-out filters inside it belong to ONE parameter set, and no other call of this engine may rewrite them (a shared, per-shape
        workspace would be rewritten by any other same-shape forward: another FrameStylizer with another checkpoint, a Trainer, an eval)."""
        import weakref
        nbytes = self._tnet_key(N, H, W, bf16)[4]
        # a private workspace counts in MAX_CACHED_BYTES for as long as its owner keeps it: make room among the cached (unpinned) entries first,
        # largest cache first -- several stylizers plus a Trainer otherwise add up outside every budget (the caller's workspace itself is never refused)
        for cache in sorted((self._tnet_ws, self._perc_ws), key=lambda c: -sum(nb for _, nb in c.values())):
            self._evict(cache, nbytes)
        self.invalidate_frozen()          # (a fresh allocation may re-use an address the library remembers)
        t = self.mem.empty((nbytes // 4,))
        try:
            self._private.append((weakref.ref(t), nbytes))
        except TypeError:                 # (a memory backend whose buffers take no weak references: not counted)
            pass
        return (t, nbytes)

    @staticmethod
    def _method_flag(upsample_method):
        assert upsample_method in ("resize", "deconv")
        return L.FS_FLAG_UPSAMPLE_DECONV if upsample_method == "deconv" else 0

    def tnet_forward(self, params, x, save_for_bwd=False, upsample_method="resize", bf16=False, frozen=False, workspace=None, out=None):
        """create_net(x, upsample_method): x [N,H,W,3] float32 RGB 0..255 -> y [N,Ho,Wo,3].
        bf16=True: the mixed-precision inference path (FS_FLAG_BF16; ~1e-2 of the pixel range off the fp32 path).
        frozen=True: `params` is not modified between calls (FS_FLAG_PARAMS_FROZEN: the filter re-layouts run once per sequence).
        workspace: a (tensor, nbytes) pair from new_tnet_workspace() instead of the engine's shared per-shape one.
        out: write y into this [N,Ho,Wo,3] tensor (e.g. perceptual_inputs()[0]) instead of a fresh one."""
        self._sync_stream()
        N, H, W, C = (int(s) for s in x.shape)
        assert C == 3
        Ho, Wo = self.tnet_out_shape(H, W)
        ws, nbytes = workspace if workspace is not None else self._tnet_workspace(N, H, W, bf16)
        y = out if out is not None else self.mem.empty((N, Ho, Wo, 3))
        assert tuple(int(v) for v in y.shape) == (N, Ho, Wo, 3)
        p = self.mem.ptr
        L.check(self.lib, self.lib.fs_tnet_forward(self.ctx, p(params), p(x), N, H, W, p(y), p(ws), nbytes,
                                                   (L.FS_FLAG_SAVE_FOR_BWD if save_for_bwd else 0) |
                                                   (L.FS_FLAG_BF16 if bf16 else 0) | (L.FS_FLAG_PARAMS_FROZEN if frozen and not bf16 else 0) |
                                                   self._method_flag(upsample_method)), "fs_tnet_forward")
        return y

    def tnet_backward(self, params, x, dy, grads=None, upsample_method="resize"):
        """Gradient of the 48 tensors given dL/dy; must follow tnet_forward(save_for_bwd=True)."""
        self._sync_stream()
        N, H, W, _ = (int(s) for s in x.shape)
        if self._tnet_key(N, H, W) not in self._tnet_ws:
            raise L.FaststyleError("tnet_backward(%dx%dx%d) without a tnet_forward(save_for_bwd=True) of that shape" % (N, H, W))
        ws, nbytes = self._tnet_workspace(N, H, W)
        if grads is None:
            grads = self.mem.empty((L.FS_TNET_NPARAMS,))
        p = self.mem.ptr
        L.check(self.lib, self.lib.fs_tnet_backward(self.ctx, p(params), p(x), p(dy), N, H, W, p(grads), p(ws), nbytes,
                                                    self._method_flag(upsample_method)), "fs_tnet_backward")
        return grads

    # ------------------------------------------------------------------ VGG / losses
    def vgg_load(self, weights):
        """weights: mapping in the npz convention of vgg16.load_weights (vgg16.py:257-266):
        'conv1_1_W' [3,3,3,64], 'conv1_1_b' [64], ...  Keeps device copies + dgrad re-layout."""
        self._sync_stream()
        self.vgg_w, self.vgg_b = [], []
        for i, n in enumerate(L.VGG_LAYER_NAMES):
            w = np.asarray(weights[n + "_W"], dtype=np.float32)
            b = np.asarray(weights[n + "_b"], dtype=np.float32)
            if w.shape != (3, 3, L.VGG_CIN[i], L.VGG_COUT[i]) or b.shape != (L.VGG_COUT[i],):
                raise L.FaststyleError("VGG weight %s has shape %s" % (n, w.shape))
            self.vgg_w.append(self.mem.from_numpy(w))
            self.vgg_b.append(self.mem.from_numpy(b))
        self._wp = (ctypes.c_void_p * L.FS_VGG_NLAYERS)(*[self.mem.ptr(t) for t in self.vgg_w])
        self._bp = (ctypes.c_void_p * L.FS_VGG_NLAYERS)(*[self.mem.ptr(t) for t in self.vgg_b])
        self.vgg_prepared = self.mem.empty((self.lib.fs_vgg_prepared_floats(),))
        L.check(self.lib, self.lib.fs_vgg_prepare(self.ctx, ctypes.byref(self._wp), self.mem.ptr(self.vgg_prepared)),
                "fs_vgg_prepare")

    def _cfg(self, cfg, target_grams=None):
        c = L.fs_loss_cfg()
        # the reference asserts equal lengths (losses.py:28, :58 iterate by index over both lists)
        if len(cfg["content_layers"]) != len(cfg["content_weights"]) or len(cfg["style_layers"]) != len(cfg["style_weights"]):
            raise L.FaststyleError("loss layers and weights differ in length: %s / %s, %s / %s" % (
                cfg["content_layers"], cfg["content_weights"], cfg["style_layers"], cfg["style_weights"]))
        c.n_content = len(cfg["content_layers"])
        for i, (n, w) in enumerate(zip(cfg["content_layers"], cfg["content_weights"])):
            c.content_layer[i] = L.VGG_LAYER_NAMES.index(n)
            c.content_weight[i] = w
        c.n_style = len(cfg["style_layers"])
        for i, (n, w) in enumerate(zip(cfg["style_layers"], cfg["style_weights"])):
            c.style_layer[i] = L.VGG_LAYER_NAMES.index(n)
            c.style_weight[i] = w
            if target_grams is not None:
                c.target_gram[i] = self.mem.ptr(target_grams[i])
        c.beta = cfg.get("beta", 0.0)
        return c

    def style_targets(self, style_img, cfg):
        """utils.get_grams on the style image (train.py:144-151): list of [1,C,C] device tensors."""
        self._sync_stream()
        _, H, W, _ = (int(s) for s in style_img.shape)
        c = self._cfg(cfg)
        grams = [self.mem.empty((1, L.VGG_COUT[c.style_layer[i]], L.VGG_COUT[c.style_layer[i]]))
                 for i in range(c.n_style)]
        gp = (ctypes.c_void_p * 4)(*([self.mem.ptr(g) for g in grams] + [None] * (4 - len(grams))))
        nbytes = self.lib.fs_style_targets_workspace_bytes(H, W)
        ws = self.mem.empty((nbytes // 4,))
        L.check(self.lib, self.lib.fs_style_targets(self.ctx, ctypes.byref(self._wp), ctypes.byref(self._bp), ctypes.byref(c),
                                                    self.mem.ptr(style_img), H, W, ctypes.byref(gp), self.mem.ptr(ws), nbytes),
                "fs_style_targets")
        return grams

    def _perceptual_workspace(self, N, H, W, cfg, c):
        key = (N, H, W, tuple(cfg["content_layers"]), tuple(cfg["style_layers"]))
        nbytes = self.lib.fs_perceptual_workspace_bytes(N, H, W, ctypes.byref(c))
        if key not in self._perc_ws or self._perc_ws[key][1] != nbytes:
            self._perc_ws.pop(key, None)
            self._evict(self._perc_ws, nbytes)
            self._perc_ws[key] = (self.mem.empty((nbytes // 4,)), nbytes)
        else:
            self._perc_ws[key] = self._perc_ws.pop(key)
        return self._perc_ws[key]

    def perceptual_inputs(self, N, H, W, cfg, with_ws=False):
        """(y, content) views INSIDE the (cached) perceptual workspace of this shape, where fs_perceptual_loss stages its two inputs
        (fs_perceptual_ws_input): a caller that lets tnet_forward(out=y) write there and keeps its batch in `content` saves both
        staging copies of a step.  content is None when cfg has no content layer.  The views die with the workspace: a caller that keeps
        one across calls (a hipGraph capturer) asks for the workspace tensor too (with_ws=True -> (y, content, ws)) and pins exactly that
        tensor (pin_workspaces([ws]))."""
        c = self._cfg(cfg)
        ws, _ = self._perceptual_workspace(N, H, W, cfg, c)
        key = (N, H, W, tuple(cfg["content_layers"]), tuple(cfg["style_layers"]))
        if key not in self._perc_io:      # (the offsets are a pure function of the key; an eager loop asks every step)
            yo, co = ctypes.c_size_t(), ctypes.c_size_t()
            L.check(self.lib, self.lib.fs_perceptual_ws_input(N, H, W, ctypes.byref(c), ctypes.byref(yo), ctypes.byref(co)), "fs_perceptual_ws_input")
            self._perc_io[key] = (yo.value, None if co.value == ctypes.c_size_t(-1).value else co.value)
        yo, co = self._perc_io[key]
        out = (self.mem.view(ws, yo, (N, H, W, 3)), (None if co is None else self.mem.view(ws, co, (N, H, W, 3))))
        return out + (ws,) if with_ws else out

    def perceptual_loss(self, y, content, target_grams, cfg):
        """loss = content + style + beta*tv (train.py:164-184) and dL/dy.
        Returns (losses[4] device tensor {loss, content, style, beta*tv}, dy)."""
        self._sync_stream()
        N, H, W, _ = (int(s) for s in y.shape)
        if tuple(content.shape) != tuple(y.shape):
            # the reference feeds VGG(batch) into placeholders shaped like VGG(Y) (train.py:171-176, 250-254)
            raise L.FaststyleError("content batch %s and net output %s differ: training sizes must be multiples "
                                   "of 4 (create_net maps H -> 4*ceil(ceil((H+80)/2)/2)-80)" % (tuple(content.shape), tuple(y.shape)))
        c = self._cfg(cfg, target_grams)
        ws, nbytes = self._perceptual_workspace(N, H, W, cfg, c)
        losses = self.mem.empty((4,))
        dy = self.mem.empty((N, H, W, 3))
        p = self.mem.ptr
        L.check(self.lib, self.lib.fs_perceptual_loss(self.ctx, ctypes.byref(self._wp), ctypes.byref(self._bp),
                                                      p(self.vgg_prepared), ctypes.byref(c), p(y), p(content), N, H, W,
                                                      p(losses), p(dy), p(ws), nbytes), "fs_perceptual_loss")
        return losses, dy

    # ------------------------------------------------------------------ builder-level pieces (vgg16 / utils / losses)
    def vgg_features(self, x, layer_names):
        """libs/vgg16.py:36-220: post-ReLU activations `convX_Y` of x [N,H,W,3] (RGB 0..255); needs vgg_load()."""
        self._sync_stream()
        N, H, W, _ = (int(s) for s in x.shape)
        ids = [L.VGG_LAYER_NAMES.index(n) for n in layer_names]
        outs, h, w, shapes = [], H, W, {}
        for l in range(max(ids) + 1):
            shapes[l] = (N, h, w, L.VGG_COUT[l])
            if l in (1, 3, 6, 9):                        # max_pool 2x2 s2 SAME after conv1_2 / 2_2 / 3_3 / 4_3
                h, w = (h + 1) // 2, (w + 1) // 2
        outs = [self.mem.empty(shapes[l]) for l in ids]
        nbytes = self.lib.fs_vgg_features_workspace_bytes(N, H, W, max(ids))
        ws = self.mem.empty((nbytes // 4,))
        lay = (ctypes.c_int * len(ids))(*ids)
        op = (ctypes.c_void_p * len(ids))(*[self.mem.ptr(t) for t in outs])
        L.check(self.lib, self.lib.fs_vgg_features(self.ctx, ctypes.byref(self._wp), ctypes.byref(self._bp), self.mem.ptr(x), N, H, W,
                                                   len(ids), lay, op, self.mem.ptr(ws), nbytes), "fs_vgg_features")
        return outs

    def gram(self, feat):
        """utils.get_grams for one layer (utils.py:76-82): feat [N,h,w,c] -> [N,c,c] = F^T F / (h*w*c)  (fs_gram_fwd)."""
        self._sync_stream()
        N, h, w, c = (int(s) for s in feat.shape)
        G = self.mem.empty((N, c, c))
        nbytes = self.lib.fs_gram_workspace_bytes(N, h * w, c)
        ws = self.mem.empty((max(nbytes // 4, 1),))
        p = self.mem.ptr
        L.check(self.lib, self.lib.fs_gram_fwd(self.ctx, p(feat), N, h * w, c, p(G), p(ws), nbytes), "fs_gram_fwd")
        return G

    def gram_bwd(self, feat, dG):
        """Gradient through utils.get_grams: dF = F (dG + dG^T) / (h*w*c), feat [N,h,w,c], dG [N,c,c]  (fs_gram_bwd)."""
        self._sync_stream()
        N, h, w, c = (int(s) for s in feat.shape)
        dF = self.mem.empty((N, h, w, c))
        nbytes = self.lib.fs_gram_workspace_bytes(N, h * w, c)
        ws = self.mem.empty((max(nbytes // 4, 1),))
        p = self.mem.ptr
        L.check(self.lib, self.lib.fs_gram_bwd(self.ctx, p(feat), p(dG), N, h * w, c, p(dF), p(ws), nbytes), "fs_gram_bwd")
        return dF

    # ------------------------------------------------------------------ inspection of the saved tensors (parity tests)
    def tnet_saved(self, N, H, W, unit, what, upsample_method="resize"):
        """View of a tensor fs_tnet_forward(save_for_bwd=True) left in the (cached) workspace of this shape."""
        off, dims = ctypes.c_size_t(), (ctypes.c_int * 4)()
        L.check(self.lib, self.lib.fs_tnet_ws_tensor(N, H, W, L.FS_FLAG_SAVE_FOR_BWD | self._method_flag(upsample_method), unit, what,
                                                     ctypes.byref(off), ctypes.byref(dims)), "fs_tnet_ws_tensor")
        key = self._tnet_key(N, H, W)
        if key not in self._tnet_ws:
            raise L.FaststyleError("no transform-net workspace of shape %s" % ((N, H, W),))
        shape = tuple(dims) if what in (L.FS_TNET_WS_Z, L.FS_TNET_WS_H) else (dims[0], dims[1])
        return self.mem.view(self._tnet_ws[key][0], off.value, shape)

    def tnet_bf16_plan(self, N, H, W, unit):
        """How unit 0..15 of the bf16 inference path is planned under the library's tuning knobs of the moment (FS_TNET_BWS_PLAN)."""
        dims = (ctypes.c_int * 8)()
        L.check(self.lib, self.lib.fs_tnet_bf16_ws_tensor(N, H, W, unit, L.FS_TNET_BWS_PLAN, None, ctypes.byref(dims), None), "fs_tnet_bf16_ws_tensor")
        return dict(zip(("bs", "BN", "WM", "CC", "cout_pad", "tiles_y", "tiles_x", "c4"), (int(v) for v in dims)))

    def tnet_bf16_saved(self, workspace, N, H, W, unit, what):
        """Host copy of a tensor tnet_forward(bf16=True, workspace=workspace) left in `workspace`, a new_tnet_workspace(N, H, W, bf16=True) pair:
        numpy uint16 (bfloat16 bit patterns) or float32, whichever the path stores (fs_tnet_bf16_ws_tensor)."""
        off, dims, esz = ctypes.c_size_t(), (ctypes.c_int * 8)(), ctypes.c_int()
        L.check(self.lib, self.lib.fs_tnet_bf16_ws_tensor(N, H, W, unit, what, ctypes.byref(off), ctypes.byref(dims), ctypes.byref(esz)),
                "fs_tnet_bf16_ws_tensor")
        ws, nbytes = workspace
        if nbytes != self._tnet_key(N, H, W, True)[4]:
            raise L.FaststyleError("not a bf16 transform-net workspace of shape %s" % ((N, H, W),))
        shape = tuple(int(d) for d in dims[:4])
        if what in (L.FS_TNET_BWS_A, L.FS_TNET_BWS_B, L.FS_TNET_BWS_MEAN, L.FS_TNET_BWS_RSTD):
            shape = shape[:2]
        elif what == L.FS_TNET_BWS_WPK:
            shape = shape[:3]
        n = int(np.prod(shape))
        assert off.value % 4 == 0 and off.value + n * esz.value <= nbytes
        raw = np.ascontiguousarray(self.mem.to_numpy(self.mem.view(ws, off.value // 4, ((n * esz.value + 3) // 4,))))
        return raw.view(np.uint16 if esz.value == 2 else np.float32)[:n].reshape(shape).copy()

    def vgg_saved(self, N, H, W, cfg, layer_name):
        """View of the post-ReLU activations fs_perceptual_loss left in its (cached) workspace: [NB,h,w,c], the first N
        samples are the net outputs, the next N (up to the last content layer) the content batch."""
        c = self._cfg(cfg)
        off, dims = ctypes.c_size_t(), (ctypes.c_int * 4)()
        L.check(self.lib, self.lib.fs_perceptual_ws_tensor(N, H, W, ctypes.byref(c), L.VGG_LAYER_NAMES.index(layer_name),
                                                           ctypes.byref(off), ctypes.byref(dims)), "fs_perceptual_ws_tensor")
        key = (N, H, W, tuple(cfg["content_layers"]), tuple(cfg["style_layers"]))
        if key not in self._perc_ws:
            raise L.FaststyleError("no perceptual workspace of shape %s" % ((N, H, W),))
        return self.mem.view(self._perc_ws[key][0], off.value, tuple(dims))

    def loss_sqdiff(self, x, t, scale):
        """scale * sum((x - t)^2) with t broadcast over the leading (batch) axis when smaller; device scalar [1]."""
        self._sync_stream()
        n, period = int(np.prod(x.shape)), int(np.prod(t.shape))
        assert n % period == 0
        out, scratch = self.mem.empty((1,)), self.mem.empty((1024,))
        p = self.mem.ptr
        L.check(self.lib, self.lib.fs_loss_sqdiff(self.ctx, p(x), p(t), period, n, float(scale), p(out), p(scratch)), "fs_loss_sqdiff")
        return out

    def loss_tv(self, x):
        self._sync_stream()
        N, H, W, C = (int(s) for s in x.shape)
        out, scratch = self.mem.empty((1,)), self.mem.empty((1024,))
        p = self.mem.ptr
        L.check(self.lib, self.lib.fs_loss_tv(self.ctx, p(x), N, H, W, C, p(out), p(scratch)), "fs_loss_tv")
        return out

    # ------------------------------------------------------------------ value + gradient forms (round 6; faststyle_amd/autograd.py builds on these)
    def loss_sqdiff_grad(self, x, t, scale):
        """(scale * sum((x - t)^2) as a device scalar [1], d/dx = 2 * scale * (x - t)) -- losses.py:32-37 / :61-64 with their derivative."""
        self._sync_stream()
        n, period = int(np.prod(x.shape)), int(np.prod(t.shape))
        assert n % period == 0
        out, scratch, grad = self.mem.empty((1,)), self.mem.empty((1024,)), self.mem.empty(tuple(x.shape))
        p = self.mem.ptr
        L.check(self.lib, self.lib.fs_loss_sqdiff_grad(self.ctx, p(x), p(t), period, n, float(scale), p(out), p(grad), p(scratch)), "fs_loss_sqdiff_grad")
        return out, grad

    def loss_tv_grad(self, x, scale=1.0, grad=None):
        """(scale * TV(x) [1], scale * dTV/dx); grad given: the gradient is ADDED to it (train.py:184's beta * tv on top of the perceptual gradient)."""
        self._sync_stream()
        N, H, W, C = (int(s) for s in x.shape)
        out, scratch = self.mem.empty((1,)), self.mem.empty((1024,))
        acc = grad is not None
        if grad is None:
            grad = self.mem.empty((N, H, W, C))
        p = self.mem.ptr
        L.check(self.lib, self.lib.fs_loss_tv_grad(self.ctx, p(x), N, H, W, C, float(scale), p(out), p(grad), int(acc), p(scratch)), "fs_loss_tv_grad")
        return out, grad

    def vgg_dgrad(self, x, layer_names, dfeats, use_prepared=True):
        """Adjoint of vgg_features: dfeats[i] = dL/d(activation layer_names[i]) -> dL/dx [N,H,W,3] (fs_vgg_dgrad; the forward is recomputed)."""
        self._sync_stream()
        N, H, W, _ = (int(s) for s in x.shape)
        ids = [L.VGG_LAYER_NAMES.index(n) for n in layer_names]
        dx = self.mem.empty((N, H, W, 3))
        nbytes = self.lib.fs_vgg_dgrad_workspace_bytes(N, H, W, max(ids))
        ws = self.mem.empty((nbytes // 4,))
        lay = (ctypes.c_int * len(ids))(*ids)
        gp = (ctypes.c_void_p * len(ids))(*[self.mem.ptr(t) for t in dfeats])
        L.check(self.lib, self.lib.fs_vgg_dgrad(self.ctx, ctypes.byref(self._wp), ctypes.byref(self._bp),
                                                self.mem.ptr(self.vgg_prepared) if use_prepared else None, self.mem.ptr(x), N, H, W,
                                                len(ids), lay, gp, self.mem.ptr(dx), self.mem.ptr(ws), nbytes), "fs_vgg_dgrad")
        return dx

    def conv2d_dgrad(self, dy, w, in_hw, stride=1, padding="SAME"):
        """tf.nn.conv2d_backprop_input: dy [N,Ho,Wo,Cout], w HWIO [K,K,Cin,Cout] -> dx [N,H,W,Cin] (fs_conv2d_dgrad)."""
        self._sync_stream()
        N = int(dy.shape[0])
        K, _, Cin, Cout = (int(s) for s in w.shape)
        H, W = in_hw
        d = L.fs_conv_desc()
        d.N, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride = N, H, W, Cin, Cout, K, K, stride
        if isinstance(padding, str):
            d.pad_mode = L.FS_PAD_SAME if padding == "SAME" else L.FS_PAD_VALID
        else:
            d.pad_mode = L.FS_PAD_EXPLICIT
            d.pad_t, d.pad_l, d.Ho, d.Wo = padding
        d.w = self.mem.ptr(w)
        nbytes = self.lib.fs_conv2d_dgrad_workspace_bytes(ctypes.byref(d))
        ws, dx = self.mem.empty((nbytes // 4,)), self.mem.empty((N, H, W, Cin))
        L.check(self.lib, self.lib.fs_conv2d_dgrad(self.ctx, ctypes.byref(d), self.mem.ptr(dy), self.mem.ptr(dx), self.mem.ptr(ws), nbytes), "fs_conv2d_dgrad")
        return dx

    def _resizeconv(self, fn, name, a, b, N, H, W, Cin, Cout, out_shape):
        self._sync_stream()
        nbytes = self.lib.fs_resizeconv_workspace_bytes(N, H, W, Cin, Cout)
        if not nbytes:
            raise L.FaststyleError("%s: Cin and Cout must be multiples of 4 (got %d -> %d)" % (name, Cin, Cout))
        ws, out = self.mem.empty((nbytes // 4,)), self.mem.empty(out_shape)
        p = self.mem.ptr
        L.check(self.lib, fn(self.ctx, p(a), p(b), N, H, W, Cin, Cout, p(out), p(ws), nbytes), name)
        return out

    def resizeconv_fwd(self, x, w):
        """upconv2d's conv (im_transf_net.py:122-155: NEAREST x4 + 3x3 stride-2 SAME), phase-collapsed: x [N,H,W,Cin] -> [N,2H,2W,Cout]."""
        N, H, W, Cin = (int(s) for s in x.shape)
        Cout = int(w.shape[3])
        return self._resizeconv(self.lib.fs_resizeconv_fwd, "fs_resizeconv_fwd", x, w, N, H, W, Cin, Cout, (N, 2 * H, 2 * W, Cout))

    def resizeconv_dgrad(self, dy, w):
        N, H2, W2, Cout = (int(s) for s in dy.shape)
        Cin = int(w.shape[2])
        return self._resizeconv(self.lib.fs_resizeconv_dgrad, "fs_resizeconv_dgrad", dy, w, N, H2 // 2, W2 // 2, Cin, Cout, (N, H2 // 2, W2 // 2, Cin))

    def resizeconv_wgrad(self, x, dy):
        N, H, W, Cin = (int(s) for s in x.shape)
        Cout = int(dy.shape[3])
        return self._resizeconv(self.lib.fs_resizeconv_wgrad, "fs_resizeconv_wgrad", x, dy, N, H, W, Cin, Cout, (3, 3, Cin, Cout))

    def instnorm_apply(self, z, a, b, mode=0, skip=None, skip_a=None, skip_b=None):
        """act(a z + b) materialised (mode 0 none / 1 ReLU / 2 scaled tanh), or the residual block's sum with `skip` [N,H+4,W+4,C] (fs_instnorm_apply)."""
        self._sync_stream()
        N, H, W, C = (int(s) for s in z.shape)
        out = self.mem.empty((N, H, W, C))
        p = self.mem.ptr
        L.check(self.lib, self.lib.fs_instnorm_apply(self.ctx, p(z), p(a), p(b), N, H, W, C, int(mode), p(skip), p(skip_a), p(skip_b), p(out)), "fs_instnorm_apply")
        return out

    def resize_bicubic_u8(self, img_u8, out):
        """tf.image.resize_images(img, out.shape[:2], method=2) of TF 1.0 (datapipe.py:24) on the device:
        img_u8 host uint8 [H,W,3] (packed RGB) or [H,W,4] (RGBX as a decoder stores it: datapipe.decode_jpeg; the fourth byte is ignored)
        -> ``out`` (device float32 [Ho,Wo,3], written in place)."""
        self._sync_stream()
        H, W, C = (int(s) for s in img_u8.shape)
        Ho, Wo, Co = (int(s) for s in out.shape)
        assert C in (3, 4) and Co == 3
        src = self.mem.upload_u8(img_u8)
        if C == 3:
            L.check(self.lib, self.lib.fs_resize_bicubic_u8(self.ctx, self.mem.ptr_u8(src), H, W, self.mem.ptr(out), Ho, Wo),
                    "fs_resize_bicubic_u8")
        else:
            L.check(self.lib, self.lib.fs_resize_bicubic_u8x(self.ctx, self.mem.ptr_u8(src), H, W, 4, self.mem.ptr(out), Ho, Wo),
                    "fs_resize_bicubic_u8x")
        return out

    # ------------------------------------------------------------------ device-fed input path (csrc/fs_feed.hip)
    RESIZE_ITEM = np.dtype([("src_offset", "<u8"), ("H", "<i4"), ("W", "<i4"), ("pixel_bytes", "<i4"), ("dst_row", "<i4")])   # fs_resize_item

    def _table_ptr(self, table, dev):
        """Device address of an integer table: ``dev`` = (device u8 buffer, byte offset) where the caller has staged it already, else it is
        uploaded here.  Returns (address, keep-alive)."""
        if dev is not None:
            return self.mem.ptr_u8(dev[0]) + int(dev[1]), dev[0]
        up = self.mem.upload_u8(np.ascontiguousarray(table).view(np.uint8).reshape(-1))
        return self.mem.ptr_u8(up), up

    def resize_bicubic_u8_many(self, staged, items, store, items_dev=None):
        """K resize_bicubic_u8 calls in one launch (fs_resize_bicubic_u8x_many).  staged: device uint8 buffer holding the decoded images;
        items: host array of RESIZE_ITEM rows (where each image lies, its shape, its row of ``store``); store: device float32
        [capacity,Ho,Wo,3].  items_dev: (device u8 buffer, byte offset) of a copy of ``items`` already on the device."""
        self._sync_stream()
        items = np.ascontiguousarray(items, dtype=self.RESIZE_ITEM)
        capacity, Ho, Wo, C = (int(s) for s in store.shape)
        assert C == 3
        ptr, keep = self._table_ptr(items, items_dev)
        L.check(self.lib, self.lib.fs_resize_bicubic_u8x_many(self.ctx, self.mem.ptr_u8(staged), int(np.prod(staged.shape)), items.ctypes.data, ptr,
                                                              int(items.shape[0]), self.mem.ptr(store), capacity, Ho, Wo),
                "fs_resize_bicubic_u8x_many")
        self._keep = [keep, items]
        return store

    def queue_take(self, store, take_idx, move_src, move_dst, out, tables_dev=None):
        """tf.RandomShuffleQueue.dequeue_many in one launch (fs_queue_take): out[i] = store[take_idx[i]], then store[move_dst[j]] =
        store[move_src[j]].  tables_dev: (device u8 buffer, byte offset) of the three int32 tables back to back, staged by the caller."""
        self._sync_stream()
        take_idx, move_src, move_dst = (np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (take_idx, move_src, move_dst))
        B, M = int(take_idx.size), int(move_src.size)
        assert int(move_dst.size) == M
        capacity = int(store.shape[0])
        row = int(np.prod(store.shape[1:]))
        assert int(np.prod(out.shape)) == B * row
        ptr, keep = self._table_ptr(np.concatenate([take_idx, move_src, move_dst]), tables_dev)
        L.check(self.lib, self.lib.fs_queue_take(self.ctx, self.mem.ptr(store), capacity, row, ptr, B, ptr + 4 * B if M else None,
                                                 ptr + 4 * (B + M) if M else None, M, self.mem.ptr(out)), "fs_queue_take")
        self._keep = [keep]
        return out

    # ------------------------------------------------------------------ baseline JPEG decoding (csrc/fs_jpeg.hip)
    JPEG_ITEM = np.dtype([("coef_offset", "<u8"), ("qt_offset", "<u8"), ("dst_offset", "<u8"), ("width", "<i4"), ("height", "<i4"),
                          ("ncomp", "<i4"), ("hs", "<i4"), ("vs", "<i4"), ("pixel_bytes", "<i4")])      # fs_jpeg_item

    @classmethod
    def jpeg_item(cls, info, coef_offset, dst_offset, pixel_bytes):
        """The JPEG_ITEM row of an image that fs_jpeg_decode wrote at byte coef_offset of the coefficient buffer."""
        return (coef_offset, coef_offset + info.qt_offset, dst_offset, info.width, info.height, info.ncomp, info.hs[0], info.vs[0], pixel_bytes)

    def jpeg_reconstruct_many(self, coef, items, rgb, items_dev=None):
        """fs_jpeg_reconstruct_many: coef, rgb device uint8 buffers; items host JPEG_ITEM rows; the u8 pixels of every image are written into
        ``rgb`` where its row says.  ``coef`` is working memory (its coefficients are consumed).  items_dev as for resize_bicubic_u8_many."""
        self._sync_stream()
        items = np.ascontiguousarray(items, dtype=self.JPEG_ITEM)
        ptr, keep = self._table_ptr(items, items_dev)
        L.check(self.lib, self.lib.fs_jpeg_reconstruct_many(self.ctx, self.mem.ptr_u8(coef), int(np.prod(coef.shape)), items.ctypes.data, ptr,
                                                            int(items.shape[0]), self.mem.ptr_u8(rgb), int(np.prod(rgb.shape))),
                "fs_jpeg_reconstruct_many")
        self._keep = [keep, items]
        return rgb

    # ------------------------------------------------------------------ baseline JPEG encoding (csrc/fs_jpegenc.hip)
    JPEGENC_ITEM = np.dtype([("src_offset", "<u8"), ("coef_offset", "<u8"), ("qt_offset", "<u8"), ("width", "<i4"), ("height", "<i4"),
                             ("ncomp", "<i4"), ("hs", "<i4"), ("vs", "<i4"), ("pixel_bytes", "<i4"), ("quality", "<i4"),
                             ("reserved", "<i4")])      # fs_jpegenc_item

    @classmethod
    def jpegenc_item(cls, info, src_offset, coef_offset, pixel_bytes, quality):
        """The JPEGENC_ITEM row of an image (info: jpeg_encode_plan's) whose pixels lie at byte src_offset of the source buffer and whose
        coefficient buffer, the one jpeg_write reads, goes to byte coef_offset."""
        return (src_offset, coef_offset, coef_offset + info.qt_offset, info.width, info.height, info.ncomp, info.hs[0], info.vs[0], pixel_bytes,
                quality, 0)

    def jpeg_forward_many(self, src, items, coef, items_dev=None):
        """fs_jpeg_forward_many: src, coef device uint8 buffers; items host JPEGENC_ITEM rows; the coefficient buffer of every image is written
        into ``coef`` where its row says.  ``src`` is only read.  items_dev as for resize_bicubic_u8_many."""
        self._sync_stream()
        items = np.ascontiguousarray(items, dtype=self.JPEGENC_ITEM)
        ptr, keep = self._table_ptr(items, items_dev)
        L.check(self.lib, self.lib.fs_jpeg_forward_many(self.ctx, self.mem.ptr_u8(src), int(np.prod(src.shape)), items.ctypes.data, ptr,
                                                        int(items.shape[0]), self.mem.ptr_u8(coef), int(np.prod(coef.shape))),
                "fs_jpeg_forward_many")
        self._keep = [keep, items]
        return coef

    # ------------------------------------------------------------------ cv2.resize on u8 images (csrc/fs_cvresize.hip)
    def cvresize_u8(self, src_dev, plan, out_dev, swap_rb=False):
        """fs_cvresize_u8: src_dev device uint8 [H,W,3|4] or [N,H,W,3|4] (4: RGBX, the fourth byte never read) -> out_dev device uint8
        [Hd,Wd,3] / [N,Hd,Wd,3], the result of cvresize.resize_cubic_u8 / resize_area_u8 for the plan's (fx, fy); swap_rb: R and B exchanged.
        The plan's tables go to the device on its first use."""
        self._sync_stream()
        shape = tuple(int(d) for d in src_dev.shape)
        N = shape[0] if len(shape) == 4 else 1
        pb = shape[-1]
        if shape[-3:-1] != plan.src_shape or int(np.prod(out_dev.shape)) != N * plan.dst_shape[0] * plan.dst_shape[1] * 3:
            raise L.FaststyleError("cvresize_u8: source %s / destination %s do not fit the plan %s -> %s" % (shape, tuple(out_dev.shape), plan.src_shape,
                                                                                                          plan.dst_shape))
        if plan.tables_dev is None and plan.tables.size:
            plan.tables_dev = self.mem.upload_u8(plan.tables)
        tab = self.mem.ptr_u8(plan.tables_dev) if plan.tables_dev is not None else None
        L.check(self.lib, self.lib.fs_cvresize_u8(self.ctx, ctypes.byref(plan.info), tab, self.mem.ptr_u8(src_dev), pb, N, 1 if swap_rb else 0,
                                                  self.mem.ptr_u8(out_dev)), "fs_cvresize_u8")
        return out_dev

    def cvresize(self, img, fx, fy, interpolation=None, swap_rb=False):
        """Host uint8 [H,W,3] -> host uint8 [Hd,Wd,3]: upload, cvresize_u8, download (utils.imresize with an engine)."""
        img = np.ascontiguousarray(img, dtype=np.uint8)
        plan = self.cvresize_plan(img.shape[0], img.shape[1], fx, fy, interpolation)
        out = self.mem.upload_u8(np.zeros(plan.dst_shape + (3,), np.uint8))
        self.cvresize_u8(self.mem.upload_u8(img), plan, out, swap_rb=swap_rb)
        return np.array(self.mem.to_numpy(out), copy=True)

    # ------------------------------------------------------------------ planar YCbCr <-> packed RGB (csrc/fs_yuv.hip)
    def _yuv_count(self, desc, yuv_dev, rgb_dev, what):
        """(N, pixel_bytes) of a pair of device buffers: yuv_dev holds N frames of desc.frame_bytes, rgb_dev [N,]H,W,3|4."""
        shape = tuple(int(d) for d in rgb_dev.shape)
        pb = shape[-1]
        N = int(np.prod(yuv_dev.shape)) // int(desc.frame_bytes)
        if len(shape) not in (3, 4) or shape[-3:-1] != (int(desc.height), int(desc.width)) or N < 1 or \
                N * int(desc.frame_bytes) != int(np.prod(yuv_dev.shape)) or int(np.prod(shape[:-3])) != N:
            raise L.FaststyleError("%s: planes %s / pixels %s do not fit %dx%d frames of %d bytes" % (what, tuple(yuv_dev.shape), shape, desc.width,
                                                                                                  desc.height, desc.frame_bytes))
        return N, pb

    def yuv_to_rgb_u8(self, yuv_dev, desc, out_dev, swap_rb=False):
        """fs_yuv_to_rgb_u8: yuv_dev device uint8 [frame_bytes] or [N, frame_bytes] (the planes as YUV4MPEG2 stores them) -> out_dev device
        uint8 [H,W,3|4] / [N,H,W,3|4] (4: RGBX); swap_rb: written B,G,R."""
        self._sync_stream()
        N, pb = self._yuv_count(desc, yuv_dev, out_dev, "yuv_to_rgb_u8")
        L.check(self.lib, self.lib.fs_yuv_to_rgb_u8(self.ctx, ctypes.byref(desc), self.mem.ptr_u8(yuv_dev), N, pb, 1 if swap_rb else 0,
                                                    self.mem.ptr_u8(out_dev)), "fs_yuv_to_rgb_u8")
        return out_dev

    def rgb_to_yuv_u8(self, rgb_dev, desc, out_dev, swap_rb=False):
        """fs_rgb_to_yuv_u8: rgb_dev device uint8 [H,W,3|4] / [N,H,W,3|4] (swap_rb: the pixels are B,G,R) -> out_dev device uint8
        [frame_bytes] / [N, frame_bytes]."""
        self._sync_stream()
        N, pb = self._yuv_count(desc, out_dev, rgb_dev, "rgb_to_yuv_u8")
        L.check(self.lib, self.lib.fs_rgb_to_yuv_u8(self.ctx, ctypes.byref(desc), self.mem.ptr_u8(rgb_dev), pb, 1 if swap_rb else 0, N,
                                                    self.mem.ptr_u8(out_dev)), "fs_rgb_to_yuv_u8")
        return out_dev

    # ------------------------------------------------------------------ planar YCbCr of 9 to 16 bits <-> fp32 RGB (csrc/fs_yuv16.hip)
    def yuv_deep_to_f32(self, yuv_dev, desc, out_f32, swap_rb=False):
        """fs_yuv_deep_to_f32: yuv_dev device uint8 [frame_bytes] or [N, frame_bytes] (16-bit little-endian samples, desc of yuv_plan with
        bits > 8) -> out_f32 device float32 [H,W,3] / [N,H,W,3] on the net's 0..255 scale; swap_rb: written B,G,R."""
        self._sync_stream()
        N, pb = self._yuv_count(desc, yuv_dev, out_f32, "yuv_deep_to_f32")
        if pb != 3:
            raise L.FaststyleError("yuv_deep_to_f32: the destination %s is not [..., 3]" % (tuple(out_f32.shape),))
        L.check(self.lib, self.lib.fs_yuv_deep_to_f32(self.ctx, ctypes.byref(desc), self.mem.ptr_u8(yuv_dev), N, 1 if swap_rb else 0,
                                                      self.mem.ptr(out_f32)), "fs_yuv_deep_to_f32")
        return out_f32

    def f32_to_yuv_deep(self, f32_dev, desc, out_dev, swap_rb=False):
        """fs_f32_to_yuv_deep: f32_dev device float32 [H,W,3] / [N,H,W,3] (swap_rb: the channels are B,G,R) -> out_dev device uint8
        [frame_bytes] / [N, frame_bytes], 16-bit little-endian samples."""
        self._sync_stream()
        N, pb = self._yuv_count(desc, out_dev, f32_dev, "f32_to_yuv_deep")
        if pb != 3:
            raise L.FaststyleError("f32_to_yuv_deep: the source %s is not [..., 3]" % (tuple(f32_dev.shape),))
        L.check(self.lib, self.lib.fs_f32_to_yuv_deep(self.ctx, ctypes.byref(desc), self.mem.ptr(f32_dev), 1 if swap_rb else 0, N,
                                                      self.mem.ptr_u8(out_dev)), "fs_f32_to_yuv_deep")
        return out_dev

    # ------------------------------------------------------------------ strength, colour preservation, mask (csrc/fs_compose.hip)
    def compose_f32(self, src, net, dst, strength_q8=256, keep_color=False, matrix="bt601", bgr=False, mask=None, src_swapped=False):
        """fs_compose_f32: src device float32 [H,W,3] / [N,H,W,3] (the net's input), net and dst device float32 [Ho,Wo,3] / [N,Ho,Wo,3] (the
        net's output and the composed tensor; dst may be net) -> dst = src + (net - src) * strength_q8 / 256 * mask on the 8.8 scale, under
        keep_color with the luma delta (matrix 'bt601' / 'bt709' or 0 / 1; bgr: channel 0 of net is blue) on every channel.  mask: device
        uint8 [H,W].  src_swapped: src holds R and B the other way round than net and is read with them exchanged (the call's bgr + 2)."""
        self._sync_stream()
        ss, ns = tuple(int(d) for d in src.shape), tuple(int(d) for d in net.shape)
        if len(ss) not in (3, 4) or len(ns) != len(ss) or ss[-1] != 3 or ns[-1] != 3 or tuple(int(d) for d in dst.shape) != ns or \
                (len(ss) == 4 and ss[0] != ns[0]) or (mask is not None and tuple(int(d) for d in mask.shape) != ss[-3:-1]):
            raise L.FaststyleError("compose_f32: source %s / net output %s / destination %s / mask %s do not belong together" %
                                   (ss, ns, tuple(dst.shape), None if mask is None else tuple(mask.shape)))
        matrix = {"bt601": 0, "bt709": 1}.get(matrix, matrix)
        L.check(self.lib, self.lib.fs_compose_f32(self.ctx, self.mem.ptr(src), ss[-3], ss[-2], self.mem.ptr(net), ns[-3], ns[-2],
                                                  ss[0] if len(ss) == 4 else 1, int(strength_q8), 1 if keep_color else 0, int(matrix),
                                                  (1 if bgr else 0) + (2 if src_swapped else 0),
                                                  None if mask is None else self.mem.ptr_u8(mask), self.mem.ptr(dst)),
                "fs_compose_f32")
        return dst

    # ------------------------------------------------------------------ two nets' outputs merged (csrc/fs_mix.hip)
    def i32_buffer(self, values):
        """A device buffer of int32 entries holding ``values``: the memory backend's uint8 buffer of four bytes per entry (both backends
        allocate at 16 bytes or better), which mix_f32(weights=) and i32_upload take."""
        return self.mem.upload_u8(np.ascontiguousarray(values, dtype="<i4").reshape(-1).view(np.uint8))

    def i32_staging(self, n):
        """A host staging buffer of n int32 entries for i32_upload (pinned on the GPU engine): (numpy int32 view, the buffer)."""
        if hasattr(self.mem, "torch"):
            t = self.mem.torch.zeros(4 * int(n), dtype=self.mem.torch.uint8, pin_memory=True)
            return t.numpy().view("<i4"), t
        a = np.zeros(int(n), "<i4")
        return a, a.view(np.uint8)

    def i32_upload(self, buf, values, staging):
        """``values`` -> the entries of an i32_buffer, through ``staging`` (i32_staging's) with an asynchronous copy on the current stream:
        the host does not wait, and the caller rewrites the staging buffer only after that copy has completed."""
        staging[0][...] = np.asarray(values, dtype="<i4").reshape(-1)
        if hasattr(self.mem, "torch"):
            buf.copy_(staging[1], non_blocking=True)
        else:
            buf[...] = staging[1]
        return buf

    def _i32_ptr(self, buf, n, what):
        """The address of a device buffer of n int32 entries: an i32_buffer, or the backend's own int32 array"""
        if str(buf.dtype).endswith("int32"):
            ok, ptr = int(np.prod(tuple(buf.shape))) == n, (buf.data_ptr() if hasattr(buf, "data_ptr") else buf.ctypes.data)
        else:
            ok, ptr = str(buf.dtype).endswith("uint8") and int(np.prod(tuple(buf.shape))) == 4 * n, None
            ptr = self.mem.ptr_u8(buf) if ok else None
        if not ok:
            raise L.FaststyleError("%s: the weights are a device buffer of %d int32 entries (i32_buffer), got %s %s" %
                                   (what, n, tuple(buf.shape), buf.dtype))
        return ptr

    def mix_f32(self, a, b, dst, weight_q8=256, weights=None, mask=None, in_hw=None):
        """fs_mix_f32: a, b and dst device float32 [Ho,Wo,3] / [N,Ho,Wo,3] (two nets' outputs and the mixed tensor; dst may be a or b, a may
        be b) -> dst = a + (b - a) * weight / 256 * mask on the 8.8 scale.  weight_q8 in [0, 256] serves every image; weights: a device
        buffer of N int32 entries (i32_buffer), one weight per image, read and clamped to [0, 256] by the kernel, takes its place.  mask:
        device uint8 [H,W] at the net's input size in_hw = (H, W), H <= Ho <= H + 3 and W <= Wo <= W + 3; in_hw defaults to the mask's shape,
        without a mask to (Ho, Wo)."""
        self._sync_stream()
        sa, sb, sd = (tuple(int(d) for d in t.shape) for t in (a, b, dst))
        ms = None if mask is None else tuple(int(d) for d in mask.shape)
        if in_hw is None:
            in_hw = ms if ms is not None and len(ms) == 2 else sa[-3:-1]
        in_hw = tuple(int(d) for d in in_hw)
        if len(sa) not in (3, 4) or sa[-1] != 3 or sb != sa or sd != sa or len(in_hw) != 2 or (ms is not None and ms != in_hw):
            raise L.FaststyleError("mix_f32: outputs %s and %s / destination %s / mask %s / input size %s do not belong together" %
                                   (sa, sb, sd, ms, in_hw))
        N = sa[0] if len(sa) == 4 else 1
        L.check(self.lib, self.lib.fs_mix_f32(self.ctx, self.mem.ptr(a), self.mem.ptr(b), in_hw[0], in_hw[1], sa[-3], sa[-2], N, int(weight_q8),
                                              None if weights is None else self._i32_ptr(weights, N, "mix_f32"),
                                              None if mask is None else self.mem.ptr_u8(mask), self.mem.ptr(dst)), "fs_mix_f32")
        return dst

    # ------------------------------------------------------------------ resampling between fp32 tensors (csrc/fs_resample.hip)
    def resample_f32(self, src, plan, dst):
        """fs_resample_f32: src device float32 [Hs,Ws,3] / [N,Hs,Ws,3] -> dst device float32 [Hd,Wd,3] / [N,Hd,Wd,3], Pillow's resize of
        mode-F images per channel with the plan's filter.  The crop form: a source [N,R,P,3] / [R,P,3] with R >= Hs and P >= Ws, whose
        top-left Hs x Ws is read and whose margin never is.  The plan's tables go to the device on its first use."""
        self._sync_stream()
        ss, ds = tuple(int(d) for d in src.shape), tuple(int(d) for d in dst.shape)
        Hs, Ws = plan.src_shape
        if len(ss) not in (3, 4) or len(ds) != len(ss) or ss[-1] != 3 or ds[-3:] != plan.dst_shape + (3,) or ss[-3] < Hs or ss[-2] < Ws or \
                (len(ss) == 4 and ss[0] != ds[0]):
            raise L.FaststyleError("resample_f32: source %s / destination %s do not fit the plan %s -> %s" % (ss, ds, plan.src_shape, plan.dst_shape))
        if plan.tables_dev is None and plan.tables.size:
            plan.tables_dev = self.mem.upload_u8(plan.tables)
        tab = self.mem.ptr_u8(plan.tables_dev) if plan.tables_dev is not None else None
        L.check(self.lib, self.lib.fs_resample_f32(self.ctx, ctypes.byref(plan.info), tab, self.mem.ptr(src), ss[-3], ss[-2],
                                                   ss[0] if len(ss) == 4 else 1, self.mem.ptr(dst)), "fs_resample_f32")
        return dst

    # ------------------------------------------------------------------ guided delivery (csrc/fs_guided.hip)
    def guided_workspace_bytes(self, H, W, N=1):
        """fs_guided_workspace: the bytes of the workspace of guided_f32 for N images on an H x W grid (host only)."""
        n = ctypes.c_size_t()
        L.check(self.lib, self.lib.fs_guided_workspace(int(H), int(W), int(N), ctypes.byref(n)), "fs_guided_workspace")
        return int(n.value)

    def guided_workspace(self, H, W, N=1):
        """The workspace of guided_f32 as a device uint8 buffer (the memory backend's): coef [N,H,W,6] int32 in its first half, mean
        [N,H,W,6] int32 in its second (each half N H W 24 bytes rounded up to a multiple of 16; guided_parts reads them)."""
        return self.mem.upload_u8(np.zeros((self.guided_workspace_bytes(H, W, N),), np.uint8))

    def guided_parts(self, work, H, W, N=1):
        """For tests and debugging: what guided_f32 left in its workspace, as host arrays -> (coef, mean), int32 [N,H,W,6] (synchronises)."""
        raw = np.array(self.mem.to_numpy(work), dtype=np.uint8, copy=True).reshape(-1)
        if raw.size != self.guided_workspace_bytes(H, W, N):
            raise L.FaststyleError("guided_parts: not the workspace of %d %dx%d images (guided_workspace)" % (N, H, W))
        n = int(N) * int(H) * int(W) * 24
        return tuple(raw[o:o + n].view(np.int32).reshape(int(N), int(H), int(W), 6) for o in (0, raw.size // 2))

    def guided_f32(self, lo_src, lo_out, hi_src, dst, work, radius=2, smoothness=4, matrix="bt601", lo_bgr=False, hi_bgr=False):
        """fs_guided_f32: lo_src device float32 [H,W,3] / [N,H,W,3] (the net's input), lo_out device float32 [Ho,Wo,3] / [N,Ho,Wo,3] (the
        net's, composed or stabilised output), hi_src the source at the delivery size -- device uint8 [..,Hd,Wd,3] (kind 0), uint8
        [..,Hd,Wd,4] (kind 1) or float32 [..,Hd,Wd,3] (kind 2) --, dst device float32 [..,Hd,Wd,3], work guided_workspace(H, W, N) -> dst =
        the guided upsampling of lo_out: per channel a * luma(hi_src) + b with the window-averaged coefficients of the local linear model
        lo_out ~ a * luma(lo_src) + b, interpolated bilinearly.  matrix 'bt601' / 'bt709' or 0 / 1; lo_bgr / hi_bgr: channel 0 of lo_src /
        hi_src is blue."""
        self._sync_stream()
        ss, os_, hs, ds = (tuple(int(d) for d in t.shape) for t in (lo_src, lo_out, hi_src, dst))
        is_u8 = str(hi_src.dtype).endswith("uint8")
        kind = (0 if hs[-1:] == (3,) else 1) if is_u8 else 2
        if len(ss) not in (3, 4) or len(os_) != len(ss) or len(hs) != len(ss) or len(ds) != len(ss) or ss[-1] != 3 or os_[-1] != 3 or \
                hs[-1] != (4 if kind == 1 else 3) or (is_u8 and hs[-1] not in (3, 4)) or ds != hs[:-1] + (3,) or \
                (len(ss) == 4 and not ss[0] == os_[0] == hs[0]) or not (is_u8 or str(hi_src.dtype).endswith("float32")):
            raise L.FaststyleError("guided_f32: net input %s / output %s / source %s %s / destination %s do not belong together" %
                                   (ss, os_, hs, hi_src.dtype, ds))
        N = ss[0] if len(ss) == 4 else 1
        nbytes = int(np.prod(tuple(int(d) for d in work.shape)))
        if not str(work.dtype).endswith("uint8"):
            raise L.FaststyleError("guided_f32: the workspace is a uint8 buffer (guided_workspace), got %s" % (work.dtype,))
        matrix = {"bt601": 0, "bt709": 1}.get(matrix, matrix)
        hp = self.mem.ptr_u8(hi_src) if is_u8 else self.mem.ptr(hi_src)
        L.check(self.lib, self.lib.fs_guided_f32(self.ctx, self.mem.ptr(lo_src), ss[-3], ss[-2], self.mem.ptr(lo_out), os_[-3], os_[-2], hp, kind,
                                                 hs[-3], hs[-2], N, int(radius), int(smoothness), int(matrix), 1 if lo_bgr else 0,
                                                 1 if hi_bgr else 0, self.mem.ptr_u8(work), nbytes, self.mem.ptr(dst)), "fs_guided_f32")
        return dst

    # ------------------------------------------------------------------ temporal stabilisation (csrc/fs_temporal.hip)
    def temporal_pyr_layout(self, Ho, Wo, levels):
        """fs_temporal_pyr_layout: the level sizes, block counts and offsets of the extra state buffer of a `levels`-level search (host only)."""
        info = L.fs_temporal_pyr_info()
        L.check(self.lib, self.lib.fs_temporal_pyr_layout(int(Ho), int(Wo), int(levels), ctypes.byref(info)), "fs_temporal_pyr_layout")
        return info

    def temporal_state(self, Ho, Wo, levels=1, subpel=0):
        """One state slot of fs_temporal_f32 for an Ho x Wo output, as device uint8 buffers (the memory backend's): (luma [Ho,Wo], out88
        [Ho,Wo,3,2] -- little-endian u16 on the 8.8 scale --, mv [nby,nbx,2] -- signed char (dy, dx) per 16 x 16 block).  levels > 1
        (fs_temporal_pyr_f32) appends pyr [pyr_bytes]: the halved lumas and the coarse vectors, laid out as temporal_pyr_layout says.
        subpel > 0 (fs_temporal_sub_f32) appends mvf [nby,nbx,2] as the last buffer: signed char (fy, fx) per block, in quarter pixels."""
        Ho, Wo = int(Ho), int(Wo)
        up = self.mem.upload_u8
        slot = (up(np.zeros((Ho, Wo), np.uint8)), up(np.zeros((Ho, Wo, 3, 2), np.uint8)), up(np.zeros(((Ho + 15) // 16, (Wo + 15) // 16, 2), np.uint8)))
        if subpel != 0:
            self._temporal_whole(levels=levels, subpel=subpel)
        if levels != 1:
            slot = slot + (up(np.zeros((int(self.temporal_pyr_layout(Ho, Wo, levels).pyr_bytes),), np.uint8)),)
        if subpel != 0:
            slot = slot + (up(np.zeros(((Ho + 15) // 16, (Wo + 15) // 16, 2), np.uint8)),)
        return slot

    def temporal_pyramid(self, state, Ho, Wo, levels):
        """For tests and debugging: what a slot of a `levels`-level search holds beyond level 0, as host arrays -> (lumas, vectors), the
        uint8 [H_l,W_l] lumas and the int8 [nby_l,nbx_l,2] vectors of the levels 1 .. levels - 1 (synchronises)."""
        lay = self.temporal_pyr_layout(Ho, Wo, levels)
        if levels > 1 and (len(state) != 4 or int(np.prod(state[3].shape)) != lay.pyr_bytes):
            raise L.FaststyleError("temporal_pyramid: not the slot of a %dx%d output with %d levels (temporal_state)" % (Ho, Wo, levels))
        raw = np.array(self.mem.to_numpy(state[3]), dtype=np.uint8, copy=True).reshape(-1) if levels > 1 else None
        lumas, vectors = [], []
        for l in range(1, levels):
            h, w, nby, nbx = lay.h[l], lay.w[l], lay.nby[l], lay.nbx[l]
            lumas.append(raw[lay.luma_offset[l]:lay.luma_offset[l] + h * w].reshape(h, w))
            vectors.append(raw[lay.mv_offset[l]:lay.mv_offset[l] + nby * nbx * 2].view(np.int8).reshape(nby, nbx, 2))
        return lumas, vectors

    def temporal_f32(self, src, cur, dst, state, prev=None, strength_q8=256, sensitivity=16, radius=7, matrix="bt601", src_bgr=False, levels=1,
                     subpel=0, overlap=0):
        """fs_temporal_f32: src device float32 [H,W,3] (the net's input), cur and dst device float32 [Ho,Wo,3] (the tensor the output
        conversions would read and the stabilised one; dst may be cur; a leading axis of 1 is taken), state the slot written (temporal_state's
        triple), prev the slot the previous frame wrote (None: no previous frame) -> dst = cur blended towards prev's output along the
        block vectors found between the two lumas; matrix 'bt601' / 'bt709' or 0 / 1, src_bgr: channel 0 of src is blue.  levels > 1:
        fs_temporal_pyr_f32, the coarse-to-fine search, on slots of temporal_state(Ho, Wo, levels).  subpel 1 / 2: fs_temporal_sub_f32, vectors
        in half / quarter pixels and a bilinear fetch, on slots of temporal_state(Ho, Wo, levels, subpel).  overlap 1: fs_temporal_obmc_f32,
        every pixel blended along the vectors of the four blocks around it, on the slots that (levels, subpel) take without it."""
        return self._temporal_call("temporal_f32", False, src, cur, dst, state, None, prev, strength_q8, sensitivity, radius, matrix, src_bgr, levels,
                                   subpel, overlap)

    @staticmethod
    def _temporal_whole(who="temporal_f32", **options):
        """The temporal options given by name are whole numbers in their ranges."""
        for name, v in options.items():
            lo, hi = {"levels": (1, 3), "subpel": (0, 2), "overlap": (0, 1)}[name]
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise L.FaststyleError("%s: %s must be a whole number in [%d, %d], got %r" % (who, name, lo, hi, v))

    # the single-frame entry points, narrowest first: (function, takes levels and the pyramid buffers, takes subpel and mvf, takes overlap)
    _TEMPORAL_ENTRIES = (("fs_temporal_f32", False, False, False), ("fs_temporal_pyr_f32", True, False, False),
                         ("fs_temporal_sub_f32", True, True, False), ("fs_temporal_obmc_f32", True, True, True))

    def _temporal_call(self, who, batch, src, cur, dst, state, work, prev, strength_q8, sensitivity, radius, matrix, src_bgr, levels, subpel, overlap):
        """temporal_f32 (one image; the narrowest entry point that takes the keys that are not at their defaults, so that every exported
        wrapper is reached through it) and temporal_batch_f32 (batch: N frames, fs_temporal_batch_f32): the options' and shapes' checks, the
        slots held against (levels, subpel) -- the pyramid buffer fourth when levels > 1, mvf last when subpel > 0 --, then the call."""
        self._sync_stream()
        fn, has_levels, has_subpel, has_overlap = ("fs_temporal_batch_f32", True, True, True) if batch else \
            self._TEMPORAL_ENTRIES[3 if overlap != 0 else 2 if subpel != 0 else 1 if levels != 1 else 0]
        if has_levels:                                      # (an option the function lacks is at its default)
            self._temporal_whole(levels=levels)
        if has_subpel:
            self._temporal_whole(subpel=subpel)
        if has_overlap:
            self._temporal_whole(who, overlap=overlap)
        ss, cs, ds = (tuple(int(d) for d in t.shape) for t in (src, cur, dst))
        if not batch and not (len(ss) == 4 and len(cs) == 4 and ss[0] == 1 and cs[0] == 1 and ds[:1] == (1,)):
            ss, cs, ds = (1,) + ss, (1,) + cs, (1,) + ds                                    # (one image: a leading axis of 1 is taken)
        if len(ss) != 4 or len(cs) != 4 or ss[3] != 3 or cs[3] != 3 or ds != cs or ss[0] != cs[0]:
            raise L.FaststyleError("%s: source %s / current %s / destination %s do not belong together (%s)" %
                                   (who, tuple(src.shape), tuple(cur.shape), tuple(dst.shape),
                                    "[N,H,W,3] / [N,Ho,Wo,3] each" if batch else "one image per call"))
        N, Ho, Wo = cs[:3]
        if not 1 <= N <= 64:
            raise L.FaststyleError("%s: 1 to 64 frames per call, got %d" % (who, N))
        blocks = ((Ho + 15) // 16, (Wo + 15) // 16, 2)
        want = ((Ho, Wo), (Ho, Wo, 3, 2), blocks)
        if levels > 1:
            want += ((int(self.temporal_pyr_layout(Ho, Wo, levels).pyr_bytes),),)
        if subpel > 0:
            want += (blocks,)
        for name, slot in (("state", state), ("prev", prev)):
            if slot is not None and (len(slot) != len(want) or tuple(tuple(int(d) for d in b.shape) for b in slot) != want):
                raise L.FaststyleError("%s: %s is not the slot of a %dx%d output%s (temporal_state)" % (
                    who, name, Ho, Wo, " with %d levels and subpel %d" % (levels, subpel) if has_subpel else
                    " with %d levels" % levels if has_levels else ""))
        nbytes = 0 if work is None else int(np.prod(work.shape))
        if batch:
            need = int(self.temporal_batch_layout(Ho, Wo, N, levels, subpel).work_bytes)
            if nbytes < need:
                raise L.FaststyleError("%s: %d frames of %dx%d need a work buffer of %d bytes (temporal_batch_work), got %d" %
                                       (who, N, Ho, Wo, need, nbytes))
        matrix = {"bt601": 0, "bt709": 1}.get(matrix, matrix)
        p8 = self.mem.ptr_u8
        pyr = (lambda slot: p8(slot[3])) if levels > 1 else (lambda slot: None)
        pl, po, pp = (None, None, None) if prev is None else (p8(prev[0]), p8(prev[1]), pyr(prev))
        args = [self.ctx, self.mem.ptr(src), ss[1], ss[2], self.mem.ptr(cur), Ho, Wo] + [N] * batch + [int(strength_q8), int(sensitivity), int(radius)] + \
            [int(levels)] * has_levels + [int(subpel)] * has_subpel + [int(overlap)] * has_overlap + [int(matrix), 1 if src_bgr else 0, pl, po] + \
            [pp] * has_levels + [p8(state[0]), p8(state[1])] + [pyr(state)] * has_levels + [p8(state[2])] + \
            [p8(state[-1]) if subpel > 0 else None] * has_subpel + [None if work is None else p8(work), nbytes] * batch + [self.mem.ptr(dst)]
        L.check(self.lib, getattr(self.lib, fn)(*args), fn)
        return dst

    def temporal_batch_layout(self, Ho, Wo, frames, levels=1, subpel=0):
        """fs_temporal_batch_layout: the size of the work buffer of `frames` consecutive frames per call and where the vectors of the frames
        before the last lie in it (host only)."""
        info = L.fs_temporal_batch_info()
        L.check(self.lib, self.lib.fs_temporal_batch_layout(int(Ho), int(Wo), int(levels), int(subpel), int(frames), ctypes.byref(info)),
                "fs_temporal_batch_layout")
        return info

    def temporal_batch_work(self, Ho, Wo, frames, levels=1, subpel=0):
        """The work buffer of temporal_batch_f32 as a device uint8 buffer (the memory backend's) of temporal_batch_layout's work_bytes (at
        least 16, so that one frame per call has a buffer too)."""
        return self.mem.upload_u8(np.zeros((max(16, int(self.temporal_batch_layout(Ho, Wo, frames, levels, subpel).work_bytes)),), np.uint8))

    def temporal_batch_f32(self, src, cur, dst, state, work, prev=None, strength_q8=256, sensitivity=16, radius=7, matrix="bt601", src_bgr=False,
                           levels=1, subpel=0, overlap=0):
        """fs_temporal_batch_f32: temporal_f32 over N consecutive frames of one stream, oldest first -- src device float32 [N,H,W,3], cur and dst
        [N,Ho,Wo,3] (dst may be cur), state the slot that receives frame N - 1's state, prev the slot the previous call wrote (None: no previous
        frame before frame 0), both temporal_state(Ho, Wo, levels, subpel)'s; work temporal_batch_work's for at least N frames.  dst[i] is what
        the i-th of N chained temporal_f32 calls gives, bit for bit."""
        return self._temporal_call("temporal_batch_f32", True, src, cur, dst, state, work, prev, strength_q8, sensitivity, radius, matrix, src_bgr,
                                   levels, subpel, overlap)

    def temporal_batch_vectors(self, work, state, Ho, Wo, frames, levels=1, subpel=0):
        """For tests and motion_vectors(): the vectors of every frame of the last temporal_batch_f32 call as host arrays -> (mv int8
        [frames,nby,nbx,2], mvf likewise or None with subpel 0): the frames before the last from `work`, the last from `state` (synchronises)."""
        lay = self.temporal_batch_layout(Ho, Wo, frames, levels, subpel)
        nby, nbx = (int(Ho) + 15) // 16, (int(Wo) + 15) // 16
        n = nby * nbx * 2
        raw = np.array(self.mem.to_numpy(work), dtype=np.uint8, copy=True).reshape(-1) if frames > 1 else None

        def gather(offset, stride, last):
            rows = [raw[offset + i * stride:offset + i * stride + n] for i in range(frames - 1)]
            rows.append(np.array(self.mem.to_numpy(last), dtype=np.uint8, copy=True).reshape(-1))
            return np.stack(rows).view(np.int8).reshape(frames, nby, nbx, 2)
        mv = gather(int(lay.mv_offset), int(lay.mv_stride), state[2])
        return mv, (gather(int(lay.mvf_offset), int(lay.mvf_stride), state[-1]) if subpel > 0 else None)

    def temporal_streams_layout(self, Ho, Wo, streams, levels=1, subpel=0):
        """fs_temporal_streams_layout: where the parts of a slot lie, the strides of a slot and of a stream and the size of the state buffer of
        `streams` independent streams (host only)."""
        info = L.fs_temporal_streams_info()
        L.check(self.lib, self.lib.fs_temporal_streams_layout(int(Ho), int(Wo), int(levels), int(subpel), int(streams), ctypes.byref(info)),
                "fs_temporal_streams_layout")
        return info

    def temporal_streams_state(self, Ho, Wo, streams, levels=1, subpel=0):
        """The state of temporal_streams_f32 as one device uint8 buffer (the memory backend's) of temporal_streams_layout's state_bytes."""
        return self.mem.upload_u8(np.zeros((int(self.temporal_streams_layout(Ho, Wo, streams, levels, subpel).state_bytes),), np.uint8))

    def temporal_streams_f32(self, src, cur, dst, ctl, state, strength_q8=256, sensitivity=16, radius=7, matrix="bt601", src_bgr=False, levels=1,
                             subpel=0, overlap=0):
        """fs_temporal_streams_f32: temporal_f32 over one frame of each of S independent streams -- src device float32 [S,H,W,3], cur and dst
        [S,Ho,Wo,3] (dst may be cur), ctl a device buffer of S int32 control words (i32_buffer; FS_TS_PREV, FS_TS_SLOT, FS_TS_SKIP per stream),
        state temporal_streams_state's for at least S streams.  Stream s gets what temporal_f32 gives image s with the slot the word names,
        bit for bit; a skipped stream is not touched."""
        self._sync_stream()
        who = "temporal_streams_f32"
        self._temporal_whole(who, levels=levels, subpel=subpel, overlap=overlap)
        ss, cs, ds = (tuple(int(d) for d in t.shape) for t in (src, cur, dst))
        if len(ss) != 4 or len(cs) != 4 or ss[3] != 3 or cs[3] != 3 or ds != cs or ss[0] != cs[0]:
            raise L.FaststyleError("%s: source %s / current %s / destination %s do not belong together ([S,H,W,3] / [S,Ho,Wo,3] each)" %
                                   (who, tuple(src.shape), tuple(cur.shape), tuple(dst.shape)))
        S, Ho, Wo = cs[:3]
        if not 1 <= S <= 64:
            raise L.FaststyleError("%s: 1 to 64 streams per call, got %d" % (who, S))
        need = int(self.temporal_streams_layout(Ho, Wo, S, levels, subpel).state_bytes)
        nbytes = int(np.prod(state.shape))
        if not str(state.dtype).endswith("uint8") or nbytes < need:
            raise L.FaststyleError("%s: %d streams of %dx%d need a state buffer of %d bytes (temporal_streams_state), got %s of %d" %
                                   (who, S, Ho, Wo, need, state.dtype, nbytes))
        matrix = {"bt601": 0, "bt709": 1}.get(matrix, matrix)
        L.check(self.lib, self.lib.fs_temporal_streams_f32(self.ctx, self.mem.ptr(src), ss[1], ss[2], self.mem.ptr(cur), Ho, Wo, S, int(strength_q8),
                                                           int(sensitivity), int(radius), int(levels), int(subpel), int(overlap), int(matrix),
                                                           1 if src_bgr else 0, self._i32_ptr(ctl, S, who), self.mem.ptr_u8(state), nbytes,
                                                           self.mem.ptr(dst)), "fs_temporal_streams_f32")
        return dst

    def temporal_streams_slot(self, state, ctl_host, stream, Ho, Wo, levels=1, subpel=0, written=True):
        """For tests and inspection: one slot of one stream as host arrays -> dict(luma uint8 [Ho,Wo], out88 uint16 [Ho,Wo,3], pyr uint8
        [pyr_bytes], mv int8 [nby,nbx,2], mvf likewise or None with subpel 0): the slot that the pass with the host control words ctl_host
        wrote, or with written=False the other one (synchronises)."""
        S = len(ctl_host)
        lay = self.temporal_streams_layout(Ho, Wo, S, levels, subpel)
        Ho, Wo = int(Ho), int(Wo)
        nby, nbx = (Ho + 15) // 16, (Wo + 15) // 16
        w = (int(ctl_host[stream]) >> 1 & 1) ^ (0 if written else 1)
        base = int(stream) * int(lay.stream_stride) + w * int(lay.slot_stride)
        raw = np.array(self.mem.to_numpy(state), dtype=np.uint8, copy=True).reshape(-1)[base:base + int(lay.slot_stride)]
        part = lambda off, n: raw[int(off):int(off) + n]
        return dict(luma=part(lay.luma_offset, Ho * Wo).reshape(Ho, Wo), out88=part(lay.out88_offset, Ho * Wo * 6).view("<u2").reshape(Ho, Wo, 3),
                    pyr=part(lay.pyr_offset, int(lay.mv_offset - lay.pyr_offset)), mv=part(lay.mv_offset, nby * nbx * 2).view(np.int8).reshape(nby, nbx, 2),
                    mvf=part(lay.mvf_offset, nby * nbx * 2).view(np.int8).reshape(nby, nbx, 2) if subpel > 0 else None)

    def temporal_streams_vectors(self, state, ctl_host, Ho, Wo, levels=1, subpel=0):
        """For tests and motion_vectors(): every stream's vectors from the slot that the pass with the host control words ctl_host wrote (a
        skipped stream's: from the slot the word names, whatever it holds) -> (mv int8 [S,nby,nbx,2], mvf likewise or None with subpel 0)
        (synchronises)."""
        slots = [self.temporal_streams_slot(state, ctl_host, s, Ho, Wo, levels, subpel) for s in range(len(ctl_host))]
        return np.stack([t["mv"] for t in slots]), (np.stack([t["mvf"] for t in slots]) if subpel > 0 else None)

    def synth_uniform(self, out, seed, rank, batch_index):
        """Uniform [0,255) float32 values into ``out``: Philox4x32-10 keyed by seed, counter (element block, batch_index, rank) (fs_synth_uniform)."""
        self._sync_stream()
        L.check(self.lib, self.lib.fs_synth_uniform(self.ctx, self.mem.ptr(out), int(np.prod(out.shape)), int(seed) & (2 ** 64 - 1),
                                                    int(rank) & 0xFFFFFFFF, int(batch_index) & (2 ** 64 - 1)), "fs_synth_uniform")
        return out

    def u8_to_f32(self, src_u8, dst):
        """device u8 buffer -> device float32 (same element order)."""
        self._sync_stream()
        n = int(np.prod(dst.shape))
        L.check(self.lib, self.lib.fs_u8_to_f32(self.ctx, self.mem.ptr_u8(src_u8), n, self.mem.ptr(dst)), "fs_u8_to_f32")
        return dst

    def f32_to_u8(self, src, dst_u8, swap_rb=False):
        """device float32 [...,3] -> device u8 by truncation (numpy astype(uint8)), optional R<->B swap."""
        self._sync_stream()
        npix = int(np.prod(src.shape)) // 3
        L.check(self.lib, self.lib.fs_f32_to_u8(self.ctx, self.mem.ptr(src), npix, 1 if swap_rb else 0,
                                                self.mem.ptr_u8(dst_u8)), "fs_f32_to_u8")
        return dst_u8

    def adam_tf_step(self, p, g, m, v, t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
        """tf.train.AdamOptimizer(lr) update (train.py:203), in place; t = 1-based step."""
        self._sync_stream()
        P = self.mem.ptr
        L.check(self.lib, self.lib.fs_adam_tf_step(self.ctx, P(p), P(g), P(m), P(v), int(np.prod(p.shape)), lr, beta1,
                                                   beta2, eps, t), "fs_adam_tf_step")

    # ------------------------------------------------------------------ single ops (tests)
    def conv2d(self, x, w, stride=1, padding="SAME", **kw):
        self._sync_stream()
        d = L.fs_conv_desc()
        N, H, W, Cin = (int(s) for s in x.shape)
        KH, KW, _, Cout = (int(s) for s in w.shape[-4:])
        d.N, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride = N, H, W, Cin, Cout, KH, KW, stride
        if isinstance(padding, str):
            d.pad_mode = L.FS_PAD_SAME if padding == "SAME" else L.FS_PAD_VALID
        else:
            d.pad_mode = L.FS_PAD_EXPLICIT
            d.pad_t, d.pad_l, d.Ho, d.Wo = padding
        d.src_mode = kw.get("src_mode", 0)
        d.refl = kw.get("refl", 0)
        p = self.mem.ptr
        d.x, d.w = p(x), p(w)
        for k in ("in_a", "in_b", "bias", "add_src"):
            setattr(d, k, p(kw.get(k)))
        d.in_per_sample = int(kw.get("in_per_sample", 0))
        d.in_relu = int(kw.get("in_relu", 0))
        d.out_relu = int(kw.get("out_relu", 0))
        d.shuffle = int(kw.get("shuffle", 0))
        d.add_pad = int(kw.get("add_pad", 0))
        d.w_nstride = int(kw.get("w_nstride", 0))
        d.mask_src = p(kw.get("mask_src"))
        d.route_src = p(kw.get("route_src"))
        inb = kw.get("inb")      # (z, mean, rstd, a, b, relu): also leave the instance-norm-backward partial sums of the unit that produced z
        if kw.get("winograd") == 6:        # F(4x4,3x3), split-bf16 pipeline (fs_wino6.hip); the output extent is known only after the plan: SAME / explicit pads here
            U = self.mem.empty((self.lib.fs_wino6_filter_bytes(Cin, Cout) // 4,))
            L.check(self.lib, self.lib.fs_wino6_transform_filter(self.ctx, p(w), Cin, Cout, p(U)), "fs_wino6_transform_filter")
            ho, wo = (H, W) if isinstance(padding, str) and padding == "SAME" else ((H - 2, W - 2) if isinstance(padding, str) else (padding[2], padding[3]))
            nb = self.lib.fs_wino6_workspace_bytes(N, ho, wo, Cin, Cout)
            if kw.get("w6_chunk_tiles"):    # a smaller scratch: the launch runs in tile chunks
                nb = 36 * int(kw["w6_chunk_tiles"]) * (Cin + Cout) * 4
            ws6 = self.mem.empty((nb // 4,))
            d.w_wino6, d.w6_ws, d.w6_ws_bytes = p(U), p(ws6), nb
            self._keep = [U, ws6]
        elif kw.get("winograd") == "4t":     # F(4x4,3x3), 16-tile items (fs_wino4t.hip)
            U = self.mem.empty((36, Cin, Cout))
            L.check(self.lib, self.lib.fs_wino4t_transform_filter(self.ctx, p(w), Cin, Cout, p(U)), "fs_wino4t_transform_filter")
            d.w_wino4t = p(U)
            self._keep = [U]
        elif kw.get("winograd") == 4:     # F(4x4,3x3) (fs_wino4.hip)
            U = self.mem.empty((36, Cin, Cout))
            L.check(self.lib, self.lib.fs_wino4_transform_filter(self.ctx, p(w), Cin, Cout, p(U)), "fs_wino4_transform_filter")
            d.w_wino4 = p(U)
            self._keep = [U]
        elif kw.get("winograd"):     # F(2x2,3x3): transform the filter into a caller-owned buffer, hand it over with the conv
            U = self.mem.empty((16, Cin, Cout))
            L.check(self.lib, self.lib.fs_wino_transform_filter(self.ctx, p(w), Cin, Cout, p(U)), "fs_wino_transform_filter")
            d.w_wino = p(U)
            self._keep = [U]
        if inb is not None:      # (set before planning: the launch is then planned with 16 x 16-pixel items whatever the grid)
            d.inb_z, d.inb_mean, d.inb_rstd, d.inb_a, d.inb_b = (p(t) for t in inb[:5])
            d.inb_relu = int(inb[5])
            d.inb_rec = 16       # placeholder until the record count is known
        tiles = ctypes.c_int()
        L.check(self.lib, self.lib.fs_conv2d_plan(ctypes.byref(d), ctypes.byref(tiles)), "fs_conv2d_plan")
        if d.shuffle:
            y = self.mem.empty((N, 2 * d.Ho, 2 * d.Wo, Cout // 4))
        else:
            y = self.mem.empty((N, d.Ho, d.Wo, Cout))
        d.y = p(y)
        pool = None
        if kw.get("want_pool"):
            pool = self.mem.empty((N, d.Ho // 2, d.Wo // 2, Cout))
            d.pool_out = p(pool)
        rec = None
        if inb is not None:
            rec = self.mem.empty((N, tiles.value, Cout, 2))
            d.inb_rec = p(rec)
        stats = None
        if kw.get("want_stats"):
            stats = self.mem.empty((N, tiles.value, Cout, 3))
            d.stats = p(stats)
        L.check(self.lib, self.lib.fs_conv2d_fwd(self.ctx, ctypes.byref(d)), "fs_conv2d_fwd")
        if pool is not None:
            return y, pool
        if rec is not None:
            return y, rec
        return (y, stats, tiles.value) if kw.get("want_stats") else y

    def instnorm_finalize(self, stats, tiles, C, groups, gamma, beta, eps=1e-3):
        self._sync_stream()
        N = int(stats.shape[0])
        out = [self.mem.empty((N, C)) for _ in range(4)]
        p = self.mem.ptr
        L.check(self.lib, self.lib.fs_instnorm_finalize(self.ctx, p(stats), N, tiles, C, groups, p(gamma), p(beta), eps,
                                                        *[p(o) for o in out]), "fs_instnorm_finalize")
        return out  # mean, rstd, a, b

    def instnorm_bwd(self, gin, z, mean, rstd, a, b, mode):
        self._sync_stream()
        N, H, W, C = (int(s) for s in z.shape)
        dz = self.mem.empty(z.shape)
        dg, db = self.mem.empty((C,)), self.mem.empty((C,))
        nbytes = self.lib.fs_instnorm_bwd_workspace_bytes(N, H * W, C)
        ws = self.mem.empty((nbytes // 4,))
        p = self.mem.ptr
        L.check(self.lib, self.lib.fs_instnorm_bwd(self.ctx, p(gin), p(z), p(mean), p(rstd), p(a), p(b), mode, N, H * W, C,
                                                   p(dz), p(dg), p(db), p(ws), nbytes), "fs_instnorm_bwd")
        return dz, dg, db

    def conv2d_wgrad(self, x, dy, k, stride=1, padding="SAME", per_sample=False, scale=1.0, **kw):
        self._sync_stream()
        d = L.fs_wgrad_desc()
        N, H, W, Cin = (int(s) for s in x.shape)
        Cout = int(dy.shape[-1])
        d.N, d.H, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride = N, H, W, Cin, Cout, k, k, stride
        if isinstance(padding, str):
            d.pad_mode = L.FS_PAD_SAME if padding == "SAME" else L.FS_PAD_VALID
        else:
            d.pad_mode = L.FS_PAD_EXPLICIT
            d.pad_t, d.pad_l, d.Ho, d.Wo = padding
        d.src_mode = kw.get("src_mode", 0)
        d.refl = kw.get("refl", 0)
        p = self.mem.ptr
        d.x, d.dy = p(x), p(dy)
        d.in_a, d.in_b = p(kw.get("in_a")), p(kw.get("in_b"))
        d.in_per_sample = int(kw.get("in_per_sample", 0))
        d.in_relu = int(kw.get("in_relu", 0))
        d.per_sample = int(per_sample)
        d.scale = scale
        dw = self.mem.empty((N, Cin, Cout) if per_sample else (k, k, Cin, Cout))
        d.dw = p(dw)
        nbytes = self.lib.fs_conv2d_wgrad_workspace_bytes(ctypes.byref(d))
        ws = self.mem.empty((max(nbytes // 4, 1),))
        L.check(self.lib, self.lib.fs_conv2d_wgrad(self.ctx, ctypes.byref(d), p(ws), nbytes), "fs_conv2d_wgrad")
        return dw
