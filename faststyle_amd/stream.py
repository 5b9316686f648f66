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

With ``source=dict(height=Hs, width=Ws, interpolation=None, swap_rb=False, jpeg=None)`` the input side moves onto the device as well: pixel
frames arrive at the source size and the device pass begins with cv2.resize's resampling to the stylizer's size (fs_cvresize_u8, csrc/
fs_cvresize.hip; interpolation None: area when shrinking, cubic otherwise; swap_rb: R and B exchanged on the way, a cv2 capture's order); with
``jpeg=dict(width=, height=, components=, sampling=(hs, vs))`` (jpeg_source() builds the dict from a first file) a frame may also arrive as the
bytes of a baseline JPEG file of that geometry: fs_jpeg_parse / fs_jpeg_decode run on the host into a pinned coefficient buffer, and
fs_jpeg_reconstruct_many, the resize, the net and the optional encoder run in the captured graph.  A file that does not fit raises
FrameNotTaken before anything is enqueued; the caller decodes it with PIL and hands the pixels to the same stylizer.

Raw video (faststyle_amd/y4m.py): with ``source=dict(height=, width=, yuv=dict(sampling=(hs, vs), siting=, matrix=, full_range=, components=))``
the frames are planar 8-bit YCbCr as a YUV4MPEG2 stream stores them -- a flat uint8 array of frame_bytes, or [B, frame_bytes] -- and the device
pass begins with fs_yuv_to_rgb_u8 (csrc/fs_yuv.hip): straight into the net's input when the source has the net's size, otherwise into an RGBX
buffer that the resize reads; ``swap_rb`` of the source keeps its meaning.  Such a stylizer takes YCbCr frames only.  With
``yuv_out=dict(sampling=, siting=, matrix=, full_range=, components=3)`` (not together with ``jpeg=``) the pass ends with fs_rgb_to_yuv_u8 on the u8
frame and the stylizer returns the planes, a uint8 array of frame_bytes, instead of the pixels.

Deep video: either dict takes ``bits=N``, 9 to 16 bits per sample in little-endian 16-bit words (y4m.Reader(f, deep=True)); the frames are
still flat uint8 arrays of frame_bytes, now two bytes per sample (an array of ``<u2`` samples is taken as well).  A deep source writes the
net's fp32 input directly (fs_yuv_deep_to_f32, csrc/fs_yuv16.hip) and the pass has no fs_u8_to_f32; a deep ``yuv_out`` reads the net's fp32
output directly (fs_f32_to_yuv_deep) and the pass has no fs_f32_to_u8: no u8 stage on that side.  Either end may be deep on its own, with
the 8-bit kernels on the other.  A deep source has the net's size (the resize is u8 only); ``jpeg=`` behind a deep source works as before.

Strength, colour preservation, a region mask: with ``compose=dict(strength=1.0, keep_color=False, matrix='bt601', mask=None)`` one launch
behind the forward pass (fs_compose_f32, csrc/fs_compose.hip, inside the graph) blends the net's fp32 output back towards the net's fp32
input, which is still resident, into a tensor of the lane's own, and every output conversion above reads that tensor instead: ``strength`` in
[0, 1] (quantised to 1 / 256), ``keep_color`` the stylized luma under the source's colours (``matrix`` names the luma weights), ``mask`` a host
uint8 [H, W] at the net's input size, 0 keeps the source and 255 takes the blend.  The launch is told that the tensors are B,G,R exactly
when the lane's output conversion swaps.  ``source_swapped=True`` says that the frames reach the net with R and B the other way round than
its output is shown -- the reference's channel handling, which the command-line tools keep -- so that the source is read with the two
exchanged and shows through in its own colours.  Without ``compose=`` nothing is allocated or launched.

Temporal stabilisation: with ``temporal=dict(strength=, sensitivity=16, radius=7, matrix='bt601', source_bgr=<the lane's swap_rb>)`` three
launches behind compose (fs_temporal_f32, csrc/fs_temporal.hip) blend the tensor the output conversions would read towards the previous
frame's stabilised output, fetched along 16 x 16 block vectors found between the byte lumas of the two source frames and weighted by how well
the source matched there; every output conversion then reads the lane's stabilised tensor.  ``strength`` in [0, 1] is quantised as compose's,
``sensitivity`` K in [1, 256] takes the weight to zero at a luma difference of 256 / K, ``radius`` in [0, 7] bounds the search, ``matrix``
names the luma weights and ``source_bgr`` says that channel 0 of the net's input is blue.  One frame per pass (batch 1).  The lane keeps two
state slots (luma, the output on the 8.8 scale, the vectors): frame n reads slot (n - 1) & 1 and writes slot n & 1.  The slot parity changes
pointers and "no previous frame" is a launch argument, so such a lane's pass is captured in pieces: the head (input conversions, forward,
compose) as before, and the tail (the stage and the output conversions) once per parity and once for a first frame, each when it first
occurs.  ``reset()`` forgets the previous frame.  Without ``temporal=`` nothing is allocated or launched and the one graph is captured whole.
``levels`` in [1, 3] (default 1) searches coarse to fine over that many halved lumas (fs_temporal_pyr_f32): vectors up to ``radius`` (2^levels
- 1) pixels, found reliably up to about ``radius`` 2^(levels - 1); each slot then has a fourth buffer, the halved lumas and the coarse vectors,
and the tail has one launch more for the pyramid and one search launch per level.  With ``levels=1`` or without the key nothing changes.
``subpel`` in [0, 2] (default 0) gives the block vectors in whole, half or quarter pixels (fs_temporal_sub_f32): a fraction per block fitted
through the winner's SAD and its four neighbours, and a bilinear fetch of the previous luma and output, so that a slow pan keeps its
confidence; each slot then has a last buffer more, the fractions, and the tail one launch more.  ``motion_vectors_subpel()`` returns 4 mv + mvf.
With ``subpel=0`` or without the key nothing changes.
``overlap`` in [0, 1] (default 0): with 1 every pixel is blended along the vectors of the four blocks whose centres surround it, weighted by
a bilinear window and by how well the source matched along each (fs_temporal_obmc_f32), so that a block that straddles a motion edge keeps
its weight on both sides; the slots and the number of launches are those of ``levels`` and ``subpel``.  With ``overlap=0`` or without the key
nothing changes.
``sequence=True`` on a lane with ``batch=N`` says that the batch's images are N consecutive frames of one stream, oldest first
(fs_temporal_batch_f32): luma, pyramid, searches and refinement run once over the N frames and N blends follow in order, frame i reading
what frame i - 1 left, frame 0 what the previous pass left.  Slot parity, the three tail graphs, ``reset()`` and the frame counter then go by
pass; the lane has one work buffer more for the frames inside a pass, ``stabilised_output()`` is [N, Ho, Wo, 3] and ``motion_vectors()`` /
``motion_vectors_subpel()`` have a leading axis of N.  A pass always takes N frames: the caller pads a stream's end by repeating its last
frame.  Without this key or ``streams`` a batch other than 1 is refused (the stage must be told which of the two a batch is); with it at
batch 1 nothing changes.
``streams=True`` on a lane with ``batch=S`` is that other reading: the batch's images are one frame of each of S independent streams
(fs_temporal_streams_f32), every one stabilised against its own previous frame.  Nothing is recursive inside such a pass, so every launch of
the stage, the blend included, runs once over all streams: the stage has the launches of one stream whatever S is.  The lane holds one state
buffer (per stream two slots), and what differs per stream -- whether it has a previous frame, which slot it writes, whether it takes part --
is a device control word, written from a pinned host array by an asynchronous copy on the lane's stream ahead of the tail and advanced on the
host only behind the pass; so there is one tail graph whatever the passes were.  ``set_streams(active)`` names the streams of the passes that
follow (S booleans; an inactive stream keeps its state and parity, and its row of the results is whatever the lane held), ``reset(stream=)``
forgets one stream's previous frame (None: every stream's).  ``stabilised_output()`` is [S, Ho, Wo, 3], ``motion_vectors()`` /
``motion_vectors_subpel()`` have a leading axis of S.  Mutually exclusive with ``sequence=True``; at batch 1 the frames are, byte for byte, those
of the lane without the key.

Delivery at another size: with ``deliver=dict(height=, width=, filter='bicubic')`` one launch ahead of the output conversions (fs_resample_f32,
csrc/fs_resample.hip) resamples the top-left H x W of the tensor they would read -- the net's output, the composed or the stabilised tensor --
into a delivery tensor of the lane's own, in Pillow's mode-F arithmetic (``filter`` 'box', 'bilinear', 'bicubic' or 'lanczos'), and every
output conversion reads that tensor: the u8 frame, the JPEG file and the YCbCr planes have the delivery size (``delivery_shape``), while
``out_shape``, compose, temporal and their state stay on the net's grid.  The stage is part of the output conversions, so it lies in the
whole-pass graph and in every temporal tail graph.  ``source=dict(..., resample='bicubic')`` is its counterpart on the input side for sources
of 9 to 16 bits per sample: the planes are converted at the source's own size into an fp32 tensor of the lane's and resampled into the net's
input; it is the only way such a source of another size than the net's is taken, and 8-bit sources are refused with it (``interpolation=``
serves them).  Without the keys nothing is allocated or launched.

Guided delivery: ``deliver=dict(height=, width=, guided=dict(radius=2, smoothness=4, matrix='bt601', source_bgr=<the lane's swap_rb>))`` puts
fs_guided_f32 (csrc/fs_guided.hip, three launches) where the resampling stands: the fast guided filter fits output ~ a * luma(source) + b per
channel on the net's grid, smooths a and b over a (2 radius + 1)^2 window, interpolates them to the delivery grid and applies them to the luma
of the source at its own size, so that the source's edges return at the delivery resolution.  ``smoothness`` in [1, 64] is in 8-bit levels
(larger: smoother, nearer to a plain bilinear enlargement), ``source_bgr`` says that channel 0 of the net's input is blue.  It needs a
``source=`` of exactly the delivery's size that is resized to the net's, and reads the buffer the lane holds that source in anyway: the pixel
frames, the decoded RGBX of JPEG and 8-bit ``yuv=`` sources, or the fp32 planes of a deep source with ``resample=``.  Not together with
``filter=``.

Two styles per stream: with ``mix=dict(variables=, weight=1.0, mask=None)`` the lane holds a second parameter set with a workspace of its
own, runs a second forward pass behind the first and merges the two fp32 outputs with one launch (fs_mix_f32, csrc/fs_mix.hip) into a mixed
tensor of the lane's own, which compose, the temporal stage, delivery and every output conversion take where they took the net's output.
``weight`` in [0, 1] (quantised as compose's strength) is the share of the second model, ``mask`` a host uint8 [H, W] at the net's input
size, 0 shows the first model and 255 the mix.  The weight lives in a device buffer of one int32 per image, so that ``set_mix(weight)`` --
a number, or ``batch`` numbers for a pass of consecutive frames -- changes it between passes without a new graph: the values go up with an
asynchronous copy on the lane's stream ahead of the replay.  A model nobody will see is not run: model B is live if any weight of the pass
is above 0, model A if there is a mask or any weight is below 1; the launch then reads the live model's output twice.  The head graph is
captured per liveness kind ('a', 'b', 'ab') when the kind first occurs; ``last_forwards()`` names the last pass's.  Both forwards stay on the
lane's one stream.  Without ``mix=`` nothing is allocated or launched and the lane captures the graph it always captured.
"""
import ctypes

import numpy as np

from . import _lib as L


class FrameNotTaken(L.FaststyleError):
    """A frame given as JPEG bytes that the native decoder does not take (another geometry than the stylizer's source, a file outside the
    handled set, a scan that does not decode): nothing was enqueued; decode it otherwise and pass the pixels."""


def jpeg_source(eng, data, **kw):
    """The ``source=`` dict of a stylizer fed with JPEG files like ``data`` (the bytes of a first file): its size and JPEG geometry, plus
    whatever ``kw`` adds (interpolation=, swap_rb=).  None for a file fs_jpeg_parse does not take."""
    rc, info = eng.jpeg_parse(data)
    if rc != 0:
        return None
    return dict(kw, height=int(info.height), width=int(info.width),
                jpeg=dict(width=int(info.width), height=int(info.height), components=int(info.ncomp), sampling=(int(info.hs[0]), int(info.vs[0]))))


class FrameStylizer(object):
    KEEP_GRAPH = False     # tests: keep the captured hipGraph_t so that its node types can be inspected

    def __init__(self, eng, variables, height, width, upsample_method="resize", batch=1, swap_rb=True, use_graph=True,
                 bf16=False, jpeg=None, jpeg_threads=4, source=None, yuv_out=None, compose=None, temporal=None, deliver=None,
                 mix=None, _temporal_slots=None):
        self.eng = eng
        self.variables = variables
        self.method = upsample_method
        self.bf16 = bf16                 # FS_FLAG_BF16 mixed-precision path (~2x the frame rate, ~52 dB vs fp32)
        self.shape = (int(batch), int(height), int(width), 3)
        self.swap_rb = swap_rb
        mem = eng.mem
        Ho, Wo = eng.tnet_out_shape(height, width)
        self.out_shape = (int(batch), Ho, Wo, 3)
        self.delivery_shape = self.out_shape   # the frames the output conversions write; with deliver=: (batch, height, width, 3) of the delivery
        self.deliver = None              # with deliver=: dict(height=, width=, filter=)
        self._deliver_plan = None        # ... the plan from the top-left H x W of the net's Ho x Wo output to the delivery size
        self._delivered = None           # ... and the delivery tensor every output conversion then reads
        self._guided = None              # with deliver guided=: dict(radius=, smoothness=, matrix=, lo_bgr=) as the launch takes them
        self._guided_work = None         # ... the workspace of the three launches (Engine.guided_workspace)
        self._guided_src = None          # ... {jpeg_in: (the device buffer that holds the source at its own size, hi_bgr)}
        self._hi_jpeg = False            # ... whether the pass under way began with JPEG coefficients
        if deliver is not None:
            self._deliver_setup(dict(deliver))
        self._in_u8 = mem.upload_u8(np.zeros(self.shape, np.uint8))
        self._in_f32 = mem.empty(self.shape)
        self._out_u8 = mem.upload_u8(np.zeros(self.delivery_shape, np.uint8))
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
        self.yuv_out = None
        self._out_deep = False           # yuv_out= with bits above 8: the conversion reads the net's fp32 output itself
        self.yuv_out_desc = None         # with yuv_out=: the fs_yuv_desc of an output frame (what a y4m.Writer takes)
        self._result = self._out_u8      # the device buffer __call__ downloads (without jpeg=)
        if yuv_out is not None:
            if jpeg is not None:
                raise L.FaststyleError("jpeg= and yuv_out= are mutually exclusive: a stylizer returns one kind of frame")
            self._yuv_out_setup(dict(yuv_out))
        self.source = None
        self.in_shape = self.shape       # the pixel frames __call__ takes, and the device buffer they are uploaded into
        self._pix_dst = self._in_u8
        self._src_plan = None
        self._src_jpeg = None
        self._graph_jpeg = None
        self._src_host = None
        self._src_yuv = None
        self._src_deep = False           # source yuv= with bits above 8: the conversion writes the net's fp32 input itself
        self._src_rplan = None           # source resample= at another size than the net's: the plan from the source size to the net's
        self._src_f32 = None             # ... and the deep source converted at its own size
        if source is not None:
            self._source_setup(dict(source))
        if self._guided is not None:
            self._guided_bind()
        self.compose = None              # with compose=: dict(strength_q8=, keep_color=, matrix=, mask=, source_swapped=) as the launch takes them
        self._composed = None            # ... and the composed tensor every output conversion then reads instead of the net's output
        self._mask = None
        if compose is not None:
            self._compose_setup(dict(compose))
        self.mix = None                  # with mix=: dict(mask=) -- the weights are state (set_mix), not options
        self._mixed = None               # ... the mixed tensor compose and every later stage then read instead of the net's output
        if mix is not None:
            self._mix_setup(dict(mix))
        self.temporal = None             # with temporal=: dict(strength_q8=, sensitivity=, radius=, matrix=, source_bgr=) as the launch takes them
        self._stab = None                # ... the stabilised tensor every output conversion then reads
        self._tslots = None              # ... the two state slots (Engine.temporal_state), shared by the lanes of a PipelinedStylizer
        self._tn = 0                     # ... frames since construction or reset(): frame n reads slot (n - 1) & 1 and writes slot n & 1
        self._twork = None               # ... with sequence=True and a batch: the work buffer of the frames inside a pass (then _tn counts passes)
        self._cur = None                 # ... the head's result: the net's output or the composed tensor
        self._tail_graphs = {}           # ... captured tails by the parity written (None: a first frame's); a streams lane has one
        self._sctl = None                # ... with streams=True: the device control words (one per stream) and their pinned staging words,
        self._sctl_stage = None          #     the lane's own; _tslots is then the one state buffer of all streams, shared by the lanes
        self._sh = None                  #     and the host's view of the streams (prev, parity, active, last), shared by the lanes too
        if temporal is not None:
            self._temporal_setup(dict(temporal), _temporal_slots)

    DELIVER_KEYS = ("height", "width", "filter")
    GUIDED_KEYS = ("radius", "smoothness", "matrix", "source_bgr")

    def _deliver_setup(self, opt):
        """The delivery stage's fixed parts: the checked size and filter, the plan and the lane's own delivery tensor."""
        guided = opt.pop("guided", None)
        kw = {k: opt.pop(k) for k in self.DELIVER_KEYS if k in opt}
        if opt:
            raise L.FaststyleError("deliver takes %s, got also %r" % (", ".join(self.DELIVER_KEYS), opt))
        if guided is not None and "filter" in kw:
            raise L.FaststyleError("deliver guided= takes the place of filter=: the delivery is resampled or guided, got both")
        if "height" not in kw or "width" not in kw:
            raise L.FaststyleError("deliver needs height and width, got %r" % kw)
        size = []
        for name in ("height", "width"):
            v = kw[name]
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise L.FaststyleError("deliver %s must be a whole number of at least 1, got %r" % (name, v))
            size.append(int(v))
        B, H, W, _ = self.shape
        if guided is not None:
            self._guided_setup(dict(guided), size)
            return
        filt = kw.get("filter", "bicubic")
        self._deliver_plan = self.eng.resample_plan(H, W, size[0], size[1], filt)      # (an unknown filter or a refused plan raises)
        self.deliver = dict(height=size[0], width=size[1], filter=filt)
        self.delivery_shape = (B, size[0], size[1], 3)
        self._delivered = self.eng.mem.empty(self.delivery_shape)

    def _guided_setup(self, opt, size):
        """The guided delivery's checked parameters and the lane's delivery tensor; the source is bound once it is known (_guided_bind)."""
        kw = {k: opt.pop(k) for k in self.GUIDED_KEYS if k in opt}
        if opt:
            raise L.FaststyleError("deliver guided takes %s, got also %r" % (", ".join(self.GUIDED_KEYS), opt))

        def whole(name, default, lo, hi):
            try:
                v = float(kw.get(name, default))
            except (TypeError, ValueError):
                raise L.FaststyleError("deliver guided %s %r is not a number" % (name, kw[name]))
            if not lo <= v <= hi or v != int(v):                 # (NaN fails both comparisons)
                raise L.FaststyleError("deliver guided %s must be a whole number in [%d, %d], got %r" % (name, lo, hi, v))
            return int(v)

        matrix = {"bt601": 0, "bt709": 1, 0: 0, 1: 1}.get(kw.get("matrix", "bt601"))
        if matrix is None:
            raise L.FaststyleError("deliver guided matrix is 'bt601' or 'bt709', got %r" % (kw["matrix"],))
        B, H, W, _ = self.shape
        if size[0] < H or size[1] < W or tuple(size) == (H, W) or max(size) > 32767:
            raise L.FaststyleError("deliver guided= upsamples to the source's size: a delivery of %dx%d from a net of %dx%d (at least the net's "
                                   "size on both sides, larger on one, at most 32767)" % (size[0], size[1], H, W))
        self._guided = dict(radius=whole("radius", 2, 1, 8), smoothness=whole("smoothness", 4, 1, 64), matrix=matrix,
                            lo_bgr=bool(kw.get("source_bgr", self.swap_rb)))
        self.deliver = dict(height=size[0], width=size[1], guided=dict(self._guided))
        self.delivery_shape = (B, size[0], size[1], 3)
        self._delivered = self.eng.mem.empty(self.delivery_shape)

    def _guided_bind(self):
        """The guide of the guided delivery: the buffer in which the lane already holds the source at its own size, which must be the
        delivery's.  hi_bgr follows from where R and B are exchanged: in the resize behind that buffer (cvresize_u8(swap_rb=): the buffer has
        the other order than the net's input) or in the conversion in front of it (yuv_deep_to_f32(swap_rb=): the same order)."""
        B, H, W, _ = self.shape
        size = self.delivery_shape[1:3]
        if self.source is None:
            raise L.FaststyleError("deliver guided= needs source= at the delivery's size %dx%d, resized to the net's: the full-size source is the guide" % size)
        if (self.source["height"], self.source["width"]) != size:
            raise L.FaststyleError("deliver guided= needs a source of the delivery's size %dx%d, got %dx%d" %
                                   (size + (self.source["height"], self.source["width"])))
        lo_bgr = self._guided["lo_bgr"]
        behind = lo_bgr != self._src_swap                        # (the swap happens behind the buffer)
        if self._src_f32 is not None:
            self._guided_src = {False: (self._src_f32, lo_bgr)}
        elif self._src_yuv is not None and not self._src_deep and self._src_rgbx is not None:
            self._guided_src = {False: (self._src_rgbx, behind)}
        elif self._src_yuv is None and self._src_plan is not None:
            self._guided_src = {False: (self._pix_dst, behind)}
            if self._src_jpeg is not None:
                self._guided_src[True] = (self._src_rgbx, behind)
        else:
            raise L.FaststyleError("deliver guided= needs a source that is resized to the net's size (interpolation=, or resample= for 9 to 16 bits)")
        self._guided_work = self.eng.guided_workspace(H, W, B)

    TEMPORAL_KEYS = ("strength", "sensitivity", "radius", "matrix", "source_bgr", "levels", "subpel", "overlap", "sequence", "streams")

    def _temporal_setup(self, opt, slots):
        """The temporal stage's fixed parts: the quantised strength, the checked parameters, the state slots and the stabilised tensor."""
        kw = {k: opt.pop(k) for k in self.TEMPORAL_KEYS if k in opt}
        if opt:
            raise L.FaststyleError("temporal takes %s, got also %r" % (", ".join(self.TEMPORAL_KEYS), opt))
        sequence = kw.get("sequence", False)
        if not isinstance(sequence, (bool, np.bool_)):
            raise L.FaststyleError("temporal sequence is True or False, got %r" % (sequence,))
        streams = kw.get("streams", False)
        if not isinstance(streams, (bool, np.bool_)):
            raise L.FaststyleError("temporal streams is True or False, got %r" % (streams,))
        if streams and sequence:
            raise L.FaststyleError("temporal streams and sequence are mutually exclusive: a batch is independent streams or consecutive frames of one")
        if streams and self.shape[0] > 64:
            raise L.FaststyleError("temporal streams takes at most 64 streams per pass, this stylizer has a batch of %d" % self.shape[0])
        if self.shape[0] != 1 and not sequence and not streams:
            raise L.FaststyleError("temporal takes one frame per pass, this stylizer has a batch of %d" % self.shape[0])

        def number(name, default, lo, hi, whole):
            try:
                v = float(kw.get(name, default))
            except (TypeError, ValueError):
                raise L.FaststyleError("temporal %s %r is not a number" % (name, kw[name]))
            if not lo <= v <= hi or (whole and v != int(v)):     # (NaN fails both comparisons)
                raise L.FaststyleError("temporal %s must be %s in [%d, %d], got %r" % (name, "a whole number" if whole else "a number", lo, hi, v))
            return v

        s = number("strength", 1.0, 0, 1, False)
        matrix = {"bt601": 0, "bt709": 1, 0: 0, 1: 1}.get(kw.get("matrix", "bt601"))
        if matrix is None:
            raise L.FaststyleError("temporal matrix is 'bt601' or 'bt709', got %r" % (kw["matrix"],))
        self.temporal = dict(strength_q8=int(np.floor(s * 256.0 + 0.5)), sensitivity=int(number("sensitivity", 16, 1, 256, True)),
                             radius=int(number("radius", 7, 0, 7, True)), matrix=matrix, source_bgr=bool(kw.get("source_bgr", self.swap_rb)))
        levels = int(number("levels", 1, 1, 3, True))
        if levels > 1:                                       # (a lane of one level keeps the dict, the slots and the launches it always had)
            self.temporal["levels"] = levels
        subpel = int(number("subpel", 0, 0, 2, True))
        if subpel > 0:                                       # (likewise: without the key, or with 0, nothing changes)
            self.temporal["subpel"] = subpel
        overlap = int(number("overlap", 0, 0, 1, True))
        if overlap > 0:                                      # (likewise; the slots are those of (levels, subpel))
            self.temporal["overlap"] = overlap
        Ho, Wo = self.out_shape[1:3]
        if streams:                                          # one state buffer and one control word per stream instead of two slots and a parity
            S = self.shape[0]
            self.temporal["streams"] = True
            self._tslots = self.eng.temporal_streams_state(Ho, Wo, S, levels, subpel) if slots is None else slots
            self._sctl = self.eng.i32_buffer([0] * S)
            self._sctl_stage = self.eng.i32_staging(S)
            self._sh = dict(prev=[False] * S, parity=[0] * S, active=[True] * S, last=None)
            self._stab = self.eng.mem.empty(self.out_shape)
            return
        if slots is None:
            slots = [self.eng.temporal_state(Ho, Wo, levels, subpel) if subpel > 0 else self.eng.temporal_state(Ho, Wo, levels) for _ in range(2)]
        self._tslots = slots
        self._stab = self.eng.mem.empty(self.out_shape)
        if self.shape[0] != 1:                               # (sequence=True at batch 1 is the lane without the key)
            self.temporal["sequence"] = True
            self._twork = self.eng.temporal_batch_work(Ho, Wo, self.shape[0], levels, subpel)

    COMPOSE_KEYS = ("strength", "keep_color", "matrix", "mask", "source_swapped")

    def _compose_setup(self, opt):
        """The compose stage's fixed parts: the quantised strength, the mask on the device (once) and the lane's own composed tensor."""
        kw = {k: opt.pop(k) for k in self.COMPOSE_KEYS if k in opt}
        if opt:
            raise L.FaststyleError("compose takes %s, got also %r" % (", ".join(self.COMPOSE_KEYS), opt))
        try:
            s = float(kw.get("strength", 1.0))
        except (TypeError, ValueError):
            raise L.FaststyleError("compose strength %r is not a number" % (kw["strength"],))
        if not 0.0 <= s <= 1.0:                                  # (NaN fails both comparisons)
            raise L.FaststyleError("compose strength must be in [0, 1], got %r" % s)
        matrix = {"bt601": 0, "bt709": 1, 0: 0, 1: 1}.get(kw.get("matrix", "bt601"))
        if matrix is None:
            raise L.FaststyleError("compose matrix is 'bt601' or 'bt709', got %r" % (kw["matrix"],))
        mask = kw.get("mask")
        if mask is not None:
            mask = np.asarray(mask)
            if mask.dtype != np.uint8 or mask.shape != self.shape[1:3]:
                raise L.FaststyleError("compose mask shape %s dtype %s, the net's input takes uint8 %s" % (mask.shape, mask.dtype, self.shape[1:3]))
            self._mask = self.eng.mem.upload_u8(mask)
        self.compose = dict(strength_q8=int(np.floor(s * 256.0 + 0.5)), keep_color=bool(kw.get("keep_color", False)), matrix=matrix,
                            mask=mask is not None, source_swapped=bool(kw.get("source_swapped", False)))
        self._composed = self.eng.mem.empty(self.out_shape)

    MIX_KEYS = ("variables", "weight", "mask")

    def _mix_q8_of(self, weight):
        """set_mix's argument -> the batch's weights by 256: a number serves every image, a sequence names ``batch`` consecutive frames'.
        Quantised as compose's strength, floor(t * 256 + 0.5)."""
        B = self.shape[0]
        try:
            t = np.asarray(weight, dtype=np.float64)
        except (TypeError, ValueError):
            raise L.FaststyleError("mix weight %r is not a number" % (weight,))
        if t.ndim > 1 or (t.ndim == 1 and t.shape[0] != B):
            raise L.FaststyleError("mix weight is a number or a sequence of %d numbers (the batch), got %r" % (B, weight))
        if not np.all((t >= 0.0) & (t <= 1.0)):                  # (NaN fails both comparisons)
            raise L.FaststyleError("mix weight must be in [0, 1], got %r" % (weight,))
        return tuple(int(v) for v in np.broadcast_to(np.floor(t * 256.0 + 0.5).astype(np.int64), (B,)))

    def _mix_setup(self, opt):
        """The mix stage's fixed parts: the second parameter set's own workspace, the two nets' output tensors (one per model whichever
        graph writes them), the mask on the device (once), the mixed tensor, the weight buffer and its host staging."""
        kw = {k: opt.pop(k) for k in self.MIX_KEYS if k in opt}
        if opt:
            raise L.FaststyleError("mix takes %s, got also %r" % (", ".join(self.MIX_KEYS), opt))
        if kw.get("variables") is None:
            raise L.FaststyleError("mix needs variables, the second model's parameters")
        e, mem = self.eng, self.eng.mem
        q8 = self._mix_q8_of(kw.get("weight", 1.0))
        mask = kw.get("mask")
        self._mix_mask = None
        if mask is not None:
            mask = np.asarray(mask)
            if mask.dtype != np.uint8 or mask.shape != self.shape[1:3]:
                raise L.FaststyleError("mix mask shape %s dtype %s, the net's input takes uint8 %s" % (mask.shape, mask.dtype, self.shape[1:3]))
            self._mix_mask = mem.upload_u8(mask)
        self.variables2 = kw["variables"]
        self._ws2 = e.new_tnet_workspace(self.shape[0], self.shape[1], self.shape[2], self.bf16)
        self._mix_ya = mem.empty(self.out_shape)
        self._mix_yb = mem.empty(self.out_shape)
        self._mixed = mem.empty(self.out_shape)
        self._mix_q8 = q8                                        # the weights of the passes that follow (set_mix)
        self._mix_w = e.i32_buffer(q8)                           # ... on the device, where the launch reads them
        self._mix_w_q8 = q8                                      # ... as the device buffer holds them (or will, behind the copies enqueued)
        self._mix_stage = e.i32_staging(self.shape[0])
        self._mix_kind = None                                    # the liveness kind of the pass under way: 'a', 'b' or 'ab'
        self._mix_graphs = {}                                    # captured heads by (kind, JPEG frames)
        self.mix = dict(mask=mask is not None)

    def set_mix(self, weight):
        """The share of the second model in the passes that follow: a number in [0, 1], or ``batch`` numbers for a pass of consecutive
        frames (mix= only).  Nothing is enqueued here; the next pass uploads the values ahead of its launches."""
        if self.mix is None:
            raise L.FaststyleError("set_mix: this stylizer was built without mix=")
        self._mix_q8 = self._mix_q8_of(weight)

    def _mix_prepare(self):
        """Ahead of a pass (and of the capture of its graph): the weights into the device buffer where they changed -- an asynchronous
        copy on the current stream, the lane's, from the lane's staging words, which the previous pass's download has long left behind --
        and the liveness kind: B runs if any weight is above 0, A if there is a mask or any weight is below 256."""
        q8 = self._mix_q8
        if q8 != self._mix_w_q8:
            self.eng.i32_upload(self._mix_w, q8, self._mix_stage)
            self._mix_w_q8 = q8
        a = self.mix["mask"] or min(q8) < 256
        b = max(q8) > 0
        self._mix_kind = "ab" if a and b else ("b" if b else "a")

    def last_forwards(self):
        """The models the last pass ran: ('a',), ('b',) or ('a', 'b') (mix= only)."""
        if self.mix is None:
            raise L.FaststyleError("last_forwards: this stylizer was built without mix=")
        if self._y is None:
            raise L.FaststyleError("last_forwards: this stylizer has not run a frame yet")
        return tuple(self._mix_kind)

    YUV_KEYS = ("sampling", "siting", "matrix", "full_range", "components", "bits")

    def _yuv_desc(self, opt, width, height, what):
        """The fs_yuv_desc of a yuv= / yuv_out= dict at a frame size; unknown keys raise."""
        opt = dict(opt)
        kw = {k: opt.pop(k) for k in self.YUV_KEYS if k in opt}
        if opt:
            raise L.FaststyleError("%s takes %s, got also %r" % (what, ", ".join(self.YUV_KEYS), opt))
        return self.eng.yuv_plan(width, height, **kw), kw

    def _yuv_out_setup(self, opt):
        """The output side's colour conversion: the descriptor of one output frame and the device buffer of the batch's planes."""
        B, Ho, Wo, _ = self.delivery_shape
        self.yuv_out_desc, kw = self._yuv_desc(opt, Wo, Ho, "yuv_out")
        self.yuv_out = kw
        self._out_deep = int(self.yuv_out_desc.reserved[0]) != 0
        self._result = self.eng.mem.upload_u8(np.zeros((B, int(self.yuv_out_desc.frame_bytes)), np.uint8))

    def _source_setup(self, opt):
        """The input side's fixed parts: the resize plan from the source size (none when nothing is to be resized or swapped), the device buffer
        of source pixels, and for JPEG frames the descriptor table, the device coefficient buffer and the decoded RGBX pixels."""
        e, mem = self.eng, self.eng.mem
        B, H, W, _ = self.shape
        try:
            Hs, Ws = int(opt.pop("height")), int(opt.pop("width"))
        except KeyError:
            raise L.FaststyleError("source needs height and width, got %r" % opt)
        interpolation, swap, jp = opt.pop("interpolation", None), bool(opt.pop("swap_rb", False)), opt.pop("jpeg", None)
        yuv = opt.pop("yuv", None)
        has_resample = "resample" in opt
        resample = opt.pop("resample", None)
        if opt:
            raise L.FaststyleError("source takes height, width, interpolation, swap_rb, jpeg, yuv and resample, got also %r" % opt)
        if has_resample and resample not in L.FS_RESAMPLE_FILTERS:
            raise L.FaststyleError("source resample is one of %s, got %r" % (", ".join(sorted(L.FS_RESAMPLE_FILTERS)), resample))
        self.source = dict(height=Hs, width=Ws, interpolation=interpolation, swap_rb=swap, jpeg=None if jp is None else dict(jp))
        self._src_swap = swap
        if yuv is not None:
            if jp is not None:
                raise L.FaststyleError("source jpeg= and yuv= are mutually exclusive: the frames of a stylizer have one form")
            self._src_yuv, self.source["yuv"] = self._yuv_desc(yuv, Ws, Hs, "source yuv")
            self._src_deep = int(self._src_yuv.reserved[0]) != 0
            if has_resample and not self._src_deep:
                raise L.FaststyleError("source resample= takes sources of 9 to 16 bits per sample only: an 8-bit source is resized by "
                                       "interpolation= (cv2.resize on the u8 frames)")
            if self._src_deep and has_resample:
                self.source["resample"] = resample
                self.in_shape = (B, int(self._src_yuv.frame_bytes))
                self._pix_dst = mem.upload_u8(np.zeros(self.in_shape, np.uint8))
                if (Hs, Ws) != (H, W):                       # converted at its own size, then resampled into the net's fp32 input
                    self._src_rplan = e.resample_plan(Hs, Ws, H, W, resample)
                    self._src_f32 = mem.empty((B, Hs, Ws, 3))
                return
            if self._src_deep and (Hs, Ws) != (H, W):
                raise L.FaststyleError("a source of %d bits per sample has the net's size %dx%d, got %dx%d: the resize takes 8-bit frames only" %
                                       (self._src_yuv.reserved[0], H, W, Hs, Ws))
            self.in_shape = (B, int(self._src_yuv.frame_bytes))
            self._pix_dst = mem.upload_u8(np.zeros(self.in_shape, np.uint8))             # the planes as uploaded
            if (Hs, Ws) != (H, W):                                                      # (a swap alone is the conversion's own)
                self._src_plan = e.cvresize_plan(Hs, Ws, W / float(Ws), H / float(Hs), interpolation)
                if self._src_plan.dst_shape != (H, W):
                    raise L.FaststyleError("source %dx%d does not resize to %dx%d but to %dx%d" % ((Hs, Ws, H, W) + self._src_plan.dst_shape))
                self._src_rgbx = mem.upload_u8(np.zeros((B, Hs, Ws, 4), np.uint8))
            return
        if has_resample:
            raise L.FaststyleError("source resample= takes sources of 9 to 16 bits per sample only (yuv= with bits=): 8-bit frames are resized by "
                                   "interpolation= (cv2.resize on the u8 frames)")
        self.in_shape = (B, Hs, Ws, 3)
        if (Hs, Ws) != (H, W) or swap:
            self._src_plan = e.cvresize_plan(Hs, Ws, W / float(Ws), H / float(Hs), interpolation)
            if self._src_plan.dst_shape != (H, W):
                raise L.FaststyleError("source %dx%d does not resize to %dx%d but to %dx%d" % ((Hs, Ws, H, W) + self._src_plan.dst_shape))
            self._pix_dst = mem.upload_u8(np.zeros(self.in_shape, np.uint8))
        if jp is None:
            return
        jp = dict(jp)
        try:
            geom = (int(jp.pop("width")), int(jp.pop("height")), int(jp.pop("components")), tuple(int(v) for v in jp.pop("sampling")))
        except (KeyError, TypeError):
            raise L.FaststyleError("source jpeg needs width, height, components and sampling=(hs, vs), got %r" % self.source["jpeg"])
        if jp or geom[:2] != (Ws, Hs):
            raise L.FaststyleError("source jpeg %r does not describe the %dx%d source" % (self.source["jpeg"], Ws, Hs))
        rc, info = e.jpeg_encode_plan(geom[0], geom[1], geom[2], *geom[3])      # (the fs_jpeg_info of this geometry: the buffer sizes)
        L.check(e.lib, rc, "fs_jpeg_encode_plan")
        self._src_jpeg = geom
        self._sstride = (int(info.coef_bytes) + 15) & ~15
        pb = 4 if self._src_plan is not None else 3              # RGBX for the resize to read; nothing to resize: straight into the net's input
        self._sitems = np.zeros(B, dtype=e.JPEG_ITEM)
        for b in range(B):
            self._sitems[b] = e.jpeg_item(info, b * self._sstride, b * Hs * Ws * pb, pb)
        self._sitems_dev = mem.upload_u8(self._sitems.view(np.uint8).reshape(-1))
        self._src_coef = mem.upload_u8(np.zeros(B * self._sstride, np.uint8))
        self._src_rgbx = mem.upload_u8(np.zeros((B, Hs, Ws, 4), np.uint8)) if pb == 4 else None
        self._src_host = self.new_coef_staging()

    def new_coef_staging(self):
        """A host buffer for the decoded coefficients of one batch of JPEG frames (pinned on the GPU engine): (numpy view, the buffer)."""
        mem = self.eng.mem
        n = self.shape[0] * self._sstride
        if hasattr(mem, "torch"):
            t = mem.torch.zeros(n, dtype=mem.torch.uint8, pin_memory=True)
            return t.numpy(), t
        a = np.zeros(n, np.uint8)
        return a, a

    def decode_frames(self, files, staging):
        """The host half of JPEG frames: fs_jpeg_parse + fs_jpeg_decode of each file into its slot of ``staging`` (new_coef_staging's).  Raises
        FrameNotTaken for a file of another geometry, one the parser does not take, or one that does not decode.  Touches no device state and
        holds no interpreter lock inside fs_jpeg_decode: decode threads call it ahead of the device."""
        e = self.eng
        if self._src_jpeg is None:
            raise FrameNotTaken("this stylizer was built without source jpeg=: it takes pixel frames only")
        if len(files) != self.shape[0]:
            raise L.FaststyleError("%d JPEG frames, stylizer was built for a batch of %d" % (len(files), self.shape[0]))
        view = staging[0]
        for b, data in enumerate(files):
            rc, info = e.jpeg_parse(data)
            if rc != 0:
                raise FrameNotTaken("fs_jpeg_parse answers %d for this frame" % rc)
            geom = (int(info.width), int(info.height), int(info.ncomp), (int(info.hs[0]), int(info.vs[0])))
            if geom != self._src_jpeg:
                raise FrameNotTaken("frame geometry %r, stylizer was built for %r" % (geom, self._src_jpeg))
            rc = e.jpeg_decode(data, info, view.ctypes.data + b * self._sstride, self._sstride)
            if rc != 0:
                raise FrameNotTaken("fs_jpeg_decode answers %d for this frame" % rc)
        return staging

    # luma sampling factors of PIL's ``subsampling`` values
    SUBSAMPLING = {0: (1, 1), 1: (2, 1), 2: (2, 2), "4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}

    def _jpeg_setup(self, opt, threads):
        """The encoder's fixed parts: the plan of one output frame, the descriptor table (on the device once: the graph replays its address),
        the device coefficient buffer of the batch and one output buffer per image that surely holds its file."""
        quality, sub = int(opt.pop("quality", 95)), opt.pop("subsampling", 2)
        if opt or sub not in self.SUBSAMPLING or not 1 <= quality <= 100:
            raise L.FaststyleError("jpeg takes quality (1..100) and subsampling (0, 1, 2), got %r" % dict(opt, quality=quality, subsampling=sub))
        e, mem = self.eng, self.eng.mem
        B, Ho, Wo, _ = self.delivery_shape
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
        B = self.delivery_shape[0]
        if B == 1 or pool is None:
            return [self._write_one(coef_addr, b) for b in range(B)]
        return list(pool.map(lambda b: self._write_one(coef_addr, b), range(B)))

    def _device_pass(self, jpeg_in=False):
        e = self.eng
        self._hi_jpeg = jpeg_in
        if jpeg_in:                                          # the coefficients of the frame(s) are in self._src_coef
            if self._src_plan is not None:
                e.jpeg_reconstruct_many(self._src_coef, self._sitems, self._src_rgbx, items_dev=(self._sitems_dev, 0))
                e.cvresize_u8(self._src_rgbx, self._src_plan, self._in_u8, swap_rb=self._src_swap)
            else:
                e.jpeg_reconstruct_many(self._src_coef, self._sitems, self._in_u8, items_dev=(self._sitems_dev, 0))
        elif self._src_yuv is not None:                      # the planes of the frame(s) are in self._pix_dst
            if self._src_rplan is not None:                  # 16-bit samples of another size: fp32 at the source's size, resampled to the net's
                e.yuv_deep_to_f32(self._pix_dst, self._src_yuv, self._src_f32, swap_rb=self._src_swap)
                e.resample_f32(self._src_f32, self._src_rplan, self._in_f32)
            elif self._src_deep:                             # 16-bit samples: straight to the net's fp32 input
                e.yuv_deep_to_f32(self._pix_dst, self._src_yuv, self._in_f32, swap_rb=self._src_swap)
            elif self._src_plan is not None:
                e.yuv_to_rgb_u8(self._pix_dst, self._src_yuv, self._src_rgbx)
                e.cvresize_u8(self._src_rgbx, self._src_plan, self._in_u8, swap_rb=self._src_swap)
            else:
                e.yuv_to_rgb_u8(self._pix_dst, self._src_yuv, self._in_u8, swap_rb=self._src_swap)
        elif self._src_plan is not None:                     # source pixels are in self._pix_dst
            e.cvresize_u8(self._pix_dst, self._src_plan, self._in_u8, swap_rb=self._src_swap)
        if not self._src_deep:                               # (a deep source has written self._in_f32 itself)
            e.u8_to_f32(self._in_u8, self._in_f32)
        if self.mix is not None:                             # two models: the live ones, one behind the other, then their merge
            y = self._mix_pass()
        else:
            self._y = e.tnet_forward(self.variables, self._in_f32, upsample_method=self.method, bf16=self.bf16, frozen=True,   # one checkpoint, many frames
                                     workspace=self._ws)
            y = self._y
        if self.compose is not None:                         # strength / colour / mask: every conversion below reads the composed tensor
            c = self.compose                                 # (the tensors are B,G,R exactly when the output conversion swaps)
            y = e.compose_f32(self._in_f32, y, self._composed, strength_q8=c["strength_q8"], keep_color=c["keep_color"], matrix=c["matrix"],
                              bgr=self.swap_rb, mask=self._mask, src_swapped=c["source_swapped"])
        if self.temporal is not None:                        # the output conversions belong to the tail (_tail), which reads this
            self._cur = y
            return
        self._outputs(y)

    def _mix_pass(self):
        """The forward passes of the live models into the lane's two output tensors, on the lane's one stream, and fs_mix_f32 of the two; a
        model that is not live lends the other's output, so that there is one arithmetic path (its weights are all 0, or all 256 without a
        mask: the result is to88 of the live output either way).  Each parameter set has its own workspace: with both live the frozen-filter
        check of fs_tnet_forward, which remembers one (parameters, workspace) pair, never matches and both re-layouts are rebuilt per pass;
        a wrong reuse is impossible, since a workspace only ever holds its own parameter set's filters."""
        e, kind = self.eng, self._mix_kind
        if "a" in kind:
            e.tnet_forward(self.variables, self._in_f32, upsample_method=self.method, bf16=self.bf16, frozen=True, workspace=self._ws,
                           out=self._mix_ya)
        if "b" in kind:
            e.tnet_forward(self.variables2, self._in_f32, upsample_method=self.method, bf16=self.bf16, frozen=True, workspace=self._ws2,
                           out=self._mix_yb)
        self._y = self._mix_ya
        return e.mix_f32(self._mix_ya if "a" in kind else self._mix_yb, self._mix_yb if "b" in kind else self._mix_ya, self._mixed,
                         weights=self._mix_w, mask=self._mix_mask, in_hw=self.shape[1:3])

    def _outputs(self, y):
        """The output conversions of y: the net's output, the composed or the stabilised tensor; with deliver= of its top-left H x W
        resampled to the delivery size."""
        e = self.eng
        if self._deliver_plan is not None:
            y = e.resample_f32(e.mem.view(y, 0, self.out_shape), self._deliver_plan, self._delivered)
        elif self._guided is not None:                       # the net's grid against the source at its own size, which the lane still holds
            g = self._guided
            hi, hi_bgr = self._guided_src[self._hi_jpeg]
            y = e.guided_f32(self._in_f32, e.mem.view(y, 0, self.out_shape), hi, self._delivered, self._guided_work, radius=g["radius"],
                             smoothness=g["smoothness"], matrix=g["matrix"], lo_bgr=g["lo_bgr"], hi_bgr=hi_bgr)
        if self._out_deep:                                   # 16-bit samples: straight from the net's fp32 output
            e.f32_to_yuv_deep(y, self.yuv_out_desc, self._result, swap_rb=self.swap_rb)
            return
        e.f32_to_u8(y, self._out_u8, swap_rb=self.swap_rb)
        if self.jpeg is not None:
            e.jpeg_forward_many(self._out_u8, self._jitems, self._coef, items_dev=(self._jitems_dev, 0))
        if self.yuv_out is not None:
            e.rgb_to_yuv_u8(self._out_u8, self.yuv_out_desc, self._result)

    def _tail(self, n):
        """The temporal stage of frame n since construction or reset(), and the output conversions of the stabilised tensor.  It writes
        slot n & 1 and reads slot (n - 1) & 1, so running it twice on one frame (the warm-up of a capture, then the replay) changes nothing."""
        t = self.temporal
        if self._sh is not None:                             # independent streams: which slot and whether there is a previous frame are device words
            self.eng.temporal_streams_f32(self._in_f32, self.eng.mem.view(self._cur, 0, self.out_shape), self._stab, self._sctl, self._tslots,
                                          strength_q8=t["strength_q8"], sensitivity=t["sensitivity"], radius=t["radius"], matrix=t["matrix"],
                                          src_bgr=t["source_bgr"], levels=t.get("levels", 1), subpel=t.get("subpel", 0), overlap=t.get("overlap", 0))
            self._outputs(self._stab)
            return
        kw = dict(prev=None if n == 0 else self._tslots[(n - 1) & 1], strength_q8=t["strength_q8"], sensitivity=t["sensitivity"], radius=t["radius"],
                  matrix=t["matrix"], src_bgr=t["source_bgr"], levels=t.get("levels", 1), **{k: t[k] for k in ("subpel", "overlap") if k in t})
        if self._twork is not None:                          # a pass of consecutive frames: n counts passes
            self.eng.temporal_batch_f32(self._in_f32, self.eng.mem.view(self._cur, 0, self.out_shape), self._stab, self._tslots[n & 1], self._twork, **kw)
        else:
            self.eng.temporal_f32(self._in_f32, self._cur, self._stab, self._tslots[n & 1], **kw)
        self._outputs(self._stab)

    def _captured(self, launches):
        """A graph of what ``launches`` enqueues, after one run of it outside capture (one-time initialisation)."""
        torch = self.eng.mem.torch
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launches()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph(keep_graph=True) if self.KEEP_GRAPH else torch.cuda.CUDAGraph()
        # thread_local: calls made by OTHER threads (e.g. the RCCL watchdog of a data-parallel run) must not
        # invalidate this thread's capture
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            launches()
        return g

    def _capture(self, jpeg_in=False):
        """Capture the device pass of pixel frames (self._graph) or of JPEG frames (self._graph_jpeg).  The warm-up runs the pass once on
        whatever the input buffers hold, and the JPEG pass consumes its coefficients: callers capture BEFORE they upload a JPEG frame."""
        self.eng.invalidate_frozen()                       # the warm-up rebuilds the filters in self._ws whatever the library remembers
        g = self._captured(lambda: self._device_pass(jpeg_in))
        if self.mix is not None:                           # (one head per liveness kind; _mix_prepare has named this pass's)
            self._mix_graphs[(self._mix_kind, jpeg_in)] = g
        elif jpeg_in:
            self._graph_jpeg = g
        else:
            self._graph = g                                # (replays raw pointers into self._ws, which lives as long as this object)

    def _run(self, jpeg_in=False, before_tail=None):
        """The device pass of the frame(s) just uploaded: the captured graph's replay, or eager.  With temporal= that pass is the head, and
        the tail follows: eager, or the replay of the graph of its kind (a first frame's, or the parity's), captured when first needed.
        before_tail: called between the two (a PipelinedStylizer's wait for the previous frame's tail on another stream)."""
        self._hi_jpeg = jpeg_in
        if self.mix is not None:
            self._mix_prepare()                            # (the weights go up ahead of the launches that read them)
        if self._sh is not None:
            self._streams_prepare()                        # (likewise the streams' control words, ahead of the tail)
        if not self._use_graph:
            self._device_pass(jpeg_in)
        elif self.mix is not None:
            if (self._mix_kind, jpeg_in) not in self._mix_graphs:      # (a JPEG pass's: captured by _upload_jpeg, ahead of the upload)
                self._capture(jpeg_in)
            self._mix_graphs[(self._mix_kind, jpeg_in)].replay()
        elif jpeg_in:
            self._graph_jpeg.replay()                      # (captured by _upload_jpeg, ahead of the upload)
        else:
            if self._graph is None:
                self._capture()
            self._graph.replay()
        if self.temporal is None:
            return
        if before_tail is not None:
            before_tail()
        n = self._tn
        if not self._use_graph:
            self._tail(n)
        else:
            kind = "streams" if self._sh is not None else None if n == 0 else n & 1
            if self._guided is not None and jpeg_in:             # (a JPEG frame's guide is another buffer than a pixel frame's)
                kind = (kind, True)
            if kind not in self._tail_graphs:
                self._tail_graphs[kind] = self._captured(lambda: self._tail(n))
            self._tail_graphs[kind].replay()
        self._tn = n + 1
        if self._sh is not None:
            self._streams_advance()

    def reset(self, stream=None):
        """Forget the previous frame: the next one is stabilised as a first frame (temporal= only).  On a streams lane: of one stream
        (its index) or of all (None); the next pass in which that stream is active is its first frame."""
        if self.temporal is None:
            raise L.FaststyleError("reset: this stylizer was built without temporal=")
        if self._sh is None:
            if stream is not None:
                raise L.FaststyleError("reset: stream= names a stream of a lane built with temporal streams=True")
            self._tn = 0
            return
        S = self.shape[0]
        if stream is None:
            self._sh["prev"][:] = [False] * S
            return
        if isinstance(stream, (bool, np.bool_)) or not isinstance(stream, (int, np.integer)) or not 0 <= stream < S:
            raise L.FaststyleError("reset: stream must be a whole number in [0, %d), got %r" % (S, stream))
        self._sh["prev"][int(stream)] = False

    def set_streams(self, active=None):
        """Which streams take part in the passes that follow: ``batch`` booleans, None for all (temporal streams=True only).  An inactive
        stream is skipped by the temporal stage: its state and its slot parity stay, and its row of the stabilised tensor, and so of
        the results, is whatever this lane held there.  Nothing is enqueued here; the next pass uploads the control words ahead of its tail."""
        if self._sh is None:
            raise L.FaststyleError("set_streams: this stylizer was built without temporal streams=True")
        S = self.shape[0]
        if active is None:
            active = [True] * S
        try:
            active = list(active)
        except TypeError:
            raise L.FaststyleError("set_streams: active is %d booleans (the batch), got %r" % (S, active))
        if len(active) != S or not all(isinstance(a, (bool, np.bool_)) for a in active):
            raise L.FaststyleError("set_streams: active is %d booleans (the batch), got %r" % (S, active))
        self._sh["active"][:] = [bool(a) for a in active]

    def _streams_words(self):
        """The control words of the pass under way from the host's view of the streams"""
        h = self._sh
        return [(L.FS_TS_SLOT if p else 0) | ((L.FS_TS_PREV if v else 0) if a else L.FS_TS_SKIP) for v, p, a in zip(h["prev"], h["parity"], h["active"])]

    def _streams_prepare(self):
        """Ahead of a pass (and of the capture of its tail): the control words into the lane's device buffer -- an asynchronous copy on
        the current stream, the lane's, from the lane's staging words, which the previous pass's download has long left behind."""
        self.eng.i32_upload(self._sctl, self._streams_words(), self._sctl_stage)

    def _streams_advance(self):
        """Behind a pass, on the host only (so that the warm-up of a capture and the replay see the same words): every active stream has a
        previous frame now and writes its other slot next; `last` names, per stream, the slot it wrote last."""
        h = self._sh
        for s, a in enumerate(h["active"]):
            if a:
                h["prev"][s] = True
                h["parity"][s] ^= 1
        h["last"] = [L.FS_TS_SLOT * (p ^ 1) for p in h["parity"]]

    def _upload_jpeg(self, staging):
        """Decoded coefficients (decode_frames' staging) -> the device coefficient buffer, on the current stream."""
        mem = self.eng.mem
        if self.mix is not None:
            self._mix_prepare()
            if self._use_graph and (self._mix_kind, True) not in self._mix_graphs:
                self._capture(True)
        elif self._use_graph and self._graph_jpeg is None:
            self._capture(True)
        if hasattr(mem, "torch"):
            self._src_coef.copy_(staging[1], non_blocking=True)
        else:
            self._src_coef[...] = staging[0]

    def release(self):
        """Drop the captured graph (and the encode threads)."""
        self._graph = None
        self._graph_jpeg = None
        self._tail_graphs = {}
        if getattr(self, "mix", None) is not None:
            self._mix_graphs = {}
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def net_input(self):
        """For tests and inspection: a host float32 copy [B,H,W,3] of the net's input tensor as the last pass left it (synchronises)."""
        return np.array(self.eng.mem.to_numpy(self._in_f32), dtype=np.float32, copy=True)

    def net_output(self):
        """For tests and inspection: a host float32 copy [B,Ho,Wo,3] of the net's output tensor of the last pass (synchronises)."""
        if self._y is None:
            raise L.FaststyleError("net_output: this stylizer has not run a frame yet")
        if self.mix is not None and "a" not in self._mix_kind:
            raise L.FaststyleError("net_output: the last pass did not run the first model (every weight was 1 and there is no mask)")
        return np.array(self.eng.mem.to_numpy(self._y), dtype=np.float32, copy=True).reshape(self.out_shape)

    def net_output2(self):
        """For tests and inspection: a host float32 copy [B,Ho,Wo,3] of the second model's output tensor of the last pass (synchronises);
        a stylizer built without mix= has none, and a pass whose weights were all 0 did not run that model."""
        if self.mix is None:
            raise L.FaststyleError("net_output2: this stylizer was built without mix=")
        if self._y is None:
            raise L.FaststyleError("net_output2: this stylizer has not run a frame yet")
        if "b" not in self._mix_kind:
            raise L.FaststyleError("net_output2: the last pass did not run the second model (every weight was 0)")
        return np.array(self.eng.mem.to_numpy(self._mix_yb), dtype=np.float32, copy=True)

    def mixed_output(self):
        """For tests and inspection: a host float32 copy [B,Ho,Wo,3] of the mixed tensor of the last pass (synchronises); a stylizer built
        without mix= has none."""
        if self.mix is None:
            raise L.FaststyleError("mixed_output: this stylizer was built without mix=")
        if self._y is None:
            raise L.FaststyleError("mixed_output: this stylizer has not run a frame yet")
        return np.array(self.eng.mem.to_numpy(self._mixed), dtype=np.float32, copy=True)

    def composed_output(self):
        """For tests and inspection: a host float32 copy [B,Ho,Wo,3] of the composed tensor of the last pass (synchronises); a stylizer built
        without compose= has none."""
        if self._composed is None:
            raise L.FaststyleError("composed_output: this stylizer was built without compose=")
        if self._y is None:
            raise L.FaststyleError("composed_output: this stylizer has not run a frame yet")
        return np.array(self.eng.mem.to_numpy(self._composed), dtype=np.float32, copy=True)

    def stabilised_output(self):
        """For tests and inspection: a host float32 copy [B,Ho,Wo,3] of the stabilised tensor of the last pass (synchronises; B is 1 but on a
        sequence or streams lane, where an inactive stream's row is whatever the lane held); a stylizer built without temporal= has none."""
        if self._stab is None:
            raise L.FaststyleError("stabilised_output: this stylizer was built without temporal=")
        if self._y is None:
            raise L.FaststyleError("stabilised_output: this stylizer has not run a frame yet")
        return np.array(self.eng.mem.to_numpy(self._stab), dtype=np.float32, copy=True)

    def delivered_output(self):
        """For tests and inspection: a host float32 copy [B,Hd,Wd,3] of the delivery tensor of the last pass (synchronises); a stylizer built
        without deliver= has none."""
        if self._delivered is None:
            raise L.FaststyleError("delivered_output: this stylizer was built without deliver=")
        if self._y is None:
            raise L.FaststyleError("delivered_output: this stylizer has not run a frame yet")
        return np.array(self.eng.mem.to_numpy(self._delivered), dtype=np.float32, copy=True)

    def motion_vectors(self):
        """For tests and inspection: the block vectors (dy, dx) of the last pass, host int8 [ceil(Ho / 16), ceil(Wo / 16), 2], on a sequence
        lane of batch N [N, ...], on a streams lane of batch S [S, ...], every stream's from the pass it last took part in (synchronises)."""
        if self._tslots is None:
            raise L.FaststyleError("motion_vectors: this stylizer was built without temporal=")
        if self._tn == 0:
            raise L.FaststyleError("motion_vectors: this stylizer has not run a frame since it was built or reset")
        if self._twork is not None or self._sh is not None:
            return self._batch_vectors()[0]
        return np.array(self.eng.mem.to_numpy(self._tslots[(self._tn - 1) & 1][2]), dtype=np.uint8, copy=True).view(np.int8)

    def _batch_vectors(self):
        """(mv, mvf or None) of the N frames of a sequence lane's last pass"""
        t = self.temporal
        if self._sh is not None:                                 # every stream's from the slot it wrote last
            return self.eng.temporal_streams_vectors(self._tslots, self._sh["last"], self.out_shape[1], self.out_shape[2], t.get("levels", 1),
                                                     t.get("subpel", 0))
        return self.eng.temporal_batch_vectors(self._twork, self._tslots[(self._tn - 1) & 1], self.out_shape[1], self.out_shape[2], self.shape[0],
                                               t.get("levels", 1), t.get("subpel", 0))

    def motion_vectors_subpel(self):
        """For tests and inspection: the block vectors (dy, dx) of the last pass in quarter pixels, 4 mv + mvf, host int16 [ceil(Ho / 16),
        ceil(Wo / 16), 2] (synchronises); a stylizer built without temporal subpel= has none."""
        if self._tslots is None or "subpel" not in self.temporal:
            raise L.FaststyleError("motion_vectors_subpel: this stylizer was built without temporal subpel=")
        mv = self.motion_vectors()                               # (refuses a lane that has not run a frame)
        if self._twork is not None or self._sh is not None:
            return 4 * mv.astype(np.int16) + self._batch_vectors()[1].astype(np.int16)
        mvf = np.array(self.eng.mem.to_numpy(self._tslots[(self._tn - 1) & 1][-1]), dtype=np.uint8, copy=True).view(np.int8)
        return 4 * mv.astype(np.int16) + mvf.astype(np.int16)

    def as_planes(self, a):
        """A frame of a deep source given as 16-bit samples -> the bytes the stylizer takes (anything else: as it is)."""
        if self._src_deep and a.dtype == np.uint16:
            return np.ascontiguousarray(a, dtype="<u2").view(np.uint8)
        return a

    def __call__(self, frames_u8):
        """frames_u8: host uint8 [H,W,3] (or [B,H,W,3]) -> host uint8 stylized frame(s) of the net's output size; with jpeg=: the bytes of
        its JPEG file (a list of them for a batch); with yuv_out=: its planes, uint8 [frame_bytes] (or [B, frame_bytes]).  With source=: the
        frames have the source's size; with source jpeg=: a frame may be the bytes of a JPEG file (a list of them for a batch); with source
        yuv=: a frame is its planes, uint8 [frame_bytes] (or [B, frame_bytes])."""
        mem = self.eng.mem
        files = as_jpeg_frames(frames_u8)
        if files is not None:                                    # JPEG bytes (source jpeg=): host Huffman pass, then everything on the device
            single = isinstance(frames_u8, (bytes, bytearray, memoryview))
            self._upload_jpeg(self.decode_frames(files, self._src_host))       # (raises FrameNotTaken before anything is enqueued)
            self._run(True)
        else:
            a = self.as_planes(np.asarray(frames_u8))
            single = a.ndim == len(self.in_shape) - 1                # ([H,W,3] pixels, or with source yuv= the flat planes of one frame)
            if single:
                a = a[np.newaxis]
            if a.shape != self.in_shape or a.dtype != np.uint8:
                raise L.FaststyleError("frame shape %s dtype %s, stylizer was built for uint8 %s" % (a.shape, a.dtype, self.in_shape))
            if hasattr(mem, "torch"):
                self._pix_dst.copy_(mem.torch.from_numpy(np.ascontiguousarray(a)), non_blocking=True)
            else:
                self._pix_dst[...] = a
            self._run()
        if self.jpeg is not None:
            coef = np.ascontiguousarray(mem.to_numpy(self._coef))  # (synchronises)
            if self._pool is None and self.out_shape[0] > 1 and self._jthreads > 1:
                from concurrent.futures import ThreadPoolExecutor
                self._pool = ThreadPoolExecutor(self._jthreads)
            files = self._write_all(coef.ctypes.data, self._pool)
            return files[0] if single else files
        out = np.array(mem.to_numpy(self._result), copy=True)     # (synchronises; the device buffer is reused next frame)
        return out[0] if single else out


def as_jpeg_frames(frames):
    """[bytes, ...] when ``frames`` is one JPEG file's bytes or a list of them, else None (pixel frames)."""
    if isinstance(frames, (bytes, bytearray, memoryview)):
        return [bytes(frames)]
    if isinstance(frames, (list, tuple)) and frames and all(isinstance(f, (bytes, bytearray, memoryview)) for f in frames):
        return [bytes(f) for f in frames]
    return None


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
    device (fs_jpeg_write holds no interpreter lock).  fetch() / run() then give bytes, in submission order.

    source yuv= and yuv_out= (raw video, see the module docstring) pass through to the lanes: the planes go up from and come down into the
    lanes' pinned buffers, which are sized from the descriptors' frame_bytes (two bytes per sample with bits=N); order and depth are unchanged.
    next_input() lends the next lane's pinned input buffer to a stream reader.  compose= passes through as well; every lane uploads the mask.

    temporal= passes through too.  The recursion orders the tails, not the heads: the two state slots are shared by the lanes and indexed by
    frame parity (with depth 3 a lane meets both), and frame n's tail waits, between its head's and its tail's replay, for an event recorded
    right behind frame n - 1's tail on the other lane's stream; the forward passes of two frames still overlap, and frame n + 1 overwrites
    the slot frame n reads only behind that chain.  Results equal the one-lane results, in order, for any depth.  reset() forgets the
    previous frame and is allowed with nothing in flight.  With temporal sequence=True and batch=N all of this goes by pass of N frames; every
    lane has its own work buffer.  With temporal streams=True the lanes share the one state buffer and the host's view of the streams, each
    has its own control words, and the tails are chained by events per pass in the same way; set_streams() and reset(stream=) apply to the
    passes submitted after them, also with passes in flight.

    mix= is handed to every lane: each has its own second workspace, output tensors, mixed tensor, weight buffer and pinned staging words.
    set_mix(weight) applies to the frames submitted after it: submit() hands the weights to the frame's lane, which uploads them on its own
    stream ahead of its replay.  Results equal the one-lane results, in order, for any depth, also with temporal= and sequence lanes."""

    def __init__(self, eng, variables, height, width, depth=2, jpeg_threads=4, **kw):
        if not hasattr(eng.mem, "torch"):
            raise L.FaststyleError("PipelinedStylizer needs the GPU engine (streams); use FrameStylizer on the emulator")
        import collections
        torch = eng.mem.torch
        self.torch = torch
        self.depth = int(depth)
        self.lanes = []
        for _ in range(self.depth):                              # (temporal=: the first lane allocates the state slots, the others share them)
            more = dict(kw, _temporal_slots=self.lanes[0]._tslots) if self.lanes and kw.get("temporal") is not None else kw
            self.lanes.append(FrameStylizer(eng, variables, height, width, **more))
            self.lanes[-1]._sh = self.lanes[0]._sh               # (temporal streams=True: one host view of the streams; each lane has its own control words)
        self.streams = [torch.cuda.Stream() for _ in self.lanes]
        self.events = [torch.cuda.Event() for _ in self.lanes]
        self.temporal = self.lanes[0].temporal
        self._tail_done = [torch.cuda.Event() for _ in self.lanes] if self.temporal is not None else None
        self._tframe = 0                                         # (temporal=) frames since construction or reset()
        self.mix = self.lanes[0].mix
        self._mix_q8 = self.lanes[0]._mix_q8 if self.mix is not None else None      # (mix=) the weights of the frames submitted from now on
        self.host_in = [torch.empty(ln.in_shape, dtype=torch.uint8, pin_memory=True) for ln in self.lanes]
        self.host_out = [torch.empty(tuple(ln._result.shape), dtype=torch.uint8, pin_memory=True) for ln in self.lanes]
        self.jpeg = self.lanes[0].jpeg
        self._pool = None
        if self.jpeg is not None:
            from concurrent.futures import ThreadPoolExecutor
            self.host_coef = [torch.empty(ln._coef.shape, dtype=torch.uint8, pin_memory=True) for ln in self.lanes]
            self._pool = ThreadPoolExecutor(max(1, int(jpeg_threads)))
        self._pending = collections.deque()
        self._n = 0
        self._single = collections.deque()
        self.source = self.lanes[0].source
        self.yuv_out_desc = self.lanes[0].yuv_out_desc
        # JPEG frames (source jpeg=): run() decodes up to `_ahead` frames beyond the submitted ones (one per decode thread, `depth` at least), and
        # frame number n decodes into staging buffer n % (_ahead + depth) -- when frame n is decoded, frame n - _ahead has been submitted, so frame
        # n - _ahead - depth has been fetched and its upload from that buffer is complete
        self._staging = None
        self._decode_pool = None
        self._ahead = self.depth
        if self.lanes[0]._src_jpeg is not None:
            from concurrent.futures import ThreadPoolExecutor
            threads = max(1, int(jpeg_threads))
            self._ahead = max(self.depth, threads)
            self._staging = [self.lanes[0].new_coef_staging() for _ in range(self._ahead + self.depth)]
            self._decode_pool = ThreadPoolExecutor(threads)

    def _decode(self, files, n):
        """Frame number n's host half (any thread): its decoded staging buffer, or raises FrameNotTaken."""
        return self.lanes[0].decode_frames(files, self._staging[n % len(self._staging)])

    def submit(self, frames_u8, _decoded=None):
        """Enqueue one frame (pixels; with source jpeg= also the bytes of a JPEG file, decoded here on the calling thread)."""
        if len(self._pending) >= self.depth:
            raise L.FaststyleError("PipelinedStylizer: %d frames in flight already -- fetch() one first" % self.depth)
        k = self._n % self.depth
        ln, st, torch = self.lanes[k], self.streams[k], self.torch
        files = as_jpeg_frames(frames_u8)
        if files is not None:
            single = not isinstance(frames_u8, (list, tuple))
            staged = _decoded if _decoded is not None else self._decode(files, self._n)      # (FrameNotTaken: nothing is enqueued)
        else:
            a = ln.as_planes(np.asarray(frames_u8))
            single = a.ndim == len(ln.in_shape) - 1
            if single:
                a = a[np.newaxis]
            if a.shape != ln.in_shape or a.dtype != np.uint8:
                raise L.FaststyleError("frame shape %s dtype %s, stylizer was built for uint8 %s" % (a.shape, a.dtype, ln.in_shape))
            if a.ctypes.data != self.host_in[k].data_ptr():                        # (next_input()'s buffer, filled in place: nothing to copy)
                self.host_in[k].copy_(torch.from_numpy(np.ascontiguousarray(a)))   # (host -> pinned host; the lane's previous frame was fetched: its buffers are free)
        before_tail = None
        if self.temporal is not None:                             # this frame's tail follows the previous frame's, wherever that one ran
            ln._tn = self._tframe
            if self._tframe > 0:
                done = self._tail_done[(self._n - 1) % self.depth]
                before_tail = lambda: st.wait_event(done)
        if self.mix is not None:                                  # the lane uploads them on its stream, from its own pinned words,
            ln._mix_q8 = self._mix_q8                             # ahead of its replay (its previous frame was fetched: the words are free)
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            if files is not None:
                ln._upload_jpeg(staged)
                ln._run(True, before_tail)
            else:
                ln._pix_dst.copy_(self.host_in[k], non_blocking=True)
                ln._run(False, before_tail)
            if self.temporal is not None:
                self._tail_done[k].record(st)
                self._tframe += 1
            if self.jpeg is not None:
                self.host_coef[k].copy_(ln._coef, non_blocking=True)
            else:
                self.host_out[k].copy_(ln._result, non_blocking=True)
            self.events[k].record(st)
        if self.jpeg is not None:
            k = (k, self._pool.submit(self._encode, k))           # (the lane is reused only after fetch() has taken this result)
        self._pending.append(k)
        self._single.append(single)
        self._n += 1

    @property
    def in_flight(self):
        """Frames submitted and not yet fetched (at most `depth`)."""
        return len(self._pending)

    def reset(self, stream=None):
        """Forget the previous frame (temporal= only); with nothing in flight.  With temporal streams=True: of one stream (its index) or of
        all (None), for the passes submitted after this call -- passes in flight keep the control words they were submitted with."""
        if self.temporal is None:
            raise L.FaststyleError("reset: this stylizer was built without temporal=")
        if self.lanes[0]._sh is not None or stream is not None:  # (the chain of tails goes on: _tframe stays)
            self.lanes[0].reset(stream)
            return
        if self._pending:
            raise L.FaststyleError("reset: %d frames in flight -- fetch() them first" % len(self._pending))
        self._tframe = 0

    def set_streams(self, active=None):
        """Which streams take part in the passes submitted after this call (temporal streams=True only): ``batch`` booleans, None for all.
        Passes in flight keep the control words they were submitted with."""
        self.lanes[0].set_streams(active)

    def set_mix(self, weight):
        """The share of the second model in the frames submitted after this call (mix= only): a number in [0, 1], or ``batch`` numbers for
        a pass of consecutive frames.  Frames in flight keep the weights they were submitted with."""
        if self.mix is None:
            raise L.FaststyleError("set_mix: this stylizer was built without mix=")
        self._mix_q8 = self.lanes[0]._mix_q8_of(weight)

    def next_input(self):
        """The pinned input buffer of the lane the next submit() uses, as a numpy array of the lane's in_shape: a reader fills it in place
        (y4m.Reader.read_frame_into) and hands it -- or its first row, for a single frame -- to submit(), which then copies nothing on the
        host.  Valid while fewer than `depth` frames are in flight: the lane's previous upload has completed once its result was fetched."""
        if len(self._pending) >= self.depth:
            raise L.FaststyleError("PipelinedStylizer: %d frames in flight already -- fetch() one first" % self.depth)
        return self.host_in[self._n % self.depth].numpy()

    def _encode(self, k):
        """On an encode thread: wait for lane k's download, then Huffman-code its frame(s)."""
        self.events[k].synchronize()
        return self.lanes[k]._write_all(self.host_coef[k].data_ptr())

    def fetch(self):
        """The oldest submitted frame's result (host uint8; bytes with jpeg=; the planes with yuv_out=), waiting for its lane only."""
        k = self._pending.popleft()
        single = self._single.popleft()
        if self.jpeg is not None:
            files = k[1].result()
            return files[0] if single else files
        self.events[k].synchronize()
        out = self.host_out[k].numpy().copy()
        return out[0] if single else out

    def run(self, frames, not_taken=None, before_submit=None):
        """Results of ``frames`` in order, `depth` of them in flight.  JPEG frames (bytes) are decoded ahead on the thread pool, one frame
        per decode thread beyond the submitted ones: the Huffman pass of the next frames overlaps device work.  not_taken: called with the bytes of a
        frame that raised FrameNotTaken, returns its pixels (the driver's PIL decode); without it the exception reaches the caller.
        before_submit: called ahead of every submit(), in order (a driver's set_mix() of that frame: frames are decoded ahead, so the
        iterable itself runs ahead of the submits)."""
        import collections
        ahead = collections.deque()                              # (frame, decode future or None), in order
        it = iter(frames)
        done = False
        while True:
            while not done and len(ahead) < self._ahead:
                try:
                    f = next(it)
                except StopIteration:
                    done = True
                    break
                files = as_jpeg_frames(f)
                n = self._n + len(ahead)
                ahead.append((f, self._decode_pool.submit(self._decode, files, n) if files is not None and self._decode_pool is not None else None))
            if not ahead:
                break
            f, fut = ahead.popleft()
            staged = None
            if fut is not None:
                try:
                    staged = fut.result()
                except FrameNotTaken:
                    if not_taken is None:
                        for _, other in ahead:                   # (let the decodes in flight finish: they write into this object's buffers)
                            if other is not None:
                                other.exception()
                        raise
                    f = not_taken(f)
            if len(self._pending) >= self.depth:
                yield self.fetch()
            if before_submit is not None:
                before_submit()
            self.submit(f, _decoded=staged)
        while self._pending:
            yield self.fetch()

    def release(self):
        for ln in self.lanes:
            ln.release()
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        if getattr(self, "_decode_pool", None) is not None:
            self._decode_pool.shutdown(wait=True)
            self._decode_pool = None
