"""YUV4MPEG2 ("Y4M") streams: the raw video container that ``ffmpeg -f yuv4mpegpipe``, x264, mpv and others read and write on pipes.

A stream is one text header line

    YUV4MPEG2 W<width> H<height> F<num>:<den> I<interlacing> A<num>:<den> C<colour space> X<extension> ...\\n

(tags in any order, only W and H required) and then, per frame, the line ``FRAME`` (optionally followed by parameters, which are ignored) and
the frame's planes: Y, then Cb, then Cr, 8 bits per sample (or, in a deep stream, 9 to 16 bits in little-endian 16-bit words), no padding
-- exactly the layout of include/faststyle_io.h's fs_yuv_desc, so a frame goes from the stream into a lane's pinned staging buffer with one
``readinto`` and from there to the device as it is.

Taken: ``C420jpeg``, a bare ``C420`` and a missing C tag (4:2:0, chroma sited at the centre of its 2x2 cell), ``C420mpeg2`` and ``C420paldv``
(4:2:0, chroma horizontally co-sited with the even luma column; paldv's vertical chroma offset of half a line is ignored: its chroma rows are
treated as mpeg2's), ``C422`` (co-sited), ``C444``, ``Cmono``; ``XCOLORRANGE=FULL`` / ``=LIMITED`` (default limited); progressive streams
(``Ip``, ``I?`` or no I tag).  With ``deep=True`` (``parse_header``, ``Reader``) also the deep tags ``ffmpeg -f yuv4mpegpipe`` writes for
sources of more than 8 bits: ``C420pN`` (centre-sited, like a bare ``C420``), ``C422pN`` (co-sited), ``C444pN`` and ``CmonoN`` for N in 9..16;
``Format.bits`` is N and ``frame_bytes`` counts two bytes per sample.  Refused, with a message that names the tag: without ``deep=True`` every
bit depth above 8 (``C420p10`` ...; the message says how to opt in), always ``C411``, ``C444alpha``, depths outside 9..16 and interlaced
streams (``It``, ``Ib``, ``Im``).  ``header(..., bits=N)`` and ``Writer`` (from a desc of ``fs_yuv_plan_deep``) write the deep tags; a deep
co-sited 4:2:0 stream has no tag and raises.  Host code only; it needs neither the library nor a device."""
import collections

MAGIC = b"YUV4MPEG2"
FRAME = b"FRAME"
MAX_LINE = 4096          # a header or frame line longer than this is not a Y4M stream

# C tag -> (sampling (hs, vs), siting, components)
COLOURSPACES = {
    "420jpeg": ((2, 2), 0, 3), "420": ((2, 2), 0, 3), "420mpeg2": ((2, 2), 1, 3), "420paldv": ((2, 2), 1, 3),
    "422": ((2, 1), 1, 3), "444": ((1, 1), 0, 3), "mono": ((1, 1), 0, 1),
}

# deep C tags (deep=True): prefix -> (sampling, siting, components); the depth follows the prefix
DEEP_COLOURSPACES = {"420p": ((2, 2), 0, 3), "422p": ((2, 1), 1, 3), "444p": ((1, 1), 0, 3), "mono": ((1, 1), 0, 1)}
DEEP_BITS = range(9, 17)
DEEP_HINT = "pass deep=True (stylize_webcam.py: --video_depth stream) to take 9 to 16 bits per sample"


def deep_colourspace(text):
    """(sampling, siting, components, bits) of a deep C tag's text (``420p10``, ``mono16`` ...); None for anything else."""
    prefix, digits = text[:4], text[4:]
    if prefix not in DEEP_COLOURSPACES or not digits.isdigit() or digits[0] == "0" or int(digits) not in DEEP_BITS:
        return None
    return DEEP_COLOURSPACES[prefix] + (int(digits),)


class Y4MError(ValueError):
    pass


Format = collections.namedtuple("Format", "width height sampling siting components full_range rate aspect colourspace frame_bytes bits")
Format.__doc__ = """What a stream's header says: sampling (hs, vs), siting 0 centre / 1 co-sited, components 3 / 1, rate and aspect as (num, den)
(None where the header has no such tag), the C tag as written (None: absent), the bytes of one frame's planes, and the bits per sample
(8; 9 to 16 for a deep stream, whose samples are 16-bit words)."""


def frame_bytes(width, height, sampling, components, bits=8):
    hs, vs = sampling
    per = 1 if int(bits) == 8 else 2
    if components == 1:
        return per * width * height
    return per * (width * height + 2 * ((width + hs - 1) // hs) * ((height + vs - 1) // vs))


def _ratio(tag, text):
    try:
        num, den = text.split(":")
        return int(num), int(den)
    except ValueError:
        raise Y4MError("Y4M header: tag %s%s is not <num>:<den>" % (tag, text))


def parse_header(line, deep=False):
    """The Format of a header line (bytes, with or without the newline).  deep: also take the tags of 9 to 16 bits per sample."""
    try:
        fields = line.decode("ascii").split()
    except UnicodeDecodeError:
        raise Y4MError("not a YUV4MPEG2 stream: the header is not ASCII")
    if not fields or fields[0] != MAGIC.decode():
        raise Y4MError("not a YUV4MPEG2 stream: the header begins %r" % line[:16])
    width = height = rate = aspect = cs = None
    full = False
    layout = None
    for f in fields[1:]:
        tag, text = f[0], f[1:]
        if tag in "WH":
            try:
                v = int(text)
            except ValueError:
                v = 0
            if v < 1:
                raise Y4MError("Y4M header: tag %s is not a positive size" % f)
            if tag == "W":
                width = v
            else:
                height = v
        elif tag == "F":
            rate = _ratio(tag, text)
        elif tag == "A":
            aspect = _ratio(tag, text)
        elif tag == "I":
            if text not in ("p", "?"):
                raise Y4MError("Y4M header: tag %s: interlaced streams are not taken (progressive only)" % f)
        elif tag == "C":
            layout = COLOURSPACES[text] + (8,) if text in COLOURSPACES else deep_colourspace(text)
            if layout is None or (layout[3] != 8 and not deep):
                why = "alpha planes are not taken" if "alpha" in text else "4:1:1 is not taken" if text[:3] == "411" else \
                    "bit depths above 8 are not taken; " + DEEP_HINT if layout is not None else \
                    "bit depths outside 9..16 are not taken" if text[:4] == "mono" or (text[:3] in ("420", "422", "444") and text[3:4] == "p") else \
                    "unknown colour space"
                raise Y4MError("Y4M header: tag %s: %s" % (f, why))
            cs = text
        elif tag == "X":
            if text.startswith("COLORRANGE="):
                value = text[len("COLORRANGE="):]
                if value not in ("FULL", "LIMITED"):
                    raise Y4MError("Y4M header: tag %s: the range is FULL or LIMITED" % f)
                full = value == "FULL"
        else:
            raise Y4MError("Y4M header: unknown tag %s" % f)
    if width is None or height is None:
        raise Y4MError("Y4M header: no W or no H tag in %r" % line[:80])
    sampling, siting, components, bits = layout if layout is not None else COLOURSPACES["420jpeg"] + (8,)
    return Format(width, height, sampling, siting, components, full, rate, aspect, cs, frame_bytes(width, height, sampling, components, bits), bits)


def _read_line(f, what):
    """One line of ``f`` without its newline (readline: a buffered object keeps what it read ahead for the readinto calls that follow, a raw one
    reads byte by byte); None at the end of the stream."""
    line = f.readline(MAX_LINE + 1)
    if line and not line.endswith(b"\n"):
        if len(line) > MAX_LINE:
            raise Y4MError("%s: no newline within %d bytes" % (what, MAX_LINE))
        raise Y4MError("%s: the stream ends inside the line %r" % (what, line[:32]))
    return line[:-1] if line else None


def _write_all(f, view):
    """f.write of the whole view: a raw (unbuffered) object may take less than it is given."""
    while len(view):
        k = f.write(view)
        if k is None or k >= len(view):
            return
        view = view[k:]


class Reader(object):
    """Frames of a YUV4MPEG2 stream from any binary file object -- a pipe or ``sys.stdin.buffer`` as well: nothing seeks.

        r = Reader(f)                        # reads the header: r.format
        while r.read_frame_into(buf): ...    # buf: a writable buffer of r.format.frame_bytes bytes (a lane's pinned staging)

    deep=True also takes streams of 9 to 16 bits per sample (r.format.bits), two bytes per sample in the buffer.
    """

    def __init__(self, f, deep=False):
        self.f = f
        line = _read_line(f, "Y4M header")
        if line is None:
            raise Y4MError("not a YUV4MPEG2 stream: it is empty")
        self.format = parse_header(line, deep)
        self.frames = 0

    def read_frame_into(self, buffer):
        """Fills ``buffer`` with the next frame's planes; False on a clean end of stream (at a frame boundary).  Raises Y4MError for a bad
        frame line or a stream that ends inside a frame."""
        view = memoryview(buffer).cast("B")
        n = self.format.frame_bytes
        if len(view) != n:
            raise Y4MError("a frame of this stream is %d bytes, the buffer holds %d" % (n, len(view)))
        line = _read_line(self.f, "Y4M frame %d" % self.frames)
        if line is None:
            return False
        if line[:len(FRAME)] != FRAME or line[len(FRAME):len(FRAME) + 1] not in (b"", b" "):
            raise Y4MError("Y4M frame %d: expected FRAME, found %r" % (self.frames, line[:16]))
        got = 0
        while got < n:
            k = self.f.readinto(view[got:])
            if not k:
                raise Y4MError("Y4M frame %d: the stream ends after %d of %d bytes" % (self.frames, got, n))
            got += k
        self.frames += 1
        return True


def header(width, height, sampling=(2, 2), siting=0, components=3, full_range=False, rate=None, aspect=None, bits=8):
    """The header line of a stream of such frames (bytes, with the newline): progressive; the C tag by sampling and siting (420jpeg, 420mpeg2,
    422, 444, mono; the format has no tag for centre-sited 4:2:2, which is refused); XCOLORRANGE always written, so that a reader need not know
    the default.  bits 9..16: the deep tags 420pN, 422pN, 444pN, monoN (no tag for co-sited 4:2:0 either, which is refused)."""
    sampling = tuple(int(v) for v in sampling)
    bits = int(bits)
    if bits != 8 and bits not in DEEP_BITS:
        raise Y4MError("no Y4M colour space for %r bits per sample" % bits)
    if components == 1:
        cs = "mono"
    else:
        names = {((2, 2), 0): "420jpeg", ((2, 2), 1): "420mpeg2", ((2, 1), 1): "422", ((1, 1), 0): "444", ((1, 1), 1): "444"} if bits == 8 else \
            {((2, 2), 0): "420p", ((2, 1), 1): "422p", ((1, 1), 0): "444p", ((1, 1), 1): "444p"}
        cs = names.get((sampling, int(siting)))
        if cs is None or components != 3:
            raise Y4MError("no Y4M colour space for sampling %r, siting %r, %r components at %d bits" % (sampling, siting, components, bits))
    if bits != 8:
        cs += "%d" % bits
    fields = ["YUV4MPEG2", "W%d" % width, "H%d" % height]
    if rate is not None:
        fields.append("F%d:%d" % tuple(rate))
    fields.append("Ip")
    if aspect is not None:
        fields.append("A%d:%d" % tuple(aspect))
    fields += ["C" + cs, "XCOLORRANGE=" + ("FULL" if full_range else "LIMITED")]
    return (" ".join(fields) + "\n").encode("ascii")


class Writer(object):
    """Writes a stream: the header from a frame descriptor (an fs_yuv_desc, or anything with width, height, hs, vs, ncomp, siting, full_range)
    plus frame rate and aspect, then frames from buffers of frame_bytes bytes.  A desc of fs_yuv_plan_deep (reserved[0] = bits per sample)
    writes a deep stream."""

    def __init__(self, f, desc, rate=None, aspect=None):
        self.f = f
        reserved = getattr(desc, "reserved", None)
        self.bits = int(reserved[0]) if reserved is not None and int(reserved[0]) else 8
        self.frame_bytes = frame_bytes(int(desc.width), int(desc.height), (int(desc.hs), int(desc.vs)), int(desc.ncomp), self.bits)
        f.write(header(int(desc.width), int(desc.height), (int(desc.hs), int(desc.vs)), int(desc.siting), int(desc.ncomp), bool(desc.full_range),
                       rate, aspect, self.bits))
        self.frames = 0

    def write_frame(self, buffer):
        view = memoryview(buffer).cast("B")
        if len(view) != self.frame_bytes:
            raise Y4MError("a frame of this stream is %d bytes, the buffer holds %d" % (self.frame_bytes, len(view)))
        _write_all(self.f, memoryview(b"FRAME\n"))
        _write_all(self.f, view)
        self.frames += 1

    def flush(self):
        self.f.flush()
