"""CPU: what every frame entry point of libsba_hip.so answers to a bad call -- the status and the WHOLE sentence of
sba_last_error, which of two faults is reported, that no output is touched -- and what it answers to a good one when no GPU is
there.  Raw ctypes calls, as tests/test_adaptive_symbol.py makes them.  The literals were recorded from the library as it was
before the entry points were given one description of a batch (FrameBatch) and shared checks; they pin that nothing a caller can
see of the argument checks has moved since.

The batch of every call: 2 frames of 4 rows of 6 pixels, 3 channels, packed.  A table row is (what is changed of the valid
call, status, sentence after "<function>: ")."""
import ctypes
import os

import numpy as np
import pytest

from lasercalib_amd import _native

N, H, W, CH = 2, 4, 6, 3
ROW, FRAME = W * CH, H * W * CH
SENTINEL = 0xA5
INVALID, NO_DEVICE, UNSUPPORTED = -1, -2, -6
NAN, INF = float("nan"), float("inf")
BIG = 16385                                                                # one more than the largest height or width

NEG, NULL_FRAMES, CHANNELS = "negative size", "null frames", "channels must be 1, 3 or 4"
CHANNEL, THRESHOLD = "channel out of range", "threshold must be in 0..255"
ROW_PITCH, FRAME_PITCH = "row_pitch is smaller than width * channels", "frame_pitch is smaller than height * row_pitch"
OVERFLOW = "n_frames * frame_pitch overflows"
LIMIT = "width and height are limited to 16384"
OUT_OVERFLOW = "n_frames * out_frame_pitch overflows"
OUT_FRAME = "out_frame_pitch is smaller than height * out_row_pitch"
GRAY_NEG, GRAY_SUM = "a gray weight is negative", "the gray weights must sum to 2^15"
GRAY_ONE = "channel -1 (gray) needs 3 or 4 channels"
NULL_LENS, LENS_FINITE, NEWK_FINITE, FOCAL = ("null lens or new_k", "a lens value is not finite", "a new_k value is not finite",
                                              "a focal length is not > 0")
OUT_SIZE, INTERP = "the output size must be in 0..16384", "interpolation must be 0 (bilinear) or 1 (nearest)"
NO_OUT = "null out and no diagnostic asked for"
NULL_PLANE, C_STEP = "null plane", "c_step must be 1 (planar) or 2 (interleaved)"
Y_ROW, Y_FRAME = "y_row_pitch is smaller than width", "y_frame_pitch is smaller than height * y_row_pitch"
C_ROW = "c_row_pitch is smaller than c_step * ((width + 1) / 2 - 1) + 1"
C_FRAME = "c_frame_pitch is smaller than ((height + 1) / 2) * c_row_pitch"
PLANE_OVERFLOW = "n_frames * a frame pitch overflows"
Y_OFFSET = "matrix: y_offset must be in 0..255"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _native.load()


def buf(nbytes):
    return np.full(nbytes, SENTINEL, np.uint8)


LENS = dict(fx=5.0, fy=5.0, cx=3.0, cy=2.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0)
PLANES = dict(y_row_pitch=W, y_frame_pitch=H * W, c_row_pitch=W // 2, c_frame_pitch=(H // 2) * (W // 2), c_step=1, reserved=0)


class Entry:
    """One entry point: its parameters in the order of the ABI with the values of a valid call, and the class and the values
    of its options.  A parameter's value is None, an integer, an array (its address is passed), a tuple (an array of float64;
    of int64 for corner_start) or, for a parameter that points at a structure (``structs``), a dict of the structure's fields.
    call(**changes) replaces parameters by name; a dict for a structure replaces single fields; any other name is a field of
    the options.  Every array among the defaults is filled with the sentinel and must still be after a call that fails."""

    def __init__(self, name, params, opts_cls, opts, structs=None, early_return=True):
        self.name, self.params, self.opts_cls, self.opts, self.structs = name, params, opts_cls, opts, structs or {}
        self.early_return = early_return                                  # returns for n_frames == 0 before any work on the device
        self.buffers = [v for v in params.values() if isinstance(v, np.ndarray)]
        for v in params.values():
            if isinstance(v, dict):
                self.buffers += [x for x in v.values() if isinstance(x, np.ndarray)]

    def call(self, lib, **changes):
        fn, keep, args = getattr(lib, self.name), [], []
        opts = dict(self.opts)
        opts.update({k: v for k, v in changes.items() if k not in self.params})
        for (name, value), argtype in zip(self.params.items(), fn.argtypes):
            if name in changes:
                value = dict(value or {}, **changes[name]) if isinstance(changes[name], dict) else changes[name]
            if name == "opts" and "opts" not in changes:
                value = self.opts_cls()
                for k, v in opts.items():
                    field = getattr(value, k)
                    setattr(value, k, type(field)(*v) if isinstance(v, tuple) else v)
            elif isinstance(value, dict):
                value = self.structs[name](**{k: v.ctypes.data if isinstance(v, np.ndarray) else v for k, v in value.items()})
            elif isinstance(value, tuple):
                value = np.array(value, np.int64 if name == "corner_start" else np.float64)
            keep.append(value)
            if isinstance(value, ctypes.Structure):
                value = ctypes.byref(value)
            elif isinstance(value, np.ndarray):
                value = value.ctypes.data
            if isinstance(value, int) and issubclass(argtype, ctypes._Pointer):
                value = ctypes.cast(ctypes.c_void_p(value), argtype)
            args.append(value)
        rc = fn(*args)
        return rc, (lib.sba_last_error(None) or b"").decode()

    def untouched(self):
        return all(bool(np.all(b == SENTINEL)) for b in self.buffers)


def source(channels=CH):
    """The eight scalars every call with interleaved frames starts with; the frames themselves are never read here."""
    return dict(device=0, frames=np.zeros(N * H * W * channels, np.uint8), n_frames=N, height=H, width=W, channels=channels,
                row_pitch=W * channels, frame_pitch=H * W * channels)


def planes():
    return dict(PLANES, y=buf(N * H * W), u=buf(N * H * W // 4), v=buf(N * H * W // 4))


def entry(name, extra, opts_cls, opts, **kw):
    p = source()
    p["frames"] = p["frames"].copy()
    e = Entry(name, dict(p, **extra), opts_cls, opts, **kw)
    e.buffers = [b for b in e.buffers if b is not e.params["frames"]]
    return e


# ---- rows that several tables share
SOURCE = [                                                                 # frame_args_invalid, without the channel and the threshold
    (dict(n_frames=-1), INVALID, NEG),
    (dict(height=-1), INVALID, NEG),
    (dict(width=-1), INVALID, NEG),
    (dict(frames=None), INVALID, NULL_FRAMES),
    (dict(channels=2), INVALID, CHANNELS),
    (dict(channels=0), INVALID, CHANNELS),
]
PITCHES = [                                                                # frame_layout_invalid
    (dict(row_pitch=ROW - 1), INVALID, ROW_PITCH),
    (dict(frame_pitch=FRAME - 1), INVALID, FRAME_PITCH),
    (dict(n_frames=3, frame_pitch=1 << 62), INVALID, OVERFLOW),
]
GRAY_W = [(dict(gray_w=(-1, 32768, 1)), INVALID, GRAY_NEG), (dict(gray_w=(1, 2, 3)), INVALID, GRAY_SUM)]
TALL = dict(height=BIG, frame_pitch=BIG * ROW)                             # a source one row too tall, its pitches in order
LENS_ROWS = [
    (dict(lens=None), INVALID, NULL_LENS),
    (dict(lens=dict(fx=NAN)), INVALID, LENS_FINITE),
    (dict(lens=dict(k3=INF)), INVALID, LENS_FINITE),
    (dict(lens=dict(fx=0.0)), INVALID, FOCAL),
    (dict(lens=dict(fy=-1.0)), INVALID, FOCAL),
]
NEWK_ROWS = [
    (dict(new_k=None), INVALID, NULL_LENS),
    (dict(new_k=(5.0, 5.0, INF, 2.0)), INVALID, NEWK_FINITE),
    (dict(new_k=(0.0, 5.0, 3.0, 2.0)), INVALID, FOCAL),
    (dict(new_k=(5.0, -5.0, 3.0, 2.0)), INVALID, FOCAL),
]
RESAMPLE = [
    (dict(out_height=-1), INVALID, OUT_SIZE),
    (dict(out_height=BIG), INVALID, OUT_SIZE),
    (dict(out_width=-1), INVALID, OUT_SIZE),
    (dict(out_width=BIG), INVALID, OUT_SIZE),
    (dict(interpolation=2), INVALID, INTERP),
    (dict(interpolation=-1), INVALID, INTERP),
]


def plane_rows(key, side, width="width"):
    """yuv_planes_invalid for the planes in parameter ``key`` (None: loose arguments), with what opens the sentence."""
    def ch(**d):
        return {key: d} if key else d
    return [
        (ch(y=None), INVALID, side + NULL_PLANE),
        (ch(u=None), INVALID, side + NULL_PLANE),
        (ch(v=None), INVALID, side + NULL_PLANE),
        (ch(c_step=0), INVALID, side + C_STEP),
        (ch(c_step=3), INVALID, side + C_STEP),
        (ch(y_row_pitch=W - 1), INVALID, side + Y_ROW),
        (ch(y_frame_pitch=H * W - 1), INVALID, side + Y_FRAME),
        (ch(c_row_pitch=W // 2 - 1), INVALID, side + C_ROW),
        (ch(c_row_pitch=-1), INVALID, side + C_ROW),
        (dict(ch(c_row_pitch=-1), **{width: 0}), INVALID, side + C_FRAME),     # no chroma samples in a row: the row pitch is not compared
        (ch(c_frame_pitch=(H // 2) * (W // 2) - 1), INVALID, side + C_FRAME),
        (dict(ch(y_frame_pitch=1 << 62), n_frames=3), INVALID, side + PLANE_OVERFLOW),
        (dict(ch(c_frame_pitch=1 << 62), n_frames=3), INVALID, side + PLANE_OVERFLOW),
    ]


def through_lens(name, model_key, model_value):
    return entry(name, dict(lens=dict(LENS), **{model_key: model_value}, out_height=H, out_width=W, out_row_pitch=ROW,
                            out_frame_pitch=FRAME, opts=None, out=buf(N * FRAME), flags_out=buf(H * W), map_out=buf(8 * H * W)),
                 _native.UndistortOpts, dict(), structs=dict(lens=_native.LensStruct), early_return=False)


def through_lens_rows():
    """What sba_undistort_frames and sba_warp_frames share after the lens and the model: (single faults, order)."""
    single = RESAMPLE + [
        (dict(border_value=256), INVALID, "border_value must be in 0..255"),
        (dict(border_value=-1), INVALID, "border_value must be in 0..255"),
        (dict(out=None, flags_out=None, map_out=None), INVALID, NO_OUT),
        (dict(out_row_pitch=ROW - 1), INVALID, "out_row_pitch is smaller than out_width * channels"),
        (dict(out_frame_pitch=FRAME - 1), INVALID, "out_frame_pitch is smaller than out_height * out_row_pitch"),
        (dict(n_frames=3, frame_pitch=FRAME, out_frame_pitch=1 << 62), INVALID, OUT_OVERFLOW),
    ] + PITCHES + [(TALL, UNSUPPORTED, LIMIT), (dict(width=BIG, row_pitch=BIG * CH, frame_pitch=H * BIG * CH), UNSUPPORTED, LIMIT)]
    order = [
        (dict(n_frames=-1, lens=None), INVALID, NEG),                     # the source, then the lens
        (dict(lens=None, out_height=-1), INVALID, NULL_LENS),             # the lens, then the options
        (dict(out_width=BIG, interpolation=2), INVALID, OUT_SIZE),
        (dict(interpolation=2, border_value=256), INVALID, INTERP),
        (dict(border_value=256, out_row_pitch=ROW - 1), INVALID, "border_value must be in 0..255"),
        (dict(out=None, flags_out=None, map_out=None, row_pitch=ROW - 1), INVALID, NO_OUT),
        (dict(out_row_pitch=ROW - 1, row_pitch=ROW - 1), INVALID, "out_row_pitch is smaller than out_width * channels"),
        (dict(out=None, out_row_pitch=ROW - 1, row_pitch=ROW - 1), INVALID, ROW_PITCH),     # no out: its pitches are not looked at
        (dict(out=None, out_frame_pitch=0, **TALL), UNSUPPORTED, LIMIT),
        (dict(row_pitch=ROW - 1, **TALL), INVALID, ROW_PITCH),            # the pitches, then the limit
        (dict(out_frame_pitch=FRAME - 1, **TALL), INVALID, "out_frame_pitch is smaller than out_height * out_row_pitch"),
    ]
    return single, order


# ---- the entry points: (entry, single faults, order, calls that return early)
def dots():
    e = entry("sba_detect_dots", dict(opts=None, sums=buf(256), box=buf(64), centroid=buf(64), status=buf(16)),
              _native.DotOpts, dict(channel=1, threshold=50))
    why = LIMIT + " (the bound under which every sum fits 64 bits)"
    single = SOURCE + [
        (dict(channel=3), INVALID, CHANNEL),
        (dict(channel=-1), INVALID, CHANNEL),
        (dict(threshold=256), INVALID, THRESHOLD),
        (dict(threshold=-1), INVALID, THRESHOLD),
        (dict(min_area=-1), INVALID, "negative area or extent limit"),
        (dict(max_area=-1), INVALID, "negative area or extent limit"),
        (dict(max_extent=-1), INVALID, "negative area or extent limit"),
    ] + PITCHES + [(TALL, UNSUPPORTED, why), (dict(width=BIG, row_pitch=BIG * CH, frame_pitch=H * BIG * CH), UNSUPPORTED, why)]
    order = [
        (dict(n_frames=-1, min_area=-1), INVALID, NEG),
        (dict(frames=None, channels=2), INVALID, NULL_FRAMES),
        (dict(channels=2, channel=3), INVALID, CHANNELS),
        (dict(channel=3, threshold=256), INVALID, CHANNEL),
        (dict(threshold=256, max_extent=-1), INVALID, THRESHOLD),
        (dict(min_area=-1, row_pitch=ROW - 1), INVALID, "negative area or extent limit"),
        (dict(row_pitch=ROW - 1, frame_pitch=0), INVALID, ROW_PITCH),
        (dict(row_pitch=ROW - 1, **TALL), INVALID, ROW_PITCH),
        (dict(n_frames=0, **TALL), UNSUPPORTED, why),                     # no frames, but the limit is looked at first
    ]
    return e, single, order, [dict(n_frames=0), dict(n_frames=0, frames=None)]


def blobs():
    e = entry("sba_detect_blobs", dict(opts=None, n_components=buf(16), blobs=buf(8 * 12 * 8 * N), accepted=buf(16), centroid=buf(64),
                                       status=buf(16), mask_out=buf(N * H * W), labels_out=buf(4 * N * H * W)),
              _native.BlobOpts, dict(channel=1, threshold=70, dilate_radius=1, close_radius=4, max_blobs=8))
    single = SOURCE + [
        (dict(channel=3), INVALID, CHANNEL),
        (dict(threshold=256), INVALID, THRESHOLD),
        (dict(dilate_radius=9), INVALID, "a radius must be in 0..8"),
        (dict(dilate_radius=-1), INVALID, "a radius must be in 0..8"),
        (dict(close_radius=9), INVALID, "a radius must be in 0..8"),
        (dict(close_radius=-1), INVALID, "a radius must be in 0..8"),
        (dict(max_blobs=65), INVALID, "max_blobs must be in 0..64"),
        (dict(max_blobs=-1), INVALID, "max_blobs must be in 0..64"),
        (dict(min_area=-1), INVALID, "negative area or distance limit"),
        (dict(max_area=-1), INVALID, "negative area or distance limit"),
        (dict(max_centre_dist=-1), INVALID, "negative area or distance limit"),
    ] + PITCHES + [(TALL, UNSUPPORTED, LIMIT)]
    order = [
        (dict(width=-1, dilate_radius=9), INVALID, NEG),
        (dict(threshold=-1, close_radius=9), INVALID, THRESHOLD),
        (dict(close_radius=9, max_blobs=65), INVALID, "a radius must be in 0..8"),
        (dict(max_blobs=65, min_area=-1), INVALID, "max_blobs must be in 0..64"),
        (dict(max_centre_dist=-1, frame_pitch=FRAME - 1), INVALID, "negative area or distance limit"),
        (dict(n_frames=3, frame_pitch=1 << 62, height=BIG), INVALID, OVERFLOW),
        (dict(n_frames=0, **TALL), UNSUPPORTED, LIMIT),
    ]
    return e, single, order, [dict(n_frames=0)]


def undistort():
    e = through_lens("sba_undistort_frames", "new_k", (5.0, 5.0, 3.0, 2.0))
    single, order = through_lens_rows()
    order = order + [(dict(new_k=None, interpolation=2), INVALID, NULL_LENS),
                     (dict(lens=dict(fx=NAN), new_k=(INF, 5.0, 3.0, 2.0)), INVALID, LENS_FINITE),
                     (dict(lens=dict(fx=0.0), new_k=(NAN, 5.0, 3.0, 2.0)), INVALID, NEWK_FINITE)]
    return e, SOURCE + LENS_ROWS + NEWK_ROWS + single, order, []


def warp():
    unit = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    e = through_lens("sba_warp_frames", "m", unit)
    single, order = through_lens_rows()
    model = [(dict(m=None), INVALID, "null m"),
             (dict(m=unit[:8] + (NAN,)), INVALID, "a value of m is not finite"),
             (dict(m=(INF,) + unit[1:]), INVALID, "a value of m is not finite")]
    order = order + [(dict(lens=dict(fx=0.0), m=None), INVALID, FOCAL),    # the lens, then the matrix, then the options
                     (dict(m=None, out_height=-1), INVALID, "null m"),
                     (dict(m=unit[:8] + (NAN,), border_value=-1), INVALID, "a value of m is not finite")]
    return e, SOURCE + LENS_ROWS + model + single, order, []


def accumulate():
    e = entry("sba_background_accumulate", dict(opts=None, use=None, sum=buf(4 * H * W), sumsq=buf(8 * H * W), hot=buf(4 * H * W),
                                                vmax=buf(H * W), n_used=buf(8)),
              _native.BgAccumulateOpts, dict(channel=1, threshold=50), early_return=False)
    many = "more than 2^24 frames in all (the bound under which the 32-bit sum cannot overflow)"
    full = np.array([(1 << 24) - 1], np.uint64)                           # one frame short of the bound
    single = SOURCE + [
        (dict(channel=3), INVALID, CHANNEL),
        (dict(threshold=256), INVALID, THRESHOLD),
        (dict(n_frames=(1 << 24) + 1), UNSUPPORTED, many),
        (dict(accumulate=1, n_used=full), UNSUPPORTED, many),
    ] + PITCHES + [(TALL, UNSUPPORTED, LIMIT)]
    order = [
        (dict(threshold=256, n_frames=(1 << 24) + 1), INVALID, THRESHOLD),
        (dict(n_frames=(1 << 24) + 1, row_pitch=ROW - 1), UNSUPPORTED, many),
        (dict(accumulate=1, n_used=full, **TALL), UNSUPPORTED, many),
        (dict(frame_pitch=FRAME - 1, height=BIG), INVALID, FRAME_PITCH),
    ]
    return e, single, order, []


def suppress():
    e = entry("sba_background_suppress", dict(level=np.zeros(H * W, np.uint8), mask=None, out_row_pitch=W, out_frame_pitch=H * W, opts=None,
                                              out=buf(N * H * W)),
              _native.BgSuppressOpts, dict(channel=1))
    e.buffers = [e.params["out"]]
    single = SOURCE + [
        (dict(channel=3), INVALID, CHANNEL),
        (dict(channel=-1), INVALID, CHANNEL),
        (dict(mode=2), INVALID, "mode must be 0 (gate) or 1 (subtract)"),
        (dict(mode=-1), INVALID, "mode must be 0 (gate) or 1 (subtract)"),
        (dict(out=None), INVALID, "null out"),
        (dict(out_row_pitch=W - 1), INVALID, "out_row_pitch is smaller than width"),
        (dict(out_frame_pitch=H * W - 1), INVALID, OUT_FRAME),
        (dict(n_frames=3, frame_pitch=FRAME, out_frame_pitch=1 << 62), INVALID, OUT_OVERFLOW),
    ] + PITCHES + [(dict(out_frame_pitch=BIG * W, **TALL), UNSUPPORTED, LIMIT)]
    order = [
        (dict(channel=3, mode=2), INVALID, CHANNEL),
        (dict(mode=2, out=None), INVALID, "mode must be 0 (gate) or 1 (subtract)"),
        (dict(out=None, out_row_pitch=W - 1), INVALID, "null out"),
        (dict(out_row_pitch=W - 1, row_pitch=ROW - 1), INVALID, "out_row_pitch is smaller than width"),
        (dict(out_frame_pitch=H * W - 1, row_pitch=ROW - 1), INVALID, OUT_FRAME),
        (dict(row_pitch=ROW - 1, out_frame_pitch=BIG * W, **TALL), INVALID, ROW_PITCH),
        (dict(n_frames=0, out=None, out_row_pitch=W - 1), INVALID, "out_row_pitch is smaller than width"),
    ]
    return e, single, order, [dict(n_frames=0), dict(n_frames=0, out=None)]


def convert():
    p = planes()
    params = dict(device=0, y=p["y"], u=p["u"], v=p["v"], n_frames=N, height=H, width=W, y_row_pitch=W, y_frame_pitch=H * W,
                  c_row_pitch=W // 2, c_frame_pitch=(H // 2) * (W // 2), c_step=1, matrix=None, out_row_pitch=ROW, out_frame_pitch=FRAME,
                  opts=None, out=buf(N * FRAME))
    e = Entry("sba_convert_frames", params, _native.ConvertOpts, dict(), structs=dict(matrix=_native.YuvMatrix))
    e.buffers = [params["out"]]
    bt601 = dict(zip(("y_offset", "cy", "cvr", "cug", "cvg", "cub"), _native.YUV_BT601))
    sums = "matrix: 255 |cy| + 128 (|a| + |b|) + 2^19 must stay below 2^31 for every output row"
    row = "out_row_pitch is smaller than width * bytes of a pixel"
    tall = dict(height=BIG, y_frame_pitch=BIG * W, c_frame_pitch=(BIG + 1) // 2 * (W // 2), out_frame_pitch=BIG * ROW)
    single = [
        (dict(n_frames=-1), INVALID, NEG),
        (dict(height=-1), INVALID, NEG),
        (dict(width=-1), INVALID, NEG),
        (dict(out=None), INVALID, "null out"),
        (dict(out_format=-1), INVALID, "unknown out_format"),
        (dict(out_format=7), INVALID, "unknown out_format"),
        (dict(matrix=dict(bt601, y_offset=256)), INVALID, Y_OFFSET),
        (dict(matrix=dict(bt601, y_offset=-1)), INVALID, Y_OFFSET),
        (dict(matrix=dict(bt601, cy=1 << 23)), INVALID, sums),
        (dict(matrix=dict(bt601, cub=-(1 << 24))), INVALID, sums),
    ] + plane_rows(None, "") + [
        (dict(out_row_pitch=ROW - 1), INVALID, row),
        (dict(out_format=2, out_row_pitch=4 * W - 1), INVALID, row),
        (dict(out_frame_pitch=FRAME - 1), INVALID, OUT_FRAME),
        (dict(n_frames=3, out_frame_pitch=1 << 62), INVALID, PLANE_OVERFLOW),
        (tall, UNSUPPORTED, LIMIT),
    ]
    order = [
        (dict(width=-1, out=None), INVALID, NEG),
        (dict(out=None, out_format=7), INVALID, "null out"),
        (dict(out_format=7, matrix=dict(bt601, y_offset=256)), INVALID, "unknown out_format"),
        (dict(matrix=dict(bt601, y_offset=256, cy=1 << 23)), INVALID, Y_OFFSET),
        (dict(matrix=dict(bt601, cy=1 << 23), y=None), INVALID, sums),
        (dict(c_step=3, out_row_pitch=ROW - 1), INVALID, C_STEP),
        (dict(out_row_pitch=ROW - 1, height=BIG, y_frame_pitch=BIG * W, c_frame_pitch=(BIG + 1) // 2 * (W // 2)), INVALID, row),
        (dict(n_frames=0, out=None, out_format=7), INVALID, "unknown out_format"),
        (dict(tall, n_frames=0), UNSUPPORTED, LIMIT),
    ]
    return e, single, order, [dict(n_frames=0), dict(n_frames=0, y=None, u=None, v=None, out=None)]


def resize():
    e = entry("sba_resize_frames", dict(fx=2, fy=2, out_row_pitch=W // 2 * CH, out_frame_pitch=H // 2 * (W // 2) * CH, opts=None,
                                        out=buf(N * (H // 2) * (W // 2) * CH)),
              _native.ResizeOpts, dict())
    factor = "fx and fy must be in 1..16"
    empty = "a factor is larger than the frame: the output would have no pixels"
    row = "out_row_pitch is smaller than (width / fx) times the bytes of an output pixel"
    rows = "out_frame_pitch is smaller than (height / fy) * out_row_pitch"
    single = SOURCE + [
        (dict(fx=0), INVALID, factor),
        (dict(fx=17), INVALID, factor),
        (dict(fy=0), INVALID, factor),
        (dict(fy=17), INVALID, factor),
        (dict(fx=7), INVALID, empty),
        (dict(fy=5), INVALID, empty),
        (dict(gray=1, channels=1, row_pitch=W, frame_pitch=H * W), INVALID, "gray needs 3 or 4 channels"),
    ] + [(dict(d, gray=1), rc, text) for d, rc, text in GRAY_W] + [
        (dict(out=None), INVALID, "null out"),
        (dict(out_row_pitch=W // 2 * CH - 1), INVALID, row),
        (dict(gray=1, out_row_pitch=W // 2 - 1), INVALID, row),
        (dict(out_frame_pitch=H // 2 * (W // 2) * CH - 1), INVALID, rows),
        (dict(n_frames=3, frame_pitch=FRAME, out_frame_pitch=1 << 62), INVALID, OUT_OVERFLOW),
    ] + PITCHES + [(dict(out_frame_pitch=BIG // 2 * (W // 2) * CH, **TALL), UNSUPPORTED, LIMIT)]
    order = [
        (dict(channels=2, fx=0), INVALID, CHANNELS),
        (dict(fx=0, fy=5), INVALID, factor),
        (dict(fy=5, gray=1, gray_w=(1, 2, 3)), INVALID, empty),
        (dict(gray=1, gray_w=(-1, 2, 3)), INVALID, GRAY_NEG),
        (dict(gray=1, gray_w=(1, 2, 3), out=None), INVALID, GRAY_SUM),
        (dict(gray_w=(1, 2, 3), out=None), INVALID, "null out"),           # the weights are not looked at without gray
        (dict(out=None, out_row_pitch=0), INVALID, "null out"),
        (dict(out_row_pitch=0, row_pitch=ROW - 1), INVALID, row),
        (dict(frame_pitch=FRAME - 1, height=BIG, out_frame_pitch=BIG // 2 * (W // 2) * CH), INVALID, FRAME_PITCH),
        (dict(n_frames=0, fx=7, out=None, out_row_pitch=-1), INVALID, row),     # no frames: only the pitches are left
    ]
    return e, single, order, [dict(n_frames=0), dict(n_frames=0, fx=16, fy=16, out=None, out_row_pitch=0, out_frame_pitch=0)]


def to_yuv():
    p = planes()
    e = entry("sba_frames_to_yuv", dict(y=p["y"], u=p["u"], v=p["v"], y_row_pitch=W, y_frame_pitch=H * W, c_row_pitch=W // 2,
                                        c_frame_pitch=(H // 2) * (W // 2), c_step=1, matrix=None, opts=None),
              _native.ToYuvOpts, dict(), structs=dict(matrix=_native.RgbMatrix))
    bt601 = dict(zip(("y_offset", "cry", "cgy", "cby", "cru", "cgu", "cbu", "crv", "cgv", "cbv"), _native.RGB_BT601))
    fmt = "in_format must be BGR, RGB, BGRA or RGBA"
    fits = "in_format does not have `channels` bytes per pixel"
    chroma = "chroma must be 0 (nearest) or 1 (average)"
    sums = "matrix: 255 (|a| + |b| + |c|) must stay below 2^28 for every row"
    tall = dict(TALL, y_frame_pitch=BIG * W, c_frame_pitch=(BIG + 1) // 2 * (W // 2))
    single = SOURCE + [
        (dict(in_format=-1), INVALID, fmt),
        (dict(in_format=4), INVALID, fmt),
        (dict(in_format=2), INVALID, fits),
        (dict(in_format=0, channels=4, row_pitch=4 * W, frame_pitch=4 * W * H), INVALID, fits),
        (dict(chroma=2), INVALID, chroma),
        (dict(chroma=-1), INVALID, chroma),
        (dict(matrix=dict(bt601, y_offset=256)), INVALID, Y_OFFSET),
        (dict(matrix=dict(bt601, cry=1 << 21)), INVALID, sums),
        (dict(matrix=dict(bt601, cbv=-(1 << 21))), INVALID, sums),
    ] + plane_rows(None, "") + PITCHES + [(tall, UNSUPPORTED, LIMIT)]
    order = [
        (dict(frames=None, in_format=4), INVALID, NULL_FRAMES),
        (dict(in_format=4, chroma=2), INVALID, fmt),
        (dict(in_format=2, chroma=2), INVALID, fits),
        (dict(chroma=2, matrix=dict(bt601, y_offset=-1)), INVALID, chroma),
        (dict(matrix=dict(bt601, cgu=1 << 21), c_step=0), INVALID, sums),
        (dict(y_row_pitch=W - 1, row_pitch=ROW - 1), INVALID, Y_ROW),      # the planes written, then the frames read
        (dict(row_pitch=ROW - 1, **tall), INVALID, ROW_PITCH),
        (dict(tall, n_frames=0), UNSUPPORTED, LIMIT),
    ]
    return e, single, order, [dict(n_frames=0), dict(n_frames=0, frames=None, y=None, u=None, v=None)]


def undistort_yuv():
    params = dict(device=0, src=planes(), n_frames=N, height=H, width=W, lens=dict(LENS), new_k=(5.0, 5.0, 3.0, 2.0), out_height=H,
                  out_width=W, out=planes(), opts=None, flags_out=buf(H * W), map_out=buf(8 * H * W))
    e = Entry("sba_undistort_yuv", params, _native.UndistortYuvOpts, dict(border_u=128, border_v=128),
              structs=dict(src=_native.YuvPlanes, out=_native.YuvPlanes, lens=_native.LensStruct), early_return=False)
    border = "border_y, border_u and border_v must be in 0..255"
    tall = dict(height=BIG, src=dict(y_frame_pitch=BIG * W, c_frame_pitch=(BIG + 1) // 2 * (W // 2)))
    single = [
        (dict(n_frames=-1), INVALID, NEG),
        (dict(height=-1), INVALID, NEG),
        (dict(width=-1), INVALID, NEG),
        (dict(src=None), INVALID, "null src"),
    ] + plane_rows("src", "src: ") + LENS_ROWS + NEWK_ROWS + RESAMPLE + [
        (dict(border_y=256), INVALID, border),
        (dict(border_u=-1), INVALID, border),
        (dict(border_v=256), INVALID, border),
        (dict(out=None, flags_out=None, map_out=None), INVALID, NO_OUT),
    ] + plane_rows("out", "out: ", "out_width") + [(tall, UNSUPPORTED, LIMIT)]
    order = [
        (dict(n_frames=-1, src=None), INVALID, NEG),
        (dict(src=dict(c_step=3), lens=None), INVALID, "src: " + C_STEP),
        (dict(new_k=None, out_width=BIG), INVALID, NULL_LENS),
        (dict(out_width=BIG, interpolation=2), INVALID, OUT_SIZE),
        (dict(interpolation=2, border_y=-1), INVALID, INTERP),
        (dict(border_v=256, out=dict(c_step=3)), INVALID, border),
        (dict(out=None, flags_out=None, map_out=None, **tall), INVALID, NO_OUT),
        (dict(out=dict(y_row_pitch=W - 1), **tall), INVALID, "out: " + Y_ROW),
        (dict(out=None, **tall), UNSUPPORTED, LIMIT),                     # no out: only the limit is left
        (dict(out=dict(y=None), n_frames=0, **tall), UNSUPPORTED, LIMIT),  # without frames a null plane is no fault
    ]
    return e, single, order, []


def hist():
    e = entry("sba_frame_histograms", dict(opts=None, hist=buf(4 * 256 * N), total=buf(8 * 256)), _native.HistOpts, dict(channel=1))
    why = LIMIT + " (the bound under which a count fits 32 bits)"
    single = SOURCE + [(dict(channel=3), INVALID, CHANNEL), (dict(channel=-1), INVALID, CHANNEL)] + PITCHES + [(TALL, UNSUPPORTED, why)]
    order = [
        (dict(channels=2, row_pitch=0), INVALID, CHANNELS),
        (dict(channel=3, row_pitch=ROW - 1), INVALID, CHANNEL),
        (dict(hist=None, total=None, row_pitch=ROW - 1), INVALID, ROW_PITCH),     # nothing asked for, and still checked
        (dict(hist=None, total=None, **TALL), UNSUPPORTED, why),
        (dict(n_frames=3, frame_pitch=1 << 62, height=BIG), INVALID, OVERFLOW),
    ]
    return e, single, order, [dict(n_frames=0), dict(hist=None, total=None), dict(n_frames=0, frames=None, hist=None, total=None)]


def corners():
    win = 7 * 7
    e = entry("sba_refine_corners", dict(corner_start=(0, 1, 2), corners=(2.0, 2.0, 3.0, 1.0), opts=None, weights=None, refined=buf(32),
                                         status=buf(8), iterations=buf(8), tensor=buf(48)),
              _native.CornerOpts, dict(eps=1e-5, channel=-1, win_x=3, win_y=3, zero_x=-1, zero_y=-1, max_iter=200))
    windows, iters = "win_x and win_y must be in 1..15", "max_iter must be in 1..10000"
    weight, null = "a weight is negative or not finite", "null corners, refined or status"
    single = SOURCE + [
        (dict(channel=3), INVALID, CHANNEL),
        (dict(channel=-2), INVALID, CHANNEL),
        (dict(channels=1, row_pitch=W, frame_pitch=H * W), INVALID, GRAY_ONE),
    ] + GRAY_W + [
        (dict(win_x=0), INVALID, windows),
        (dict(win_x=16), INVALID, windows),
        (dict(win_y=0), INVALID, windows),
        (dict(win_y=16), INVALID, windows),
        (dict(max_iter=0), INVALID, iters),
        (dict(max_iter=10001), INVALID, iters),
        (dict(eps=-1.0), INVALID, "eps must be >= 0"),
        (dict(eps=NAN), INVALID, "eps must be >= 0"),
        (dict(corner_start=None), INVALID, "null corner_start"),
        (dict(corner_start=(1, 1, 2)), INVALID, "corner_start[0] must be 0"),
        (dict(corner_start=(0, 2, 1)), INVALID, "corner_start must not decrease"),
        (dict(weights=(1.0,) * (win - 1) + (-1.0,)), INVALID, weight),
        (dict(weights=(NAN,) + (1.0,) * (win - 1)), INVALID, weight),
        (dict(corners=None), INVALID, null),
        (dict(refined=None), INVALID, null),
        (dict(status=None), INVALID, null),
        (dict(height=0), INVALID, "corners in frames without pixels"),
        (dict(width=0), INVALID, "corners in frames without pixels"),
    ] + PITCHES + [(TALL, UNSUPPORTED, LIMIT)]
    order = [
        (dict(channel=3, gray_w=(1, 2, 3)), INVALID, CHANNEL),
        (dict(channel=1, gray_w=(1, 2, 3), win_x=0), INVALID, windows),    # the weights are not looked at with a channel
        (dict(gray_w=(1, 2, 3), win_x=0), INVALID, GRAY_SUM),
        (dict(win_y=16, max_iter=0), INVALID, windows),
        (dict(max_iter=0, eps=-1.0), INVALID, iters),
        (dict(eps=-1.0, corner_start=None), INVALID, "eps must be >= 0"),
        (dict(corner_start=(0, 2, 1), weights=(-1.0,) * win), INVALID, "corner_start must not decrease"),
        (dict(weights=(-1.0,) * win, corners=None), INVALID, weight),
        (dict(corners=None, height=0), INVALID, null),
        (dict(width=0, row_pitch=-1), INVALID, "corners in frames without pixels"),
        (dict(status=None, row_pitch=ROW - 1), INVALID, null),
        (dict(corner_start=(0, 0, 0), corners=None, row_pitch=ROW - 1), INVALID, ROW_PITCH),     # no corners, and still checked
        (dict(n_frames=0, corner_start=None, **TALL), UNSUPPORTED, LIMIT),
    ]
    early = [dict(n_frames=0), dict(n_frames=0, corner_start=None), dict(corner_start=(0, 0, 0)),
             dict(corner_start=(0, 0, 0), corners=None, refined=None, status=None, height=0, frame_pitch=0)]
    return e, single, order, early


def adaptive():
    e = entry("sba_adaptive_threshold", dict(opts=None, out_row_pitch=W, out_frame_pitch=H * W, out_window_pitch=N * H * W,
                                             out=buf(2 * N * H * W), mean_out=buf(2 * N * H * W)),
              _native.AdaptiveOpts, dict(n_windows=2, block=(3, 5, 0, 0), delta=(7, 7, 0, 0), invert=1, channel=-1))
    windows, block, delta = "n_windows must be in 1..4", "a block must be odd and in 3..127", "a delta must be in -256..256"
    window = "out_window_pitch is smaller than n_frames * out_frame_pitch"
    tall = dict(TALL, out_frame_pitch=BIG * W, out_window_pitch=N * BIG * W)
    single = SOURCE + [
        (dict(channel=3), INVALID, CHANNEL),
        (dict(channel=-2), INVALID, CHANNEL),
        (dict(n_windows=0), INVALID, windows),
        (dict(n_windows=5), INVALID, windows),
        (dict(block=(3, 4, 0, 0)), INVALID, block),
        (dict(block=(1, 5, 0, 0)), INVALID, block),
        (dict(block=(3, 129, 0, 0)), INVALID, block),
        (dict(delta=(7, 257, 0, 0)), INVALID, delta),
        (dict(delta=(-257, 0, 0, 0)), INVALID, delta),
        (dict(invert=2), INVALID, "invert must be 0 (binary) or 1 (binary, inverted)"),
        (dict(max_value=256), INVALID, "max_value must be in 0..255"),
        (dict(max_value=-1), INVALID, "max_value must be in 0..255"),
        (dict(channels=1, row_pitch=W, frame_pitch=H * W), INVALID, GRAY_ONE),
    ] + GRAY_W + [
        (dict(out_row_pitch=W - 1), INVALID, "out_row_pitch is smaller than width"),
        (dict(out_frame_pitch=H * W - 1), INVALID, OUT_FRAME),
        (dict(n_frames=3, frame_pitch=FRAME, out_frame_pitch=1 << 62), INVALID, OUT_OVERFLOW),
        (dict(out_window_pitch=N * H * W - 1), INVALID, window),
        (dict(out_window_pitch=1 << 62), INVALID, "n_windows * out_window_pitch overflows"),
        (dict(out=None, mean_out=None), INVALID, "null out and null mean_out"),
    ] + [(dict(d, out_window_pitch=3 * H * W), rc, text) for d, rc, text in PITCHES] + [(tall, UNSUPPORTED, LIMIT)]
    order = [
        (dict(channel=3, n_windows=0), INVALID, CHANNEL),
        (dict(n_windows=5, block=(4, 4, 4, 4)), INVALID, windows),
        (dict(block=(3, 4, 0, 0), delta=(300, 0, 0, 0)), INVALID, delta),   # window by window: the first one's delta comes first
        (dict(delta=(7, 300, 0, 0), invert=2), INVALID, delta),
        (dict(invert=2, max_value=256), INVALID, "invert must be 0 (binary) or 1 (binary, inverted)"),
        (dict(max_value=256, gray_w=(1, 2, 3)), INVALID, "max_value must be in 0..255"),
        (dict(gray_w=(1, 2, 3), out_row_pitch=W - 1), INVALID, GRAY_SUM),
        (dict(out_frame_pitch=H * W - 1, out_window_pitch=0), INVALID, OUT_FRAME),
        (dict(out_window_pitch=0, out=None, mean_out=None), INVALID, window),
        (dict(n_windows=1, out_window_pitch=0, out=None, mean_out=None), INVALID, "null out and null mean_out"),   # one window: no window pitch
        (dict(out=None, mean_out=None, row_pitch=ROW - 1), INVALID, "null out and null mean_out"),
        (dict(row_pitch=ROW - 1, **tall), INVALID, ROW_PITCH),
    ]
    return e, single, order, [dict(n_frames=0), dict(n_frames=0, frames=None, out=None, mean_out=None)]


ENTRIES = [dots, blobs, undistort, warp, accumulate, suppress, convert, resize, to_yuv, undistort_yuv, hist, corners, adaptive]
IDS = [f.__name__ for f in ENTRIES]


def check_rows(lib, e, rows):
    assert rows
    for changes, status, sentence in rows:
        rc, text = e.call(lib, **changes)
        assert (rc, text) == (status, e.name + ": " + sentence), (e.name, changes, rc, text)
        assert e.untouched(), (e.name, changes)


@pytest.mark.parametrize("make", ENTRIES, ids=IDS)
def test_every_single_fault_has_its_status_and_sentence_and_touches_no_output(lib, make):
    e, single, _order, _early = make()
    check_rows(lib, e, single)


@pytest.mark.parametrize("make", ENTRIES, ids=IDS)
def test_of_two_faults_the_one_checked_first_is_reported(lib, make):
    e, _single, order, _early = make()
    check_rows(lib, e, order)


@pytest.mark.parametrize("make", ENTRIES, ids=IDS)
def test_calls_with_nothing_to_do(lib, make):
    """An entry point that returns before any work on the device when there is nothing to do still asks for the device first:
    with one the call is SBA_OK and writes nothing, without one it is SBA_ERR_NO_DEVICE.  sba_undistort_frames, sba_warp_frames,
    sba_background_accumulate and sba_undistort_yuv have no such return: an empty batch goes to the device like any other, so
    with a GPU it is left to their GPU suites."""
    e, _single, _order, early = make()
    gpu = lib.sba_device_count() > 0
    assert bool(early) == e.early_return
    if not e.early_return:
        if gpu:
            return                                                        # an empty batch runs on the device: the GPU suite has it
        early = [dict(n_frames=0)]
    for changes in early:
        rc, text = e.call(lib, **changes)
        if gpu:
            assert rc == 0, (e.name, changes, rc, text)
        else:
            assert rc == NO_DEVICE and text.startswith("no HIP device"), (e.name, changes, rc, text)
        assert e.untouched(), (e.name, changes)


@pytest.mark.parametrize("make", ENTRIES, ids=IDS)
def test_a_valid_call_passes_every_check_and_fails_loudly_without_a_gpu(lib, make):
    if lib.sba_device_count() > 0:
        return                                                            # with a GPU the entry point's tests/test_gpu_*.py take over
    e, _single, _order, _early = make()
    for changes in [dict(), dict(opts=None)]:                              # with options, and with the defaults of a NULL opts
        if changes and e.name == "sba_adaptive_threshold":
            changes = dict(changes, out_window_pitch=N * H * W, out=buf(3 * N * H * W), mean_out=None)      # its default is three windows
        rc, text = e.call(lib, **changes)
        assert rc == NO_DEVICE and text.startswith("no HIP device"), (e.name, rc, text)
        assert e.untouched()
