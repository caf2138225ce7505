"""Taking the lens out of the pictures: what a finished calibration is used for (``scripts/charuco_intrinsics.py:163-184`` of
the reference: ``cv.getOptimalNewCameraMatrix``, ``cv.undistort``, ``probe_monotonicity``), on sba_undistort_frames
(include/sba_hip.h).

* :class:`Lens`                        -- OpenCV's 5-coefficient model (fx, fy, cx, cy, k1, k2, p1, p2, k3), from a camera row of
  the bundle adjustment or from a camera matrix and distortion coefficients
* :func:`undistort_frames`             -- ``cv.undistort`` for a whole batch of frames of one camera, on the GPU
* :func:`warp_frames`, :func:`plane_view`, :class:`PlaneGrid`, :func:`virtual_camera_matrix`, :func:`plane_mosaic` -- the
  extrinsics put to use on the pictures (sba_warp_frames): the metric top-down view of the floor or of a laser plane through
  every calibrated camera, rotated virtual cameras (rectification, levelling), and the views of a rig in one picture
* :func:`optimal_new_camera_matrix`    -- ``cv.getOptimalNewCameraMatrix``: the camera matrix that keeps only valid pixels
  (alpha = 0), every source pixel (alpha = 1) or a blend; 81 points, on the host
* :func:`invertible_region`            -- where the distortion model is locally invertible (the FOLDED flag), as a bool image
* :class:`BackgroundModel`             -- what every pixel of a camera shows over a video (sba_background_accumulate) and the
  removal of the light that is always there (sba_background_suppress), for rigs that cannot be made dark
* :func:`convert_frames`, :class:`YuvMatrix` -- a decoder's YUV 4:2:0 frames (NV12, NV21, I420, YV12) into BGR / RGB frames or the
  one plane the detectors read (sba_convert_frames): ``cv.cvtColor(frame, cv.COLOR_YUV2BGR_NV12)`` for a batch, on the GPU
* :func:`frames_to_yuv`, :class:`RgbMatrix` -- the way back: BGR / RGB frames or one plane into the YUV 4:2:0 an encoder takes
  (sba_frames_to_yuv): ``cv.cvtColor(frame, cv.COLOR_BGR2YUV_I420)`` for a batch, on the GPU; ``undistort_frames`` can hand its
  result over in that form (``out_pixel_format``), so that 1.5 bytes per pixel leave the device instead of 3
* :func:`undistort_yuv`                -- the lens taken out of a video plane by plane: decoder YUV 4:2:0 in, encoder YUV 4:2:0
  out, in one call and without a colour matrix (sba_undistort_yuv)
* :func:`resize_frames`, :func:`mosaic` -- previews: ``cv2.resize(frame, size, interpolation=cv2.INTER_AREA)`` at an integer factor
  and ``cv2.cvtColor(frame, cv2.COLOR_BGR2GRAY)`` for a batch (sba_resize_frames), and the cameras of a rig side by side in one canvas
* :func:`frame_histograms`, :class:`FrameHistograms` -- the 256-bin histogram of the detectors' channel of every frame
  (sba_frame_histograms) and what follows from it: the pixels above every threshold at once, saturation, the dark level, Otsu's
  threshold, and the threshold that leaves a dot of a sane size in most frames -- what the reference finds by clicking pixels
  (``lasercalib/get_video_pixel.py``)
* :func:`refine_corners`, :func:`corner_sub_pix`, :class:`CornerRefinement`, :func:`corner_weights` -- ``cv.cornerSubPix`` for the
  marker corners of a batch of frames (sba_refine_corners; ``scripts/charuco_intrinsics.py:39-44``), with what OpenCV throws away:
  the window's structure tensor, which tells an edge from a corner and gives every corner a weight
* :func:`adaptive_threshold`, :func:`adaptive_threshold_cv`, :func:`marker_threshold_windows` -- ``cv.adaptiveThreshold`` with
  ``ADAPTIVE_THRESH_MEAN_C`` for a batch of frames and up to four window sizes at once (sba_adaptive_threshold): the first stage
  of ``cv2.aruco``'s ``detectMarkers`` (``scripts/run_viewers.py:72-77``), whose masks ``find_laser_blobs`` can label in place

Sizes are ``(width, height)``, as in OpenCV.  Pixels follow the rule written out in include/sba_hip.h: a float64 model, the
source position on a 1/32-pixel grid, integer bilinear weights.  That is OpenCV's scheme, but OpenCV rounds its weight table to
15 bits, so single bytes may differ from ``cv.undistort`` by a grey level.
"""
from __future__ import annotations

import numpy as np

from . import _native
from ._native import UNDIST_FOLDED, UNDIST_OUTSIDE, UNDIST_RANGE, WARP_BEHIND

SBA_UNDIST_OUTSIDE, SBA_UNDIST_FOLDED, SBA_UNDIST_RANGE = UNDIST_OUTSIDE, UNDIST_FOLDED, UNDIST_RANGE
SBA_WARP_BEHIND = WARP_BEHIND

__all__ = ["Lens", "undistort_frames", "undistort_yuv", "optimal_new_camera_matrix", "invertible_region", "BackgroundModel",
           "YuvMatrix", "convert_frames", "RgbMatrix", "frames_to_yuv", "resize_frames", "mosaic", "frame_histograms", "FrameHistograms", "SBA_UNDIST_OUTSIDE", "SBA_UNDIST_FOLDED", "SBA_UNDIST_RANGE",
           "warp_frames", "plane_view", "PlaneGrid", "virtual_camera_matrix", "plane_mosaic", "SBA_WARP_BEHIND",
           "refine_corners", "corner_sub_pix", "corner_window", "corner_weights", "CornerRefinement",
           "adaptive_threshold", "adaptive_threshold_cv", "marker_threshold_windows", "ADAPTIVE_THRESH_MEAN_C", "THRESH_BINARY",
           "THRESH_BINARY_INV"]


class Lens:
    """A pinhole camera with OpenCV's 5-coefficient distortion: focal lengths, principal point, radial k1, k2, k3 and tangential
    p1, p2.  Every value must be finite and the focal lengths positive."""

    __slots__ = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3")

    def __init__(self, fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
        vals = [float(v) for v in (fx, fy, cx, cy, k1, k2, p1, p2, k3)]
        if not all(np.isfinite(vals)):
            raise ValueError(f"Lens: every value must be finite, got {vals}")
        if not (vals[0] > 0 and vals[1] > 0):
            raise ValueError(f"Lens: the focal lengths must be > 0, got {vals[:2]}")
        for name, v in zip(self.__slots__, vals):
            setattr(self, name, v)

    @classmethod
    def from_camera_row(cls, row):
        """From a camera row of the bundle adjustment: 11 columns [rvec(3), t(3), f, k1, k2, cx, cy] or 13 columns
        [rvec(3), t(3), f, k1, k2, p1, p2, cx, cy]; fx = fy = f, k3 = 0."""
        r = np.asarray(row, dtype=np.float64).reshape(-1)
        if r.shape[0] == 11:
            return cls(r[6], r[6], r[9], r[10], r[7], r[8])
        if r.shape[0] == 13:
            return cls(r[6], r[6], r[11], r[12], r[7], r[8], r[9], r[10])
        raise ValueError(f"a camera row has 11 columns (radial model) or 13 (radial + tangential), not {r.shape[0]}")

    @classmethod
    def from_opencv(cls, camera_matrix, distortion_coefficients):
        """From OpenCV's 3 x 3 camera matrix and its distortion vector (k1, k2, p1, p2[, k3]).  Longer vectors (the rational and
        thin-prism models) are accepted only when their further coefficients are zero."""
        K = np.asarray(camera_matrix, dtype=np.float64)
        if K.shape != (3, 3):
            raise ValueError(f"camera_matrix must be 3 x 3, got {K.shape}")
        if K[0, 1] != 0 or K[1, 0] != 0 or K[2, 0] != 0 or K[2, 1] != 0 or K[2, 2] != 1:
            raise ValueError("camera_matrix must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]: skew is not supported")
        d = np.asarray(distortion_coefficients, dtype=np.float64).reshape(-1)
        if d.shape[0] < 4:
            raise ValueError(f"distortion_coefficients must hold (k1, k2, p1, p2[, k3]), got {d.shape[0]} values")
        if d.shape[0] > 5 and np.any(d[5:] != 0):
            raise ValueError("only the 5-coefficient model is supported: k4..k6 and the prism / tilt terms must be zero")
        return cls(K[0, 0], K[1, 1], K[0, 2], K[1, 2], d[0], d[1], d[2], d[3], d[4] if d.shape[0] > 4 else 0.0)

    def as_tuple(self):
        return tuple(getattr(self, n) for n in self.__slots__)

    @property
    def camera_matrix(self):
        return np.array([[self.fx, 0.0, self.cx], [0.0, self.fy, self.cy], [0.0, 0.0, 1.0]])

    @property
    def distortion_coefficients(self):
        """(k1, k2, p1, p2, k3), OpenCV's order."""
        return np.array([self.k1, self.k2, self.p1, self.p2, self.k3])

    def __repr__(self):
        return "Lens(" + ", ".join(f"{n}={getattr(self, n)!r}" for n in self.__slots__) + ")"

    # ---- the forward model on normalised coordinates, and its inverse (host, float64)
    def distort(self, x, y):
        """(xd, yd) and the Jacobian entries (j00, j01, j11) of the distortion at normalised (x, y); j10 = j01."""
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        x2, y2, xy = x * x, y * y, x * y
        r2 = x2 + y2
        rad = 1.0 + r2 * (self.k1 + r2 * (self.k2 + r2 * self.k3))
        dp = self.k1 + r2 * (2.0 * self.k2 + r2 * (3.0 * self.k3))
        xd = x * rad + (2.0 * self.p1 * xy + self.p2 * (r2 + 2.0 * x2))
        yd = y * rad + (self.p1 * (r2 + 2.0 * y2) + 2.0 * self.p2 * xy)
        j00 = rad + 2.0 * x2 * dp + (2.0 * self.p1 * y + 6.0 * self.p2 * x)
        j11 = rad + 2.0 * y2 * dp + (6.0 * self.p1 * y + 2.0 * self.p2 * x)
        j01 = 2.0 * xy * dp + (2.0 * self.p1 * x + 2.0 * self.p2 * y)
        return xd, yd, j00, j01, j11

    def undistort_points(self, uv, steps=20):
        """Normalised undistorted coordinates (n, 2) of the pixels ``uv`` (n, 2): Newton steps on distort(x, y) = ((u - cx) / fx,
        (v - cy) / fy) from the distorted point, with the analytic Jacobian.  NaN where the Jacobian becomes singular."""
        uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
        xd, yd = (uv[:, 0] - self.cx) / self.fx, (uv[:, 1] - self.cy) / self.fy
        x, y = xd.copy(), yd.copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            for _ in range(steps):
                fx_, fy_, j00, j01, j11 = self.distort(x, y)
                ex, ey = fx_ - xd, fy_ - yd
                det = j00 * j11 - j01 * j01
                x, y = x - (j11 * ex - j01 * ey) / det, y - (j00 * ey - j01 * ex) / det
        return np.stack([x, y], axis=1)


def _lens(lens):
    if not isinstance(lens, Lens):
        raise ValueError("lens must be a Lens (Lens.from_camera_row, Lens.from_opencv)")
    return lens


def _new_k(lens, new_camera_matrix):
    """(fxn, fyn, cxn, cyn) from None (the lens's own matrix, as in cv.undistort), a 3 x 3 matrix or those four values."""
    if new_camera_matrix is None:
        return (lens.fx, lens.fy, lens.cx, lens.cy)
    K = np.asarray(new_camera_matrix, dtype=np.float64)
    if K.shape == (4,):
        k = tuple(float(v) for v in K)
    elif K.shape == (3, 3):
        if K[0, 1] != 0 or K[1, 0] != 0 or K[2, 0] != 0 or K[2, 1] != 0 or K[2, 2] != 1:
            raise ValueError("new_camera_matrix must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]]: skew and rectification are not supported")
        k = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))
    else:
        raise ValueError(f"new_camera_matrix must be None, 3 x 3 or (fx, fy, cx, cy), got shape {K.shape}")
    if not all(np.isfinite(k)) or not (k[0] > 0 and k[1] > 0):
        raise ValueError(f"new_camera_matrix: values must be finite and the focal lengths > 0, got {k}")
    return k


def _size(size, name):
    try:
        w, h = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be (width, height), got {size!r}") from None
    if not (0 <= w <= _native.DOT_MAX_DIM and 0 <= h <= _native.DOT_MAX_DIM):
        raise ValueError(f"{name} must be (width, height) within 0..{_native.DOT_MAX_DIM}, got {(w, h)}")
    return w, h


def undistort_frames(frames, lens, new_camera_matrix=None, out_size=None, interpolation="linear", border_value=0, out=None,
                     want_flags=False, want_map=False, chunk_frames=0, device=0, out_pixel_format=None, out_matrix="bt601",
                     out_chroma="nearest", in_format="bgr"):
    """``cv.undistort(frame, K, dist, None, new_camera_matrix)`` for every frame of a batch of one camera.

    ``frames``: uint8, (B, H, W, C) with C in (1, 3, 4) or (B, H, W); a numpy array in any layout with contiguous pixels, or a
    torch tensor on ``device``, read in place.  The result is a numpy array for numpy frames and a device tensor for tensor
    frames (allocated by torch, or ``out``: same kind, shape (B, height, width[, C]), any row and frame strides, whose padding is
    left untouched).  ``new_camera_matrix=None`` means the lens's own matrix; ``out_size=(width, height)`` defaults to the size
    of the frames.  ``interpolation`` is "linear" or "nearest"; ``border_value`` (0..255) fills what lies outside the source.
    With ``want_flags`` / ``want_map`` returns ``(frames, flags, map)``: ``flags`` (height, width) uint8 of SBA_UNDIST_OUTSIDE |
    FOLDED | RANGE, ``map`` (height, width, 2) int32, the source position in 1/32 pixels; whichever was not asked for is None.
    With an ``out_pixel_format`` ("nv12", "nv21", "i420", "yv12") the result is YUV 4:2:0 as :func:`frames_to_yuv` returns it,
    under ``out_matrix`` and ``out_chroma``, with ``in_format`` saying which channel of the frames is which: the frames are
    undistorted chunk by chunk (``chunk_frames`` frames; 0 = as many as ``CONVERT_CHUNK_BYTES`` of undistorted pixels hold) into
    device memory and each chunk is converted there, so only YUV leaves the device; ``out`` is then what ``frames_to_yuv``
    takes.  The bytes are those of ``frames_to_yuv(undistort_frames(frames, ...))``."""
    lens = _lens(lens)
    nk = _new_k(lens, new_camera_matrix)
    tensor, arr, B, H, W, Cn, _sr, _sf = _native._frame_layout(frames, device)
    w, h = (W, H) if out_size is None else _size(out_size, "out_size")
    if out_pixel_format is not None:
        pix = str(out_pixel_format).lower()
        if pix not in _native.YUV_FORMATS:
            raise ValueError(f"out_pixel_format must be one of {_native.YUV_FORMATS}, not {out_pixel_format!r}")
        m = _matrix(out_matrix, RgbMatrix)
        if out is None:
            out = _native.yuv_planes_alloc(pix, B, h, w, tensor, device)
        L = _native._yuv_layout(out, pix, device)
        if (L.n_frames, L.height, L.width) != (B, h, w):
            raise ValueError(f"out holds {L.n_frames} frames of {L.width} x {L.height}, the result is {B} of {w} x {h}")
        step = int(chunk_frames) if chunk_frames > 0 else max(1, CONVERT_CHUNK_BYTES // max(1, Cn * h * w))
        flags = qmap = None
        for lo in range(0, max(B, 1), step):                 # a batch without frames: one call, for the diagnostics
            hi = min(lo + step, B)
            bgr, fl, qm = _native.undistort_frames(arr[lo:hi], lens.as_tuple(), nk, (h, w), interpolation=interpolation,
                                                   border_value=border_value, want_flags=want_flags and lo == 0,
                                                   want_map=want_map and lo == 0, device=device, out_on_device=True)
            flags, qmap = (fl, qm) if lo == 0 else (flags, qmap)
            _native.frames_to_yuv(bgr, pix, in_format=in_format, matrix=m, chroma=out_chroma,
                                  out=_native.yuv_frame_slice(out, lo, hi), device=device)
        return (out, flags, qmap) if (want_flags or want_map) else out
    res, flags, qmap = _native.undistort_frames(frames, lens.as_tuple(), nk, (h, w), interpolation=interpolation, border_value=border_value,
                                                out=out, want_flags=want_flags, want_map=want_map, chunk_frames=chunk_frames, device=device)
    return (res, flags, qmap) if (want_flags or want_map) else res


def undistort_yuv(frames, pixel_format, lens, new_camera_matrix=None, out_size=None, interpolation="linear", border=(16, 128, 128),
                  out_pixel_format=None, out=None, want_flags=False, want_map=False, chunk_frames=0, device=0):
    """The lens taken out of a video without leaving its colour space: a decoder's 8-bit YUV 4:2:0 frames in, an encoder's out,
    resampled plane by plane in one call (sba_undistort_yuv, include/sba_hip.h), as ffmpeg's ``lenscorrection`` works.

    ``frames`` and ``pixel_format`` ("nv12", "nv21", "i420", "yv12") are what :func:`convert_frames` takes: a stacked array or a
    tuple of planes, numpy or tensors on ``device`` read in place.  The luma plane goes through the rule of
    :func:`undistort_frames` as a one-channel image; the chroma planes are half-size images under the same lens, their
    samples sited at the centres of their 2 x 2 blocks.  No colour matrix is applied and nothing is clipped: with
    ``new_camera_matrix=None`` and a lens without distortion the frames come back bit for bit.  ``out_size=(width, height)``
    defaults to the size of the frames; ``interpolation`` is "linear" or "nearest"; ``border`` = (Y, U, V), each 0..255 and
    taken literally, fills what lies outside the source (the default is limited-range black).  ``out_pixel_format=None``
    means the format of the input.  The result is what :func:`frames_to_yuv` returns -- numpy for numpy frames, tensors for
    tensors: the stacked array when width and height are even, else the tuple of planes -- or ``out``, which may be of either
    kind and of any strides :func:`convert_frames` reads; what lies between its samples is left untouched.  With
    ``want_flags`` / ``want_map`` returns ``(frames, flags, map)`` as :func:`undistort_frames` does, for the luma plane."""
    lens = _lens(lens)
    nk = _new_k(lens, new_camera_matrix)
    L = _native._yuv_layout(frames, pixel_format, device)
    w, h = (L.width, L.height) if out_size is None else _size(out_size, "out_size")
    res, flags, qmap = _native.undistort_yuv(frames, pixel_format, lens.as_tuple(), nk, (h, w), interpolation=interpolation, border=border,
                                             out_pixel_format=out_pixel_format, out=out, want_flags=want_flags, want_map=want_map,
                                             chunk_frames=chunk_frames, device=device)
    return (res, flags, qmap) if (want_flags or want_map) else res


def _matrix3(matrix, name="matrix"):
    m = np.asarray(matrix, dtype=np.float64)
    if m.shape != (3, 3) or not np.all(np.isfinite(m)):
        raise ValueError(f"{name} must be a finite 3 x 3 matrix, got shape {m.shape}")
    return m


def warp_frames(frames, lens, matrix, out_size, interpolation="linear", border_value=0, out=None, want_flags=False, want_map=False,
                chunk_frames=0, device=0):
    """The frames of one camera seen through a projective front end (sba_warp_frames, include/sba_hip.h): pixel (x, y) of the
    result is the normalised camera position ``matrix @ (x, y, 1)`` taken through ``lens``.  ``matrix`` (3 x 3) is defined up
    to a positive factor; a pixel whose third coordinate is not positive lies behind the camera and holds ``border_value``.
    :meth:`PlaneGrid.matrix` gives the matrix of a world plane, :func:`virtual_camera_matrix` that of a rotated pinhole camera.
    Everything else -- ``frames``, ``out_size`` = (width, height), ``interpolation``, ``border_value``, ``out``, ``want_flags``,
    ``want_map``, ``chunk_frames`` and what is returned -- is as for :func:`undistort_frames`; ``flags`` may also hold
    SBA_WARP_BEHIND."""
    lens = _lens(lens)
    m = _matrix3(matrix)
    w, h = _size(out_size, "out_size")
    res, flags, qmap = _native.warp_frames(frames, lens.as_tuple(), m, (h, w), interpolation=interpolation, border_value=border_value,
                                           out=out, want_flags=want_flags, want_map=want_map, chunk_frames=chunk_frames, device=device)
    return (res, flags, qmap) if (want_flags or want_map) else res


def rodrigues(rvec):
    """The rotation matrix of a rotation vector, in float64: R = cos I + sin [a]x + (1 - cos) a a^T with a = rvec / |rvec|; the
    identity for the zero vector.  The library's convention: X_cam = R X + t."""
    r = np.asarray(rvec, dtype=np.float64).reshape(-1)
    if r.shape != (3,) or not np.all(np.isfinite(r)):
        raise ValueError(f"a rotation vector has three finite values, got {r}")
    angle = np.linalg.norm(r)
    if angle == 0.0:
        return np.eye(3)
    a = r / angle
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.cos(angle) * np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * np.outer(a, a)


def _camera(camera):
    """(lens, R, t) of a camera row of the bundle adjustment (11 or 13 columns) or of a (Lens, R, t) triple."""
    if isinstance(camera, (tuple, list)) and len(camera) == 3 and isinstance(camera[0], Lens):
        lens, R, t = camera
        R, t = _matrix3(R, "R"), np.asarray(t, dtype=np.float64).reshape(-1)
        if t.shape != (3,) or not np.all(np.isfinite(t)):
            raise ValueError(f"t must hold three finite values, got {t}")
        return lens, R, t
    row = np.asarray(camera, dtype=np.float64).reshape(-1)
    lens = Lens.from_camera_row(row)
    return lens, rodrigues(row[:3]), row[3:6].copy()


class PlaneGrid:
    """A regular grid of points on a world plane, the pixels of a plane view: pixel (x, y) is the world point
    ``origin + x * u_step + y * v_step`` (mm, as the calibration's world), ``size`` = (width, height)."""

    def __init__(self, origin, u_step, v_step, size):
        vec = [np.asarray(v, dtype=np.float64).reshape(-1) for v in (origin, u_step, v_step)]
        if any(v.shape != (3,) or not np.all(np.isfinite(v)) for v in vec):
            raise ValueError("origin, u_step and v_step must each hold three finite values")
        self.origin, self.u_step, self.v_step = vec
        if not np.any(np.cross(self.u_step, self.v_step)):
            raise ValueError("u_step and v_step must span a plane")
        self.size = _size(size, "size")

    @classmethod
    def z_plane(cls, z, x_range, y_range, mm_per_pixel):
        """The plane z = ``z`` over x_range = (x0, x1) and y_range = (y0, y1), half open, at ``mm_per_pixel``: pixel (i, j) is
        (x0 + i mm, y0 + j mm, z) and there are ceil((x1 - x0) / mm) x ceil((y1 - y0) / mm) of them."""
        mm = float(mm_per_pixel)
        (x0, x1), (y0, y1) = (float(v) for v in x_range), (float(v) for v in y_range)
        if not (mm > 0 and x1 > x0 and y1 > y0 and np.isfinite([mm, x0, x1, y0, y1, float(z)]).all()):
            raise ValueError("mm_per_pixel must be > 0 and the ranges finite and ascending")
        w, h = int(np.ceil((x1 - x0) / mm)), int(np.ceil((y1 - y0) / mm))
        return cls((x0, y0, float(z)), (mm, 0.0, 0.0), (0.0, mm, 0.0), (w, h))

    def world_points(self):
        """(height, width, 3): the world point of every pixel."""
        w, h = self.size
        x, y = np.arange(w, dtype=np.float64)[None, :, None], np.arange(h, dtype=np.float64)[:, None, None]
        return self.origin + x * self.u_step + y * self.v_step

    def pixel_of(self, world_xyz):
        """(..., 2): the pixel (x, y), not rounded, of world points (..., 3); a point off the plane counts as its foot on it."""
        d = np.asarray(world_xyz, dtype=np.float64) - self.origin
        A = np.stack([self.u_step, self.v_step], axis=1)                     # 3 x 2
        return d @ np.linalg.pinv(A).T

    def matrix(self, camera):
        """The matrix of :func:`warp_frames` for this grid seen by ``camera`` (a camera row of 11 or 13 columns, or a
        ``(Lens, R, t)`` triple): ``[R u_step | R v_step | R origin + t]`` with X_cam = R X + t and Z > 0 in front."""
        _lens_, R, t = _camera(camera)
        return np.stack([R @ self.u_step, R @ self.v_step, R @ self.origin + t], axis=1)


def plane_view(frames, camera, grid, **kw):
    """The frames of a calibrated camera resampled onto the world plane of ``grid`` (a :class:`PlaneGrid`): a metric picture
    of the floor or of a laser plane, in which what lies on the plane lands on the same pixel from every camera.  ``camera``:
    a camera row of the bundle adjustment (11 or 13 columns) or a ``(Lens, R, t)`` triple with X_cam = R X + t, for cameras read
    from OpenCV yaml files (``rc_ext``, ``tc_ext``).  Keywords and result as :func:`warp_frames`."""
    if not isinstance(grid, PlaneGrid):
        raise ValueError("grid must be a PlaneGrid")
    lens, _R, _t = _camera(camera)
    return warp_frames(frames, lens, grid.matrix(camera), grid.size, **kw)


def virtual_camera_matrix(new_camera_matrix, rotation=None):
    """The matrix of :func:`warp_frames` for a virtual pinhole camera K_new at the place of the source camera, turned by
    ``rotation``: X_virtual = rotation @ X_source, the rectification matrix of ``cv.stereoRectify`` and
    ``cv.initUndistortRectifyMap`` -> ``rotation.T @ inv(K_new)``.  K_new = [[fx, s, cx], [0, fy, cy], [0, 0, 1]] may have skew; without a rotation the result is
    :func:`undistort_frames` restated (bit for bit when fx and fy are powers of two)."""
    K = _matrix3(new_camera_matrix, "new_camera_matrix")
    if K[1, 0] != 0 or K[2, 0] != 0 or K[2, 1] != 0 or K[2, 2] != 1 or not (K[0, 0] > 0 and K[1, 1] > 0):
        raise ValueError("new_camera_matrix must be [[fx, s, cx], [0, fy, cy], [0, 0, 1]] with fx, fy > 0")
    a, b, s, cx, cy = 1.0 / K[0, 0], 1.0 / K[1, 1], K[0, 1], K[0, 2], K[1, 2]
    inv = np.array([[a, -s * a * b, (s * cy * b - cx) * a], [0.0, b, -cy * b], [0.0, 0.0, 1.0]])
    if rotation is None:
        return inv
    R = _matrix3(rotation, "rotation")
    if np.max(np.abs(R @ R.T - np.eye(3))) > 1e-9 or np.linalg.det(R) < 0:
        raise ValueError("rotation must be a rotation matrix")
    return R.T @ inv


def plane_mosaic(views, flags, maps, source_sizes, fill=0):
    """The plane views of the cameras of a rig in one picture -> ``(mosaic, owner)``.

    ``views``: one batch per camera, (B, height, width[, C]) of one shape, numpy arrays or device tensors; ``flags`` and
    ``maps``: what the calls returned with ``want_flags`` and ``want_map``; ``source_sizes``: (width, height) of every camera's
    frames.  The owner of a pixel is the camera with flags == 0 there whose source position lies farthest from the edge of its
    own image -- the integer ``min(qx, 32 (W - 1) - qx, qy, 32 (H - 1) - qy)`` of its map entry --, the lowest index on ties;
    a pixel nobody owns holds ``fill`` and owner -1.  ``owner`` is (height, width) int32, of the kind of the views.  Nothing is
    blended: a pixel of the mosaic is a pixel of one view."""
    n = len(views)
    if n == 0 or not (len(flags) == len(maps) == len(source_sizes) == n):
        raise ValueError("views, flags, maps and source_sizes must hold one entry per camera, at least one")
    fill = int(fill)
    if not 0 <= fill <= 255:
        raise ValueError(f"fill must be in 0..255, got {fill}")
    shape = tuple(views[0].shape)
    tensor = _native._is_tensor(views[0])
    if len(shape) not in (3, 4) or any(tuple(v.shape) != shape or _native._is_tensor(v) != tensor for v in views):
        raise ValueError("every view must be (B, height, width[, C]) of one shape and kind")
    hw = shape[1:3]
    best = np.full(hw, np.iinfo(np.int64).min, np.int64)
    owner = np.full(hw, -1, np.int32)
    for k in range(n):
        fl, qm = (a.cpu().numpy() if _native._is_tensor(a) else np.asarray(a) for a in (flags[k], maps[k]))
        W, H = _size(source_sizes[k], "source_sizes")
        if fl.shape != hw or qm.shape != hw + (2,):
            raise ValueError(f"camera {k}: flags {fl.shape} and map {qm.shape} do not fit views of {hw}")
        qx, qy = qm[..., 0].astype(np.int64), qm[..., 1].astype(np.int64)
        score = np.minimum(np.minimum(qx, 32 * (W - 1) - qx), np.minimum(qy, 32 * (H - 1) - qy))
        take = (fl == 0) & ((owner < 0) | (score > best))                   # strictly farther: ties stay with the lower index
        best[take], owner[take] = score[take], k
    if tensor:
        import torch
        own = torch.from_numpy(owner).to(views[0].device)
        mask = own.reshape((1,) + hw + (1,) * (len(shape) - 3))
        mosaic = torch.full(shape, fill, dtype=views[0].dtype, device=views[0].device)
        for k in range(n):
            mosaic = torch.where(mask == k, views[k], mosaic)
        return mosaic, own
    mosaic = np.full(shape, fill, views[0].dtype)
    for k in range(n):
        mosaic[:, owner == k] = np.asarray(views[k])[:, owner == k]
    return mosaic, owner


def invertible_region(lens, new_camera_matrix, size, device=0):
    """A (height, width) bool image of the destination pixels at which the distortion model is locally invertible (the Jacobian
    determinant of the distortion is positive: the FOLDED flag of a call without frames is clear).  Like the reference's
    ``probe_monotonicity`` this is a pointwise test: behind a second turning point of the polynomial it passes again."""
    lens = _lens(lens)
    w, h = _size(size, "size")
    _o, flags, _m = _native.undistort_frames(np.zeros((0, 1, 1, 1), np.uint8), lens.as_tuple(), _new_k(lens, new_camera_matrix), (h, w),
                                             want_flags=True, want_frames=False, device=device)
    return (flags & UNDIST_FOLDED) == 0


def optimal_new_camera_matrix(lens, image_size, alpha, new_size=None):
    """``cv.getOptimalNewCameraMatrix(K, dist, image_size, alpha, new_size)`` -> ``(K_new, roi)``.

    A 9 x 9 grid of source pixels spanning the image (corners included) is undistorted to normalised coordinates.  The INNER
    rectangle is the largest axis-parallel one the grid shows to lie inside the undistorted image: bounded by the largest x of
    the left column, the smallest x of the right column, the largest y of the top row and the smallest y of the bottom row.  The
    OUTER rectangle is the bounding box of all 81 points.  A rectangle (x0, y0, x1, y1) gives the camera matrix that maps it onto
    the pixel centres of the new image: fx = (width - 1) / (x1 - x0), cx = -fx x0, and likewise in y.  ``alpha`` in [0, 1] blends
    the inner matrix (0: only valid pixels, some source pixels are lost) into the outer one (1: every source pixel is kept,
    with border between them).  ``roi`` = (x, y, width, height) is the inner rectangle in pixels of the new image, rounded inwards
    (a value within 1e-9 of a whole pixel counts as that pixel) and clipped to it: the region where all pixels are valid.  As in OpenCV, the rectangles come from 9 samples per edge: an
    extremum of an edge between two samples is missed by a fraction of a pixel."""
    lens = _lens(lens)
    w, h = _size(image_size, "image_size")
    nw, nh = (w, h) if new_size is None else _size(new_size, "new_size")
    if min(w, h, nw, nh) < 2:
        raise ValueError("image_size and new_size must be at least 2 x 2")
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"alpha must be in [0, 1], got {alpha}")
    n = 9
    gx, gy = np.meshgrid(np.arange(n) * (w - 1) / (n - 1), np.arange(n) * (h - 1) / (n - 1))      # [row j][column i]
    pts = lens.undistort_points(np.stack([gx.ravel(), gy.ravel()], axis=1)).reshape(n, n, 2)
    if not np.all(np.isfinite(pts)):
        raise ValueError("the distortion cannot be inverted over the whole image: the model folds inside it")
    inner = (pts[:, 0, 0].max(), pts[0, :, 1].max(), pts[:, -1, 0].min(), pts[-1, :, 1].min())
    outer = (pts[..., 0].min(), pts[..., 1].min(), pts[..., 0].max(), pts[..., 1].max())
    if not (inner[2] > inner[0] and inner[3] > inner[1]):
        raise ValueError("the undistorted image has no inner rectangle: the model folds inside the image")

    def matrix(r):
        fx, fy = (nw - 1) / (r[2] - r[0]), (nh - 1) / (r[3] - r[1])
        return np.array([fx, fy, -fx * r[0], -fy * r[1]])

    k = matrix(inner) * (1.0 - alpha) + matrix(outer) * alpha
    K_new = np.array([[k[0], 0.0, k[2]], [0.0, k[1], k[3]], [0.0, 0.0, 1.0]])
    x0, y0 = int(np.ceil(inner[0] * k[0] + k[2] - 1e-9)), int(np.ceil(inner[1] * k[1] + k[3] - 1e-9))
    x1, y1 = int(np.floor(inner[2] * k[0] + k[2] + 1e-9)), int(np.floor(inner[3] * k[1] + k[3] + 1e-9))
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, nw - 1), min(y1, nh - 1)
    roi = (x0, y0, max(x1 - x0 + 1, 0), max(y1 - y0 + 1, 0))
    return K_new, roi


class _IntMatrix:
    """What :class:`YuvMatrix` and :class:`RgbMatrix` share: integer coefficients times 2^SHIFT named by ``__slots__``, checked
    against the bound of the C entry point (``_in_bound``, worded by ``_BOUND``); ``_COUNT`` and ``_A`` word the other errors,
    ``_OPENCV`` is the table of the preset "bt601"."""

    __slots__ = ()
    SHIFT = 20

    def _set(self, *vals):
        name = type(self).__name__
        if any(int(v) != v for v in vals):
            raise ValueError(f"{name}: the {self._COUNT} values must be integers, got {vals}")
        for slot, v in zip(self.__slots__, vals):
            setattr(self, slot, int(v))
        if not type(self)._in_bound(self.as_tuple()):
            raise ValueError(f"{name}{self.as_tuple()}: {self._BOUND}")

    @classmethod
    def preset(cls, name):
        """"bt601": OpenCV's table for this direction (limited range, three-decimal constants); "bt709", "bt601-full",
        "bt709-full": ``from_standard``."""
        key = str(name).lower()
        if key == "bt601":
            return cls(*cls._OPENCV)
        if key in ("bt709", "bt601-full", "bt709-full"):
            kr, kb = (0.299, 0.114) if key.startswith("bt601") else (0.2126, 0.0722)
            return cls.from_standard(kr, kb, full_range=key.endswith("-full"))
        raise ValueError(f"unknown matrix {name!r}: one of 'bt601', 'bt709', 'bt601-full', 'bt709-full' or {cls._A} {cls.__name__}")

    def as_tuple(self):
        return tuple(getattr(self, n) for n in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, type(self)) and self.as_tuple() == other.as_tuple()

    def __hash__(self):
        return hash(self.as_tuple())

    def __repr__(self):
        return type(self).__name__ + "(" + ", ".join(f"{n}={getattr(self, n)}" for n in self.__slots__) + ")"


def _matrix(matrix, cls):
    """The integers of a matrix of class ``cls``, of a preset's name or of a sequence of as many integers."""
    if isinstance(matrix, cls):
        return matrix.as_tuple()
    return (cls.preset(matrix) if isinstance(matrix, str) else cls(*matrix)).as_tuple()


class YuvMatrix(_IntMatrix):
    """The six integers of sba_convert_frames' rule (include/sba_hip.h), coefficients times 2^20:
    ``l = max(Y - y_offset, 0) cy``, ``R = l + cvr v``, ``G = l + cug u + cvg v``, ``B = l + cub u`` with u = U - 128,
    v = V - 128, each sum rounded by ``(s + 2^19) >> 20`` and clipped to 0..255.  The kernel knows nothing of standards:
    ``from_standard`` and the presets ("bt601" is the table of OpenCV's ``cvtColor(COLOR_YUV2BGR_NV12 / _I420)``) compute the
    integers here, on the host."""

    __slots__ = ("y_offset", "cy", "cvr", "cug", "cvg", "cub")
    _COUNT, _A, _OPENCV, _in_bound = "six", "a", _native.YUV_BT601, staticmethod(_native.yuv_matrix_in_bound)
    _BOUND = ("y_offset must be in 0..255 and 255 |cy| + 128 (|a| + |b|) + 2^19 below 2^31 "
              "for the chroma coefficients a, b of every output row (the bound under which the sums fit 32 bits)")

    def __init__(self, y_offset, cy, cvr, cug, cvg, cub):
        self._set(y_offset, cy, cvr, cug, cvg, cub)

    @classmethod
    def from_standard(cls, kr, kb, full_range=False):
        """From the luma weights of a standard (BT.601: 0.299, 0.114; BT.709: 0.2126, 0.0722), each coefficient c as
        ``round(c * 2**20)``.  Limited range (Y in 16..235, chroma in 16..240): cy = 255/219, cvr = 2 (1 - kr) 255/224,
        cub = 2 (1 - kb) 255/224, cug = -2 kb (1 - kb) / kg 255/224, cvg = -2 kr (1 - kr) / kg 255/224 with kg = 1 - kr - kb,
        y_offset = 16.  Full range: without the factors 255/219 and 255/224, y_offset = 0."""
        kr, kb = float(kr), float(kb)
        kg = 1.0 - kr - kb
        if not (0.0 < kr < 1.0 and 0.0 < kb < 1.0 and kg > 0.0):
            raise ValueError(f"kr, kb and 1 - kr - kb must lie in (0, 1), got kr = {kr}, kb = {kb}")
        sy, sc = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
        coeff = (sy, 2.0 * (1.0 - kr) * sc, -2.0 * kb * (1.0 - kb) / kg * sc, -2.0 * kr * (1.0 - kr) / kg * sc, 2.0 * (1.0 - kb) * sc)
        return cls(0 if full_range else 16, *(int(round(c * (1 << cls.SHIFT))) for c in coeff))


def convert_frames(frames, pixel_format, out_format="bgr", matrix="bt601", out=None, chunk_frames=0, device=0):
    """What a video decoder produces -- 8-bit YUV 4:2:0 -- into what the rest of the library reads, on the GPU
    (sba_convert_frames, include/sba_hip.h): ``cv.cvtColor(frame, cv.COLOR_YUV2BGR_NV12 / _I420)`` for a whole batch.

    ``pixel_format``: "nv12", "nv21", "i420" or "yv12".  ``frames``: a tuple of planes in the format's order, ``(y, uv)`` or
    ``(y, u, v)`` (yv12: ``(y, v, u)``), with y (B, H, W), uv (B, ceil(H / 2), ceil(W / 2), 2), u and v (B, ceil(H / 2),
    ceil(W / 2)) and any strides; or one stacked array (B, H + ceil(H / 2), W), as ffmpeg's rawvideo pipe delivers ``nv12``
    (even W) and ``yuv420p`` (even W and H).  numpy arrays, or torch tensors on ``device`` read in place.
    ``out_format``: "bgr", "rgb", "bgra", "rgba" -> (B, H, W, 3 | 4), or "b", "g", "r" -> the (B, H, W) plane, the input of the
    detectors and the background model (``channel=0``).  ``matrix``: "bt601" (OpenCV's table, limited range), "bt709",
    "bt601-full", "bt709-full" or a :class:`YuvMatrix`.  Chroma is taken from the nearest sample, as OpenCV does.  The result is
    a numpy array for numpy frames and a device tensor for tensors, or ``out`` (either kind, any row and frame strides)."""
    return _native.convert_frames(frames, pixel_format, out_format=out_format, matrix=_matrix(matrix, YuvMatrix), out=out,
                                  chunk_frames=chunk_frames, device=device)


class RgbMatrix(_IntMatrix):
    """The ten integers of sba_frames_to_yuv's rule (include/sba_hip.h), coefficients times 2^20: ``Y = cry R + cgy G + cby B``
    plus ``y_offset``, ``U = cru R' + cgu G' + cbu B'`` plus 128, ``V = crv R' + cgv G' + cbv B'`` plus 128, each sum rounded by
    ``(s + 2^19) >> 20`` and clipped to 0..255.  The mirror of :class:`YuvMatrix`: the kernel knows nothing of standards,
    ``from_standard`` and the presets ("bt601" is the table of OpenCV's ``cvtColor(COLOR_BGR2YUV_I420)``) compute the integers
    here, on the host."""

    __slots__ = ("y_offset", "cry", "cgy", "cby", "cru", "cgu", "cbu", "crv", "cgv", "cbv")
    _COUNT, _A, _OPENCV, _in_bound = "ten", "an", _native.RGB_BT601, staticmethod(_native.rgb_matrix_in_bound)
    _BOUND = ("y_offset must be in 0..255 and 255 (|a| + |b| + |c|) below 2^28 for every "
              "row (a, b, c) (the bound under which the sums fit 32 bits)")

    def __init__(self, y_offset, cry, cgy, cby, cru, cgu, cbu, crv, cgv, cbv):
        self._set(y_offset, cry, cgy, cby, cru, cgu, cbu, crv, cgv, cbv)

    @classmethod
    def from_standard(cls, kr, kb, full_range=False):
        """From the luma weights of a standard (BT.601: 0.299, 0.114; BT.709: 0.2126, 0.0722), each coefficient c as
        ``round(c * 2**20)``.  With kg = 1 - kr - kb the rows are Y: (kr, kg, kb) sy; U: (-kr, -kg, 1 - kb) sc / (2 (1 - kb));
        V: (1 - kr, -kg, -kb) sc / (2 (1 - kr)).  Limited range: sy = 219/255, sc = 224/255, y_offset = 16; full range: sy = sc =
        1, y_offset = 0.  The exact coefficients of a chroma row sum to 0, so the rounded ones sum to -1, 0 or 1, and grey g maps
        to exactly 128 in both chroma modes (|255 sum| < 2^19, |4 * 255 sum| < 2^21): plain rounding needs no adjustment."""
        kr, kb = float(kr), float(kb)
        kg = 1.0 - kr - kb
        if not (0.0 < kr < 1.0 and 0.0 < kb < 1.0 and kg > 0.0):
            raise ValueError(f"kr, kb and 1 - kr - kb must lie in (0, 1), got kr = {kr}, kb = {kb}")
        sy, sc = (1.0, 1.0) if full_range else (219.0 / 255.0, 224.0 / 255.0)
        su, sv = sc / (2.0 * (1.0 - kb)), sc / (2.0 * (1.0 - kr))
        coeff = (kr * sy, kg * sy, kb * sy, -kr * su, -kg * su, (1.0 - kb) * su, (1.0 - kr) * sv, -kg * sv, -kb * sv)
        return cls(0 if full_range else 16, *(int(round(c * (1 << cls.SHIFT))) for c in coeff))


def frames_to_yuv(frames, pixel_format="nv12", in_format="bgr", matrix="bt601", chroma="nearest", out=None, chunk_frames=0, device=0):
    """What the rest of the library produces -- BGR / RGB frames or one plane -- into what a video encoder takes, 8-bit YUV
    4:2:0, on the GPU (sba_frames_to_yuv, include/sba_hip.h): ``cv.cvtColor(frame, cv.COLOR_BGR2YUV_I420)`` for a whole batch.

    ``frames``: uint8, (B, H, W, C) with C in (1, 3, 4) or (B, H, W); a numpy array in any layout with contiguous pixels, or a
    torch tensor on ``device``, read in place.  ``in_format``: "bgr", "rgb" (C = 3), "bgra", "rgba" (C = 4, the fourth channel is
    ignored) or "gray"; frames with one channel are grey whatever it says.  ``pixel_format``: "nv12", "nv21", "i420" or "yv12".
    ``matrix``: "bt601" (OpenCV's table, limited range), "bt709", "bt601-full", "bt709-full" or an :class:`RgbMatrix`.
    ``chroma``: "nearest" takes a chroma sample from the top-left pixel of its 2 x 2 block, as OpenCV does; "average" from the
    sum of the four (at an odd edge the existing pixel is repeated), with one rounding.
    Returns, on the side the frames are on, the stacked (B, H + H / 2, W) array of ffmpeg's rawvideo pipe when W and H are even,
    else the tuple of planes in the format's order -- ``(y, uv)`` with uv (B, ceil(H / 2), ceil(W / 2), 2), or ``(y, u, v)``
    (yv12: ``(y, v, u)``); or ``out``, a stacked array or such a tuple, numpy or tensors on ``device`` whatever side the frames
    are on, with any strides :func:`convert_frames` reads: what lies between the samples is left untouched."""
    return _native.frames_to_yuv(frames, pixel_format, in_format=in_format, matrix=_matrix(matrix, RgbMatrix), chroma=chroma, out=out,
                                 chunk_frames=chunk_frames, device=device)


CONVERT_CHUNK_BYTES = 1 << 30       # bytes of the one-channel plane held at a time when decoder frames go to a detector or the model
_PLANE_OF_CHANNEL = ("b", "g", "r")


def planes_in_chunks(frames, pixel_format, matrix, channel, chunk_frames, device):
    """Yields (lo, hi, plane) over a batch of YUV 4:2:0 frames: ``plane`` is the (hi - lo, H, W) device tensor of channel
    ``channel`` (0, 1, 2 = B, G, R: the reference's ``channel=1`` keeps meaning green) of the frames [lo, hi).  One chunk is
    held at a time, whatever the length of the video; a batch without frames yields one empty plane."""
    if channel not in (0, 1, 2):
        raise ValueError(f"with a pixel_format, channel names a plane of BGR: 0, 1 or 2, not {channel!r}")
    L = _native._yuv_layout(frames, pixel_format, device)
    m = _matrix(matrix, YuvMatrix)
    step = int(chunk_frames) if chunk_frames > 0 else max(1, CONVERT_CHUNK_BYTES // max(1, L.height * L.width))
    for lo in range(0, max(L.n_frames, 1), step):
        hi = min(lo + step, L.n_frames)
        yield lo, hi, _native.convert_frames(_native.yuv_frame_slice(frames, lo, hi), pixel_format, out_format=_PLANE_OF_CHANNEL[channel],
                                             matrix=m, out_on_device=True, device=device)


def _factor(factor):
    """(fx, fy) from an int or a pair, each in 1..16."""
    try:
        fx, fy = (factor, factor) if np.ndim(factor) == 0 else factor
        if int(fx) != fx or int(fy) != fy:
            raise ValueError
        fx, fy = int(fx), int(fy)
    except (TypeError, ValueError):
        raise ValueError(f"factor must be an integer or (fx, fy), got {factor!r}") from None
    if not (1 <= fx <= _native.RESIZE_MAX_FACTOR and 1 <= fy <= _native.RESIZE_MAX_FACTOR):
        raise ValueError(f"factor must be within 1..{_native.RESIZE_MAX_FACTOR}, got {(fx, fy)}")
    return fx, fy


def _gray_weights(gray, channel_order):
    """None (keep the channels) or the three integer weights of the channels 0, 1, 2, which sum to 2^15."""
    order = str(channel_order).lower()
    if order not in ("bgr", "rgb"):
        raise ValueError(f"channel_order must be 'bgr' or 'rgb', not {channel_order!r}")
    if gray is None or isinstance(gray, (bool, np.bool_)):
        w = _native.GRAY_BGR
        return None if not gray else w if order == "bgr" else w[::-1]
    try:
        w = tuple(int(v) for v in gray)
        if len(w) != 3 or any(a != b for a, b in zip(w, gray)):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"gray must be a bool or three integer weights, got {gray!r}") from None
    if min(w) < 0 or sum(w) != 1 << _native.GRAY_SHIFT:
        raise ValueError(f"the gray weights must be >= 0 and sum to 2^{_native.GRAY_SHIFT}, got {w}")
    return w


def resize_frames(frames, factor, gray=False, channel_order="bgr", out=None, chunk_frames=0, pixel_format=None, matrix="bt601", device=0):
    """Previews of a batch of frames, on the GPU (sba_resize_frames, include/sba_hip.h): ``cv2.resize(frame, (W // fx, H // fy),
    interpolation=cv2.INTER_AREA)`` for sizes that are multiples of the factor -- every pixel the average of a block of
    fx x fy pixels --, after ``cv2.cvtColor(frame, cv2.COLOR_BGR2GRAY)`` with ``gray``.

    ``frames``: uint8, (B, H, W, C) with C in (1, 3, 4) or (B, H, W); a numpy array in any layout with contiguous pixels, or a
    torch tensor on ``device``, read in place.  ``factor``: an int, or ``(fx, fy)``, each in 1..16; columns and rows beyond the
    last whole block are not read (OpenCV would spread fractional weights over them).  ``gray``: False keeps the channels ->
    (B, H // fy, W // fx[, C]); True writes the grey value of OpenCV's weights -> (B, H // fy, W // fx), with
    ``channel_order`` "bgr" or "rgb" saying which channel is which; or three integer weights >= 0 of the channels 0, 1, 2 that
    sum to 2^15.  A factor of 1 with ``gray`` only converts.  The result is a numpy array for numpy frames and a device tensor
    for tensors, or ``out`` (either kind), which may be a view into a larger array or tensor: what lies between its rows and
    frames is left untouched.  With a ``pixel_format`` ("nv12", "nv21", "i420", "yv12") the frames are YUV 4:2:0 as
    :func:`convert_frames` takes them: they are converted to BGR chunk by chunk (``chunk_frames`` frames; 0 = the default) on
    the device under ``matrix``, and each chunk is resized."""
    fx, fy = _factor(factor)
    w = _gray_weights(gray, channel_order)
    if pixel_format is None:
        return _native.resize_frames(frames, fx, fy, gray_w=w, out=out, chunk_frames=chunk_frames, device=device)
    L = _native._yuv_layout(frames, pixel_format, device)
    m = _matrix(matrix, YuvMatrix)
    shape = (L.n_frames, L.height // fy, L.width // fx) + (() if w is not None else (3,))
    if out is None:
        if L.tensor:
            import torch
            out = torch.empty(shape, dtype=torch.uint8, device=f"cuda:{device}")
        else:
            out = np.empty(shape, np.uint8)
    elif tuple(out.shape) != shape:
        raise ValueError(f"out has the shape {tuple(out.shape)}, expected {shape}")
    w = _gray_weights(gray, "bgr")                           # the converted chunks are BGR: channel_order says nothing about them
    step = int(chunk_frames) if chunk_frames > 0 else max(1, CONVERT_CHUNK_BYTES // max(1, 3 * L.height * L.width))
    for lo in range(0, L.n_frames, step):
        hi = min(lo + step, L.n_frames)
        bgr = _native.convert_frames(_native.yuv_frame_slice(frames, lo, hi), pixel_format, out_format="bgr", matrix=m, out_on_device=True,
                                     device=device)
        _native.resize_frames(bgr, fx, fy, gray_w=w, out=out[lo:hi], device=device)
    return out


def mosaic(batches, factor, columns=None, gap=0, fill=0, gray=False, on_device=False, channel_order="bgr", device=0):
    """The cameras of a rig side by side: one canvas per frame index, each camera's preview in its own tile, as the reference's
    tiled viewer shows them.  Returns ``(canvas, origins)``.

    ``batches``: a list of per-camera frame batches as :func:`resize_frames` takes them, of equal length and the same number
    of channels; their sizes may differ.  ``factor``, ``gray`` and ``channel_order`` as there.  The tiles are as large as the
    largest preview and lie row-major, ``columns`` to a row (default ``ceil(sqrt(n))``), ``gap`` pixels apart; the gaps and the
    part of a tile that its preview does not cover hold ``fill`` (0..255).  ``canvas`` is (n_frames, H, W[, C]) uint8, a numpy
    array or with ``on_device`` a tensor on ``device``; every camera is ONE resize_frames call that writes straight into its
    tile.  ``origins`` is (n, 2) int64, the (x, y) of every tile's first pixel: a click at (X, Y) inside camera k's preview is
    the source pixel ((X - x_k) fx, (Y - y_k) fy) of that camera."""
    fx, fy = _factor(factor)
    w = _gray_weights(gray, channel_order)
    n = len(batches)
    if n == 0:
        raise ValueError("mosaic needs at least one camera")
    columns = int(np.ceil(np.sqrt(n))) if columns is None else int(columns)
    gap, fill = int(gap), int(fill)
    if columns < 1 or gap < 0 or not 0 <= fill <= 255:
        raise ValueError(f"columns must be >= 1, gap >= 0 and fill in 0..255, got {(columns, gap, fill)}")
    layouts = [_native._frame_layout(b, device) for b in batches]
    n_frames = layouts[0][2]
    if any(L[2] != n_frames for L in layouts):
        raise ValueError(f"every camera must have the same number of frames, got {[L[2] for L in layouts]}")
    tails = {() if w is not None or len(L[1].shape) == 3 else (L[5],) for L in layouts}
    if len(tails) != 1:
        raise ValueError("every camera must have the same number of channels")
    sizes = [(L[3] // fy, L[4] // fx) for L in layouts]                   # (height, width) of every preview
    th, tw = max(s[0] for s in sizes), max(s[1] for s in sizes)
    if min(min(s) for s in sizes) == 0:
        raise ValueError(f"a factor is larger than a camera's frames: previews of {sizes}")
    rows = (n + columns - 1) // columns
    shape = (n_frames, rows * th + (rows - 1) * gap, columns * tw + (columns - 1) * gap) + next(iter(tails))
    if on_device:
        import torch
        canvas = torch.full(shape, fill, dtype=torch.uint8, device=f"cuda:{device}")
    else:
        canvas = np.full(shape, fill, np.uint8)
    origins = np.array([[(k % columns) * (tw + gap), (k // columns) * (th + gap)] for k in range(n)], np.int64)
    for b, (h, wd), (x, y) in zip(batches, sizes, origins):
        _native.resize_frames(b, fx, fy, gray_w=w, out=canvas[:, y:y + h, x:x + wd], device=device)
    return canvas, origins


class FrameHistograms:
    """Result of :func:`frame_histograms`: ``hist`` (B, 256) uint32, one row per frame, or None when only the total was asked
    for, and ``total`` (256,) uint64, the sum over every frame counted so far.  The methods are exact integer arithmetic on the
    host and return one entry per frame; without ``hist`` they treat ``total`` as the one row there is."""

    def __init__(self, hist, total):
        self.hist, self.total = hist, total

    def _rows(self):
        """(B, 256) int64 counts; a total beyond 2^63 does not occur (2^28 pixels a frame)."""
        return (self.total[None] if self.hist is None else self.hist).astype(np.int64)

    def count_above(self):
        """(B, 256) int64: entry [f, t] is the number of pixels with value > t -- the ``n`` of ``find_laser_dots(threshold=t)``."""
        h = self._rows()
        return h.sum(axis=1, keepdims=True) - np.cumsum(h, axis=1)

    def n_saturated(self):
        """(B,) the pixels with the value 255: the weighted centroid of a dot that holds some is biased."""
        return self._rows()[:, 255]

    def vmax(self):
        """(B,) the largest value present, -1 for an empty region."""
        h = self._rows()
        return np.where(h.any(axis=1), 255 - np.argmax(h[:, ::-1] > 0, axis=1), -1)

    def vmin(self):
        """(B,) the smallest value present, -1 for an empty region."""
        h = self._rows()
        return np.where(h.any(axis=1), np.argmax(h > 0, axis=1), -1)

    def percentile(self, q):
        """(B,) the smallest v whose cumulative count -- the pixels with value <= v -- reaches ceil(q n / 100) of the frame's n
        pixels, taken exactly (q as the fraction it is); -1 when n = 0.  q = 0 asks for a count of 0 and gives 0."""
        from fractions import Fraction
        if not 0 <= q <= 100:
            raise ValueError(f"q must be within 0..100, got {q}")
        cum = np.cumsum(self._rows(), axis=1)
        out = np.full(cum.shape[0], -1, np.int64)
        for f, c in enumerate(cum):
            n = int(c[-1])
            if n:
                need = Fraction(q) * n / 100
                out[f] = np.searchsorted(c, -((-need.numerator) // need.denominator), side="left")
        return out

    def otsu(self):
        """(B,) Otsu's threshold: the t that maximises the between-class variance of the classes value <= t and value > t,
        (s0 N - S n0)^2 / (n0 (N - n0)) with n0, s0 the count and the sum of the values up to t and N, S those of the frame,
        compared as exact fractions of integers; the lowest t on ties (a frame of one value: 0); -1 for an empty region."""
        h = self._rows().astype(object)
        n0, s0 = np.cumsum(h, axis=1), np.cumsum(h * np.arange(256).astype(object), axis=1)
        N, S = n0[:, -1:], s0[:, -1:]
        num, den = (s0 * N - S * n0) ** 2, n0 * (N - n0)
        den[den == 0] = 1                                     # a class is empty: the numerator is 0 there
        best, bn, bd = np.zeros(h.shape[0], np.int64), num[:, 0], den[:, 0]
        for t in range(1, 256):
            better = num[:, t] * bd > bn * den[:, t]
            best[better.astype(bool)] = t
            bn, bd = np.where(better, num[:, t], bn), np.where(better, den[:, t], bd)
        best[(N[:, 0] == 0).astype(bool)] = -1
        return best

    def threshold_table(self, min_area, max_area):
        """(256,) int64: for every threshold t the number of frames with min_area <= count_above[f, t] <= max_area."""
        above = self.count_above()
        return ((above >= int(min_area)) & (above <= int(max_area))).sum(axis=0).astype(np.int64)

    def suggest_threshold(self, min_area, max_area):
        """The middle, rounded down, of the longest run of thresholds on which ``threshold_table`` attains its maximum -- the
        lowest such run on ties --, or None when no threshold leaves a dot of that size in any frame."""
        table = self.threshold_table(min_area, max_area)
        if table.size == 0 or table.max() == 0:
            return None
        at_max = np.concatenate([[False], table == table.max(), [False]])
        edges = np.flatnonzero(at_max[1:] != at_max[:-1])     # starts and ends (exclusive) of the runs, in turn
        starts, ends = edges[::2], edges[1::2]
        k = int(np.argmax(ends - starts))                     # the first of the longest
        return int((starts[k] + ends[k] - 1) // 2)


def frame_histograms(frames, channel=1, roi_rect=None, roi_circle=None, per_frame=True, total=None, chunk_frames=0, device=0,
                     background=None, pixel_format=None, matrix="bt601") -> FrameHistograms:
    """The 256-bin histogram of byte ``channel`` of every frame of a batch inside ``roi_rect`` and ``roi_circle``
    (sba_frame_histograms) -> :class:`FrameHistograms`.  Everything is as for ``feature_detection.find_laser_dots`` -- the
    frames (numpy or a tensor on the device), the regions, ``background=`` (the static light is gated out first) and
    ``pixel_format=`` / ``matrix`` (decoder YUV 4:2:0, converted to the plane ``channel`` names) -- so the histogram is taken of
    exactly the plane that detector would threshold.  ``per_frame=False`` returns only the running total, for whole videos;
    ``total=`` (a (256,) array or a previous result) is continued, not written."""
    from . import feature_detection as fd
    total = total.total if isinstance(total, FrameHistograms) else total
    if background is None and pixel_format is None:
        return FrameHistograms(*_native.frame_histograms(frames, channel=channel, roi_rect=roi_rect, roi_circle=roi_circle, total=total,
                                                         want_hist=per_frame, chunk_frames=chunk_frames, device=device))
    running = [total]

    def count(clean):
        hist, running[0] = _native.frame_histograms(clean, channel=0, roi_rect=roi_rect, roi_circle=roi_circle, total=running[0],
                                                    want_hist=per_frame, device=device)
        return FrameHistograms(hist, None)

    def make(hist):
        return FrameHistograms(hist, running[0])

    if pixel_format is not None:
        return fd._from_decoder_frames(frames, pixel_format, matrix, background, channel, chunk_frames, device, count, ("hist",), make)
    return fd._without_background(frames, background, channel, chunk_frames, device, count, ("hist",), make)


class CornerRefinement:
    """What :func:`refine_corners` returns.  ``corners``: the refined positions in the shape of the input (a list of (k, 2)
    arrays, or one array); over all corners in the order given ``xy`` (n, 2), ``status`` (n,) int32 of sba_corner_status bits,
    ``iterations`` (n,) int32 and ``tensor`` (n, 3): a, b, c of the window's structure tensor [[a, b], [b, c]] at the last
    position sampled."""

    def __init__(self, corners, xy, status, iterations, tensor):
        self.corners, self.xy, self.status, self.iterations, self.tensor = corners, xy, status, iterations, tensor

    @property
    def ok(self):
        """(n,) bool: converged and not put back to its start."""
        return (self.status & (_native.CORNER_CONVERGED | _native.CORNER_RESTORED)) == _native.CORNER_CONVERGED

    def covariance_shape(self):
        """(n, 2, 2): the inverse of the structure tensor, the shape of a corner's positional covariance up to the image
        noise; NaN where the corner is SINGULAR or INVALID or the tensor has no inverse."""
        a, b, c = self.tensor.T
        det = a * c - b * b
        bad = (self.status & (_native.CORNER_SINGULAR | _native.CORNER_INVALID)) != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = np.stack([c, -b, -b, a], axis=1) / np.where(bad | (det == 0), np.nan, det)[:, None]
        return inv.reshape(-1, 2, 2)


def _pair(value, name):
    try:
        a, b = (int(v) for v in value)
        if (a, b) != tuple(value):
            raise ValueError
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be two integers, got {value!r}") from None
    return a, b


def corner_window(win, zero_zone=(-1, -1)):
    """OpenCV's window of ``cv.cornerSubPix`` as (2 win_y + 1, 2 win_x + 1) float64 weights: entry (i, j) is
    exp(-(i / win_y)^2) * exp(-(j / win_x)^2) with ``math.exp``, and 0 inside the zero zone when both of its half sizes are
    >= 0 and it is smaller than the window (sba_refine_corners, include/sba_hip.h).  ``win`` and ``zero_zone`` are (x, y)."""
    import math
    (wx, wy), (zx, zy) = _pair(win, "win"), _pair(zero_zone, "zero_zone")
    if not (1 <= wx <= _native.CORNER_MAX_WIN and 1 <= wy <= _native.CORNER_MAX_WIN):
        raise ValueError(f"win must be in 1..{_native.CORNER_MAX_WIN}, got {(wx, wy)}")
    m = np.empty((2 * wy + 1, 2 * wx + 1))
    for i in range(2 * wy + 1):
        yy = float(i - wy) / float(wy)
        vy = math.exp(-(yy * yy))
        for j in range(2 * wx + 1):
            xx = float(j - wx) / float(wx)
            m[i, j] = vy * math.exp(-(xx * xx))
    if zx >= 0 and zy >= 0 and zx < wx and zy < wy:
        m[wy - zy:wy + zy + 1, wx - zx:wx + zx + 1] = 0.0
    return m


def refine_corners(frames, corners, win=(3, 3), zero_zone=(-1, -1), max_iter=200, eps=1e-5, channel=None, weights=None,
                   channel_order="bgr", chunk_frames=0, device=0) -> CornerRefinement:
    """``cv.cornerSubPix`` for the corners of a batch of frames, on the GPU (sba_refine_corners, include/sba_hip.h) ->
    :class:`CornerRefinement`.

    ``frames`` as for ``feature_detection.find_laser_dots``: (B, H, W[, C]) uint8, numpy or a tensor on ``device`` read in
    place.  ``corners``: a list of B arrays (k_f, 2) of (x, y) pixel coordinates, one per frame (a frame may have none), or one
    (n, 2) array when there is a single frame.  ``win`` and ``zero_zone`` are OpenCV's winSize and zeroZone (half sizes, x
    first), ``max_iter`` and ``eps`` its criteria.  ``channel``: the byte of a pixel that is read, or -1 for the grey value of
    ``resize_frames`` (``channel_order`` as there); None is -1 for colour frames and 0 for one plane.  ``weights``: None is
    OpenCV's window (:func:`corner_window`), else (2 win_y + 1, 2 win_x + 1) weights, finite and >= 0, to which ``zero_zone``
    is not applied.  The weights are always built here and handed over explicitly, so the library's bits do not depend on the C
    runtime's ``exp``."""
    wx, wy = _pair(win, "win")
    zero_zone = _pair(zero_zone, "zero_zone")
    if not (1 <= wx <= _native.CORNER_MAX_WIN and 1 <= wy <= _native.CORNER_MAX_WIN):
        raise ValueError(f"win must be in 1..{_native.CORNER_MAX_WIN}, got {(wx, wy)}")
    if not 1 <= int(max_iter) <= _native.CORNER_MAX_ITERATIONS:
        raise ValueError(f"max_iter must be in 1..{_native.CORNER_MAX_ITERATIONS}, got {max_iter!r}")
    if not float(eps) >= 0.0:
        raise ValueError(f"eps must be >= 0, got {eps!r}")
    if weights is None:
        weights = corner_window((wx, wy), zero_zone)
    else:
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != (2 * wy + 1, 2 * wx + 1):
            raise ValueError(f"weights must have the shape {(2 * wy + 1, 2 * wx + 1)}, got {weights.shape}")
        if not np.all(np.isfinite(weights)) or weights.min() < 0:
            raise ValueError("weights must be finite and >= 0")
    shape = tuple(frames.shape)
    if len(shape) not in (3, 4):
        raise ValueError(f"frames must be (B, H, W, C) or (B, H, W), got {shape}")
    B, Cn = int(shape[0]), int(shape[3]) if len(shape) == 4 else 1
    channel = (0 if Cn == 1 else -1) if channel is None else int(channel)
    if not (-1 <= channel < Cn) or (channel == -1 and Cn == 1):
        raise ValueError(f"channel must be in 0..{Cn - 1}" + (" or -1 (gray)" if Cn > 1 else "") + f", got {channel}")
    gray_w = _gray_weights(True, channel_order) if channel == -1 else None
    single = isinstance(corners, np.ndarray) and corners.ndim == 2
    per_frame = [corners] if single else list(corners)
    if len(per_frame) != B:
        raise ValueError(f"corners must be one (k, 2) array per frame ({B}), got {len(per_frame)}"
                         + (": a single array needs a single frame" if single else ""))
    per_frame = [np.asarray(c, dtype=np.float64).reshape(-1, 2) if np.size(c) == 0 else np.asarray(c, dtype=np.float64) for c in per_frame]
    for f, c in enumerate(per_frame):
        if c.ndim != 2 or c.shape[1] != 2:
            raise ValueError(f"corners of frame {f} must be (k, 2), got {c.shape}")
    start = np.zeros(B + 1, np.int64)
    np.cumsum([len(c) for c in per_frame], out=start[1:])
    xy = np.concatenate(per_frame) if per_frame else np.zeros((0, 2))
    refined, status, iterations, tensor = _native.refine_corners(frames, start, xy, win=(wx, wy), zero_zone=zero_zone, max_iter=int(max_iter),
                                                                 eps=float(eps), channel=channel, gray_w=gray_w, weights=weights,
                                                                 chunk_frames=chunk_frames, device=device)
    out = refined if single else [refined[start[f]:start[f + 1]] for f in range(B)]
    return CornerRefinement(out, refined, status, iterations, tensor)


def corner_sub_pix(gray, corners, winSize=(3, 3), zeroZone=(-1, -1), criteria=(3, 200, 1e-5), device=0):
    """``cv.cornerSubPix(gray, corners, winSize, zeroZone, criteria)`` for one image -> the refined corners in the shape and dtype
    of ``corners``, which may be (n, 1, 2) float32 as ``cv.aruco`` returns them.  ``criteria`` is OpenCV's (type, max_iter, eps):
    bit 1 of the type (COUNT) makes max_iter count, bit 2 (EPS) eps; without them OpenCV's own 100 and 0 apply.  ``gray`` is
    (H, W) uint8, or a colour image, of which the grey value is read."""
    gray = gray if _native._is_tensor(gray) else np.ascontiguousarray(gray)
    if len(gray.shape) not in (2, 3):
        raise ValueError(f"gray must be one image (H, W) or (H, W, C), got the shape {tuple(gray.shape)}")
    pts = np.asarray(corners)
    if pts.size % 2 or (pts.ndim and pts.shape[-1] != 2):
        raise ValueError(f"corners must hold (x, y) pairs, got the shape {pts.shape}")
    kind, count, eps = criteria
    count = min(max(int(count), 1), _native.CORNER_MAX_ITERATIONS) if int(kind) & 1 else 100
    eps = max(float(eps), 0.0) if int(kind) & 2 else 0.0
    res = refine_corners(gray[None], np.asarray(pts, dtype=np.float64).reshape(-1, 2), win=winSize, zero_zone=zeroZone, max_iter=count,
                         eps=eps, device=device)
    return res.xy.reshape(pts.shape).astype(pts.dtype if pts.dtype.kind == "f" else np.float64)


def corner_weights(result, floor=0.0):
    """One weight per corner of a :class:`CornerRefinement`, usable as ``PySBA`` ``pointWeights``: the smaller eigenvalue of the
    structure tensor -- large at a crisp corner, near zero along an edge --, divided by its median over the corners that are
    ``ok``, so that a typical corner weighs 1; 0 where not ``ok``.  ``floor``: the least weight an ``ok`` corner gets."""
    a, b, c = result.tensor.T
    lam = 0.5 * (a + c) - np.sqrt((0.5 * (a - c)) ** 2 + b * b)
    ok = result.ok & np.isfinite(lam)
    w = np.zeros(len(lam))
    if ok.any():
        med = np.median(lam[ok])
        w[ok] = np.maximum(lam[ok] / med, float(floor)) if med > 0 else 1.0
    return w


ADAPTIVE_THRESH_MEAN_C, THRESH_BINARY, THRESH_BINARY_INV = 0, 0, 1      # OpenCV's constants


def marker_threshold_windows(win_min=3, win_max=23, win_step=10):
    """The window sizes ``cv2.aruco``'s ``detectMarkers`` thresholds with (its adaptiveThreshWinSizeMin, -Max and -Step):
    ``range(win_min, win_max + 1, win_step)``, an even size made odd by adding 1.  The default gives (3, 13, 23)."""
    win_min, win_max, win_step = int(win_min), int(win_max), int(win_step)
    if win_min < 3 or win_max < win_min or win_step < 1:
        raise ValueError(f"need 3 <= win_min <= win_max and win_step >= 1, got {(win_min, win_max, win_step)}")
    return tuple(w + 1 if w % 2 == 0 else w for w in range(win_min, win_max + 1, win_step))


def adaptive_threshold(frames, block_size, C=7, threshold_type="binary_inv", max_value=255, channel=None, return_mean=False,
                       out=None, channel_order="bgr", chunk_frames=0, device=0):
    """``cv.adaptiveThreshold(grey, max_value, ADAPTIVE_THRESH_MEAN_C, type, block_size, C)`` for a batch of frames, on the GPU
    (sba_adaptive_threshold, include/sba_hip.h): a pixel is set where it is darker (``"binary_inv"``, what ArUco uses) or
    brighter (``"binary"``) than the mean of the ``block_size`` x ``block_size`` window around it, less ``C``.

    ``frames`` as for ``feature_detection.find_laser_dots``: (B, H, W[, C]) uint8, numpy or a tensor on ``device`` read in
    place.  ``block_size``: an odd int in 3..127 -> (B, H, W), or a sequence of up to four -> (K, B, H, W): all windows in one
    call, the frames read once (:func:`marker_threshold_windows` gives ArUco's).  ``C``: a number or one per window, turned
    into the integer OpenCV compares with (``ceil`` for binary, ``floor`` for binary_inv).  ``channel``: the byte of a pixel
    that is read, or -1 for the grey value of ``resize_frames`` (``channel_order`` as there); None is -1 for colour frames and
    0 for one plane.  ``return_mean``: also return the local means (``cv.blur`` with a replicated border) -> (masks, means).
    The result lies where the frames lie, or is the caller's ``out`` of the result's shape (a view with strides is written in
    place); a mask left on the device is a one-channel frame that ``find_laser_blobs`` labels at ``threshold=127``."""
    kind = {"binary": 0, "binary_inv": 1, THRESH_BINARY: 0, THRESH_BINARY_INV: 1}.get(
        threshold_type.lower() if isinstance(threshold_type, str) else threshold_type)
    if kind is None:
        raise ValueError(f"threshold_type must be 'binary' or 'binary_inv', not {threshold_type!r}")
    single = np.ndim(block_size) == 0
    blocks = [block_size] if single else list(block_size)
    if not 1 <= len(blocks) <= _native.ADAPTIVE_MAX_WINDOWS:
        raise ValueError(f"block_size must be one window size or up to {_native.ADAPTIVE_MAX_WINDOWS}, got {len(blocks)}")
    for b in blocks:
        if int(b) != b or int(b) % 2 == 0 or not 3 <= int(b) <= _native.ADAPTIVE_MAX_BLOCK:
            raise ValueError(f"a block size must be an odd integer in 3..{_native.ADAPTIVE_MAX_BLOCK}, got {b!r}")
    cs = [C] * len(blocks) if np.ndim(C) == 0 else list(C)
    if len(cs) != len(blocks):
        raise ValueError(f"C must be one number or one per window ({len(blocks)}), got {len(cs)}")
    if not all(np.isfinite(float(c)) for c in cs):
        raise ValueError(f"C must be finite, got {C!r}")
    deltas = [int(np.floor(float(c))) if kind else int(np.ceil(float(c))) for c in cs]
    if any(abs(d) > _native.ADAPTIVE_MAX_DELTA for d in deltas):
        raise ValueError(f"C must lie in -{_native.ADAPTIVE_MAX_DELTA}..{_native.ADAPTIVE_MAX_DELTA}, got {C!r}")
    if not 0 < int(max_value) <= 255:
        raise ValueError(f"max_value must be in 1..255, got {max_value!r}")
    shape = tuple(frames.shape)
    if len(shape) not in (3, 4):
        raise ValueError(f"frames must be (B, H, W, C) or (B, H, W), got {shape}")
    Cn = int(shape[3]) if len(shape) == 4 else 1
    channel = (0 if Cn == 1 else -1) if channel is None else int(channel)
    if not (-1 <= channel < Cn) or (channel == -1 and Cn == 1):
        raise ValueError(f"channel must be in 0..{Cn - 1}" + (" or -1 (gray)" if Cn > 1 else "") + f", got {channel}")
    gray_w = _gray_weights(True, channel_order) if channel == -1 else None
    if out is not None and single:
        if len(out.shape) != 3:
            raise ValueError(f"out has the shape {tuple(out.shape)}, expected {shape[:3]}")
        out = out[None]
    masks, means = _native.adaptive_threshold(frames, [int(b) for b in blocks], deltas, invert=bool(kind), max_value=int(max_value),
                                              channel=channel, gray_w=gray_w, out=out, mean_out=True if return_mean else None,
                                              chunk_frames=chunk_frames, device=device)
    if single:
        masks, means = masks[0], None if means is None else means[0]
    return (masks, means) if return_mean else masks


def adaptive_threshold_cv(src, maxValue, adaptiveMethod, thresholdType, blockSize, C, device=0):
    """``cv.adaptiveThreshold(src, maxValue, adaptiveMethod, thresholdType, blockSize, C)`` for one 2-D grey image -> (H, W)
    uint8.  ``adaptiveMethod`` must be ``ADAPTIVE_THRESH_MEAN_C`` (0), ``thresholdType`` ``THRESH_BINARY`` (0) or
    ``THRESH_BINARY_INV`` (1); ``maxValue`` is saturated to 0..255 as OpenCV does, and 0 gives an empty mask."""
    if adaptiveMethod != ADAPTIVE_THRESH_MEAN_C:
        raise ValueError(f"only ADAPTIVE_THRESH_MEAN_C (0) is implemented, got adaptiveMethod = {adaptiveMethod!r}")
    if thresholdType not in (THRESH_BINARY, THRESH_BINARY_INV):
        raise ValueError(f"thresholdType must be THRESH_BINARY (0) or THRESH_BINARY_INV (1), got {thresholdType!r}")
    src = src if _native._is_tensor(src) else np.ascontiguousarray(src)
    if len(src.shape) != 2:
        raise ValueError(f"src must be one grey image (H, W), got the shape {tuple(src.shape)}")
    top = int(min(max(np.rint(float(maxValue)), 0), 255))
    if top == 0:
        if _native._is_tensor(src):
            return src.new_zeros(tuple(src.shape))
        if src.dtype != np.uint8:
            raise ValueError(f"frames must be uint8, not {src.dtype}")
        return np.zeros(src.shape, np.uint8)
    return adaptive_threshold(src[None], int(blockSize), C=C, threshold_type=thresholdType, max_value=top, device=device)[0]


class BackgroundModel:
    """Per-pixel statistics over time of one channel of one camera's frames, and what follows from them.

    The laser dot visits a pixel in a handful of frames; a status LED, a leaking illuminator or a reflection is there in all of
    them.  ``add`` streams frames through sba_background_accumulate (exact integers: the sum, the square sum, the number of
    frames above ``threshold`` and the maximum of every pixel; any batching gives the same bits), ``level`` and ``hot_mask``
    turn the statistics into a per-pixel level and a mask of the pixels that are lit too often, and ``suppress`` takes both out
    of a batch of frames (sba_background_suppress) -> one-channel frames for the detectors, which
    ``feature_detection.find_laser_dots`` / ``find_laser_blobs`` do by themselves when given ``background=model``.

    ``on_device=True`` keeps the accumulators in device memory (torch tensors on ``device``, created with the first ``add``);
    otherwise they are numpy arrays.  ``state()`` / ``from_state`` give and take a dict of plain numpy arrays, to be pickled
    next to the centroids."""

    _KINDS = (("sum", np.uint32), ("sumsq", np.uint64), ("hot", np.uint32), ("vmax", np.uint8))

    def __init__(self, height, width, channel=1, threshold=50, device=0, on_device=True):
        self.height, self.width, self.channel, self.threshold = int(height), int(width), int(channel), int(threshold)
        self.device, self.on_device = int(device), bool(on_device)
        if not (0 <= self.height <= _native.DOT_MAX_DIM and 0 <= self.width <= _native.DOT_MAX_DIM):
            raise ValueError(f"height and width must be within 0..{_native.DOT_MAX_DIM}, got {(height, width)}")
        if not 0 <= self.threshold <= 255:
            raise ValueError(f"threshold must be in 0..255, got {threshold}")
        self.n = 0
        self._acc = {name: np.zeros((self.height, self.width), dt) for name, dt in self._KINDS}

    # ---- accumulators
    def _numpy(self, name):
        a = self._acc[name]
        if _native._is_tensor(a):
            a = a.cpu().numpy().view(dict(self._KINDS)[name])
        return a

    def _to_device(self):
        import torch
        signed = {"sum": np.int32, "sumsq": np.int64, "hot": np.int32, "vmax": np.uint8}      # the same bits
        for name, a in self._acc.items():
            if not _native._is_tensor(a):
                self._acc[name] = torch.from_numpy(a.view(signed[name])).to(f"cuda:{self.device}")

    def _add_planes(self, frames, use, pixel_format, matrix, chunk_frames):
        L = _native._yuv_layout(frames, pixel_format, self.device)
        if (L.height, L.width) != (self.height, self.width):
            raise ValueError(f"frames are {L.height} x {L.width}, the model is {self.height} x {self.width}")
        if use is not None:
            use = np.asarray(use)
            if use.shape != (L.n_frames,):
                raise ValueError(f"use must hold one flag per frame ({L.n_frames}), got the shape {use.shape}")
        if self.on_device:
            self._to_device()
        for lo, hi, plane in planes_in_chunks(frames, pixel_format, matrix, self.channel, chunk_frames, self.device):
            self.n = _native.background_accumulate(plane, n_used=self.n, use=None if use is None else use[lo:hi], threshold=self.threshold,
                                                   channel=0, accumulate=True, device=self.device, **self._acc)
        return self

    def add(self, frames, use=None, pixel_format=None, matrix="bt601", chunk_frames=0):
        """Adds the frames (uint8 (B, H, W, C) or (B, H, W), numpy or a tensor on the device) whose ``use`` flag is set -- None:
        all -- to the statistics.  Returns self.  With a ``pixel_format`` ("nv12", "nv21", "i420", "yv12") the frames are YUV
        4:2:0 as :func:`convert_frames` takes them; they are converted chunk by chunk (``chunk_frames`` frames, 0 = the default)
        to the plane the model's ``channel`` names (0, 1, 2 = B, G, R) under ``matrix``, and the plane is added."""
        if pixel_format is not None:
            return self._add_planes(frames, use, pixel_format, matrix, chunk_frames)
        _t, _f, _B, H, W, _C, _sr, _sf = _native._frame_layout(frames, self.device)
        if (H, W) != (self.height, self.width):
            raise ValueError(f"frames are {H} x {W}, the model is {self.height} x {self.width}")
        if self.on_device:
            self._to_device()
        self.n = _native.background_accumulate(frames, n_used=self.n, use=use, threshold=self.threshold, channel=self.channel,
                                               accumulate=True, device=self.device, **self._acc)
        return self

    def state(self):
        """A dict of plain numbers and numpy arrays that ``from_state`` turns back into the model."""
        out = {k: getattr(self, k) for k in ("height", "width", "channel", "threshold", "n")}
        out.update({name: self._numpy(name).copy() for name, _dt in self._KINDS})
        return out

    @classmethod
    def from_state(cls, state, device=0, on_device=True):
        m = cls(state["height"], state["width"], channel=state["channel"], threshold=state["threshold"], device=device, on_device=on_device)
        m.n = int(state["n"])
        if not 0 <= m.n <= _native.BG_MAX_FRAMES:
            raise ValueError(f"n must be within 0..2^24, got {m.n}")
        for name, dt in cls._KINDS:
            a = np.ascontiguousarray(state[name], dtype=dt)
            if a.shape != (m.height, m.width):
                raise ValueError(f"{name} has the shape {a.shape}, expected {(m.height, m.width)}")
            m._acc[name] = a.copy()
        return m

    # ---- what the statistics say (host, float64: H x W arithmetic once per video)
    def _need_frames(self):
        if self.n <= 0:
            raise ValueError("the model has seen no frame yet")

    def mean(self):
        self._need_frames()
        return self._numpy("sum").astype(np.float64) / self.n

    def std(self):
        """sqrt(max(sumsq / n - mean^2, 0)): the population standard deviation."""
        mean = self.mean()
        return np.sqrt(np.maximum(self._numpy("sumsq").astype(np.float64) / self.n - mean * mean, 0.0))

    def max(self):
        return self._numpy("vmax").copy()

    def hot_fraction(self):
        """The fraction of the frames in which the pixel was above the threshold."""
        self._need_frames()
        return self._numpy("hot").astype(np.float64) / self.n

    def level(self, k_sigma=4.0, margin=4):
        """clip(ceil(mean + k_sigma * std) + margin, 0, 255) as uint8: what a pixel has to exceed to be more than its background.
        The dot's own visits are part of the statistics: a pixel it lit once with the value v in n frames has about
        v (1 / n + k_sigma / sqrt(n)), which stays below v -- the dot passes its own level -- from some twenty frames on at
        k_sigma = 4; a video has thousands."""
        return np.clip(np.ceil(self.mean() + float(k_sigma) * self.std()) + margin, 0, 255).astype(np.uint8)

    def hot_mask(self, fraction=0.05, grow=0):
        """1 where the pixel was above the threshold in more than ``fraction`` of the frames (the dot passes, a lamp stays),
        dilated by ``disk(grow)``; uint8."""
        self._need_frames()
        mask = self._numpy("hot") > float(fraction) * self.n
        if grow:
            from scipy import ndimage
            r = int(grow)
            d = np.arange(-r, r + 1)
            mask = ndimage.binary_dilation(mask, structure=d[:, None] ** 2 + d[None, :] ** 2 <= r * r)
        return mask.astype(np.uint8)

    def suppress(self, frames, mode="gate", level=None, mask=None, out=None, chunk_frames=0, pixel_format=None, matrix="bt601"):
        """The model's channel of ``frames`` without the static light -> (B, H, W) uint8 on the side the frames are on.
        ``level`` / ``mask``: (H, W) planes, None = ``self.level()`` / ``self.hot_mask()`` with their defaults.  With a
        ``pixel_format`` the frames are YUV 4:2:0 as for ``add``: each chunk is converted to the model's plane on the device and
        the static light is taken out of that."""
        level = self.level() if level is None else level
        mask = self.hot_mask() if mask is None else mask
        if pixel_format is not None:
            L = _native._yuv_layout(frames, pixel_format, self.device)
            if out is None:
                if L.tensor:
                    import torch
                    out = torch.empty((L.n_frames, L.height, L.width), dtype=torch.uint8, device=f"cuda:{self.device}")
                else:
                    out = np.empty((L.n_frames, L.height, L.width), np.uint8)
            elif tuple(out.shape) != (L.n_frames, L.height, L.width):
                raise ValueError(f"out has the shape {tuple(out.shape)}, expected {(L.n_frames, L.height, L.width)}")
            if not _native._is_tensor(level) or not _native._is_tensor(mask):      # one upload for all chunks
                import torch
                level, mask = (a if _native._is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to(f"cuda:{self.device}")
                               for a in (level, mask))
            for lo, hi, plane in planes_in_chunks(frames, pixel_format, matrix, self.channel, chunk_frames, self.device):
                if _native._is_tensor(out):
                    _native.background_suppress(plane, level=level, mask=mask, mode=mode, channel=0, out=out[lo:hi], device=self.device)
                else:
                    out[lo:hi] = _native.background_suppress(plane, level=level, mask=mask, mode=mode, channel=0, device=self.device).cpu().numpy()
            return out
        return _native.background_suppress(frames, level=level, mask=mask, mode=mode, channel=self.channel, out=out,
                                           chunk_frames=chunk_frames, device=self.device)
