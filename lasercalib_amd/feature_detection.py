"""Laser-dot detection on the GPU: the first stage of the workflow (``lasercalib/feature_detection.py`` and
``scripts/detect_laser_points.py`` of the reference), on sba_detect_dots (include/sba_hip.h).

* :func:`green_laser_finder_faster` -- the reference's function (feature_detection.py:44-54), same signature and return value
* :func:`find_laser_dots`           -- the batched call: many frames, one pass, exact integer moments -> ``LaserDots``
* :func:`centroid_table`            -- the (n_frames, 2) array detect_laser_points.py:39-57 pickles, truncated like the
  reference's or sub-pixel
* :func:`green_laser_finder`        -- the reference's careful detector (feature_detection.py:6-40), same signature and return
  value, on sba_detect_blobs: threshold, dilation, closing, 8-connected components, "exactly one component"
* :func:`find_laser_blobs`          -- its batched call -> ``LaserBlobs``
* :func:`blob_centroid_table`       -- the (n_frames, 2) (row, col) table of the accepted components

The reference thresholds the green channel with ``cv.threshold(green, t, 255, 0)`` and takes ``cv.moments`` of the result:
m00 = 255 n, m10 = 255 sum x, m01 = 255 sum y over the n pixels above t, and returns ``(int(m01 / m00), int(m10 / m00))`` =
``(sum y // n, sum x // n)`` -- (row, col).  Video decoding stays with the caller; what the decoder produced -- YUV 4:2:0 -- can be passed as it is with
``pixel_format=`` (sba_convert_frames turns it into the detector's plane on the device).
"""
from __future__ import annotations

import numpy as np

from . import _native
from ._native import (BLOB_MULTIPLE, BLOB_NONE, BLOB_OK, BLOB_OVERFLOW, BLOB_REJECTED, DOT_NONE, DOT_OK, DOT_SPREAD,  # noqa: F401
                      DOT_TOO_LARGE, DOT_TOO_SMALL, LaserBlobs, LaserDots)

SBA_DOT_OK, SBA_DOT_NONE, SBA_DOT_TOO_SMALL, SBA_DOT_TOO_LARGE, SBA_DOT_SPREAD = DOT_OK, DOT_NONE, DOT_TOO_SMALL, DOT_TOO_LARGE, DOT_SPREAD
SBA_BLOB_OK, SBA_BLOB_NONE, SBA_BLOB_OVERFLOW, SBA_BLOB_REJECTED, SBA_BLOB_MULTIPLE = BLOB_OK, BLOB_NONE, BLOB_OVERFLOW, BLOB_REJECTED, BLOB_MULTIPLE

__all__ = ["green_laser_finder_faster", "find_laser_dots", "centroid_table", "LaserDots",
           "SBA_DOT_OK", "SBA_DOT_NONE", "SBA_DOT_TOO_SMALL", "SBA_DOT_TOO_LARGE", "SBA_DOT_SPREAD",
           "green_laser_finder", "find_laser_blobs", "blob_centroid_table", "disk", "LaserBlobs",
           "SBA_BLOB_OK", "SBA_BLOB_NONE", "SBA_BLOB_OVERFLOW", "SBA_BLOB_REJECTED", "SBA_BLOB_MULTIPLE"]


SUPPRESS_CHUNK_BYTES = 64 << 20     # one-channel frames held at a time when a background is taken out in front of a detector


def _level_and_mask(background, channel):
    """(level, mask) of an ``imaging.BackgroundModel`` built on ``channel`` or of a ``(level, mask)`` pair."""
    if hasattr(background, "suppress"):
        if background.channel != channel:
            raise ValueError(f"the background model was built on channel {background.channel}, the detector reads channel {channel}")
        return background.level(), background.hot_mask()
    level, mask = background
    return level, mask


def _join(parts, fields, make):
    return make(*(None if getattr(parts[0], f) is None else np.concatenate([getattr(p, f) for p in parts]) for f in fields))


def _without_background(frames, background, channel, chunk_frames, device, detect, fields, make):
    """Runs ``detect(one-channel frames)`` on the frames with the background taken out (gate mode), chunk by chunk, and joins
    the results' ``fields`` with ``make``.  ``background``: an ``imaging.BackgroundModel`` or a ``(level, mask)`` pair."""
    level, mask = _level_and_mask(background, channel)
    _t, frames, B, H, W, _C, _sr, _sf = _native._frame_layout(frames, device)
    step = int(chunk_frames) if chunk_frames > 0 else max(1, SUPPRESS_CHUNK_BYTES // max(1, H * W))
    parts = []
    for lo in range(0, max(B, 1), step):
        clean = _native.background_suppress(frames[lo:lo + step], level=level, mask=mask, mode="gate", channel=channel, device=device)
        parts.append(detect(clean))
    return _join(parts, fields, make)


def _from_decoder_frames(frames, pixel_format, matrix, background, channel, chunk_frames, device, detect, fields, make):
    """Runs ``detect(one-channel frames)`` on YUV 4:2:0 frames (``imaging.convert_frames`` describes them): chunk by chunk they are
    converted on the device to the plane ``channel`` names (0, 1, 2 = B, G, R; sba_convert_frames), the background, if any, is
    gated out of that plane, and the results' ``fields`` are joined with ``make``.  One chunk of one-channel frames is held on
    the device at a time, whatever the length of the video."""
    from . import imaging
    level, mask = (None, None) if background is None else _level_and_mask(background, channel)
    parts = []
    for _lo, _hi, plane in imaging.planes_in_chunks(frames, pixel_format, matrix, channel, chunk_frames, device):
        if background is not None:
            plane = _native.background_suppress(plane, level=level, mask=mask, mode="gate", channel=0, device=device)
        parts.append(detect(plane))
    return _join(parts, fields, make)


def find_laser_dots(frames, threshold=50, channel=1, min_area=0, max_area=0, max_extent=0, roi_rect=None, roi_circle=None,
                    chunk_frames=0, device=0, background=None, pixel_format=None, matrix="bt601") -> LaserDots:
    """Moments, bounding box, centroids and status of the laser dot of every frame of a batch: ``_native.detect_dots``.
    ``frames`` is a uint8 numpy array or a torch tensor on the device, (B, H, W, C) or (B, H, W); a single (H, W, C) frame has
    to be passed as ``frame[None]``.  ``max_extent`` rejects frames whose bright pixels do not fit a box of that size (status
    SPREAD): the one-pass stand-in for the one-connected-component rule of the reference's ``green_laser_finder``.
    ``background``: an ``imaging.BackgroundModel`` (its ``level()`` and ``hot_mask()``) or a ``(level, mask)`` pair of (H, W)
    planes; the static light is then gated out chunk by chunk (sba_background_suppress) and the detector reads the one-channel
    result, whose surviving pixels keep their values.
    ``pixel_format``: "nv12", "nv21", "i420" or "yv12" when ``frames`` are what the video decoder produced, 8-bit YUV 4:2:0 as
    ``imaging.convert_frames`` takes them (a tuple of planes or a stacked array, numpy or device tensors); they are converted on
    the device, chunk by chunk, to the plane ``channel`` names -- 0, 1, 2 = B, G, R, so that 1 stays green -- under ``matrix``."""
    if background is not None or pixel_format is not None:
        def detect(clean):
            return _native.detect_dots(clean, threshold=threshold, channel=0, min_area=min_area, max_area=max_area,
                                       max_extent=max_extent, roi_rect=roi_rect, roi_circle=roi_circle, device=device)
        fields = ("sums", "box", "centroid", "status")
        if pixel_format is not None:
            return _from_decoder_frames(frames, pixel_format, matrix, background, channel, chunk_frames, device, detect, fields, LaserDots)
        return _without_background(frames, background, channel, chunk_frames, device, detect, fields, LaserDots)
    return _native.detect_dots(frames, threshold=threshold, channel=channel, min_area=min_area, max_area=max_area,
                               max_extent=max_extent, roi_rect=roi_rect, roi_circle=roi_circle, chunk_frames=chunk_frames,
                               device=device)


def green_laser_finder_faster(frame, laser_intensity_thresh):
    """The reference's detector (feature_detection.py:44-54) on one (H, W, C >= 2) frame: ``(row, col)`` of the centroid of the
    pixels whose green channel (index 1) is above the threshold, truncated to whole pixels, or None when there is none."""
    frame = frame if _native._is_tensor(frame) else np.asarray(frame)
    if frame.ndim != 3 or frame.shape[2] not in (3, 4):
        raise ValueError("green_laser_finder_faster expects one (H, W, 3) or (H, W, 4) frame")
    dots = find_laser_dots(frame[None], threshold=laser_intensity_thresh, channel=1)
    n, sx, sy = (int(v) for v in dots.sums[0, :3])
    if n == 0:
        return None
    return (sy // n, sx // n)


def centroid_table(dots: LaserDots, subpixel=True, weighted=True, accept=(SBA_DOT_OK,)) -> np.ndarray:
    """The (n_frames, 2) float array the reference pickles per camera (detect_laser_points.py:39-57): one (row, col) per frame,
    NaN where the frame's status is not in ``accept`` -- get_points3d.py:48 flips it to (x, y) afterwards, as before.
    ``subpixel=False`` gives the reference's truncated integers (sum y // n, sum x // n); otherwise the float centroid,
    weighted by value - threshold or binary."""
    out = np.full((dots.status.shape[0], 2), np.nan)
    keep = np.isin(dots.status, np.asarray(accept, dtype=np.int32)) & (dots.sums[:, 0] > 0)
    if subpixel:
        cx, cy = (2, 3) if weighted else (0, 1)
        out[keep, 0], out[keep, 1] = dots.centroid[keep, cy], dots.centroid[keep, cx]
    else:
        n = dots.sums[keep, 0]
        out[keep, 0], out[keep, 1] = dots.sums[keep, 2] // n, dots.sums[keep, 1] // n
    return out


# ----------------------------------------------------------------------------- connected components (sba_detect_blobs)
def disk(radius):
    """``skimage.morphology.disk``: the (2 r + 1, 2 r + 1) uint8 footprint of the pixels with dx^2 + dy^2 <= r^2."""
    r = int(radius)
    d = np.arange(-r, r + 1)
    return (d[:, None] ** 2 + d[None, :] ** 2 <= r * r).astype(np.uint8)


def _disk_radius(footprint, default, name):
    """The r of a footprint equal to disk(r), r <= 8; ``default`` for None; ValueError for anything else."""
    if footprint is None:
        return default
    fp = np.asarray(footprint)
    if fp.ndim == 2 and fp.shape[0] == fp.shape[1] and fp.shape[0] % 2 == 1:
        r = fp.shape[0] // 2
        if r <= _native.BLOB_MAX_RADIUS and np.array_equal(fp != 0, disk(r) != 0):
            return r
    raise ValueError(f"{name} must be None or equal to disk(r) with r <= {_native.BLOB_MAX_RADIUS}: other footprints are not supported")


def find_laser_blobs(frames, threshold=70, channel=1, dilate_radius=1, close_radius=4, max_blobs=8, min_area=0, max_area=0,
                     centre=None, max_centre_dist=0, roi_rect=None, roi_circle=None, chunk_frames=0, device=0,
                     want_mask=False, want_labels=False, background=None, pixel_format=None, matrix="bt601") -> LaserBlobs:
    """The connected components of every frame of a batch and the verdict on each frame: ``_native.detect_blobs``.
    ``frames`` as for :func:`find_laser_dots`.  With the defaults (disk(1), disk(4), no filter) a frame's status is SBA_BLOB_OK
    exactly when the reference's ``green_laser_finder`` returns a centroid, and ``centroid[:, :2]`` is that centroid as (x, y).
    ``background``, ``pixel_format`` and ``matrix`` as for :func:`find_laser_dots`."""
    if background is not None or pixel_format is not None:
        def detect(clean):
            return _native.detect_blobs(clean, threshold=threshold, channel=0, dilate_radius=dilate_radius, close_radius=close_radius,
                                        max_blobs=max_blobs, min_area=min_area, max_area=max_area, centre=centre,
                                        max_centre_dist=max_centre_dist, roi_rect=roi_rect, roi_circle=roi_circle, device=device,
                                        want_mask=want_mask, want_labels=want_labels)
        fields = ("n_components", "blobs", "accepted", "centroid", "status", "mask", "labels")
        if pixel_format is not None:
            return _from_decoder_frames(frames, pixel_format, matrix, background, channel, chunk_frames, device, detect, fields, LaserBlobs)
        return _without_background(frames, background, channel, chunk_frames, device, detect, fields, LaserBlobs)
    return _native.detect_blobs(frames, threshold=threshold, channel=channel, dilate_radius=dilate_radius, close_radius=close_radius,
                                max_blobs=max_blobs, min_area=min_area, max_area=max_area, centre=centre,
                                max_centre_dist=max_centre_dist, roi_rect=roi_rect, roi_circle=roi_circle, chunk_frames=chunk_frames,
                                device=device, want_mask=want_mask, want_labels=want_labels)


def green_laser_finder(img, laser_intensity_thresh=70, centroid_dist_thresh=1100, small_footprint=None, big_footprint=None):
    """The reference's detector (feature_detection.py:6-40) on one (H, W, C >= 2) frame: the green channel above the threshold,
    ``binary_dilation`` with ``small_footprint``, ``binary_closing`` with ``big_footprint``, ``measure.label``; returns the float
    ``(row, col)`` centroid of the component (``regionprops(...).centroid``) when there is exactly one, else None.
    A footprint is None (disk(1) / disk(4), the reference's defaults) or an array equal to some ``disk(r)``, r <= 8; anything
    else raises ValueError.  ``centroid_dist_thresh`` is accepted and IGNORED, as in the reference, whose distance filter is
    commented out (:32-34); ``find_laser_blobs(..., centre=, max_centre_dist=)`` applies it.  The closing keeps a dot at the image
    border, as skimage >= 0.23 does (older versions wipe it)."""
    r1 = _disk_radius(small_footprint, 1, "small_footprint")
    r2 = _disk_radius(big_footprint, 4, "big_footprint")
    img = img if _native._is_tensor(img) else np.asarray(img)
    if img.ndim != 3 or img.shape[2] not in (3, 4):
        raise ValueError("green_laser_finder expects one (H, W, 3) or (H, W, 4) frame")
    blobs = find_laser_blobs(img[None], threshold=laser_intensity_thresh, channel=1, dilate_radius=r1, close_radius=r2, max_blobs=2)
    if blobs.n_components[0] != 1:
        return None
    return (float(blobs.centroid[0, 1]), float(blobs.centroid[0, 0]))


def blob_centroid_table(blobs: LaserBlobs, weighted=False) -> np.ndarray:
    """The (n_frames, 2) float (row, col) table of the accepted components, NaN rows where the status is not SBA_BLOB_OK:
    the centroid over the morphed pixels (the reference's ``regionprops`` centroid) or, ``weighted``, the one over the raw pixels
    weighted by value - threshold (NaN too where the component holds no raw pixel)."""
    out = np.full((blobs.status.shape[0], 2), np.nan)
    keep = blobs.status == SBA_BLOB_OK
    cx, cy = (2, 3) if weighted else (0, 1)
    out[keep, 0], out[keep, 1] = blobs.centroid[keep, cy], blobs.centroid[keep, cx]
    return out
