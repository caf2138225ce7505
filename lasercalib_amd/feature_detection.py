"""Laser-dot detection on the GPU: the first stage of the workflow (``lasercalib/feature_detection.py`` and
``scripts/detect_laser_points.py`` of the reference), on sba_detect_dots (include/sba_hip.h).

* :func:`green_laser_finder_faster` -- the reference's function (feature_detection.py:44-54), same signature and return value
* :func:`find_laser_dots`           -- the batched call: many frames, one pass, exact integer moments -> ``LaserDots``
* :func:`centroid_table`            -- the (n_frames, 2) array detect_laser_points.py:39-57 pickles, truncated like the
  reference's or sub-pixel

The reference thresholds the green channel with ``cv.threshold(green, t, 255, 0)`` and takes ``cv.moments`` of the result:
m00 = 255 n, m10 = 255 sum x, m01 = 255 sum y over the n pixels above t, and returns ``(int(m01 / m00), int(m10 / m00))`` =
``(sum y // n, sum x // n)`` -- (row, col).  Video decoding stays with the caller.
"""
from __future__ import annotations

import numpy as np

from . import _native
from ._native import DOT_NONE, DOT_OK, DOT_SPREAD, DOT_TOO_LARGE, DOT_TOO_SMALL, LaserDots  # noqa: F401

SBA_DOT_OK, SBA_DOT_NONE, SBA_DOT_TOO_SMALL, SBA_DOT_TOO_LARGE, SBA_DOT_SPREAD = DOT_OK, DOT_NONE, DOT_TOO_SMALL, DOT_TOO_LARGE, DOT_SPREAD

__all__ = ["green_laser_finder_faster", "find_laser_dots", "centroid_table", "LaserDots",
           "SBA_DOT_OK", "SBA_DOT_NONE", "SBA_DOT_TOO_SMALL", "SBA_DOT_TOO_LARGE", "SBA_DOT_SPREAD"]


def find_laser_dots(frames, threshold=50, channel=1, min_area=0, max_area=0, max_extent=0, roi_rect=None, roi_circle=None,
                    chunk_frames=0, device=0) -> LaserDots:
    """Moments, bounding box, centroids and status of the laser dot of every frame of a batch: ``_native.detect_dots``.
    ``frames`` is a uint8 numpy array or a torch tensor on the device, (B, H, W, C) or (B, H, W); a single (H, W, C) frame has
    to be passed as ``frame[None]``.  ``max_extent`` rejects frames whose bright pixels do not fit a box of that size (status
    SPREAD): the one-pass stand-in for the one-connected-component rule of the reference's ``green_laser_finder``."""
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
