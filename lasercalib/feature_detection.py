"""``lasercalib.feature_detection`` -> the device detector of ``lasercalib_amd.feature_detection`` (no cv2, no skimage).

``green_laser_finder_faster`` and ``green_laser_finder`` (the connected-component detector) keep the reference's signatures
and return values.  Names this module does not define are looked up in the upstream file when LASERCALIB_UPSTREAM points at it.
"""
import importlib.util as _ilu
import os as _os

from lasercalib_amd.feature_detection import (  # noqa: F401
    SBA_BLOB_MULTIPLE, SBA_BLOB_NONE, SBA_BLOB_OK, SBA_BLOB_OVERFLOW, SBA_BLOB_REJECTED,
    SBA_DOT_NONE, SBA_DOT_OK, SBA_DOT_SPREAD, SBA_DOT_TOO_LARGE, SBA_DOT_TOO_SMALL, LaserBlobs, LaserDots, blob_centroid_table,
    centroid_table, find_laser_blobs, find_laser_dots, green_laser_finder, green_laser_finder_faster,
)

_upstream = None


def __getattr__(name):
    global _upstream
    up = _os.environ.get("LASERCALIB_UPSTREAM")
    path = _os.path.join(up, "feature_detection.py") if up else None
    if path and _os.path.isfile(path):
        if _upstream is None:
            spec = _ilu.spec_from_file_location("lasercalib._upstream_feature_detection", path)
            _upstream = _ilu.module_from_spec(spec)
            spec.loader.exec_module(_upstream)
        if hasattr(_upstream, name):
            return getattr(_upstream, name)
    raise AttributeError(f"module 'lasercalib.feature_detection' has no attribute {name!r}")
