"""ctypes binding of include/molahip_live.h: the view of a device-resident scan, see-through votes on the stored records of a
live map and the erasing of flagged points.  The library is capi's; this module holds the signature table of
the third public header and thin wrappers for tests and tools."""
import ctypes as C
import os
import re

import numpy as np

from . import capi, capi_clean
from .capi import MEM_DEVICE, MEM_HOST, Map, Scan, _chk, _vp
from .capi_clean import Views

LIVE_API_VERSION = 1
MAX_VIEWS = 64

_SIGNATURES = {
    "mh_live_api_version": (C.c_uint32, []),
    "mh_views_put_scan": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "mh_views_vote_map": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32]),
    "mh_map_erase_points": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32]),
    "mh_map_erase_seen_through": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "mh_map_erased_total": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64)]),
}

_lib = None


def lib():
    """capi's library with the signatures of molahip_live.h (and molahip_clean.h) set.  Raises if the library is absent or lacks
    the surface."""
    global _lib
    if _lib is None:
        L = capi_clean.lib()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        want = _header_api_version()
        if want is not None and int(L.mh_live_api_version()) != want:
            raise OSError(f"{capi.LIB_PATH} speaks live-cleaning API version {int(L.mh_live_api_version())}, "
                          f"include/molahip_live.h says {want}: rebuild")
        _lib = L
    return _lib


def _header_api_version():
    h = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "molahip_live.h")
    try:
        m = re.search(r"^#define\s+MH_LIVE_API_VERSION\s+(\d+)", open(h).read(), re.M)
    except OSError:
        return None
    return int(m.group(1)) if m else None


def _nbr(nbr_view, nbr_T):
    view = np.ascontiguousarray(np.asarray(nbr_view, np.uint32).reshape(-1))
    T = np.ascontiguousarray(np.asarray(nbr_T, np.float64).reshape(-1))
    assert len(T) == 12 * len(view)
    return view, T


def put_scan(views: Views, slot: int, scan: Scan):
    """mh_views_put_scan: the view of a device-resident scan into `slot` (len(views) appends)."""
    _chk(lib().mh_views_put_scan(views._h, int(slot), scan._h))


def vote_map(views: Views, m: Map, nbr_view, nbr_T, capacity=None):
    """mh_views_vote_map: uint32 [n_points], through | agree << 16 per stored point in download order."""
    view, T = _nbr(nbr_view, nbr_T)
    n = int(m.info().n_points)
    cap = n if capacity is None else int(capacity)
    out = np.zeros(max(cap, 1), np.uint32)
    _chk(lib().mh_views_vote_map(views._h, m._h, len(view), _vp(view), _vp(T), _vp(out), cap, MEM_HOST))
    return out[:n]


def vote_map_device(views: Views, m: Map, nbr_view, nbr_T, votes_ptr: int, capacity: int):
    """The same into the device array at votes_ptr (room for `capacity` words)."""
    view, T = _nbr(nbr_view, nbr_T)
    _chk(lib().mh_views_vote_map(views._h, m._h, len(view), _vp(view), _vp(T), C.c_void_p(votes_ptr), int(capacity), MEM_DEVICE))


def erase_points(m: Map, drop):
    """mh_map_erase_points: drop[i] != 0 removes stored point i (download order)."""
    d = np.ascontiguousarray(np.asarray(drop).astype(np.uint8).reshape(-1))
    _chk(lib().mh_map_erase_points(m._h, _vp(d), len(d), MEM_HOST))


def erase_points_device(m: Map, drop_ptr: int, n: int):
    _chk(lib().mh_map_erase_points(m._h, C.c_void_p(drop_ptr), int(n), MEM_DEVICE))


def erase_seen_through(m: Map, views: Views, nbr_view, nbr_T, min_through_votes=2, agree_weight=1):
    """mh_map_erase_seen_through: vote, decide and erase on the device; queued."""
    view, T = _nbr(nbr_view, nbr_T)
    _chk(lib().mh_map_erase_seen_through(m._h, views._h, len(view), _vp(view), _vp(T), int(min_through_votes), int(agree_weight)))


def erased_total(m: Map) -> int:
    n = C.c_uint64(0)
    _chk(lib().mh_map_erased_total(m._h, C.byref(n)))
    return int(n.value)
