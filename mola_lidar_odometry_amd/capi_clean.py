"""ctypes binding of include/molahip_clean.h: views of key-frames and see-through votes.  The library is
capi's; this module holds the signature table of the second public header and thin wrappers for tests and tools."""
import ctypes as C
import os
import re

import numpy as np

from . import capi
from .capi import MEM_DEVICE, MEM_HOST, Context, MapFrame, _chk, _soa, _vp

CLEAN_API_VERSION = 1
EMPTY = 0xFFFFFFFF


class CleanParams(C.Structure):
    """mh_clean_params: rings x sectors of a view, its elevation window (radians) and range shell, the see-through margin,
    the sensor's position in the vehicle frame and the window half-widths."""
    _fields_ = [("n_rings", C.c_uint32), ("n_sectors", C.c_uint32), ("el_min", C.c_float), ("el_max", C.c_float),
                ("min_range", C.c_float), ("max_range", C.c_float), ("rel_margin", C.c_float), ("origin", C.c_float * 3),
                ("win_rings", C.c_uint32), ("win_sectors", C.c_uint32)]


_SIGNATURES = {
    "mh_clean_api_version": (C.c_uint32, []),
    "mh_views_create": (C.c_int32, [C.c_void_p, C.POINTER(CleanParams), C.POINTER(C.c_void_p)]),
    "mh_views_destroy": (C.c_int32, [C.c_void_p]),
    "mh_views_size": (C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "mh_views_add_frames": (C.c_int32, [C.c_void_p, C.POINTER(MapFrame), C.c_size_t, C.c_int32, C.c_uint64]),
    "mh_views_download": (C.c_int32, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "mh_views_vote_frames": (C.c_int32, [C.c_void_p, C.POINTER(MapFrame), C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_int32, C.c_uint64]),
}

_lib = None


def lib():
    """capi's library with the signatures of molahip_clean.h set.  Raises if the library is absent or lacks the surface."""
    global _lib
    if _lib is None:
        L = capi.lib()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        want = _header_api_version()
        if want is not None and int(L.mh_clean_api_version()) != want:
            raise OSError(f"{capi.LIB_PATH} speaks cleaning API version {int(L.mh_clean_api_version())}, "
                          f"include/molahip_clean.h says {want}: rebuild")
        _lib = L
    return _lib


def _header_api_version():
    h = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "molahip_clean.h")
    try:
        m = re.search(r"^#define\s+MH_CLEAN_API_VERSION\s+(\d+)", open(h).read(), re.M)
    except OSError:
        return None
    return int(m.group(1)) if m else None


def clean_params(n_rings=32, n_sectors=128, el_min=float(np.radians(-25.0)), el_max=float(np.radians(15.0)), min_range=2.0,
                 max_range=60.0, rel_margin=0.10, origin=(0.0, 0.0, 0.0), win_rings=0, win_sectors=1) -> CleanParams:
    return CleanParams(int(n_rings), int(n_sectors), el_min, el_max, min_range, max_range, rel_margin, (C.c_float * 3)(*origin),
                       int(win_rings), int(win_sectors))


def _frames(frames):
    keep = [_soa(xyz) for xyz in frames]
    arr = (MapFrame * max(len(keep), 1))()
    for e, (x, y, z) in zip(arr, keep):
        e.x, e.y, e.z, e.n = _vp(x), _vp(y), _vp(z), len(x)
    return keep, arr


class Views:
    """A store of key-frame views on one context's device (mh_views)."""

    def __init__(self, ctx: Context, params: CleanParams):
        self.ctx = ctx
        self.params = params
        self._h = C.c_void_p()
        _chk(lib().mh_views_create(ctx._h, C.byref(params), C.byref(self._h)))
        ctx._children.add(self)

    def __len__(self):
        n = C.c_uint64(0)
        _chk(lib().mh_views_size(self._h, C.byref(n)))
        return int(n.value)

    def add_frames(self, frames, max_points_per_pass=0):
        """One view per frame (mh_views_add_frames): `frames` is a sequence of xyz [n, 3]."""
        keep, arr = _frames(frames)
        _chk(lib().mh_views_add_frames(self._h, arr, len(keep), MEM_HOST, int(max_points_per_pass)))
        return self

    def add_frames_device(self, frames, max_points_per_pass=0):
        """The same from device arrays: `frames` is a sequence of (x_ptr, y_ptr, z_ptr, n)."""
        frames = list(frames)
        arr = (MapFrame * max(len(frames), 1))()
        for e, (xp, yp, zp, n) in zip(arr, frames):
            e.x, e.y, e.z, e.n = xp, yp, zp, int(n)
        _chk(lib().mh_views_add_frames(self._h, arr, len(frames), MEM_DEVICE, int(max_points_per_pass)))
        return self

    def download(self, first=0, n=None):
        """uint32 [n, n_rings, n_sectors] (mh_views_download)."""
        n = len(self) - first if n is None else int(n)
        out = np.zeros((max(n, 1), self.params.n_rings, self.params.n_sectors), np.uint32)
        _chk(lib().mh_views_download(self._h, int(first), n, _vp(out)))
        return out[:n]

    def vote_frames(self, frames, nbr_view, nbr_T, max_points_per_pass=0):
        """mh_views_vote_frames: `frames` a sequence of xyz [n, 3]; nbr_view[f] the view indices frame f votes against and
        nbr_T[f] their poses T_j^-1 T_i ([k, 12] or [k, 3, 4]).  Returns one uint32 array of packed votes per frame."""
        keep, arr = _frames(frames)
        start = np.zeros(len(keep) + 1, np.uint32)
        start[1:] = np.cumsum([len(v) for v in nbr_view])
        view = np.ascontiguousarray(np.concatenate([np.asarray(v, np.uint32).reshape(-1) for v in nbr_view] + [np.zeros(0, np.uint32)]))
        T = np.ascontiguousarray(np.concatenate([np.asarray(t, np.float64).reshape(-1) for t in nbr_T] + [np.zeros(0)]))
        assert len(T) == 12 * len(view)
        sizes = [len(x) for x, _, _ in keep]
        out = np.zeros(max(sum(sizes), 1), np.uint32)
        _chk(lib().mh_views_vote_frames(self._h, arr, len(keep), _vp(start), _vp(view), _vp(T), _vp(out), MEM_HOST,
                                        int(max_points_per_pass)))
        return np.split(out[:sum(sizes)], np.cumsum(sizes)[:-1]) if sizes else []

    def vote_frames_device(self, frames, nbr_view, nbr_T, votes_ptr: int, max_points_per_pass=0):
        """The same from device arrays: `frames` is a sequence of (x_ptr, y_ptr, z_ptr, n); the packed votes of all points go to
        the device array at votes_ptr, frame after frame.  The neighbour list stays in host memory."""
        frames = list(frames)
        arr = (MapFrame * max(len(frames), 1))()
        for e, (xp, yp, zp, n) in zip(arr, frames):
            e.x, e.y, e.z, e.n = xp, yp, zp, int(n)
        start = np.zeros(len(frames) + 1, np.uint32)
        start[1:] = np.cumsum([len(v) for v in nbr_view])
        view = np.ascontiguousarray(np.concatenate([np.asarray(v, np.uint32).reshape(-1) for v in nbr_view] + [np.zeros(0, np.uint32)]))
        T = np.ascontiguousarray(np.concatenate([np.asarray(t, np.float64).reshape(-1) for t in nbr_T] + [np.zeros(0)]))
        assert len(T) == 12 * len(view)
        _chk(lib().mh_views_vote_frames(self._h, arr, len(frames), _vp(start), _vp(view), _vp(T), C.c_void_p(votes_ptr), MEM_DEVICE,
                                        int(max_points_per_pass)))

    def close(self):
        if self._h:
            if self.ctx._h:
                lib().mh_views_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
