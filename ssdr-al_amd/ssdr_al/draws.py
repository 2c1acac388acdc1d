"""The tile generators' per-row randomness, drawn on the device (csrc/draw.hip; the chain is stated in include/ssdr_al.h and in DESIGN.md
section 24): shuffle permutations, padding draws and augmentation noise as pure functions of (seed, epoch, step, kind, element).  The wrappers
only enqueue on ``stream``; ``out`` (a DevArray of the right size) is filled in place when given."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DevArray

PERM, DUP, AUG_NOISE = 0, 1, 2          # SSDR_DRAW_*: the `kind` word of the counter

_M32 = 0xffffffff


def _bind(L):
    if getattr(L, "_draw_bound", False):
        return L
    vp, sz, i32, u32, u64 = C.c_void_p, C.c_size_t, C.c_int, C.c_uint32, C.c_uint64
    L.ssdr_draw_perm_dev.argtypes = [u64, u32, u32, u64, sz, sz, i32, vp, vp]
    L.ssdr_draw_uniform_dev.argtypes = [u64, u32, u32, u32, u64, sz, vp, vp]
    L.ssdr_draw_normal_dev.argtypes = [u64, u32, u32, u32, u64, sz, C.c_double, vp, vp]
    L._draw_bound = True
    return L


def _out(out, shape, dtype):
    if out is None:
        return DevArray(shape, dtype)
    if out.dtype != np.dtype(dtype) or out.nbytes < int(np.prod(shape)) * np.dtype(dtype).itemsize:
        raise ValueError("draws: out must be a %s DevArray of at least %s elements" % (np.dtype(dtype).name, shape))
    return out


def perm(seed, epoch, step, num_tiles, num_points, first_tile=0, key_bits=32, out=None, stream=None):
    """int32 [num_tiles, num_points]: row t = the stable argsort of the hashed keys of tile first_tile + t"""
    out = _out(out, (num_tiles, num_points), np.int32)
    L = _bind(_lib.lib())
    _lib.check(L.ssdr_draw_perm_dev(int(seed), int(epoch) & _M32, int(step) & _M32, int(first_tile), int(num_tiles), int(num_points), int(key_bits),
                                    out.ptr, stream))
    return out


def uniform(seed, epoch, step, kind, n, first=0, out=None, stream=None):
    """float32 [n] in [0, 1 - 2^-24]: elements first .. first + n - 1"""
    out = _out(out, (n,), np.float32)
    L = _bind(_lib.lib())
    _lib.check(L.ssdr_draw_uniform_dev(int(seed), int(epoch) & _M32, int(step) & _M32, int(kind), int(first), int(n), out.ptr, stream))
    return out


def normal(seed, epoch, step, kind, n, scale=1.0, first=0, out=None, stream=None):
    """float64 [n] = scale * standard normal (Box-Muller): elements first .. first + n - 1"""
    out = _out(out, (n,), np.float64)
    L = _bind(_lib.lib())
    _lib.check(L.ssdr_draw_normal_dev(int(seed), int(epoch) & _M32, int(step) & _M32, int(kind), int(first), int(n), float(scale), out.ptr, stream))
    return out
