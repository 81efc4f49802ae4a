"""ctypes binding of the denoiser's checker (tests/build/libdenoise_oracle.so, tests/cpp/denoise_oracle.cpp).
TEST INFRASTRUCTURE.

The checker restates include/rtc.h's contract of rtc_denoise_device as plain loops in doubles.
denoise() takes the mean [h][w][3], the sums of squares [h][w] and either `passes` or (`tile_passes`, `tile`); `flags` selects
a variant for the tests that show a mistake missing its bound: NO_CANCEL (a distance without the c3 term).  accumulate() is the
accumulation's arithmetic on the host: what a list of passes leaves in mean and sumsq.  The tolerance of every comparison with the GPU is TOL * max(1, |value|) per channel.
"""
import ctypes as C
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENOISE_SO = os.path.join(REPO, "tests", "build", "libdenoise_oracle.so")
NO_CANCEL = 1
DEFAULTS = {"radius": 7, "patch": 2, "strength": 0.45, "cancel": 1.0}
TOL = 1e-12

_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(DENOISE_SO)
        l.denoise_oracle.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                     C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_uint32, C.c_uint32, C.c_void_p]
        l.denoise_oracle_flags.restype = C.c_uint32
        assert l.denoise_oracle_flags() == NO_CANCEL
        _lib = l
    return _lib


def denoise(mean, sumsq, passes=0, tile_passes=None, tile=(0, 0), radius=7, patch=2, strength=0.45, cancel=1.0, flags=0, threads=0):
    """-> [h][w][3] f64"""
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    sumsq = np.ascontiguousarray(sumsq, dtype=np.float64)
    h, w = sumsq.shape
    assert mean.shape == (h, w, 3)
    tp = None if tile_passes is None else np.ascontiguousarray(tile_passes, dtype=np.uint32)
    if tp is not None:
        assert len(tp) == (-(-w // tile[0])) * (-(-h // tile[1]))
    out = np.empty_like(mean)
    st = lib().denoise_oracle(mean.ctypes.data, sumsq.ctypes.data, w, h, passes, tp.ctypes.data if tp is not None else None, tile[0], tile[1],
                              radius, patch, strength, cancel, flags, threads, out.ctypes.data)
    if st != 0:
        raise ValueError("denoise checker: an argument the contract refuses")
    return out


def accumulate(frames):
    """(mean, sumsq) of a list of [h][w][3] passes, in rtc_accum's order of operations: the sums in pass order, one divide"""
    total = np.zeros_like(frames[0])
    sumsq = np.zeros(frames[0].shape[:2])
    for f in frames:
        total = total + f
        sumsq = sumsq + ((f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]) + f[..., 2] * f[..., 2])
    return total / float(len(frames)), sumsq


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a) - np.asarray(b)) ** 2)))


def close(got, want):
    """max over channels of |got - want| / max(1, |want|), and whether it is within TOL (non-finite values must agree in kind)"""
    got, want = np.asarray(got), np.asarray(want)
    finite = np.isfinite(want)
    if not np.array_equal(finite, np.isfinite(got)):
        return float("inf"), False
    if not finite.any():
        return 0.0, True
    err = float((np.abs(got[finite] - want[finite]) / np.maximum(1.0, np.abs(want[finite]))).max())
    return err, err <= TOL
