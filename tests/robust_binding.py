"""ctypes binding of robust accumulation's checker (tests/build/librobust_oracle.so, tests/cpp/robust_oracle.cpp).
TEST INFRASTRUCTURE.

The checker restates include/rtc.h's contract of rtc_robust_device as plain loops in doubles.  No library
function is involved, so every comparison with the kernels is of bits.  bucket_sums() deals frames to buckets as the contract
does (pass p into bucket p % M, in order); robust() resolves them; speck_share() and rmse() are the measures the fixture
robust_lamp.json is held to.
"""
import ctypes as C
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBUST_SO = os.path.join(REPO, "tests", "build", "librobust_oracle.so")
ROBUST_LAMP = os.path.join(REPO, "tests", "golden", "robust_scenes", "robust_lamp.json")
DEFAULTS = {"buckets": 5, "gain": 1.0}

_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(ROBUST_SO)
        l.robust_oracle.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]
        l.robust_oracle_rgba.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        l.robust_oracle_rgba.restype = None
        _lib = l
    return _lib


def bucket_sums(frames, buckets):
    """frames: a sequence of P arrays of one shape [...][3]; -> [M][...][3]: bucket p % M holds the in-order sum of its frames"""
    sums = [None] * buckets
    for p, frame in enumerate(frames):
        j = p % buckets
        sums[j] = np.array(frame, dtype=np.float64) if sums[j] is None else sums[j] + frame
    return np.stack(sums)


def robust(sums, passes, gain=1.0):
    """sums [M][...][3] -> dict(mean [...][3], sumsq [...], rejected [...] u32, gini [...] (G0), variance [...] (v))"""
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    M, shape = sums.shape[0], sums.shape[1:-1]
    assert sums.shape[-1] == 3
    n = int(np.prod(shape, dtype=np.int64))
    out = {"mean": np.empty(shape + (3,)), "sumsq": np.empty(shape), "rejected": np.empty(shape, dtype=np.uint32),
           "gini": np.empty(shape), "variance": np.empty(shape)}
    st = lib().robust_oracle(sums.ctypes.data, n, passes, M, gain, out["mean"].ctypes.data, out["sumsq"].ctypes.data,
                             out["rejected"].ctypes.data, out["gini"].ctypes.data, out["variance"].ctypes.data)
    if st != 0:
        raise ValueError("robust checker: an argument the contract refuses")
    return out


def rgba(image):
    """[...] u32: the clamp of image [...][3]"""
    image = np.ascontiguousarray(image, dtype=np.float64)
    px = np.empty(image.shape[:-1], dtype=np.uint32)
    lib().robust_oracle_rgba(image.ctypes.data, px.size, px.ctypes.data)
    return px


def luminance(image):
    return (0.2126 * image[..., 0] + 0.7152 * image[..., 1]) + 0.0722 * image[..., 2]


def speck_share(image):
    """the share of an image's pixels whose luminance exceeds 4 times the median of their 3 x 3 neighbourhood (the pixel
    itself included; the neighbourhood is cut at the image's edges)"""
    y = luminance(np.asarray(image, dtype=np.float64))
    h, w = y.shape
    padded = np.full((h + 2, w + 2), np.nan)
    padded[1:-1, 1:-1] = y
    stack = np.stack([padded[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    return float((y > 4.0 * np.nanmedian(stack, axis=0)).mean())


def rmse(image, truth):
    return float(np.sqrt(np.mean((np.asarray(image, dtype=np.float64) - truth) ** 2)))
