"""ctypes binding of the film stage's checker (tests/build/libfilm_oracle.so, tests/cpp/film_oracle.cpp).
TEST INFRASTRUCTURE.

The checker restates include/rtc.h's contract of rtc_film_device as plain loops in doubles.  film() takes
an image [h][w][3] and rtc_film_setting's fields as keywords (DEFAULTS where absent) and returns (out, E); `E`, where given,
is used in place of the checker's own exposure.  The tolerance of a comparison that involves exp, log or pow is
TOL * max(1, |value|) per channel (denoise_binding's); without them the bits are equal.
"""
import ctypes as C
import os

import numpy as np

from denoise_binding import TOL, close  # noqa: F401  (the project's tolerance and its comparison)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILM_SO = os.path.join(REPO, "tests", "build", "libfilm_oracle.so")
FILM_LAMP = os.path.join(REPO, "tests", "golden", "film_scenes", "film_lamp.json")
LINEAR, REINHARD, ACES, HABLE = 0, 1, 2, 3          # RTC_FILM_CURVE_*
T_LINEAR, T_SRGB, T_GAMMA = 0, 1, 2                 # RTC_FILM_TRANSFER_*
DEFAULTS = {"exposure": 1.0, "auto_key": 0.0, "bloom_radius": 0, "bloom_sigma": 4.0, "bloom_threshold": 1.0, "bloom_intensity": 0.0,
            "curve": ACES, "white": 4.0, "transfer": T_SRGB, "gamma": 2.2}
BLOOM = {"bloom_radius": 12, "bloom_sigma": 4.0, "bloom_threshold": 1.0, "bloom_intensity": 0.15}   # ("bloom": true)
IDENTITY = dict(DEFAULTS, curve=LINEAR, transfer=T_LINEAR)

_lib = None


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(FILM_SO)
        l.film_oracle.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_uint32, C.c_double, C.c_double, C.c_double,
                                  C.c_uint32, C.c_double, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        l.film_oracle_develop.argtypes = [C.c_uint32, C.c_double, C.c_uint32, C.c_double, C.c_double]
        l.film_oracle_develop.restype = C.c_double
        l.film_oracle_weights.argtypes = [C.c_uint32, C.c_double, C.c_void_p]
        l.film_oracle_rgba.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        l.film_oracle_rgba.restype = None
        _lib = l
    return _lib


def film(image, E=None, **setting):
    """-> (out [h][w][3] f64, the E used)"""
    image = np.ascontiguousarray(image, dtype=np.float64)
    h, w, three = image.shape
    assert three == 3
    s = dict(DEFAULTS)
    assert set(setting) <= set(s), setting
    s.update(setting)
    out = np.empty_like(image)
    given = C.c_double(E) if E is not None else None
    used = C.c_double()
    st = lib().film_oracle(image.ctypes.data, w, h, s["exposure"], s["auto_key"], s["bloom_radius"], s["bloom_sigma"], s["bloom_threshold"],
                           s["bloom_intensity"], s["curve"], s["white"], s["transfer"], s["gamma"],
                           C.addressof(given) if given is not None else None, out.ctypes.data, C.addressof(used))
    if st != 0:
        raise ValueError("film checker: an argument the contract refuses")
    return out, used.value


def develop(c, curve=LINEAR, white=4.0, transfer=T_LINEAR, gamma=2.2):
    """one channel through the curve and the transfer"""
    return lib().film_oracle_develop(curve, white, transfer, gamma, c)


def weights(radius, sigma):
    g = np.empty(radius + 1)
    assert lib().film_oracle_weights(radius, sigma, g.ctypes.data) == 0
    return g


def rgba(out):
    """[h][w] u32: the clamp of out"""
    out = np.ascontiguousarray(out, dtype=np.float64)
    px = np.empty(out.shape[:2], dtype=np.uint32)
    lib().film_oracle_rgba(out.ctypes.data, px.size, px.ctypes.data)
    return px


def share_at_255(px):
    """the share of an rgba image's colour channels at 255"""
    b = np.ascontiguousarray(px).view(np.uint8).reshape(-1, 4)[:, :3]
    return float((b == 255).mean())
