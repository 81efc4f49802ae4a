"""The simple kernels skip the specular power in a wave none of whose lanes needs it: a lane whose material has `specular` zero
and an integer shininess keeps ks = specular at a base in (0, 1] (`ks_is_specular`, csrc/rtc_kernels.hip; the arithmetic
argument is held in tests/test_specular_skip_cpu.py).  Here small worlds against the oracle's image and ray counters, through
the five kernels that carry the skip - rtc_render_kernel_simple_b, _simple3_b, _simple, _simple3, pinned as
tests/test_cube_behind_gpu.py pins them, and _simple_ext (the floor slab given a texture map) - and one that does not
(rtc_render_kernel_flat: a cylinder added).

  mixed     cubes with specular 0 / shininess 200, a glass sphere with specular 1 / shininess 200 whose highlight is in view
            (test_the_highlight_is_in_view), a cube with specular 0.3 / shininess 10, a backdrop plane with diffuse 0,
            specular 0, ambient 1 (cover.json's), two point lights; the sphere fills a corner of the image, so that some waves
            hold specular-zero lanes only and others both kinds.
  one_lane  the same world at 8 x 8: cooperative iterations on the two-wave kernels.
  fallback  a specular-zero sphere with shininess 199.5 and one with shininess -2000: both take zig_pow's path.  On the second the
            reference multiplies the zero by an overflowed power wherever 0 < reflect_dot_eye < 2^(-1024/2000) = 0.701: NaN
            pixels, beside finite ones on the same sphere (test_the_fallback_sphere_is_half_nan holds the oracle to that); the
            GPU image is NaN in exactly those pixels.
  negzero   specular -0.0 on the cubes, a light with a negative intensity component.  (The signs of zeros are held by the CPU
            test; the image shows a wrong product.)
"""
import json

import numpy as np
import pytest

import oracle_binding as ob

pytestmark = pytest.mark.gpu

# (tests/test_containers_gpu.py: the same arithmetic in the same order but for pixels whose ray tree is shared between lanes - a
# few roundings of 2^-53 on colours of order one; a highlight wrongly dropped or a zero wrongly kept changes a pixel by 1e-3 or more)
TOL = 1e-12
DEPTH = 5

OPTIONS = ("box_cull", "simple3_min_chunks")
# variant -> [(options, kernel)]; an option not named is the library's own choice (-1)
FORMS = {
    "simple": [({"box_cull": 1, "simple3_min_chunks": 1e9}, "rtc_render_kernel_simple_b"), ({"box_cull": 1, "simple3_min_chunks": 0}, "rtc_render_kernel_simple3_b"),
               ({"box_cull": 0, "simple3_min_chunks": 1e9}, "rtc_render_kernel_simple"), ({"box_cull": 0, "simple3_min_chunks": 0}, "rtc_render_kernel_simple3")],
    "textured": [({}, "rtc_render_kernel_simple_ext")],   # the simple kernel with texture maps: carries the skip
    "flat": [({}, "rtc_render_kernel_flat")],             # does not
}
CHECKERS_MAP = {"type": {"texture-map": {"planar": {"uv-pattern": {"checkers": {"width": 2, "height": 2, "patterns": [
    {"type": {"solid": [0.4, 0.6, 0.4]}}, {"type": {"solid": [0.2, 0.3, 0.5]}}]}}}}}}

GLASS = {"diffuse": 0.2, "ambient": 0.0, "specular": 1, "shininess": 200, "reflective": 0.7, "transparency": 0.7, "refractive-index": 1.5}
FALLBACK_CENTRE, FALLBACK_RADIUS = (1.2, 1.0, -1.0), 1.0


def _cube(transform, colour, **material):
    return {"type": {"cube": {}}, "transform": transform,
            "material": dict({"pattern": {"type": {"solid": colour}}, "ambient": 0.1, "diffuse": 0.7, "specular": 0, "shininess": 200,
                              "reflective": 0.1}, **material)}


def _backdrop():
    return {"type": {"plane": {}}, "transform": [{"rotate-x": 1.5707963267948966}, {"translate": [0, 0, 30]}],
            "material": {"pattern": {"type": {"solid": [1, 1, 1]}}, "ambient": 1, "diffuse": 0, "specular": 0}}


def _mixed(width=64, height=48, specular=0, sphere_specular=1, intensity=(1.0, 1.0, 1.0)):
    objs = [
        _cube([{"translate": [-2.5, 1, 0]}], [1, 1, 1], specular=specular),
        _cube([{"scale": [0.8, 0.8, 0.8]}, {"rotate-y": 0.5}, {"translate": [-0.2, 0.8, 1.5]}], [0.9, 0.3, 0.3], specular=specular),
        _cube([{"scale": [3, 0.2, 3]}, {"translate": [-0.5, -0.2, 0]}], [0.4, 0.6, 0.4], specular=specular, reflective=0.3),
        _cube([{"scale": [0.6, 1.4, 0.6]}, {"rotate-y": -0.3}, {"translate": [-4.4, 1.4, 2]}], [0.3, 0.4, 0.9], specular=specular),
        _cube([{"scale": [0.7, 0.7, 0.7]}, {"translate": [0.6, 0.7, -1.6]}], [0.9, 0.8, 0.2], specular=0.3, shininess=10),
        {"type": {"sphere": {}}, "transform": [{"scale": [1.3, 1.3, 1.3]}, {"translate": [2.9, 1.3, -0.5]}],
         "material": dict(GLASS, specular=sphere_specular, pattern={"type": {"solid": [0.373, 0.404, 0.55]}})},
    ]
    lights = [{"point-light": {"position": [10, 12, -10], "intensity": list(intensity)}},
              {"point-light": {"position": [-12, 6, -8], "intensity": [0.2, 0.2, 0.2]}}]
    camera = {"width": width, "height": height, "field-of-view": 0.9, "from": [0.5, 4, -9], "to": [0, 0.8, 0], "up": [0, 1, 0]}
    return camera, lights, objs + [_backdrop()]


def _fallback():
    camera, lights, objs = _mixed()
    objs = objs[:4] + [_backdrop()]
    objs.append({"type": {"sphere": {}}, "transform": [{"translate": list(FALLBACK_CENTRE)}],      # nothing between it and the camera
                 "material": {"pattern": {"type": {"solid": [0.8, 0.8, 0.3]}}, "diffuse": 0.6, "specular": 0, "shininess": -2000}})
    objs.append({"type": {"sphere": {}}, "transform": [{"scale": [0.7, 0.7, 0.7]}, {"translate": [3.4, 0.7, 0.5]}],
                 "material": {"pattern": {"type": {"solid": [0.3, 0.8, 0.8]}}, "diffuse": 0.6, "specular": 0, "shininess": 199.5}})
    return camera, lights, objs


WORLDS = {
    "mixed": _mixed,
    "one_lane": lambda: _mixed(8, 8),
    "fallback": _fallback,
    "negzero": lambda: _mixed(specular=-0.0, intensity=(0.8, -0.3, 0.5)),
}
_oracle = {}


def _scene(rtc, world, variant="simple"):
    """-> (HostScene, camera, the oracle's image and counters: computed once per world and variant, shared and left unchanged)"""
    key = (world, variant)
    if key not in _oracle:
        camera, lights, objs = WORLDS[world]()
        if variant == "textured":   # the floor slab (specular 0, shininess 200) with a texture map
            objs[2] = dict(objs[2], material=dict(objs[2]["material"], pattern=CHECKERS_MAP))
        elif variant == "flat":     # a leaf kind the simple kernels do not carry
            objs = objs + [{"type": {"cylinder": {"min": -1, "max": 1, "closed": True}}, "transform": [{"scale": [0.3, 0.5, 0.3]}, {"translate": [-1.2, 0.5, -2.5]}],
                            "material": {"diffuse": 0.7, "specular": 0, "shininess": 200}}]
        hs = rtc.HostScene(json.dumps({"camera": camera, "lights": lights, "objects": objs}))
        cam = hs.camera()
        want, counters = ob.OracleScene(hs.desc).render(cam, DEPTH)
        want.setflags(write=False)
        _oracle[key] = (hs, cam, want, counters)
    return _oracle[key]


def _on_fallback_sphere(cam):
    """pixels whose camera ray meets the shininess -2000 sphere well inside its outline (camera.zig's ray, a sphere test in numpy)"""
    inv = np.array(list(cam.inv_view)).reshape(4, 4)
    px, py = np.meshgrid(np.arange(cam.hsize), np.arange(cam.vsize))
    wx = cam.half_width - (px + 0.5) * cam.pixel_size
    wy = cam.half_height - (py + 0.5) * cam.pixel_size
    pixel = np.stack([wx, wy, -np.ones_like(wx), np.ones_like(wx)], axis=-1) @ inv.T
    origin = (inv @ np.array([0.0, 0.0, 0.0, 1.0]))[:3]
    d = pixel[..., :3] - origin
    d /= np.sqrt((d * d).sum(axis=-1, keepdims=True))
    oc = origin - np.array(FALLBACK_CENTRE)
    b = (d * oc).sum(axis=-1)
    return b * b - ((oc * oc).sum() - (0.9 * FALLBACK_RADIUS) ** 2) > 0.0


@pytest.mark.parametrize("variant", list(FORMS))
@pytest.mark.parametrize("world", list(WORLDS))
def test_specular_skip(rtc, world, variant):
    hs, cam, want, counters = _scene(rtc, world, variant)
    assert cam.hsize <= 64 and cam.vsize <= 48
    assert counters["secondary"] > 0 and counters["shadow"] > 0, world
    nan = np.isnan(want)
    assert nan.any() == (world == "fallback")
    for options, kernel in FORMS[variant]:
        for name, value in options.items():
            rtc.set_option(name, value)
        try:
            gpu = rtc.GpuScene(hs.desc)
            got = gpu.render(cam, DEPTH)
            st = gpu.stats()
            ran = gpu.last_kernel_name()
            gpu.close()
        finally:
            for name in OPTIONS:
                rtc.set_option(name, -1)
        assert ran == kernel, (world, variant, ran)
        assert (np.isnan(got) == nan).all(), (world, kernel, int(np.isnan(got).sum()), int(nan.sum()))
        delta = np.abs(got - want)[~nan]
        print(f"{world} {kernel}: max |delta| {delta.max():.3e}, NaN pixels {int(nan.any(axis=-1).sum())}")
        assert np.isfinite(got[~nan]).all() and delta.max() < TOL, (world, kernel, float(delta.max()))
        assert [st["overflow"], st["primary"], st["secondary"], st["shadow_calls"]] == \
            [0, counters["primary"], counters["secondary"], counters["shadow"]], (world, kernel)


def test_the_highlight_is_in_view(rtc):
    """`mixed` tests a lane that needs the power only if the glass sphere's highlight is on the image: without the sphere's
    specular term the oracle's image loses more than 0.5 somewhere, and only on a few pixels (the rest of the image is lanes that
    do not need it)."""
    _, _, want, _ = _scene(rtc, "mixed")
    camera, lights, objs = _mixed(sphere_specular=0)
    hs = rtc.HostScene(json.dumps({"camera": camera, "lights": lights, "objects": objs}))
    dull, _ = ob.OracleScene(hs.desc).render(hs.camera(), DEPTH)
    lost = (want - dull).max(axis=-1)
    print(f"highlight: up to {lost.max():.3f} on {int((lost > 1e-3).sum())} pixels of {lost.size}")
    assert lost.max() > 0.5 and 0 < (lost > 1e-3).sum() < lost.size // 8


def test_the_fallback_sphere_is_half_nan(rtc):
    """The oracle's image of `fallback` holds NaN and finite pixels on the shininess -2000 sphere."""
    _, cam, want, _ = _scene(rtc, "fallback")
    on = _on_fallback_sphere(cam)
    nan = np.isnan(want).any(axis=-1)
    print(f"fallback sphere: {int(on.sum())} pixels, {int((on & nan).sum())} NaN, {int((on & ~nan).sum())} finite; NaN elsewhere {int((~on & nan).sum())}")
    assert on.sum() >= 50 and (on & nan).sum() >= 10 and (on & ~nan).sum() >= 10
