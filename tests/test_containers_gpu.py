"""The containers pass of a world of planes, spheres and cubes (n1 / n2 of a refracted ray, PreComputations.new) uses a root only
if an odd number of its entries lies behind the origin.  In the simple kernels its phase 1 drops a sphere or cube whose bound
lies entirely behind the origin (an even count) and its plane test makes no division where the entry cannot be negative
(csrc/rtc_kernels.hip: trace(), RTC_CONTAINERS_SOLIDS; the arithmetic argument is held in tests/test_containers_cpu.py).  Here
the smallest worlds in which the ORDER of the containers can go wrong, small images against the oracle's - image and ray
counters - through the four simple kernels, and once each through the flat kernel (a cylinder added) and the kernels that walk
groups (a group added), whose pass is the one it always was.  (Images this small are rendered with cooperative iterations on
the two-wave kernels of worlds without groups.)

  nested   a glass sphere inside a glass cube inside a larger glass sphere, three refractive indices, the camera inside the
           outermost; a glass cube and a glass sphere that overlap without nesting (entered in either order, by the pixel); an
           opaque cube with refractive-index 2.0 overlapping a glass sphere (opaque containers count).
  planes   glass planes seen from above and - by way of a mirror floor - from below, two of them parallel; a glass sphere
           across them (a ray that starts inside it has a plane's entry behind it as well: the plane's quotient decides which
           is the later one); a plane squeezed by 1e-11 along its normal (|d.y| > 1e10 in its own space) and one by 1e-9; a
           plane stretched by 2e4 (|d.y| <= 1e-5 for the flatter rays: the reference's parallel rule ends those tests; the
           squeezed ones are as much wider as keeps their determinant above the loader's 1e-5); the camera exactly ON a plane
           (o.y = 0 in its space: the quotient is a zero).
  ties     two glass cubes sharing a face; two glass spheres with the same transform (equal t: the order is the leaves'); an odd
           image size whose centre ray, from (1, 0, -5) towards (1, 0, 0), is tangent to a glass unit sphere at the origin (two
           entries at t_hit).
  ties3    THREE glass spheres with one transform and three indices inside a larger glass sphere that comes after them in
           World.objects: the tie between open leaves is decided twice, and the second time in the flush BETWEEN two leaves
           (the third sphere's, when the larger sphere's entries arrive), not in the last one.
  blocks   72 bounded roots and a floor, glass solids in both blocks of 64 (the table is sorted spheres, cubes, planes: the
           second block holds the last cubes and the floor).  Two-wave kernels only (a three-wave kernel holds 32 roots).

The `ties` world found a fault older than this test: on a tie in t between two open leaves the simple kernels' LAST flush of
the containers visitor moved the later leaf but kept the earlier leaf's material (n1 of the wrong sphere; 108 pixels of
the two spheres off by up to 0.196 on all four simple kernels, the flat and general kernels exact).  The simple kernels
make that flush with selects on one condition (BehindVisitorT<SELECTS>, csrc/rtc_kernels.hip; the instructions that were wrong:
profiles/containers/flush_tie_isa.txt).
"""
import copy
import json

import numpy as np
import pytest

import oracle_binding as ob

pytestmark = pytest.mark.gpu

# (tests/test_cube_behind_gpu.py: the same arithmetic in the same order but for pixels whose ray tree is shared between lanes -
# a few roundings of 2^-53 on colours of order one; a wrong n1 or n2 bends a refracted ray: at least 1e-3)
TOL = 1e-12
DEPTH = 5


CHECKERS = {"type": {"checkers": [{"type": {"solid": [0.9, 0.9, 0.9]}}, {"type": {"solid": [0.2, 0.2, 0.2]}}]}}


def _glass(ior, **more):
    return dict({"transparency": 0.8, "refractive-index": ior, "reflective": 0.2, "diffuse": 0.2, "ambient": 0.1}, **more)


def _obj(kind, transform, material, **more):
    return dict({"type": {kind: {}}, "transform": transform, "material": material}, **more)


def _floor(y, **material):
    return _obj("plane", [{"translate": [0, y, 0]}], dict({"diffuse": 0.8, "specular": 0.1}, **material))


def _nested():
    objs = [
        _obj("sphere", [{"scale": [6, 6, 6]}], _glass(1.2), **{"casts-shadow": False}),                 # the camera is inside
        _obj("cube", [{"scale": [2, 2, 2]}, {"rotate-y": 0.5}], _glass(1.5)),
        _obj("sphere", [], _glass(1.33, reflective=0.0)),
        _obj("cube", [{"scale": [0.7, 0.7, 0.7]}, {"translate": [3.0, 0, 1]}], _glass(1.4)),            # overlap, neither inside the other
        _obj("sphere", [{"scale": [0.8, 0.8, 0.8]}, {"translate": [3.8, 0.2, 1]}], _glass(1.7)),
        _obj("cube", [{"scale": [0.6, 0.6, 0.6]}, {"translate": [-3.0, 0, 1]}], {"refractive-index": 2.0, "diffuse": 0.6}),   # opaque
        _obj("sphere", [{"scale": [0.8, 0.8, 0.8]}, {"translate": [-3.5, 0.3, 0.5]}], _glass(1.5)),
    ]
    lights = [{"point-light": {"position": [0, 4, -3], "intensity": [0.9, 0.9, 0.9]}}]
    camera = {"width": 64, "height": 47, "field-of-view": 1.4, "from": [0, 0.5, -4.5], "to": [0, 0, 0], "up": [0, 1, 0]}
    return camera, lights, objs, [_floor(-2.5, pattern=CHECKERS)]


def _planes():
    no_shadow = {"casts-shadow": False}
    objs = [
        _obj("sphere", [{"scale": [1.2, 1.2, 1.2]}, {"translate": [0, -0.5, 0]}], _glass(1.5)),         # across the planes y = 0 and y = -1
        _obj("sphere", [{"scale": [0.6, 0.6, 0.6]}, {"translate": [2, 0.8, 1]}], _glass(1.3)),
        _obj("cube", [{"scale": [0.5, 0.5, 0.5]}, {"rotate-y": 0.3}, {"translate": [-2, -1.6, 1.5]}], {"diffuse": 0.7, "pattern": {"type": {"solid": [0.9, 0.3, 0.2]}}}),
    ]
    planes = [
        _obj("plane", [{"translate": [0, 2, 0]}], _glass(1.0, reflective=0.0, transparency=0.9), **no_shadow),      # the camera is ON it
        _obj("plane", [], _glass(1.3), **no_shadow),
        _obj("plane", [{"translate": [0, -1, 0]}], _glass(1.6), **no_shadow),
        _obj("plane", [{"scale": [2e3, 1e-11, 2e3]}, {"translate": [0, -2, 0]}], _glass(1.2, reflective=0.0), **no_shadow),
        _obj("plane", [{"scale": [200, 1e-9, 200]}, {"translate": [0, -2.25, 0]}], _glass(1.25, reflective=0.0), **no_shadow),
        _obj("plane", [{"scale": [1, 2e4, 1]}, {"translate": [0, -2.5, 0]}], _glass(1.4, reflective=0.0), **no_shadow),
        _floor(-4, reflective=0.6, pattern=CHECKERS),             # the way back up
    ]
    lights = [{"point-light": {"position": [-3, 5, -4], "intensity": [0.9, 0.9, 0.9]}}]
    camera = {"width": 64, "height": 48, "field-of-view": 1.1, "from": [0, 2, -6], "to": [0, -1, 0], "up": [0, 1, 0]}
    return camera, lights, objs, planes


def _ties():
    objs = [
        _obj("sphere", [], _glass(1.5)),                                                               # tangent to the centre ray at (1, 0, 0)
        _obj("cube", [{"scale": [0.5, 0.5, 0.5]}, {"translate": [-2.75, 0, 0]}], _glass(1.3)),         # faces x = -2.25 of both
        _obj("cube", [{"scale": [0.5, 0.5, 0.5]}, {"translate": [-1.75, 0, 0]}], _glass(1.6)),
        _obj("sphere", [{"translate": [3.5, 0, 1]}], _glass(1.3)),                                     # the same transform twice
        _obj("sphere", [{"translate": [3.5, 0, 1]}], _glass(1.7)),
    ]
    lights = [{"point-light": {"position": [-2, 6, -6], "intensity": [0.9, 0.9, 0.9]}}]
    camera = {"width": 63, "height": 47, "field-of-view": 1.5, "from": [1, 0, -5], "to": [1, 0, 0], "up": [0, 1, 0]}
    return camera, lights, objs, [_floor(-1, pattern=CHECKERS)]


def _ties3():
    objs = [
        _obj("sphere", [{"translate": [0.5, 0, 1]}], _glass(1.3)),                                     # one transform three times
        _obj("sphere", [{"translate": [0.5, 0, 1]}], _glass(1.7)),
        _obj("sphere", [{"translate": [0.5, 0, 1]}], _glass(1.5, reflective=0.0)),
        _obj("sphere", [{"scale": [2.5, 2.5, 2.5]}, {"translate": [0.5, 0, 1]}], _glass(1.1), **{"casts-shadow": False}),   # around them, and after them
    ]
    lights = [{"point-light": {"position": [-2, 6, -6], "intensity": [0.9, 0.9, 0.9]}}]
    camera = {"width": 48, "height": 36, "field-of-view": 1.2, "from": [1, 0.5, -5], "to": [0.5, 0, 1], "up": [0, 1, 0]}
    return camera, lights, objs, [_floor(-3, pattern=CHECKERS)]


def _blocks():
    objs = []
    for i in range(72):   # 8 spheres (table positions 0..7) and 64 cubes (8..71): glass among the first and among the last of them
        x, z = (i % 9 - 4.0) * 1.2, (i // 9) * 1.2 - 2.0
        glass = i % 9 in (1, 5)
        if i % 9 == 3:
            objs.append(_obj("sphere", [{"scale": [0.5, 0.5, 0.5]}, {"translate": [x, 0.5, z]}], _glass(1.5) if i < 36 else {"reflective": 0.3}))
        else:
            h = 0.3 + 0.05 * (i % 5)
            objs.append(_obj("cube", [{"scale": [0.45, h, 0.45]}, {"rotate-y": 0.21 * i}, {"translate": [x, h, z]}],
                             _glass(1.3 + 0.2 * (i % 2)) if glass else {"diffuse": round(0.4 + 0.1 * (i % 4), 3)}))
    # a glass sphere over several of the far cubes, and a glass cube around two near ones: containers in both blocks at once
    objs[3] = _obj("sphere", [{"scale": [1.6, 1.6, 1.6]}, {"translate": [0.6, 0.9, 6.2]}], _glass(1.5))
    objs.append(_obj("cube", [{"scale": [1.3, 0.9, 0.7]}, {"translate": [-0.6, 0.9, -2.0]}], _glass(1.2)))
    lights = [{"point-light": {"position": [-8, 9, -7], "intensity": [0.6, 0.6, 0.6]}},
              {"point-light": {"position": [7, 5, -4], "intensity": [0.4, 0.4, 0.4]}}]
    camera = {"width": 64, "height": 48, "field-of-view": 1.1, "from": [0.4, 6, -11], "to": [0, 0.3, 2], "up": [0, 1, 0]}
    return camera, lights, objs, [_floor(0.0, reflective=0.2)]


WORLDS = {"nested": _nested, "planes": _planes, "ties": _ties, "ties3": _ties3, "blocks": _blocks}

# variant -> [(options, kernel)]; an option not named is the library's own choice (-1)
OPTIONS = ("box_cull", "simple3_min_chunks", "waves3")
FORMS = {
    "simple": [({"box_cull": 1, "simple3_min_chunks": 1e9}, "rtc_render_kernel_simple_b"), ({"box_cull": 1, "simple3_min_chunks": 0}, "rtc_render_kernel_simple3_b"),
               ({"box_cull": 0, "simple3_min_chunks": 1e9}, "rtc_render_kernel_simple"), ({"box_cull": 0, "simple3_min_chunks": 0}, "rtc_render_kernel_simple3")],
    "flat": [({}, "rtc_render_kernel_flat")],
    "group": [({"waves3": 0}, "rtc_render_kernel"), ({"waves3": 1}, "rtc_render_kernel3")],
}


def _scene(world, variant, reflective=True):
    camera, lights, objs, planes = WORLDS[world]()
    if variant == "flat":     # a leaf kind the simple kernels do not carry
        objs = objs + [{"type": {"cylinder": {"min": -1, "max": 1, "closed": True}}, "transform": [{"scale": [0.3, 0.5, 0.3]}, {"translate": [-5.5, 0.5, 9]}]}]
    elif variant == "group":  # a group at top level: the general root loop, everything else stays a top-level object
        objs = objs + [{"type": {"group": [{"type": {"sphere": {}}, "transform": [{"scale": [0.3, 0.3, 0.3]}, {"translate": [-5.5, 0.3, 9]}]},
                                           {"type": {"cube": {}}, "transform": [{"scale": [0.3, 0.3, 0.3]}, {"translate": [-5.5, 0.9, 9]}]}]}}]
    everything = copy.deepcopy(objs + planes)
    if not reflective:
        for o in everything:
            if "material" in o:
                o["material"]["reflective"] = 0.0
    return json.dumps({"camera": camera, "lights": lights, "objects": everything})


_WANT = {}


def _oracle(rtc, world, variant):
    """(host scene, camera, the oracle's image, its counters) - rendered once per world and variant"""
    if (world, variant) not in _WANT:
        hs = rtc.HostScene(_scene(world, variant))
        cam = hs.camera()
        want, counters = ob.OracleScene(hs.desc).render(cam, DEPTH)
        # the same world without a reflective material: every secondary ray it has left is a refracted one, spawned at the same
        # first hits - a world that never runs the containers pass cannot pass silently
        plain = rtc.HostScene(_scene(world, variant, reflective=False))
        _, refracted = ob.OracleScene(plain.desc).render(plain.camera(), DEPTH)
        _WANT[(world, variant)] = (hs, cam, want, counters, refracted["secondary"])
    return _WANT[(world, variant)]


@pytest.mark.parametrize("variant", list(FORMS))
@pytest.mark.parametrize("world", list(WORLDS))
def test_containers_in_order(rtc, world, variant):
    hs, cam, want, counters, refracted = _oracle(rtc, world, variant)
    assert cam.hsize <= 64 and cam.vsize <= 48
    if world == "blocks":
        assert hs.desc.n_roots >= 65
    assert refracted > 100 and counters["secondary"] > 0, (world, variant, refracted)
    forms = FORMS[variant]
    if world == "blocks":   # (a three-wave kernel holds 32 roots: a second block exists on the two-wave kernels only)
        forms = [f for f in forms if "3" not in f[1]]
    assert forms
    for options, kernel in forms:
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
        delta = np.abs(got - want)
        print(f"{world} {variant} {kernel}: max |delta| {delta.max():.3e}, {refracted} refracted rays without reflection")
        assert np.isfinite(got).all() and delta.max() < TOL, (world, variant, kernel, float(delta.max()), np.unravel_index(np.argmax(delta), delta.shape))
        assert [st["overflow"], st["primary"], st["secondary"], st["shadow_calls"]] == \
            [0, counters["primary"], counters["secondary"], counters["shadow"]], (world, variant, kernel)


def test_the_centre_ray_of_ties_is_tangent(rtc):
    """The `ties` world has two entries at t_hit only if the centre pixel's ray is the line x = 1, y = 0: recomputed as
    camera.zig builds it."""
    hs = rtc.HostScene(_scene("ties", "simple"))
    cam = hs.camera()
    assert cam.hsize % 2 == 1 and cam.vsize % 2 == 1
    inv = np.array(list(cam.inv_view)).reshape(4, 4)
    px, py = cam.hsize // 2, cam.vsize // 2
    wx = cam.half_width - (px + 0.5) * cam.pixel_size
    wy = cam.half_height - (py + 0.5) * cam.pixel_size
    pixel = inv @ np.array([wx, wy, -1.0, 1.0])
    origin = inv @ np.array([0.0, 0.0, 0.0, 1.0])
    d = pixel[:3] - origin[:3]
    d /= np.sqrt((d * d).sum())
    print("centre ray", origin[:3], d)
    assert origin[:3].tolist() == [1.0, 0.0, -5.0] and abs(d[0]) < 1e-15 and abs(d[1]) < 1e-15 and d[2] > 0
