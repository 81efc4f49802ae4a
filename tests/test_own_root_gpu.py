"""A wave of a simple kernel whose transparent hits all lie on roots that are ALONE takes n1 / n2 from each hit root's own two
entries and makes no containers pass (csrc/rtc_kernels.hip: render_body, kOwnRoot; which roots are alone and why that is
enough: tests/test_own_root_cpu.py).  Here small images - rendered with cooperative iterations on the
two-wave kernels, where the lanes of a group hold one ray and must leave without merging - against the oracle's, image and
ray counters, through the four simple kernels, each with option containers_own_root 1 (the flags as built) and 0 (no root
marked: every hit makes the pass as before).

  alone    a glass sphere (ior 1.5) among opaque cubes of the default ior on a floor, a mirror cube next to it (rays that
           start on a neighbour's surface).  The sphere is alone: every pass of the frame is the short one.
  inside   a rotated glass cube with the camera inside it: the hit root is open from the first hit on.
  mixed    the alone sphere, and two overlapping transparent spheres of ior exactly 1.0: neither of the pair is alone, waves
           hold lanes of both kinds and make the pass for all of them.
  off      the glass sphere with a cube whose box touches its box: no root is alone, the frame is what it was.
"""
import json

import numpy as np
import pytest

import oracle_binding as ob

pytestmark = pytest.mark.gpu

# (tests/test_containers_gpu.py: the same arithmetic in the same order but for pixels whose ray tree is shared between lanes - a
# few roundings of 2^-53 on colours of order one; a wrong n1 or n2 bends a refracted ray: at least 1e-3)
TOL = 1e-12
DEPTH = 5
ALONE = 0x800

CHECKERS = {"type": {"checkers": [{"type": {"solid": [0.9, 0.9, 0.9]}}, {"type": {"solid": [0.2, 0.2, 0.2]}}]}}


def _glass(ior, **more):
    return dict({"transparency": 0.8, "refractive-index": ior, "reflective": 0.2, "diffuse": 0.2, "ambient": 0.1}, **more)


def _obj(kind, transform, material, **more):
    return dict({"type": {kind: {}}, "transform": transform, "material": material}, **more)


def _floor(y, **material):
    return _obj("plane", [{"translate": [0, y, 0]}], dict({"diffuse": 0.8, "specular": 0.1}, **material))


def _solid(r, g, b, **more):
    return dict({"diffuse": 0.7, "pattern": {"type": {"solid": [r, g, b]}}}, **more)


GLASS_SPHERE = _obj("sphere", [{"translate": [0, 1.05, 0]}], _glass(1.5))


def _alone():
    objs = [
        GLASS_SPHERE,
        _obj("cube", [{"scale": [0.5, 0.5, 0.5]}, {"translate": [1.6, 0.5, 0.2]}], _solid(0.8, 0.8, 0.9, reflective=0.9, diffuse=0.1)),   # a mirror, 0.1 from the sphere's box
        _obj("cube", [{"scale": [0.4, 0.7, 0.4]}, {"rotate-y": 0.5}, {"translate": [-2.2, 0.7, 1.0]}], _solid(0.9, 0.3, 0.2)),
        _obj("cube", [{"scale": [0.6, 0.3, 0.6]}, {"rotate-y": -0.3}, {"translate": [0.5, 0.3, 3.0]}], _solid(0.2, 0.7, 0.3)),
        _obj("cube", [{"scale": [0.3, 0.3, 0.3]}, {"translate": [-0.8, 0.3, -2.0]}], _solid(0.2, 0.3, 0.9)),
    ]
    lights = [{"point-light": {"position": [-4, 6, -5], "intensity": [0.9, 0.9, 0.9]}}]
    camera = {"width": 64, "height": 48, "field-of-view": 1.0, "from": [0.5, 2.0, -5.5], "to": [0, 0.9, 0], "up": [0, 1, 0]}
    return camera, lights, objs + [_floor(0.0, pattern=CHECKERS)], {0}


def _inside():
    objs = [
        _obj("cube", [{"scale": [3, 2, 3]}, {"rotate-y": 0.4}, {"rotate-z": 0.1}], _glass(1.5)),          # the camera is inside
        _obj("sphere", [{"translate": [0.5, 0, 6]}], _solid(0.9, 0.3, 0.2)),
        _obj("cube", [{"scale": [0.7, 0.7, 0.7]}, {"rotate-y": 0.8}, {"translate": [-3, -0.5, 7]}], _solid(0.2, 0.4, 0.9, reflective=0.3)),
        _obj("sphere", [{"scale": [0.8, 0.8, 0.8]}, {"translate": [3.5, 1.0, 8]}], _solid(0.3, 0.8, 0.3)),
    ]
    lights = [{"point-light": {"position": [-6, 8, -8], "intensity": [0.9, 0.9, 0.9]}}]
    camera = {"width": 63, "height": 47, "field-of-view": 1.3, "from": [0.2, 0.3, -1.0], "to": [0, 0, 5], "up": [0, 1, 0]}
    return camera, lights, objs + [_floor(-4.0, pattern=CHECKERS)], {0}


def _mixed():
    clear = {"transparency": 0.7, "refractive-index": 1.0, "reflective": 0.1, "diffuse": 0.3, "ambient": 0.1}
    objs = [
        GLASS_SPHERE,
        _obj("sphere", [{"scale": [0.8, 0.8, 0.8]}, {"translate": [-2.4, 0.9, 0.5]}], dict(clear, pattern={"type": {"solid": [0.9, 0.6, 0.6]}})),   # the pair overlaps
        _obj("sphere", [{"scale": [0.8, 0.8, 0.8]}, {"translate": [-3.2, 1.1, 1.0]}], dict(clear, pattern={"type": {"solid": [0.6, 0.6, 0.9]}})),
        _obj("cube", [{"scale": [0.5, 0.5, 0.5]}, {"rotate-y": 0.4}, {"translate": [2.2, 0.5, 1.5]}], _solid(0.9, 0.8, 0.2)),
    ]
    lights = [{"point-light": {"position": [-4, 6, -5], "intensity": [0.9, 0.9, 0.9]}}]
    camera = {"width": 64, "height": 48, "field-of-view": 1.1, "from": [-1.2, 2.0, -5.5], "to": [-1.2, 0.9, 0], "up": [0, 1, 0]}
    return camera, lights, objs + [_floor(0.0, pattern=CHECKERS)], {0}


def _off():
    objs = [
        _obj("sphere", [], _glass(1.5)),
        _obj("cube", [{"scale": [0.5, 0.5, 0.5]}, {"translate": [1.5, 0, 0]}], _solid(0.9, 0.3, 0.2)),     # box against box, gap 0
    ]
    lights = [{"point-light": {"position": [-3, 6, -5], "intensity": [1, 1, 1]}}]
    camera = {"width": 64, "height": 48, "field-of-view": 0.9, "from": [0.5, 1.0, -5], "to": [0.4, 0, 0], "up": [0, 1, 0]}
    return camera, lights, objs + [_floor(-3.0, pattern=CHECKERS)], set()


WORLDS = {"alone": _alone, "inside": _inside, "mixed": _mixed, "off": _off}

OPTIONS = ("box_cull", "simple3_min_chunks")
FORMS = [({"box_cull": 1, "simple3_min_chunks": 1e9}, "rtc_render_kernel_simple_b"), ({"box_cull": 1, "simple3_min_chunks": 0}, "rtc_render_kernel_simple3_b"),
         ({"box_cull": 0, "simple3_min_chunks": 1e9}, "rtc_render_kernel_simple"), ({"box_cull": 0, "simple3_min_chunks": 0}, "rtc_render_kernel_simple3")]


def _scene(world, reflective=True):
    camera, lights, objs, _ = WORLDS[world]()
    objs = json.loads(json.dumps(objs))
    if not reflective:
        for o in objs:
            o["material"]["reflective"] = 0.0
    return json.dumps({"camera": camera, "lights": lights, "objects": objs})


_WANT = {}


def _oracle(rtc, world):
    """(host scene, camera, the oracle's image, its counters, its secondary rays without reflection) - rendered once per world"""
    if world not in _WANT:
        hs = rtc.HostScene(_scene(world))
        cam = hs.camera()
        want, counters = ob.OracleScene(hs.desc).render(cam, DEPTH)
        # the same world without a reflective material: every secondary ray it has left is a refracted one - a world that
        # never computes n1 and n2 cannot pass silently
        plain = rtc.HostScene(_scene(world, reflective=False))
        _, refracted = ob.OracleScene(plain.desc).render(plain.camera(), DEPTH)
        _WANT[world] = (hs, cam, want, counters, refracted["secondary"])
    return _WANT[world]


@pytest.mark.parametrize("world", list(WORLDS))
def test_own_root_against_the_oracle_and_against_the_pass(rtc, world):
    hs, cam, want, counters, refracted = _oracle(rtc, world)
    assert cam.hsize <= 64 and cam.vsize <= 48
    assert refracted > 100 and counters["secondary"] > 0, (world, refracted)
    # the roots the host marks are the ones the world was built to have
    flags = rtc.root_flags(hs.desc)
    _, order, _ = rtc.root_boxes(hs.desc)
    marked = {int(order[pos]) for pos in range(hs.desc.n_roots) if flags[pos] & ALONE}
    assert marked == WORLDS[world]()[3], (world, marked)
    for options, kernel in FORMS:
        images = {}
        for own_root in (1, 0):
            for name, value in options.items():
                rtc.set_option(name, value)
            rtc.set_option("containers_own_root", own_root)
            try:
                gpu = rtc.GpuScene(hs.desc)
                got = gpu.render(cam, DEPTH)
                st = gpu.stats()
                ran = gpu.last_kernel_name()
                gpu.close()
            finally:
                for name in OPTIONS:
                    rtc.set_option(name, -1)
                rtc.set_option("containers_own_root", 1)
            assert ran == kernel, (world, ran)
            delta = np.abs(got - want)
            print(f"{world} {kernel} containers_own_root={own_root}: max |delta| {delta.max():.3e}, {refracted} refracted rays without reflection")
            assert np.isfinite(got).all() and delta.max() < TOL, (world, kernel, own_root, float(delta.max()), np.unravel_index(np.argmax(delta), delta.shape))
            assert [st["overflow"], st["primary"], st["secondary"], st["shadow_calls"]] == \
                [0, counters["primary"], counters["secondary"], counters["shadow"]], (world, kernel, own_root)
            images[own_root] = got
        between = float(np.abs(images[1] - images[0]).max())
        print(f"{world} {kernel}: with the flags against without, max |delta| {between:.3e}")
        assert between < TOL, (world, kernel, between)
