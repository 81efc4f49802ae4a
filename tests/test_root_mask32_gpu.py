"""A three-wave simple kernel's world has at most 32 roots, and rtc_render_kernel_simple3_b runs the root loop of its closest-hit
and shadow traces in the 32-root form (csrc/rtc_kernels.hip: MAX_ROOTS, RTC_ROOTS32): one block, a 32-bit survivor mask, the
box table walked from its top record down with every root's bit shifted into the mask as it is formed.  Here the worlds in
which that can go wrong, small images against the oracle's - image and ray counters - through rtc_render_kernel_simple3_b (a
world of cubes) and, the same shapes, through rtc_render_kernel_simple3 (a world of spheres; it keeps the 64-root form, where
the 32-bit mask lost, and is held to the same worlds so that it can be tried again):

  * 1, 2, 3, 4, 5, 7, 8, 9, 18, 30, 31 and 32 bounded roots: every remainder of the step of four roots and of the half step,
    and bit 31 set;
  * each with no plane, one plane and three planes behind the bounded roots while the world stays within 32 roots (30 bounded
    roots take two planes, 31 one: exactly 32), so that the planes' bits [nc, n) end at bit 31 as well;
  * one world of 33 roots, which a three-wave kernel must not be given.

Every world has a glass solid (the rays refracted into it start inside it: the containers pass meets an open root), two point
lights, one of them among the objects (the roots beyond it are clipped by t_hi), and - from three bounded roots on - the FIRST
and the LAST bounded root of the table (sorted spheres, cubes, planes) in a colour of their own that only ambient light
carries, each alone in some pixels: a survivor bit at the wrong index is a pixel of the wrong colour.
"""
import json

import numpy as np
import pytest

import oracle_binding as ob
from test_parity_gpu import TOL, _check_launch

pytestmark = pytest.mark.gpu

DEPTH = 5
OPTIONS = ("box_cull", "simple3_min_chunks")
# form -> (options, the three-wave kernel, the two-wave kernel a world of more than 32 roots runs)
FORMS = {
    "boxes": ({"box_cull": 1, "simple3_min_chunks": 0}, "rtc_render_kernel_simple3_b", "rtc_render_kernel_simple_b"),
    "spheres": ({"box_cull": 0, "simple3_min_chunks": 0}, "rtc_render_kernel_simple3", "rtc_render_kernel_simple"),
}
BOUNDED = (1, 2, 3, 4, 5, 7, 8, 9, 18, 30, 31, 32)
CASES = [(b, p) for b in BOUNDED for p in sorted({0, min(1, 32 - b), min(3, 32 - b)})]
FIRST, LAST = [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]


def _marker(colour):
    return {"ambient": 1.0, "diffuse": 0.0, "specular": 0.0, "pattern": {"type": {"solid": colour}}}


def _scene(form, bounded, planes):
    """`bounded` solids on a grid of eight columns, in table order: [first marker][the glass solid][...][last marker]."""
    mostly, other = ("cube", "sphere") if form == "boxes" else ("sphere", "cube")
    objs = []
    for i in range(bounded):
        x, z = (i % 8 - 3.5) * 1.1, (i // 8) * 1.1
        s = 0.3 + 0.02 * (i % 4)
        transform = [{"scale": [s, s, s]}, {"rotate-y": 0.2 * i}, {"translate": [x, s + 0.15, z]}]
        kind = mostly
        if bounded >= 3 and i == 0:
            material = _marker(FIRST)
        elif bounded >= 3 and i == bounded - 1:
            material = _marker(LAST)
        elif i == min(1, bounded - 1):
            material = {"transparency": 0.8, "refractive-index": 1.5, "reflective": 0.2, "diffuse": 0.2, "ambient": 0.1}
        else:   # (four materials among all the others: a three-wave kernel's tables hold 16)
            v = i % 4
            material = {"diffuse": round(0.5 + 0.1 * v, 3), "reflective": 0.3 if v == 2 else 0.0,
                        "pattern": {"type": {"solid": [0.9, round(0.3 + 0.15 * v, 3), 0.3]}}}
        objs.append({"type": {kind: {}}, "transform": transform, "material": material})
    # the table is sorted spheres, cubes, planes: a world of cubes begins with its one sphere, a world of spheres ends with its one cube
    if bounded >= 3:
        objs[0 if form == "boxes" else -1]["type"] = {other: {}}
    walls = [
        {"type": {"plane": {}}, "transform": [], "material": {"diffuse": 0.8, "specular": 0.1, "reflective": 0.2}},
        {"type": {"plane": {}}, "transform": [{"rotate-x": 1.5707963267948966}, {"translate": [0, 0, 6]}], "material": {"diffuse": 0.7}},
        {"type": {"plane": {}}, "transform": [{"rotate-z": 1.5707963267948966}, {"translate": [-7, 0, 0]}], "material": {"diffuse": 0.6}},
    ]
    lights = [{"point-light": {"position": [-6, 8, -6], "intensity": [0.6, 0.6, 0.6]}},
              {"point-light": {"position": [-0.55, 0.45, 0.55], "intensity": [0.4, 0.4, 0.4]}}]   # between the solids of the first two rows
    camera = {"width": 64, "height": 48, "field-of-view": 1.1, "from": [0, 7, -6], "to": [0, 0, 1.6], "up": [0, 1, 0]}
    return json.dumps({"camera": camera, "lights": lights, "objects": objs + walls[:planes]})


def _render(rtc, form, bounded, planes, kernel):
    hs = rtc.HostScene(_scene(form, bounded, planes))
    cam = hs.camera()
    assert cam.hsize <= 64 and cam.vsize <= 48
    assert hs.desc.n_roots == bounded + planes
    want, counters = ob.OracleScene(hs.desc).render(cam, DEPTH)
    assert counters["shadow"] > 0 and (bounded + planes < 2 or counters["secondary"] > 0)
    if bounded >= 3:    # each marker alone in some pixel: its colour times the two lights' intensities, nothing else
        rgb = want.reshape(-1, 3)
        for colour in (FIRST, LAST):
            assert (np.abs(rgb - np.array(colour)).max(axis=1) < 1e-12).any(), (form, bounded, planes, colour)
    for name, value in FORMS[form][0].items():
        rtc.set_option(name, value)
    try:
        gpu = rtc.GpuScene(hs.desc)
        what = (form, bounded, planes, kernel)
        _check_launch(gpu, cam, DEPTH, want, counters, what)
        ran = gpu.last_kernel_name()
        gpu.close()
    finally:
        for name in OPTIONS:
            rtc.set_option(name, -1)
    assert ran == kernel, (what, ran)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("bounded,planes", CASES)
def test_up_to_32_roots(rtc, form, bounded, planes):
    assert bounded + planes <= 32
    _render(rtc, form, bounded, planes, FORMS[form][1])


def test_cases_reach_bit_31():
    assert (32, 0) in CASES and (31, 1) in CASES and (30, 2) in CASES and (18, 3) in CASES and (1, 0) in CASES


@pytest.mark.parametrize("form", list(FORMS))
def test_33_roots_run_a_two_wave_kernel(rtc, form):
    _render(rtc, form, 32, 1, FORMS[form][2])
