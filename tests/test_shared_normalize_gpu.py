"""Three of the simple kernels normalise a vector with ONE refined reciprocal (csrc/rtc_kernels.hip: shared_normalize_ok /
shared_normalize; render_body, kSharedNormalize): the world normal, the point-light vector and the camera ray.

`test_shared_quotients_are_exact` runs the arithmetic beside the plain divisions on 2^28 vectors
(tests/hip/shared_normalize_check.hip, which carries a copy of the two functions: a change to one is a change to both).
The render tests put worlds whose normals and light vectors sit on the helper's edges - a -0 component, a component of
6e-17, a zero vector, two zero components, operands outside the guard's range in some lanes or in all - through every
kernel that has the shared form, each forced by option, against the oracle's image and ray counters."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from test_parity_gpu import TOL

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = 5
SIZE = (64, 48)
# (box_cull, simple3_min_chunks) -> the kernel that must run: the three kernels that have the shared form
FORMS = {(0, 1e9): "rtc_render_kernel_simple", (1, 1e9): "rtc_render_kernel_simple_b", (1, 0): "rtc_render_kernel_simple3_b"}


# ---------------------------------------------------------------- the arithmetic
def test_shared_quotients_are_exact(tmp_path):
    """Guard accepts: the shared quotients are x / m bit for bit, the sign of a zero included.  The shared form also runs
    unguarded on every vector: each mismatch it has lies outside the guard (none inside is the same statement).  The
    check has teeth: unguarded, the extreme class (exponents -1070 .. +500) does mismatch, and so does the form without
    the sign copy inside the guard.  And the guard does not hide behind rejection: it accepts every vector of the
    ordinary class (components zero or of an exponent within +-100)."""
    exe = str(tmp_path / "shared_normalize_check")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-o", exe,
                    os.path.join(REPO, "tests", "hip", "shared_normalize_check.hip")], check=True, capture_output=True, timeout=600)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    total = int(re.search(r"shared_normalize_check: (\d+) vectors", run.stdout).group(1))
    assert total >= 2 ** 27
    rows = {m.group(1): {k: int(v) for k, v in re.findall(r"(\w+) (\d+)", m.group(2))}
            for m in re.finditer(r"^class (\w+): (.*)$", run.stdout, re.M)}
    assert set(rows) == {"ordinary", "extreme", "near_magnitude", "band_edges"}, run.stdout
    for name, row in rows.items():
        assert row["bad_guarded"] == 0, (name, run.stdout)
        assert 0 < row["accepted"] <= row["divided"] <= row["vectors"], (name, run.stdout)
    assert rows["ordinary"]["accepted"] == rows["ordinary"]["divided"] > 0.99 * rows["ordinary"]["vectors"], run.stdout
    assert rows["near_magnitude"]["accepted"] == rows["near_magnitude"]["divided"], run.stdout
    assert 0 < rows["band_edges"]["accepted"] < rows["band_edges"]["divided"], run.stdout   # both sides of the edges
    assert rows["extreme"]["bad_unguarded"] >= 1, run.stdout
    assert sum(row["bad_unsigned_guarded"] for row in rows.values()) >= 1, run.stdout


# ---------------------------------------------------------------- the worlds
def _shape(kind, transform, color=(1, 1, 1), **material):
    return {"type": {kind: {}}, "transform": transform,
            "material": dict({"pattern": {"type": {"solid": list(color)}}, "diffuse": 0.7, "specular": 0.3, "shininess": 50,
                              "reflective": 0.1}, **material)}


def _scene(objects, lights, frm=(0, 1.5, -5), to=(0, 1, 0)):
    return json.dumps({"camera": {"width": SIZE[0], "height": SIZE[1], "field-of-view": 1.0, "from": list(frm), "to": list(to), "up": [0, 1, 0]},
                       "lights": [{"point-light": {"position": list(p), "intensity": list(i)}} for p, i in lights], "objects": objects})


TWO_LIGHTS = [((-5, 8, -6), (0.7, 0.7, 0.7)), ((4, 3, -7), (0.3, 0.3, 0.4))]
FLOOR = _shape("plane", [], color=[0.8, 0.8, 0.7], specular=0.0)


def _mirrored_cubes():
    """Axis-aligned cubes with negative scales: a face normal's zero components times negative entries of the inverse
    transform are -0 in the world normal, and -0 / mag is -0."""
    objs = [FLOOR,
            _shape("cube", [{"scale": [-1, 1, 1]}, {"translate": [-2.2, 1, 0]}], color=[0.9, 0.3, 0.2]),
            _shape("cube", [{"scale": [0.8, -0.8, -0.8]}, {"translate": [0, 0.8, 1]}], color=[0.2, 0.8, 0.3], reflective=0.4),
            _shape("cube", [{"scale": [-0.6, -1.2, -0.6]}, {"translate": [2.1, 1.2, -0.5]}], color=[0.3, 0.3, 0.9],
                   transparency=0.6, **{"refractive-index": 1.3}),
            _shape("sphere", [{"scale": [-0.5, 0.5, -0.5]}, {"translate": [0.6, 0.5, -2]}], color=[0.8, 0.8, 0.2])]
    return _scene(objs, TWO_LIGHTS)


def _quarter_turn_plane():
    """A wall that is a plane rotated by pi/2: cos(pi/2) = 6.1e-17 is its world normal's y component."""
    objs = [FLOOR,
            _shape("plane", [{"rotate-x": math.pi / 2}, {"translate": [0, 0, 4]}], color=[0.4, 0.5, 0.9], reflective=0.3),
            _shape("plane", [{"rotate-z": math.pi / 2}, {"translate": [-4, 0, 0]}], color=[0.9, 0.5, 0.4]),
            _shape("sphere", [{"translate": [0.5, 1, 0]}], color=[0.9, 0.9, 0.9], reflective=0.5),
            _shape("cube", [{"scale": [0.5, 0.5, 0.5]}, {"rotate-y": math.pi / 2}, {"translate": [-1.5, 0.5, -1]}], color=[0.2, 0.7, 0.6])]
    return _scene(objs, TWO_LIGHTS)


def _floor_over_point(rtc, px, py):
    """over_point of pixel (px, py)'s hit on the floor plane y = 0 under the camera of _scene(), in the kernels' own
    arithmetic (Camera.rayForPixel, Plane.localIntersect, position, normalToWorld of an untransformed plane: (0, 1, 0))."""
    hs = rtc.HostScene(_scene([FLOOR], TWO_LIGHTS))
    cam = hs.camera()
    inv = list(cam.inv_view)
    row = lambda r, x, y, z: ((inv[4 * r] * x + inv[4 * r + 1] * y) + inv[4 * r + 2] * z) + inv[4 * r + 3]
    wx = cam.half_width - (px + 0.5) * cam.pixel_size
    wy = cam.half_height - (py + 0.5) * cam.pixel_size
    pix = [row(r, wx, wy, -1.0) for r in range(3)]
    org = [row(r, 0.0, 0.0, 0.0) for r in range(3)]
    d = [p - o for p, o in zip(pix, org)]
    mag = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    d = [c / mag for c in d]
    t = -org[1] / d[1]
    assert t > 0
    pt = [o + c * t for o, c in zip(org, d)]
    return [pt[0] + 0.0 * 1e-5, pt[1] + 1.0 * 1e-5, pt[2] + 0.0 * 1e-5]


def _assert_is_over_point(rtc, point, px, py):
    """Host-side proof that `point` IS pixel (px, py)'s over_point on the floor, to the bit, by the oracle: above a floor of
    ambient 0, diffuse 1, specular 1, shininess 1 a single light AT the over_point gives that pixel the colour 0 exactly -
    the light vector stays (0, 0, 0): no diffuse and no specular term -, while a light one ulp from it along an axis has a
    unit light vector along that axis: bright on one side (light_dot_normal = 1 above; along x and z the mirrored vector
    against the eye is positive on one side) and dark on the other.  A `point` that is off by any number of ulps along an
    axis fails one of the three statements for that axis."""
    probe = _shape("plane", [], ambient=0.0, diffuse=1.0, specular=1.0, shininess=1.0, reflective=0.0)

    def colour(light):
        hs = rtc.HostScene(_scene([probe], [(light, (1, 1, 1))]))
        image, _ = ob.OracleScene(hs.desc).render(hs.camera(), 1)
        return float(np.abs(image[py, px]).max())

    assert colour(point) == 0.0, (point, colour(point))
    for axis in range(3):
        sides = []
        for towards in (math.inf, -math.inf):
            moved = list(point)
            moved[axis] = math.nextafter(point[axis], towards)
            sides.append(colour(moved))
        assert min(sides) == 0.0 and max(sides) > 1e-3, (axis, sides)


def _lights_on_the_hit(rtc):
    """A light exactly at a floor hit's over_point - distance == 0: the vector stays (0, 0, 0), nothing is divided - and a
    light straight above another hit's over_point: its vector has two zero components.  Both over_points are proved by the
    oracle before they are used (_assert_is_over_point): the cases cannot drift off their edge unnoticed."""
    at = _floor_over_point(rtc, 20, 40)
    above = _floor_over_point(rtc, 45, 36)
    _assert_is_over_point(rtc, at, 20, 40)
    _assert_is_over_point(rtc, above, 45, 36)
    lights = [(at, (0.5, 0.5, 0.5)), ((above[0], 4.0, above[2]), (0.6, 0.6, 0.6)), ((-5, 8, -6), (0.3, 0.3, 0.3))]
    objs = [FLOOR, _shape("sphere", [{"translate": [-1.5, 1, 1]}], color=[0.9, 0.2, 0.2]),
            _shape("cube", [{"scale": [0.5, 0.5, 0.5]}, {"translate": [1.8, 0.5, 1.5]}], color=[0.2, 0.3, 0.9])]
    return _scene(objs, lights)


# (the loader refuses a transform whose determinant is below 1e-5 or no double - NotInvertible, as the reference does: the
# factors of 1e-150 and 1e+120 are along one axis, the other axes making up for them)
HUGE = [1e120, 1e90, 1e80]
THIN_X = [1e-150, 1e80, 1e80]
THIN_Y = [1e80, 1e-150, 1e80]


def _beyond_the_guard():
    """Shapes whose world normals lie beyond the guard's range beside ordinary ones: two spheres scaled by 1e-150 along
    one axis - sheets, one of glass; their normals have a magnitude of 1e150 - and, around everything, a sphere scaled by 1e+120 (normals of
    1e-80 and less, light vectors of 1e80 and more from its hits): waves that hold such a hit take the plain divisions."""
    objs = [FLOOR,
            _shape("sphere", [{"scale": THIN_X}, {"rotate-y": 1.0}, {"translate": [2.5, 1, 1]}], color=[0.9, 0.9, 0.3],
                   transparency=0.5, **{"refractive-index": 1.2}),
            _shape("sphere", [{"scale": THIN_Y}, {"rotate-x": -0.4}, {"translate": [0, 4, 3]}], color=[0.9, 0.4, 0.8]),
            _shape("sphere", [{"scale": HUGE}], color=[0.3, 0.5, 0.9], ambient=0.4, specular=0.0, reflective=0.0),
            _shape("sphere", [{"translate": [-0.2, 1, 1.5]}], color=[0.9, 0.3, 0.2], reflective=0.3),
            _shape("cube", [{"scale": [0.4, 0.4, 0.4]}, {"rotate-y": 0.5}, {"translate": [0.2, 0.4, -1.5]}], color=[0.3, 0.8, 0.3])]
    return _scene(objs, TWO_LIGHTS)


def _straddling_the_guard():
    """Ordinary shapes in front of walls whose transforms put their normals outside the guard's range - a plane scaled by
    1e-70 along its normal (normal 1e70) and one by 1e90 (normal 1e-90), the sphere scaled by 1e+120 around everything: the lanes of a wave that
    covers a silhouette lie on both sides of the guard, and the wave takes the plain divisions for all of them."""
    objs = [_shape("plane", [{"scale": [1e70, 1e-70, 1]}], color=[0.8, 0.8, 0.7], specular=0.0),
            _shape("plane", [{"scale": [1e-90, 1e90, 1]}, {"rotate-x": math.pi / 2}, {"translate": [0, 0, 6]}], color=[0.5, 0.5, 0.8]),
            _shape("sphere", [{"scale": HUGE}], color=[0.3, 0.5, 0.9], ambient=0.4, specular=0.0, reflective=0.0),
            _shape("sphere", [{"translate": [-1.2, 1, 0]}], color=[0.9, 0.3, 0.2], reflective=0.3),
            _shape("sphere", [{"scale": [0.5, 0.5, 0.5]}, {"translate": [0.3, 0.5, -1.5]}], color=[0.9, 0.9, 0.3],
                   transparency=0.7, **{"refractive-index": 1.5}),
            _shape("cube", [{"scale": [0.6, 0.6, 0.6]}, {"rotate-y": 0.5}, {"translate": [1.5, 0.6, 0.5]}], color=[0.3, 0.8, 0.3])]
    return _scene(objs, TWO_LIGHTS)


WORLDS = {"mirrored_cubes": lambda rtc: _mirrored_cubes(), "quarter_turn_plane": lambda rtc: _quarter_turn_plane(),
          "lights_on_the_hit": _lights_on_the_hit, "beyond_the_guard": lambda rtc: _beyond_the_guard(),
          "straddling_the_guard": lambda rtc: _straddling_the_guard()}


@pytest.fixture(scope="module")
def references(rtc):
    """world -> (HostScene, camera, the oracle's image, the oracle's counters): rendered once, read by every form."""
    cache = {}

    def get(name):
        if name not in cache:
            hs = rtc.HostScene(WORLDS[name](rtc))
            cam = hs.camera()
            want, counters = ob.OracleScene(hs.desc).render(cam, DEPTH)
            want.setflags(write=False)
            cache[name] = (hs, cam, want, counters)
        return cache[name]
    return get


@pytest.mark.parametrize("form", sorted(FORMS), ids=[FORMS[f].replace("rtc_render_kernel_", "") for f in sorted(FORMS)])
@pytest.mark.parametrize("world", sorted(WORLDS))
def test_worlds_on_the_helper_s_edges(rtc, references, world, form):
    hs, cam, want, counters = references(world)
    rtc.set_option("box_cull", form[0])
    rtc.set_option("simple3_min_chunks", form[1])
    try:
        gpu = rtc.GpuScene(hs.desc)
        got = gpu.render(cam, DEPTH)
        st = gpu.stats()
        name = gpu.last_kernel_name()
    finally:
        rtc.set_option("box_cull", -1)
        rtc.set_option("simple3_min_chunks", -1)
    assert name == FORMS[form], name
    assert got.shape == want.shape and np.isfinite(got).all()
    delta = np.abs(got - want)
    assert delta.max() < TOL, (world, name, delta.max(), np.unravel_index(np.argmax(delta), delta.shape))
    assert [st["overflow"], st["primary"], st["secondary"], st["shadow_calls"]] == \
        [0, counters["primary"], counters["secondary"], counters["shadow"]], (world, name)
