"""A closest-hit or shadow trace skips the exact test of a cube that lies behind the ray's origin on one of the cube's own
axes (`cube_entirely_behind`, csrc/rtc_kernels.hip; the arithmetic argument is held in tests/test_cube_behind_cpu.py).
Here the worlds in which that decision is closest to wrong, small images against the oracle's - image and ray counters -
through every form of kernel that carries the path: the simple kernels on boxes and on spheres at two and three waves,
the flat kernel, the kernels that walk groups at two and three waves.  (Images this small are rendered with cooperative
iterations on the two-wave kernels of worlds without groups: tests/test_parity_gpu.py,
test_three_lights_same_bits_whatever_the_kernel_and_the_schedule.)

  faces    a cube on a floor, a cube stacked on it and one beside it with coplanar, touching faces (a ray that leaves one
           stands exactly on the neighbour's face: o = 1 + 1e-5 on one, o = 1 on the other); two lights 1e-13 either side
           of the plane in which the over_points of the third cube's top face lie, y = 2 + 1e-5 (shading starts from
           over_point, so that is where light_dot_normal changes sign: about +-2e-14 on that face, a shadow ray for the
           light above whose direction component along the cube's axis is 2e-14 - the predicate's `d >= 0` / parallel
           clause on the cube the ray stands on; test_the_lights_graze_the_top_face recomputes it), a rotated and sheared cube, a
           non-uniformly scaled one, a glass cube (refracted rays start inside it; the containers pass wants the entries
           behind the origin), a glass cube with a light inside; odd image size, the centre pixel's ray through a corner of
           the first cube and the centre column along its edge.
  room     the camera and both lights inside one large cube (rtc_scene_create marks it as a room), cubes inside it.
  blocks   64 bounded roots and a floor: the root loop's second block of 64 exists (on the two-wave kernels: a three-wave
           kernel holds 32 roots).
"""
import json

import numpy as np
import pytest

import oracle_binding as ob

pytestmark = pytest.mark.gpu

# A render against the oracle: the same arithmetic in the same order but for pixels whose ray tree is shared between lanes
# (glass: the shares are summed in completion order) - a few roundings of 2^-53 on colours of order one.  A cube test
# wrongly skipped or wrongly kept changes a pixel by a shadow, a reflection or a hit: at least 1e-3.
TOL = 1e-12
DEPTH = 5


# where the over_points of a top face y = 2 lie: the hit point moved by 1e-5 along the normal (shape.zig, EPSILON)
GRAZE_Y = 2.0 + 1e-5


def _cube(transform, **material):
    return {"type": {"cube": {}}, "transform": transform, "material": dict({"diffuse": 0.7, "specular": 0.3, "reflective": 0.1}, **material)}


def _floor(y=0.0):
    return {"type": {"plane": {}}, "transform": [{"translate": [0, y, 0]}], "material": {"diffuse": 0.8, "specular": 0.1, "reflective": 0.2}}


def _faces():
    glass = {"transparency": 0.8, "refractive-index": 1.5, "reflective": 0.3, "diffuse": 0.2}
    objs = [
        _cube([{"translate": [0, 1, 0]}]),                                                # faces x = +-1, y = 0 (ON the floor) and 2, z = +-1
        _cube([{"translate": [0, 3, 0]}], diffuse=0.5),                                   # stacked: its bottom face is the first one's top face
        _cube([{"translate": [2, 1, 0]}], reflective=0.4),                                # beside: faces x = 1 touch; its top face y = 2 is seen from above
        _cube([{"rotate-y": 0.6}, {"shear": {"xy": 0.4, "zy": -0.3}}, {"rotate-z": 0.2}, {"translate": [-3.5, 1.3, 1]}]),
        _cube([{"scale": [0.3, 1.7, 0.9]}, {"rotate-y": -0.4}, {"translate": [4.6, 1.7, 2]}]),
        _cube([{"scale": [0.8, 0.8, 0.8]}, {"rotate-y": 0.5}, {"translate": [-1.8, 0.8, -2.5]}], **glass),
        _cube([{"scale": [0.5, 0.5, 0.5]}, {"translate": [2.5, 0.5, -3]}], **dict(glass, **{"refractive-index": 1.1})),   # the third light is inside
        {"type": {"sphere": {}}, "transform": [{"scale": [0.6, 0.6, 0.6]}, {"translate": [-0.5, 0.6, -3.5]}], "material": {"reflective": 0.3}},
    ]
    lights = [{"point-light": {"position": [-4, GRAZE_Y + 1e-13, -5], "intensity": [0.4, 0.4, 0.4]}},   # a hair above the over_points of the top face y = 2 ...
              {"point-light": {"position": [6, GRAZE_Y - 1e-13, -4], "intensity": [0.3, 0.3, 0.3]}},    # ... and a hair below them
              {"point-light": {"position": [2.5, 0.5, -3], "intensity": [0.3, 0.3, 0.3]}}]
    # 63 x 47: the centre pixel's ray goes through `to`, the corner (1, 2, -1) of the first cube; from x = 1, so the centre
    # column looks along the face x = 1 and the edge x = 1, z = -1
    camera = {"width": 63, "height": 47, "field-of-view": 1.2, "from": [1, 6, -9], "to": [1, 2, -1], "up": [0, 1, 0]}
    return camera, lights, objs, [_floor()]


def _room():
    objs = [
        _cube([{"scale": [12, 12, 12]}, {"translate": [0, 11.5, 0]}], diffuse=0.6, reflective=0.2),    # the room: camera and lights inside
        _cube([{"translate": [-2, 0.5, 2]}], reflective=0.5),
        _cube([{"scale": [0.7, 0.7, 0.7]}, {"rotate-y": 0.8}, {"translate": [1.5, 0.2, 0]}], transparency=0.7, **{"refractive-index": 1.3}),
        _cube([{"scale": [1, 0.2, 1]}, {"translate": [3, 2, 4]}]),
        {"type": {"sphere": {}}, "transform": [{"translate": [0, 0.5, 4]}], "material": {"reflective": 0.4}},
    ]
    lights = [{"point-light": {"position": [-5, 8, -6], "intensity": [0.6, 0.6, 0.6]}},
              {"point-light": {"position": [6, 3, 2], "intensity": [0.4, 0.4, 0.4]}}]
    camera = {"width": 64, "height": 48, "field-of-view": 1.3, "from": [0.5, 2.5, -9], "to": [0, 0.5, 1], "up": [0, 1, 0]}
    return camera, lights, objs, []


def _blocks():
    objs = []
    for i in range(64):   # 56 cubes (every one reflective: a hit leaves three rays standing on it) and 8 spheres
        x, z = (i % 8 - 3.5) * 1.2, (i // 8) * 1.2 - 2.0
        if i % 8 == 3:
            objs.append({"type": {"sphere": {}}, "transform": [{"scale": [0.4, 0.4, 0.4]}, {"translate": [x, 0.4, z]}], "material": {"reflective": 0.2}})
        else:
            objs.append(_cube([{"scale": [0.4, 0.3 + 0.05 * (i % 5), 0.4]}, {"rotate-y": 0.21 * i}, {"translate": [x, 0.3 + 0.05 * (i % 5), z]}],
                              diffuse=round(0.4 + 0.1 * (i % 4), 3)))
    lights = [{"point-light": {"position": [-8, 9, -7], "intensity": [0.6, 0.6, 0.6]}},
              {"point-light": {"position": [7, 5, -4], "intensity": [0.4, 0.4, 0.4]}}]
    camera = {"width": 64, "height": 48, "field-of-view": 1.1, "from": [0.4, 6, -11], "to": [0, 0.3, 2], "up": [0, 1, 0]}
    return camera, lights, objs, [_floor()]


WORLDS = {"faces": _faces, "room": _room, "blocks": _blocks}

# variant -> (what is added to the world, [(options, kernel)]); an option not named is the library's own choice (-1)
OPTIONS = ("box_cull", "simple3_min_chunks", "waves3")
FORMS = {
    "simple": [({"box_cull": 1, "simple3_min_chunks": 1e9}, "rtc_render_kernel_simple_b"), ({"box_cull": 1, "simple3_min_chunks": 0}, "rtc_render_kernel_simple3_b"),
               ({"box_cull": 0, "simple3_min_chunks": 1e9}, "rtc_render_kernel_simple"), ({"box_cull": 0, "simple3_min_chunks": 0}, "rtc_render_kernel_simple3")],
    "flat": [({}, "rtc_render_kernel_flat")],
    "group": [({"waves3": 0}, "rtc_render_kernel"), ({"waves3": 1}, "rtc_render_kernel3")],
}


def _scene(world, variant):
    camera, lights, objs, planes = WORLDS[world]()
    if variant == "flat":     # a leaf kind the simple kernels do not carry
        objs = objs + [{"type": {"cylinder": {"min": -1, "max": 1, "closed": True}}, "transform": [{"scale": [0.3, 0.5, 0.3]}, {"translate": [-5.5, 0.5, 5]}]}]
    elif variant == "group":  # a group at top level: the general root loop, the cubes stay top-level objects
        objs = objs + [{"type": {"group": [{"type": {"sphere": {}}, "transform": [{"scale": [0.3, 0.3, 0.3]}, {"translate": [-5.5, 0.3, 5]}]},
                                           _cube([{"scale": [0.3, 0.3, 0.3]}, {"translate": [-5.5, 0.9, 5]}])]}}]
    return json.dumps({"camera": camera, "lights": lights, "objects": objs + planes})


@pytest.mark.parametrize("variant", list(FORMS))
@pytest.mark.parametrize("world", list(WORLDS))
def test_cubes_behind_the_origin(rtc, world, variant):
    hs = rtc.HostScene(_scene(world, variant))
    cam = hs.camera()
    assert cam.hsize <= 64 and cam.vsize <= 48
    if world == "blocks":
        assert hs.desc.n_roots >= 65   # 64 bounded roots and the floor
    want, counters = ob.OracleScene(hs.desc).render(cam, DEPTH)
    assert counters["secondary"] > 0 and counters["shadow"] > 0, (world, variant)
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
        print(f"{world} {variant} {kernel}: max |delta| {delta.max():.3e}")
        assert np.isfinite(got).all() and delta.max() < TOL, (world, variant, kernel, float(delta.max()), np.unravel_index(np.argmax(delta), delta.shape))
        assert [st["overflow"], st["primary"], st["secondary"], st["shadow_calls"]] == \
            [0, counters["primary"], counters["secondary"], counters["shadow"]], (world, variant, kernel)


def test_the_lights_graze_the_top_face(rtc):
    """The `faces` world is only a test of a grazing light if light_dot_normal on the third cube's top face is within 1e-12
    of 0, positive for the first light and negative for the second.  Recomputed on the host for every pixel whose ray meets
    that face (x in (1, 3), y = 2, z in (-1, 1); the camera stands at x = 1 and above everything in front of the face, so
    nothing hides it): the ray as camera.zig builds it, the hit as the cube's test finds it in object space (the cube is
    moved by (2, 1, 0), nothing else), over_point = point + 1e-5 normal, lightv = normalize(light - over_point)."""
    hs = rtc.HostScene(_scene("faces", "simple"))
    cam = hs.camera()
    inv = np.array(list(cam.inv_view)).reshape(4, 4)
    px, py = np.meshgrid(np.arange(cam.hsize), np.arange(cam.vsize))
    wx = cam.half_width - (px + 0.5) * cam.pixel_size
    wy = cam.half_height - (py + 0.5) * cam.pixel_size
    pixel = np.stack([wx, wy, -np.ones_like(wx), np.ones_like(wx)], axis=-1) @ inv.T
    origin = inv @ np.array([0.0, 0.0, 0.0, 1.0])
    d = pixel[..., :3] - origin[:3]
    d /= np.sqrt((d * d).sum(axis=-1, keepdims=True))
    with np.errstate(all="ignore"):
        t = (1.0 - (origin[1] - 1.0)) / d[..., 1]            # the object-space quotient of the face y = 1
        point = origin[:3] + t[..., None] * d
    on_face = (d[..., 1] < 0) & (point[..., 0] > 1.01) & (point[..., 0] < 2.99) & (np.abs(point[..., 2]) < 0.99)
    assert on_face.sum() >= 20, int(on_face.sum())
    over = point[on_face] + 1e-5 * np.array([0.0, 1.0, 0.0])
    _, lights, _, _ = _faces()
    for light, sign in ((lights[0], 1.0), (lights[1], -1.0)):
        lv = np.array(light["point-light"]["position"]) - over
        ldn = lv[:, 1] / np.sqrt((lv * lv).sum(axis=1))
        print(f"light_dot_normal on the top face: {ldn.min():.3e} .. {ldn.max():.3e} over {len(ldn)} pixels")
        assert (np.abs(ldn) < 1e-12).all() and (ldn * sign > 0).all(), (ldn.min(), ldn.max())
