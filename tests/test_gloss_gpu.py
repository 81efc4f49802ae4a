"""Glossy reflection and refraction on the GPU (rtc_scene_set_gloss, the gloss kernels): every render of
the fixture against the checker (tests/cpp/gloss_oracle.cpp) within 1e-12 with equal ray counts, no overflow and no pixel
masked - default sampling, a sample grid with a lens, a later pass, a moving root, both kernel forms, band clones, a
shuffled tile list, Progressive, an adaptive run, rtch_scene_render -, a deep ray tree whose path codes reach 17 bits, gloss
against no gloss, the gloss kernels forced on handles without a rough material, the kernel's name, the setter's refusals,
and the seed.  80 x 45 at depth 5 unless stated.

Figures: DESIGN.md section 20."""
import json

import numpy as np
import pytest

import camera_binding as cb
import gloss_binding as gb
import meshuv_binding as mb
import test_table_limits_gpu as limits
import torus_binding as tb

pytestmark = pytest.mark.gpu

TOL = 1e-12         # (the issue's bound for a render against its checker)
FORCED_TOL = 1e-14  # (the issue's bound for the gloss kernels forced on a handle against the handle's ordinary render)
SPLIT_TOL = 1e-14   # (shares of a split frame's pixels added in another order: tests/test_meshuv_gpu.py)
L_LIGHTS = limits.LIMITS["LDS"]["LIGHTS"]
GLOSS, GLOSS_BIG = "rtc_render_kernel_gloss", "rtc_render_kernel_gloss_bigworld"
W, H, DEPTH = 80, 45, 5


def compare(got, want, tol=TOL):
    """No mask: every pixel counts."""
    delta = float(np.abs(got - want).max())
    print(f"max |delta| {delta:.3e}")
    assert delta <= tol, f"max |delta| {delta}"


def handle(rtc, hs, smp=None, sample_pass=0, disp=None, light_seed=0, gloss="scene"):
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    if smp is not None:
        gpu.set_sampling(smp)
    if light_seed:
        gpu.set_light_seed(light_seed)
    if sample_pass:
        gpu.set_sample_pass(sample_pass)
    if disp is not None:
        gpu.set_motion(disp)
    gpu.set_spots(hs.spots())
    gpu.set_bumps(hs.bumps())
    gpu.set_mesh_uvs(hs.mesh_uvs())
    gpu.set_gloss(hs.gloss() if isinstance(gloss, str) else gloss)
    return gpu


def checker(hs, gloss="scene"):
    return gb.GlossScene(hs.desc, hs.lights, hs.bumps(), hs.mesh_uvs(), hs.gloss() if isinstance(gloss, str) else gloss)


def same_counts(st, counters):
    print({k: st[k] for k in ("primary", "secondary", "shadow_calls", "shadow_traced", "overflow")}, counters)
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    assert st["overflow"] == 0


def check(rtc, hs, cam, smp=None, sample_pass=0, disp=None, light_seed=0, kernel=GLOSS, gloss="scene", depth=DEPTH):
    gpu = handle(rtc, hs, smp, sample_pass, disp, light_seed, gloss)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    assert gpu.last_kernel_name() == kernel
    want, counters = checker(hs, gloss).render(cam, depth, smp, hs.spots(), disp, sample_pass, light_seed=light_seed)
    compare(got, want)
    same_counts(st, counters)
    grid = smp.grid if smp is not None else 1
    assert st["primary"] == cam.hsize * cam.vsize * grid * grid
    return got, gpu, counters


# ---- the fixture against the checker
def test_fixture_against_the_checker(rtc):
    hs = gb.mix(rtc)
    g = hs.gloss()
    assert np.count_nonzero(g["reflection"]) == 6 and np.count_nonzero(g["transmission"]) == 3 and len(tb.tori_of(hs.desc)) == 1
    got, _, counters = check(rtc, hs, hs.camera(W, H), light_seed=3)
    assert counters["used"] > 0 and counters["fell_back"] > 0   # both branches of the side rule are in the picture
    assert got.std() > 0.05


def test_fixture_with_a_sample_grid_and_a_lens(rtc):
    hs = gb.mix(rtc)
    check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, aperture=0.08, focal_distance=7.0, seed=5), light_seed=3)


def test_fixture_at_sample_pass_3(rtc):
    hs = gb.mix(rtc)
    cam = hs.camera(W, H)
    p0, _, _ = check(rtc, hs, cam, cb.sampling(1, False))   # (gloss is sampled even without jitter)
    p3, _, _ = check(rtc, hs, cam, cb.sampling(1, False), sample_pass=3)
    assert not np.array_equal(p0, p3)


def test_fixture_with_a_moving_root(rtc):
    hs = gb.mix(rtc)
    disp = np.zeros((hs.desc.n_roots, 3))
    disp[1] = (0.5, 0.0, 0.3)
    moving, _, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, seed=6), disp=disp, light_seed=11)
    still, _, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, seed=6), light_seed=11)
    assert not np.array_equal(moving, still)


def _with_many_lights(n):
    """gloss_mix.json with point lights added until it has n: RTC_LDS_LIGHTS lights select the LDS kernel, one more the
    big-world one (tests/test_torus_gpu.py's way)"""
    scene = json.loads(open(gb.GLOSS_MIX).read())
    k = 0
    while len(scene["lights"]) < n:
        a = 0.7 * k
        scene["lights"].append({"point-light": {"position": [6 * np.cos(a), 6 + k % 3, 6 * np.sin(a)], "intensity": [0.03, 0.03, 0.04]}})
        k += 1
    return json.dumps(scene)


@pytest.mark.parametrize("extra", [0, 1])
def test_fixture_in_both_kernel_forms(rtc, extra):
    hs = rtc.HostScene(_with_many_lights(L_LIGHTS + extra), gb.GLOSS_DIR)
    assert hs.lights.n_lights == L_LIGHTS + extra
    check(rtc, hs, hs.camera(W, H), light_seed=3, kernel=GLOSS_BIG if extra else GLOSS)


# ---- band clones, a clone, a shuffled tile list
def test_a_clone_and_band_clones_follow(rtc):
    hs = gb.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs)
    rtc.set_option("host_bands", 3)
    try:
        banded = gpu.render(cam, DEPTH)
        st = gpu.stats()
    finally:
        rtc.set_option("host_bands", 0)
    want, counters = checker(hs).render(cam, DEPTH, spots=hs.spots())
    compare(banded, want)
    same_counts(st, counters)   # (the bands' counts, summed)
    whole = gpu.render(cam, DEPTH)
    assert float(np.abs(whole - banded).max()) <= SPLIT_TOL
    clone = gpu.clone()
    assert np.array_equal(clone.render(cam, DEPTH), whole)   # a clone starts with its source's table
    assert clone.last_kernel_name() == GLOSS
    # the setter after the band clones exist: they follow
    other = dict(hs.gloss(), seed=9)
    gpu.set_gloss(other)
    rtc.set_option("host_bands", 3)
    try:
        banded9 = gpu.render(cam, DEPTH)
    finally:
        rtc.set_option("host_bands", 0)
    want9, _ = checker(hs, other).render(cam, DEPTH, spots=hs.spots())
    compare(banded9, want9)
    assert not np.array_equal(banded9, banded)


def test_a_shuffled_tile_list(rtc):
    import torch
    hs = gb.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs)
    tw, th = 16, 16
    tiles_x, tiles_y = -(-W // tw), -(-H // th)
    n_tiles = tiles_x * tiles_y
    tiles = np.random.default_rng(5).permutation(n_tiles).astype(np.uint32)
    buf = torch.zeros((n_tiles, th, tw, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    gpu.render_tile_list_device(cam, buf.data_ptr(), tw, th, tiles, DEPTH)
    gpu.synchronize()
    st = gpu.stats()
    assert gpu.last_kernel_name() == GLOSS
    want, counters = checker(hs).render(cam, DEPTH, spots=hs.spots())
    b = buf.cpu().numpy()
    got = np.zeros((H, W, 3))
    for k, t in enumerate(tiles):
        ty, tx = divmod(int(t), tiles_x)
        h, w = min(th, H - ty * th), min(tw, W - tx * tw)
        got[ty * th:ty * th + h, tx * tw:tx * tw + w] = b[k, :h, :w]
    compare(got, want)
    same_counts(st, counters)


# ---- Progressive, an adaptive run, rtch_scene_render
def test_progressive_mean_is_the_checkers(rtc):
    import torch
    hs = gb.mix(rtc)
    cam = hs.camera(W, H)
    smp = cb.sampling(1, True, seed=4)
    gpu = handle(rtc, hs, smp)
    ck = checker(hs)
    want = [ck.render(cam, DEPTH, smp, hs.spots(), sample_pass=p) for p in range(4)]
    prog = rtc.Progressive(gpu, cam, DEPTH)
    for p in range(4):
        prog.step()
        same_counts(gpu.stats(), want[p][1])                    # (the handle's counts are its last launch's: pass p)
    mean = prog.mean().cpu().numpy()
    torch.cuda.synchronize()
    assert gpu.last_kernel_name() == GLOSS
    compare(mean, np.mean([im for im, _ in want], axis=0))


def test_adaptive_and_host_render_of_the_fixture(rtc):
    scene = json.loads(open(gb.GLOSS_MIX).read())
    scene["camera"].update(width=80, height=48, sampling={"grid": 1, "jitter": True, "seed": 4, "passes": 5, "gloss-seed": 7,
                                                          "adaptive": {"threshold": 0.004, "min-passes": 2, "tile": [16, 16]}})
    hs = rtc.HostScene(json.dumps(scene), gb.GLOSS_DIR)
    assert hs.gloss()["seed"] == 7
    a = hs.adaptive()
    out = np.zeros((48, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, DEPTH, out.ctypes.data))
    gpu = handle(rtc, hs, hs.sampling())
    rgb, passes = gpu.render_adaptive(hs.camera(), a)
    assert gpu.last_kernel_name() == GLOSS
    assert np.array_equal(out, rgb)
    assert passes.min() >= 2 and passes.max() <= 5
    ck = checker(hs)
    images = [ck.render(hs.camera(), DEPTH, hs.sampling(), hs.spots(), sample_pass=p)[0] for p in range(5)]
    want = np.zeros_like(rgb)
    tiles_x = 80 // 16
    for t, k in enumerate(passes):
        ty, tx = divmod(t, tiles_x)
        want[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = np.mean([im[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] for im in images[:k]], axis=0)
    compare(rgb, want)
    # without "adaptive": rtch_scene_render is one rtc_render of the handle, the roughness rows applied.  (Its handle lives
    # and dies inside the call, so of the host render the image alone is held to the checker.)
    plain = gb.mix(rtc)
    out1 = np.zeros((H, W, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(plain._h, W, H, DEPTH, out1.ctypes.data))
    want1, _ = checker(plain).render(plain.camera(W, H), DEPTH, spots=plain.spots())
    compare(out1, want1)


# ---- a deep ray tree
def _mirror_hall():
    """Two facing rough mirrors with a rough glass pane between them, seen at a slant: every level of the tree has a
    reflection and a refraction."""
    cam = {"width": 16, "height": 9, "field-of-view": 0.9, "from": [0.4, 0.3, -1.6], "to": [0, 0, 2], "up": [0, 1, 0]}
    mirror = {"pattern": {"type": {"solid": [0.1, 0.12, 0.1]}}, "diffuse": 0.3, "specular": 0.2, "reflective": 0.9,
              "roughness": {"reflection": 0.04}}
    glass = {"pattern": {"type": {"solid": [0.05, 0.05, 0.1]}}, "diffuse": 0.1, "reflective": 0.6, "transparency": 0.9,
             "refractive-index": 1.3, "roughness": {"reflection": 0.03, "transmission": 0.05}}
    objects = [{"type": {"cube": {}}, "transform": [{"scale": [3, 3, 0.05]}, {"translate": [0, 0, 2]}], "material": mirror},
               {"type": {"cube": {}}, "transform": [{"scale": [3, 3, 0.05]}, {"translate": [0, 0, -2]}], "material": mirror},
               {"type": {"cube": {}}, "transform": [{"scale": [3, 3, 0.05]}, {"rotate-y": 0.2}], "material": glass}]
    lights = [{"point-light": {"position": [0.5, 2, -1], "intensity": [0.9, 0.9, 0.9]}}]
    return json.dumps({"camera": cam, "lights": lights, "objects": objects})


def test_a_deep_tree_at_max_depth_16(rtc):
    hs = rtc.HostScene(_mirror_hall(), gb.GLOSS_DIR)
    _, _, counters = check(rtc, hs, hs.camera(), depth=16)
    print("secondary per primary", counters["secondary"] / counters["primary"])
    # (one child a level is at most 16 secondary rays a primary: more means levels with both children, the refraction pushed
    # and popped.  144 pixels with trees of a thousand rays in three waves: lanes run dry and take over pending rays - the
    # handle's counters do not show a hand-out, the equal image and counts are what holds it.)
    assert counters["secondary"] > 16 * counters["primary"]


# ---- gloss against no gloss
def _two_spheres():
    """A matte floor, a rough mirror sphere and a smooth mirror sphere far apart (the smooth one shows the rough one small)"""
    cam = {"width": 96, "height": 48, "field-of-view": 1.0, "from": [0, 1.5, -7], "to": [0, 0.8, 0], "up": [0, 1, 0]}
    floor = {"type": {"plane": {}}, "material": {"specular": 0, "pattern": {"type": {"solid": [0.7, 0.7, 0.7]}}}}
    rough = {"type": {"sphere": {}}, "transform": [{"translate": [-2.5, 1, 0]}],
             "material": {"pattern": {"type": {"solid": [0.6, 0.3, 0.3]}}, "reflective": 0.6, "roughness": 0.3}}
    smooth = {"type": {"sphere": {}}, "transform": [{"translate": [2.5, 1, 0]}],
              "material": {"pattern": {"type": {"solid": [0.3, 0.3, 0.6]}}, "reflective": 0.6}}
    lights = [{"point-light": {"position": [0, 9, -3], "intensity": [1, 1, 1]}}]
    return json.dumps({"camera": cam, "lights": lights, "objects": [floor, rough, smooth]})


def test_only_pixels_that_meet_a_rough_material_differ(rtc):
    """Which pixels' trees meet the rough material is the checker's count of scattered children, pixel by pixel: every
    pixel outside that set has the bits of the render without gloss."""
    hs = rtc.HostScene(_two_spheres(), gb.GLOSS_DIR)
    c = hs.camera()
    glossy, gpu, _ = check(rtc, hs, c)
    gpu.set_gloss(None)
    sharp = gpu.render(c, DEPTH)
    assert gpu.last_kernel_name() != GLOSS
    ck = checker(hs)
    meets = np.zeros((c.vsize, c.hsize), dtype=bool)
    for y in range(c.vsize):
        for x in range(c.hsize):
            n = ck.render(c, DEPTH, tile=(x, y, 1, 1), threads=1)[1]
            meets[y, x] = n["used"] + n["fell_back"] > 0
    differ = (glossy != sharp).any(axis=2)
    print("pixels that meet the rough sphere", int(meets.sum()), "that differ", int(differ.sum()))
    assert differ.any() and not (differ & ~meets).any()
    assert meets[:, :48].sum() > 100 and 0 < meets[:, 48:].sum() < meets[:, :48].sum()   # the sphere itself; its image in the other
    assert (~meets).sum() > meets.sum()                                                   # most of the frame is untouched


def test_a_rough_material_no_ray_reaches_leaves_every_bit(rtc):
    cam = {"width": 64, "height": 36, "field-of-view": 0.8, "from": [0, 1.5, -6], "to": [0, 1, 0], "up": [0, 1, 0]}
    objects = [{"type": {"plane": {}}, "material": {"specular": 0, "pattern": {"type": {"checkers": [{"type": {"solid": [1, 1, 1]}},
                                                                                                   {"type": {"solid": [0.2, 0.2, 0.2]}}]}}}},
               {"type": {"sphere": {}}, "transform": [{"translate": [0, 1, 0]}],
                "material": {"pattern": {"type": {"solid": [0.3, 0.3, 0.6]}}, "transparency": 0.5, "refractive-index": 1.2}},
               {"type": {"sphere": {}}, "transform": [{"translate": [0, 1, -30]}], "casts-shadow": False,
                "material": {"reflective": 0.5, "roughness": 0.5}}]
    lights = [{"point-light": {"position": [3, 9, -3], "intensity": [1, 1, 1]}}]
    hs = rtc.HostScene(json.dumps({"camera": cam, "lights": lights, "objects": objects}), gb.GLOSS_DIR)
    c = hs.camera()
    glossy, gpu, counters = check(rtc, hs, c)
    assert counters["used"] + counters["fell_back"] == 0
    gpu.set_gloss(None)
    assert np.array_equal(gpu.render(c, DEPTH), glossy)
    assert gpu.last_kernel_name() != GLOSS


# ---- which kernel; the gloss kernels on a handle without a rough material
@pytest.mark.parametrize("name", ["cover.json", "mesh_mix", "torus_mix", "teapot.json"])
def test_gloss_kernels_without_gloss_are_the_ordinary_render(rtc, name):
    hs = mb.mix(rtc) if name == "mesh_mix" else tb.mix(rtc) if name == "torus_mix" else rtc.HostScene.from_file(name)
    cam = hs.camera(W, H)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_spots(hs.spots())
    gpu.set_bumps(hs.bumps())
    gpu.set_mesh_uvs(hs.mesh_uvs())
    ordinary = gpu.render(cam, DEPTH)
    st0 = gpu.stats()
    old_name = gpu.last_kernel_name()
    assert "_gloss" not in old_name
    rtc.set_option("gloss_kernels", 1)
    try:
        forced = gpu.render(cam, DEPTH)
        st1 = gpu.stats()
        assert gpu.last_kernel_name() == GLOSS
    finally:
        rtc.set_option("gloss_kernels", 0)
    delta = float(np.abs(forced - ordinary).max())
    print(f"{name}: {old_name} against {GLOSS}: max |delta| {delta:.3e}")
    assert delta <= FORCED_TOL
    for k in ("primary", "secondary", "shadow_calls", "overflow"):
        assert st0[k] == st1[k], k
    again = gpu.render(cam, DEPTH)
    assert float(np.abs(again - ordinary).max()) <= FORCED_TOL
    assert gpu.last_kernel_name() == old_name


# ---- rtc_scene_set_gloss
def _status_name(rtc, code):
    return rtc.hip_lib().rtc_status_name(code).decode()


def test_selection_refusals_and_reset(rtc):
    hs = gb.mix(rtc)
    cam = hs.camera(W, H)
    g = hs.gloss()
    n = hs.desc.n_materials
    gpu = handle(rtc, hs, gloss=None)
    sharp = gpu.render(cam, DEPTH)
    old_name = gpu.last_kernel_name()
    assert old_name == "rtc_render_kernel_meshuv"        # (the fixture has a mesh map and a torus)
    gpu.set_gloss(g)
    first = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == GLOSS and not np.array_equal(first, sharp)
    clone = gpu.clone()
    bad = [dict(g, reflection=g["reflection"][:-1], transmission=g["transmission"][:-1]),
           dict(g, reflection=np.where(np.arange(n) == 2, np.nan, g["reflection"])),
           dict(g, reflection=np.where(np.arange(n) == 2, np.inf, g["reflection"])),
           dict(g, transmission=np.where(np.arange(n) == 1, 1.0000001, g["transmission"])),
           dict(g, transmission=np.where(np.arange(n) == 0, -1e-9, g["transmission"]))]
    for target in (gpu, clone):
        for b in bad:
            with pytest.raises(rtc.RtcError) as e:
                target.set_gloss(b)
            assert e.value.name == _status_name(rtc, 1)                   # RTC_ERR_INVALID_ARGUMENT
            assert np.array_equal(target.render(cam, DEPTH), first)       # a refused table changes nothing
            assert target.last_kernel_name() == GLOSS
    # an array that is missing is all zeros
    gpu.set_gloss({"reflection": g["reflection"]})
    want, _ = checker(hs, {"reflection": g["reflection"], "transmission": np.zeros(n)}).render(cam, DEPTH, spots=hs.spots())
    compare(gpu.render(cam, DEPTH), want)
    # all-zero rows and NULL restore the previous kernel and its bits; the clone keeps its own table
    gpu.set_gloss({"reflection": np.zeros(n), "transmission": np.zeros(n), "seed": 5})
    assert np.array_equal(gpu.render(cam, DEPTH), sharp) and gpu.last_kernel_name() == old_name
    gpu.set_gloss(g)
    assert np.array_equal(gpu.render(cam, DEPTH), first)
    gpu.set_gloss(None)
    assert np.array_equal(gpu.render(cam, DEPTH), sharp) and gpu.last_kernel_name() == old_name
    assert np.array_equal(clone.render(cam, DEPTH), first) and clone.last_kernel_name() == GLOSS
    clone.set_gloss(None)
    assert np.array_equal(clone.render(cam, DEPTH), sharp) and clone.last_kernel_name() == old_name


def test_two_seeds_differ_on_rough_pixels_only(rtc):
    hs = gb.mix(rtc)
    cam = hs.camera(W, H)
    g = hs.gloss()
    a, gpu, _ = check(rtc, hs, cam, gloss=dict(g, seed=1))
    b, _, _ = check(rtc, hs, cam, gloss=dict(g, seed=2))
    gpu.set_gloss(None)
    sharp = gpu.render(cam, DEPTH)
    rough = (a != sharp).any(axis=2) | (b != sharp).any(axis=2)
    differ = (a != b).any(axis=2)
    assert differ.any() and not (differ & ~rough).any()
    assert (~rough).any() and np.array_equal(a[~rough], b[~rough])
