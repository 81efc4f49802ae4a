"""Normal perturbation on the GPU (rtc_scene_set_bumps, the bump kernels): every bumped render against the checker
(tests/cpp/bump_oracle.cpp) within 1e-12 with equal ray counts and no overflow and with no pixel masked - sampling with a
lens, a later pass, a moving root, the light table's edge in both kernel forms -, the bumped image against the un-bumped
one, a scene whose bumped material no ray reaches, the bump kernels on a handle without bumps against its ordinary render,
the kernel's name, the setter's refusals and the reset, clones and band clones, Progressive, an adaptive run and
rtch_scene_render."""
import json

import numpy as np
import pytest

import bump_binding as bb
import camera_binding as cb
import test_table_limits_gpu as limits

pytestmark = pytest.mark.gpu

TOL = 1e-12         # (tests/test_spot_lights_gpu.py: a render against its checker)
SPLIT_TOL = 1e-14   # (tests/test_sampling_gpu.py: shares of a split frame's pixels added in another order)
L_LIGHTS = limits.LIMITS["LDS"]["LIGHTS"]
NONE, NOISE, RIPPLES = 0, 1, 2
BUMP, BUMP_BIG = "rtc_render_kernel_bump", "rtc_render_kernel_bump_bigworld"


def compare(got, want):
    """No mask: a bump feeds no geometric decision."""
    delta = float(np.abs(got - want).max())
    print(f"max |delta| {delta:.3e}")
    assert delta <= TOL, f"max |delta| {delta}"


def check(rtc, hs, cam, bumps, smp=None, sample_pass=0, disp=None, depth=5, light_seed=0, kernel=BUMP):
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    if smp is not None:
        gpu.set_sampling(smp)
    if light_seed:
        gpu.set_light_seed(light_seed)
    if sample_pass:
        gpu.set_sample_pass(sample_pass)
    if disp is not None:
        gpu.set_motion(disp)
    spots = hs.spots()
    gpu.set_spots(spots)
    gpu.set_bumps(bumps)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    assert gpu.last_kernel_name() == kernel
    want, counters = bb.BumpScene(hs.desc, hs.lights, bumps).render(cam, depth, smp, spots, disp, sample_pass, light_seed=light_seed)
    print({k: st[k] for k in ("primary", "secondary", "shadow_calls", "shadow_traced", "overflow")}, counters)
    compare(got, want)
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    grid = smp.grid if smp is not None else 1
    assert st["primary"] == cam.hsize * cam.vsize * grid * grid
    assert st["overflow"] == 0
    return got, gpu


# ---- the fixture against the checker: 80 x 45, depth 5
def test_fixture_against_the_checker(rtc):
    hs = bb.mix(rtc)
    check(rtc, hs, hs.camera(80, 45), hs.bumps(), light_seed=3)


def test_fixture_with_a_sample_grid_and_a_lens(rtc):
    hs = bb.mix(rtc)
    check(rtc, hs, hs.camera(80, 45), hs.bumps(), cb.sampling(2, True, aperture=0.08, focal_distance=6.0, seed=5), light_seed=3)


def test_fixture_at_sample_pass_3(rtc):
    hs = bb.mix(rtc)
    cam = hs.camera(80, 45)
    p0, _ = check(rtc, hs, cam, hs.bumps(), cb.sampling(1, True, seed=2))
    p3, _ = check(rtc, hs, cam, hs.bumps(), cb.sampling(1, True, seed=2), sample_pass=3)
    assert not np.array_equal(p0, p3)


def test_fixture_with_a_moving_root(rtc):
    hs = bb.mix(rtc)
    disp = np.zeros((hs.desc.n_roots, 3))
    disp[1] = (0.5, 0.0, 0.3)      # the noisy reflective sphere: its field moves with it
    check(rtc, hs, hs.camera(80, 45), hs.bumps(), cb.sampling(2, True, seed=6), disp=disp, light_seed=11)


def _with_many_lights(n):
    """bump_mix.json with point lights added until it has n: RTC_LDS_LIGHTS lights select the LDS kernel, one more the
    big-world one (tests/test_spot_lights_gpu.py's way)"""
    scene = json.loads(open(bb.BUMP_MIX).read())
    k = 0
    while len(scene["lights"]) < n:
        a = 0.7 * k
        scene["lights"].append({"point-light": {"position": [6 * np.cos(a), 6 + k % 3, 6 * np.sin(a)], "intensity": [0.03, 0.03, 0.04]}})
        k += 1
    return json.dumps(scene)


@pytest.mark.parametrize("extra", [0, 1])
def test_fixture_in_both_kernel_forms(rtc, extra):
    hs = rtc.HostScene(_with_many_lights(L_LIGHTS + extra), bb.BUMP_DIR)
    assert hs.lights.n_lights == L_LIGHTS + extra
    check(rtc, hs, hs.camera(80, 45), hs.bumps(), light_seed=3, kernel=BUMP_BIG if extra else BUMP)


# ---- bumped against un-bumped
def test_bumps_change_the_bumped_objects_pixels_only(rtc):
    """A matte floor nothing is reflected in, a bumped sphere and an un-bumped one far apart, one light straight above:
    pixels that show the un-bumped sphere or the floor away from the bumped sphere's shadow keep their bits."""
    cam = {"width": 96, "height": 48, "field-of-view": 1.0, "from": [0, 1.5, -7], "to": [0, 0.8, 0], "up": [0, 1, 0]}
    objects = [{"type": {"plane": {}}, "material": {"specular": 0}},
               {"type": {"sphere": {}}, "transform": [{"translate": [-2, 1, 0]}],
                "material": {"normal-perturbation": {"type": "noise", "amplitude": 0.4, "transform": [{"scale": [0.2, 0.2, 0.2]}]}}},
               {"type": {"sphere": {}}, "transform": [{"translate": [2, 1, 0]}], "material": {"diffuse": 0.8}}]
    text = json.dumps({"camera": cam, "lights": [{"point-light": {"position": [0, 9, 0], "intensity": [1, 1, 1]}}], "objects": objects})
    hs = rtc.HostScene(text)
    c = hs.camera()
    plain = rtc.GpuScene(hs.desc, lights=hs.lights)
    flat = plain.render(c, 5)
    bumped, gpu = check(rtc, hs, c, hs.bumps())
    differs = np.abs(bumped - flat).max(axis=2) > 0
    assert not differs[:, 48:].any()                 # the right half: the un-bumped sphere, floor, sky - the old kernel's bits
    assert differs[:, :48].mean() > 0.05             # the bumped sphere's pixels
    assert float(np.abs(bumped - flat).max()) > 0.05


def test_a_bumped_material_no_ray_reaches_leaves_every_bit(rtc):
    """The bumped sphere lies behind the camera of a scene without reflection: the bump kernel's image is the ordinary one's."""
    cam = {"width": 64, "height": 36, "field-of-view": 0.8, "from": [0, 1.5, -6], "to": [0, 1, 0], "up": [0, 1, 0]}
    objects = [{"type": {"plane": {}}, "material": {"specular": 0, "pattern": {"type": {"checkers": [{"type": {"solid": [1, 1, 1]}},
                                                                                                  {"type": {"solid": [0.2, 0.2, 0.2]}}]}}}},
               {"type": {"cube": {}}, "transform": [{"rotate-y": 0.5}, {"translate": [0, 1, 0]}], "material": {"diffuse": 0.6}},
               {"type": {"sphere": {}}, "transform": [{"translate": [0, 1, -40]}], "casts-shadow": False,
                "material": {"normal-perturbation": {"type": "ripples", "amplitude": 0.5}}}]
    text = json.dumps({"camera": cam, "lights": [{"point-light": {"position": [-4, 8, -4], "intensity": [1, 1, 1]}}], "objects": objects})
    hs = rtc.HostScene(text)
    c = hs.camera()
    plain = rtc.GpuScene(hs.desc, lights=hs.lights)
    flat = plain.render(c, 5)
    assert "_bump" not in plain.last_kernel_name()
    bumped, _ = check(rtc, hs, c, hs.bumps())
    assert np.array_equal(bumped, flat)


# ---- the bump kernels on a handle without bumps; the kernel's name
@pytest.mark.parametrize("name", ["cover.json", "spot_mix"])
def test_bump_kernels_without_bumps_are_the_ordinary_render(rtc, name):
    hs = rtc.HostScene.from_file(bb.SPOT_MIX if name == "spot_mix" else name)
    cam = hs.camera(128, 72)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_spots(hs.spots())
    ordinary = gpu.render(cam, 5)
    st0 = gpu.stats()
    old_name = gpu.last_kernel_name()
    assert "_bump" not in old_name
    rtc.set_option("bump_kernels", 1)
    try:
        forced = gpu.render(cam, 5)
        st1 = gpu.stats()
        assert gpu.last_kernel_name() == BUMP
    finally:
        rtc.set_option("bump_kernels", 0)
    delta = float(np.abs(forced - ordinary).max())
    print(f"{name}: {old_name} against {BUMP}: max |delta| {delta:.3e}")
    assert delta <= SPLIT_TOL
    for k in ("primary", "secondary", "shadow_calls", "overflow"):
        assert st0[k] == st1[k], k
    # (cover's handle may move between its ordinary kernels while it measures them, and cover has a material both
    # transparent and reflective: the ordinary renders are held to each other within SPLIT_TOL, spot_mix's by name too)
    def ordinary_again():
        again = gpu.render(cam, 5)
        assert float(np.abs(again - ordinary).max()) <= SPLIT_TOL
        assert "_bump" not in gpu.last_kernel_name()
        assert name == "cover.json" or gpu.last_kernel_name() == old_name
    ordinary_again()
    n = hs.desc.n_materials
    bumps = rtc.no_bumps(n)
    bumps["kind"][0], bumps["amplitude"][0] = RIPPLES, 0.1
    gpu.set_bumps(bumps)
    gpu.render(cam, 5)
    assert gpu.last_kernel_name() == BUMP
    gpu.set_bumps(None)
    ordinary_again()


# ---- refusals change nothing; NULL, every kind none and every amplitude 0 are the old handle again, bit for bit
def test_refused_settings_and_reset(rtc):
    hs = bb.mix(rtc)
    cam = hs.camera(80, 45)
    plain = rtc.GpuScene(hs.desc, lights=hs.lights)
    plain.set_spots(hs.spots())
    old = plain.render(cam, 5)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_spots(hs.spots())
    bumps = hs.bumps()
    gpu.set_bumps(bumps)
    lit = gpu.render(cam, 5)
    assert gpu.last_kernel_name() == BUMP and not np.array_equal(lit, old)
    n = hs.desc.n_materials
    bad = []
    for k, v in (("kind", 3), ("amplitude", -0.5), ("amplitude", np.nan), ("octaves", 0), ("octaves", 17), ("persistence", np.inf)):
        b = {kk: np.array(vv) for kk, vv in bumps.items()}
        b[k][1] = v
        bad.append(b)
    b = {kk: np.array(vv) for kk, vv in bumps.items()}
    b["inverse"][0, 3] = np.nan
    bad.append(b)
    bad.append({k: np.array(v)[:n - 1] for k, v in bumps.items()})
    for b in bad:
        with pytest.raises(rtc.RtcError) as e:
            gpu.set_bumps(b)
        assert e.value.name == "InvalidArgument"
        assert np.array_equal(gpu.render(cam, 5), lit)
        assert gpu.last_kernel_name() == BUMP
    gpu.set_bumps(None)
    assert np.array_equal(gpu.render(cam, 5), old)
    assert gpu.last_kernel_name() == plain.last_kernel_name()
    gpu.set_bumps(bumps)
    gpu.set_bumps(rtc.no_bumps(n))
    assert np.array_equal(gpu.render(cam, 5), old) and gpu.last_kernel_name() == plain.last_kernel_name()
    zero = {k: np.array(v) for k, v in bumps.items()}
    zero["amplitude"][:] = 0.0
    gpu.set_bumps(bumps)
    gpu.set_bumps(zero)
    assert np.array_equal(gpu.render(cam, 5), old) and gpu.last_kernel_name() == plain.last_kernel_name()
    # one material of amplitude 0 beside bumped ones takes the unperturbed branch: the checker says the same
    part = {k: np.array(v) for k, v in bumps.items()}
    part["amplitude"][0] = 0.0
    check(rtc, hs, cam, part)


# ---- a clone, band clones
def test_a_clone_and_band_clones_follow(rtc):
    hs = bb.mix(rtc)
    cam = hs.camera(160, 96)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_spots(hs.spots())
    rtc.set_option("host_bands", 3)
    try:
        first = gpu.render(cam, 5)          # makes the band clones, without bumps
        gpu.set_bumps(hs.bumps())
        banded = gpu.render(cam, 5)
        st = gpu.stats()
    finally:
        rtc.set_option("host_bands", 0)
    want, counters = bb.BumpScene(hs.desc, hs.lights, hs.bumps()).render(cam, 5, spots=hs.spots())
    compare(banded, want)
    assert st["primary"] == counters["primary"] and st["shadow_calls"] == counters["shadow_calls"]
    assert not np.array_equal(first, banded)
    whole = gpu.render(cam, 5)
    assert float(np.abs(whole - banded).max()) <= SPLIT_TOL
    clone = gpu.clone()            # a clone starts with its source's bumps
    assert float(np.abs(clone.render(cam, 5) - whole).max()) <= SPLIT_TOL
    assert clone.last_kernel_name() == BUMP
    gpu.set_bumps(None)            # ... and keeps them
    assert float(np.abs(clone.render(cam, 5) - whole).max()) <= SPLIT_TOL


# ---- Progressive, an adaptive run, rtch_scene_render
def _pass_images(hs, cam, smp, n):
    ck = bb.BumpScene(hs.desc, hs.lights, hs.bumps())
    return [ck.render(cam, 5, smp, hs.spots(), sample_pass=p)[0] for p in range(n)]


def test_progressive_mean_is_the_checkers(rtc):
    import torch
    hs = bb.mix(rtc)
    cam = hs.camera(64, 36)
    smp = cb.sampling(1, True, seed=4)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(smp)
    gpu.set_spots(hs.spots())
    gpu.set_bumps(hs.bumps())
    prog = rtc.Progressive(gpu, cam, 5)
    for _ in range(4):
        prog.step()
    mean = prog.mean().cpu().numpy()
    torch.cuda.synchronize()
    assert gpu.last_kernel_name() == BUMP
    compare(mean, np.mean(_pass_images(hs, cam, smp, 4), axis=0))


def test_adaptive_and_host_render_of_the_fixture(rtc):
    scene = json.loads(open(bb.BUMP_MIX).read())
    scene["camera"].update(width=80, height=48, sampling={"grid": 1, "jitter": True, "seed": 4, "passes": 6,
                                                          "adaptive": {"threshold": 0.004, "min-passes": 2, "tile": [16, 16]}})
    hs = rtc.HostScene(json.dumps(scene), bb.BUMP_DIR)
    a = hs.adaptive()
    out = np.zeros((48, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, 5, out.ctypes.data))
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_sampling(hs.sampling())
    gpu.set_spots(hs.spots())
    gpu.set_bumps(hs.bumps())
    rgb, passes = gpu.render_adaptive(hs.camera(), a)
    assert gpu.last_kernel_name() == BUMP
    run = rtc.AdaptiveProgressive(gpu, hs.camera(), 5, a)
    run.run()
    mean = run.mean().cpu().numpy()
    assert np.array_equal(out, rgb) and np.array_equal(rgb, mean)
    assert passes.min() >= 2 and passes.max() <= 6
    # each tile's mean over its own passes, from the checker's pass images
    images = _pass_images(hs, hs.camera(), hs.sampling(), 6)
    want = np.zeros_like(rgb)
    tiles_x = 80 // 16
    for t, k in enumerate(passes):
        ty, tx = divmod(t, tiles_x)
        want[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = np.mean([im[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] for im in images[:k]], axis=0)
    compare(rgb, want)
    # without "adaptive": rtch_scene_render is one rtc_render of the bumped handle
    plain = bb.mix(rtc)
    out1 = np.zeros((45, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(plain._h, 80, 45, 5, out1.ctypes.data))
    want1, _ = bb.BumpScene(plain.desc, plain.lights, plain.bumps()).render(plain.camera(80, 45), 5, spots=plain.spots())
    compare(out1, want1)
