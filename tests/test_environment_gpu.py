"""The environment on the GPU (rtc_scene_set_environment, the environment kernels): every render of the
fixture against the checker (tests/cpp/environment_oracle.cpp) within 1e-12 with equal ray counts, no overflow and no pixel
masked - default sampling, a sample grid with a lens, a later pass, a moving occluder under a sun, both kernel forms, band
clones and a clone, a shuffled tile list, Progressive, an adaptive run, rtch_scene_render -, the sky box, the derived small
cases of tests/test_environment_cpu.py, the counts against the same handle without an environment, the environment kernels
forced on handles without one, and the setter's refusals.  80 x 45 at depth 5 unless stated.

Figures: DESIGN.md section 24."""
import json

import numpy as np
import pytest

import camera_binding as cb
import environment_binding as eb
import gloss_binding as gb
import media_binding as mdb
import meshuv_binding as mb
import occlusion_binding as ob
import sfilter_binding as sb
import test_environment_cpu as cpu
import test_table_limits_gpu as limits
import torus_binding as tb

pytestmark = pytest.mark.gpu

TOL = 1e-12         # (the suite's bound for a render against its checker: test_media_gpu.py's)
FORCED_TOL = 1e-14  # (the bound of the last features for their kernels forced on a handle against the handle's ordinary render)
SPLIT_TOL = 1e-14   # (shares of a split frame's pixels added in another order: tests/test_meshuv_gpu.py)
L_LIGHTS = limits.LIMITS["LDS"]["LIGHTS"]
ENV, ENV_BIG = "rtc_render_kernel_env", "rtc_render_kernel_env_bigworld"
MEDIA = "rtc_render_kernel_media"
W, H, DEPTH = 80, 45, 5


def compare(got, want, tol=TOL):
    """No mask: every pixel counts."""
    delta = float(np.abs(got - want).max())
    print(f"max |delta| {delta:.3e}")
    assert delta <= tol, f"max |delta| {delta}"


def handle(rtc, hs, smp=None, sample_pass=0, disp=None, light_seed=0, environment="scene"):
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
    gpu.set_gloss(hs.gloss())
    gpu.set_occlusion(hs.occlusion())
    gpu.set_shadow_filters(hs.shadow_filters())
    gpu.set_media(hs.media())
    gpu.set_environment(hs.environment() if isinstance(environment, str) else environment)
    return gpu


def checker(rtc, hs, environment="scene"):
    return eb.scene_of(rtc, hs, "file" if isinstance(environment, str) else environment)


def same_counts(st, counters):
    print({k: st[k] for k in ("primary", "secondary", "shadow_calls", "shadow_traced", "overflow")}, counters)
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    assert st["overflow"] == 0


def check(rtc, hs, cam, smp=None, sample_pass=0, disp=None, light_seed=0, kernel=ENV, environment="scene", depth=DEPTH):
    gpu = handle(rtc, hs, smp, sample_pass, disp, light_seed, environment)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    assert gpu.last_kernel_name() == kernel
    want, counters = checker(rtc, hs, environment).render(cam, depth, smp, hs.spots(), disp, sample_pass, light_seed=light_seed)
    compare(got, want)
    same_counts(st, counters)
    grid = smp.grid if smp is not None else 1
    assert st["primary"] == cam.hsize * cam.vsize * grid * grid
    return got, gpu, counters


# ---- the fixture against the checker
def test_fixture_against_the_checker(rtc):
    hs = eb.mix(rtc)
    got, gpu, c = check(rtc, hs, hs.camera(W, H), light_seed=3)
    for k in eb.ENV_COUNTERS:
        assert c[k] > 0, k
    assert got.std() > 0.05


def test_fixture_with_a_sample_grid_and_a_lens(rtc):
    hs = eb.mix(rtc)
    check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, aperture=0.08, focal_distance=9.0, seed=5), light_seed=3)


def test_fixture_at_sample_pass_3(rtc):
    hs = eb.mix(rtc)
    cam = hs.camera(W, H)
    p0, _, _ = check(rtc, hs, cam, cb.sampling(1, True, seed=2), light_seed=3)
    p3, _, _ = check(rtc, hs, cam, cb.sampling(1, True, seed=2), sample_pass=3, light_seed=3)
    assert not np.array_equal(p0, p3)


def test_fixture_with_a_moving_occluder_under_a_sun(rtc):
    hs = eb.mix(rtc)
    far = hs.desc.n_roots - 1                   # the last root: the occluder far above the scene, in the high sun's way
    disp = np.zeros((hs.desc.n_roots, 3))
    disp[far] = (2.5, 0.0, -1.5)                # its shadow sweeps the floor while the shutter is open
    moving, _, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, seed=6), disp=disp, light_seed=11)
    still, _, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, seed=6), light_seed=11)
    assert not np.array_equal(moving, still)


def _with_many_lights(n):
    """sky_mix.json with point lights added until it has n: RTC_LDS_LIGHTS lights select the LDS kernel, one more the
    big-world one (tests/test_media_gpu.py's way); the suns do not count"""
    scene = json.loads(open(eb.SKY_MIX).read())
    k = 0
    while len(scene["lights"]) < n:
        a = 0.7 * k
        scene["lights"].append({"point-light": {"position": [6 * np.cos(a), 6 + k % 3, 6 * np.sin(a)], "intensity": [0.03, 0.03, 0.04]}})
        k += 1
    return json.dumps(scene)


@pytest.mark.parametrize("extra", [0, 1])
def test_fixture_in_both_kernel_forms(rtc, extra):
    hs = rtc.HostScene(_with_many_lights(L_LIGHTS + extra))
    assert hs.lights.n_lights == L_LIGHTS + extra and len(hs.environment()["sun_rgb"]) == 2
    check(rtc, hs, hs.camera(W, H), light_seed=3, kernel=ENV_BIG if extra else ENV)


# ---- band clones, a clone, a shuffled tile list
def test_a_clone_and_band_clones_follow(rtc):
    hs = eb.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs)
    rtc.set_option("host_bands", 3)
    try:
        banded = gpu.render(cam, DEPTH)
        st = gpu.stats()
    finally:
        rtc.set_option("host_bands", 0)
    want, counters = checker(rtc, hs).render(cam, DEPTH, spots=hs.spots())
    compare(banded, want)
    same_counts(st, counters)   # (the bands' counts, summed)
    whole = gpu.render(cam, DEPTH)
    assert float(np.abs(whole - banded).max()) <= SPLIT_TOL
    clone = gpu.clone()
    assert float(np.abs(clone.render(cam, DEPTH) - whole).max()) <= SPLIT_TOL   # a clone starts with its source's environment
    assert clone.last_kernel_name() == ENV
    # the setter after the band clones exist: they follow
    other = hs.environment()
    other["rgb"] = [0.4, 0.6, 0.5]
    other["sun_direction"] = other["sun_direction"][::-1].copy()
    gpu.set_environment(other)
    rtc.set_option("host_bands", 3)
    try:
        banded2 = gpu.render(cam, DEPTH)
    finally:
        rtc.set_option("host_bands", 0)
    want2, _ = checker(rtc, hs, other).render(cam, DEPTH, spots=hs.spots())
    compare(banded2, want2)
    assert not np.array_equal(banded2, banded)


def test_a_shuffled_tile_list(rtc):
    import torch
    hs = eb.mix(rtc)
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
    assert gpu.last_kernel_name() == ENV
    want, counters = checker(rtc, hs).render(cam, DEPTH, spots=hs.spots())
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
    hs = eb.mix(rtc)
    cam = hs.camera(W, H)
    smp = cb.sampling(1, True, seed=4)
    gpu = handle(rtc, hs, smp)
    ck = checker(rtc, hs)
    want = [ck.render(cam, DEPTH, smp, hs.spots(), sample_pass=p) for p in range(4)]
    prog = rtc.Progressive(gpu, cam, DEPTH)
    for p in range(4):
        prog.step()
        same_counts(gpu.stats(), want[p][1])                    # (the handle's counts are its last launch's: pass p)
    mean = prog.mean().cpu().numpy()
    torch.cuda.synchronize()
    assert gpu.last_kernel_name() == ENV
    compare(mean, np.mean([im for im, _ in want], axis=0))


def test_adaptive_and_host_render_of_the_fixture(rtc):
    scene = json.loads(open(eb.SKY_MIX).read())
    scene["camera"].update(width=80, height=48, sampling={"grid": 1, "jitter": True, "seed": 4, "passes": 5, "occlusion-seed": 7,
                                                          "occlusion-samples": 2,
                                                          "adaptive": {"threshold": 0.004, "min-passes": 2, "tile": [16, 16]}})
    hs = rtc.HostScene(json.dumps(scene))
    a = hs.adaptive()
    out = np.zeros((48, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, DEPTH, out.ctypes.data))
    gpu = handle(rtc, hs, hs.sampling())
    rgb, passes = gpu.render_adaptive(hs.camera(), a)
    assert gpu.last_kernel_name() == ENV
    assert np.array_equal(out, rgb)
    assert passes.min() >= 2 and passes.max() <= 5
    ck = checker(rtc, hs)
    images = [ck.render(hs.camera(), DEPTH, hs.sampling(), hs.spots(), sample_pass=p)[0] for p in range(5)]
    want = np.zeros_like(rgb)
    tiles_x = 80 // 16
    for t, k in enumerate(passes):
        ty, tx = divmod(t, tiles_x)
        want[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = np.mean([im[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] for im in images[:k]], axis=0)
    compare(rgb, want)
    # without "adaptive": rtch_scene_render is one rtc_render of the handle, the environment applied.  (Its handle lives and
    # dies inside the call, so of the host render the image alone is held to the checker.)
    plain = eb.mix(rtc)
    out1 = np.zeros((H, W, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(plain._h, W, H, DEPTH, out1.ctypes.data))
    want1, _ = checker(rtc, plain).render(plain.camera(W, H), DEPTH, spots=plain.spots())
    compare(out1, want1)
    # ... and it is not the same file's render without its environment
    bare = checker(rtc, plain, None).render(plain.camera(W, H), DEPTH, spots=plain.spots())[0]
    assert float(np.abs(out1 - bare).max()) > 0.1


# ---- the sky box
def test_sky_box_against_the_checker(rtc):
    hs = eb.box(rtc)
    got, _, c = check(rtc, hs, hs.camera(80, 40))
    assert c["miss_camera"] > 0 and c["miss_reflected"] > 0 and c["miss_refracted"] > 0 and got.std() > 0.05


# ---- the derived small cases, on the GPU
def _gpu_render(rtc, scene, depth):
    """The scene on the environment kernels, held to the checker."""
    hs = rtc.HostScene(scene)
    gpu = handle(rtc, hs)
    got = gpu.render(hs.camera(), depth)
    assert gpu.last_kernel_name() == ENV
    st = gpu.stats()
    want, c = checker(rtc, hs).render(hs.camera(), depth, spots=hs.spots())
    compare(got, want)
    same_counts(st, c)
    return got, st["shadow_traced"]


def test_derived_cases_on_the_gpu(rtc):
    """An empty world under a sky and in fog, stripes and gradient skies in both projections, a mirror floor, a sun on a
    matte floor, occluders 1e6 units up and down its line and a closed room of two sizes at 9 x 9, against the values derived
    in tests/test_environment_cpu.py."""
    cpu.check_derived_cases(lambda scene, depth: _gpu_render(rtc, scene, depth))


# ---- the counts; which kernel
def test_counts_against_the_handle_without_an_environment(rtc):
    hs = eb.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs, light_seed=3, environment=None)
    without = gpu.render(cam, DEPTH)
    st0 = gpu.stats()
    assert gpu.last_kernel_name() == MEDIA
    gpu.set_environment(hs.environment())
    with_env = gpu.render(cam, DEPTH)
    st1 = gpu.stats()
    assert gpu.last_kernel_name() == ENV and not np.array_equal(with_env, without)
    for k in ("primary", "secondary", "overflow"):
        assert st0[k] == st1[k], k
    _, c = checker(rtc, hs).render(cam, DEPTH, spots=hs.spots(), light_seed=3)
    hits = c["primary"] + c["secondary"] - (c["miss_camera"] + c["miss_reflected"] + c["miss_refracted"] + c["miss_dark"])
    assert st1["shadow_calls"] == st0["shadow_calls"] + 2 * hits          # n_suns per hit
    assert st1["shadow_traced"] == st0["shadow_traced"] + c["sun_clear"] + c["sun_blocked"] + c["sun_partial"]


def test_null_and_the_all_zero_table_restore_the_media_kernel(rtc):
    hs = eb.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs, environment=None)
    bare = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == MEDIA
    gpu.set_environment(hs.environment())
    assert not np.array_equal(gpu.render(cam, DEPTH), bare) and gpu.last_kernel_name() == ENV
    gpu.set_environment({"rgb": [0.0, 0.0, 0.0], "projection": rtc.ENV_CUBE})
    assert np.array_equal(gpu.render(cam, DEPTH), bare) and gpu.last_kernel_name() == MEDIA
    gpu.set_environment(hs.environment())
    gpu.set_environment(None)
    assert np.array_equal(gpu.render(cam, DEPTH), bare) and gpu.last_kernel_name() == MEDIA
    # a sky colour alone selects the environment kernels; so does a sun alone
    gpu.set_environment({"rgb": [0.0, 0.25, 0.0]})
    sky = gpu.render(cam, DEPTH)
    assert not np.array_equal(sky, bare) and gpu.last_kernel_name() == ENV
    want, _ = checker(rtc, hs, {"rgb": [0.0, 0.25, 0.0]}).render(cam, DEPTH, spots=hs.spots())
    compare(sky, want)
    gpu.set_environment({"sun_direction": [[0, -1, 0]], "sun_rgb": [[0.5, 0.5, 0.5]]})
    assert not np.array_equal(gpu.render(cam, DEPTH), bare) and gpu.last_kernel_name() == ENV


@pytest.mark.parametrize("name", ["cover.json", "media_mix", "filter_mix", "occlusion_mix", "gloss_mix", "torus_mix", "mesh_mix", "teapot.json"])
def test_environment_kernels_without_an_environment_are_the_ordinary_render(rtc, name):
    hs = gb.mix(rtc) if name == "gloss_mix" else mb.mix(rtc) if name == "mesh_mix" else tb.mix(rtc) if name == "torus_mix" \
        else ob.mix(rtc) if name == "occlusion_mix" else sb.mix(rtc) if name == "filter_mix" else mdb.mix(rtc) if name == "media_mix" \
        else rtc.HostScene.from_file(name)
    cam = hs.camera(W, H)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_spots(hs.spots())
    gpu.set_bumps(hs.bumps())
    gpu.set_mesh_uvs(hs.mesh_uvs())
    gpu.set_gloss(hs.gloss())
    gpu.set_occlusion(hs.occlusion())
    gpu.set_shadow_filters(hs.shadow_filters())
    gpu.set_media(hs.media())
    ordinary = gpu.render(cam, DEPTH)
    st0 = gpu.stats()
    old_name = gpu.last_kernel_name()
    assert "_env" not in old_name
    rtc.set_option("environment_kernels", 1)
    try:
        forced = gpu.render(cam, DEPTH)
        st1 = gpu.stats()
        assert gpu.last_kernel_name() == ENV
    finally:
        rtc.set_option("environment_kernels", 0)
    delta = float(np.abs(forced - ordinary).max())
    print(f"{name}: {old_name} against {ENV}: max |delta| {delta:.3e}")
    assert delta <= FORCED_TOL
    for k in ("primary", "secondary", "shadow_calls", "overflow"):
        assert st0[k] == st1[k], k
    again = gpu.render(cam, DEPTH)
    assert float(np.abs(again - ordinary).max()) <= FORCED_TOL
    assert gpu.last_kernel_name() == old_name


# ---- rtc_scene_set_environment
def _status_name(rtc, code):
    return rtc.hip_lib().rtc_status_name(code).decode()


def test_selection_refusals_and_reset(rtc):
    hs = eb.mix(rtc)
    cam = hs.camera(W, H)
    e = hs.environment()
    gpu = handle(rtc, hs, environment=None)
    bare = gpu.render(cam, DEPTH)
    old_name = gpu.last_kernel_name()
    assert old_name == MEDIA         # (the fixture has absorbing glass)
    gpu.set_environment(e)
    first = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == ENV and not np.array_equal(first, bare)
    clone = gpu.clone()

    def poked(**kw):
        out = dict(e, rgb=list(e["rgb"]), sun_direction=e["sun_direction"].copy(), sun_rgb=e["sun_rgb"].copy())
        for k, v in kw.items():
            if k == "colour":
                out["rgb"][v[0]] = v[1]
            elif k in ("sun_direction", "sun_rgb") and isinstance(v, tuple):
                out[k][v[0], v[1]] = v[2]
            else:
                out[k] = v
        return out

    bad = [poked(colour=(1, np.nan)), poked(colour=(0, -1e-9)), poked(colour=(2, np.inf)), poked(pattern=hs.desc.n_patterns),
           poked(projection=2), poked(sun_rgb=(1, 2, -0.5)), poked(sun_rgb=(0, 0, np.nan)), poked(sun_direction=(0, 1, np.inf)),
           poked(sun_direction=np.zeros((2, 3))), poked(sun_direction=np.tile(e["sun_direction"][0], (17, 1)), sun_rgb=np.ones((17, 3)))]
    for target in (gpu, clone):
        for b in bad:
            with pytest.raises(rtc.RtcError) as err:
                target.set_environment(b)
            assert err.value.name == _status_name(rtc, 1)                 # RTC_ERR_INVALID_ARGUMENT
        got = target.render(cam, DEPTH)                                   # the refused tables changed nothing
        assert float(np.abs(got - first).max()) <= SPLIT_TOL and target.last_kernel_name() == ENV
    # NULL restores the previous kernel and its bits; the clone keeps its own table
    gpu.set_environment(None)
    assert np.array_equal(gpu.render(cam, DEPTH), bare) and gpu.last_kernel_name() == old_name
    assert float(np.abs(clone.render(cam, DEPTH) - first).max()) <= SPLIT_TOL and clone.last_kernel_name() == ENV
    clone.set_environment(None)
    assert np.array_equal(clone.render(cam, DEPTH), bare) and clone.last_kernel_name() == old_name
