"""The sky light on the GPU (rtc_scene_set_sky_light, the sky-light kernels): every render of the fixture
against the checker (tests/cpp/skylight_oracle.cpp) within 1e-12 with equal ray counts, no overflow and no pixel masked -
default sampling, a sample grid with a lens, a later pass, a moving occluder, 1, 4 and 64 samples, both kernel forms, band
clones and a clone, a shuffled tile list, Progressive, an adaptive run, rtch_scene_render -, the derived and the statistical
cases of tests/test_skylight_cpu.py, monotonicity, what restores the environment kernels, the order of the two setters, the
sky-light kernels forced on handles without a sky light, and the setter's refusals.  80 x 45 at depth 5 unless stated.

Figures: DESIGN.md section 25."""
import json

import numpy as np
import pytest

import camera_binding as cb
import environment_binding as eb
import media_binding as mdb
import occlusion_binding as ob
import sfilter_binding as fb
import skylight_binding as sb
import test_skylight_cpu as cpu
import test_table_limits_gpu as limits

pytestmark = pytest.mark.gpu

TOL = 1e-12         # (the suite's bound for a render against its checker: test_environment_gpu.py's)
FORCED_TOL = 1e-14  # (the bound of the last features for their kernels forced on a handle against the handle's ordinary render)
SPLIT_TOL = 1e-14   # (shares of a split frame's pixels added in another order: tests/test_meshuv_gpu.py)
L_LIGHTS = limits.LIMITS["LDS"]["LIGHTS"]
SKYL, SKYL_BIG = "rtc_render_kernel_skyl", "rtc_render_kernel_skyl_bigworld"
ENV = "rtc_render_kernel_env"
W, H, DEPTH = 80, 45, 5


def compare(got, want, tol=TOL):
    """No mask: every pixel counts."""
    delta = float(np.abs(got - want).max())
    print(f"max |delta| {delta:.3e}")
    assert delta <= tol, f"max |delta| {delta}"


def handle(rtc, hs, smp=None, sample_pass=0, disp=None, light_seed=0, sky_light="scene", environment="scene"):
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
    gpu.set_sky_light(hs.sky_light() if isinstance(sky_light, str) else sky_light)
    return gpu


def checker(rtc, hs, sky_light="scene", environment="scene"):
    return sb.scene_of(rtc, hs, "file" if isinstance(sky_light, str) else sky_light, "file" if isinstance(environment, str) else environment)


def same_counts(st, counters):
    print({k: st[k] for k in ("primary", "secondary", "shadow_calls", "shadow_traced", "overflow")}, counters)
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    assert st["overflow"] == 0


def check(rtc, hs, cam, smp=None, sample_pass=0, disp=None, light_seed=0, kernel=SKYL, sky_light="scene", depth=DEPTH):
    gpu = handle(rtc, hs, smp, sample_pass, disp, light_seed, sky_light)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    assert gpu.last_kernel_name() == kernel
    want, counters = checker(rtc, hs, sky_light).render(cam, depth, smp, hs.spots(), disp, sample_pass, light_seed=light_seed)
    compare(got, want)
    same_counts(st, counters)
    grid = smp.grid if smp is not None else 1
    assert st["primary"] == cam.hsize * cam.vsize * grid * grid
    return got, gpu, counters


# ---- the fixture against the checker
def test_fixture_against_the_checker(rtc):
    hs = sb.mix(rtc)
    got, gpu, c = check(rtc, hs, hs.camera(W, H), light_seed=3)
    for k in sb.SKY_COUNTERS:
        assert c[k] > 0, k
    assert got.std() > 0.05


def test_fixture_with_a_sample_grid_and_a_lens(rtc):
    hs = sb.mix(rtc)
    check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, aperture=0.08, focal_distance=9.0, seed=5), light_seed=3)


def test_fixture_at_sample_pass_3(rtc):
    hs = sb.mix(rtc)
    cam = hs.camera(W, H)
    p0, _, _ = check(rtc, hs, cam, cb.sampling(1, True, seed=2), light_seed=3)
    p3, _, _ = check(rtc, hs, cam, cb.sampling(1, True, seed=2), sample_pass=3, light_seed=3)
    assert not np.array_equal(p0, p3)


def test_fixture_with_a_moving_occluder(rtc):
    """The opaque slab over the floor moves while the shutter is open: the hemisphere rays meet it where it is at the ray's time."""
    hs = sb.mix(rtc)
    assert hs.desc.n_roots == 7
    disp = np.zeros((hs.desc.n_roots, 3))
    disp[1] = (1.5, 0.0, 0.8)                    # the second object of the file: the slab
    moving, _, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, seed=6), disp=disp, light_seed=11)
    still, _, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, seed=6), light_seed=11)
    assert not np.array_equal(moving, still)


@pytest.mark.parametrize("samples", [1, 4, 64])
def test_fixture_with_1_4_and_64_samples(rtc, samples):
    hs = sb.mix(rtc)
    _, _, c = check(rtc, hs, hs.camera(W, H), sky_light=dict(hs.sky_light(), samples=samples))
    assert (c["sky_clear"] + c["sky_partial"] + c["sky_blocked"]) % samples == 0


def _with_many_lights(n):
    """skylight_mix.json with point lights added until it has n: RTC_LDS_LIGHTS lights select the LDS kernel, one more the
    big-world one (tests/test_environment_gpu.py's way)"""
    scene = json.loads(open(sb.SKYLIGHT_MIX).read())
    k = 0
    while len(scene["lights"]) < n:
        a = 0.7 * k
        scene["lights"].append({"point-light": {"position": [6 * np.cos(a), 6 + k % 3, 6 * np.sin(a)], "intensity": [0.03, 0.03, 0.04]}})
        k += 1
    return json.dumps(scene)


@pytest.mark.parametrize("extra", [0, 1])
def test_fixture_in_both_kernel_forms(rtc, extra):
    hs = rtc.HostScene(_with_many_lights(L_LIGHTS + extra))
    assert hs.lights.n_lights == L_LIGHTS + extra and hs.sky_light()["samples"] == 4
    check(rtc, hs, hs.camera(W, H), light_seed=3, kernel=SKYL_BIG if extra else SKYL)


# ---- band clones, a clone, a shuffled tile list
def test_a_clone_and_band_clones_follow(rtc):
    hs = sb.mix(rtc)
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
    assert float(np.abs(clone.render(cam, DEPTH) - whole).max()) <= SPLIT_TOL   # a clone starts with its source's sky light
    assert clone.last_kernel_name() == SKYL
    # the setter after the band clones exist: they follow
    other = dict(hs.sky_light(), gain=1.7, samples=2, seed=5)
    gpu.set_sky_light(other)
    rtc.set_option("host_bands", 3)
    try:
        banded2 = gpu.render(cam, DEPTH)
    finally:
        rtc.set_option("host_bands", 0)
    want2, _ = checker(rtc, hs, other).render(cam, DEPTH, spots=hs.spots())
    compare(banded2, want2)
    assert not np.array_equal(banded2, banded)
    compare(clone.render(cam, DEPTH), want)      # ... and the clone keeps the table it started with


def test_a_shuffled_tile_list(rtc):
    import torch
    hs = sb.mix(rtc)
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
    assert gpu.last_kernel_name() == SKYL
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
    hs = sb.mix(rtc)
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
    assert gpu.last_kernel_name() == SKYL
    compare(mean, np.mean([im for im, _ in want], axis=0))
    assert not np.array_equal(want[0][0], want[1][0])           # the draws are new per pass


def test_adaptive_and_host_render_of_the_fixture(rtc):
    scene = json.loads(open(sb.SKYLIGHT_MIX).read())
    scene["camera"].update(width=80, height=48, sampling={"grid": 1, "jitter": True, "seed": 4, "passes": 5, "occlusion-seed": 5,
                                                          "occlusion-samples": 2,
                                                          "adaptive": {"threshold": 0.004, "min-passes": 2, "tile": [16, 16]}})
    hs = rtc.HostScene(json.dumps(scene))
    a = hs.adaptive()
    out = np.zeros((48, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, DEPTH, out.ctypes.data))
    gpu = handle(rtc, hs, hs.sampling())
    rgb, passes = gpu.render_adaptive(hs.camera(), a)
    assert gpu.last_kernel_name() == SKYL
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
    # without "adaptive": rtch_scene_render is one rtc_render of the handle, the environment and the sky light applied
    plain = sb.mix(rtc)
    out1 = np.zeros((H, W, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(plain._h, W, H, DEPTH, out1.ctypes.data))
    want1, _ = checker(rtc, plain).render(plain.camera(W, H), DEPTH, spots=plain.spots())
    compare(out1, want1)
    # ... and it is not the same file's render without its sky light
    bare = checker(rtc, plain, None).render(plain.camera(W, H), DEPTH, spots=plain.spots())[0]
    assert float(np.abs(out1 - bare).max()) > 0.1


# ---- the derived and the statistical cases, on the GPU
def _gpu_render(rtc, scene, depth):
    """The scene on the sky-light kernels (the environment kernels without the key), held to the checker."""
    hs = rtc.HostScene(scene)
    gpu = handle(rtc, hs)
    got = gpu.render(hs.camera(), depth)
    assert gpu.last_kernel_name() == (SKYL if hs.sky_light() is not None else ENV)
    st = gpu.stats()
    want, c = checker(rtc, hs).render(hs.camera(), depth, spots=hs.spots())
    compare(got, want)
    same_counts(st, c)
    assert st["shadow_traced"] == st["shadow_calls"]        # (no lights and no suns: every call is a sky-light sample, and traced)
    return got, st["shadow_calls"]


def test_derived_cases_on_the_gpu(rtc):
    """The open sky for 1, 2 and 4 samples, the opaque and the filtering lid, the filtering sphere around, the mirror floor
    and the counts at 9 x 9, against the values derived in tests/test_skylight_cpu.py."""
    cpu.check_derived_cases(lambda scene, depth: _gpu_render(rtc, scene, depth))


def _progressive_mean(rtc, scene):
    import torch
    hs = rtc.HostScene(scene)
    gpu = handle(rtc, hs)
    prog = rtc.Progressive(gpu, hs.camera(), DEPTH, noise=False)
    for _ in range(cpu.N_PASSES):
        prog.step()
    mean = prog.mean().cpu().numpy()
    torch.cuda.synchronize()
    assert gpu.last_kernel_name() == SKYL and gpu.stats()["overflow"] == 0
    want = cpu._mean_over_passes(rtc, scene)
    delta = float(np.abs(mean - want).max())
    print(f"256 passes against the checker's: max |delta| {delta:.3e}")
    assert delta <= TOL
    return mean


def test_half_the_rays_of_a_floor_see_the_white_half_of_the_sky(rtc):
    cpu.check_statistical_case("halves", _progressive_mean(rtc, cpu.halves_scene()), 0.5, cpu.BOUND_HALVES)


def test_the_mean_cosine_of_a_walls_rays_is_two_thirds(rtc):
    cpu.check_statistical_case("ramp", _progressive_mean(rtc, cpu.ramp_scene()), 2.0 / 3.0, cpu.BOUND_RAMP)


# ---- monotonicity; what restores the environment kernels; the order of the setters
def test_the_sky_only_adds_light(rtc):
    hs = sb.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs, light_seed=3, sky_light=None)
    without = gpu.render(cam, DEPTH)
    st0 = gpu.stats()
    assert gpu.last_kernel_name() == ENV
    gpu.set_sky_light(hs.sky_light())
    with_light = gpu.render(cam, DEPTH)
    st1 = gpu.stats()
    assert gpu.last_kernel_name() == SKYL
    print("least difference", float((with_light - without).min()), "largest", float((with_light - without).max()))
    assert (with_light >= without - TOL).all() and not np.array_equal(with_light, without)
    for k in ("primary", "secondary", "overflow"):
        assert st0[k] == st1[k], k
    _, c = checker(rtc, hs).render(cam, DEPTH, spots=hs.spots(), light_seed=3)
    n = c["sky_clear"] + c["sky_partial"] + c["sky_blocked"]
    assert st1["shadow_calls"] == st0["shadow_calls"] + n and st1["shadow_traced"] == st0["shadow_traced"] + n


def test_null_a_gain_of_zero_and_no_sky_restore_the_environment_kernel(rtc):
    hs = sb.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs, sky_light=None)
    bare = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == ENV
    light = hs.sky_light()
    gpu.set_sky_light(light)
    assert not np.array_equal(gpu.render(cam, DEPTH), bare) and gpu.last_kernel_name() == SKYL
    gpu.set_sky_light(dict(light, gain=0.0))
    assert np.array_equal(gpu.render(cam, DEPTH), bare) and gpu.last_kernel_name() == ENV
    gpu.set_sky_light(light)
    gpu.set_sky_light(None)
    assert np.array_equal(gpu.render(cam, DEPTH), bare) and gpu.last_kernel_name() == ENV
    # an environment without a sky - its suns alone -: the environment kernels with the table in place, and their bits
    gpu.set_sky_light(light)
    suns = dict(hs.environment(), rgb=[0.0, 0.0, 0.0], pattern=rtc.ENV_NO_PATTERN)
    gpu.set_environment(suns)
    got = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == ENV
    other = handle(rtc, hs, sky_light=None, environment=suns)
    assert np.array_equal(got, other.render(cam, DEPTH)) and other.last_kernel_name() == ENV
    # ... and the sky back: the sky light is still there
    gpu.set_environment(hs.environment())
    want, _ = checker(rtc, hs).render(cam, DEPTH, spots=hs.spots())
    compare(gpu.render(cam, DEPTH), want)
    assert gpu.last_kernel_name() == SKYL


def test_the_order_of_the_two_setters_does_not_matter(rtc):
    hs = sb.mix(rtc)
    cam = hs.camera(W, H)
    after = handle(rtc, hs).render(cam, DEPTH)                  # the environment, then the sky light
    gpu = handle(rtc, hs, sky_light=None, environment=None)
    gpu.set_sky_light(hs.sky_light())                           # the sky light first, on a handle without an environment
    gpu.render(cam, DEPTH)
    assert "_skyl" not in gpu.last_kernel_name() and "_env" not in gpu.last_kernel_name()
    gpu.set_environment(hs.environment())
    before = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == SKYL and np.array_equal(before, after)


@pytest.mark.parametrize("name", ["cover.json", "sky_mix", "media_mix", "filter_mix", "occlusion_mix", "teapot.json"])
def test_sky_light_kernels_without_a_sky_light_are_the_ordinary_render(rtc, name):
    hs = eb.mix(rtc) if name == "sky_mix" else ob.mix(rtc) if name == "occlusion_mix" else fb.mix(rtc) if name == "filter_mix" \
        else mdb.mix(rtc) if name == "media_mix" else rtc.HostScene.from_file(name)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs)
    ordinary = gpu.render(cam, DEPTH)
    st0 = gpu.stats()
    old_name = gpu.last_kernel_name()
    assert "_skyl" not in old_name
    rtc.set_option("sky_light_kernels", 1)
    try:
        forced = gpu.render(cam, DEPTH)
        st1 = gpu.stats()
        assert gpu.last_kernel_name() == SKYL
    finally:
        rtc.set_option("sky_light_kernels", 0)
    delta = float(np.abs(forced - ordinary).max())
    print(f"{name}: {old_name} against {SKYL}: max |delta| {delta:.3e}")
    assert delta <= FORCED_TOL
    for k in ("primary", "secondary", "shadow_calls", "overflow"):
        assert st0[k] == st1[k], k
    again = gpu.render(cam, DEPTH)
    assert float(np.abs(again - ordinary).max()) <= FORCED_TOL
    assert gpu.last_kernel_name() == old_name


# ---- rtc_scene_set_sky_light
def _status_name(rtc, code):
    return rtc.hip_lib().rtc_status_name(code).decode()


def test_refusals_change_nothing(rtc):
    hs = sb.mix(rtc)
    cam = hs.camera(W, H)
    light = hs.sky_light()
    gpu = handle(rtc, hs)
    first = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == SKYL
    clone = gpu.clone()
    bad = [dict(light, gain=np.nan), dict(light, gain=np.inf), dict(light, gain=-1e-9), dict(light, samples=0), dict(light, samples=65),
           dict(light, gain=0.0, samples=65)]
    for target in (gpu, clone):
        for b in bad:
            with pytest.raises(rtc.RtcError) as err:
                target.set_sky_light(b)
            assert err.value.name == _status_name(rtc, 1)                 # RTC_ERR_INVALID_ARGUMENT
        got = target.render(cam, DEPTH)                                   # the refused tables changed nothing
        assert float(np.abs(got - first).max()) <= SPLIT_TOL and target.last_kernel_name() == SKYL
    # NULL on the handle; the clone keeps its own table
    gpu.set_sky_light(None)
    assert gpu.render(cam, DEPTH) is not None and gpu.last_kernel_name() == ENV
    assert float(np.abs(clone.render(cam, DEPTH) - first).max()) <= SPLIT_TOL and clone.last_kernel_name() == SKYL
