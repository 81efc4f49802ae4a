"""Shadow filters on the GPU (rtc_scene_set_shadow_filters, the shadow-filter kernels): every render
of the fixture against the checker (tests/cpp/sfilter_oracle.cpp) within 1e-12 with equal ray counts, no overflow and no
pixel masked - default sampling, a sample grid with a lens, a later pass, a moving root that carries a filter, both kernel
forms, band clones and a clone, a shuffled tile list, Progressive, an adaptive run, rtch_scene_render -, the exact small
cases of tests/test_shadow_filter_cpu.py at 16 x 9, a light at an object's surface, the bounds between the all-opaque and the
"casts-shadow": false render, the shadow-filter kernels forced on handles without a filter, and the setter's refusals.
80 x 45 at depth 5 unless stated.

Figures: DESIGN.md section 22."""
import json

import numpy as np
import pytest

import camera_binding as cb
import gloss_binding as gb
import meshuv_binding as mb
import occlusion_binding as ob
import sfilter_binding as sb
import test_shadow_filter_cpu as cpu
import test_table_limits_gpu as limits
import torus_binding as tb

pytestmark = pytest.mark.gpu

TOL = 1e-12         # (the suite's bound for a render against its checker: test_occlusion_gpu.py's)
FORCED_TOL = 1e-14  # (the bound of the last two features for their kernels forced on a handle against the handle's ordinary render)
SPLIT_TOL = 1e-14   # (shares of a split frame's pixels added in another order: tests/test_meshuv_gpu.py)
L_LIGHTS = limits.LIMITS["LDS"]["LIGHTS"]
SFILT, SFILT_BIG = "rtc_render_kernel_sfilter", "rtc_render_kernel_sfilter_bigworld"
OCCL = "rtc_render_kernel_occl"
W, H, DEPTH = 80, 45, 5


def compare(got, want, tol=TOL):
    """No mask: every pixel counts."""
    delta = float(np.abs(got - want).max())
    print(f"max |delta| {delta:.3e}")
    assert delta <= tol, f"max |delta| {delta}"


def handle(rtc, hs, smp=None, sample_pass=0, disp=None, light_seed=0, filters="scene"):
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
    gpu.set_shadow_filters(hs.shadow_filters() if isinstance(filters, str) else filters)
    return gpu


def checker(rtc, hs, filters="scene"):
    return sb.scene_of(rtc, hs, "file" if isinstance(filters, str) else filters)


def same_counts(st, counters):
    print({k: st[k] for k in ("primary", "secondary", "shadow_calls", "shadow_traced", "overflow")}, counters)
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    assert st["overflow"] == 0


def check(rtc, hs, cam, smp=None, sample_pass=0, disp=None, light_seed=0, kernel=SFILT, filters="scene", depth=DEPTH):
    gpu = handle(rtc, hs, smp, sample_pass, disp, light_seed, filters)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    assert gpu.last_kernel_name() == kernel
    want, counters = checker(rtc, hs, filters).render(cam, depth, smp, hs.spots(), disp, sample_pass, light_seed=light_seed)
    compare(got, want)
    same_counts(st, counters)
    grid = smp.grid if smp is not None else 1
    assert st["primary"] == cam.hsize * cam.vsize * grid * grid
    return got, gpu, counters


# ---- the fixture against the checker
def test_fixture_against_the_checker(rtc):
    hs = sb.mix(rtc)
    got, gpu, c = check(rtc, hs, hs.camera(W, H), light_seed=3)
    n = c["t_one"] + c["t_partial"] + c["t_blocked"]
    assert c["t_partial"] >= 0.1 * n and c["t_blocked"] >= 0.1 * n and c["t_one"] >= 0.1 * n and c["three_partial"] >= 0.01 * n
    assert gpu.stats()["shadow_traced"] == n + c["occluded"] + c["unoccluded"]   # the rays the checker calls traced, and the occlusion rays
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


def test_fixture_with_a_moving_root_that_carries_a_filter(rtc):
    hs = sb.mix(rtc)
    assert hs.shadow_filters()["rgb"][int(hs.desc.leaf_material[3])].tolist() == [0.9, 0.3, 0.3]   # root 3: the tinted sphere
    disp = np.zeros((hs.desc.n_roots, 3))
    disp[3] = (0.6, 0.0, 0.4)
    moving, _, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, seed=6), disp=disp, light_seed=11)
    still, _, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, seed=6), light_seed=11)
    assert not np.array_equal(moving, still)


def _with_many_lights(n):
    """filter_mix.json with point lights added until it has n: RTC_LDS_LIGHTS lights select the LDS kernel, one more the
    big-world one (tests/test_torus_gpu.py's way)"""
    scene = json.loads(open(sb.SFILT_MIX).read())
    k = 0
    while len(scene["lights"]) < n:
        a = 0.7 * k
        scene["lights"].append({"point-light": {"position": [6 * np.cos(a), 6 + k % 3, 6 * np.sin(a)], "intensity": [0.03, 0.03, 0.04]}})
        k += 1
    return json.dumps(scene)


@pytest.mark.parametrize("extra", [0, 1])
def test_fixture_in_both_kernel_forms(rtc, extra):
    hs = rtc.HostScene(_with_many_lights(L_LIGHTS + extra), sb.SFILT_DIR)
    assert hs.lights.n_lights == L_LIGHTS + extra
    check(rtc, hs, hs.camera(W, H), light_seed=3, kernel=SFILT_BIG if extra else SFILT)


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
    assert np.array_equal(clone.render(cam, DEPTH), whole)   # a clone starts with its source's table
    assert clone.last_kernel_name() == SFILT
    # the setter after the band clones exist: they follow
    other = {"rgb": np.sqrt(hs.shadow_filters()["rgb"])}
    gpu.set_shadow_filters(other)
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
    assert gpu.last_kernel_name() == SFILT
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
    assert gpu.last_kernel_name() == SFILT
    compare(mean, np.mean([im for im, _ in want], axis=0))


def test_adaptive_and_host_render_of_the_fixture(rtc):
    scene = json.loads(open(sb.SFILT_MIX).read())
    scene["camera"].update(width=80, height=48, sampling={"grid": 1, "jitter": True, "seed": 4, "passes": 5, "occlusion-seed": 7,
                                                          "occlusion-samples": 2, "gloss-seed": 4,
                                                          "adaptive": {"threshold": 0.004, "min-passes": 2, "tile": [16, 16]}})
    hs = rtc.HostScene(json.dumps(scene), sb.SFILT_DIR)
    a = hs.adaptive()
    out = np.zeros((48, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, DEPTH, out.ctypes.data))
    gpu = handle(rtc, hs, hs.sampling())
    rgb, passes = gpu.render_adaptive(hs.camera(), a)
    assert gpu.last_kernel_name() == SFILT
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
    # without "adaptive": rtch_scene_render is one rtc_render of the handle, the filter rows applied.  (Its handle lives
    # and dies inside the call, so of the host render the image alone is held to the checker.)
    plain = sb.mix(rtc)
    out1 = np.zeros((H, W, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(plain._h, W, H, DEPTH, out1.ctypes.data))
    want1, _ = checker(rtc, plain).render(plain.camera(W, H), DEPTH, spots=plain.spots())
    compare(out1, want1)
    # ... and it is brighter than the same file's render without the key
    opaque = checker(rtc, plain, None).render(plain.camera(W, H), DEPTH, spots=plain.spots())[0]
    assert out1.mean() > opaque.mean()


# ---- the exact small cases, on the GPU
def _gpu_render(rtc, scene, light_seed=0, counters=None):
    """The scene on the shadow-filter kernels - also where it has no filter, so that every image of a comparison comes from
    one kernel -, held to the checker."""
    hs = rtc.HostScene(scene, sb.SFILT_DIR)
    gpu = handle(rtc, hs, light_seed=light_seed)
    rtc.set_option("shadow_filter_kernels", 1)
    try:
        got = gpu.render(hs.camera(), DEPTH)
        assert gpu.last_kernel_name() == SFILT
    finally:
        rtc.set_option("shadow_filter_kernels", 0)
    want, c = checker(rtc, hs).render(hs.camera(), DEPTH, spots=hs.spots(), light_seed=light_seed)
    compare(got, want)
    same_counts(gpu.stats(), c)
    if counters is not None:
        counters.update(c)
    return got


def test_small_cases_on_the_gpu(rtc):
    """One plane, the sphere squared, the light inside the sphere, the object behind, filter 1 against "casts-shadow": false
    and the stacked planes in two orders, at 16 x 9: a missed, doubled or misplaced factor shows as a full-scale difference,
    and the properties hold to the bit as they do on the checker."""
    cpu.check_small_cases(lambda scene: _gpu_render(rtc, scene))


def test_area_light_cases_on_the_gpu(rtc):
    cpu.check_area_cases(lambda scene: _gpu_render(rtc, scene, light_seed=5))


def test_an_entry_at_the_light_does_not_count(rtc):
    """The light lies in an opaque pane's plane: the pane's one entry of a shadow ray falls at t == distance - to the bit for
    the rays the checker counts as "at_light" -, and `t < distance` leaves it out: the floor is lit as without the pane.  A
    walk that took `t <= distance` would render those pixels black."""
    c = {}
    with_pane = _gpu_render(rtc, cpu.AT_LIGHT, counters=c)
    without = _gpu_render(rtc, cpu.AT_LIGHT_BARE)
    print("entries at t == distance:", c["at_light"], "blocked:", c["t_blocked"])
    assert c["at_light"] == 16 * 9 and c["t_blocked"] == 0   # (what the checker finds for this scene: tests/test_shadow_filter_cpu.py)
    assert (with_pane > 0).all() and np.array_equal(with_pane, without)


# ---- the bounds
def test_filtered_render_lies_between_opaque_and_no_shadow(rtc):
    hs = sb.mix(rtc)
    cam = hs.camera(W, H)
    filtered, gpu, _ = check(rtc, hs, cam, light_seed=3)
    gpu.set_shadow_filters(None)
    opaque = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == OCCL
    scene = json.loads(open(sb.SFILT_MIX).read())
    for o in scene["objects"]:
        if "shadow-filter" in o["material"]:
            del o["material"]["shadow-filter"]
            o["casts-shadow"] = False
    clear_hs = rtc.HostScene(json.dumps(scene), sb.SFILT_DIR)
    assert clear_hs.shadow_filters() is None
    clear = handle(rtc, clear_hs, light_seed=3).render(cam, DEPTH)
    assert (filtered >= opaque - 1e-12).all() and (filtered <= clear + 1e-12).all()
    assert not np.array_equal(filtered, opaque) and not np.array_equal(filtered, clear)


# ---- which kernel; the shadow-filter kernels on a handle without a filter
def test_an_all_zero_table_restores_the_occlusion_kernel(rtc):
    hs = sb.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs, filters=None)
    opaque = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == OCCL
    gpu.set_shadow_filters(hs.shadow_filters())
    assert not np.array_equal(gpu.render(cam, DEPTH), opaque) and gpu.last_kernel_name() == SFILT
    gpu.set_shadow_filters({"rgb": np.zeros((hs.desc.n_materials, 3))})
    assert np.array_equal(gpu.render(cam, DEPTH), opaque)
    assert gpu.last_kernel_name() == OCCL
    gpu.set_shadow_filters({"rgb": None, "n_materials": hs.desc.n_materials})
    assert np.array_equal(gpu.render(cam, DEPTH), opaque) and gpu.last_kernel_name() == OCCL


@pytest.mark.parametrize("name", ["cover.json", "occlusion_mix", "gloss_mix", "torus_mix", "mesh_mix", "teapot.json"])
def test_shadow_filter_kernels_without_a_filter_are_the_ordinary_render(rtc, name):
    hs = gb.mix(rtc) if name == "gloss_mix" else mb.mix(rtc) if name == "mesh_mix" else tb.mix(rtc) if name == "torus_mix" \
        else ob.mix(rtc) if name == "occlusion_mix" else rtc.HostScene.from_file(name)
    cam = hs.camera(W, H)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_spots(hs.spots())
    gpu.set_bumps(hs.bumps())
    gpu.set_mesh_uvs(hs.mesh_uvs())
    gpu.set_gloss(hs.gloss())
    gpu.set_occlusion(hs.occlusion())
    ordinary = gpu.render(cam, DEPTH)
    st0 = gpu.stats()
    old_name = gpu.last_kernel_name()
    assert "_sfilter" not in old_name
    rtc.set_option("shadow_filter_kernels", 1)
    try:
        forced = gpu.render(cam, DEPTH)
        st1 = gpu.stats()
        assert gpu.last_kernel_name() == SFILT
    finally:
        rtc.set_option("shadow_filter_kernels", 0)
    delta = float(np.abs(forced - ordinary).max())
    print(f"{name}: {old_name} against {SFILT}: max |delta| {delta:.3e}")
    assert delta <= FORCED_TOL
    for k in ("primary", "secondary", "shadow_calls", "overflow"):
        assert st0[k] == st1[k], k
    again = gpu.render(cam, DEPTH)
    assert float(np.abs(again - ordinary).max()) <= FORCED_TOL
    assert gpu.last_kernel_name() == old_name


# ---- rtc_scene_set_shadow_filters
def _status_name(rtc, code):
    return rtc.hip_lib().rtc_status_name(code).decode()


def test_selection_refusals_and_reset(rtc):
    hs = sb.mix(rtc)
    cam = hs.camera(W, H)
    f = hs.shadow_filters()
    n = hs.desc.n_materials
    gpu = handle(rtc, hs, filters=None)
    opaque = gpu.render(cam, DEPTH)
    old_name = gpu.last_kernel_name()
    assert old_name == OCCL         # (the fixture has a material with an occlusion radius)
    gpu.set_shadow_filters(f)
    first = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == SFILT and not np.array_equal(first, opaque)
    clone = gpu.clone()

    def poked(i, c, v):
        rgb = f["rgb"].copy()
        rgb[i, c] = v
        return {"rgb": rgb}

    bad = [{"rgb": f["rgb"][:-1]}, poked(2, 1, np.nan), poked(2, 0, np.inf), poked(0, 2, -1e-9), poked(n - 1, 2, 1.0 + 1e-9),
           {"rgb": None, "n_materials": n + 1}]
    for target in (gpu, clone):
        for b in bad:
            with pytest.raises(rtc.RtcError) as e:
                target.set_shadow_filters(b)
            assert e.value.name == _status_name(rtc, 1)                   # RTC_ERR_INVALID_ARGUMENT
            assert np.array_equal(target.render(cam, DEPTH), first)       # a refused table changes nothing
            assert target.last_kernel_name() == SFILT
    # NULL restores the previous kernel and its bits; the clone keeps its own table
    gpu.set_shadow_filters(None)
    assert np.array_equal(gpu.render(cam, DEPTH), opaque) and gpu.last_kernel_name() == old_name
    assert np.array_equal(clone.render(cam, DEPTH), first) and clone.last_kernel_name() == SFILT
    clone.set_shadow_filters(None)
    assert np.array_equal(clone.render(cam, DEPTH), opaque) and clone.last_kernel_name() == old_name
