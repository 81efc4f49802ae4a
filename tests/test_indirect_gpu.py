"""Indirect light on the GPU (rtc_scene_set_indirect, the indirect kernels): every render of the fixture
against the checker (tests/cpp/indirect_oracle.cpp) within 1e-12 with equal ray counts, no overflow and no pixel masked -
default sampling, a sample grid with a lens, a later pass, both kernel forms, band clones and a clone, a shuffled tile list,
Progressive, an adaptive run, rtch_scene_render -, the furnace and the open sky of tests/test_indirect_cpu.py, a world whose
hits form three children, what restores the previous kernels, the order of the setters, the indirect kernels forced on handles
without a table, emission alone, and the setter's refusals.  80 x 45 at depth 5 unless stated.

Figures: DESIGN.md section 27."""
import json

import numpy as np
import pytest

import camera_binding as cb
import environment_binding as eb
import gloss_binding as gb
import indirect_binding as ib
import media_binding as mdb
import skylight_binding as sb
import test_indirect_cpu as cpu
import test_table_limits_gpu as limits

pytestmark = pytest.mark.gpu

TOL = 1e-12         # (the suite's bound for a render against its checker: test_skylight_gpu.py's)
FORCED_TOL = 1e-14  # (the bound of the last features for their kernels forced on a handle against the handle's ordinary render)
SPLIT_TOL = 1e-14   # (shares of a split frame's pixels added in another order: tests/test_meshuv_gpu.py)
L_LIGHTS = limits.LIMITS["LDS"]["LIGHTS"]
INDIR, INDIR_BIG = "rtc_render_kernel_indir", "rtc_render_kernel_indir_bigworld"
SKYL, ENV = "rtc_render_kernel_skyl", "rtc_render_kernel_env"
W, H, DEPTH = 80, 45, 5


def compare(got, want, tol=TOL):
    """No mask: every pixel counts."""
    delta = float(np.abs(got - want).max())
    print(f"max |delta| {delta:.3e}")
    assert delta <= tol, f"max |delta| {delta}"


def handle(rtc, hs, smp=None, sample_pass=0, light_seed=0, indirect="scene", sky_light="scene", environment="scene"):
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    if smp is not None:
        gpu.set_sampling(smp)
    if light_seed:
        gpu.set_light_seed(light_seed)
    if sample_pass:
        gpu.set_sample_pass(sample_pass)
    gpu.set_spots(hs.spots())
    gpu.set_bumps(hs.bumps())
    gpu.set_mesh_uvs(hs.mesh_uvs())
    gpu.set_gloss(hs.gloss())
    gpu.set_occlusion(hs.occlusion())
    gpu.set_shadow_filters(hs.shadow_filters())
    gpu.set_media(hs.media())
    gpu.set_environment(hs.environment() if isinstance(environment, str) else environment)
    gpu.set_sky_light(hs.sky_light() if isinstance(sky_light, str) else sky_light)
    gpu.set_indirect(hs.indirect() if isinstance(indirect, str) else indirect)
    return gpu


def checker(rtc, hs, indirect="scene"):
    return ib.scene_of(rtc, hs, "file" if isinstance(indirect, str) else indirect)


def same_counts(st, counters):
    print({k: st[k] for k in ("primary", "secondary", "shadow_calls", "shadow_traced", "overflow")}, {k: counters[k] for k in ib.IND_COUNTERS})
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    assert st["overflow"] == 0


def check(rtc, hs, cam, smp=None, sample_pass=0, light_seed=0, kernel=INDIR, indirect="scene", depth=DEPTH):
    gpu = handle(rtc, hs, smp, sample_pass, light_seed, indirect)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    assert gpu.last_kernel_name() == kernel
    want, counters = checker(rtc, hs, indirect).render(cam, depth, smp, hs.spots(), None, sample_pass, light_seed=light_seed)
    compare(got, want)
    same_counts(st, counters)
    grid = smp.grid if smp is not None else 1
    assert st["primary"] == cam.hsize * cam.vsize * grid * grid
    return got, gpu, counters


@pytest.fixture(scope="module")
def fixture_reference(rtc):
    """The checker's render of the fixture at default sampling, computed once and left unchanged."""
    hs = ib.mix(rtc)
    want, counters = checker(rtc, hs).render(hs.camera(W, H), DEPTH, spots=hs.spots())
    want.setflags(write=False)
    return hs, want, counters


# ---- the fixture against the checker
def test_fixture_against_the_checker(rtc):
    hs = ib.mix(rtc)
    got, gpu, c = check(rtc, hs, hs.camera(W, H), light_seed=3)
    for k in ("ind_formed", "ind_no_remaining", "ind_no_bounces", "ind_suppressed", "ind_emitted"):
        assert c[k] > 0, k
    assert c["ind_max_pending"] > DEPTH + 2     # (the stack every other family gets would have overflowed)
    assert got.std() > 0.05


def test_fixture_with_a_sample_grid_and_a_lens(rtc):
    hs = ib.mix(rtc)
    check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, aperture=0.08, focal_distance=6.0, seed=5), light_seed=3)


def test_fixture_at_sample_pass_3(rtc, fixture_reference):
    hs = ib.mix(rtc)
    p3, _, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(1, True, seed=2), sample_pass=3, light_seed=3)
    assert not np.array_equal(p3, fixture_reference[1])


def _with_many_lights(n):
    """indirect_mix.json with point lights added until it has n: RTC_LDS_LIGHTS lights select the LDS kernel, one more the
    big-world one (tests/test_environment_gpu.py's way)"""
    scene = json.loads(open(ib.INDIRECT_MIX).read())
    k = 0
    while len(scene["lights"]) < n:
        a = 0.7 * k
        scene["lights"].append({"point-light": {"position": [2.5 * np.cos(a), 2.0 + 0.4 * (k % 3), 2.5 * np.sin(a)], "intensity": [0.01, 0.01, 0.012]}})
        k += 1
    return json.dumps(scene)


@pytest.mark.parametrize("extra", [0, 1])
def test_fixture_in_both_kernel_forms(rtc, extra):
    hs = rtc.HostScene(_with_many_lights(L_LIGHTS + extra))
    assert hs.lights.n_lights == L_LIGHTS + extra and hs.indirect()["bounces"] == 2
    check(rtc, hs, hs.camera(W, H), light_seed=3, kernel=INDIR_BIG if extra else INDIR)


# ---- band clones, a clone, a shuffled tile list
def test_a_clone_and_band_clones_follow(rtc, fixture_reference):
    hs, want, counters = fixture_reference
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs)
    rtc.set_option("host_bands", 3)
    try:
        banded = gpu.render(cam, DEPTH)
        st = gpu.stats()
    finally:
        rtc.set_option("host_bands", 0)
    compare(banded, want)
    same_counts(st, counters)   # (the bands' counts, summed)
    whole = gpu.render(cam, DEPTH)
    assert float(np.abs(whole - banded).max()) <= SPLIT_TOL
    clone = gpu.clone()
    assert float(np.abs(clone.render(cam, DEPTH) - whole).max()) <= SPLIT_TOL   # a clone starts with its source's table
    assert clone.last_kernel_name() == INDIR
    # the setter after the band clones exist: they follow
    other = dict(hs.indirect(), gain=1.3, bounces=1, seed=5)
    gpu.set_indirect(other)
    rtc.set_option("host_bands", 3)
    try:
        banded2 = gpu.render(cam, DEPTH)
    finally:
        rtc.set_option("host_bands", 0)
    want2, _ = checker(rtc, hs, other).render(cam, DEPTH, spots=hs.spots())
    compare(banded2, want2)
    assert not np.array_equal(banded2, banded)
    compare(clone.render(cam, DEPTH), want)      # ... and the clone keeps the table it started with


def test_a_shuffled_tile_list(rtc, fixture_reference):
    import torch
    hs, want, counters = fixture_reference
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
    assert gpu.last_kernel_name() == INDIR
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
    hs = ib.mix(rtc)
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
    assert gpu.last_kernel_name() == INDIR
    compare(mean, np.mean([im for im, _ in want], axis=0))
    assert not np.array_equal(want[0][0], want[1][0])           # the draws are new per pass


def test_adaptive_and_host_render_of_the_fixture(rtc, fixture_reference):
    scene = json.loads(open(ib.INDIRECT_MIX).read())
    scene["camera"].update(width=80, height=48, sampling={"grid": 1, "jitter": True, "seed": 4, "passes": 5, "occlusion-seed": 5,
                                                          "occlusion-samples": 2, "gloss-seed": 9,
                                                          "adaptive": {"threshold": 0.004, "min-passes": 2, "tile": [16, 16]}})
    hs = rtc.HostScene(json.dumps(scene))
    a = hs.adaptive()
    out = np.zeros((48, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, DEPTH, out.ctypes.data))
    gpu = handle(rtc, hs, hs.sampling())
    rgb, passes = gpu.render_adaptive(hs.camera(), a)
    assert gpu.last_kernel_name() == INDIR
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
    # without "adaptive": rtch_scene_render is one rtc_render of the handle, the file's tables applied - the indirect one among them
    plain, want1, _ = fixture_reference
    out1 = np.zeros((H, W, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(plain._h, W, H, DEPTH, out1.ctypes.data))
    compare(out1, want1)
    bare = checker(rtc, plain, None).render(plain.camera(W, H), DEPTH, spots=plain.spots())[0]
    assert float(np.abs(out1 - bare).max()) > 0.1


# ---- the furnace, the open sky and a world of three children
def _gpu_render(rtc, scene, depth):
    """The scene on the indirect kernels, held to the checker -> (image, secondary)"""
    hs = rtc.HostScene(scene)
    gpu = handle(rtc, hs)
    got = gpu.render(hs.camera(), depth)
    assert gpu.last_kernel_name() == INDIR
    st = gpu.stats()
    want, c = checker(rtc, hs).render(hs.camera(), depth, spots=hs.spots())
    compare(got, want)
    same_counts(st, c)
    return got, st["secondary"]


def test_furnace_on_the_gpu(rtc):
    """bounces 0, 1, 2 and 16 at depth 16 - the deepest chain - and 16 at depth 3, 4 x 4, against the geometric series."""
    cpu.check_furnace(lambda scene, depth: _gpu_render(rtc, scene, depth), 4)


def test_open_sky_on_the_gpu(rtc):
    cpu.check_open_sky(lambda scene, depth: _gpu_render(rtc, scene, depth))


def three_children_scene():
    """Nested panes that reflect, refract and scatter at once, in a matte room: every hit of a pane forms three children."""
    pane = {"pattern": cpu._solid([0.7, 0.8, 0.9]), "ambient": 0.05, "diffuse": 0.4, "specular": 0.2, "reflective": 0.3, "transparency": 0.6,
            "refractive-index": 1.3}
    objects = [{"type": {"sphere": {}}, "transform": [{"scale": [9, 9, 9]}],
                "material": {"pattern": cpu._solid([0.8, 0.6, 0.4]), "ambient": 0.1, "diffuse": 0.8, "specular": 0, "emission": [0.2, 0.2, 0.25]}}]
    for k, s in enumerate((2.4, 1.9, 1.4, 0.9)):
        objects.append({"type": {"cube": {}}, "transform": [{"scale": [s, s, s]}, {"rotate-y": 0.3 + 0.1 * k}],
                        "material": dict(pane, **{"refractive-index": 1.3 + 0.1 * k})})
    camera = {"width": 8, "height": 8, "field-of-view": 0.7, "from": [0.5, 1.0, -7.5], "to": [0, 0, 0], "up": [0, 1, 0]}
    return json.dumps({"camera": camera, "lights": [{"point-light": {"position": [3, 6, -6], "intensity": [0.6, 0.6, 0.6]}}],
                       "objects": objects, "indirect": {"gain": 0.8, "bounces": 6, "seed": 2}})


def test_a_world_of_three_children_fits_the_stack(rtc):
    hs = rtc.HostScene(three_children_scene())
    depth = 6
    gpu = handle(rtc, hs)
    got = gpu.render(hs.camera(), depth)
    st = gpu.stats()
    assert gpu.last_kernel_name() == INDIR
    want, c = checker(rtc, hs).render(hs.camera(), depth, spots=hs.spots())
    compare(got, want)
    same_counts(st, c)
    print("largest pending count", c["ind_max_pending"])
    assert c["ind_max_pending"] > depth + 2      # (max_depth + 2 levels would have overflowed)
    assert c["ind_max_pending"] <= 2 * depth     # (the bound the family's stack is sized by)


# ---- what restores the previous kernels; the order of the setters; the kernels forced
def test_null_a_gain_of_zero_and_no_bounces_restore_the_previous_kernel(rtc):
    hs = ib.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs, indirect=None)
    bare = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == SKYL
    table = dict(hs.indirect(), emission=None)
    gpu.set_indirect(table)
    assert not np.array_equal(gpu.render(cam, DEPTH), bare) and gpu.last_kernel_name() == INDIR
    for none in (dict(table, gain=0.0), dict(table, bounces=0), dict(table, gain=0.0, emission=np.zeros((hs.desc.n_materials, 3))), None):
        gpu.set_indirect(none)
        assert np.array_equal(gpu.render(cam, DEPTH), bare) and gpu.last_kernel_name() == SKYL
        gpu.set_indirect(table)
        assert gpu.render(cam, DEPTH) is not None and gpu.last_kernel_name() == INDIR
    # ... and on a handle without an environment the family below is what comes back
    plain = handle(rtc, hs, indirect=None, sky_light=None, environment=None)
    before = plain.render(cam, DEPTH)
    name = plain.last_kernel_name()
    assert "_indir" not in name and "_skyl" not in name and "_env" not in name
    plain.set_indirect(table)
    assert plain.render(cam, DEPTH) is not None and plain.last_kernel_name() == INDIR
    plain.set_indirect(None)
    assert np.array_equal(plain.render(cam, DEPTH), before) and plain.last_kernel_name() == name


def test_the_order_of_the_setters_does_not_matter(rtc, fixture_reference):
    hs, want, _ = fixture_reference
    cam = hs.camera(W, H)
    after = handle(rtc, hs).render(cam, DEPTH)                  # the environment, the sky light, then the indirect table
    gpu = handle(rtc, hs, sky_light=None, environment=None)     # the indirect table first
    gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == INDIR
    gpu.set_sky_light(hs.sky_light())
    gpu.set_environment(hs.environment())
    before = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == INDIR and np.array_equal(before, after)
    compare(before, want)


@pytest.mark.parametrize("name", ["cover.json", "sky_mix", "skylight_mix", "media_mix", "gloss_mix", "teapot.json"])
def test_indirect_kernels_without_a_table_are_the_ordinary_render(rtc, name):
    hs = eb.mix(rtc) if name == "sky_mix" else sb.mix(rtc) if name == "skylight_mix" else gb.mix(rtc) if name == "gloss_mix" \
        else mdb.mix(rtc) if name == "media_mix" else rtc.HostScene.from_file(name)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs)
    ordinary = gpu.render(cam, DEPTH)
    st0 = gpu.stats()
    old_name = gpu.last_kernel_name()
    assert "_indir" not in old_name
    rtc.set_option("indirect_kernels", 1)
    try:
        forced = gpu.render(cam, DEPTH)
        st1 = gpu.stats()
        assert gpu.last_kernel_name() == INDIR
    finally:
        rtc.set_option("indirect_kernels", 0)
    delta = float(np.abs(forced - ordinary).max())
    print(f"{name}: {old_name} against {INDIR}: max |delta| {delta:.3e}")
    assert delta <= FORCED_TOL
    for k in ("primary", "secondary", "shadow_calls", "overflow"):
        assert st0[k] == st1[k], k
    again = gpu.render(cam, DEPTH)
    assert float(np.abs(again - ordinary).max()) <= FORCED_TOL
    assert gpu.last_kernel_name() == old_name


def test_emission_alone_selects_the_family_and_adds_itself(rtc):
    """A flat-lit case: a matte sphere with ambient alone under one light, depth 0.  Every primary hit gets exactly its
    material's emission more; a miss nothing."""
    scene = {"camera": {"width": 16, "height": 16, "field-of-view": 0.9, "from": [0, 0, -4], "to": [0, 0, 0], "up": [0, 1, 0]},
             "lights": [{"point-light": {"position": [0, 5, -5], "intensity": [1, 1, 1]}}],
             "objects": [{"type": {"sphere": {}}, "material": {"pattern": cpu._solid([0.5, 0.25, 0.75]), "ambient": 0.5, "diffuse": 0, "specular": 0}}]}
    hs = rtc.HostScene(json.dumps(scene))
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    flat = gpu.render(hs.camera(), 0)
    old_name = gpu.last_kernel_name()
    emission = np.zeros((hs.desc.n_materials, 3))
    emission[:] = (0.125, 0.25, 2.0)
    gpu.set_indirect({"gain": 0.0, "bounces": 0, "emission": emission})
    lit = gpu.render(hs.camera(), 0)
    assert gpu.last_kernel_name() == INDIR and "_indir" not in old_name
    hit = flat.any(axis=2)
    assert hit.any() and not hit.all()
    assert np.array_equal(lit[hit], flat[hit] + np.array([0.125, 0.25, 2.0])) and not lit[~hit].any()
    gpu.set_indirect(None)
    assert np.array_equal(gpu.render(hs.camera(), 0), flat) and gpu.last_kernel_name() == old_name


# ---- rtc_scene_set_indirect
def _status_name(rtc, code):
    return rtc.hip_lib().rtc_status_name(code).decode()


def test_refusals_change_nothing(rtc):
    hs = ib.mix(rtc)
    cam = hs.camera(W, H)
    table = hs.indirect()
    n = hs.desc.n_materials
    gpu = handle(rtc, hs)
    first = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == INDIR
    clone = gpu.clone()
    negative, nan = table["emission"].copy(), table["emission"].copy()
    negative[1, 1], nan[n - 1, 2] = -1e-9, np.nan
    bad = [dict(table, gain=np.nan), dict(table, gain=np.inf), dict(table, gain=-1e-9), dict(table, bounces=17), dict(table, gain=0.0, bounces=17),
           dict(table, emission=negative), dict(table, emission=nan), dict(table, emission=np.zeros((n + 1, 3))), dict(table, emission=np.zeros((n - 1, 3)))]
    for target in (gpu, clone):
        for b in bad:
            with pytest.raises(rtc.RtcError) as err:
                target.set_indirect(b)
            assert err.value.name == _status_name(rtc, 1)                 # RTC_ERR_INVALID_ARGUMENT
        got = target.render(cam, DEPTH)                                   # the refused tables changed nothing
        assert float(np.abs(got - first).max()) <= SPLIT_TOL and target.last_kernel_name() == INDIR
    # NULL on the handle; the clone keeps its own table
    gpu.set_indirect(None)
    assert gpu.render(cam, DEPTH) is not None and gpu.last_kernel_name() == SKYL
    assert float(np.abs(clone.render(cam, DEPTH) - first).max()) <= SPLIT_TOL and clone.last_kernel_name() == INDIR
