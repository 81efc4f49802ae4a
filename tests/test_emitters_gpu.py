"""Emitter sampling on the GPU (rtc_scene_set_emitters, the emitter kernels): every render of the fixture
against the checker (tests/cpp/emitters_oracle.cpp) within 1e-12 * max(1, |value|) with equal ray counts and no overflow -
default sampling, a sample grid with a lens, a later pass, both kernel forms, band clones and a clone, a shuffled tile list,
Progressive, an adaptive run, rtch_scene_render -, the cube furnace and the small worlds of tests/test_emitters_cpu.py, the
emitter kernels forced on handles without a list, what restores the previous kernels, the order of the setters and the
refusals that need a handle.  80 x 45 at depth 5 unless stated.

Figures: DESIGN.md section 28."""
import json

import numpy as np
import pytest

import camera_binding as cb
import emitters_binding as mb
import indirect_binding as ib
import media_binding as mdb
import skylight_binding as sb
import test_emitters_cpu as cpu
import test_table_limits_gpu as limits

pytestmark = pytest.mark.gpu

TOL = 1e-12         # (per channel, times max(1, |value|))
FORCED_TOL = 1e-14  # (the family forced on a handle against the handle's ordinary render)
SPLIT_TOL = 1e-14   # (shares of a split frame's pixels added in another order: tests/test_meshuv_gpu.py)
L_LIGHTS = limits.LIMITS["LDS"]["LIGHTS"]
EMIT, EMIT_BIG = "rtc_render_kernel_emit", "rtc_render_kernel_emit_bigworld"
INDIR = "rtc_render_kernel_indir"
W, H, DEPTH = 80, 45, 5


def compare(got, want, tol=TOL):
    """No mask: every pixel and channel counts, each within tol * max(1, |value|)."""
    delta = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"max |delta| / max(1, |value|) {float(delta.max()):.3e}")
    assert float(delta.max()) <= tol, f"max scaled |delta| {float(delta.max())}"


def handle(rtc, hs, smp=None, sample_pass=0, light_seed=0, emitters="scene", indirect="scene", emitters_first=False):
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    if smp is not None:
        gpu.set_sampling(smp)
    if light_seed:
        gpu.set_light_seed(light_seed)
    if sample_pass:
        gpu.set_sample_pass(sample_pass)
    em = hs.emitters() if isinstance(emitters, str) else emitters
    if emitters_first:
        gpu.set_emitters(em)
    gpu.set_spots(hs.spots())
    gpu.set_bumps(hs.bumps())
    gpu.set_mesh_uvs(hs.mesh_uvs())
    gpu.set_gloss(hs.gloss())
    gpu.set_occlusion(hs.occlusion())
    gpu.set_shadow_filters(hs.shadow_filters())
    gpu.set_media(hs.media())
    gpu.set_environment(hs.environment())
    gpu.set_sky_light(hs.sky_light())
    gpu.set_indirect(hs.indirect() if isinstance(indirect, str) else indirect)
    if not emitters_first:
        gpu.set_emitters(em)
    return gpu


def checker(rtc, hs, emitters="scene"):
    return mb.scene_of(rtc, hs, "file" if isinstance(emitters, str) else emitters)


def same_counts(st, counters):
    print({k: st[k] for k in ("primary", "secondary", "shadow_calls", "shadow_traced", "overflow")}, {k: counters[k] for k in mb.EMIT_COUNTERS})
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    assert st["overflow"] == 0


def check(rtc, hs, cam, smp=None, sample_pass=0, light_seed=0, kernel=EMIT, emitters="scene", depth=DEPTH):
    gpu = handle(rtc, hs, smp, sample_pass, light_seed, emitters)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    assert gpu.last_kernel_name() == kernel
    want, counters = checker(rtc, hs, emitters).render(cam, depth, smp, hs.spots(), None, sample_pass, light_seed=light_seed)
    compare(got, want)
    same_counts(st, counters)
    grid = smp.grid if smp is not None else 1
    assert st["primary"] == cam.hsize * cam.vsize * grid * grid
    return got, gpu, counters


@pytest.fixture(scope="module")
def fixture_reference(rtc):
    """The checker's render of the fixture at default sampling, computed once and left unchanged."""
    hs = mb.mix(rtc)
    want, counters = checker(rtc, hs).render(hs.camera(W, H), DEPTH, spots=hs.spots())
    want.setflags(write=False)
    return hs, want, counters


# ---- the fixture against the checker
def test_fixture_against_the_checker(rtc):
    hs = mb.mix(rtc)
    got, gpu, c = check(rtc, hs, hs.camera(W, H), light_seed=3)
    for k in ("emit_drawn", "emit_skip_cos_x", "emit_walks", "emit_blocked", "emit_suppressed", "ind_formed", "t_partial"):
        assert c[k] > 0, k
    assert got.std() > 0.05


def test_fixture_with_a_sample_grid_and_a_lens(rtc):
    hs = mb.mix(rtc)
    check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, aperture=0.08, focal_distance=6.0, seed=5), light_seed=3)


def test_fixture_at_sample_pass_3(rtc, fixture_reference):
    hs = mb.mix(rtc)
    p3, _, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(1, True, seed=2), sample_pass=3, light_seed=3)
    assert not np.array_equal(p3, fixture_reference[1])


def _with_many_lights(n):
    """emitters_mix.json with point lights added until it has n: RTC_LDS_LIGHTS lights select the LDS kernel, one more the
    big-world one (tests/test_indirect_gpu.py's way)"""
    scene = json.loads(open(mb.EMITTERS_MIX).read())
    k = 0
    while len(scene["lights"]) < n:
        a = 0.7 * k
        scene["lights"].append({"point-light": {"position": [2.5 * np.cos(a), 2.0 + 0.4 * (k % 3), 2.5 * np.sin(a)], "intensity": [0.01, 0.01, 0.012]}})
        k += 1
    return json.dumps(scene)


@pytest.mark.parametrize("extra", [0, 1])
def test_fixture_in_both_kernel_forms(rtc, extra):
    hs = rtc.HostScene(_with_many_lights(L_LIGHTS + extra))
    assert hs.lights.n_lights == L_LIGHTS + extra and hs.emitters()["samples"] == 2
    check(rtc, hs, hs.camera(W, H), light_seed=3, kernel=EMIT_BIG if extra else EMIT)


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
    assert clone.last_kernel_name() == EMIT
    # the setter after the band clones exist: they follow
    other = {"samples": 3, "seed": 5}
    gpu.set_emitters(other)
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
    assert gpu.last_kernel_name() == EMIT
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
    hs = mb.mix(rtc)
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
    assert gpu.last_kernel_name() == EMIT
    compare(mean, np.mean([im for im, _ in want], axis=0))
    assert not np.array_equal(want[0][0], want[1][0])           # the draws are new per pass


def test_adaptive_and_host_render_of_the_fixture(rtc, fixture_reference):
    scene = json.loads(open(mb.EMITTERS_MIX).read())
    scene["camera"].update(width=80, height=48, sampling={"grid": 1, "jitter": True, "seed": 4, "passes": 5, "gloss-seed": 9,
                                                          "adaptive": {"threshold": 0.004, "min-passes": 2, "tile": [16, 16]}})
    hs = rtc.HostScene(json.dumps(scene))
    a = hs.adaptive()
    out = np.zeros((48, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, DEPTH, out.ctypes.data))
    gpu = handle(rtc, hs, hs.sampling())
    rgb, passes = gpu.render_adaptive(hs.camera(), a)
    assert gpu.last_kernel_name() == EMIT
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
    # without "adaptive": rtch_scene_render is one rtc_render of the handle, the file's tables applied - the emitter one among them
    plain, want1, _ = fixture_reference
    out1 = np.zeros((H, W, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(plain._h, W, H, DEPTH, out1.ctypes.data))
    compare(out1, want1)
    bare = checker(rtc, plain, None).render(plain.camera(W, H), DEPTH, spots=plain.spots())[0]
    assert not np.array_equal(out1, bare)


# ---- small worlds
def _gpu_render(rtc, scene, depth, emitters, kernel=EMIT):
    """The scene on the GPU, held to the checker -> (image, counters)"""
    hs = rtc.HostScene(scene)
    gpu = handle(rtc, hs, emitters=emitters)
    got = gpu.render(hs.camera(), depth)
    assert gpu.last_kernel_name() == kernel
    st = gpu.stats()
    want, c = checker(rtc, hs, emitters).render(hs.camera(), depth, spots=hs.spots())
    compare(got, want)
    same_counts(st, c)
    return got, c


def test_cube_furnace_at_the_deepest_chain(rtc):
    """the camera inside the emissive cube, 4 x 4, bounces = max_depth = 6: every hit samples the six faces, every child is
    suppressed"""
    scene = json.loads(cpu.cube_furnace_scene(6))
    _, c = _gpu_render(rtc, json.dumps(scene), 6, {"samples": 2, "seed": 13})
    assert c["ind_formed"] == 6 * 16 and c["emit_suppressed"] == 6 * 16 and c["emit_drawn"] == 2 * 6 * 16
    # ... and without the table the series of section 27, on the indirect kernels
    off, _ = _gpu_render(rtc, json.dumps(scene), 6, None, kernel=INDIR)
    assert np.abs(off - cpu.furnace_value(6, 6)).max() <= 1e-12


@pytest.mark.parametrize("world", ["one", "two", "mesh", "sheared"])
def test_small_worlds_against_the_checker(rtc, world):
    scene = {"one": cpu.one_entry_world, "two": cpu.two_entry_world, "mesh": lambda: cpu.mesh_world(rtc.MAX_EMITTERS),
             "sheared": cpu.sheared_cube_world}[world]()
    _, c = _gpu_render(rtc, scene, DEPTH, {"samples": 16 if world == "two" else 3, "seed": 4})
    assert c["emit_walks"] > 0 and c["emit_drawn"] == (16 if world == "two" else 3) * c["ind_formed"]


def test_one_entry_too_many_is_refused_and_leaves_the_previous_table(rtc):
    hs = rtc.HostScene(cpu.mesh_world(rtc.MAX_EMITTERS + 1))
    gpu = handle(rtc, hs, emitters=None)
    before = gpu.render(hs.camera(), DEPTH)
    assert gpu.last_kernel_name() == INDIR
    with pytest.raises(rtc.RtcError) as err:
        gpu.set_emitters({"samples": 1})
    assert err.value.name == "Unsupported"
    assert np.array_equal(gpu.render(hs.camera(), DEPTH), before) and gpu.last_kernel_name() == INDIR
    # ... and the other way round: the table first, then the emission rows that would make the list too long
    gpu.set_indirect(None)
    gpu.set_emitters({"samples": 1})
    with pytest.raises(rtc.RtcError) as err:
        gpu.set_indirect(hs.indirect())
    assert err.value.name == "Unsupported"
    gpu.render(hs.camera(), DEPTH)
    assert "_emit" not in gpu.last_kernel_name() and "_indir" not in gpu.last_kernel_name()


# ---- the family with the feature off
@pytest.mark.parametrize("name", ["cover.json", "indirect_mix", "skylight_mix", "media_mix", "teapot.json"])
def test_emitter_kernels_without_a_list_are_the_ordinary_render(rtc, name):
    hs = ib.mix(rtc) if name == "indirect_mix" else sb.mix(rtc) if name == "skylight_mix" else mdb.mix(rtc) if name == "media_mix" \
        else rtc.HostScene.from_file(name)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs, emitters=None)
    ordinary = gpu.render(cam, DEPTH)
    st0 = gpu.stats()
    old_name = gpu.last_kernel_name()
    assert "_emit" not in old_name
    rtc.set_option("emitter_kernels", 1)
    try:
        forced = gpu.render(cam, DEPTH)
        st1 = gpu.stats()
        assert gpu.last_kernel_name() == EMIT
    finally:
        rtc.set_option("emitter_kernels", 0)
    delta = float(np.abs(forced - ordinary).max())
    print(f"{name}: {old_name} against {EMIT}: max |delta| {delta:.3e}")
    assert delta <= FORCED_TOL
    for k in ("primary", "secondary", "shadow_calls", "overflow"):
        assert st0[k] == st1[k], k
    again = gpu.render(cam, DEPTH)
    assert float(np.abs(again - ordinary).max()) <= FORCED_TOL
    assert gpu.last_kernel_name() == old_name


# ---- turning it off restores the old kernel; refusals; the order of the setters
def test_null_restores_the_previous_kernel_and_a_refusal_changes_nothing(rtc):
    hs = mb.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs, emitters=None)
    bare = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == INDIR
    gpu.set_emitters(hs.emitters())
    first = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == EMIT and not np.array_equal(first, bare)
    for samples in (0, 17):
        with pytest.raises(rtc.RtcError) as err:
            gpu.set_emitters({"samples": samples})
        assert err.value.name == "InvalidArgument"
        assert np.array_equal(gpu.render(cam, DEPTH), first) and gpu.last_kernel_name() == EMIT
    gpu.set_emitters(None)
    assert np.array_equal(gpu.render(cam, DEPTH), bare) and gpu.last_kernel_name() == INDIR
    # a table whose list is empty - no material emits - keeps the previous kernel too
    gpu.set_emitters(hs.emitters())
    gpu.set_indirect(dict(hs.indirect(), emission=None))
    gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == INDIR


def test_the_order_of_the_setters_does_not_matter(rtc, fixture_reference):
    hs, want, _ = fixture_reference
    cam = hs.camera(W, H)
    after = handle(rtc, hs).render(cam, DEPTH)                          # the filters, the indirect table, then the emitter table
    gpu = handle(rtc, hs, emitters_first=True)                          # the emitter table first
    before = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == EMIT and np.array_equal(before, after)
    compare(before, want)
    # the filters last: the pane's material is filtered, the list does not change; without the filter table a filtered
    # emitter would be listed - here the panel is not filtered, so only the image changes
    gpu.set_shadow_filters(None)
    unfiltered = gpu.render(cam, DEPTH)
    gpu.set_shadow_filters(hs.shadow_filters())
    assert not np.array_equal(unfiltered, after) and np.array_equal(gpu.render(cam, DEPTH), after)


def test_a_moving_emitter_is_refused_in_both_call_orders(rtc):
    hs = mb.mix(rtc)
    cam = hs.camera(W, H)
    n = hs.desc.n_roots
    scene = json.loads(open(mb.EMITTERS_MIX).read())
    panel = next(i for i, o in enumerate(scene["objects"]) if "cube" in o["type"] and "emission" in o["material"])
    ball = next(i for i, o in enumerate(scene["objects"]) if o["material"].get("reflective") == 0.9)
    moving_panel, moving_ball = np.zeros((n, 3)), np.zeros((n, 3))
    moving_panel[panel], moving_ball[ball] = (0.2, 0.0, 0.0), (0.2, 0.0, 0.0)
    # the table, then the motion
    gpu = handle(rtc, hs)
    first = gpu.render(cam, DEPTH)
    with pytest.raises(rtc.RtcError) as err:
        gpu.set_motion(moving_panel)
    assert err.value.name == "Unsupported"
    assert np.array_equal(gpu.render(cam, DEPTH), first) and gpu.last_kernel_name() == EMIT
    gpu.set_motion(moving_ball)                                         # (a root that holds no listed leaf may move)
    moved = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == EMIT and not np.array_equal(moved, first)
    # the motion, then the table
    gpu = handle(rtc, hs, emitters=None)
    gpu.set_motion(moving_panel)
    before = gpu.render(cam, DEPTH)
    with pytest.raises(rtc.RtcError) as err:
        gpu.set_emitters(hs.emitters())
    assert err.value.name == "Unsupported"
    assert np.array_equal(gpu.render(cam, DEPTH), before) and gpu.last_kernel_name() == INDIR
