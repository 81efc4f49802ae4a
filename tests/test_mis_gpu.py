"""Multiple importance sampling on the GPU (rtc_scene_set_emitter_mis, the MIS kernels): every render of
the fixture against the checker (tests/cpp/mis_oracle.cpp) within 1e-12 * max(1, |value|) with equal ray counts and no overflow
- default sampling, a sample grid with a lens, a later pass, both kernel forms, band clones and a clone, a shuffled tile list,
Progressive, an adaptive run, rtch_scene_render -, the cube furnace at the deepest stack, the bound fixture, a 1-entry world, a
medium, the MIS kernels forced with mode 0 on handles that do not need them, what restores the emitter kernels, a refusal, and
the order of the setters.  80 x 45 at depth 5 unless stated.

Figures: DESIGN.md section 32."""
import json

import numpy as np
import pytest

import camera_binding as cb
import emitters_binding as eb
import indirect_binding as ib
import media_binding as mdb
import mis_binding as mb
import test_emitters_cpu as ecpu
import test_mis_cpu as cpu
import test_table_limits_gpu as limits

pytestmark = pytest.mark.gpu

TOL = 1e-12         # (per channel, times max(1, |value|))
FORCED_TOL = 1e-14  # (the family forced on a handle against the handle's ordinary render)
SPLIT_TOL = 1e-14   # (shares of a split frame's pixels added in another order: tests/test_meshuv_gpu.py)
L_LIGHTS = limits.LIMITS["LDS"]["LIGHTS"]
MIS, MIS_BIG = "rtc_render_kernel_mis", "rtc_render_kernel_mis_bigworld"
EMIT = "rtc_render_kernel_emit"
W, H, DEPTH = 80, 45, 5


def compare(got, want, tol=TOL):
    """No mask: every pixel and channel counts, each within tol * max(1, |value|)."""
    delta = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print(f"max |delta| / max(1, |value|) {float(delta.max()):.3e}")
    assert float(delta.max()) <= tol, f"max scaled |delta| {float(delta.max())}"


def handle(rtc, hs, smp=None, sample_pass=0, light_seed=0, emitters="scene", mode="scene", mis_first=False):
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    mode = hs.emitter_mis() if isinstance(mode, str) else mode
    if mis_first:
        gpu.set_emitter_mis(mode)
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
    gpu.set_environment(hs.environment())
    gpu.set_sky_light(hs.sky_light())
    gpu.set_indirect(hs.indirect())
    gpu.set_emitters(hs.emitters() if isinstance(emitters, str) else emitters)
    if not mis_first:
        gpu.set_emitter_mis(mode)
    return gpu


def checker(rtc, hs, emitters="scene"):
    return mb.scene_of(rtc, hs, "file" if isinstance(emitters, str) else emitters)


def same_counts(st, counters):
    print({k: st[k] for k in ("primary", "secondary", "shadow_calls", "shadow_traced", "overflow")},
          {k: counters[k] for k in mb.EMIT_COUNTERS + mb.MIS_COUNTERS})
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    assert st["overflow"] == 0


def check(rtc, hs, cam, smp=None, sample_pass=0, light_seed=0, kernel=MIS, emitters="scene", depth=DEPTH):
    gpu = handle(rtc, hs, smp, sample_pass, light_seed, emitters)
    got = gpu.render(cam, depth)
    st = gpu.stats()
    assert gpu.last_kernel_name() == kernel
    want, counters = checker(rtc, hs, emitters).render(cam, depth, smp, hs.spots(), None, sample_pass, light_seed=light_seed, mode=1)
    compare(got, want)
    same_counts(st, counters)
    grid = smp.grid if smp is not None else 1
    assert st["primary"] == cam.hsize * cam.vsize * grid * grid
    return got, gpu, counters


@pytest.fixture(scope="module")
def fixture_reference(rtc):
    """The checker's render of the fixture at default sampling, computed once and left unchanged."""
    hs = mb.mix(rtc)
    want, counters = checker(rtc, hs).render(hs.camera(W, H), DEPTH, spots=hs.spots(), mode=1)
    want.setflags(write=False)
    return hs, want, counters


# ---- the fixture against the checker
def test_fixture_against_the_checker(rtc):
    hs = mb.mix(rtc)
    got, gpu, c = check(rtc, hs, hs.camera(W, H), light_seed=3)
    for k in ("emit_drawn", "emit_skip_cos_x", "emit_walks", "emit_blocked", "mis_weighted", "ind_formed", "t_partial"):
        assert c[k] > 0, k
    assert c["emit_suppressed"] == 0 and c["ind_max_pending"] >= 5      # (a diffuse child waits under two siblings, and deeper)
    plain = checker(rtc, hs).render(hs.camera(W, H), DEPTH, spots=hs.spots(), light_seed=3, mode=0)[0]
    assert not np.array_equal(got, plain)


def test_fixture_with_a_sample_grid_and_a_lens(rtc):
    hs = mb.mix(rtc)
    check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, aperture=0.08, focal_distance=6.0, seed=5), light_seed=3)


def test_fixture_at_sample_pass_3(rtc, fixture_reference):
    hs = mb.mix(rtc)
    p3, _, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(1, True, seed=2), sample_pass=3, light_seed=3)
    assert not np.array_equal(p3, fixture_reference[1])


def _with_many_lights(n):
    """mis_mix.json with point lights added until it has n: RTC_LDS_LIGHTS lights select the LDS kernel, one more the
    big-world one (tests/test_indirect_gpu.py's way)"""
    scene = json.loads(open(mb.MIS_MIX).read())
    k = 0
    while len(scene["lights"]) < n:
        a = 0.7 * k
        scene["lights"].append({"point-light": {"position": [2.5 * np.cos(a), 2.0 + 0.4 * (k % 3), 2.5 * np.sin(a)], "intensity": [0.01, 0.01, 0.012]}})
        k += 1
    return json.dumps(scene)


@pytest.mark.parametrize("extra", [0, 1])
def test_fixture_in_both_kernel_forms(rtc, extra):
    hs = rtc.HostScene(_with_many_lights(L_LIGHTS + extra))
    assert hs.lights.n_lights == L_LIGHTS + extra and hs.emitter_mis() == 1
    check(rtc, hs, hs.camera(W, H), light_seed=3, kernel=MIS_BIG if extra else MIS)


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
    assert float(np.abs(clone.render(cam, DEPTH) - whole).max()) <= SPLIT_TOL   # a clone starts with its source's mode
    assert clone.last_kernel_name() == MIS
    # the setter after the band clones exist: they follow
    gpu.set_emitter_mis(0)
    rtc.set_option("host_bands", 3)
    try:
        banded0 = gpu.render(cam, DEPTH)
    finally:
        rtc.set_option("host_bands", 0)
    want0, _ = checker(rtc, hs).render(cam, DEPTH, spots=hs.spots(), mode=0)
    compare(banded0, want0)
    assert not np.array_equal(banded0, banded) and gpu.last_kernel_name() == EMIT
    compare(clone.render(cam, DEPTH), want)      # ... and the clone keeps the mode it started with


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
    assert gpu.last_kernel_name() == MIS
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
    want = [ck.render(cam, DEPTH, smp, hs.spots(), sample_pass=p, mode=1) for p in range(4)]
    prog = rtc.Progressive(gpu, cam, DEPTH)
    for p in range(4):
        prog.step()
        same_counts(gpu.stats(), want[p][1])                    # (the handle's counts are its last launch's: pass p)
    mean = prog.mean().cpu().numpy()
    torch.cuda.synchronize()
    assert gpu.last_kernel_name() == MIS
    compare(mean, np.mean([im for im, _ in want], axis=0))
    assert not np.array_equal(want[0][0], want[1][0])           # the draws are new per pass


def test_adaptive_and_host_render_of_the_fixture(rtc, fixture_reference):
    scene = json.loads(open(mb.MIS_MIX).read())
    scene["camera"].update(width=80, height=48, sampling={"grid": 1, "jitter": True, "seed": 4, "passes": 5, "gloss-seed": 9,
                                                          "adaptive": {"threshold": 0.004, "min-passes": 2, "tile": [16, 16]}})
    hs = rtc.HostScene(json.dumps(scene))
    a = hs.adaptive()
    out = np.zeros((48, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, DEPTH, out.ctypes.data))
    gpu = handle(rtc, hs, hs.sampling())
    rgb, passes = gpu.render_adaptive(hs.camera(), a)
    assert gpu.last_kernel_name() == MIS
    assert np.array_equal(out, rgb)
    assert passes.min() >= 2 and passes.max() <= 5
    ck = checker(rtc, hs)
    images = [ck.render(hs.camera(), DEPTH, hs.sampling(), hs.spots(), sample_pass=p, mode=1)[0] for p in range(5)]
    want = np.zeros_like(rgb)
    tiles_x = 80 // 16
    for t, k in enumerate(passes):
        ty, tx = divmod(t, tiles_x)
        want[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = np.mean([im[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] for im in images[:k]], axis=0)
    compare(rgb, want)
    # without "adaptive": rtch_scene_render is one rtc_render of the handle, the file's tables and its mode applied
    plain, want1, _ = fixture_reference
    out1 = np.zeros((H, W, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(plain._h, W, H, DEPTH, out1.ctypes.data))
    compare(out1, want1)
    switch = checker(rtc, plain).render(plain.camera(W, H), DEPTH, spots=plain.spots(), mode=0)[0]
    assert not np.array_equal(out1, switch)


# ---- small worlds
def _gpu_render(rtc, scene, depth, emitters, kernel=MIS, media="scene"):
    """The scene on the GPU with mode 1, held to the checker -> (image, counters)"""
    hs = rtc.HostScene(scene)
    gpu = handle(rtc, hs, emitters=emitters, mode=1)
    got = gpu.render(hs.camera(), depth)
    assert gpu.last_kernel_name() == kernel
    st = gpu.stats()
    want, c = checker(rtc, hs, emitters).render(hs.camera(), depth, spots=hs.spots(), mode=1)
    compare(got, want)
    same_counts(st, c)
    return got, c


def test_cube_furnace_at_the_deepest_stack(rtc):
    """the camera inside the emissive cube, 4 x 4, bounces = max_depth = 6: every hit samples the six faces, every child meets a
    face and is weighted - the deepest chain of carried values; with a mirror coat the child waits under a sibling at every level"""
    scene = json.loads(ecpu.cube_furnace_scene(6))
    _, c = _gpu_render(rtc, json.dumps(scene), 6, {"samples": 2, "seed": 13})
    assert c["ind_formed"] == 6 * 16 and c["mis_weighted"] + c["mis_whole"] == 6 * 16 and c["emit_suppressed"] == 0
    scene["objects"][0]["material"].update(reflective=0.3, transparency=0.2)
    scene["objects"][0]["material"]["refractive-index"] = 1.3
    _, c = _gpu_render(rtc, json.dumps(scene), 6, {"samples": 2, "seed": 13})
    assert c["ind_max_pending"] > 6 + 2 and c["mis_weighted"] > 6 * 16          # (deeper than any other family's stack)


def test_the_bound_fixture(rtc):
    hs = rtc.HostScene.from_file(mb.MIS_BOUND)
    got, _, c = check(rtc, hs, hs.camera(16, 16), depth=DEPTH)
    assert c["mis_weighted"] > 0
    assert got.max() <= cpu.BOUND


def test_a_one_entry_world(rtc):
    _, c = _gpu_render(rtc, ecpu.one_entry_world(), DEPTH, {"samples": 3, "seed": 4})
    assert c["emit_walks"] > 0 and c["emit_drawn"] == 3 * c["ind_formed"]


def test_a_medium_with_mis(rtc):
    """media_mix.json's atmosphere and absorbing glass around the bound fixture's panel: the transmittance multiplies the
    weighted term, the child's weight is the geometry's alone"""
    media = json.loads(open(mdb.MEDIA_MIX).read())
    scene = json.loads(open(mb.MIS_BOUND).read())
    scene["atmosphere"] = media["atmosphere"]
    glass = next(o for o in media["objects"] if "absorption" in o.get("material", {}))
    pane = {"type": {"cube": {}}, "transform": [{"scale": [0.3, 0.004, 0.3]}, {"translate": [0.1, 0.02, 0.05]}],
            "material": dict(glass["material"], diffuse=0.2)}
    scene["objects"].append(pane)
    scene["camera"].update({"from": [0.3, 0.4, -0.9], "to": [0.1, 0.0, 0.05], "up": [0, 1, 0], "field-of-view": 0.9})
    _, c = _gpu_render(rtc, json.dumps(scene), DEPTH, {"samples": 2, "seed": 5})
    assert c["mis_weighted"] > 0 and c["emit_walks"] > 0


# ---- the family with mode 0
@pytest.mark.parametrize("name", ["cover.json", "indirect_mix", "emitters_mix"])
def test_mis_kernels_with_mode_0_are_the_ordinary_render(rtc, name):
    hs = ib.mix(rtc) if name == "indirect_mix" else eb.mix(rtc) if name == "emitters_mix" else rtc.HostScene.from_file(name)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs, mode=0)
    ordinary = gpu.render(cam, DEPTH)
    st0 = gpu.stats()
    old_name = gpu.last_kernel_name()
    assert "_mis" not in old_name
    rtc.set_option("mis_kernels", 1)
    try:
        forced = gpu.render(cam, DEPTH)
        st1 = gpu.stats()
        assert gpu.last_kernel_name() == MIS
    finally:
        rtc.set_option("mis_kernels", 0)
    delta = float(np.abs(forced - ordinary).max())
    print(f"{name}: {old_name} against {MIS}: max |delta| {delta:.3e}")
    assert delta <= FORCED_TOL
    for k in ("primary", "secondary", "shadow_calls", "overflow"):
        assert st0[k] == st1[k], k
    again = gpu.render(cam, DEPTH)
    assert float(np.abs(again - ordinary).max()) <= FORCED_TOL
    assert gpu.last_kernel_name() == old_name


# ---- turning it off restores the emitter kernels; a refusal; the order of the setters
def test_mode_0_restores_the_emitter_kernels_and_a_refusal_changes_nothing(rtc):
    hs = mb.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs, mode=0)
    switch = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == EMIT
    gpu.set_emitter_mis(1)
    first = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == MIS and not np.array_equal(first, switch)
    for mode in (2, 0xFFFFFFFF):
        with pytest.raises(rtc.RtcError) as err:
            gpu.set_emitter_mis(mode)
        assert err.value.name == "InvalidArgument"
        assert np.array_equal(gpu.render(cam, DEPTH), first) and gpu.last_kernel_name() == MIS
    gpu.set_emitter_mis(0)
    assert np.array_equal(gpu.render(cam, DEPTH), switch) and gpu.last_kernel_name() == EMIT
    # the mode has no effect without a list: no table, and a table whose list is empty
    gpu.set_emitter_mis(1)
    gpu.set_emitters(None)
    gpu.render(cam, DEPTH)
    assert "_mis" not in gpu.last_kernel_name() and "_emit" not in gpu.last_kernel_name()
    gpu.set_emitters(hs.emitters())
    assert np.array_equal(gpu.render(cam, DEPTH), first) and gpu.last_kernel_name() == MIS


def test_the_order_of_the_setters_does_not_matter(rtc, fixture_reference):
    hs, want, _ = fixture_reference
    cam = hs.camera(W, H)
    after = handle(rtc, hs).render(cam, DEPTH)                          # every table, then the mode
    gpu = handle(rtc, hs, mis_first=True)                               # the mode first
    before = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == MIS and np.array_equal(before, after)
    compare(before, want)
    # each of the three setters that derive the list again, after the mode: one image
    gpu.set_shadow_filters(hs.shadow_filters())
    gpu.set_indirect(hs.indirect())
    gpu.set_emitters(hs.emitters())
    assert np.array_equal(gpu.render(cam, DEPTH), after) and gpu.last_kernel_name() == MIS
