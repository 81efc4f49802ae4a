"""UV-mapped mesh textures on the GPU (RTC_TEX_MESH, the meshuv kernels): every render of the fixture
against the checker (tests/cpp/meshuv_oracle.cpp) within 1e-12 with equal ray counts, no overflow and no pixel masked -
default sampling, a sample grid with a lens, a later pass, the moving mesh, both kernel forms, a close-up of the tiling
triangle, band clones, Progressive, an adaptive run, rtch_scene_render -, the kernel's name, the meshuv kernels on handles
without a mesh map against their ordinary renders, rtc_scene_set_mesh_uvs (NULL, again, clones, refusals), mapping 5 and
librtc_multi's refusal.  80 x 45 at depth 5 throughout.

Measured on an MI355X: see DESIGN.md section 19."""
import ctypes as C
import json

import numpy as np
import pytest

import bump_binding as bb
import camera_binding as cb
import meshuv_binding as mb
import test_table_limits_gpu as limits
import torus_binding as tb

pytestmark = pytest.mark.gpu

TOL = 1e-12         # (the project's bound for a render against its checker: tests/test_torus_gpu.py)
FORCED_TOL = 1e-14  # (a kernel family forced on a handle against the handle's ordinary render)
SPLIT_TOL = 1e-14   # (shares of a split frame's pixels added in another order)
L_LIGHTS = limits.LIMITS["LDS"]["LIGHTS"]
MESHUV, MESHUV_BIG = "rtc_render_kernel_meshuv", "rtc_render_kernel_meshuv_bigworld"
W, H, DEPTH = 80, 45, 5


def compare(got, want, tol=TOL):
    """No mask: every pixel counts."""
    delta = float(np.abs(got - want).max())
    print(f"max |delta| {delta:.3e}")
    assert delta <= tol, f"max |delta| {delta}"


def handle(rtc, hs, smp=None, sample_pass=0, disp=None, light_seed=0, uvs="scene"):
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
    gpu.set_mesh_uvs(hs.mesh_uvs() if isinstance(uvs, str) else uvs)
    return gpu


def checker(hs, uvs="scene"):
    return mb.MeshUvScene(hs.desc, hs.lights, hs.bumps(), hs.mesh_uvs() if isinstance(uvs, str) else uvs)


def check(rtc, hs, cam, smp=None, sample_pass=0, disp=None, light_seed=0, kernel=MESHUV, uvs="scene"):
    gpu = handle(rtc, hs, smp, sample_pass, disp, light_seed, uvs)
    got = gpu.render(cam, DEPTH)
    st = gpu.stats()
    assert gpu.last_kernel_name() == kernel
    want, counters = checker(hs, uvs).render(cam, DEPTH, smp, hs.spots(), disp, sample_pass, light_seed=light_seed)
    print({k: st[k] for k in ("primary", "secondary", "shadow_calls", "shadow_traced", "overflow")}, counters)
    compare(got, want)
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    grid = smp.grid if smp is not None else 1
    assert st["primary"] == cam.hsize * cam.vsize * grid * grid
    assert st["overflow"] == 0
    return got, gpu


def static(hs):
    return np.zeros((hs.desc.n_roots, 3))


# ---- the fixture against the checker
def test_fixture_against_the_checker(rtc):
    hs = mb.mix(rtc)
    assert len(mb.mesh_maps_of(hs.desc)) == 9 and hs.desc.n_tris == 262 and len(tb.tori_of(hs.desc)) == 1
    got, _ = check(rtc, hs, hs.camera(W, H), disp=static(hs), light_seed=3)
    assert got.std() > 0.05


def test_fixture_with_a_sample_grid_and_a_lens(rtc):
    hs = mb.mix(rtc)
    check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, aperture=0.08, focal_distance=9.0, seed=5), disp=static(hs), light_seed=3)


def test_fixture_at_sample_pass_3(rtc):
    hs = mb.mix(rtc)
    cam = hs.camera(W, H)
    p0, _ = check(rtc, hs, cam, cb.sampling(1, True, seed=2), disp=static(hs))
    p3, _ = check(rtc, hs, cam, cb.sampling(1, True, seed=2), sample_pass=3, disp=static(hs))
    assert not np.array_equal(p0, p3)


def test_fixture_with_the_moving_mesh(rtc):
    hs = mb.mix(rtc)
    disp = hs.motion()
    assert np.count_nonzero(np.abs(disp).sum(axis=1)) == 1   # the fixture's one moving mesh
    moving, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, seed=6), disp=disp, light_seed=11)
    still, _ = check(rtc, hs, hs.camera(W, H), cb.sampling(2, True, seed=6), disp=static(hs), light_seed=11)
    assert not np.array_equal(moving, still)


def _with_many_lights(n):
    """mesh_mix.json with point lights added until it has n: RTC_LDS_LIGHTS lights select the LDS kernel, one more the
    big-world one (tests/test_torus_gpu.py's way)"""
    scene = json.loads(open(mb.MESH_MIX).read())
    k = 0
    while len(scene["lights"]) < n:
        a = 0.7 * k
        scene["lights"].append({"point-light": {"position": [6 * np.cos(a), 6 + k % 3, 6 * np.sin(a)], "intensity": [0.03, 0.03, 0.04]}})
        k += 1
    return json.dumps(scene)


@pytest.mark.parametrize("extra", [0, 1])
def test_fixture_in_both_kernel_forms(rtc, extra):
    hs = rtc.HostScene(_with_many_lights(L_LIGHTS + extra), mb.MESHUV_DIR)
    assert hs.lights.n_lights == L_LIGHTS + extra
    check(rtc, hs, hs.camera(W, H), disp=hs.motion(), light_seed=3, kernel=MESHUV_BIG if extra else MESHUV)


def test_close_up_of_the_tiling_triangle(rtc):
    """The tiling triangle of the row under the uv test pattern fills the frame: its edges and the wrap lines of both
    coordinates cross many pixels."""
    scene = json.loads(open(mb.MESH_MIX).read())
    scene["camera"] = {"width": W, "height": H, "field-of-view": 0.5, "from": [0.7, 3.5, -0.4], "to": [0.7, 3.35, 2.8], "up": [0, 1, 0]}
    hs = rtc.HostScene(json.dumps(scene), mb.MESHUV_DIR)
    got, _ = check(rtc, hs, hs.camera(), disp=static(hs))
    # (the uv test pattern's colour is (tu, tv, 0) times the lights: a wrap line is a jump in the red or the green channel)
    assert got.std() > 0.05
    assert np.abs(np.diff(got[..., 0], axis=1)).max() > 0.3 and np.abs(np.diff(got[..., 1], axis=0)).max() > 0.3


# ---- band clones, a clone
def test_a_clone_and_band_clones_follow(rtc):
    hs = mb.mix(rtc)
    cam = hs.camera(W, H)
    gpu = handle(rtc, hs, disp=hs.motion())
    rtc.set_option("host_bands", 3)
    try:
        banded = gpu.render(cam, DEPTH)
        st = gpu.stats()
    finally:
        rtc.set_option("host_bands", 0)
    want, counters = checker(hs).render(cam, DEPTH, spots=hs.spots(), disp=hs.motion())
    compare(banded, want)
    for k in ("primary", "secondary", "shadow_calls"):           # (the bands' counts, summed)
        assert st[k] == counters[k], (k, st[k], counters[k])
    assert st["overflow"] == 0
    whole = gpu.render(cam, DEPTH)
    assert float(np.abs(whole - banded).max()) <= SPLIT_TOL
    clone = gpu.clone()
    assert np.array_equal(clone.render(cam, DEPTH), whole)   # a clone starts with its source's rows
    assert clone.last_kernel_name() == MESHUV


# ---- Progressive, an adaptive run, rtch_scene_render
def _passes(hs, cam, smp, n):
    """[(image, counters)] of the checker's sample passes 0 .. n-1"""
    ck = checker(hs)
    return [ck.render(cam, DEPTH, smp, hs.spots(), hs.motion(), sample_pass=p) for p in range(n)]


def _pass_images(hs, cam, smp, n):
    return [im for im, _ in _passes(hs, cam, smp, n)]


def _same_counts(st, counters):
    print({k: st[k] for k in ("primary", "secondary", "shadow_calls", "overflow")}, counters)
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counters[k], (k, st[k], counters[k])
    assert st["overflow"] == 0


def test_progressive_mean_is_the_checkers(rtc):
    import torch
    hs = mb.mix(rtc)
    cam = hs.camera(W, H)
    smp = cb.sampling(1, True, seed=4)
    gpu = handle(rtc, hs, smp, disp=hs.motion())
    want = _passes(hs, cam, smp, 3)
    prog = rtc.Progressive(gpu, cam, DEPTH)
    for p in range(3):
        prog.step()
        _same_counts(gpu.stats(), want[p][1])                    # (the handle's counts are its last launch's: pass p)
    mean = prog.mean().cpu().numpy()
    torch.cuda.synchronize()
    assert gpu.last_kernel_name() == MESHUV
    compare(mean, np.mean([im for im, _ in want], axis=0))


def test_adaptive_and_host_render_of_the_fixture(rtc):
    scene = json.loads(open(mb.MESH_MIX).read())
    scene["camera"].update(width=80, height=48, sampling={"grid": 1, "jitter": True, "seed": 4, "passes": 5,
                                                          "adaptive": {"threshold": 0.004, "min-passes": 2, "tile": [16, 16]}})
    hs = rtc.HostScene(json.dumps(scene), mb.MESHUV_DIR)
    a = hs.adaptive()
    out = np.zeros((48, 80, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(hs._h, 0, 0, DEPTH, out.ctypes.data))
    gpu = handle(rtc, hs, hs.sampling(), disp=hs.motion())
    rgb, passes = gpu.render_adaptive(hs.camera(), a)
    assert gpu.last_kernel_name() == MESHUV
    assert np.array_equal(out, rgb)
    assert passes.min() >= 2 and passes.max() <= 5
    images = _pass_images(hs, hs.camera(), hs.sampling(), 5)
    want = np.zeros_like(rgb)
    tiles_x = 80 // 16
    for t, k in enumerate(passes):
        ty, tx = divmod(t, tiles_x)
        want[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = np.mean([im[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] for im in images[:k]], axis=0)
    compare(rgb, want)
    # the ray counts, round by round: round R renders the tiles still active at sample pass R in one launch, whose counts
    # the handle reports - the checker's counts of those tiles at that pass, summed
    import adaptive_binding as ab
    ck = checker(hs)
    cam = hs.camera()
    run = rtc.AdaptiveProgressive(gpu, cam, DEPTH, a)
    before = np.zeros(len(passes), dtype=np.uint32)
    rounds = 0
    while True:
        left = run.step()
        now = run.tile_passes().cpu().numpy().view(np.uint32).copy()
        rendered = np.nonzero(now != before)[0]
        if len(rendered) == 0:
            break
        total = {"primary": 0, "secondary": 0, "shadow_calls": 0}
        for t in rendered:
            _, c = ck.render(cam, DEPTH, hs.sampling(), hs.spots(), hs.motion(), sample_pass=rounds, tile=ab.tile_rect(int(t), 80, 48, 16, 16))
            total = {k: total[k] + c[k] for k in total}
        _same_counts(gpu.stats(), total)
        before, rounds = now, rounds + 1
        if left == 0:
            break
    assert np.array_equal(before, passes) and rounds == passes.max()
    # without "adaptive": rtch_scene_render is one rtc_render of the handle, the texture rows applied.  (Its handle lives and
    # dies inside the call - rtc_host.h has no way to its rtc_get_stats -, so of the host render the image alone is held to
    # the checker; the same description's counts are the ones test_fixture_with_the_moving_mesh holds equal.)
    plain = mb.mix(rtc)
    out1 = np.zeros((H, W, 3))
    rtc._check_host(rtc.host_lib().rtch_scene_render(plain._h, W, H, DEPTH, out1.ctypes.data))
    want1, _ = checker(plain).render(plain.camera(W, H), DEPTH, spots=plain.spots(), disp=plain.motion())
    compare(out1, want1)


# ---- which kernel; the meshuv kernels on a handle without a mesh map
@pytest.mark.parametrize("name", ["cover.json", "teapot.json", "torus_mix"])
def test_handles_without_a_mesh_map_keep_their_kernel(rtc, name):
    hs = tb.mix(rtc) if name == "torus_mix" else rtc.HostScene.from_file(name)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.render(hs.camera(W, H), DEPTH)
    # (what renderKernel picked for these handles before the meshuv family stood in front of it: cover's simple world that
    # is mostly cubes runs the box-culling simple kernel, in its three-wave form where the pixel map is large enough for
    # it - usesSimple3 -; teapot's groups the general kernel, or its three-wave form after the handle's trial)
    want = {"cover.json": ("rtc_render_kernel_simple_b", "rtc_render_kernel_simple3_b"),
            "teapot.json": ("rtc_render_kernel", "rtc_render_kernel3"), "torus_mix": ("rtc_render_kernel_torus",)}[name]
    print(name, gpu.last_kernel_name())
    assert gpu.last_kernel_name() in want


@pytest.mark.parametrize("name", ["cover.json", "bump_mix", "torus_mix", "teapot.json"])
def test_meshuv_kernels_without_a_mesh_map_are_the_ordinary_render(rtc, name):
    hs = bb.mix(rtc) if name == "bump_mix" else tb.mix(rtc) if name == "torus_mix" else rtc.HostScene.from_file(name)
    cam = hs.camera(W, H)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    gpu.set_spots(hs.spots())
    gpu.set_bumps(hs.bumps())
    ordinary = gpu.render(cam, DEPTH)
    st0 = gpu.stats()
    old_name = gpu.last_kernel_name()
    assert "_meshuv" not in old_name
    rtc.set_option("meshuv_kernels", 1)
    try:
        forced = gpu.render(cam, DEPTH)
        st1 = gpu.stats()
        assert gpu.last_kernel_name() == MESHUV
    finally:
        rtc.set_option("meshuv_kernels", 0)
    delta = float(np.abs(forced - ordinary).max())
    print(f"{name}: {old_name} against {MESHUV}: max |delta| {delta:.3e}")
    assert delta <= FORCED_TOL
    for k in ("primary", "secondary", "shadow_calls", "overflow"):
        assert st0[k] == st1[k], k
    again = gpu.render(cam, DEPTH)
    assert float(np.abs(again - ordinary).max()) <= FORCED_TOL
    assert gpu.last_kernel_name() == old_name


# ---- rtc_scene_set_mesh_uvs
def _quad_scene():
    """the unit quad of mesh_quads.obj alone, under the uv test pattern, lit by one light"""
    cam = {"width": W, "height": H, "field-of-view": 0.6, "from": [-2.7, 0.5, -4], "to": [-2.7, 0.5, 0], "up": [0, 1, 0]}
    obj = {"type": {"from-obj": {"file": "mesh_quads.obj", "normalize": False, "texture-coordinates": True}},
           "material": {"pattern": {"type": {"texture-map": {"mesh": {"uv-pattern": {"checkers": {"width": 4, "height": 4, "patterns": [
               {"type": {"solid": [1, 0.2, 0.2]}}, {"type": {"solid": [0.2, 0.2, 1]}}]}}}}}}, "ambient": 1, "diffuse": 0, "specular": 0}}
    lights = [{"point-light": {"position": [-3, 4, -6], "intensity": [1, 1, 1]}}]
    return json.dumps({"camera": cam, "lights": lights, "objects": [obj]})


def test_set_mesh_uvs_null_again_and_refusals(rtc):
    hs = rtc.HostScene(_quad_scene(), mb.MESHUV_DIR)
    cam = hs.camera()
    rows = hs.mesh_uvs()
    first, gpu = check(rtc, hs, cam)
    assert len(np.unique(first.reshape(-1, 3), axis=0)) >= 3          # both checker colours and the background
    gpu.set_mesh_uvs(None)
    zero = gpu.render(cam, DEPTH)
    assert gpu.last_kernel_name() == MESHUV
    want, _ = checker(hs, uvs=None).render(cam, DEPTH)
    compare(zero, want)
    hit = zero.sum(axis=2) > 0
    assert hit.any() and np.all(zero[hit] == np.array([1.0, 0.2, 0.2]))   # the colour of (0, 0): every triangle, every pixel
    gpu.set_mesh_uvs(rows)
    assert np.array_equal(gpu.render(cam, DEPTH), first)
    with pytest.raises(rtc.RtcError) as e:
        gpu.set_mesh_uvs(rows[:-1])
    assert e.value.name == _status_name(rtc, 1)                       # RTC_ERR_INVALID_ARGUMENT
    bad = rows.copy()
    bad[2, 3] = np.nan
    with pytest.raises(rtc.RtcError) as e:
        gpu.set_mesh_uvs(bad)
    assert e.value.name == _status_name(rtc, 1)                       # RTC_ERR_INVALID_ARGUMENT
    assert np.array_equal(gpu.render(cam, DEPTH), first)              # a refused table changes nothing
    assert np.array_equal(gpu.clone().render(cam, DEPTH), first)


def _status_name(rtc, code):
    return rtc.hip_lib().rtc_status_name(code).decode()


def _desc_with_mapping(rtc, hs, value):
    d, (kinds, maps) = mb.with_placeholders(hs.desc, mapping=value)
    return d, (kinds, maps)


def test_mapping_5_is_unsupported_and_multi_refuses_the_fixture(rtc):
    hs = mb.mix(rtc)
    d, keep = _desc_with_mapping(rtc, hs, 5)
    with pytest.raises(rtc.RtcError) as e:
        rtc.GpuScene(d, lights=hs.lights)
    assert e.value.name == _status_name(rtc, 4) and "mapping 5" in str(e.value)   # RTC_ERR_UNSUPPORTED
    d4, keep4 = _desc_with_mapping(rtc, hs, 4)                        # (the same copy with mapping 4 is accepted)
    rtc.GpuScene(d4, lights=hs.lights).close()
    with pytest.raises(rtc.RtcError) as e:
        rtc.MultiGpu(hs.desc, 1)
    assert e.value.name == _status_name(rtc, 4) and "RTC_TEX_MESH" in str(e.value)
