"""The priority order of the render-kernel families (family() in rtc_capi.hip): the `*_kernels` options set one after the
other, lowest first and the lower ones left set, take a handle up the whole list - sampling, motion, spot, bump, torus,
meshuv, gloss, occlusion, shadow filter, media, environment, sky light - and cleared highest first take it down again.
Every step renders the handle's ordinary image with the ordinary ray counts under the kernel of the highest family set.

Three worlds: cover.json (a simple world, tables in LDS), soft_shadows.json (an area world: its sampling kernel is
rtc_render_kernel_area_ms) and a generated world one light past the LDS limit (every name ends in _bigworld).  32 x 18 at
depth 5: more than one chunk, reflected and refracted rays; nothing here depends on the image's size."""
import os

import numpy as np
import pytest

import test_table_limits_gpu as limits

pytestmark = pytest.mark.gpu

FORCED_TOL = 1e-14  # (the feature modules' bound for their kernels forced on a handle against the handle's ordinary render)
W, H, DEPTH = 32, 18, 5
SOFT_SHADOWS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "area_scenes", "soft_shadows.json")
# (option, the family's kernel suffix), in ascending priority
LADDER = [("sampling_kernels", "_ms"), ("motion_kernels", "_motion"), ("spot_kernels", "_spot"), ("bump_kernels", "_bump"),
          ("torus_kernels", "_torus"), ("meshuv_kernels", "_meshuv"), ("gloss_kernels", "_gloss"), ("occlusion_kernels", "_occl"),
          ("shadow_filter_kernels", "_sfilter"), ("media_kernels", "_media"), ("environment_kernels", "_env"),
          ("sky_light_kernels", "_skyl")]


def _world(rtc, name):
    if name == "cover":
        return rtc.HostScene.from_file("cover.json")
    if name == "soft_shadows":
        return rtc.HostScene.from_file(SOFT_SHADOWS)
    case = next(c for c in limits.LIMIT_CASES if c.limit == ("LDS", "LIGHTS", "L+1"))
    return limits._host_scene(rtc, case)


def _same(gpu, got, first, counts, name, what):
    st = gpu.stats()
    delta = float(np.abs(got - first).max())
    print(f"{what}: {gpu.last_kernel_name()}: max |delta| {delta:.3e}")
    assert gpu.last_kernel_name() == name, what
    for k in ("primary", "secondary", "shadow_calls"):
        assert st[k] == counts[k], (what, k, st[k], counts[k])
    assert st["overflow"] == 0, what
    assert delta <= FORCED_TOL, (what, delta)


@pytest.mark.parametrize("world", ["cover", "soft_shadows", "lights_past_lds"])
def test_options_climb_and_descend_the_family_list(rtc, world):
    hs = _world(rtc, world)
    cam = hs.camera(W, H)
    gpu = rtc.GpuScene(hs.desc, lights=hs.lights)
    first = gpu.render(cam, DEPTH)
    counts = gpu.stats()
    base = gpu.last_kernel_name()
    print(f"{world}: {base} {counts}")
    big = "_bigworld" if world == "lights_past_lds" else ""
    assert base.endswith("_bigworld") == bool(big) and counts["overflow"] == 0
    ms = "_area_ms" if world == "soft_shadows" else "_ms"
    names = ["rtc_render_kernel" + (ms if suffix == "_ms" else suffix) + big for _, suffix in LADDER]
    try:
        for (option, _), name in zip(LADDER, names):
            rtc.set_option(option, 1)
            _same(gpu, gpu.render(cam, DEPTH), first, counts, name, f"up to {option}")
        # (a clone at the top: the sky-light pair's occupancy is asked for on a handle that has launched other kernels)
        twin = gpu.clone()
        _same(twin, twin.render(cam, DEPTH), first, counts, names[-1], "the clone at the top")
        twin.close()
        for k in reversed(range(len(LADDER))):
            rtc.set_option(LADDER[k][0], 0)
            _same(gpu, gpu.render(cam, DEPTH), first, counts, names[k - 1] if k else base, f"down past {LADDER[k][0]}")
    finally:
        for option, _ in LADDER:
            rtc.set_option(option, 0)
    gpu.close()
