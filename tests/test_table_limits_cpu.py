"""CPU guards of tests/test_table_limits_gpu.py and of the diagnostic build it reads.

* Every render kernel the library declares is the expected kernel of some case of the GPU module, and every table limit
  of csrc/rtc_device.h has a case at the limit and one past it, where the kernel changes: a new kernel or a new limit
  fails here until it has boundary tests.
* The generated worlds have the table sizes the cases state (the loader's description, no GPU).
* The -DRTC_PROFILE build - the one that counts accesses outside their allocation - still compiles for gfx950.
"""
import os
import re
import subprocess

import pytest

import test_table_limits_gpu as limits

CAPI = os.path.join(limits.CSRC, "rtc_capi.hip")


def _declared_render_kernels():
    with open(CAPI) as f:
        return set(re.findall(r'extern "C" __global__ void (rtc_render_kernel\w*)\s*\(', f.read()))


def test_every_render_kernel_is_expected_somewhere():
    declared = _declared_render_kernels()
    assert len(declared) >= 12, declared
    expected = {k for c in limits.ALL_CASES for k in c.kernels()}
    assert declared - expected == set(), f"render kernels without a boundary case: {sorted(declared - expected)}"
    assert expected - declared == set(), f"expected kernels the library does not declare: {sorted(expected - declared)}"


def test_every_limit_is_crossed():
    parsed = limits.header_limits()
    assert set(parsed) == {"LDS", "LDS3"} and all(set(v) == set(limits.TABLES) for v in parsed.values()), parsed
    for group, tables in parsed.items():
        for table, lim in tables.items():
            at = [c for c in limits.LIMIT_CASES if c.limit == (group, table, "L")]
            past = [c for c in limits.LIMIT_CASES if c.limit == (group, table, "L+1")]
            assert at and past, (group, table)
            assert all(c.world.counts[table] == lim for c in at), (group, table)
            assert all(c.world.counts[table] == lim + 1 for c in past), (group, table)
            # the same world classes on both sides, and on each the kernel changes at L + 1
            by_class = {c.name.split("-")[1]: c.kernels() for c in at}
            for c in past:
                cls = c.name.split("-")[1]
                assert cls in by_class, (group, table, cls)
                assert by_class[cls] != c.kernels(), (group, table, cls, c.kernels())


def test_root_sweep_covers_the_remainders():
    names = {c.name for c in limits.SWEEP_CASES}
    for nb in limits.SWEEP_BOUNDED:
        assert any(n.startswith(f"bounded{nb}-") for n in names), nb
    assert "round5-18roots-mostly-cubes-simple3_b" in names
    kernels = {k for c in limits.SWEEP_CASES for k in c.kernels()}
    assert {"rtc_render_kernel_simple", "rtc_render_kernel_simple_b", "rtc_render_kernel_simple3", "rtc_render_kernel_simple3_b",
            "rtc_render_kernel_bigworld"} <= kernels


def test_generated_worlds_have_the_stated_table_sizes(rtc):
    """The loader's description of every case's world (the GPU module asserts the same before it renders)."""
    for case in limits.ALL_CASES:
        limits._host_scene(rtc, case)


@pytest.mark.parametrize("source", ["rtc_kernels.hip", "rtc_capi.hip"])
def test_profile_build_compiles(source, tmp_path):
    """The diagnostic build (-DRTC_PROFILE: section stamps, walk counters, the out-of-bounds counts) cross-compiles for
    gfx950, so that it cannot rot while only the product build is made."""
    hipcc = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-O3", "-ffp-contract=off", "-fPIC", "-Wall", "-Wno-unused-result",
           "-DRTC_PROFILE", "-c", "-o", str(tmp_path / "out.o"), os.path.join(limits.CSRC, source)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=230)
    assert r.returncode == 0, r.stderr[-4000:]
