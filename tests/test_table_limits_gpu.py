"""Every render kernel at the edges of its tables, against the oracle.

rtc_scene_create picks one of twelve render kernels for a world (`renderKernel` / `ldsKernel` in csrc/rtc_capi.hip) by what
the world is made of and by four table sizes - top-level objects, materials, patterns, lights - held against two sets of
limits (`RTC_LDS_*` for the two-wave LDS kernels, `RTC_LDS3_*` for the three-wave ones, csrc/rtc_device.h).  Inside the
kernels the same sizes decide how the tables are staged into LDS and walked: phase 1 of the root loop takes the roots in
blocks of 64, four at a time with a half step for a remainder of one or two, and stops where the planes begin.

Here every kernel runs on both sides of every limit it has, and the simple kernels on every remainder of the root loop,
each case against the oracle's image and ray counters.  The limits are read from the header; the kernel each case must
run is stated by `expected_kernel` below, a restatement of the selection rules, and asserted on every launch.  The
worlds are generated with exact table sizes, and every case asserts them on the loader's description, so that a loader
change cannot move a case off its edge unnoticed.

Image parity cannot see an access outside a table whose result is masked, culled or overwritten.  The diagnostic build
(-DRTC_PROFILE) counts such accesses instead of making them; `test_no_access_out_of_bounds` reads the counts of every
case from that build's RTC_PROFILE_DUMP output (and skips against the product build, which has none).
"""
import json
import math
import os
import random
import re
from dataclasses import dataclass, field

import numpy as np
import pytest

import oracle_binding as ob
from test_parity_gpu import REPEAT_TOL, TOL

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "ray-tracer-challenge_amd", "csrc")
DEPTH = 5
TABLES = ("ROOTS", "MATERIALS", "PATTERNS", "LIGHTS")


def header_limits():
    """{"LDS": {"ROOTS": 128, ...}, "LDS3": {...}}: the RTC_LDS_* and RTC_LDS3_* limits as csrc/rtc_device.h defines them."""
    with open(os.path.join(CSRC, "rtc_device.h")) as f:
        text = f.read()
    limits = {}
    for group, table, value in re.findall(r"^\s*#define\s+RTC_(LDS3?)_([A-Z]+)\s+(\d+)\s*$", text, re.M):
        limits.setdefault(group, {})[table] = int(value)
    return limits


LIMITS = header_limits()


# ---------------------------------------------------------------- the selection rules, restated
@dataclass(frozen=True)
class Options:
    """What the test forces through rtc_set_option: box_cull (None: the world's own choice, more cubes than spheres),
    three waves per SIMD or two (simple3_min_chunks 0 / 1e9 and waves3 1 / 0)."""
    box_cull: object = None
    three: bool = False

    def apply(self, rtc):
        rtc.set_option("box_cull", -1 if self.box_cull is None else int(self.box_cull))
        rtc.set_option("simple3_min_chunks", 0 if self.three else 1e9)
        rtc.set_option("waves3", 1 if self.three else 0)

    @staticmethod
    def reset(rtc):
        for name in ("box_cull", "simple3_min_chunks", "waves3"):
            rtc.set_option(name, -1)

    def label(self):
        return f"box{'-' if self.box_cull is None else int(self.box_cull)}-{'3w' if self.three else '2w'}"


def fits(counts, group):
    lim = LIMITS[group]
    return all(counts[t] <= lim[t] for t in TABLES)


def expected_kernel(world, opts):
    """The kernel rtc_scene_create + launch pick (renderKernel, ldsKernel, usesSimple3, usesGeneral3 in rtc_capi.hip).
    `world`: the World's counts and what it is made of: groups or csg (a node), leaves other than spheres, planes and
    cubes, and whether it needs an `_ext` kernel (csg, a texture map, a gradient or blend nested in another)."""
    c = world.counts
    ext = world.ext is not None
    if not fits(c, "LDS"):
        return "rtc_render_kernel_bigworld_ext" if ext else "rtc_render_kernel_bigworld"
    flat = not world.has_nodes
    simple = flat and not world.others
    box = (world.cubes > world.spheres) if opts.box_cull is None else bool(opts.box_cull)
    fits3 = fits(c, "LDS3")
    if opts.three and simple and not ext and fits3:
        return "rtc_render_kernel_simple3_b" if box else "rtc_render_kernel_simple3"
    if opts.three and not flat and not ext and fits3:
        return "rtc_render_kernel3"
    if simple:
        return "rtc_render_kernel_simple_ext" if ext else ("rtc_render_kernel_simple_b" if box else "rtc_render_kernel_simple")
    if flat:
        return "rtc_render_kernel_flat_ext" if ext else "rtc_render_kernel_flat"
    return "rtc_render_kernel_ext" if ext else "rtc_render_kernel"


# ---------------------------------------------------------------- worlds with exact table sizes
def _colour(k):
    """Pairwise different solid colours (the third channel grows with k)."""
    return [round(0.15 + 0.7 * ((k * 0.6180339887) % 1.0), 6), round(0.2 + 0.1 * (k % 7), 6), round(0.1 + 0.8 * k / 512.0, 6)]


def _solid(k):
    return {"type": {"solid": _colour(k)}}


@dataclass
class World:
    """Top-level objects by kind, an optional `_ext` trigger and the sizes of the material, pattern and light tables.

    spheres, cubes, planes, others (closed cylinders and cones), groups (a sphere and a cube each), and `ext`: None,
    "csg" (one more top-level object: a sphere minus a cube), "texture" (a spherical texture map on a sphere's material)
    or "blend" (a gradient nested in a blend).  `order`: "table" lists World.objects in the kernels' table order,
    [spheres][cubes][the rest][planes]; "shuffled" interleaves the kinds (seeded), so that the table is a permutation of
    World.objects."""
    spheres: int = 0
    cubes: int = 0
    planes: int = 0
    others: int = 0
    groups: int = 0
    ext: object = None
    materials: int = 6
    patterns: int = 6
    lights: int = 2
    order: str = "table"
    twins: bool = False   # two bit-identical spheres with different materials on either side of a cube in World.objects
    size: tuple = (64, 48)
    counts: dict = field(init=False)

    def __post_init__(self):
        roots = self.spheres + self.cubes + self.planes + self.others + self.groups + (self.ext == "csg") + 2 * self.twins
        self.counts = {"ROOTS": roots, "MATERIALS": self.materials, "PATTERNS": self.patterns, "LIGHTS": self.lights}

    @property
    def has_nodes(self):
        return self.groups > 0 or self.ext == "csg"

    def leaves(self):
        return self.spheres + self.cubes + self.planes + self.others + 2 * self.groups + 2 * (self.ext == "csg") + 2 * self.twins

    def scene(self):
        """The scene JSON.  Every material is used; materials differ by diffuse, patterns by colour (both tables are
        deduplicated by the loader); material 0 is reflective, material 1 transparent."""
        trig_mat = self.ext in ("texture", "blend")
        trig_pat = {"texture": 1, "blend": 2}.get(self.ext, 0)   # the trigger's children are colours already in the table
        n_plain = self.materials - trig_mat
        p_plain = self.patterns - trig_pat
        assert n_plain >= 1 and 1 <= p_plain <= 3 * n_plain - 1, (self.materials, self.patterns, self.ext)
        assert self.leaves() >= self.materials, "every material needs an object"
        extra = max(0, p_plain - n_plain)   # patterns beyond one solid per material: checkers of two solids
        pats = [_solid(j % p_plain) for j in range(n_plain)]
        for i in range(extra // 2):   # a checkers of the material's colour and a new one: two patterns more
            j = n_plain - 1 - i
            pats[j] = {"type": {"checkers": [_solid(j), _solid(256 + j)]}, "transform": [{"scale": [0.2, 0.2, 0.2]}]}
        if extra % 2:                 # ... of the material's colour and material 0's: one more
            j = n_plain - 1 - extra // 2
            assert j > 0
            pats[j] = {"type": {"checkers": [_solid(j), _solid(0)]}, "transform": [{"scale": [0.2, 0.2, 0.2]}]}

        def material(j):
            m = {"pattern": pats[j], "diffuse": round(0.45 + 0.4 * j / n_plain, 6), "specular": 0.3}
            if j % 3 == 0:
                m["reflective"] = 0.35
            elif j % 3 == 1:
                m.update({"transparency": 0.7, "refractive-index": 1.3, "reflective": 0.1})
            return m
        mats = [material(j) for j in range(n_plain)]
        if self.ext == "texture":
            mats.append({"pattern": {"type": {"texture-map": {"spherical": {"uv-pattern": {"checkers": {
                "width": 8, "height": 4, "patterns": [_solid(0), _solid(1)]}}}}}}, "specular": 0.2})
        elif self.ext == "blend":
            mats.append({"pattern": {"type": {"blend": [{"type": {"gradient": [_solid(0), _solid(1)]}}, _solid(1)]},
                                     "transform": [{"scale": [0.3, 0.3, 0.3]}]}, "diffuse": 0.8})
        next_mat = iter(range(10 ** 6))

        def take():   # the materials in turn, the trigger's once (the loader makes a texture map per object) and second
            c = next(next_mat)
            if trig_mat and c == 1:
                return mats[-1]
            return mats[(c - trig_mat if c else 0) % n_plain]

        slots = iter(range(10 ** 6))

        def place(scale):   # a grid of cells on the floor in front of the camera
            i = next(slots)
            x, z = (i % 12 - 5.5) * 0.95, (i // 12) * 0.95 - 2.5
            return [{"scale": [scale, scale, scale]}, {"rotate-y": 0.37 * i}, {"translate": [x, scale, z]}]

        def sphere():
            return {"type": {"sphere": {}}, "transform": place(0.36), "material": take()}

        def cube():
            return {"type": {"cube": {}}, "transform": place(0.3), "material": take()}

        def other(k):
            kind = {"cylinder": {"min": -1, "max": 1, "closed": True}} if k % 2 == 0 else {"cone": {"min": -1, "max": 0, "closed": True}}
            return {"type": kind, "transform": place(0.32), "material": take()}

        def group():
            t = place(1.0)
            return {"type": {"group": [
                {"type": {"sphere": {}}, "transform": [{"scale": [0.25, 0.25, 0.25]}, {"translate": [-0.2, 0.0, 0]}], "material": take()},
                {"type": {"cube": {}}, "transform": [{"scale": [0.2, 0.2, 0.2]}, {"translate": [0.25, -0.2, 0.1]}], "material": take()}]},
                "transform": [t[1], t[2]]}

        def plane(k):
            where = [[], [{"rotate-x": math.pi / 2}, {"translate": [0, 0, 14]}], [{"rotate-z": math.pi / 2}, {"translate": [-10, 0, 0]}]]
            return {"type": {"plane": {}}, "transform": where[k] if k < 3 else [{"translate": [0, -1.0 - k, 0]}], "material": take()}

        planes = [plane(k) for k in range(self.planes)]   # (first: the floor is material 0, reflective)
        kinds = [[sphere() for _ in range(self.spheres)], [cube() for _ in range(self.cubes)],
                 [other(k) for k in range(self.others)] + [group() for _ in range(self.groups)], planes]
        if self.ext == "csg":
            kinds[2].append({"type": {"csg": {"operation": "difference", "left": {"type": {"sphere": {}}, "material": take()},
                                              "right": {"type": {"cube": {}}, "transform": [{"scale": [0.6, 0.6, 0.6]}, {"translate": [0.5, 0.5, -0.5]}],
                                                        "material": take()}}},
                             "transform": place(0.4)})
        objs = [o for k in kinds for o in k]
        if self.order == "shuffled":
            random.Random(len(objs) * 7 + self.planes).shuffle(objs)
        if self.twins:   # [.., sphere (material 0), cube, the same sphere (material 1), ..]
            t = place(0.5)
            a = {"type": {"sphere": {}}, "transform": t, "material": mats[0]}
            b = {"type": {"sphere": {}}, "transform": t, "material": mats[1]}
            at = next(i for i, o in enumerate(objs) if "cube" in o["type"])
            objs[at:at + 1] = [a, objs[at], b]
        n = self.lights
        lights = [{"point-light": {"position": [round(-9 + 18 * k / max(1, n - 1), 6), 9 + 0.5 * (k % 3), -9 + 0.7 * k],
                                   "intensity": [round(1.4 / n, 6)] * 3}} for k in range(n)]
        w, h = self.size
        return json.dumps({"camera": {"width": w, "height": h, "field-of-view": 1.15, "from": [0.5, 6.5, -13], "to": [0, 0.5, 1],
                                      "up": [0, 1, 0]}, "lights": lights, "objects": objs})


@dataclass
class Case:
    name: str
    world: World
    options: tuple   # Options, each run on a handle of its own
    limit: tuple = None   # (group, table, "L" or "L+1") of the limit matrix

    def kernels(self):
        return [expected_kernel(self.world, o) for o in self.options]


# ---------------------------------------------------------------- the limit matrix
def _class_world(cls, roots, **tables):
    """A world of class `cls` with `roots` top-level objects (a plane among them)."""
    ext = {"spheres_ext": "texture", "flat_ext": "blend", "groups_ext": "csg"}.get(cls)
    base = cls.replace("_ext", "").replace("3", "")
    n = roots - (ext == "csg") - 1   # (the floor)
    if base == "spheres":
        return World(spheres=n - n // 4, cubes=n // 4, planes=1, ext=ext, **tables)
    if base == "cubes":
        return World(spheres=n // 4, cubes=n - n // 4, planes=1, ext=ext, **tables)
    if base == "flat":
        others = max(1, n // 5)
        return World(spheres=(n - others + 1) // 2, cubes=(n - others) // 2, others=others, planes=1, ext=ext, **tables)
    groups = max(1, n // 6)
    return World(spheres=(n - groups) // 2, cubes=(n - groups + 1) // 2 - 1, others=1, groups=groups, planes=1, ext=ext, **tables)


CLASSES = {"LDS": ["spheres", "cubes", "flat", "groups", "spheres_ext", "flat_ext", "groups_ext"],
           "LDS3": ["spheres3", "cubes3", "groups3"]}


def limit_cases():
    cases = []
    for group, classes in CLASSES.items():
        for table in TABLES:
            lim = LIMITS[group][table]
            for side, value in (("L", lim), ("L+1", lim + 1)):
                for cls in classes:
                    three = group == "LDS3"
                    # the other tables stay inside the three-wave limits (a two-wave limit's cases: well inside both)
                    t = {"ROOTS": 12, "MATERIALS": 6, "PATTERNS": 6, "LIGHTS": 2}
                    t[table] = value
                    if table == "MATERIALS":
                        t["ROOTS"] = max(t["ROOTS"], value)
                    if table == "PATTERNS":
                        t["MATERIALS"] = min(value, LIMITS[group]["MATERIALS"])
                        t["ROOTS"] = max(t["ROOTS"], t["MATERIALS"])
                    k = len(cases)
                    size = (63, 65) if k % 7 == 0 else (9, 1) if k % 7 == 3 else (64, 48)
                    world = _class_world(cls, t["ROOTS"], materials=t["MATERIALS"], patterns=t["PATTERNS"], lights=t["LIGHTS"],
                                         size=size)
                    cases.append(Case(f"{group}_{table}_{side}-{cls}-{size[0]}x{size[1]}", world, (Options(three=three),),
                                      (group, table, side)))
    return cases


# ---------------------------------------------------------------- the root loop's remainders
SWEEP_BOUNDED = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 18, 19, 31, 32, 33, 63, 64, 65, 127, 128)
SWEEP_SHUFFLED = (9, 33, 65)   # World.objects with the kinds interleaved: the table is a permutation of it


def sweep_cases():
    cases = []
    for nb in SWEEP_BOUNDED:
        for planes in (0, 1, 3):
            roots = nb + planes
            if roots == 0 or roots > LIMITS["LDS"]["ROOTS"]:
                continue
            mats = min(6, roots)
            world = World(spheres=(nb + 1) // 2, cubes=nb // 2, planes=planes, materials=mats, patterns=min(mats, 5),
                          order="shuffled" if nb in SWEEP_SHUFFLED else "table", size=(63, 65) if nb in (17, 65) else (64, 48))
            threes = (False, True) if roots <= LIMITS["LDS3"]["ROOTS"] else (False,)
            opts = tuple(Options(box_cull=b, three=t) for b in (0, 1) for t in threes)
            cases.append(Case(f"bounded{nb}-planes{planes}", world, opts))
    # just past the two-wave limit: the tables in memory
    big = LIMITS["LDS"]["ROOTS"] + 1
    cases.append(Case(f"bounded{big}-planes1", World(spheres=(big + 1) // 2, cubes=big // 2, planes=1), (Options(box_cull=0), Options(box_cull=1))))
    # 63 bounded roots with one plane closing the first block of 64 and another in the second: the one-lane traces'
    # plane loop once rendered this world off the oracle (bounded63-planes3 above is the same with two planes there)
    cases.append(Case("bounded63-planes2", World(spheres=32, cubes=31, planes=2, materials=6, patterns=5),
                      (Options(box_cull=0), Options(box_cull=1))))
    # the shape of round 5's fault: 18 roots, mostly cubes, under the three-wave box kernel
    cases.append(Case("round5-18roots-mostly-cubes-simple3_b", World(spheres=3, cubes=14, planes=1), (Options(three=True),)))
    # two bit-identical spheres with different materials on either side of a cube: the reference's order decides
    cases.append(Case("twin-spheres", World(spheres=6, cubes=5, planes=1, order="shuffled", twins=True),
                      tuple(Options(box_cull=b, three=t) for b in (0, 1) for t in (False, True))))
    return cases


LIMIT_CASES = limit_cases()
SWEEP_CASES = sweep_cases()
ALL_CASES = LIMIT_CASES + SWEEP_CASES


# ---------------------------------------------------------------- running a case
def _host_scene(rtc, case):
    hs = rtc.HostScene(case.world.scene())
    d = hs.desc
    got = {"ROOTS": d.n_roots, "MATERIALS": d.n_materials, "PATTERNS": d.n_patterns, "LIGHTS": d.n_lights}
    assert got == case.world.counts, (case.name, got, case.world.counts)
    return hs


def _launch(gpu, cam, want, counters, what):
    got = gpu.render(cam, DEPTH)
    st = gpu.stats()
    assert np.isfinite(got).all(), what
    assert np.abs(got - want).max() < TOL, (what, float(np.abs(got - want).max()))
    assert st["overflow"] == 0, what
    assert [st["primary"], st["secondary"], st["shadow_calls"]] == [counters["primary"], counters["secondary"], counters["shadow"]], what
    return got


def _run_case(rtc, case):
    hs = _host_scene(rtc, case)
    cam = hs.camera(*case.world.size)
    want, counters = ob.OracleScene(hs.desc).render(cam, DEPTH)
    assert counters["primary"] == cam.hsize * cam.vsize and counters["secondary"] > 0, case.name   # (secondary rays: the pending stacks are used)
    for opts, kernel in zip(case.options, case.kernels()):
        opts.apply(rtc)
        try:
            gpu = rtc.GpuScene(hs.desc)
            # launch 1: the estimate-based schedule (rtc_estimate_kernel reads the root tables too); launch 2: packed on the device
            first = _launch(gpu, cam, want, counters, (case.name, opts.label(), "launch 1"))
            assert gpu.last_kernel_name() == kernel, (case.name, opts.label(), gpu.last_kernel_name())
            second = _launch(gpu, cam, want, counters, (case.name, opts.label(), "launch 2"))
            assert gpu.last_kernel_name() == kernel, (case.name, opts.label(), gpu.last_kernel_name())
            gpu.close()
        finally:
            Options.reset(rtc)
        assert np.abs(second - first).max() < REPEAT_TOL, (case.name, opts.label())


@pytest.mark.parametrize("case", LIMIT_CASES, ids=lambda c: c.name)
def test_kernel_at_table_limit(rtc, case):
    _run_case(rtc, case)


@pytest.mark.parametrize("case", SWEEP_CASES, ids=lambda c: c.name)
def test_root_loop_remainders(rtc, case):
    _run_case(rtc, case)


def test_twin_spheres_order_decides(rtc):
    """The twin-spheres world is only a test of order if the order matters: with the twins swapped in World.objects the
    oracle's image changes."""
    case = next(c for c in SWEEP_CASES if c.name == "twin-spheres")
    js = json.loads(case.world.scene())
    objs = js["objects"]
    a = next(i for i in range(1, len(objs) - 1) if "cube" in objs[i]["type"] and objs[i - 1]["transform"] == objs[i + 1]["transform"])
    cams = []
    images = []
    for swap in (False, True):
        if swap:
            objs[a - 1], objs[a + 1] = objs[a + 1], objs[a - 1]
        hs = rtc.HostScene(json.dumps(js))
        cam = hs.camera(*case.world.size)
        cams.append(cam)
        images.append(ob.OracleScene(hs.desc).render(cam, DEPTH)[0])
    assert np.abs(images[0] - images[1]).max() > 1e-2


# ---------------------------------------------------------------- accesses outside the tables (diagnostic build)
OOB_LINE = re.compile(r"^rtc out of bounds:(.*)$", re.M)


def _oob_counts(text):
    """[{kind: count}] of every `rtc out of bounds:` line rtc_get_stats printed (RTC_PROFILE builds, RTC_PROFILE_DUMP)."""
    return [{k: int(v) for k, v in re.findall(r"([a-z-]+) (\d+)", m)} for m in OOB_LINE.findall(text)]


_PROFILE_BUILD = []


def _is_profile_build(rtc, capfd):
    if not _PROFILE_BUILD:
        hs = rtc.HostScene(World(spheres=2, planes=1, materials=3, patterns=3).scene())
        gpu = rtc.GpuScene(hs.desc)
        gpu.render(hs.camera(8, 8), 1)
        capfd.readouterr()
        gpu.stats()
        _PROFILE_BUILD.append(bool(_oob_counts(capfd.readouterr().err)))
        gpu.close()
    return _PROFILE_BUILD[0]


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_no_access_out_of_bounds(rtc, case, capfd, monkeypatch):
    """Every case's launches on the diagnostic build: no table, staging copy, pending-ray slot or canvas access outside
    its allocation (each is counted there instead of made)."""
    monkeypatch.setenv("RTC_PROFILE_DUMP", "1")
    if not _is_profile_build(rtc, capfd):
        pytest.skip("the loaded library is not an RTC_PROFILE build: no out-of-bounds counts to read")
    hs = _host_scene(rtc, case)
    cam = hs.camera(*case.world.size)
    for opts, kernel in zip(case.options, case.kernels()):
        opts.apply(rtc)
        try:
            gpu = rtc.GpuScene(hs.desc)
            for launch in (1, 2):
                gpu.render(cam, DEPTH)
                capfd.readouterr()
                gpu.stats()
                counts = _oob_counts(capfd.readouterr().err)
                assert gpu.last_kernel_name() == kernel
                assert counts and all(v == 0 for c in counts for v in c.values()), (case.name, opts.label(), launch, counts)
            gpu.close()
        finally:
            Options.reset(rtc)
