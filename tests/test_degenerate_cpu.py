"""The scenes of tests/degenerate_scenes.py, checked on the CPU before tests/test_gpu_degenerate.py
renders them: the scalar emulation of the accelerated walk (tests/native/accel_check.cpp over the
product's accel.cpp) agrees with the oracle's reference walk on every one of them, the mutations
change what the rays see, the oracle's frames are not mostly NaN, the accelerator really is built
with bounded and always-tested shapes side by side, and the generator is deterministic.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import degenerate_scenes as dg
import oracle
import test_accel_cpu as ta
import trace_rays as tr
from test_accel_cpu import check_lib  # noqa: F401  (the fixture: accel_check.cpp + accel.cpp)

CASES = [(f, s, d) for f in dg.FAMILIES for s in dg.SEEDS for d in dg.DEPTHS]
IDS = ["%s-s%d-d%d" % c for c in CASES]
# (maxBounces, useBVH, fresnel, mt) of the frames tests/test_gpu_degenerate.py renders
FRAME_PARAMS = ((3, 1, 0, 0), (3, 1, 1, 1), (3, 0, 0, 0), (2, 0, 1, 1))
MIN_CHANGED = 0.01   # share of rays(...) whose answer a family must change
MAX_NONFINITE = 0.05  # share of an oracle frame's pixels that may be non-finite


def emulate(lib, fs, o, d, lim, tree, mt):
    """accel_check: (shape, distance, shadow) of the emulated accelerated walk, and its info words."""
    o, d, lim = (np.ascontiguousarray(a, np.float32) for a in (o, d, lim))
    R = len(o)
    outs = [np.zeros(R, np.int32), np.zeros(R, np.float32), np.zeros(R, np.int32)]
    info = np.zeros(12, np.int32)
    info[8], info[6] = tree, mt
    rc = lib.accel_check(ta._p(fs.shapes), len(fs.shapes), ta._p(fs.nodes), len(fs.nodes), ta._p(fs.indices),
                         len(fs.indices), ta._p(o), ta._p(d), ta._p(lim), R, *[ta._p(x) for x in outs], ta._p(info))
    assert rc == 0, f"accel_check could not build the accelerator (rc {rc})"
    return outs, info


@functools.lru_cache(maxsize=None)
def oracle_answers(family, seed, depth, mt):
    fs = dg.base(seed, depth) if family is None else dg.scene(family, seed, depth)
    return tr.oracle_trace(fs, *dg.rays(family, seed), mt)


def differing(a, b):
    """Rays whose (shape, distance, shadow) differ; NaN distances in the same ray are equal."""
    return (a[0] != b[0]) | (a[2] != b[2]) | ~((a[1] == b[1]) | (np.isnan(a[1]) & np.isnan(b[1])))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_emulation_matches_the_oracle(check_lib, case):  # noqa: F811
    """1. Barycentric and Moller-Trumbore, reference tree and scene tree: shape, distance (NaN ==
    NaN) and shadow answer of every ray."""
    family, seed, depth = case
    fs = dg.scene(family, seed, depth)
    o, d, lim = dg.rays(family, seed)
    for mt in (0, 1):
        want = oracle_answers(family, seed, depth, mt)
        for tree in (0, 1):
            got, _ = emulate(check_lib, fs, o, d, lim, tree, mt)
            bad = np.where(differing(got, want))[0]
            assert bad.size == 0, (f"mt {mt} tree {tree}: {bad.size} rays differ, e.g. ray {bad[0]}: "
                                   f"{[a[bad[0]] for a in got]} vs the oracle's {[a[bad[0]] for a in want]}")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_mutations_change_what_the_rays_see(case):
    """2. Oracle alone: the mutated scene and the base scene differ on at least 1 % of the rays,
    under the barycentric test and (but for the stored planes, which it never reads) under MT."""
    family, seed, depth = case
    for mt in (0, 1):
        share = float(differing(oracle_answers(family, seed, depth, mt), oracle_answers(None, seed, depth, mt)).mean())
        if mt and family in dg.MT_BLIND:
            assert share == 0.0, f"Moller-Trumbore reads the stored plane after all: {share:.4f} of the rays changed"
        else:
            assert share >= MIN_CHANGED, f"mt {mt}: the mutation changes only {share:.4f} of the rays"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_frames_are_not_mostly_nan(case):
    """3. Every oracle frame the GPU test compares against has at most 5 % non-finite pixels."""
    family, seed, depth = case
    fs = dg.scene(family, seed, depth)
    for mb, bvh, fr, mt in FRAME_PARAMS:
        img, _ = oracle.render(fs, dg.W, dg.H, oracle.params(dg.W, dg.H, mb, bvh, fr, mt))
        share = float((~np.isfinite(img)).any(axis=-1).mean())
        assert share <= MAX_NONFINITE, f"params {(mb, bvh, fr, mt)}: {share:.4f} of the pixels are non-finite"


@pytest.mark.parametrize("seed", dg.SEEDS)
@pytest.mark.parametrize("family", dg.FAMILIES)
def test_the_accelerator_is_in_use(check_lib, family, seed):  # noqa: F811
    """4. At depth 1 the leaves are large: local nodes exist, with bounded and always-tested
    shapes below them (the huge scene only has to build)."""
    o, d, lim = (a[:64] for a in dg.rays(family, seed))
    _, info = emulate(check_lib, dg.scene(family, seed, 1), o, d, lim, 1, 0)
    _, base = emulate(check_lib, dg.base(seed, 1), o, d, lim, 1, 0)
    assert base[0] > 0 and base[1] == 2 and base[2] == len(dg.base(seed, 1).shapes) - 2  # the two planes
    if family != "huge":
        assert info[0] > 0 and info[1] > 0 and info[2] > 0, info[:3]
    # every shape has a prim, the ones of unknown type among the always-tested: a refit that gives
    # one a known type rewrites that prim (without it the shape would be missing from the frame)
    assert info[1] + info[2] == len(dg.scene(family, seed, 1).shapes), info[:3]


@pytest.mark.parametrize("seed", dg.SEEDS)
@pytest.mark.parametrize("family", dg.FAMILIES)
def test_every_family_changes_a_class(check_lib, family, seed):  # noqa: F811
    """accel_bound.h::classify of the base record and of the family's record of every mutated
    shape (barycentric; the class does not depend on the tree or on origin_lim): at least one
    differs. So each step of tests/test_gpu_degenerate.py's refit test, which goes from one of the
    two sets of records to the other, changes a class, whichever set the accelerator was built
    from, and must make the host rebuild."""
    check_lib.accel_classes.restype = None
    check_lib.accel_classes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    ids = dg.mutated_ids(family, seed)
    cls = []
    for fs in (dg.base(seed, 1), dg.scene(family, seed, 1)):
        out = np.full(len(fs.shapes), -1, np.int32)
        check_lib.accel_classes(ta._p(fs.shapes), len(fs.shapes), 0, ta._p(out))
        assert set(out.tolist()) <= {0, 1, 2}
        cls.append(out)
    assert set(cls[0][ids].tolist()) <= {0, 1}  # the base has no unknown types
    changed = ids[cls[0][ids] != cls[1][ids]]
    assert changed.size > 0, f"no mutated shape of {family} changes its class: {cls[1][ids].tolist()}"
    rest = np.setdiff1d(np.arange(len(cls[0])), ids)
    assert np.array_equal(cls[0][rest], cls[1][rest])
    if family == "type":
        assert (cls[1][ids] == 2).all()


@pytest.mark.parametrize("family", dg.FAMILIES)
def test_the_generator_is_deterministic(family):
    """5. Two calls give byte-equal records, nodes and indices; the mutated ids are the records that
    differ from the base scene's; the rays are the same for every family."""
    for seed in dg.SEEDS:
        for depth in dg.DEPTHS:
            a, b = dg.scene(family, seed, depth), dg.scene(family, seed, depth)
            assert a.shapes is not b.shapes
            for f in ("shapes", "nodes", "indices", "camera", "light"):
                assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
        base = dg.base(seed, 1).shapes
        raw = lambda s: np.ascontiguousarray(s).view(np.uint8).reshape(len(s), -1)  # noqa: E731
        changed = np.where((raw(a.shapes) != raw(base)).any(axis=1))[0]
        assert np.array_equal(changed, dg.mutated_ids(family, seed))
        for x, y in zip(dg.rays(family, seed), dg.rays(None, seed)):
            assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("seed", dg.SEEDS)
def test_thresholds_fall_on_the_sides_they_claim(seed):
    """The thresholds family, recomputed in double from the float32 records as accel_bound.h
    does: each record's sin^2, stored normal length or cosine is on its side of the rule."""
    s = dg.scene("thresholds", seed, 1).shapes
    ids = dg.mutated_ids("thresholds", seed)
    want = [("sin2", v) for v in dg.SIN2] * 2 + [("len", v) for v in dg.NORMAL_LEN] + [("cos", v) for v in dg.COS] * 2
    # mutated_ids is sorted and the family takes the first triangles in order
    assert len(ids) == len(want)
    for i, (rule, v) in zip(ids, want):
        p1, p2, p3, n = (s[k][i].astype(np.float64) for k in ("triP1", "triP2", "triP3", "planeNormal"))
        cr = np.cross(p2 - p1, p3 - p1)
        sin2 = cr @ cr / ((p2 - p1) @ (p2 - p1) * ((p3 - p1) @ (p3 - p1)))
        nl = np.sqrt(n @ n)
        cos = abs(n @ cr) / (np.sqrt(cr @ cr) * nl)
        got, limit = {"sin2": (sin2, 1e-3), "len": (nl, 1e-6 if v < 1 else 1e6), "cos": (cos, 0.05)}[rule]
        assert (got >= limit) == (v >= limit) and abs(got / v - 1) < 2e-4, (i, rule, v, got)
        if rule != "sin2":
            assert sin2 > 0.1  # only the rule named decides the class
        if rule == "sin2" or rule == "len":
            assert cos > 0.999


def test_frame_helpers_see_what_a_plain_difference_does_not():
    """tests/frame_check.py on an oracle frame that has NaN pixels: a NaN where the oracle has a
    colour (which `diff > tol` and "all finite in both or in neither" let through), a colour
    where it has a NaN, an infinity of the other sign and a value off by more than the tolerance
    all fail; NaN for NaN with another payload and differences within the tolerance pass."""
    from frame_check import close_to_oracle, same_frame
    ref, _ = oracle.render(dg.scene("stored_plane", 2, 1), dg.W, dg.H, oracle.params(dg.W, dg.H, 3, 1, 1, 1))
    nan = np.argwhere(np.isnan(ref))
    fin = np.argwhere(np.isfinite(ref).all(axis=-1))
    assert len(nan) > 0 and len(fin) > 100
    img = ref.copy()
    img.view(np.uint32)[tuple(nan[0])] = 0xFFC00123  # another NaN
    img[tuple(fin[5])] += np.float32(5e-5)
    close_to_oracle(img, ref, 1e-4, "same")
    same_frame(img, img.copy(), "same")

    def fails(fn, *args):
        with pytest.raises(AssertionError):
            fn(*args)

    a = img.copy()
    a[tuple(fin[100])][1] = np.nan
    diff = np.abs(a.astype(np.float64) - ref.astype(np.float64))
    assert not (diff > 1e-4).any() and np.isfinite(a).all() == np.isfinite(ref).all()  # the comparison replaced
    fails(close_to_oracle, a, ref, 1e-4, "NaN where the oracle has none")
    fails(same_frame, a, img, "NaN in one")
    b = img.copy()
    b[tuple(nan[0])] = 0.5
    fails(close_to_oracle, b, ref, 1e-4, "a colour where the oracle has NaN")
    c, r = img.copy(), ref.copy()
    c[tuple(fin[7])][0], r[tuple(fin[7])][0] = np.inf, -np.inf
    fails(close_to_oracle, c, r, 1e-4, "infinities of opposite sign")
    fails(same_frame, c, r, "infinities of opposite sign")
    r[tuple(fin[7])][0] = np.inf
    close_to_oracle(c, r, 1e-4, "the same infinity")
    d = img.copy()
    d[tuple(fin[9])][2] += np.float32(1e-3)
    fails(close_to_oracle, d, ref, 1e-4, "off by 1e-3")
    fails(same_frame, img, ref, "5e-5 apart is not the same frame")
