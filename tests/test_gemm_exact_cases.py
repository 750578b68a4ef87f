"""The exact GEMM tests' operands and case table (tests/gemm_exact_cases.py)
-- CPU only.

Classes: for every operand class and family the numpy model of the kernel's
split reproduces the fp64 product exactly, the family drops nothing, the sum
of |terms| of any output stays below 2^24 (so fp32 accumulation is exact in
every order) and the class lights up the plane products it is named for.

Coverage: the case table of tests/test_gpu_gemm_exact.py, evaluated through
the host plan checker (tests/gemm_plan_check.cpp --variant), reaches all 48
instantiations of k_gemm_x3 and all 48 of k_gemm_x6 (4 layouts x ragged x
A + A2 x {tile 128, tile 256 general, tile 256 lean}), the four layouts of
the fp32 kernel, and every edge case lands on the plan property it is named
for.  When the planner's thresholds move, this test says which shape to fix.
"""
import os
import subprocess

import numpy as np
import pytest

import gemm_exact_cases as gx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gemm_plan_check.cpp")

# the shapes the classes are used at: the variant matrix's, the longest K, the
# K_dev form and the largest multi-item shape's K
CLASS_SHAPES = [(160, 96, 72), (301, 323, 1023), (64, 48, 4224), (40, 56, 1), (96, 64, 144)]


@pytest.mark.parametrize("a2", [0, 1])
@pytest.mark.parametrize("family,cls", [(f, c) for f in ("x6", "x3") for c in gx.FAMILY_CLASSES[f]])
def test_class_is_exact(family, cls, a2):
    for (M, N, K) in CLASS_SHAPES:
        A, A2, B = gx.operands(cls, M, N, K, seed=3, a2=bool(a2))
        As = A if A2 is None else A + A2  # the kernel's fp32 sum
        assert np.array_equal(As.astype(np.float64), A.astype(np.float64) + (0 if A2 is None else A2)), "A + A2 inexact"
        assert np.array_equal(As, np.rint(As)) and np.array_equal(B, np.rint(B))
        p = gx.kept_products(As, B, family)
        ref = gx.reference(A, A2, B)
        assert np.array_equal(p.model, ref), (cls, M, N, K)
        assert p.dropped == 0.0, (cls, M, N, K, p.dropped)
        assert p.abs_sum < 2.0 ** 24, (cls, M, N, K, np.log2(p.abs_sum))
        if K >= 72:
            lit = gx.CLASSES[cls][4]
            assert all(p.active[name] for name in lit), (cls, M, N, K, p.active)
        print(f"{family} {cls} a2={a2} {M}x{N}x{K}: log2 sum|terms| {np.log2(max(p.abs_sum, 1)):.2f} "
              f"active {[k for k, v in p.active.items() if v]}")


def test_classes_cover_every_kept_product():
    for family in ("x6", "x3"):
        lit = set()
        for cls in gx.FAMILY_CLASSES[family]:
            A, _, B = gx.operands(cls, 160, 96, 72, seed=3)
            lit |= {k for k, v in gx.kept_products(A, B, family).active.items() if v}
        assert lit == {f"{a}*{b}" for a, b in gx.KEPT[family]}, (family, lit)


def test_x3_must_not_get_19_bit_operands():
    """The contrast: 19-bit operands leave x3 a split residue, so x3 drops a
    non-zero term there (and the class would not be exact for it)."""
    A, _, B = gx.operands("a19", 160, 96, 72, seed=3)
    assert gx.kept_products(A, B, "x3").dropped > 0


def test_split_models():
    rng = np.random.default_rng(0)
    x = (rng.normal(size=4096) * 10.0 ** rng.integers(-6, 6, size=4096)).astype(np.float32)
    hi, mid, lo, res = gx.split3(x)
    assert not res.any()  # the three-way split of an fp32 is exact
    assert np.array_equal(hi.astype(np.float64) + mid + lo, x.astype(np.float64))
    for p in (hi, mid, lo):
        assert not (p.view(np.uint32) & 0xFFFF).any()
    h2, l2, r2 = gx.split2(x)
    assert np.array_equal(h2, hi) and np.all(np.abs(r2) <= np.abs(x) * 2.0 ** -16)
    # round to nearest even at the tie: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert gx.bf16(np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8])).tolist() == [1.0, 1 + 2.0 ** -6]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(cc):
        pytest.skip("hipcc not present")
    exe = str(tmp_path_factory.mktemp("gemm_variant") / "gemm_plan_check")
    subprocess.check_call([cc, "-std=c++17", "-O1", SRC, "-o", exe])
    args = [str(v) for c in gx.CASES for v in gx.checker_args(c)]
    lines = subprocess.check_output([exe, "--variant"] + args, text=True).splitlines()
    assert len(lines) == len(gx.CASES)
    return [gx.Plan(*(int(v) for v in ln.split())) for ln in lines]


@pytest.mark.parametrize("prec", [1, 2])
def test_matrix_reaches_all_48_instantiations(plans, prec):
    got = {}
    for c, p in zip(gx.CASES, plans):
        if c.prec == prec and c.group == "matrix":
            got.setdefault((p.tile, p.gen, p.at, p.bt, p.ragged, p.a2), []).append(c)
    want = {(t, g, at, bt, rg, a2) for (t, g) in ((128, 1), (256, 1), (256, 0)) for at, bt in gx.LAYOUTS
            for rg in (0, 1) for a2 in (0, 1)}
    print(f"{gx.FAMILY[prec]}: {len(set(got) & want)}/48 variant tuples")
    assert set(got) == want, sorted(want - set(got))
    assert all(len(v) == 1 for v in got.values())  # one id per instantiation


def test_fp32_layouts(plans):
    got = {(p.at, p.bt, c.m_dev is not None) for c, p in zip(gx.CASES, plans) if c.prec == 0}
    print(f"fp32: {len({g[:2] for g in got})} layouts")
    assert got == {(at, bt, d) for at, bt in gx.LAYOUTS for d in (False, True)}


def test_every_case_hits_its_plan_property(plans):
    seen = set()
    for c, p in zip(gx.CASES, plans):
        for name in c.want:
            assert gx.PROPERTIES[name](c, p), (name, c, p)
            seen.add((c.prec, name))
    # every named edge is in the table for both families
    for prec in (1, 2):
        for name in ("empty_slice", "multi_item", "dev_m_whole", "kdev", f"steps{prec}", "split", "lean", "tile128"):
            assert (prec, name) in seen, (prec, name)
    print(f"{len(gx.CASES)} cases, {len(seen)} (family, property) pairs hit")


def test_edge_plans_in_detail(plans):
    by = {}
    for c, p in zip(gx.CASES, plans):
        by.setdefault((c.group, c.prec), []).append((c, p))
    # the split-K shape: S = 32 with empty trailing slices, as worked out by hand
    (c, p), = [cp for cp in by[("splitk", 2)] if (cp[0].at, cp[0].bt) == (0, 0)]
    assert (p.ns, p.S, p.kstep) == (264, 32, 9)
    (c, p), = [cp for cp in by[("splitk", 1)] if (cp[0].at, cp[0].bt) == (0, 0)]
    assert (p.ns, p.S, p.kstep) == (132, 32, 5)
    # multi-item: 576 tiles on 288 workgroups, 289 tiles on 152
    for prec in (1, 2):
        assert {(p.tile, p.tiles, p.active) for c, p in by[("multi", prec)]} == {(128, 576, 288), (256, 289, 152)}
        # the live-row sweeps see 0, 1 and 2 M tiles and every count of live 32-row blocks
        assert {p.tiles for c, p in by[("live256", prec)]} == {0, 2, 4}
        assert {p.tiles for c, p in by[("live128", prec)]} == {0, 1, 2}
        # device M on the split shape: the device plan splits at every M, within the host's workspace
        for c, p in by[("splitk_mdev", prec)]:
            assert p.mode == 1 and p.S * c.M * c.N * 4 + 256 <= _ws(c), (c, p)
    # K steps: one step, two steps, odd and even counts (the clamped look-ahead)
    assert sorted({p.ns for c, p in by[("ksteps", 2)]}) == [1, 2, 3]
    assert sorted({p.ns for c, p in by[("ksteps", 1)]}) == [1, 2, 3]
    assert {p.ns for c, p in by[("kdev", 2)]} == {0, 1, 5}
    assert {p.ns for c, p in by[("kdev", 1)]} == {0, 1, 3}


def _ws(c):
    # gemm_workspace_bytes for a split shape: the largest S (32) of any effective M
    return (32 * c.M * c.N * 4 + 255) // 256 * 256 + 256
