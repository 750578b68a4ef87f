"""The GEMM launch planner (csrc/gemm_plan.h: plan_launch) -- CPU only.

A stand-alone host program (tests/gemm_plan_check.cpp) includes the planner's
header, makes no GPU call and prints the plan of the step's FC shapes; the
rows below were worked out from the launch logic as it stood before the
planner was factored out (the tile edge, the largest grid or the fewest
workgroups that keep the rounds, the lean whole-tile kernel, whether any
effective M splits K, the non-temporal C store).  Precisions 1 and 2 share
them.  pcnn_gemm_workspace_size of the built library must agree."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gemm_plan_check.cpp")

# name: (M, N, K, M on device) -> (tile, grid, gen, may_split, c_stream, workspace bytes)
PLANS = {
    "fc6 fwd": ((1152, 4096, 25088, 1), (256, 256, 1, 1, 0, 301990144)),
    "fc7 fwd / fc7 dX": ((1152, 4096, 4096, 1), (256, 256, 1, 1, 0, 301990144)),
    "fc8 fwd": ((1152, 88, 4096, 1), (128, 512, 1, 1, 0, 12976384)),
    "fc8 dX": ((1152, 4096, 88, 1), (128, 512, 1, 0, 0, 256)),
    "fc6 dX": ((1152, 25088, 4096, 1), (256, 256, 1, 1, 0, 231211264)),
    "fc8 dW": ((4096, 88, 1152, 0), (128, 512, 1, 1, 0, 12976384)),
    "fc7 dW": ((4096, 4096, 1152, 0), (256, 256, 0, 0, 0, 256)),
    "fc6 dW": ((25088, 4096, 1152, 0), (256, 224, 0, 0, 1, 256)),
    "small": ((333, 200, 77, 1), (128, 512, 1, 0, 0, 256)),
    "split": ((300, 520, 2048, 0), (256, 256, 1, 1, 0, 9984256)),
}


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(cc):
        pytest.skip("hipcc not present")
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_check")
    subprocess.check_call([cc, "-std=c++17", "-O1", SRC, "-o", exe])
    return exe


@pytest.mark.parametrize("precision", [1, 2])
def test_plan_of_the_step_shapes(plan_check, precision):
    args = [str(v) for shape, _ in PLANS.values() for v in shape + (precision,)]
    lines = subprocess.check_output([plan_check] + args, text=True).splitlines()
    got = {name: tuple(int(v) for v in ln.split()) for name, ln in zip(PLANS, lines)}
    assert got == {name: want for name, (_, want) in PLANS.items()}


@pytest.mark.parametrize("precision", [1, 2])
def test_library_workspace_size_agrees(precision):
    from posecnn_amd import _lib, build
    if build.needs_build():
        build.build()
    lib = _lib.load()
    for name, ((M, N, K, dyn), want) in PLANS.items():
        assert lib.pcnn_gemm_workspace_size(M, N, K, dyn, precision) == want[5], name
