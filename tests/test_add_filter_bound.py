"""The window of the ADD-S filtered search (csrc/average_distance.hip), pinned
on the CPU: the numpy emulation of the bf16 filter on the LOV models of the two
symmetric classes must keep the reference's fp32 first-minimum pick of every
query point inside the derived window, for random, near-correct and
unnormalised predictions.  The candidates inside the window per query are
recorded (printed and attached as a property): they are the filter's cost,
not a pass criterion."""
import numpy as np
import pytest

from posecnn_amd import synth

import add_filter_ref as ref


@pytest.mark.parametrize("cls", [16, 21])
@pytest.mark.parametrize("kind", ["random", "near", "scale1e-3", "scale3"])
def test_filter_window_holds_the_fp32_pick(cls, kind, record_property):
    pts, sym = synth.rescaled_points(22)
    assert sym[cls] > 0
    rng = np.random.default_rng(cls * 7 + len(kind))
    qt = rng.normal(size=4)
    qt /= np.linalg.norm(qt)
    if kind == "near":
        qp = qt + 0.02 * rng.normal(size=4)
        qp /= np.linalg.norm(qp)
    else:
        qp = rng.normal(size=4)
        qp *= {"random": 1.0 / np.linalg.norm(qp), "scale1e-3": 1e-3, "scale3": 3.0}[kind]
    q, c = ref.clouds(qp.astype(np.float32), qt.astype(np.float32), pts[cls])
    ok, inside, mean_hits, max_hits = ref.filter_verdict(q, c)
    print(f"class {cls} {kind}: candidates inside the window per query: mean {mean_hits:.2f}, max {max_hits}")
    record_property("hits_per_query_mean", mean_hits)
    record_property("hits_per_query_max", max_hits)
    assert ok, "clouds outside the range the window is proved for"
    assert inside, "an fp32 first-minimum pick fell outside the filter's window"


def test_filter_emulation_error_is_inside_the_bound():
    """|s~ - s| against a float64 evaluation stays below the derivation's (a) = 6.8e-5 M^2."""
    pts, _ = synth.rescaled_points(22)
    rng = np.random.default_rng(5)
    qt, qp = rng.normal(size=4), rng.normal(size=4)
    q, c = ref.clouds((qp / np.linalg.norm(qp)).astype(np.float32), (qt / np.linalg.norm(qt)).astype(np.float32),
                      pts[16][:700])
    s, win, ok = ref.filter_emulation(q, c)
    q64, c64 = q.astype(np.float64), c.astype(np.float64)
    exact = (c64 * c64).sum(1)[None, :] - 2.0 * q64 @ c64.T
    m2 = max((q64 * q64).sum(1).max(), (c64 * c64).sum(1).max())
    assert ok and np.abs(s - exact).max() <= 6.8e-5 * m2
    assert win >= 2 * (6.8e-5 + 1.2e-6) * m2


def test_emulation_constants_are_the_kernels():
    """The helper's window and range are the ones compiled into the kernel."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "posecnn_amd", "csrc",
                            "average_distance.hip")).read()
    win = float(re.search(r"kFiltWin = ([0-9.e+-]+)f;", src).group(1))
    lo, hi = re.search(r"kFiltM2Min = 0x1p(-?\d+)f, kFiltM2Max = 0x1p(-?\d+)f;", src).groups()
    assert win == ref.FILT_WIN and 2.0 ** int(lo) == ref.FILT_M2_MIN and 2.0 ** int(hi) == ref.FILT_M2_MAX
