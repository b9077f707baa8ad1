"""Host side of the cosine / inner-product metrics (RPT_KNN_METRIC_COSINE / _INNER): the Python
distance functions metricCosine / metricInner against an independent restatement and the oracle's
pinned innerDD, the header's flags and the ctypes table's new entry point.  No GPU needed."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rptree_hip.h")


@pytest.fixture(scope="module")
def rp():
    import rptree_amd
    return rptree_amd


def fold(a, b):
    """((0 + a0 b0) + a1 b1) + ... in Python floats (IEEE double, no FMA)"""
    acc = 0.0
    for x, y in zip(a, b):
        acc = acc + float(x) * float(y)
    return acc


def cosine_ref(a, b):
    den = math.sqrt(fold(a, a)) * math.sqrt(fold(b, b))
    num = fold(a, b)
    if den == 0.0:                      # 0 / 0 (or x / 0): IEEE gives NaN / inf, Python raises
        return math.nan if num == 0.0 or num != num else 1.0 - math.copysign(math.inf, num)
    return 1.0 - num / den


def bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def vectors():
    rng = np.random.default_rng(11)
    out = [
        (rng.standard_normal(7), rng.standard_normal(7)),
        (rng.standard_normal(130) * 1e3, rng.standard_normal(130) * 1e-3),
        (np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0, 3.0])),          # cosine of a row with itself
        (np.array([1e308, 1e308]), np.array([1.0, -1.0])),              # the fold, not a rescaled sum
        (np.array([1.0, 1e16, -1e16]), np.array([1.0, 1.0, 1.0])),      # order matters: 0.0, not 1.0
        (np.array([-0.0, -0.0]), np.array([1.0, 1.0])),                  # fold from +0.0
        (np.array([0.0, -0.0, 2.5]), np.array([-0.0, 3.0, -1.0])),
    ]
    return out


def test_metric_inner_is_the_negated_left_fold(rp):
    for a, b in vectors():
        want = -fold(a, b)
        assert bits(rp.metricInner(a, b)) == bits(want)
        assert rp.metricInner(rp.DVector(a), rp.DVector(b)) == rp.metricInner(a, b)


def test_metric_cosine_definition(rp):
    for a, b in vectors():
        want = cosine_ref(a, b)
        got = rp.metricCosine(a, b)
        assert bits(got) == bits(want) or (math.isnan(got) and math.isnan(want)), (a, b, got, want)
    # exact value of the parenthesisation 1 - dot / (sqrt(xx) * sqrt(qq))
    a, b = np.array([3.0, 4.0]), np.array([4.0, 3.0])
    assert rp.metricCosine(a, b) == 1.0 - 24.0 / (5.0 * 5.0)


def test_zero_and_nan_vectors_give_nan(rp):
    z = np.zeros(5)
    x = np.arange(1.0, 6.0)
    assert math.isnan(rp.metricCosine(z, x))
    assert math.isnan(rp.metricCosine(x, z))
    assert math.isnan(rp.metricCosine(z, z))
    assert bits(rp.metricInner(z, x)) == bits(-0.0)           # -(+0.0)
    nq = x.copy()
    nq[2] = np.nan
    assert math.isnan(rp.metricCosine(x, nq)) and math.isnan(rp.metricInner(x, nq))


def test_f32_and_bf16_inputs_are_widened_exactly(rp):
    rng = np.random.default_rng(5)
    a32 = rng.standard_normal(64).astype(np.float32)
    b32 = rng.standard_normal(64).astype(np.float32)
    a64, b64 = a32.astype(np.float64), b32.astype(np.float64)
    assert bits(rp.metricInner(a32, b32)) == bits(-fold(a64, b64))
    assert bits(rp.metricCosine(a32, b32)) == bits(cosine_ref(a64, b64))
    # bf16 rows are given by their values (from_bf16): the same widening
    ab = rp.from_bf16(rp.to_bf16(a32))
    bb = rp.from_bf16(rp.to_bf16(b32))
    assert bits(rp.metricInner(ab, bb)) == bits(-fold(ab.astype(np.float64), bb.astype(np.float64)))
    assert bits(rp.metricCosine(ab, bb)) == bits(cosine_ref(ab.astype(np.float64), bb.astype(np.float64)))
    # f32 products are NOT rounded to f32: the f64 fold differs from an f32 one here
    f32fold = np.float32(0.0)
    for x, y in zip(a32, b32):
        f32fold = np.float32(f32fold + x * y)
    assert -fold(a64, b64) != -float(f32fold)


def test_the_dot_is_the_oracles_inner_dd(rp, oracle):
    rng = np.random.default_rng(9)
    for d in (1, 7, 48, 128, 1000):
        a, b = rng.standard_normal(d) * 10.0 ** rng.integers(-3, 4), rng.standard_normal(d)
        assert bits(rp.metricInner(a, b)) == bits(-oracle.inner_dd(a, b))
        den = np.float64(math.sqrt(oracle.inner_dd(a, a))) * np.float64(math.sqrt(oracle.inner_dd(b, b)))
        assert bits(rp.metricCosine(a, b)) == bits(1.0 - np.float64(oracle.inner_dd(a, b)) / den)
    for a, b in vectors():
        assert bits(rp.metricInner(a, b)) == bits(-oracle.inner_dd(a, b))


def test_header_defines_the_metric_flags(rp):
    src = open(HEADER).read()
    assert re.search(r"#define RPT_KNN_METRIC_COSINE \(1 << 25\)", src)
    assert re.search(r"#define RPT_KNN_METRIC_INNER \(1 << 26\)", src)
    assert re.search(r"int32_t rpt_brute_knn_metric_host\(", src)
    assert rp.RPT_KNN_METRIC_COSINE == 1 << 25 and rp.RPT_KNN_METRIC_INNER == 1 << 26


def test_ctypes_table_has_the_metric_brute_force():
    from rptree_amd import _lib
    assert "rpt_brute_knn_metric_host" in _lib.SYMBOLS
    assert _lib.RPT_KNN_METRIC_COSINE == 1 << 25 and _lib.RPT_KNN_METRIC_INNER == 1 << 26


def test_distf_tokens_and_knnH(rp):
    # knnH has no flags: only metricL2
    with pytest.raises(NotImplementedError):
        rp.knnH(rp.metricCosine, 3, None, None)
    with pytest.raises(NotImplementedError):
        rp.knnH(rp.metricInner, 3, None, None)
    # an arbitrary closure cannot run on the device
    with pytest.raises(NotImplementedError):
        rp.knn(lambda x, q: 0.0, 3, None, None)
    assert rp._metric_flag(None) == 0 and rp._metric_flag(rp.metricL2) == 0
    assert rp._metric_flag(rp.metricCosine) == rp.RPT_KNN_METRIC_COSINE
    assert rp._metric_flag(rp.metricInner) == rp.RPT_KNN_METRIC_INNER


def test_cpp_mirror_metric_example_compiles(tmp_path):
    """knn(..., Metric::Cosine) of the C++ mirror builds against the library (run on the GPU by
    tests/test_gpu_knn_metrics.py)"""
    import subprocess
    lib = os.path.join(ROOT, "rp-tree_amd")
    if not os.path.exists(os.path.join(lib, "librptree_hip.so")):
        subprocess.check_call(["make", "-C", lib], stdout=subprocess.DEVNULL)
    exe = str(tmp_path / "example_metric")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(lib, "host", "example_metric.cpp"), "-L" + lib, "-lrptree_hip",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
