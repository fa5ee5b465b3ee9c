"""CPU-side checks of the device statistics (ommxDebugGetStatsDevice): the word-counting header against a decode per field, the numpy reference of
tests/stats_util.py against the library's host ommDebugGetStats, and the bound between the host's fp32 knownAreaMetric and the fp64 one."""
import os
import subprocess
import numpy as np
import ommtest as ot
import stats_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_counting_header_against_a_decode_per_field(tmp_path):
    """omm_amd/csrc/stats_count.h as plain C++ (tests/native/stats_count_check.cpp): every level 0..12 in both formats, the block at byte offsets 0..17,
    cut into segments of 1, 15, 16, 17 and 16384 bytes; bytes around the block and the unused bits of a single-byte block are set and must not count"""
    exe = str(tmp_path / "stats_count_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "omm_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "stats_count_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", str(13 * 2 * 18 * 5)], r.stdout


def test_numpy_reference_equals_host_stats_on_the_well_formed_rows(product):
    """the table of the GPU test, restricted to the descriptors the host loop may be given (it trusts them): all three index formats"""
    array_data, descs, index, _ = su.table_arrays()
    descs = descs[:su.TABLE_WELL_FORMED]
    baker = product.create_baker()
    try:
        for fmt, dt in su.INDEX_DTYPE.items():
            idx = index.astype(dt)
            ref = su.reference_stats(array_data, descs, idx)
            assert ref["skipped"] == int(((index < -4) | (index >= su.TABLE_WELL_FORMED)).sum())
            st = su.host_stats(product, baker, array_data, descs, idx, fmt)
            assert su.int_fields(st) == ref["fields"], (fmt, su.int_fields(st), ref["fields"])
            assert st.knownAreaMetric == 0.0 and ref["metric"] == 0.0
        # block 0 is referenced three times, block 8 once, block 7 never: the fields are not all zero and unreferenced blocks add nothing
        assert ref["refs"][0] == 3 and ref["refs"][8] == 1 and ref["refs"][7] == 0 and ref["state_counts"][7].sum() == 64
        assert sum(ref["fields"][:4]) == int((ref["refs"].astype(np.int64) * ref["state_counts"].sum(axis=1)).sum())
    finally:
        product.destroy_baker(baker)


def test_reference_counts_only_the_fields_of_the_block():
    """levels 0 and 1 use part of a byte: the set bits above the block's fields are not micro-triangles"""
    data = np.full(4, 0xFF, np.uint8)
    assert su.block_counts(data, 0, 0, 1).tolist() == [0, 1, 0, 0]
    assert su.block_counts(data, 1, 0, 2).tolist() == [0, 0, 0, 1]
    assert su.block_counts(data, 2, 1, 1).tolist() == [0, 4, 0, 0]
    assert su.block_counts(data, 3, 1, 2).tolist() == [0, 0, 0, 4]


def host_metric_fp32(index, counts, areas):
    """collect_stats' knownAreaMetric in its own evaluation order, every operation in fp32: the total in triangle order; the known area of the
    special indices in triangle order; per block the areas of its triangles in triangle order, times the block's known share, blocks ascending"""
    f = np.float32
    total, known = f(0), f(0)
    for a in areas:
        total = f(total + a)
    ref_area = {}
    for e, a in zip(index, areas):
        if e in (-1, -2):
            known = f(known + a)
        elif e >= 0:
            ref_area[e] = f(ref_area[e] + a) if e in ref_area else f(a)
    for e in sorted(ref_area):
        kn, un = int(counts[e][0]) + int(counts[e][1]), int(counts[e][2]) + int(counts[e][3])
        known = f(known + f(f(f(kn) / f(kn + un)) * ref_area[e]))
    return f(known / total)


def test_fp32_metric_stays_within_the_derived_bound_of_the_fp64_one():
    """The tolerance of the GPU tests between the host's knownAreaMetric and the device's, for T triangles: 4 * (T + 4) * 2^-24 absolute.

    Derivation (u = 2^-24, the unit roundoff of fp32; all terms are non-negative, so every partial sum is at most the final one and one rounding of a
    partial sum is an error of at most u times the final sum).  The host's total area is T - 1 fp32 additions: relative error at most (T - 1) u.  Its
    known area takes, over all triangles, at most T additions (into the running known area or into a block's area), then per referenced block one
    product and one more addition, and its known share is one division: with D <= T referenced blocks at most 2 T + 3 roundings relative to the final
    sum where the device has none (it uses the same fp32 known share, so that division is common to both).  The quotient adds one rounding, and the
    metric is at most 1: |host - exact| <= ((T - 1) + (2 T + 3) + 1) u = (3 T + 3) u to first order; 4 (T + 4) u leaves the second-order terms
    (below (3 T u)^2 = 1.3e-7 for T = 2000) and the device's single rounding of its fp64 quotient to fp32 (u / 2) ample room.

    Checked here on random inputs with T = 2000: the fp32 evaluation in the host's order against float64."""
    T, D = 2000, 300
    rng = np.random.default_rng(11)
    bound = su.host_metric_bound(T)
    assert bound == 4.0 * 2004 * 2.0 ** -24
    worst = 0.0
    for trial in range(5):
        areas = (rng.random(T, dtype=np.float32) * np.float32(10.0 ** rng.integers(-4, 1))).astype(np.float32)
        index = rng.integers(-4, D, T)
        counts = rng.integers(0, 4097, (D, 4)).astype(np.uint32)
        counts[counts.sum(axis=1) == 0, 0] = 1
        kf = np.zeros(T, np.float32)
        kf[(index == -1) | (index == -2)] = 1.0
        sel = index >= 0
        share = (counts[:, 0] + counts[:, 1]).astype(np.float32) / counts.sum(axis=1).astype(np.float32)
        kf[sel] = share[index[sel]]
        a64 = areas.astype(np.float64)
        exact = (a64 * kf.astype(np.float64)).sum() / a64.sum()
        host = host_metric_fp32(index.tolist(), counts, areas)
        worst = max(worst, abs(float(host) - exact))
        assert abs(float(host) - exact) <= bound, (trial, float(host), exact, bound)
    print("fp32 vs fp64 knownAreaMetric, T = 2000: worst |difference| %.3g, bound %.3g" % (worst, bound))
