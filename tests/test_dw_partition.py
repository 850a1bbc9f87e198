"""The workgroup partition of the job-parallel weight gradients (neddf_amd/csrc/train_kernels.h dw_partition) on the CPU.  The
launch gives every weight-gradient product of a backward pass a contiguous range of workgroups, in proportion to the product's cost;
a product whose range came out empty would leave its weight gradient silently at zero.  A stand-alone driver
(tests/capi/dw_partition.cpp) runs the function under AddressSanitizer + UBSan over every machine size and job list below, with the
cost tables of both operand policies, and the result is held to the invariants and to a float32 restatement of the rule."""
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

CUS = (1, 2, 8, 64, 256, 304)
MAX_JOBS = 32
F32, SPLIT = 0, 1


def cost(table, K):
    if table == F32:
        return np.float32(64.0) + np.float32(64 if K <= 64 else 96 if K <= 96 else 256)
    return np.float32(226.0 if K <= 64 else 258.0 if K <= 96 else 346.0)


def partition(table, cus, Ks):
    """The rule in float32, one rounding per operation: share = (int)(cost / total * grid + 0.5), at least 1, at most what leaves one
    workgroup for every job still to come"""
    c = [cost(table, K) for K in Ks]
    total = np.float32(0.0)
    for x in c:
        total = np.float32(total + x)
    n = len(Ks)
    grid, at, wg0 = max(cus, n), 0, []
    for i in range(n):
        wg0.append(at)
        share = int(np.float32(np.float32(np.float32(c[i] / total) * np.float32(grid)) + np.float32(0.5)))
        share = max(share, 1)
        left = n - 1 - i
        if at + share > grid - left:
            share = grid - left - at
        at += share
    return at, wg0


def job_lists():
    """job counts 1..32: all narrow, all middle, all wide, and three seeded draws from {48, 96, 256} each"""
    rng = np.random.default_rng(12)
    for n in range(1, MAX_JOBS + 1):
        for K in (48, 96, 256):
            yield [K] * n
        for _ in range(3):
            yield [int(K) for K in rng.choice((48, 96, 256), size=n)]


@pytest.fixture(scope="module")
def partitions(tmp_path_factory):
    """[(table, cus, Ks, grid, wg0)]: one compile, one run of the driver"""
    tmp = tmp_path_factory.mktemp("dwpart")
    csrc = os.path.join(ROOT, "neddf_amd", "csrc")
    exe, case_file = str(tmp / "dw_partition"), str(tmp / "cases.txt")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                           "-I", csrc, "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "capi", "dw_partition.cpp"), "-o", exe])
    cases = [(table, cus, Ks) for table in (F32, SPLIT) for cus in CUS for Ks in job_lists()]
    with open(case_file, "w") as f:
        for table, cus, Ks in cases:
            f.write("%d %d %d %s\n" % (table, cus, len(Ks), " ".join(map(str, Ks))))
    p = subprocess.run([exe, case_file], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and not any(s in p.stderr for s in ("Sanitizer", "runtime error")), p.stderr[-4000:]
    lines = p.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    out = []
    for (table, cus, Ks), line in zip(cases, lines):
        v = [int(x) for x in line.split()]
        assert len(v) == 1 + len(Ks)
        out.append((table, cus, Ks, v[0], v[1:]))
    return out


def test_sweep_covers_both_tables_every_machine_size_and_job_count(partitions):
    assert {(t, c, len(K)) for t, c, K, _, _ in partitions} == {(t, c, n) for t in (F32, SPLIT) for c in CUS for n in range(1, MAX_JOBS + 1)}
    for Kall in (48, 96, 256):
        assert {len(K) for _, _, K, _, _ in partitions if set(K) == {Kall}} == set(range(1, MAX_JOBS + 1))
    assert any(len(set(K)) == 3 for _, _, K, _, _ in partitions)


def test_every_job_gets_a_workgroup_and_the_grid_stays_in_bounds(partitions):
    for table, cus, Ks, grid, wg0 in partitions:
        what = "table %d, cus %d, K %s: grid %d, wg0 %s" % (table, cus, Ks, grid, wg0)
        n = len(Ks)
        assert wg0[0] == 0, what
        assert all(b > a for a, b in zip(wg0, wg0[1:])), what           # strictly increasing: every job but the last has >= 1 workgroup
        assert grid > wg0[-1], what                                      # ... and so has the last
        assert n <= grid <= max(cus, n), what


def test_partition_equals_the_float32_rule(partitions):
    for table, cus, Ks, grid, wg0 in partitions:
        assert (grid, wg0) == partition(table, cus, Ks), "table %d, cus %d, K %s" % (table, cus, Ks)
