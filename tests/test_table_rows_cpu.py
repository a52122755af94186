"""CPU: the guard that keeps the table offsets of the first batched-affine level in 32 bits (csrc/msm_limits.hpp, used by plan_for in
csrc/msm_host.hpp), compiled for the host.  Rows of the base fields are 256 bytes, 16 uint4s: the levels are dropped exactly when
W * n * 16 reaches 2^32."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("row_limits") / "row_limits_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), os.path.join(ROOT, "tools", "host_tests", "row_limits_check.cpp")], check=True, timeout=300)
    return str(exe)


def fits(checker, row_quads, rows):
    out = subprocess.run([checker, str(row_quads)] + [str(r) for r in rows], capture_output=True, text=True, timeout=60, check=True)
    got = [line.split() for line in out.stdout.splitlines()]
    assert [int(g[0]) for g in got] == list(rows)
    return [g[1] == "1" for g in got]


def windows(c):
    return (754 + c - 1) // c


def test_levels_dropped_exactly_at_2_pow_32(checker):
    edge = 1 << 28                                          # rows at which rows * 16 == 2^32
    rows = [1, 4097 * windows(18), edge - 2, edge - 1, edge, edge + 1, 2 * edge, (1 << 31) - 2, 1 << 40, (1 << 60) + 5]
    assert fits(checker, 16, rows) == [r * 16 < (1 << 32) for r in rows]
    assert fits(checker, 16, [edge - 1, edge]) == [True, False]


def test_the_prover_sets_keep_their_levels(checker):
    """2^20 G1 points at 19-bit windows (the benchmark), H | L | B1 with 3 * 2^20 points at 20 / 21 / 22 bits, the 2^15 + 1 points of
    MNT6753: all far inside; 2^23 points are past it at every width the plan picks (the accumulate kernel alone takes them)."""
    sets = [(1 << 20) * windows(19), 3 * (1 << 20) * windows(20), 3 * (1 << 20) * windows(21), 3 * (1 << 20) * windows(22), ((1 << 15) + 1) * windows(18)]
    assert all(fits(checker, 16, sets))
    assert not any(fits(checker, 16, [(1 << 23) * windows(c) for c in (20, 21, 22)]))


def test_other_row_widths(checker):
    """the helper is generic in the row width: 14 uint4s (packed 224-byte rows) moves the edge to ceil(2^32 / 14) rows"""
    edge = -(-(1 << 32) // 14)
    assert fits(checker, 14, [edge - 1, edge]) == [True, False]
