"""CPU: the input tables of a verification key (mnt753_vk_prepare_inputs) as far as they go without a
device -- the entry points exist and refuse, the plan arithmetic the walk kernel shares with the host (csrc/vk_input_plan.hpp) keeps
every digit of every structured scalar inside its own base's tables at every width and number of inputs, and the Python model of
tests/vk_inputs_ref.py agrees with itself on the index, the slices and the widened keys."""
import ctypes
import os
import subprocess

import pytest

import batch_exp_ref as BR
import msm_structured as S
import oracle_lib as O
import vk_inputs_ref as VR

ROOT = O.ROOT
WIDTHS = range(VR.MIN_W, VR.MAX_W + 1)


def test_entry_points_refuse_bad_arguments(pkg):
    """MNT753_EINVAL before any device is looked for, each with a message; the Python class has the three methods"""
    L = pkg.lib()
    plan = pkg.api.VkInputPlan()
    assert L.mnt753_vk_prepare_inputs(None, 0, 0) == -1 and L.mnt753_last_error()
    assert L.mnt753_vk_input_plan(None, 1, ctypes.byref(plan)) == -1
    assert L.mnt753_vk_release_inputs(None) == -1
    assert ctypes.sizeof(plan) == 32
    for name in ("prepare_inputs", "input_plan", "release_inputs"):
        assert callable(getattr(pkg.VerificationKey, name))


def all_scalars():
    ints = {0, 1}
    for curve in (0, 1):
        r = BR.modulus(curve)
        ints |= set(S.single_bits(curve)) | set(S.edges(curve)) | {r - 1, r, (1 << 768) - 1}      # (an input >= r is walked on its words)
        ints |= {s for _, s in BR.wrap_family(curve)}
        for c in WIDTHS:
            ints |= set(S.extremes(curve, c)) | set(S.carry_chains(curve, c))
            if c <= 8:
                ints |= set(S.dense(curve, c))
    return sorted(ints)


@pytest.fixture(scope="module")
def scalar_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("vk_inputs") / "scalars.bin"
    ints = all_scalars()
    path.write_bytes(b"".join(v.to_bytes(96, "little") for v in ints))
    return str(path), len(ints)


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "asan_ubsan"])
def test_plan_arithmetic_compiled_for_the_host(tmp_path, scalar_file, flags):
    """tools/host_vk_inputs_check.cpp over vk_input_plan.hpp: at every width 2 .. 16, for keys with 1, 2 and 1000 inputs, the digits of
    every structured and wrap scalar name rows inside their own base's part of the table, and the multiples those rows hold, signed,
    sum to the scalar; the default width, the table bytes and the slices at their edges.  Built plain and under ASan + UBSan; the
    program is run directly."""
    path, n = scalar_file
    exe = tmp_path / "host_vk_inputs_check"
    subprocess.run(["g++", "-std=c++17", *flags, "-o", str(exe), os.path.join(ROOT, "tools", "host_vk_inputs_check.cpp")], check=True, timeout=600)
    out = subprocess.run([str(exe), path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and f"ALL OK: {n} scalars" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("w", [2, 3, 8, 14, 16])
def test_model_index_stays_inside_its_base(w):
    """the model's row of every digit of a scalar taken for base p lies in base_rows(p), and the digits sum to the scalar"""
    r = BR.modulus(0)
    for s in (0, 1, r - 1, r, (1 << 753) - 1, BR.wrap_family(0)[0][1]):
        ds = [VR.digit(s, j, w) for j in range(VR.windows(w))]
        assert sum(d << (j * w) for j, d in enumerate(ds)) == s and all(abs(d) <= VR.rows_per_window(w) for d in ds)
        for p in (0, 1, 1000):
            lo, hi = VR.base_rows(p, w)
            for j, d in enumerate(ds):
                if d:
                    row, neg = VR.row_of(p, j, d, w)
                    assert lo <= row < hi and neg == (d < 0)
                    assert (row - lo) // VR.rows_per_window(w) == j and (row - lo) % VR.rows_per_window(w) + 1 == abs(d)


def test_model_plan():
    assert VR.default_window_bits(2) == 14 and VR.default_window_bits(2, 1) == 0 and VR.default_window_bits(2, VR.table_bytes(2, 2)) == 2
    for points in (2, 4, 34, 258, 1025):
        w = VR.default_window_bits(points)
        assert VR.table_bytes(points, w) <= VR.DEFAULT_CAP and (w == VR.MAX_W or VR.table_bytes(points, w + 1) > VR.DEFAULT_CAP)
    assert VR.default_window_bits(1025) == 3 and VR.windows(3) == 252 and VR.windows(2) == 377 and VR.windows(16) == 48
    for k in (1, 2, 3, 33, 257):
        for ipl in (1, 2, max(k - 1, 1), k, k + 3):
            sl = VR.slices(k, ipl)
            assert sl[0][0] == 0 and sl[-1][1] == k and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
            assert all(e - f == ipl for f, e in sl[:-1]) and 0 < sl[-1][1] - sl[-1][0] <= ipl
            assert VR.workspace_per_proof(k, ipl) == 336 * (len(sl) + 1) + 112
        assert VR.inputs_per_lane(1, k) == 1 and VR.inputs_per_lane(65536, k) == k and VR.inputs_per_lane(1 << 20, k) == k
    assert VR.inputs_per_lane(32768, 33) == 17 and VR.inputs_per_lane(257, 257) == 2 and VR.inputs_per_lane(65, 3) == 1


@pytest.mark.parametrize("curve", [0, 1])
def test_widened_rows_combine_to_x(curve):
    r = BR.modulus(curve)
    x = 0x1234_5678_9ABC % r
    for k in (1, 2, 3, 33):
        a = VR.ratios(r, k, k)
        rows = VR.designed_rows(r, a, x, BR.wrap_family(curve))
        assert len(rows) == (5 if k >= 3 else 3)
        for label, row in rows:
            assert len(row) == k and all(0 <= v < r for v in row) and VR.combined(r, a, row) == x, (k, label)
        if k >= 3:
            eq, op = dict(rows)["equal partials"], dict(rows)["opposite partials"]
            assert eq[0] * a[0] % r == eq[1] * a[1] % r and (op[0] * a[0] + op[1] * a[1]) % r == 0
