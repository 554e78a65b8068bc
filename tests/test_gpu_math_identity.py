"""csrc/ptmath.h returns the same bits on the device and on the host — shown here by exhaustion, not assumed. The oracle and every
host probe are the g++ build of that header (libptss_host.so, liboracle.so); tests/csrc/math_identity.hip evaluates each function in a
trivial kernel on the GPU under test, copies the results back and compares them word for word with ptss_probe_math /
ptss_probe_quantize / ptss_probe_vector of that g++ build: sin, cos, tan, atan, log, exp, pow(x, kGamma) and the literal tone map for
every one of the 2^32 float32 patterns, pow(x, y) on a grid of every exponent and the special values, the vector layer's fma chains on
a few million structured operands — each in two orders, sorted (a wave holds neighbours: the wave-uniform escapes of ptm::div / ptm::rcp
are taken or not as a whole) and scattered (a wave holds 64 unrelated patterns: the per-lane select). The criterion is equality (a NaN
equals a NaN); there is no tolerance. Controls that must mismatch show that the comparison can fail.

What this covers is the check program's own instantiation of the functions; inlined into the tracer's kernels they are compiled
again, and there the parity tests against the oracle remain the evidence."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "lib", "ptss_identitycheck")

ALL = 2 ** 32
# pow grid (tests/csrc/math_identity.hip powGrid): 2 signs x 256 exponents x 16 mantissas + 18 special patterns; y: + 3 Phong reciprocals
GRID_X = 2 * 256 * 16 + 18
GRID_Y = GRID_X + 3
# vector operands (components()): 2 signs x 256 exponents x 64 mantissas + 6 range ends x 5 offsets x 2 signs, 64 combinations of each
VECTOR_CASES = (2 * 256 * 64 + 6 * 5 * 2) * 64

UNARY = ["sin", "cos", "tan", "atan", "log", "exp", "pow_gamma", "quantize"]
VECTOR = ["dot", "cross", "div_scalar", "madd_scalar", "madd_vector", "rotate", "quat_mul", "normalize_vec3", "normalize_quat", "length"]
EXPECTED = {**{op: ALL for op in UNARY}, "pow_grid": GRID_X * GRID_Y, **{op: VECTOR_CASES for op in VECTOR}}
CONTROLS = {"sin": "control_two_step_reduction", "cos": "control_two_step_reduction", "exp": "control_hardware_exp2",
            "dot": "control_without_fma_chain"}

COLUMN = re.compile(r"^(\w+) (sorted|scattered) checked=(\d+) mismatch=(\d+) first=0x([0-9a-f]+) device=0x([0-9a-f]+) host=0x([0-9a-f]+)$", re.M)
CONTROL = re.compile(r"^(\w+) (control_\w+) checked=(\d+) mismatch=(\d+)$", re.M)


assert GRID_X * GRID_Y < 2 ** 28 and VECTOR_CASES >= 2_000_000


@pytest.mark.parametrize("op", UNARY + ["pow_grid"] + VECTOR)
def test_device_equals_host_bit_for_bit(op):
    r = subprocess.run([CHECK, op, "both"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    columns = {m.group(2): (int(m.group(3)), int(m.group(4))) for m in COLUMN.finditer(r.stdout) if m.group(1) == op}
    assert set(columns) == {"sorted", "scattered"}, r.stdout + r.stderr
    for order, (checked, mismatch) in columns.items():
        assert checked == EXPECTED[op], (op, order, checked)
        assert mismatch == 0, (op, order, r.stdout)
    controls = {m.group(2): (int(m.group(3)), int(m.group(4))) for m in CONTROL.finditer(r.stdout) if m.group(1) == op}
    assert set(controls) == ({CONTROLS[op]} if op in CONTROLS else set()), r.stdout
    for name, (checked, mismatch) in controls.items():
        assert checked > 0 and mismatch > 0, (op, name, "the control never differs: the comparison would be vacuous")
    assert r.returncode == 0, r.stdout + r.stderr
