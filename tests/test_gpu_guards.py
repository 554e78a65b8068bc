"""The helpers whose range guards are proven once instead of paid at every operation — sqrt_rcp behind both
normalize()s, the unguarded reciprocal of a sum of three uniforms and root of one, lightSample, addLambertTerm with and without the
scene's verdict on the light powers, the refraction-index quotient and the Phong exponent's reciprocal — must return the bits of the
guarded forms they replace and of the IEEE operations for every operand. tests/csrc/guards_device.hip compares them on the device
over a few million structured operands (every exponent, mantissas all-zero / all-one / random, both signs, +-0, inf, NaN, denormals,
two ulps either side of every range end), in waves of one kind and in mixed waves."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "lib", "ptss_guardcheck")
LINE = re.compile(r"^(\w+) checked=(\d+) vs_guarded=(\d+) vs_ieee=(\d+) fast_waves=(\d+) escaped_waves=(\d+)$", re.M)
BOTH_PATHS = {"sqrt_rcp", "normalize_vec3", "normalize_quat", "light_sample", "lambert_proven_powers"}   # a guard is left: both sides must run
NEVER_ESCAPES = {"rcp_uniform_sum", "sqrt_uniform", "refraction_index", "phong_exponent"}                # no guard is left
ALWAYS_GUARDED = {"lambert_guarded_powers"}                                                              # the scene's flag is off


def test_rewritten_helpers_equal_the_guarded_forms_and_ieee_on_the_device():
    r = subprocess.run([CHECK], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    rows = {m.group(1): tuple(int(g) for g in m.groups()[1:]) for m in LINE.finditer(r.stdout)}
    assert set(rows) == BOTH_PATHS | NEVER_ESCAPES | ALWAYS_GUARDED, r.stdout + r.stderr
    for name, (checked, vs_guarded, vs_ieee, fast, escaped) in rows.items():
        assert checked > 0 and (vs_guarded, vs_ieee) == (0, 0), (name, rows[name])
        if name in BOTH_PATHS:
            assert fast > 0 and escaped > 0, (name, "one side of the guard never ran: the comparison would be vacuous", rows[name])
        elif name in NEVER_ESCAPES:
            assert escaped == 0, (name, rows[name])
        else:
            assert fast == 0, (name, rows[name])
    total = re.search(r"total_checked=(\d+) total_mismatch=(\d+)", r.stdout)
    assert total and int(total.group(1)) >= 2_000_000 and int(total.group(2)) == 0
    assert r.returncode == 0
