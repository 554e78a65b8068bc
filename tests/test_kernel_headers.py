"""The device code of ptss_kernels.hip sits in layer headers, and every kernel's bit of ptss_launched_kernels comes from
one table. Checked here without a GPU: (a) each layer header compiles on its own — no header leans on something a translation unit
happened to include before it; (b) the PTSS_KERNEL_* constants of include/ptss_types.h equal ptss_types.KERNEL_BITS, and the ranges
are disjoint and inside the 64-bit word; (c) the names ptss.py gives the bits map one-to-one onto the owned bits, and a bit no kernel
owns names nothing."""
import os
import re
import shutil
import subprocess

import pytest

import ptss
import ptss_types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cuda-path-tracer-ss_amd", "csrc")
LAYER_HEADERS = ("ptwave.h", "ptraypool.h", "ptprim.h", "ptaccel.h", "pthit.h", "ptshade.h")
FREE_BITS = (36, 37, 38, 39, 61, 62, 63)


def _compiles_alone(header, tmp_path):
    src = tmp_path / "one.hip"
    src.write_text('#include "%s"\n' % header)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "-std=c++17", "-fsyntax-only", "--cuda-device-only", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function",
                        "-I", os.path.join(ROOT, "include"), "-I", CSRC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("header", LAYER_HEADERS)
def test_layer_header_compiles_alone(header, tmp_path):
    _compiles_alone(header, tmp_path)


def test_film_header_compiles_alone(tmp_path):
    """ptfilm.h, what the three film kernel files share, is no layer (it sits on ptwave.h and ptdenoise.h) but private in the same way."""
    _compiles_alone("ptfilm.h", tmp_path)


def test_layer_headers_include_only_earlier_layers():
    for i, header in enumerate(LAYER_HEADERS):
        included = re.findall(r'^#include "(\w+\.h)"', open(os.path.join(CSRC, header)).read(), re.M)
        later = [h for h in included if h in LAYER_HEADERS[i:]]
        assert not later, (header, later)


def _header_constants():
    text = open(os.path.join(ROOT, "include", "ptss_types.h")).read()
    found = {name: int(value) for name, value in re.findall(r"\bPTSS_KERNEL_(\w+) = (\d+)", text)}
    widths = {name[len("WIDTH_"):]: v for name, v in found.items() if name.startswith("WIDTH_")}
    bases = {name: v for name, v in found.items() if not name.startswith("WIDTH_")}
    return bases, widths


def test_kernel_bit_table_matches_the_header():
    bases, widths = _header_constants()
    assert bases == {name: base for name, (base, _) in ptss_types.KERNEL_BITS.items()}
    assert widths == {name: width for name, (_, width) in ptss_types.KERNEL_BITS.items()}
    assert bases == {"BOUNCE": 0, "FRAME": 32, "BOUNCE_MESH": 40, "QUERY": 48, "FEATURES": 52, "DENOISE": 54, "UPDATE": 55, "REFIT": 56,
                     "REPROJECT": 57, "FEATURES_MOTION": 58, "REPROJECT_MOTION": 60}
    owned = [base + j for base, width in ptss_types.KERNEL_BITS.values() for j in range(width)]
    assert len(owned) == len(set(owned))          # pairwise disjoint
    assert min(owned) >= 0 and max(owned) < 64
    assert sorted(set(range(64)) - set(owned)) == list(FREE_BITS)


def test_every_owned_bit_names_exactly_one_kernel():
    names = (ptss.all_kernels() | ptss.mesh_kernels() | ptss.query_kernels() | ptss.feature_kernels() | ptss.reproject_kernels() |
             ptss.motion_kernels() | {("denoise",), ("update",), ("refit",)})
    owned = {base + j for base, width in ptss_types.KERNEL_BITS.values() for j in range(width)}
    decoded = {bit: ptss.decode_launched_kernels(1 << bit) for bit in range(64)}
    for bit in range(64):
        assert len(decoded[bit]) == (1 if bit in owned else 0), (bit, decoded[bit])
    for bit in FREE_BITS:
        assert decoded[bit] == set()
    by_bit = [next(iter(decoded[bit])) for bit in sorted(owned)]
    assert len(set(by_bit)) == len(by_bit) == len(names) and set(by_bit) == names   # one-to-one onto the named kernels
    assert ptss.decode_launched_kernels((1 << 64) - 1) == names
    assert ptss.decode_launched_kernels(0) == set()


def test_kernel_names_keep_their_places():
    """The numbering inside each range, as the launch code computes it (ptss_kernels.hip bounceIndex, launchQuery, launchFeatureKernel)."""
    one = lambda bit: next(iter(ptss.decode_launched_kernels(1 << bit)))
    for v, variant in enumerate(("accel", "bounded+pairs", "bounded", "plain")):
        assert one(32 + v) == ("frame", variant)
        for j in range(8):
            assert one(v * 8 + j) == ("bounce", variant, bool(j & 4), bool(j & 2), bool(j & 1))
    for j in range(8):
        assert one(40 + j) == ("bounce", "mesh", bool(j & 4), bool(j & 2), bool(j & 1))
    assert [one(48 + j) for j in range(4)] == [("query", "closest", False), ("query", "closest", True), ("query", "any", False),
                                               ("query", "any", True)]
    assert [one(b) for b in (52, 53, 54, 55, 56, 57, 58, 59, 60)] == [("features", False), ("features", True), ("denoise",), ("update",),
                                                                     ("refit",), ("reproject",), ("features_motion", False),
                                                                     ("features_motion", True), ("reproject_motion",)]
    assert len(ptss.all_kernels()) == 36 and len(ptss.mesh_kernels()) == 8 and len(ptss.query_kernels()) == 4
    assert len(ptss.feature_kernels()) == 2 and len(ptss.reproject_kernels()) == 1 and len(ptss.motion_kernels()) == 3
