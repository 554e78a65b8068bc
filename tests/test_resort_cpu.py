"""The kd order restated level by level (csrc/ptorder.h, ptss_probe_kd_order) against the packer's recursive one
(csrc/ptpack.h kdOrder through ptss_probe_pack_scene): the same leaves — for every leaf k the same set of original indices at
positions 16 k .. 16 k + 15 — on meshes of every shape of segment tree and on tables whose centroids tie. No GPU."""
import numpy as np
import pytest

import ptss
from resort_common import flat, identical, lattice_through_zero, leaf_of, packer_positions, point_lit, scatter, table


def check(triangles):
    scene = point_lit(triangles)
    n = len(triangles)
    want = packer_positions(scene)
    got = ptss.probe_kd_order(triangles)
    assert got.dtype == np.int32 and np.array_equal(np.sort(got), np.arange(n)), "not a permutation"
    assert np.array_equal(leaf_of(got), leaf_of(want)), "a leaf holds other triangles than the packer's"
    order = np.empty(n, dtype=np.int64)
    order[got] = np.arange(n)
    starts = np.arange(n) % 16 == 0
    assert np.all((np.diff(order) > 0) | starts[1:]), "original indices must ascend inside a leaf"
    return got, want


# 512: one split of two groups; 513: a ragged last leaf and group of one; 767: left = 512 and a ragged rest; 4097, 5134: more than
# one 256-unit level; 20000: leaves beyond the LDS window
@pytest.mark.parametrize("T", [512, 513, 767, 4097, 5134, 20000])
def test_leaves_equal_the_packers(T):
    t = table(T)
    check(t)
    if T <= 5134:
        check(scatter(t))


def test_all_centroids_identical():
    got, _ = check(identical())
    assert np.array_equal(got, np.arange(len(got)))   # every key ties: the original index decides everywhere


def test_a_mesh_flat_in_one_axis():
    check(flat())


def test_a_lattice_of_ties_through_both_zeros():
    t = lattice_through_zero()
    x = np.concatenate([t[name][:, 0] for name in ("vertex0", "vertex1", "vertex2")])
    assert np.any((x == 0) & np.signbit(x)) and np.any((x == 0) & ~np.signbit(x))
    _, want = check(t)
    # ... and the canonical zero is what makes it so: with codes that keep -0.0 below +0.0 the plane x = 0 is cut elsewhere
    signed = ptss.probe_kd_order(t, signed_zero=True)
    assert np.array_equal(np.sort(signed), np.arange(len(t)))
    assert not np.array_equal(leaf_of(signed), leaf_of(want))
    # without a zero of either sign in the table the two codes agree
    t2 = table(513)
    assert np.array_equal(ptss.probe_kd_order(t2, signed_zero=True), ptss.probe_kd_order(t2))


def test_argument_checks():
    L = ptss.host_lib()
    t = table(512)
    out = np.zeros(512, dtype=np.int32)
    assert L.ptss_probe_kd_order(None, 512, out.ctypes.data_as(ptss.C.POINTER(ptss.C.c_int))) != 0
    assert L.ptss_probe_kd_order(t.ctypes.data, 0, out.ctypes.data_as(ptss.C.POINTER(ptss.C.c_int))) != 0
    assert L.ptss_probe_kd_order(t.ctypes.data, 512, None) != 0
