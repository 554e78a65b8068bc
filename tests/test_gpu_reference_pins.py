"""The product on the GPU against what THE REFERENCE'S OWN CODE answered, recorded as data in tests/golden/reference/ by
tests/golden/make_reference_golden.py on a machine that has the reference (compiled for the CPU: oracle/build.py build_ref). Reads
the fixtures only — never the reference, never oracle/_ref/.

  * ptss_intersect / ptss_occluded on the recorded scene tables and the 4,096 recorded rays per scene against the reference's
    closest hit (the intersection loops of pathTraceKernel, CudaTracer.cu:121-141) and its lineOfSight verdict (:420-455). Decisions
    equal, except the recorded cases a float64 model puts within 4 ulp of a threshold (at most 0.5 %); floats within 3 * e_ref + 1
    ulp, e_ref recorded with them (the rule and the floors: tests/reference_common.py).
  * a 512 x 512, 16-sample, 15-bounce frame of each scene against the recorded 64 x 64 x 3 block means of the reference's frame:
    channel means within 1.5 %, block correlation above 0.995 (the yardstick of tests/test_oracle_libm.py; per-pixel identity is
    not expected: the reference binds RNG streams to ray slots, tests/test_reference_frames.py)."""
import os
import types

import numpy as np
import pytest

import ptss
import refprobe
from reference_common import MAX_LEFT_OUT, distance_ulp, hit_floors

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference")
SCENES = ["cornell", "default"]


def _load(name, what):
    with np.load(os.path.join(GOLDEN, f"{name}_{what}.npz")) as z:
        return {k: z[k] for k in z.files}


def _scene(name):
    tables = _load(name, "tables")
    tables = {k: np.ascontiguousarray(tables[k].astype(dt)) for k, dt in refprobe.TABLES}
    return types.SimpleNamespace(desc=refprobe.desc_of_tables(tables)), tables


@pytest.mark.parametrize("name", SCENES)
def test_ray_queries_against_the_reference(name):
    scene, tables = _scene(name)
    q = _load(name, "queries")
    n = len(q["rays"])
    assert n == 4096 and q["left_out"].mean() <= MAX_LEFT_OUT
    keep = ~q["left_out"]
    r = ptss.Renderer(scene, 64, 64, max_iterations=1, seed=1)
    try:
        rays = ptss.make_rays(q["rays"][:, :3], q["rays"][:, 3:], q["tmax"])
        hits = r.intersect(rays)
        occluded = r.occluded(rays)
    finally:
        r.close()
    # decisions
    assert np.array_equal(hits["kind"][keep], q["kind"][keep])
    assert np.array_equal(hits["primitive"][keep], q["primitive"][keep])
    assert np.array_equal(hits["materialIdx"][keep], q["materialIdx"][keep])
    assert np.array_equal(occluded[keep] != 0, ~q["visible"][keep])
    assert (q["kind"] == 1).sum() > 100 and (q["kind"] == 2).sum() > 100 and (q["kind"] == 0).sum() > 100
    miss = keep & (q["kind"] == 0)
    assert np.array_equal(hits["distance"][miss].view(np.uint32), q["tmax"][miss].view(np.uint32))   # a miss hands tmax back
    # floats
    span, nfloor, ok = hit_floors(q["rays"], q["distance"], q["kind"], q["primitive"], tables)
    k = keep & (q["kind"] > 0) & ok
    for label, got, want, floor in (("distance", hits["distance"][:, None], q["distance"][:, None], span), ("point", hits["point"], q["point"], span),
                                    ("normal", hits["normal"], q["normal"], nfloor)):
        e_ref = float(q[f"e_ref_{label}"])
        d = distance_ulp(got[k], want[k], want[k].astype(np.float64), floor[k][:, None], True).max()
        print(f"[reference] ptss_intersect {label} [{name}]: {d:.3f} ulp from the reference (e_ref {e_ref:.3f}, allowed {3 * e_ref + 1:.3f})")
        assert e_ref <= 64.0
        assert d <= 3 * e_ref + 1


@pytest.mark.parametrize("name", SCENES)
def test_frame_against_the_reference(name):
    scene, _ = _scene(name)
    g = _load(name, "blocks")
    spp, bounces, seed = int(g["samples"]), int(g["bounces"]), int(g["seed"])
    assert (spp, bounces) == (16, 15) and g["blocks"].shape == (64, 64, 3)
    r = ptss.Renderer(scene, 512, 512, max_iterations=bounces, seed=seed)
    try:
        for _ in range(spp):
            r.generate_frame()
        img = r.accumulator().astype(np.float64).reshape(512, 512, 3) / spp
    finally:
        r.close()
    means = img.mean(axis=(0, 1))
    blocks = img.reshape(64, 8, 64, 8, 3).mean(axis=(1, 3))
    rel = np.abs(means - g["means"]) / np.maximum(g["means"], 1.0)
    corr = float(np.corrcoef(blocks.ravel(), g["blocks"].astype(np.float64).ravel())[0, 1])
    print(f"[reference] frame [{name}]: channel means off by {rel.max():.2e}, block correlation {corr:.6f}")
    assert (rel <= 0.015).all()
    assert corr > 0.995
