"""Records what the reference's own code, compiled for the CPU, answers — DATA ONLY — into tests/golden/reference/, for
tests/test_gpu_reference_pins.py, which runs where there is no reference. Reads nothing but oracle/_ref/libref_probe.so (built by
`python __graft_entry__.py build` on a machine that has the reference).

  <scene>_tables.npz    the reference's five scene tables, built by its own Scene methods
  <scene>_queries.npz   4,096 query rays with the reference's closest hit (the intersection loops of pathTraceKernel: primitive,
                        distance, point, normal) and its lineOfSight verdict; which cases sit on a threshold (float64 model);
                        e_ref per float output (tests/reference_common.py)
  <scene>_blocks.npz    the 64 x 64 x 3 block means of the reference's 16-sample 512 x 512 frame (path tracer, 15 bounces)

Run: python tests/golden/make_reference_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import reference_common as rc   # noqa: E402
import refprobe                 # noqa: E402

OUT = os.path.join(HERE, "reference")
QUERIES = 4096
SEED = 0x5EED
SPP = 16


def main():
    ref = refprobe.Probes("ref")
    os.makedirs(OUT, exist_ok=True)
    for kind, name in ((1, "cornell"), (0, "default")):
        tables = ref.build_scene(kind)
        np.savez_compressed(os.path.join(OUT, f"{name}_tables.npz"), **tables)

        rng = np.random.default_rng(1000 + kind)
        normal, p0, p1 = rc.query_cases(rng, ref, name, tables, QUERIES)
        rays, tmax = rc.los_rays(normal, p0, p1)
        visible, _ = ref.line_of_sight(normal, p0, p1)
        # the float32 ray above IS the one lineOfSight built: its own two loops over that ray give lineOfSight's verdict
        assert np.array_equal(ref.any_hit(rays, tmax), ~visible)
        kind_r, prim_r, hit = ref.closest_hit(rays, tmax)
        sc = rc.scene_arrays(tables)
        kind_m, prim_m, t, point, nrm, near_hit = rc.closest_hit_model(sc, rc.f64(rays[:, :3]), rc.f64(rays[:, 3:]), rc.f64(tmax))
        vis_m, _, _, near_los = rc.line_of_sight_model(sc, rc.f64(normal), rc.f64(p0), rc.f64(p1))
        left_out = near_hit | near_los
        keep = rc.check_left_out(f"recorded queries [{name}]", left_out)
        assert np.array_equal(kind_r[keep], kind_m[keep]) and np.array_equal(prim_r[keep], prim_m[keep]) and np.array_equal(visible[keep], vis_m[keep])
        span, nfloor, ok = rc.hit_floors(rays, hit[:, 0], kind_r, prim_r, tables)
        k = keep & (kind_r > 0) & ok
        e_ref = {}
        for label, cols, model, floor, vector in (("distance", slice(0, 1), t[:, None], span, True), ("point", slice(1, 4), point, span, True),
                                                  ("normal", slice(4, 7), nrm, nfloor, True)):
            e_ref[label] = rc.check_floats(f"recorded {label} [{name}]", hit[:, cols], hit[:, cols], model, floor=floor, vector=vector, keep=k)[0]
        np.savez_compressed(os.path.join(OUT, f"{name}_queries.npz"), rays=rays, tmax=tmax, kind=kind_r, primitive=prim_r,
                            distance=hit[:, 0], point=hit[:, 1:4], normal=hit[:, 4:7], materialIdx=hit[:, 7].astype(np.int32),
                            visible=visible, left_out=left_out, e_ref_distance=e_ref["distance"], e_ref_point=e_ref["point"],
                            e_ref_normal=e_ref["normal"])

        frames = refprobe.RefFrames(ref, SEED, True, 15)
        for _ in range(SPP):
            frames.generate_frame()
        img = frames.accumulator().astype(np.float64).reshape(refprobe.DIM, refprobe.DIM, 3) / SPP
        frames.close()
        blocks = img.reshape(64, 8, 64, 8, 3).mean(axis=(1, 3))
        np.savez_compressed(os.path.join(OUT, f"{name}_blocks.npz"), blocks=blocks.astype(np.float32), means=img.mean(axis=(0, 1)),
                            seed=SEED, samples=SPP, bounces=15)
        print(f"{name}: hits {np.bincount(kind_r, minlength=3)}, visible {int(visible.sum())}, channel means {img.mean(axis=(0, 1))}")
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
