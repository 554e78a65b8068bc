"""How often do the per-operation range guards of the shading code send a wave to the IEEE sequences? (diagnostic build:
   python tools/build_variants.py gstat=PTSS_DIAG=32;  PTSS_LIBNAME=libptss_gstat.so python tools/guard_stat.py [c3|c2|c5 ...])
One pass of each configuration of bench.py (its frame, bounces and samples per pass); the counters of csrc/ptss_diag.h bit 5: waves
that reach a guarded site, and waves in which the tests every operation used to make (sqrt's, div3's) fail for at least one lane.
profiles/guards/escape_counts.txt is this table."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-path-tracer-ss_amd"))
import ptss  # noqa: E402

CONFIGS = {"c3": ("mixed", 1920, 1080, 8, 40), "c2": ("lambert", 1280, 720, 8, 32), "c5": ("stress", 3840, 2160, 12, 16)}
NAMES = ["light samples (waves x lights)", "  sqrt(distance2) escapes", "  offset / distance escapes", "  the one window of lightSample fails",
         "Lambert terms (waves x visible lights)", "  power / (4 pi distance2) escapes", "  ... because of a numerator alone",
         "n1 / n2 in scatter escapes"]
L = ptss.device_lib()
for name in (sys.argv[1:] or ["c3", "c2", "c5"]):
    preset, w, h, bounces, S = CONFIGS[name]
    r = ptss.Renderer(ptss.Scene(preset), w, h, max_iterations=bounces, sync_each_frame=False, samples_per_pass=S, frame_lanes=1)
    before = (C.c_ulonglong * 8)()
    assert L.ptss_debug_counters(r._ctx, before) == 0
    r.generate_frame()
    r.synchronize()
    out = (C.c_ulonglong * 8)()
    assert L.ptss_debug_counters(r._ctx, out) == 0
    v = [int(a) - int(b) for a, b in zip(out, before)]
    print("%s: %s %dx%d, %d bounces, S = %d, one pass, guard flags %d" % (name, preset, w, h, bounces, S, r.guard_flags()))
    for i, n in enumerate(NAMES):
        base = v[0] if i < 4 else (v[4] if i < 7 else 0)
        share = "  (%.2f %%)" % (100.0 * v[i] / base) if base and i not in (0, 4) else ""
        print("  %-44s %12d%s" % (n, v[i], share))
    r.close()
