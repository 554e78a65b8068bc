"""tools/denoise_profile.py — per-level kernel times and hardware counters of ptss_denoise, from rocprofv3 runs.

  denoise_profile.py run WxH SCENE        the workload: 4 frames, features, 30 five-level ptss_denoise calls (run it UNDER rocprofv3)
  denoise_profile.py levels DIR...        reduce `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python
                                          tools/denoise_profile.py run ...`: denoiseKernel launches in start order, launch i is
                                          level i mod 5; the first five calls dropped; median [min, max] in us per level
                                          (profiles/denoise/kernel_trace_levels.txt)
  denoise_profile.py counters DIR...      reduce `rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY
                                          SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_VMEM_RD --output-format csv
                                          -d DIR -- ...` (a run of its own, no tracing): mean per dispatch and instantiation, the
                                          first fifth of the dispatches dropped (profiles/denoise/counters_1080p.txt)"""
import collections
import csv
import ctypes as C
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(size, scene_name):
    sys.path.insert(0, os.path.join(ROOT, "cuda-path-tracer-ss_amd"))
    import ptss
    w, h = (int(v) for v in size.split("x"))
    r = ptss.Renderer(ptss.Scene(scene_name), w, h)
    for _ in range(4):
        r.generate_frame()
    r.features()
    p = ptss.default_denoise_params(levels=5)
    d_feat, d_out = r.features_devptr(), r._device_buffer("denoised", r.local_pixels * 4)
    for _ in range(30):
        ptss._check(ptss.device_lib().ptss_denoise(r._ctx, d_feat, C.byref(p), d_out, None))
    r.synchronize()
    r.close()


def rows_of(d, pattern):
    files = glob.glob(os.path.join(d, "**", pattern), recursive=True)
    if not files:
        raise SystemExit(f"{d}: no {pattern}")
    with open(files[0]) as f:
        return list(csv.DictReader(f))


def levels(dirs):
    for d in dirs:
        rows = sorted(rows_of(d, "*kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
        per = collections.defaultdict(list)
        for i, r in enumerate(r for r in rows if "denoiseKernel" in r["Kernel_Name"]):
            per[i % 5].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        print(d)
        for k in sorted(per):
            v = per[k][5:]
            print(f"  level {k} (spacing {1 << k}): median {statistics.median(v):.1f} us [min {min(v):.1f}, max {max(v):.1f}] over {len(v)} launches")


def counters(dirs):
    for d in dirs:
        agg = collections.defaultdict(lambda: collections.defaultdict(list))
        for r in rows_of(d, "*counter_collection.csv"):
            if "denoiseKernel" in r["Kernel_Name"]:
                agg[r["Kernel_Name"].split("(")[0]][r["Counter_Name"]].append(float(r["Counter_Value"]))
        print(d)
        for name, cs in agg.items():
            print(" ", name)
            for c, v in sorted(cs.items()):
                v = v[len(v) // 5:]
                print(f"    {c}: mean {sum(v) / len(v):.4g} over {len(v)} dispatches")


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3])
    elif len(sys.argv) >= 3 and sys.argv[1] in ("levels", "counters"):
        {"levels": levels, "counters": counters}[sys.argv[1]](sys.argv[2:])
    else:
        raise SystemExit(__doc__)
