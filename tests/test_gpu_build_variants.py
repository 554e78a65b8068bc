"""Every non-ablation build of tools/build_variants.py against the oracle. The same-box A/B measurements of profiles/README.md and
the histogram tools rest on these builds tracing the image the shipped library traces; this module builds each of them and
runs a battery of the oracle-parity tests in a fresh child process that loads it (PTSS_LIBNAME=libptss_<tag>.so).

Batteries: the tile / shard builds (s8, s32, b128) get the loop-guard tests of both frame paths, the S > 1 extension, pixel
tiles and odd frame sizes; the chunk build (ck8) the many-sphere tests; register-budget and diagnostic builds a few whole-frame
cases and the committed golden vectors; every build gets tests/test_gpu_kernel_coverage.py, whose per-case instantiation sets
hold under all of them (its cases stay far from the 64 KiB LDS edge, so b128's smaller work area changes no choice) except
`knobs` with PTSS_SCENE_PATH=scalar, where that module itself maps them to the in-place instantiations. A diagnostic build
must also move its counters there (test_debug_counters_only_in_diagnostic_builds).

Left out on purpose, because their expectation is a fact of the default build rather than of the image:
test_gpu_one_launch.py::test_which_frames_qualify (which frame sizes are resident at once depends on the tile size, the shard
count and the register budget), test_gpu_lanes.py::test_automatic_lane_count (the same), and the full-size tests
(1080p / 4K, the 512 x 512 40-tick run, the bench ranks), which take minutes per build and check nothing the batteries
do not.

The children run one at a time, each under a time limit. A child that faults (a negative status, 134, 139) or runs out of
time stops the module: every later variant fails at once without starting a process, and nothing is retried. So does a
module that has run for MODULE_BUDGET_S. Measured on an MI355X box: the 16 builds 28 s with 16 workers, a child 4-6 s,
the module 108 s."""
import concurrent.futures
import importlib.util
import os
import re
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 150    # a battery takes a few seconds
MODULE_BUDGET_S = 900    # builds included: no variant starts after this

COVERAGE = ["tests/test_gpu_kernel_coverage.py"]                                                  # 16 tests
GUARD = ["tests/test_gpu_one_launch.py::test_loop_guard_is_exact_in_one_launch",                  # 7
         "tests/test_gpu_lanes.py::test_loop_guard_is_exact_across_lanes",                        # 10
         "tests/test_gpu_parity.py::test_loop_guard_leaves_rays_to_the_flush_kernel",             # 1
         "tests/test_gpu_parity.py::test_tiny_frame_below_the_guard"]                             # 1
GEOMETRY = GUARD + ["tests/test_gpu_parity.py::test_samples_per_pass_extension_matches_oracle",   # 7
                    "tests/test_gpu_tiles.py::test_tiles_reassemble_to_the_oracle_frame",         # 4
                    "tests/test_gpu_edge_scenes.py::test_frame_sizes_that_divide_by_nothing"] + COVERAGE   # 4
CHUNKS = ["tests/test_gpu_many_spheres.py::test_exact_ties_end_on_the_highest_index_like_the_sequential_loop",   # 1
          "tests/test_gpu_many_spheres.py::test_large_random_scenes",                                          # 4
          "tests/test_gpu_many_spheres.py::test_more_than_128_chunks",                                         # 2
          "tests/test_gpu_many_spheres.py::test_camera_inside_the_cluster_rays_leaving_chunks_they_start_beside",  # 1
          "tests/test_gpu_many_spheres.py::test_camera_outside_the_structures_range_falls_back",               # 1
          "tests/test_gpu_one_launch.py::test_many_spheres_in_one_launch"] + COVERAGE                          # 1
FRAMES = ["tests/test_gpu_parity.py::test_frames_match_oracle[mixed-160-90-8-8]",
          "tests/test_gpu_parity.py::test_frames_match_oracle[pointlight-96-96-5-6]",
          "tests/test_gpu_parity.py::test_frames_match_oracle[cornell-33-17-6-5]",
          "tests/test_gpu_parity.py::test_against_committed_golden_vectors"] + COVERAGE                        # 3 + 5

# run name: (build tag, extra environment, node ids, tests that must pass)
BATTERIES = {
    "s8": ("s8", {}, GEOMETRY, 50),
    "s32": ("s32", {}, GEOMETRY, 50),
    "b128": ("b128", {}, GEOMETRY, 50),
    "ck8": ("ck8", {}, CHUNKS, 26),
    **{tag: (tag, {}, FRAMES, 24) for tag in ("w6", "w8", "wb5", "wb7", "f5", "f7", "chist", "shist", "cullstat", "pairstat", "qhist")},
    "knobs-scalar": ("knobs", {"PTSS_SCENE_PATH": "scalar"}, FRAMES, 24),
    "knobs-grid-cap-1": ("knobs", {"PTSS_GRID_CAP": "1"}, FRAMES + ["tests/test_gpu_parity.py::test_samples_per_pass_extension_matches_oracle"], 31),
}


def build_variants_module():
    spec = importlib.util.spec_from_file_location("build_variants", os.path.join(ROOT, "tools", "build_variants.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def variant_tags():
    """Every build of tools/build_variants.py except the ablations (a*: wrong images by construction)."""
    return [t for t in build_variants_module().VARIANTS if not re.fullmatch(r"a\d+", t)]


def pytest_args(ids):
    return ["-m", "gpu", "-p", "no:cacheprovider"] + list(ids)


def child_command(ids):
    return [sys.executable, "-m", "pytest", "-q"] + pytest_args(ids)


def summary_counts(output):
    """{'passed': n, 'failed': m, ...} from pytest's closing line (warnings are not outcomes)."""
    lines = [ln for ln in output.strip().splitlines() if re.search(r"\d+ (passed|failed|error|errors|skipped|deselected)", ln)]
    if not lines:
        return {}
    counts = {k: int(n) for n, k in re.findall(r"(\d+) (\w+)", lines[-1])}
    counts.pop("warnings", None)
    counts.pop("warning", None)
    return counts


_start = []   # when the module's builds began


@pytest.fixture(scope="module")
def built():
    """hipcc for every tested tag, in parallel (no GPU needed): tag -> None or the build error."""
    _start.append(time.monotonic())
    bv = build_variants_module()
    workers = min(16, int(os.environ.get("MAX_JOBS", 8)))

    def one(tag):
        try:
            bv.b.build_device(force=True, defines=bv.VARIANTS[tag], name=f"libptss_{tag}.so")
            return None
        except Exception as e:   # reported by that tag's test
            return repr(e)
    tags = variant_tags()
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as ex:
        return dict(zip(tags, ex.map(one, tags)))


_stopped = []   # the reason the first fault or timeout ended the module, if one did


@pytest.mark.parametrize("run", list(BATTERIES))
def test_variant_matches_the_oracle(run, built):
    assert not _stopped, f"not started: an earlier variant faulted or timed out ({_stopped[0]})"
    if time.monotonic() - _start[0] > MODULE_BUDGET_S:
        _stopped.append(f"the module has run for more than {MODULE_BUDGET_S} s")
        raise AssertionError(f"not started: {_stopped[-1]}")
    tag, extra, ids, want = BATTERIES[run]
    assert built[tag] is None, f"libptss_{tag}.so did not build: {built[tag]}"
    env = {k: v for k, v in os.environ.items() if k not in ("PTSS_SCENE_PATH", "PTSS_GRID_CAP")}
    env.update(extra, PTSS_LIBNAME=f"libptss_{tag}.so")
    t0 = time.monotonic()
    try:
        p = subprocess.run(child_command(ids), cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _stopped.append(f"{run}: no result within {CHILD_TIMEOUT_S} s")
        raise AssertionError(_stopped[-1])
    tail = "\n".join((p.stdout + p.stderr).strip().splitlines()[-40:])
    if p.returncode < 0 or p.returncode in (134, 139):
        _stopped.append(f"{run}: child ended with status {p.returncode}")
        raise AssertionError(f"{_stopped[-1]}\n{tail}")
    counts = summary_counts(p.stdout)
    assert p.returncode == 0 and counts == {"passed": want}, f"{run}: status {p.returncode}, {counts}, want {want} passed\n{tail}"
    print(f"{run}: {want} passed in {time.monotonic() - t0:.1f} s")
