"""The parity batteries of tests/test_gpu_build_variants.py stay complete without a GPU: every non-ablation build of
tools/build_variants.py has one (a new switch cannot ship untested), and every node id in them exists and collects to the
stated number of tests, with nothing deselected by `-m gpu`."""
import subprocess
import sys

import test_gpu_build_variants as tbv


def test_every_build_has_a_battery():
    tags = set(tbv.variant_tags())
    covered = {tag for tag, _, _, _ in tbv.BATTERIES.values()}
    assert tags - covered == set(), f"builds without a parity battery: {sorted(tags - covered)}"
    assert covered - tags == set(), f"batteries for builds tools/build_variants.py does not list: {sorted(covered - tags)}"
    assert tags >= {"s8", "s32", "b128", "ck8", "knobs", "chist"} and not any(t.startswith("a") and t[1:].isdigit() for t in covered)


def test_every_node_id_collects_to_the_stated_count():
    collected = {}
    for run, (tag, _, ids, want) in tbv.BATTERIES.items():
        key = tuple(ids)
        if key not in collected:
            p = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q"] + tbv.pytest_args(ids),
                               cwd=tbv.ROOT, capture_output=True, text=True, timeout=300)
            assert p.returncode == 0, f"{run}: collection failed\n{p.stdout[-3000:]}\n{p.stderr[-3000:]}"
            assert "deselected" not in p.stdout, f"{run}: `-m gpu` deselects some of {ids}"
            collected[key] = sum(1 for ln in p.stdout.splitlines() if "::" in ln)
        assert collected[key] == want, f"{run}: the battery collects {collected[key]} tests, its table says {want}"


def test_summary_line_is_read_strictly():
    assert tbv.summary_counts("....\n24 passed in 12.3s\n") == {"passed": 24}
    assert tbv.summary_counts("24 passed, 2 warnings in 1.0s") == {"passed": 24}
    assert tbv.summary_counts("23 passed, 1 skipped in 1.0s") == {"passed": 23, "skipped": 1}
    assert tbv.summary_counts("1 failed, 23 passed in 1.0s") == {"failed": 1, "passed": 23}
    assert tbv.summary_counts("") == {}
