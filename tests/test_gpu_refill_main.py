"""ptss_main --film ... --refill: the film's trace through ptss_trace_paths_opt with PTSS_PATHS_REFILL writes the
screenshot --film writes; the flag is the film's alone."""
import subprocess

import pytest

from test_gpu_film_main import ARGS, MAIN, run_main

pytestmark = pytest.mark.gpu


def test_refill_film_writes_the_films_screenshot(tmp_path):
    plain = run_main(["--film", "pinhole"], tmp_path / "plain.tga")
    refill = run_main(["--film", "pinhole", "--refill"], tmp_path / "refill.tga")
    assert refill == plain
    assert len(set(plain[18:])) > 50   # an image


def test_refill_needs_a_film(tmp_path):
    r = subprocess.run([MAIN] + ARGS + ["--refill", "--out", str(tmp_path / "x.tga")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--refill" in r.stderr
