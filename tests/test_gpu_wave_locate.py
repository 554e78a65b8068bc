"""Bounce 0 finds the frame position of a wave's 64 consecutive local pixels once per wave (csrc/ptlocate.h, locateWave in
csrc/ptraypool.h) instead of with four integer divisions per lane. A wrong position moves a pixel's eye ray and with it every
sample of the pixel, so the GPU accumulator is compared with the oracle's, array_equal, on frames chosen for the wrap cases:

  33 x 17                       strips that cross several row ends (the per-pixel form, chosen per wave)
  64 x 9                        a strip is exactly one row
  70 x 24, bands of 8, 3 ranks  a row end inside most strips; every rank's tile
  70 x 24, bands of 4, 3 ranks  ... and each rank owns two bands: a strip that crosses from one into the next (band jump)
  200 x 16, 2 ranks             at most one row end per strip, bands of 8
  1 x 130                       width 1: 64 row ends per strip

each at S = 1 and at S = 3 samples per pass — none of the pixel counts is a multiple of the 256-pixel tile, so the last tile of a
sample plane is partly empty and the next plane starts in a tile of its own. 2 bounces, `mixed`. The arithmetic itself is checked
exhaustively on the host by tests/test_wave_locate_cpu.py."""
import numpy as np
import pytest

import oracle
import ptss
import tiles

pytestmark = pytest.mark.gpu

FRAMES = [(33, 17, 8, 1), (64, 9, 8, 1), (70, 24, 8, 3), (70, 24, 4, 3), (200, 16, 8, 2), (1, 130, 8, 1)]


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("w,h,band,world", FRAMES)
def test_accumulator_matches_the_oracle(w, h, band, world, S):
    bounces, passes = 2, 2
    scene = ptss.Scene("mixed")
    o = oracle.Oracle(scene.desc, w, h, max_iterations=bounces, samples_per_pass=S)
    rs = [ptss.Renderer(scene, w, h, max_iterations=bounces, tile_rank=k, tile_world=world, band_rows=band, samples_per_pass=S)
          for k in range(world)]
    for _ in range(passes):
        o.generate_frame()
        for r in rs:
            r.generate_frame()
    assert sum(r.local_pixels for r in rs) == w * h
    acc = tiles.untile([r.accumulator() for r in rs], w, h, band) if world > 1 else rs[0].accumulator()
    assert np.array_equal(acc, o.accumulator())
    assert sum(r.total_ray_bounces() for r in rs) == o.total_ray_bounces()
    for r in rs:
        r.close()
