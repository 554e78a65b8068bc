"""Bounce 0 finds the frame position of its pixels once per wave (csrc/ptlocate.h: waveOrigin for the strip's first pixel, then
laneCoord per lane — an add, a compare and three selects instead of four integer divisions), and per pixel (locate) only for
strips that cross more than one row end. Checked here on the host build of that very header (ptss_probe_wave_locate,
libptss_host.so): for EVERY first pixel of every frame of tests/test_gpu_wave_locate.py, and of widths 1 .. 130 with bands of 1
and 8 rows among 1 and 3 ranks, all 64 pixels of the strip get the {x, gy, globalIndex} that locate() gives them — and that an
independent numpy statement of the pixel order gives them. Integer arithmetic: equality, no tolerance. CPU only."""
import ctypes as C

import numpy as np
import pytest

import ptss

STRIP = 64
# (width, rows, band_rows, tile_world, rank): the frames of tests/test_gpu_wave_locate.py; `rows` = the whole frame's height, at
# least what any one context owns of it
FRAMES = [(33, 17, 8, 1, 0), (64, 9, 8, 1, 0), (70, 24, 8, 3, 0), (70, 24, 8, 3, 1), (70, 24, 8, 3, 2), (70, 24, 4, 3, 0), (70, 24, 4, 3, 1),
          (70, 24, 4, 3, 2), (200, 16, 8, 2, 0), (200, 16, 8, 2, 1), (1, 130, 8, 1, 0)]


def strips(width, rank, world, band_rows, first_begin, n):
    wave = np.zeros((n, STRIP, 3), dtype=np.int32)
    lane = np.zeros((n, STRIP, 3), dtype=np.int32)
    fast = np.zeros(n, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    rc = ptss.host_lib().ptss_probe_wave_locate(width, rank, world, band_rows, first_begin, n, wave.ctypes.data_as(ip),
                                                lane.ctypes.data_as(ip), fast.ctypes.data_as(ip))
    assert rc == 0
    return wave, lane, fast


def pixel_order(width, rank, world, band_rows, first_begin, n):
    """the tile's pixel order stated independently: local pixel -> (x, frame row, frame index)"""
    local = first_begin + np.arange(n, dtype=np.int64)[:, None] + np.arange(STRIP, dtype=np.int64)[None, :]
    x, ly = local % width, local // width
    gy = ((ly // band_rows) * world + rank) * band_rows + ly % band_rows
    return np.stack([x, gy, gy * width + x], axis=-1)


def check(width, rows, band_rows, world, rank):
    n = width * rows   # every first pixel of the context's tile (strips that start mid-row included)
    wave, lane, fast = strips(width, rank, world, band_rows, 0, n)
    assert np.array_equal(wave, lane), (width, rows, band_rows, world, rank)
    assert np.array_equal(lane.astype(np.int64), pixel_order(width, rank, world, band_rows, 0, n)), (width, rows, band_rows, world, rank)
    return fast


@pytest.mark.parametrize("width,rows,band_rows,world,rank", FRAMES)
def test_frames_of_the_gpu_test(width, rows, band_rows, world, rank):
    fast = check(width, rows, band_rows, world, rank)
    # which form a strip takes is decided by its first pixel's column alone: at most one row end inside the strip
    x0 = np.arange(width * rows) % width
    assert np.array_equal(fast == 1, x0 + STRIP - 1 < 2 * width)


@pytest.mark.parametrize("band_rows", [1, 8])
@pytest.mark.parametrize("world", [1, 3])
def test_every_width_to_130(band_rows, world):
    took_fast = 0
    for width in range(1, 131):
        for rank in range(world):
            fast = check(width, 3 * band_rows, band_rows, world, rank)   # three bands: two band jumps inside the tile
            took_fast += int(fast.sum())
            if width >= STRIP:
                assert fast.all()   # a real frame's strips never take the per-pixel form
    assert took_fast > 0


def test_band_jump_inside_a_strip():
    """70 x 24 among 3 ranks with bands of 8 rows: the strip that starts at column 20 of the band's last row ends in the first row of
    the context's NEXT band, 17 frame rows further down."""
    wave, lane, fast = strips(70, 1, 3, 8, 7 * 70 + 20, 1)
    assert fast[0] == 1
    assert wave[0, 0].tolist() == [20, 8 + 7, (8 + 7) * 70 + 20]
    assert wave[0, 49].tolist() == [69, 15, 15 * 70 + 69]
    assert wave[0, 50].tolist() == [0, 32, 32 * 70]
    assert np.array_equal(wave, lane)


def test_rejects_bad_arguments():
    ip = C.POINTER(C.c_int)
    out = np.zeros(STRIP * 3, dtype=np.int32)
    one = np.zeros(1, dtype=np.int32)
    L = ptss.host_lib()
    assert L.ptss_probe_wave_locate(0, 0, 1, 1, 0, 1, out.ctypes.data_as(ip), out.ctypes.data_as(ip), one.ctypes.data_as(ip)) != 0
    assert L.ptss_probe_wave_locate(8, 3, 3, 1, 0, 1, out.ctypes.data_as(ip), out.ctypes.data_as(ip), one.ctypes.data_as(ip)) != 0
