// ptlocate.h — pixel order of a tile: where local pixel `local` of a context sits in the frame, per pixel (locate) and for the
// 64 consecutive local pixels of one wave at a time (waveOrigin + laneCoord). Integer arithmetic only, restating no reference
// line; compiled for the device (ptraypool.h) and for the host, where tests/test_wave_locate_cpu.py compares the two forms
// exhaustively through ptss_probe_wave_locate.
//
// A context owns bands of `bandRows` rows: its local row ly is row ly % bandRows of its band ly / bandRows, and band b of rank r
// starts at frame row (b * world + r) * bandRows. locate() costs four 32-bit integer divisions by run-time values, each some
// twenty vector instructions on gfx950, which has no integer divide. The lanes of a wave of bounce 0 hold consecutive local
// pixels, so the divisions are needed for the first of them only, on wave-uniform values: lane k sits k pixels to the right, and
// where that runs past the row's end, at the start of the next local row — one frame row further down, or at the top of the
// context's next band, (world - 1) * bandRows + 1 frame rows further down, when the first pixel's row is the last of its band.
// That covers a strip that crosses at most ONE row end (first.x + 63 < 2 * width: every strip at width >= 64); a narrower frame's
// strips take locate() per lane (WaveOrigin::oneWrap is wave-uniform).
#pragma once
#include "ptmath.h"

namespace ptloc {

struct Coord {
    int x, gy;
    uint32_t globalIndex;
};

PTM_HD Coord locate(int width, int rank, int world, int bandRows, uint32_t local) {
    const int lx = (int)(local % (uint32_t)width);
    const int ly = (int)(local / (uint32_t)width);
    const int band = ly / bandRows, within = ly % bandRows;
    Coord p;
    p.x = lx;
    p.gy = (band * world + rank) * bandRows + within;
    p.globalIndex = (uint32_t)p.gy * (uint32_t)width + (uint32_t)lx;
    return p;
}

constexpr uint32_t kStrip = 64;   // pixels located together: one wave

struct WaveOrigin {
    Coord first;        // locate() of the strip's first pixel
    int rowStep;        // frame rows from the first pixel's row to the next local row: 1, or the jump to the context's next band
    uint32_t rowJump;   // what the global index gains at that row end beyond the lane number: (rowStep - 1) * width
    bool oneWrap;       // the strip crosses at most one row end: laneCoord applies
};

PTM_HD WaveOrigin waveOrigin(int width, int rank, int world, int bandRows, uint32_t first) {
    const int ly = (int)(first / (uint32_t)width);
    const int within = ly % bandRows;
    WaveOrigin w;
    w.first = locate(width, rank, world, bandRows, first);
    w.rowStep = (within + 1 == bandRows) ? (world - 1) * bandRows + 1 : 1;
    w.rowJump = (uint32_t)(w.rowStep - 1) * (uint32_t)width;
    w.oneWrap = (uint32_t)w.first.x + (kStrip - 1) < 2u * (uint32_t)width;
    return w;
}

// pixel first + lane of a strip with oneWrap, lane < kStrip
PTM_HD Coord laneCoord(const WaveOrigin& w, int width, uint32_t lane) {
    const int x = w.first.x + (int)lane;
    const bool wrapped = x >= width;
    Coord p;
    p.x = wrapped ? x - width : x;
    p.gy = wrapped ? w.first.gy + w.rowStep : w.first.gy;
    p.globalIndex = w.first.globalIndex + lane + (wrapped ? w.rowJump : 0u);
    return p;
}

}  // namespace ptloc
