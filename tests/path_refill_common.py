"""What tests/test_path_refill_cpu.py and tests/test_gpu_path_refill.py share (ptss_trace_paths_opt with PTSS_PATHS_REFILL; DESIGN.md
§3.27): a pure-Python model of the refill rule, the bound on the wave iterations it implies, and the plain schedule's count.

The rule, as csrc/ptss_paths.hip pathRefillKernel states it. A grid of `grid` workgroups of BLOCK lanes (WAVES waves of 64) runs a batch
of n rays, grid <= ceil(n / BLOCK). Lane t of workgroup b starts with ray b * BLOCK + t (dead if that is >= n); the head starts at
grid * BLOCK. Each wave keeps a reserve [next, end), empty at first, and a flag `drained`, set at the start when grid * BLOCK >= n.
Before every iteration the wave's dead lanes are served in at most two steps: if the reserve is empty and the wave is not drained it
claims h = head, head += chunk (one dequeue), becomes drained when h + chunk >= n, and — when h < n — its reserve is
[h, min(h + chunk, n)); then the dead lanes, ranked in lane order, take next, next + 1, .. while the reserve lasts. The wave then runs
one iteration if any lane is live, and ends otherwise. A path of `bounces` iterations retires after its last one.

The bound. A wave runs an iteration with a dead lane only after it has found its reserve empty while drained — that is, after the head
had passed n. From then on it gets no new ray, and every live lane has at most maxIterations iterations left: at most maxIterations
such iterations per wave. Every other iteration has 64 live lanes, and the lane iterations add up to sum(bounces). So
    wave iterations <= floor(sum(bounces) / 64) + W * maxIterations,   W = grid * WAVES."""
import numpy as np

BLOCK = 256
WAVES = BLOCK // 64
CHUNKS = (64, 256, 1024)


class RefillRun:
    """One simulated launch: claimed[i] = how often ray i was taken; the three counters; per wave its iterations."""

    def __init__(self, n, waves):
        self.claimed = np.zeros(n, dtype=np.int64)
        self.wave_iterations = 0
        self.lane_iterations = 0
        self.dequeues = 0
        self.per_wave = np.zeros(waves, dtype=np.int64)
        self.non_full_after_drain_only = True   # no iteration with a dead lane before the wave saw an empty reserve while drained


def simulate(bounces, grid, chunk, order):
    """Runs the rule over a batch whose ray i lives bounces[i] >= 1 iterations. order: a numpy Generator; at every step one of the
    unfinished waves, drawn from it, refills and runs one iteration (the head is the only shared word, so this covers every
    interleaving of the dequeues)."""
    bounces = np.asarray(bounces, dtype=np.int64)
    n = len(bounces)
    assert 1 <= grid <= (n + BLOCK - 1) // BLOCK and bounces.min() >= 1
    W = grid * WAVES
    run = RefillRun(n, W)
    head = grid * BLOCK
    ray = np.full((W, 64), -1, dtype=np.int64)       # the ray of each lane, -1 = dead
    left = np.zeros((W, 64), dtype=np.int64)          # iterations it still enters
    for w in range(W):
        first = w * 64
        idx = np.arange(first, first + 64)
        ok = idx < n
        ray[w, ok] = idx[ok]
        left[w, ok] = bounces[idx[ok]]
        run.claimed[idx[ok]] += 1
    nxt, end = np.zeros(W, dtype=np.int64), np.zeros(W, dtype=np.int64)
    drained = np.full(W, head >= n)
    starved = np.zeros(W, dtype=bool)   # found the reserve empty while drained
    unfinished = list(range(W))
    while unfinished:
        w = unfinished[int(order.integers(len(unfinished)))]
        for _ in range(2):
            dead = np.nonzero(ray[w] < 0)[0]
            if len(dead) == 0:
                break
            if nxt[w] == end[w]:
                if drained[w]:
                    starved[w] = True
                    break
                h = head
                head += chunk
                run.dequeues += 1
                drained[w] = h + chunk >= n
                if h >= n:
                    starved[w] = True
                    break
                nxt[w], end[w] = h, min(h + chunk, n)
            take = min(len(dead), end[w] - nxt[w])
            got = np.arange(nxt[w], nxt[w] + take)
            ray[w, dead[:take]] = got
            left[w, dead[:take]] = bounces[got]
            run.claimed[got] += 1
            nxt[w] += take
        if nxt[w] == end[w] and drained[w]:   # (the last chunk, cut off at n, may have been too short for the dead lanes)
            starved[w] = True
        live = ray[w] >= 0
        if not live.any():
            unfinished.remove(w)
            continue
        if not live.all() and not starved[w]:
            run.non_full_after_drain_only = False
        run.wave_iterations += 1
        run.per_wave[w] += 1
        run.lane_iterations += int(live.sum())
        left[w, live] -= 1
        ray[w, live & (left[w] == 0)] = -1
    return run


def wave_iteration_bound(bounces, waves, max_iterations):
    """The bound of this file's docstring."""
    return int(np.asarray(bounces, dtype=np.int64).sum()) // 64 + waves * max_iterations


def plain_wave_iterations(bounces):
    """What ptss_trace_paths' schedule runs: a wave of 64 consecutive rays iterates until its longest path has ended."""
    b = np.asarray(bounces, dtype=np.int64)
    b = np.concatenate([b, np.zeros((-len(b)) % 64, dtype=np.int64)])
    return int(b.reshape(-1, 64).max(axis=1).sum())
