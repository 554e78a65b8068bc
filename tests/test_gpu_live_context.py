"""Scene updates on LIVE contexts in every context configuration (tests/live_context_common.py holds the scenes,
configurations, scripts and the model, and tests/test_live_context_scripts.py checks that harness without a GPU).

include/ptss.h promises that after ptss_set_scene / ptss_update_triangles / ptss_reseed "the context behaves as a fresh
ptss_create(scene, cfg) would, except for the state of its random streams and those counters" — for every cfg. Here the scene
changes KIND under contexts that have rendered: frame lanes (ordered, free-running, with doubled sample words), one-launch frames,
pixel-band shards, an asynchronous caller's stream.

  the matrix     every ordered pair of the seven image kinds under the two configurations that keep cross-frame device counters
                 (one_launch, lanes3_free: 2 x 42 cases), and one closed chain through all seven kinds under each of the other six.
                 A leg: two frames on `a` equal to a's oracle; set_scene(b), reseed; three frames equal to a fresh oracle of b — live
                 counts every frame, accumulator, display pixels, float sums, RNG records of sampled pixels in every sample lane —
                 and what a fresh context of (b, cfg) reports: one_launch_frames, triangle_leaves, guard_flags, and the kernel
                 instantiations its three frames launch. ptss_launched_kernels is cumulative, so "added by the three frames" is
                 compared on what the context had not launched before: added == fresh's - launched before.
  the scripts    six random scripts of 12-16 steps per configuration. After every frame the live counts equal the twin's; while an
                 oracle can follow (from a reseed to the next scene change) twin and subject equal the oracle; the display pixels are
                 those of an accumulator with the number of samples the Model counts since the last reset; at the end everything
                 equals the twin's, update_rejected is the number of bad records sent, 2,048 query rays answer as a fresh
                 everySphereLoop context on the final scene answers, and no bounded wait expired.
                 async_stream enqueues the whole script on a side stream and reads nothing until one synchronize() at the end.
                 A pixel-band shard is refused by ptss_denoise (it has no neighbouring rows): there the step asserts the refusal.

No tolerance anywhere: array_equal or byte-equal."""
import time

import numpy as np
import pytest

import ptss
from live_context_common import (BOUNCES, CHAIN_CONFIGS, CONFIGS, FRAME, PAIR_CONFIGS, SCRIPT_SEEDS, SEED1, SEED2, Follower, Model,
                                 Reference, Subject, above_guard, bounces_of, chain, display_of, drive_state, make_script,
                                 oracle_snapshot, ordered_pairs, pair_frame, query_rays, samples_of, scene, sharded, snapshot_equal,
                                 subject_snapshot)

pytestmark = pytest.mark.gpu


def frames_equal_reference(sub, ref, done, n, tick, what):
    """Frames done + 1 .. done + n of a fresh context's oracle: live counts after every frame, then everything else."""
    for i in range(n):
        sub.generate_frame(tick + i)
        want = ref.after(done + i + 1)
        if sharded(sub.cfg):
            assert above_guard(want["live"]), (what, i, want["live"])   # else shards and oracle differ by design
        assert np.array_equal(sub.live_counts(), want["live"]), (what, "frame", done + i + 1)
    snapshot_equal(sub, ref.after(done + n), what)
    return tick + n


def per_context(r):
    return r.one_launch_frames, r.triangle_leaves(), r.guard_flags()


def transition(sub, b, seed2, bounces, tick, what):
    """set_scene(b), reseed(seed2), three frames: a fresh oracle's, and a fresh context's kernels and image facts."""
    before = sub.per_rank(lambda r: r.launched_kernels())
    sub.set_scene(scene(b))
    sub.reseed(seed2)
    ref = Reference.of(b, sub.width, sub.height, bounces, sub.S, seed2)
    tick = frames_equal_reference(sub, ref, 0, 3, tick, what)
    fresh = Subject(sub.cfg, scene(b), sub.width, sub.height, bounces, seed2)
    try:
        for t in range(1, 4):
            fresh.generate_frame(t)
        assert sub.per_rank(per_context) == fresh.per_rank(per_context), what
        for had, now, new in zip(before, sub.per_rank(lambda r: r.launched_kernels()), fresh.per_rank(lambda r: r.launched_kernels())):
            families = sorted({k[:2] for k in new})
            assert now - had == new - had, (what, families, sorted((now - had) ^ (new - had)))
            assert new <= now, (what, families)
        assert fresh.guard_timeouts() == 0, what
    finally:
        fresh.close()
    assert sub.guard_timeouts() == 0, what
    return tick


@pytest.mark.parametrize("a,b", ordered_pairs(), ids=lambda k: k)
@pytest.mark.parametrize("cfg", PAIR_CONFIGS)
def test_every_pair_of_kinds_under_cross_frame_counters(cfg, a, b):
    w, h = pair_frame(a, b)
    sub = Subject(cfg, scene(a), w, h, BOUNCES, SEED1)
    try:
        tick = frames_equal_reference(sub, Reference.of(a, w, h, BOUNCES, sub.S, SEED1), 0, 2, 1, (cfg, a, "before"))
        transition(sub, b, SEED2, BOUNCES, tick, (cfg, a, b))
    finally:
        sub.close()


@pytest.mark.parametrize("cfg", CHAIN_CONFIGS)
def test_a_closed_chain_through_every_kind(cfg):
    """One context, seven legs: the three frames that end a leg and the two that begin the next are frames 1..5 of one oracle."""
    w, h = FRAME
    bounces = bounces_of(cfg)
    legs = chain(cfg)
    sub = Subject(cfg, scene(legs[0][0]), w, h, bounces, SEED1)
    try:
        seed, done, tick = SEED1, 0, 1
        for i, (a, b) in enumerate(legs):
            tick = frames_equal_reference(sub, Reference.of(a, w, h, bounces, sub.S, seed), done, 2, tick, (cfg, i, a, "before"))
            seed, done = SEED2 + i, 3
            tick = transition(sub, b, seed, bounces, tick, (cfg, i, a, b))
    finally:
        sub.close()


def run_script(cfg, seed):
    script = make_script(cfg, seed)
    w, h = FRAME
    S, bounces = samples_of(cfg), bounces_of(cfg)
    model = Model(script[0][1], SEED1, w, h, bounces, S)
    sub = twin = follower = None
    try:
        sub = Subject(cfg, scene(model.kind), w, h, bounces, SEED1)
        twin = Subject("base", scene(model.kind), w, h, bounces, SEED1, samples_per_pass=S)
        follower = Follower(model)
        reads = sub.stream is None   # async_stream: nothing is read (every read-back synchronises) before the end
        for k, step in enumerate(script[1:]):
            name, what = step[0], (cfg, seed, k, step)
            if name in ("frames", "ticks_jump"):
                for tick in model.ticks_of(step):
                    model.frame(tick)
                    sub.generate_frame(tick)
                    twin.generate_frame(tick)
                    live = twin.live_counts()
                    if follower.frame(tick) is not None:
                        want = follower.o.live_counts()
                        assert not sharded(cfg) or above_guard(want), (what, tick, want)
                        assert np.array_equal(live, want), (what, tick, "twin against the oracle")
                    if reads:
                        assert np.array_equal(sub.live_counts(), live), (what, tick)
                if follower.o is not None:   # from a checkpoint on: the oracle
                    want = oracle_snapshot(follower.o, w * h, S)
                    snapshot_equal(twin, want, (what, "twin against the oracle"))
                    if reads:
                        snapshot_equal(sub, want, (what, "against the oracle"))
                if reads:   # the sums hold the samples since the last reset the Model knows of
                    assert np.array_equal(sub.pixels(), display_of(sub.accumulator(), model.samples_held())), (what, "samples held")
                continue
            records = model.records_of(step) if name == "update_triangles" else None
            model.note(step)
            follower.step(step, model)
            outs = []
            for target in (sub, twin):
                if drive_state(target, step, model):
                    continue
                if name == "set_scene":
                    target.set_scene(model.scene_now())
                    if target is twin:
                        target.request_reset()              # what set_scene promises, said aloud
                elif name == "reseed":
                    target.reseed(step[1])
                elif name == "update_triangles":
                    target.update_triangles(records, step[1])
                    if target is twin:
                        target.set_camera(model.camera)     # what update_triangles promises: camera rows stale, a reset
                elif name == "features_and_denoise":
                    features = target.features()
                    if target.world > 1:
                        for r in target.ranks:
                            with pytest.raises(ptss.PtssError, match="needs the whole frame"):
                                r.denoise()
                        outs.append((features, None))
                    else:
                        outs.append((features, target.denoise()))
            if name == "features_and_denoise":
                assert outs[0][0].tobytes() == outs[1][0].tobytes(), (what, "features")
                if outs[0][1] is not None:
                    assert outs[0][1] == outs[1][1], (what, "denoised")
        sub.synchronize()
        what = (cfg, seed, "end")
        assert np.array_equal(sub.live_counts(), twin.live_counts()), what
        want = subject_snapshot(twin)
        snapshot_equal(sub, want, what)
        assert np.array_equal(sub.pixels(), display_of(sub.accumulator(), model.samples_held())), (what, "samples held")
        assert sub.total_ray_bounces() == twin.total_ray_bounces(), what
        assert sub.per_rank(lambda r: r.update_rejected()) == [model.bad_records] * sub.world, what
        assert twin.per_rank(lambda r: r.update_rejected()) == [model.bad_records], what
        rays = query_rays(model.triangles_now(), w, h)
        fresh = ptss.Renderer(model.scene_now(), w, h, max_iterations=bounces, every_sphere_loop=True)
        try:
            hits, verdicts = fresh.intersect(rays).tobytes(), fresh.occluded(rays).tobytes()
        finally:
            fresh.close()
        for r in sub.ranks:
            assert r.intersect(rays).tobytes() == hits, what
            assert r.occluded(rays).tobytes() == verdicts, what
        assert sub.guard_timeouts() == 0 and twin.guard_timeouts() == 0, what
    finally:
        for x in (sub, twin, follower):
            if x is not None:
                x.close()


@pytest.mark.parametrize("seed", SCRIPT_SEEDS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_random_scripts(cfg, seed):
    t = time.perf_counter()
    run_script(cfg, seed)
    print(f"live-context script {cfg} seed {seed}: {time.perf_counter() - t:.2f} s")
