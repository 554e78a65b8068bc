"""The harness of tests/test_gpu_live_context.py checked on its own, without a GPU (tests/live_context_common.py): the script
generator is deterministic, legal and uses its whole vocabulary; the matrix enumerates the pairs it claims; the Model mirrors
camera, mode, maxIterations and reset as the oracle takes them; and every sharded script and chain keeps the oracle's frame-wide
live count above the loop guard. A failure of the GPU module with these green is the product's, not the harness's."""
import numpy as np
import pytest

import ptss
from live_context_common import (CHAIN_CONFIGS, CONFIGS, FRAME, KINDS, MESH, PAIR_CONFIGS, SCRIPT_SEEDS, SEED1, SEED2, SHARDED_BOUNCES,
                                 VOCABULARY, Follower, Model, Reference, above_guard, bounces_of, chain, display_of, drive_state,
                                 make_script, oracle_snapshot, ordered_pairs, pair_frame, replay_on_oracle, samples_of, script_faults,
                                 sharded)


def test_the_generator_is_deterministic_per_seed():
    for cfg in CONFIGS:
        scripts = [make_script(cfg, seed) for seed in SCRIPT_SEEDS]
        assert scripts == [make_script(cfg, seed) for seed in SCRIPT_SEEDS]
        assert len({repr(s) for s in scripts}) == len(SCRIPT_SEEDS), cfg          # six different scripts
    assert make_script("base", 0) != make_script("lanes2_ordered", 0)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_scripts_are_legal(cfg):
    for seed in SCRIPT_SEEDS:
        script = make_script(cfg, seed)
        assert script_faults(script, cfg) == [], (seed, script)
        assert 12 <= len(script) - 1 <= 16
        kind, targets = script[0][1], []
        for step in script[1:]:
            if step[0] == "set_scene":
                assert step[1] != kind and step[1] in KINDS
                kind = step[1]
                targets.append(kind)
            if step[0] == "update_triangles":
                assert kind == MESH, (seed, step)            # legal only while the current scene is the mesh
                first, count, phase, bad = step[1:]
                assert 0 <= first and count >= 1 and first + count <= 530 and (bad is None or 0 <= bad < count)
            if step[0] == "max_iterations":
                assert 1 <= step[1] <= 6
            if step[0] == "frames":
                assert 1 <= step[1] <= 3
        assert len(set(targets)) >= 2 and any(s[0] == "reseed" for s in script)


def test_script_faults_sees_what_is_illegal():
    good = make_script("base", 1)
    assert script_faults(good, "base") == []
    assert script_faults([s for s in good if s[0] != "reseed"], "base")
    assert script_faults([good[0], ("update_triangles", 0, 10, 0.5, None)] + good[1:], "base") or good[0][1] == MESH
    assert script_faults(good + [("bogus",), ("frames", 1)], "base")
    assert script_faults(good[:-1] + [("frames", 4)], "base")
    assert script_faults([good[0], ("camera_far",), ("frames", 1)] + good[1:], "tiles3")


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_six_seeds_use_the_whole_vocabulary_and_one_bad_record(cfg):
    scripts = [make_script(cfg, seed) for seed in SCRIPT_SEEDS]
    used = {step[0] for s in scripts for step in s[1:]}
    assert used == set(VOCABULARY)
    bad = [sum(1 for step in s if step[0] == "update_triangles" and step[4] is not None) for s in scripts]
    assert sorted(bad) == [0] * 5 + [1]                       # one script per configuration sends one refused record
    for s in scripts:
        steps = [step[0] for step in s[1:]]
        follows = lambda name: [steps[k + 1:k + 3] for k, n in enumerate(steps) if n == name]   # noqa: E731
        if sharded(cfg):                                       # a sharded script reseeds behind every scene change, then renders
            assert all(f[0] == "reseed" for f in follows("set_scene") + follows("update_triangles"))
            assert not follows("update_triangles") or follows("update_triangles")[0] == ["reseed", "frames"]
        else:                                                  # set_scene without a reseed, and a frame that only ITS reset precedes
            assert ["frames"] in [f[:1] for f in follows("set_scene")]
            assert not follows("update_triangles") or follows("update_triangles")[0][:1] == ["frames"]


def test_the_matrix_is_the_stated_one():
    pairs = ordered_pairs()
    assert len(pairs) == len(set(pairs)) == 42 and all(a != b and a in KINDS and b in KINDS for a, b in pairs)
    assert set(pairs) == {(a, b) for a in KINDS for b in KINDS if a != b}
    assert PAIR_CONFIGS == ("one_launch", "lanes3_free")
    assert set(CHAIN_CONFIGS) == set(CONFIGS) - set(PAIR_CONFIGS) and len(CONFIGS) == 8 and len(KINDS) == 7
    for cfg in CHAIN_CONFIGS:
        legs = chain(cfg)
        assert len(legs) == 7
        assert sorted(a for a, _ in legs) == sorted(b for _, b in legs) == sorted(KINDS)      # leaves and enters every kind once
        assert all(a != b for a, b in legs)
        assert all(legs[i][1] == legs[(i + 1) % 7][0] for i in range(7))                     # closed
    assert {leg for cfg in CHAIN_CONFIGS for leg in chain(cfg)} == set(pairs)                # the six chains: every pair once more
    for a, b in pairs:
        w, h = pair_frame(a, b)
        assert w <= 64 and h <= 48
        assert (w, h) == ((25, 15) if "accel_4500" in (a, b) else (48, 32) if MESH in (a, b) else FRAME)


def without_scene_changes(script):
    return [s for s in script if s[0] not in ("set_scene", "update_triangles")]


@pytest.mark.parametrize("cfg", ["base", "tiles3", "one_launch_s3"])   # S = 1, 2, 3
def test_the_model_mirrors_what_the_oracle_is_told(cfg):
    """Scripts without their scene changes, split at the last reseed. Oracle A is created with that reseed's seed (what a reseed
    leaves: fresh streams and a reset, nothing of the frames before) and told every camera, mode, bounce-count and reset step of the
    script ONE BY ONE from its creation on; oracle B is the one the Model builds at the checkpoint from what it has noted. Both then
    follow the rest of the script: equal live counts, accumulators, pixels and RNG records after every frame step, and the sums hold
    the number of samples the Model says."""
    w, h, kind = 23, 17, "bounded"   # (what is mirrored does not depend on the scene: the cheapest one)
    for seed in SCRIPT_SEEDS:
        script = without_scene_changes(make_script(cfg, seed))
        steps = script[1:]
        last = max(k for k, s in enumerate(steps) if s[0] == "reseed")
        model = Model(kind, SEED1, w, h, bounces_of(cfg), samples_of(cfg))
        told = Model(kind, steps[last][1], w, h, bounces_of(cfg), samples_of(cfg))   # (A's own camera, moved key by key)
        a = told.oracle()
        b = None
        try:
            for k, step in enumerate(steps):
                if step[0] in ("frames", "ticks_jump"):
                    for tick in model.ticks_of(step):
                        model.frame(tick)
                        if b is not None:
                            a.generate_frame(tick)
                            b.o.generate_frame(tick)
                            assert np.array_equal(a.live_counts(), b.o.live_counts()), (seed, k)
                            assert np.array_equal(display_of(b.o.accumulator(), model.samples_held()), b.o.pixels()), (seed, k)
                    if b is not None:
                        sa, sb = oracle_snapshot(a, w * h, model.samples), oracle_snapshot(b.o, w * h, model.samples)
                        for name in ("accumulator", "pixels", "float_sum"):
                            assert np.array_equal(sa[name], sb[name], equal_nan=name == "float_sum"), (seed, k, name)
                        assert all(np.array_equal(sa["rng"][key], sb["rng"][key]) for key in sa["rng"]), (seed, k)
                    continue
                model.note(step)
                told.note(step)
                if step[0] != "reseed":
                    drive_state(a, step, told)
                if k == last:
                    b = Follower(model)
                elif b is not None:
                    b.step(step, model)
            assert b is not None and model.last_tick > 0
        finally:
            a.close()
            if b is not None:
                b.close()


def test_the_model_applies_refused_records_on_the_host():
    model = Model(MESH, SEED1, 8, 8, 4, 1)
    before = model.triangles_now()
    sent = model.records_of(("update_triangles", 10, 20, 0.7, 3))
    now = model.triangles_now()
    assert model.bad_records == 1 and len(sent) == 20 and np.isnan(sent["vertex1"][3, 1])
    assert now[13].tobytes() == before[13].tobytes()                           # the refused record keeps its old geometry
    assert np.array_equal(now[:10], before[:10]) and np.array_equal(now[30:], before[30:])
    moved = np.r_[10:13, 14:30]
    assert now[moved].tobytes() == sent[np.r_[0:3, 4:20]].tobytes() and not np.array_equal(now[moved], before[moved])
    assert model.scene_now().desc.numTriangles == 530 and np.isfinite(now["vertex1"]).all()


SHARDED = [c for c in CONFIGS if sharded(c)]


@pytest.mark.parametrize("seed", SCRIPT_SEEDS)
@pytest.mark.parametrize("cfg", SHARDED)
def test_sharded_scripts_stay_above_the_loop_guard(cfg, seed):
    """A sharded context never stops early on the whole-frame live count: every frame of a tiles3 script must keep the
    oracle's frame-wide count above 128 before the last bounce, or shards and oracle would differ by design. Every frame of such a
    script is one the oracle can follow."""
    assert SHARDED == ["tiles3"]
    script = make_script(cfg, seed)
    frames = replay_on_oracle(script, cfg)
    ticks = sum(s[1] if s[0] == "frames" else 1 for s in script[1:] if s[0] in ("frames", "ticks_jump"))
    assert len(frames) == ticks                                        # none without an oracle
    for k, tick, live in frames:
        assert above_guard(live), (seed, k, tick, live)


@pytest.mark.parametrize("cfg", SHARDED)
def test_the_sharded_chain_stays_above_the_loop_guard(cfg):
    """The same for every frame of the tiles3 chain of the matrix (the seeds and frame counts of test_gpu_live_context.py's chain)."""
    w, h = FRAME
    for i, (a, b) in enumerate(chain(cfg)):
        for kind, seed, n in ((a, SEED1 if i == 0 else SEED2 + i - 1, 2 if i == 0 else 5), (b, SEED2 + i, 3)):
            ref = Reference.of(kind, w, h, SHARDED_BOUNCES, samples_of(cfg), seed)
            for f in range(1, n + 1):
                assert above_guard(ref.after(f)["live"]), (a, b, kind, f, ref.after(f)["live"])


def test_the_far_camera_leaves_every_scene_at_bounce_zero():
    """Why a sharded script's frames at the FAR camera are one-bounce frames: nothing is live behind bounce 0."""
    from live_context_common import far_camera, scene
    import oracle
    for kind in KINDS:
        o = oracle.Oracle(scene(kind).desc, 16, 12, max_iterations=3)
        o.set_camera(far_camera())
        o.generate_frame()
        assert list(o.live_counts()) == [16 * 12, 0, 0], kind
        o.close()
    assert ptss.default_camera().position.z == 0.0
