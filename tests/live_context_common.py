"""Scenes, configurations, scripts and the model shared by tests/test_gpu_live_context.py (GPU) and
tests/test_live_context_scripts.py (CPU): scene updates on LIVE contexts (ptss_set_scene, ptss_update_triangles, ptss_reseed;
DESIGN.md §3.18) in every context configuration.

A script is a list of steps (tuples, the vocabulary below). Three things follow it:

  the subject   the context under test, in one of CONFIGS (three rank contexts for "tiles3", reassembled as tests/test_gpu_tiles.py does);
  the twin      a "base" context with the same sample lanes and frame size, unsharded. Every configuration is bit-exact to the same
                oracle, so subject and twin must agree after every step, also where no oracle exists (after a set_scene without a
                reseed the random streams continue, and the oracle cannot change scene in mid-stream). The twin STATES what the API
                promises the subject does by itself: it calls request_reset() behind set_scene and set_camera(the current camera)
                behind update_triangles (include/ptss.h: "sets the reset flag and marks the camera rows stale") — no-ops in a correct
                library, so a subject that forgets either differs from its twin although both run the same library;
  the Model     what a FRESH context would need: scene (with the deformed triangles applied on the host), seed, camera, mode,
                maxIterations, and where the accumulation was last reset. At a checkpoint (a reseed; creation is one too) it builds
                oracle.Oracle(scene_now, seed_now) with that camera and mode, which then follows the script until the next scene
                change. Independently of any library it knows how many samples the sums hold (display_of)."""
import ctypes as C
import functools

import numpy as np

import oracle
import ptss
import tiles
from ptss_types import Triangle
from scene_update_common import deform, m530
from test_gpu_kernel_coverage import FAR, SCENES

KINDS = ("bounded", "pairs", "plain", "bounded_padded", "m530", "accel_300", "accel_4500")   # one scene per image kind
MESH = "m530"                                                                                 # the only kind update_triangles accepts
MIN_LIVE = 128                                                                                # CudaTracer.cu:622 `numRays > 128`

CONFIGS = {
    "base": dict(float_accumulator=True),
    "lanes2_ordered": dict(frame_lanes=2),
    "lanes3_free": dict(frame_lanes=3, lanes_free_run=True),
    "lanes2_free_s3": dict(frame_lanes=2, lanes_free_run=True, samples_per_pass=3, float_accumulator=True),   # stagedTwice
    "one_launch": dict(one_launch_frames=1),
    "one_launch_s3": dict(one_launch_frames=1, samples_per_pass=3),
    "tiles3": dict(tile_world=3, band_rows=4, samples_per_pass=2),
    "async_stream": dict(sync_each_frame=False, frame_lanes=2),   # + a torch side stream through set_stream (Subject)
}
PAIR_CONFIGS = ("one_launch", "lanes3_free")   # the two that keep cross-frame device counters: every ordered pair of kinds
CHAIN_CONFIGS = tuple(c for c in CONFIGS if c not in PAIR_CONFIGS)

# Frames. One context keeps its size, so a chain or a script that may visit every kind has one size for all of them: 61 x 47 (12
# tiles, the last one partial; 12 row bands of 4 for tiles3, the last of 3 rows), where the oracle's slowest kind (accel_4500) takes
# 0.1 s per frame. A pair of the matrix that holds accel_4500 or m530 keeps the size the older tests give that scene.
FRAME = (61, 47)
PAIR_FRAME = {"accel_4500": (25, 15), MESH: (48, 32)}
BOUNCES, SHARDED_BOUNCES = 4, 3      # tiles3: the frame-wide live count must stay above 128 before the last bounce
SEED1, SEED2 = 0x5EED, 0xC0FFEE
SCRIPT_SEEDS = tuple(range(6))

VOCABULARY = ("frames", "ticks_jump", "camera", "camera_far", "camera_home", "mode", "max_iterations", "request_reset", "set_scene",
              "reseed", "update_triangles", "features_and_denoise")
BAD_RECORD_SEED = VOCABULARY.index("update_triangles") % 6   # the seed that is given update_triangles sends the refused record
CAMERA_KEYS = "wasdqezxcv"   # the reference's movement keys (CudaTracer.cu:822-870)


def samples_of(cfg):
    return CONFIGS[cfg].get("samples_per_pass", 1)


def sharded(cfg):
    return CONFIGS[cfg].get("tile_world", 1) > 1


@functools.lru_cache(maxsize=None)
def scene(kind):
    """The scene of a kind; built once (a context copies the arrays it is given)."""
    return m530() if kind == MESH else SCENES[kind]()


def triangles_of(s):
    """(T,) TRIANGLE_DTYPE copy of a scene description's triangle table."""
    d = s.desc
    return np.frombuffer(C.string_at(d.triangles, d.numTriangles * C.sizeof(Triangle)), dtype=ptss.TRIANGLE_DTYPE).copy()


def far_camera():
    cam = ptss.default_camera()
    cam.position.x, cam.position.y, cam.position.z = FAR
    return cam


def display_of(acc, samples):
    """writeToPixelsKernel's display value (CudaTracer.cu:94-98) of an accumulator that holds `samples` samples per pixel."""
    inv = np.float32(1.0) / np.float32(samples)
    rgb = (acc.astype(np.float32) * inv + np.float32(0.5)).astype(np.uint32).astype(np.uint8)
    return np.concatenate([rgb, np.full((acc.shape[0], 1), 255, dtype=np.uint8)], axis=1)


def sampled_pixels(n):
    return (0, n // 3, n - 1)


# ---- the transition matrix ------------------------------------------------------------------------------------------------------
def ordered_pairs():
    return [(a, b) for a in KINDS for b in KINDS if a != b]


def chain(cfg):
    """A closed chain over KINDS that leaves and enters every kind once. Configuration number j (1..6) strides by j, so the six
    chains together walk every ordered pair of kinds once more."""
    stride = CHAIN_CONFIGS.index(cfg) + 1
    order = [KINDS[(i * stride) % len(KINDS)] for i in range(len(KINDS))]
    return list(zip(order, order[1:] + order[:1]))


def pair_frame(a, b):
    for kind in ("accel_4500", MESH):
        if kind in (a, b):
            return PAIR_FRAME[kind]
    return FRAME


def bounces_of(cfg):
    return SHARDED_BOUNCES if sharded(cfg) else BOUNCES


# ---- scripts --------------------------------------------------------------------------------------------------------------------
def make_script(cfg, seed):
    """12-16 steps for one configuration and seed; deterministic. At least two set_scene steps to different kinds and one reseed;
    the six seeds of a configuration use the whole vocabulary between them (seed k is given VOCABULARY[k::6]), and one seed
    (BAD_RECORD_SEED) sends one record with a non-finite vertex. script[0] is ("start", kind), the scene the context is created on,
    and no step. A sharded configuration's scripts keep every frame comparable with the oracle and above the live-count guard: a
    reseed follows every scene change at once, bounce counts stay at most 3, and frames at the FAR camera (every ray leaves the
    scene at bounce 0) are one-bounce frames."""
    for attempt in range(200):
        rng = np.random.default_rng([0x11FE, list(CONFIGS).index(cfg), seed, attempt])
        script = _draw_script(rng, cfg, seed)
        if 12 <= len(script) - 1 <= 16 and not script_faults(script, cfg):
            return script
    raise AssertionError(f"no script for {cfg}, seed {seed}")


def _draw_script(rng, cfg, seed):
    shard = sharded(cfg)
    length = int(rng.integers(12, 17))
    wanted = ["set_scene", "set_scene", "reseed"] + list(VOCABULARY[seed % 6::6])
    fillers = ["frames"] * 4 + ["camera", "mode", "max_iterations", "request_reset", "set_scene", "reseed", "ticks_jump",
                                "features_and_denoise", "camera_far", "camera_home", "update_triangles"]
    while len(wanted) < length - 4:
        wanted.append(str(rng.choice(fillers)))
    wanted = [wanted[i] for i in rng.permutation(len(wanted))]
    st = dict(kind=str(rng.choice(KINDS)), far=False, mode=True, bounces=bounces_of(cfg), bad_sent=False, framed=set())
    script = [("start", st["kind"])]

    def one_bounce():
        return not st["mode"] or st["bounces"] == 1

    def emit(step):
        script.append(step)
        name = step[0]
        if name == "set_scene":
            st["kind"] = step[1]
        elif name == "camera_far":
            st["far"] = True
        elif name == "camera_home":
            st["far"] = False
        elif name == "mode":
            st["mode"] = step[1]
        elif name == "max_iterations":
            st["bounces"] = step[1]
        if shard and name in ("set_scene", "update_triangles"):
            emit(("reseed", int(rng.integers(1, 2 ** 31))))
        # the first scene change of either kind is followed by a frame at once: nothing else may supply the reset, or the
        # refreshed camera rows, that the call itself owes
        if name in ("set_scene", "update_triangles") and name not in st["framed"]:
            st["framed"].add(name)
            if shard and st["far"] and not one_bounce():
                emit(("camera_home",))
            emit(("frames", int(rng.integers(1, 3))))

    for name in wanted:
        if name in ("frames", "ticks_jump"):
            if shard and st["far"] and not one_bounce():
                emit(("camera_home",))
            emit(("frames", int(rng.integers(1, 4))) if name == "frames" else ("ticks_jump", int(rng.integers(2, 6))))
        elif name == "camera":
            emit(("camera", "".join(str(k) for k in rng.choice(list(CAMERA_KEYS), size=3))))
        elif name == "camera_far":
            if shard and not one_bounce():
                emit(("mode", False))
            emit(("camera_far",))
            emit(("frames", 1))
        elif name == "mode":
            emit(("mode", not st["mode"]))
        elif name == "max_iterations":
            emit(("max_iterations", int(rng.integers(1, (SHARDED_BOUNCES if shard else 6) + 1))))
        elif name == "set_scene":
            emit(("set_scene", str(rng.choice([k for k in KINDS if k != st["kind"]]))))
        elif name == "reseed":
            emit(("reseed", int(rng.integers(1, 2 ** 31))))
        elif name == "update_triangles":
            if st["kind"] != MESH:
                emit(("set_scene", MESH))
            first = int(rng.integers(0, 400))
            count = int(rng.integers(1, 530 - first + 1))
            bad = None
            if seed % 6 == BAD_RECORD_SEED and not st["bad_sent"]:
                bad, st["bad_sent"] = int(rng.integers(0, count)), True
            emit(("update_triangles", first, count, round(float(rng.uniform(0.2, 1.2)), 3), bad))
        else:
            emit((name,))
    if shard and st["far"] and not one_bounce():
        emit(("camera_home",))
    emit(("frames", 2))
    return script


def script_faults(script, cfg):
    """What is wrong with a script, as a list of strings (empty: legal). Independent of how make_script builds one."""
    faults = []
    start, steps = script[0], script[1:]
    if start[0] != "start" or start[1] not in KINDS:
        faults.append("no start kind")
    kind, far, mode, bounces, dirty = start[1], False, True, bounces_of(cfg), False
    targets, reseeds = [], 0
    for k, step in enumerate(steps):
        name = step[0]
        if name not in VOCABULARY:
            faults.append(f"step {k}: {name} is not in the vocabulary")
        elif name == "frames" and not 1 <= step[1] <= 3:
            faults.append(f"step {k}: frames({step[1]})")
        elif name == "ticks_jump" and step[1] < 2:
            faults.append(f"step {k}: a jump to the next tick is no jump")
        elif name == "camera" and (not step[1] or set(step[1]) - set(CAMERA_KEYS)):
            faults.append(f"step {k}: camera keys {step[1]!r}")
        elif name == "max_iterations" and not 1 <= step[1] <= (SHARDED_BOUNCES if sharded(cfg) else 6):
            faults.append(f"step {k}: max_iterations({step[1]})")
        elif name == "set_scene":
            if step[1] not in KINDS or step[1] == kind:
                faults.append(f"step {k}: set_scene({step[1]}) on {kind}")
            kind = step[1]
            targets.append(kind)
            dirty = True
        elif name == "update_triangles":
            first, count, _, bad = step[1:]
            if kind != MESH:
                faults.append(f"step {k}: update_triangles on {kind}")
            if first < 0 or count < 1 or first + count > 530 or (bad is not None and not 0 <= bad < count):
                faults.append(f"step {k}: update_triangles range {step[1:]}")
            dirty = True
        elif name == "reseed":
            reseeds += 1
            dirty = False
        if name == "camera_far":
            far = True
        if name == "camera_home":
            far = False
        if name == "mode":
            mode = bool(step[1])
        if name == "max_iterations":
            bounces = step[1]
        if sharded(cfg) and name in ("frames", "ticks_jump"):
            if dirty:
                faults.append(f"step {k}: a sharded frame the oracle cannot follow")
            if far and mode and bounces > 1:
                faults.append(f"step {k}: a sharded frame of {bounces} bounces at the FAR camera")
    if len(set(targets)) < 2:
        faults.append("fewer than two set_scene steps to different kinds")
    if not reseeds:
        faults.append("no reseed")
    if not steps or steps[-1][0] != "frames":
        faults.append("does not end on frames")
    return faults


# ---- the model ------------------------------------------------------------------------------------------------------------------
class Model:
    """What a fresh context would need to be where the live one is, and how many samples its sums hold."""

    def __init__(self, kind, seed, width, height, max_iterations, samples):
        self.kind, self.seed = kind, seed
        self.width, self.height, self.samples = width, height, samples
        self.triangles = None            # the mesh's table once update_triangles has moved it (host-side mirror)
        self.camera = ptss.default_camera()
        self.mode = True
        self.max_iterations = max_iterations
        self.next_tick = 1               # GPUAnimBitmap::idle_func's counter
        self.reset_pending = True        # CudaTracer.cu:602-608
        self.last_reset_tick = 0
        self.last_tick = 0
        self.bad_records = 0

    def scene_now(self):
        base = scene(self.kind)
        return base if self.triangles is None else base.with_triangles(self.triangles)

    def triangles_now(self):
        return triangles_of(scene(self.kind)) if self.triangles is None else self.triangles

    def bounces(self):
        return self.max_iterations if self.mode else 1

    def samples_held(self):
        """Samples per pixel in the sums after the latest frame."""
        return self.samples * (self.last_tick - self.last_reset_tick + 1)

    def ticks_of(self, step):
        """The tick numbers a frame step passes to generate_frame."""
        if step[0] == "frames":
            return list(range(self.next_tick, self.next_tick + step[1]))
        return [self.next_tick + step[1]]

    def frame(self, tick):
        if self.reset_pending:
            self.last_reset_tick, self.reset_pending = tick, False
        self.last_tick, self.next_tick = tick, tick + 1

    def records_of(self, step):
        """update_triangles(first, count, phase, bad) -> the records to send; the table a fresh context would be created with is
        updated on the host: the refused record keeps its old geometry."""
        first, count, phase, bad = step[1:]
        now = self.triangles_now()
        new = deform(now, phase)[first:first + count]
        applied = now.copy()
        applied[first:first + count] = new
        if bad is not None:
            new["vertex1"][bad, 1] = np.nan
            applied[first + bad] = now[first + bad]
            self.bad_records += 1
        self.triangles = applied
        return new

    def note(self, step):
        """The state a step leaves (frames: see frame())."""
        name = step[0]
        if name == "camera":
            for key in step[1]:
                ptss.move_camera(self.camera, key)
        elif name == "camera_far":
            self.camera = far_camera()
        elif name == "camera_home":
            self.camera = ptss.default_camera()
        elif name == "mode":
            self.mode = bool(step[1])
        elif name == "max_iterations":
            self.max_iterations = step[1]
        elif name == "set_scene":
            self.kind, self.triangles = step[1], None
        elif name == "reseed":
            self.seed = step[1]
        if name in ("camera", "camera_far", "camera_home", "mode", "request_reset", "set_scene", "update_triangles", "reseed"):
            self.reset_pending = True

    def oracle(self):
        """The oracle of a fresh context at this point (valid at a checkpoint: the random streams are a fresh context's)."""
        o = oracle.Oracle(self.scene_now().desc, self.width, self.height, max_iterations=self.max_iterations,
                          samples_per_pass=self.samples, seed=self.seed)
        o.set_camera(self.camera)
        o.set_mode(self.mode)
        return o


def drive_state(target, step, model):
    """The steps a renderer and an oracle both take: camera, mode, bounce count, reset. `model` has noted the step already."""
    name = step[0]
    if name in ("camera", "camera_far", "camera_home"):
        target.set_camera(model.camera)
    elif name == "mode":
        target.set_mode(step[1])
    elif name == "max_iterations":
        target.set_max_iterations(step[1])
    elif name == "request_reset":
        target.request_reset()
    else:
        return False
    return True


def above_guard(live):
    """tiles3's precondition on the oracle's live counts of one frame (one entry per bounce, 0 from where the guard stopped)."""
    return bool((np.asarray(live) > MIN_LIVE).all())


class Follower:
    """The oracle that can follow the context at the moment, if any: built by the Model at every checkpoint, dropped at a scene
    change (its random streams would have to continue from the old scene's)."""

    def __init__(self, model):
        self.o = model.oracle()

    def step(self, step, model):
        """A step that is no frame; `model` has noted it already."""
        if step[0] in ("set_scene", "update_triangles", "reseed"):
            self.close()
            if step[0] == "reseed":
                self.o = model.oracle()
        elif self.o is not None:
            drive_state(self.o, step, model)

    def frame(self, tick):
        if self.o is not None:
            self.o.generate_frame(tick)
        return self.o

    def close(self):
        if self.o is not None:
            self.o.close()
            self.o = None


def replay_on_oracle(script, cfg, width=None, height=None):
    """The oracle's side of a script alone (no GPU): [(step index, tick, live counts)] of every frame an oracle can follow."""
    w, h = (width, height) if width else FRAME
    model = Model(script[0][1], SEED1, w, h, bounces_of(cfg), samples_of(cfg))
    follower, out = Follower(model), []
    try:
        for k, step in enumerate(script[1:]):
            if step[0] in ("frames", "ticks_jump"):
                for tick in model.ticks_of(step):
                    model.frame(tick)
                    if follower.frame(tick) is not None:
                        out.append((k, tick, follower.o.live_counts()))
                continue
            if step[0] == "update_triangles":
                model.records_of(step)
            model.note(step)
            follower.step(step, model)
    finally:
        follower.close()
    return out


# ---- references computed once -----------------------------------------------------------------------------------------------------
class Reference:
    """The oracle of a fresh context on one kind, frame by frame, computed once per (kind, size, bounces, S, seed) and shared by every
    leg of the matrix that needs it; snapshots are never changed."""
    _cache = {}

    @classmethod
    def of(cls, kind, w, h, bounces, S, seed):
        key = (kind, w, h, bounces, S, seed)
        if key not in cls._cache:
            cls._cache[key] = cls(*key)
        return cls._cache[key]

    def __init__(self, kind, w, h, bounces, S, seed):
        self.n, self.S = w * h, S
        self._o = oracle.Oracle(scene(kind).desc, w, h, max_iterations=bounces, samples_per_pass=S, seed=seed)
        self._frames = []

    def after(self, frames):
        """Everything a fresh context holds after `frames` frames."""
        while len(self._frames) < frames:
            o = self._o
            o.generate_frame()
            snap = oracle_snapshot(o, self.n, self.S)
            for v in snap.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            self._frames.append(snap)
        return self._frames[frames - 1]


def oracle_snapshot(o, n, S):
    return dict(live=o.live_counts(), accumulator=o.accumulator(), pixels=o.pixels(), float_sum=o.float_sum(),
                rng={(p, lane): o.rng_state(p, lane) for p in sampled_pixels(n) for lane in range(S)})


# ---- the contexts -----------------------------------------------------------------------------------------------------------------
class Subject:
    """The context(s) of one configuration behind one interface in FRAME order: one ptss.Renderer, or one per rank for a sharded
    configuration. close() in a finally."""

    def __init__(self, cfg, scene_, width, height, max_iterations, seed, **extra):
        args = dict(CONFIGS[cfg], **extra)
        self.cfg, self.width, self.height, self.n = cfg, width, height, width * height
        self.S = args.get("samples_per_pass", 1)
        self.world, self.band = args.pop("tile_world", 1), args.get("band_rows", 8)
        self.has_float_sum = bool(args.get("float_accumulator"))
        self.ranks, self.stream, self._keep = [], None, []
        try:
            for k in range(self.world):
                self.ranks.append(ptss.Renderer(scene_, width, height, max_iterations=max_iterations, seed=seed, tile_rank=k,
                                                tile_world=self.world, **args))
            if cfg == "async_stream":
                import torch
                self.stream = torch.cuda.Stream()
                for r in self.ranks:
                    r.set_stream(self.stream.cuda_stream)
        except BaseException:
            self.close()
            raise

    def close(self):
        for r in self.ranks:
            r.close()
        self.ranks = []
        self._keep = []

    # -- steps
    def generate_frame(self, tick):
        for r in self.ranks:
            r.generate_frame(ticks=tick)

    def set_camera(self, cam):
        for r in self.ranks:
            r.set_camera(cam)

    def set_mode(self, on):
        for r in self.ranks:
            r.set_mode(on)

    def set_max_iterations(self, n):
        for r in self.ranks:
            r.set_max_iterations(n)

    def request_reset(self):
        for r in self.ranks:
            r.request_reset()

    def set_scene(self, scene_):
        for r in self.ranks:
            r.set_scene(scene_)

    def reseed(self, seed):
        for r in self.ranks:
            r.reseed(seed)

    def update_triangles(self, records, first):
        if self.stream is None:
            for r in self.ranks:
                r.update_triangles(records, first=first)
            return
        import torch
        with torch.cuda.stream(self.stream):   # uploaded and consumed on the context's stream: nothing waits on the host
            t = torch.from_numpy(records.view(np.float32).reshape(-1, 19).copy()).cuda()
        self._keep.append(t)
        for r in self.ranks:
            r.update_triangles(t, first=first, stream=self.stream.cuda_stream)

    def features(self):
        """The first-hit features of the current camera, in frame order, as words."""
        feats = [r.features().view(np.uint32).reshape(-1, 8) for r in self.ranks]
        return self._untile(feats)

    def denoise(self):
        """The denoised display bytes of every rank's context."""
        return [r.denoise().tobytes() for r in self.ranks]

    def synchronize(self):
        for r in self.ranks:
            r.synchronize()

    # -- read-backs, in frame order
    def _untile(self, parts):
        return parts[0] if self.world == 1 else tiles.untile(parts, self.width, self.height, self.band)

    def live_counts(self):
        return sum(r.live_counts().astype(np.uint64) for r in self.ranks).astype(np.uint32)

    def accumulator(self):
        return self._untile([r.accumulator() for r in self.ranks])

    def pixels(self):
        return self._untile([r.pixels() for r in self.ranks])

    def float_sum(self):
        return self._untile([r.float_accumulator() for r in self.ranks])

    def rng_state(self, pixel, lane=0):
        y, x = divmod(pixel, self.width)
        rank = (y // self.band) % self.world if self.world > 1 else 0
        rows = ptss.tile_rows(self.height, self.band, rank, self.world) if self.world > 1 else np.arange(self.height)
        return self.ranks[rank].rng_state(int(np.flatnonzero(rows == y)[0]) * self.width + x, lane)

    def total_ray_bounces(self):
        return sum(r.total_ray_bounces() for r in self.ranks)

    def guard_timeouts(self):
        return sum(r.guard_timeouts() for r in self.ranks)

    def per_rank(self, what):
        """[what(renderer) for every rank]: the queries that are per context (one_launch_frames, launched_kernels, ...)."""
        return [what(r) for r in self.ranks]


def snapshot_equal(sub, want, what, float_sum=None):
    """Accumulator, display pixels, float sums (where the subject has them) and the sampled RNG records against a snapshot."""
    assert np.array_equal(sub.accumulator(), want["accumulator"]), (what, "accumulator")
    assert np.array_equal(sub.pixels(), want["pixels"]), (what, "pixels")
    if sub.has_float_sum if float_sum is None else float_sum:
        assert np.array_equal(sub.float_sum(), want["float_sum"], equal_nan=True), (what, "float sums")
    for (p, lane), state in want["rng"].items():
        assert np.array_equal(sub.rng_state(p, lane), state), (what, "rng", p, lane)


def subject_snapshot(sub):
    return dict(accumulator=sub.accumulator(), pixels=sub.pixels(), float_sum=sub.float_sum() if sub.has_float_sum else None,
                rng={(p, lane): sub.rng_state(p, lane) for p in sampled_pixels(sub.n) for lane in range(sub.S)})


def query_rays(tris, width, height, seed=4):
    """2,048 rays as tests/test_gpu_scene_update.py builds them: 1,024 pixel-centre camera rays (every few pixels of the frame), and
    1,024 rays leaving surface points in random directions, some not unit, half of them with a finite tmax."""
    rng = np.random.default_rng(seed)
    cam = ptss.camera_rays(ptss.default_camera(), width, height)
    cam = cam[np.linspace(0, len(cam) - 1, min(1024, len(cam))).astype(np.int64)]
    n = 2048 - len(cam)
    k = rng.integers(0, len(tris), n)
    b = rng.dirichlet((1, 1, 1), n).astype(np.float32)
    p = b[:, :1] * tris["vertex0"][k] + b[:, 1:2] * tris["vertex1"][k] + b[:, 2:] * tris["vertex2"][k]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[::5] *= rng.uniform(0.3, 3.0, (len(d[::5]), 1))
    tmax = np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0.1, 10.0, n))
    return np.concatenate([cam, ptss.make_rays(p, d.astype(np.float32), tmax)])
