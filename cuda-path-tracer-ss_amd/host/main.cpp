// main.cpp — the reference's main() (CudaTracer/CudaTracer.cu:649-743) on the MI355X drop-in.
// Same sequence: build the Scene, make ProgramData + GPUAnimBitmap, hand the scene vectors to the
// device (one ptss_create instead of cudaMalloc x8 + cudaMemcpy x5 + curandSetupKernel), then
// bitmap.anim_and_exit(generateFrame, NULL, Key). The reference ignores argv; this build accepts
// optional overrides with the reference's values as defaults:
//   ptss_main [--preset default] [--size 512x512] [--ticks 16] [--bounces 15] [--seed N] [--samples-per-pass S]
//             [--keys "wwd f"] [--out image.tga] [--quiet]
//             [--obj model.obj [--obj-at x,y,z,scale]]...   Wavefront OBJ models added to the preset (Scene::addObjModel), each
//                                   placed by the --obj-at after it (default: where the file puts it), in the preset's first material
//             [--gpus N]            the frame sharded by pixel tile over N GPUs of this node, one RCCL gather (MultiGpu.cpp)
//             [--emulate-gpus N]    the same N shards on device 0, the gather as device copies (rehearsal on a one-GPU box)
//             [--pick x,y]...       after the ticks and --keys: the closest hit of pixel (x, y)'s centre ray (ptss_camera_ray with
//                                   jitter 0.5, 0.5, through ptss_intersect) of the final camera, one line per pick
//             [--denoise [levels]]  with --out image.tga: also image_denoised.tga, the accumulated image through ptss_render_features
//                                   and ptss_denoise (default parameters; levels 0..6 overrides their level count)
//             [--specular-features N]  with --denoise: the filter is guided by the features BEHIND mirrors and glass, the centre ray
//                                   carried through at most N (0..8) perfect reflections and refractions
//                                   (ptss_render_features_specular); 0 writes the bytes of plain --denoise
//             [--temporal]          with --out: the keys of --keys are delivered one at a time, --ticks frames are rendered at the start
//                                   pose and after every key, and the image is carried from pose to pose (ptss_render_features,
//                                   ptss_reproject with the history kept from the previous pose); --out receives the last history
//                                   through ptss_denoise_history (default parameters) instead of the frame's own pixels
//             [--upscale F]         with --out image.tga: also image_upscaled.tga, F (1..4) times the size in each direction: the run traces at
//                                   --size; the frame's pixels — with --temporal the filtered history --out receives, with --denoise the
//                                   denoised image — go through ptss_render_features, ptss_render_features_scaled and ptss_upsample
//             [--film pinhole|thinlens|equirect [--lens radius,focus]]   the screenshot rendered through the film of a path query instead
//                                   of the frame loop: per tick ptss_generate_rays, ptss_trace_paths, ptss_accumulate_paths over the whole
//                                   --size film, streams from ptss_seed_path_rng(--seed); --keys move the camera before the first tick.
//                                   pinhole writes the frame loop's image (while that loop's guard stays silent). With --denoise:
//                                   image_denoised.tga through ptss_ray_features and ptss_denoise_history
//             [--refill]            with --film: the trace through ptss_trace_paths_opt with PTSS_PATHS_REFILL (the same bytes)
//             [--adaptive ROUNDS[,threshold]]   with --film: the --ticks uniform rounds keep second moments (ptss_accumulate_paths_stats;
//                                   the same bytes), then ROUNDS planned rounds of width * height rays each go where ptss_plan_samples
//                                   sends them (minSamples = --ticks, default maxSamples; threshold overrides the default's). Prints
//                                   the final ptss_plan_info. ROUNDS = 0 writes the bytes of the run without the flag
//             [--linear [exposure]] with --film: the samples go into a linear film (ptss_accumulate_paths_linear, default parameters) and
//                                   ptss_resolve_linear with that exposure (default 1) makes the screenshot, image.pfm — the linear means,
//                                   unexposed — beside it and, with --denoise, the history the filter takes. Not with --adaptive
//             [--adaptive-linear ROUNDS[,threshold[,floor]]]   with --linear, with or without --filter, --auto-exposure, --glare and
//                                   --refill: the --ticks uniform rounds keep luminance moments
//                                   (ptss_accumulate_paths_linear_stats; the same film bytes), then ROUNDS planned rounds of width * height rays
//                                   each go where ptss_plan_samples_linear sends them (minSamples = --ticks; threshold and floor override the
//                                   defaults'). With --filter the moments are kept by index pixel, beside ptss_splat_paths. Prints the final
//                                   ptss_plan_info. ROUNDS = 0 writes the bytes of the run without the flag
//             [--filter box|tent|gaussian[,radius[,alpha]]]   with --linear: the film is a filtered one — rounds go through
//                                   ptss_generate_rays_positions, the trace, ptss_splat_paths_homed and, at the end, ptss_resolve_splat
//                                   (radius default 1, alpha default 2). Without it the program's bytes are those of --linear alone
//             [--auto-exposure [key[,rate]]]   with --linear, with or without --filter: the exposure is metered on the device (DESIGN.md
//                                   §3.31) — after each round ptss_meter_linear (ptss_meter_splat) into a zeroed histogram,
//                                   ptss_meter_exposure (default parameters; key default 0.18, rate default 1) and the metered resolve, --linear's
//                                   exposure compensating. Prints the final ptss_meter_state. Without it every byte written is today's
//             [--glare [strength[,threshold[,levels]]]]   with --linear, with or without --filter, --auto-exposure and --refill: highlights bleed
//                                    — after the last round ptss_glare_build over the film (default parameters; strength default
//                                   0.1, threshold default 0, levels default 6) and ptss_resolve_linear_glare (ptss_resolve_splat_glare), with the
//                                   meter's state where --auto-exposure keeps one. Without it every byte written is today's
//             [--tone clamp|reinhard[,white]|filmic [--srgb] [--tone-luminance]]   with --film and --linear, with or without --filter,
//                                   --auto-exposure, --glare, --denoise-linear, --upscale-linear and --refill: the film is shown through a tone curve
//                                    — ptss_tone_build (8 bits: the TGA's depth; white default 4, the default filmic
//                                   coefficients; the 2.2 power unless --srgb) and, after the last round, ptss_resolve_toned with the meter's state
//                                   and the glare pyramid where those options keep them. --tone clamp writes the bytes of the run without it;
//                                   without the flag every byte written is today's
//             [--denoise-linear [levels[,sigmaLuminance]]]   with --linear, with or without --filter, --auto-exposure, --glare and --refill: the
//                                   film is denoised in linear light — the rounds keep the luminance moments
//                                   (ptss_accumulate_paths_linear_stats; with --filter by home pixel), the features are ptss_ray_features of the
//                                   pixel-centre rays, and ptss_denoise_linear (default parameters; levels default 5, sigmaLuminance default 3)
//                                   makes the linear film that --auto-exposure's meter (every round), --glare, the resolve and image.pfm then
//                                   read. Levels 0 and the absent flag write the same bytes
//             [--carry KEYS[,maxHistory]]   with --film and --linear, with or without --filter, --refill, --auto-exposure, --glare and
//                                   --denoise-linear: the film is carried across a camera move — after --keys, --ticks rounds
//                                   with the luminance moments at that pose; the features of the pixel-centre rays; KEYS move the camera; the
//                                   features again; ptss_reproject_linear (default parameters; maxHistory default 64) seeds a new film and new
//                                   moments; --ticks more rounds accumulate into them, and the usual tail runs. Prints the four counters of
//                                   ptss_reproject_linear_info. Not with --adaptive or --adaptive-linear: the combination is left out to keep
//                                   this program's matrix small. Without the flag every byte written is today's
//             [--bake [texelsPerUnit[,samples[,passes]]]]   a light map of the scene's triangles (--obj models included) instead of an image
//                                   (DESIGN.md §3.38): ptss_surface_atlas at --size's width (sides 1 .. 64, texelsPerUnit default 4), streams from
//                                   ptss_seed_path_rng(--seed), then `samples` (default 16) rounds of ptss_generate_rays_surface (cosine) ->
//                                   ptss_trace_paths -> ptss_accumulate_paths_linear indexed by texel, `passes` (default 1) of ptss_dilate_linear,
//                                   ptss_resolve_linear; writes the linear means to --out (default lightmap.pfm) and prints the atlas size
//                                   and the rejected count. Not with --film, --temporal, --denoise, --upscale, --pick, --gpus
//             [--bake-view [nearest|bilinear]]   with --bake: the bake goes through ptss_surface_atlas_blocks, so the spheres
//                                   get texels too (sides up to --size's width / 2 then); after the gutter fills the camera's centre rays
//                                   (ptss_generate_rays, jitter 0; --keys move the camera first) -> ptss_intersect -> ptss_lookup_lightmap with
//                                   modulate and emission (default bilinear) -> ptss_resolve_linear at --size; writes the view's linear means
//                                   next to the map (<out without .pfm>_view.pfm) and prints the four counts. Without the flag --bake writes
//                                   exactly what it wrote before
//             [--view-steps N]      with --bake-view: the view's rays are carried through mirrors and glass for at most N
//                                   (0..8) links — ptss_intersect_chain in place of ptss_intersect — and the rows come from
//                                   ptss_lookup_lightmap_chain, tinted by what the chain let through; also prints the links followed. N = 0 (the
//                                   default) is the path above and writes its bytes
//             [--upscale-linear F]  with --film and --linear, with or without --filter, --refill, --denoise-linear, --auto-exposure and --glare:
//                                   the film is traced (and denoised) at the given size and upsampled in linear light to F (1..4) times the
//                                   size — the features are ptss_ray_features of the centre rays of the same film camera at
//                                   both sizes, ptss_upsample_linear (default parameters; the wrap flag for --film equirect) makes the large
//                                   linear film, and --auto-exposure's meter (every round), --glare, the resolve, image.tga and image.pfm work
//                                   on it: both files are F times the size. Prints the three counters of ptss_upsample_linear_info. Not with
//                                   --carry, --adaptive-linear or --denoise (the 8-bit filter): left out to keep this program's matrix small
#include <hip/hip_runtime_api.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "CudaTracer.h"
#include "HostOps.h"
#include "ptsurface.h"

int main(int argc, char* argv[]) {
    std::string preset = "default", out, keys;
    std::vector<std::pair<std::string, mat4>> objs;   // --obj, --obj-at
    std::vector<std::pair<int, int>> picks;            // --pick
    int width = DIM, height = DIM, ticks = 16, gpus = 0, samples = 1;
    bool emulate = false;
    unsigned bounces = 15;
    unsigned long long seed = 0x5EED;
    bool quiet = false;
    int denoise = -2;   // --denoise: -2 absent, -1 the default level count, else the level count
    int specularSteps = -1;   // --specular-features: -1 absent (first-hit features), else maxSteps
    bool temporal = false;
    int upscale = 0;   // --upscale: 0 absent, else the factor
    int upscaleLinear = 0;   // --upscale-linear: 0 absent, else the factor
    std::string film;  // --film: the camera model, empty = the frame loop
    float lensRadius = 0.05f, focusDistance = 5.0f;   // --lens
    bool refill = false;   // --refill: the film's trace with the refill schedule
    int adaptive = -1;     // --adaptive: -1 absent, else the planned rounds behind the uniform ones
    float adaptiveThreshold = -1.f;   // ... and the plan's threshold when given
    float linear = -1.f;   // --linear: -1 absent, else the exposure of the resolve
    int adaptiveLinear = -1;                                       // --adaptive-linear: -1 absent, else the planned rounds behind the uniform ones
    float adaptiveLinearThreshold = -1.f, adaptiveLinearFloor = -1.f;   // ... and the plan's threshold and floor when given
    std::string splat;     // --filter: the reconstruction filter of the linear film, empty = none (a box by pixel index)
    bool autoExposure = false;   // --auto-exposure: the linear film's exposure is metered on the device
    float meterKey = -1.f, meterRate = -1.f;   // ... its key and rate when given
    bool glare = false;                        // --glare: the final resolve of the linear film adds the glare pyramid
    float glareStrength = -1.f, glareThreshold = -1.f;   // ... its strength, threshold and levels when given
    int glareLevels = -1;
    int toneCurve = -1;                        // --tone: the final resolve of the linear film goes through a tone curve (PTSS_TONE_*)
    float toneWhite = -1.f;                    // ... Reinhard's white point when given
    bool toneSrgb = false, toneLuminance = false;   // --srgb, --tone-luminance
    bool denoiseLinear = false;                       // --denoise-linear: the linear film is denoised in front of the meter, the glare and the resolve
    int denoiseLinearLevels = -1;                     // ... its levels and sigmaLuminance when given
    float denoiseLinearSigma = -1.f;
    bool carry = false;                               // --carry: the linear film is carried across a second camera move
    std::string carryKeys;                            // ... the keys of that move, and the cap of the history count when given
    long carryHistory = -1;
    bool bake = false;                                // --bake: a light map of the scene's triangles instead of an image
    float bakeTexels = 4.f;                           // ... texels per unit of length, samples per texel, gutter-fill passes
    int bakeSamples = 16, bakePasses = 1;
    int bakeView = -1;                                // --bake-view: the filter of the camera view looked up from the baked map, -1 none
    int viewSteps = -1;                               // --view-steps: the links the view's rays follow through mirrors and glass, -1 not given
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { return (i + 1 < argc) ? argv[++i] : ""; };
        if (a == "--preset") preset = next();
        else if (a == "--size") { if (sscanf(next(), "%dx%d", &width, &height) != 2) { fprintf(stderr, "bad --size\n"); return 2; } }
        else if (a == "--ticks") ticks = atoi(next());
        else if (a == "--bounces") bounces = (unsigned)atoi(next());
        else if (a == "--seed") seed = strtoull(next(), NULL, 0);
        else if (a == "--keys") keys = next();
        else if (a == "--out") out = next();
        else if (a == "--quiet") quiet = true;
        else if (a == "--gpus") gpus = atoi(next());
        else if (a == "--emulate-gpus") { gpus = atoi(next()); emulate = true; }
        else if (a == "--samples-per-pass") samples = atoi(next());
        else if (a == "--obj") objs.push_back({next(), mat4::identity()});
        else if (a == "--obj-at") {
            float x, y, z, k;
            if (objs.empty() || sscanf(next(), "%f,%f,%f,%f", &x, &y, &z, &k) != 4) { fprintf(stderr, "bad --obj-at (x,y,z,scale after an --obj)\n"); return 2; }
            objs.back().second = translate(v3(x, y, z)) * scale(v3(k));
        }
        else if (a == "--denoise") {
            denoise = -1;
            if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') denoise = atoi(next());
        }
        else if (a == "--specular-features") specularSteps = atoi(next());
        else if (a == "--temporal") temporal = true;
        else if (a == "--upscale") upscale = atoi(next());
        else if (a == "--upscale-linear") {
            upscaleLinear = atoi(next());
            if (upscaleLinear < 1 || upscaleLinear > 4) { fprintf(stderr, "bad --upscale-linear (a factor 1..4)\n"); return 2; }
        }
        else if (a == "--film") film = next();
        else if (a == "--refill") refill = true;
        else if (a == "--adaptive") {
            const int got = sscanf(next(), "%d,%f", &adaptive, &adaptiveThreshold);
            if (got < 1 || adaptive < 0 || (got == 2 && !(adaptiveThreshold >= 0.f && adaptiveThreshold < 1e30f))) { fprintf(stderr, "bad --adaptive (rounds[,threshold])\n"); return 2; }
        }
        else if (a == "--adaptive-linear") {
            const int got = sscanf(next(), "%d,%f,%f", &adaptiveLinear, &adaptiveLinearThreshold, &adaptiveLinearFloor);
            if (got < 1 || adaptiveLinear < 0 || (got >= 2 && !(adaptiveLinearThreshold >= 0.f && adaptiveLinearThreshold < 1e30f)) ||
                (got == 3 && !(adaptiveLinearFloor > 0.f && adaptiveLinearFloor < 1e30f))) {
                fprintf(stderr, "bad --adaptive-linear (rounds[,threshold[,floor]])\n");
                return 2;
            }
        }
        else if (a == "--linear") {
            linear = 1.f;
            if (i + 1 < argc && ((argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') || argv[i + 1][0] == '.')) linear = (float)atof(next());
            if (!(linear >= 0.f && linear < 1e30f)) { fprintf(stderr, "bad --linear (exposure)\n"); return 2; }
        }
        else if (a == "--filter") splat = next();
        else if (a == "--auto-exposure") {
            autoExposure = true;
            if (i + 1 < argc && ((argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') || argv[i + 1][0] == '.')) {
                const int got = sscanf(next(), "%f,%f", &meterKey, &meterRate);
                if (got < 1 || !(meterKey > 0.f && meterKey < 1e30f) || (got == 2 && !(meterRate >= 0.f && meterRate <= 1.f))) {
                    fprintf(stderr, "bad --auto-exposure (key[,rate])\n");
                    return 2;
                }
            }
        }
        else if (a == "--glare") {
            glare = true;
            if (i + 1 < argc && ((argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') || argv[i + 1][0] == '.')) {
                const int got = sscanf(next(), "%f,%f,%d", &glareStrength, &glareThreshold, &glareLevels);
                if (got < 1 || !(glareStrength >= 0.f && glareStrength <= 1.f) || (got >= 2 && !(glareThreshold >= 0.f && glareThreshold < 1e30f)) ||
                    (got == 3 && (glareLevels < 1 || glareLevels > PTSS_GLARE_MAX_LEVELS))) {
                    fprintf(stderr, "bad --glare (strength[,threshold[,levels]])\n");
                    return 2;
                }
            }
        }
        else if (a == "--tone") {
            const std::string v = i + 1 < argc ? next() : "";
            char tail = 0;
            if (v == "clamp") toneCurve = PTSS_TONE_CLAMP;
            else if (v == "filmic") toneCurve = PTSS_TONE_FILMIC;
            else if (v == "reinhard") toneCurve = PTSS_TONE_REINHARD;
            else if (sscanf(v.c_str(), "reinhard,%f%c", &toneWhite, &tail) == 1 && toneWhite > 0.f && toneWhite <= 65536.f && 1.f / (toneWhite * toneWhite) < 3e38f)
                toneCurve = PTSS_TONE_REINHARD;
            else {
                fprintf(stderr, "bad --tone (clamp | reinhard[,white] | filmic)\n");
                return 2;
            }
        }
        else if (a == "--srgb") toneSrgb = true;
        else if (a == "--tone-luminance") toneLuminance = true;
        else if (a == "--denoise-linear") {
            denoiseLinear = true;
            const char* v = i + 1 < argc ? argv[i + 1] : "";
            if ((v[0] >= '0' && v[0] <= '9') || (v[0] == '-' && v[1] >= '0' && v[1] <= '9')) {
                const int got = sscanf(next(), "%d,%f", &denoiseLinearLevels, &denoiseLinearSigma);
                if (got < 1 || denoiseLinearLevels < 0 || denoiseLinearLevels > PTSS_DENOISE_MAX_LEVELS ||
                    (got == 2 && !(denoiseLinearSigma > 0.f && denoiseLinearSigma < 1e30f))) {
                    fprintf(stderr, "bad --denoise-linear (levels[,sigmaLuminance])\n");
                    return 2;
                }
            }
        }
        else if (a == "--carry") {
            carry = true;
            carryKeys = next();
            const size_t comma = carryKeys.find(',');
            if (comma != std::string::npos) {
                char* end = NULL;
                carryHistory = strtol(carryKeys.c_str() + comma + 1, &end, 10);
                if (end == carryKeys.c_str() + comma + 1 || *end != 0 || carryHistory < 1 || carryHistory > (1l << 23) - 1) carryHistory = 0;
                carryKeys.erase(comma);
            }
            if (carryKeys.empty() || carryKeys.find_first_not_of("wasdqefhgt") != std::string::npos || carryHistory == 0) {
                fprintf(stderr, "bad --carry (KEYS[,maxHistory]: keys of wasdqe fhgt, maxHistory 1 .. 8388607)\n");
                return 2;
            }
        }
        else if (a == "--bake") {
            bake = true;
            if (i + 1 < argc && ((argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') || argv[i + 1][0] == '.')) {
                const int got = sscanf(next(), "%f,%d,%d", &bakeTexels, &bakeSamples, &bakePasses);
                if (got < 1 || !(bakeTexels > 0.f && bakeTexels < 1e30f) || bakeSamples < 1 || bakeSamples > (1 << 22) || bakePasses < 0 || bakePasses > 64) {
                    fprintf(stderr, "bad --bake (texelsPerUnit[,samples[,passes]]: samples 1 .. 4194304, passes 0 .. 64)\n");
                    return 2;
                }
            }
        }
        else if (a == "--bake-view") {
            bakeView = PTSS_LIGHTMAP_BILINEAR;
            if (i + 1 < argc && (!strcmp(argv[i + 1], "nearest") || !strcmp(argv[i + 1], "bilinear")))
                bakeView = !strcmp(next(), "nearest") ? PTSS_LIGHTMAP_NEAREST : PTSS_LIGHTMAP_BILINEAR;
        }
        else if (a == "--view-steps") {
            if (sscanf(next(), "%d", &viewSteps) != 1 || viewSteps < 0 || viewSteps > 8) { fprintf(stderr, "bad --view-steps (0..8)\n"); return 2; }
        }
        else if (a == "--lens") { if (sscanf(next(), "%f,%f", &lensRadius, &focusDistance) != 2) { fprintf(stderr, "bad --lens (radius,focus)\n"); return 2; } }
        else if (a == "--pick") {
            int x, y;
            if (sscanf(next(), "%d,%d", &x, &y) != 2) { fprintf(stderr, "bad --pick (x,y)\n"); return 2; }
            picks.push_back({x, y});
        }
        else { fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }

    Scene scene;
    vec3 defaultColor = v3(0, 0, 0);
    if (!scene.buildPreset(preset)) {  // scene.build() for "default"
        fprintf(stderr, "unknown preset %s\n", preset.c_str());
        return 2;
    }
    for (const auto& obj : objs) {
        std::string why;
        if (scene.materialsVec.empty() || scene.addObjModel(obj.first, obj.second, 0, &why) < 0) {
            fprintf(stderr, "--obj %s: %s\n", obj.first.c_str(), scene.materialsVec.empty() ? "the preset has no material" : why.c_str());
            return 2;
        }
    }

    // initialize bitmap and data
    ProgramData* data = new ProgramData();
    GPUAnimBitmap bitmap(width, height, data);

    // allocate GPU memory, copy the scene, seed the per-pixel random streams (CudaTracer.cu:671-724)
    ptss_render_config cfg;
    PTSS_HANDLE(ptss_default_config(&cfg));
    cfg.width = width;
    cfg.height = height;
    cfg.maxIterations = bounces;
    cfg.seed = seed;
    cfg.samplesPerPass = samples;
    const ptss_scene_desc desc = scene.desc(defaultColor);
    ptss_context* ctx = NULL;
    if (!picks.empty() && gpus > 0) { fprintf(stderr, "--pick needs one context (no --gpus)\n"); return 2; }
    if (denoise != -2 && (gpus > 0 || out.empty())) { fprintf(stderr, "--denoise needs --out and one context (no --gpus)\n"); return 2; }
    if (specularSteps != -1 && (denoise == -2 || specularSteps < 0 || specularSteps > 8)) { fprintf(stderr, "--specular-features needs --denoise and a step count 0..8\n"); return 2; }
    if (temporal && (gpus > 0 || out.empty())) { fprintf(stderr, "--temporal needs --out and one context (no --gpus)\n"); return 2; }
    if (upscale != 0 && (gpus > 0 || out.empty() || upscale < 1 || upscale > 4)) { fprintf(stderr, "--upscale needs --out, one context (no --gpus) and a factor 1..4\n"); return 2; }
    const int filmKind = film == "pinhole" ? PTSS_FILM_PINHOLE : film == "thinlens" ? PTSS_FILM_THIN_LENS : film == "equirect" ? PTSS_FILM_EQUIRECT : -1;
    if (!film.empty() && (filmKind < 0 || gpus > 0 || out.empty() || temporal || upscale != 0 || specularSteps != -1 || samples != 1 || bounces < 1 || bounces > 64)) {
        fprintf(stderr, "--film needs pinhole, thinlens or equirect, --out, one context (no --gpus), 1..64 bounces, one sample per pass and none of "
                        "--temporal, --upscale, --specular-features\n");
        return 2;
    }
    if (refill && film.empty()) { fprintf(stderr, "--refill needs --film\n"); return 2; }
    if (adaptive >= 0 && film.empty()) { fprintf(stderr, "--adaptive needs --film\n"); return 2; }
    if (linear >= 0.f && (film.empty() || adaptive >= 0)) { fprintf(stderr, "--linear needs --film and no --adaptive\n"); return 2; }
    if (adaptiveLinear >= 0 && linear < 0.f) { fprintf(stderr, "--adaptive-linear needs --film and --linear\n"); return 2; }
    if (autoExposure && linear < 0.f) { fprintf(stderr, "--auto-exposure needs --linear\n"); return 2; }
    if (glare && linear < 0.f) { fprintf(stderr, "--glare needs --linear\n"); return 2; }
    if (toneCurve >= 0 && linear < 0.f) { fprintf(stderr, "--tone needs --film and --linear\n"); return 2; }
    if ((toneSrgb || toneLuminance) && toneCurve < 0) { fprintf(stderr, "--srgb and --tone-luminance need --tone\n"); return 2; }
    if (denoiseLinear && linear < 0.f) { fprintf(stderr, "--denoise-linear needs --film and --linear\n"); return 2; }
    if (upscaleLinear != 0 && (linear < 0.f || carry || adaptiveLinear >= 0 || denoise != -2)) {
        fprintf(stderr, "--upscale-linear needs --film and --linear, and none of --carry, --adaptive-linear, --denoise\n");
        return 2;
    }
    if (carry && (linear < 0.f || adaptiveLinear >= 0 || ticks < 1)) { fprintf(stderr, "--carry needs --film, --linear, at least one tick and no --adaptive-linear\n"); return 2; }
    if (bake && (gpus > 0 || !film.empty() || temporal || denoise != -2 || upscale != 0 || !picks.empty() || samples != 1 || bounces < 1 || bounces > 64 ||
                 width < 1)) {
        fprintf(stderr, "--bake needs one context (no --gpus), 1..64 bounces, one sample per pass and none of --film, --temporal, --denoise, --upscale, "
                        "--pick\n");
        return 2;
    }
    if (bakeView >= 0 && (!bake || height < 1)) { fprintf(stderr, "--bake-view needs --bake\n"); return 2; }
    if (viewSteps >= 0 && bakeView < 0) { fprintf(stderr, "--view-steps needs --bake-view\n"); return 2; }
    ptss_splat_filter splatFilter;
    PTSS_HANDLE(ptss_default_splat_filter(&splatFilter));
    if (!splat.empty()) {
        const size_t comma = splat.find(',');
        const std::string kind = splat.substr(0, comma);
        splatFilter.kind = kind == "box" ? PTSS_SPLAT_BOX : kind == "tent" ? PTSS_SPLAT_TENT : kind == "gaussian" ? PTSS_SPLAT_GAUSSIAN : -1;
        const int got = comma == std::string::npos ? 0 : sscanf(splat.c_str() + comma + 1, "%f,%f", &splatFilter.radius, &splatFilter.alpha);
        if (linear < 0.f || splatFilter.kind < 0 || (comma != std::string::npos && got < 1)) {
            fprintf(stderr, "--filter needs --linear and box, tent or gaussian[,radius[,alpha]]\n");
            return 2;
        }
    }
    for (const auto& p : picks)
        if (p.first < 0 || p.first >= width || p.second < 0 || p.second >= height) { fprintf(stderr, "--pick outside the frame\n"); return 2; }
    if (gpus > 0) {   // one context, stream and display tile per GPU; RCCL communicator over them
        createShards(data, desc, cfg, gpus, emulate);
        ctx = data->renderData.context;
    } else {
        PTSS_HANDLE(ptss_create(&desc, &cfg, &ctx));
    }

    // put values in a data block (:703-717)
    data->camera = Camera();
    data->renderData.context = ctx;
    data->renderData.numPointLights = scene.pointLightsVec.size();
    data->renderData.numAreaLights = scene.areaLightsVec.size();
    data->renderData.numSpheres = scene.spheresVec.size();
    data->renderData.numTriangles = scene.trianglesVec.size();
    data->renderData.defaultColor = defaultColor;
    data->maxIterations = bounces;
    data->resetTicksThisFrame = true;
    data->quiet = quiet;

    // --upscale: devLo, a display image of the frame's size, rebuilt at `upscale` times the size with the first-hit
    // features of the final camera at both sizes; written beside --out. 0 on success
    auto writeUpscaled = [&](const void* devLo) -> int {
        ptss_upsample_params up;
        PTSS_HANDLE(ptss_default_upsample_params(&up));
        up.factor = upscale;
        const size_t n = (size_t)width * (size_t)height, nHi = n * (size_t)(upscale * upscale);
        void *dfLo = nullptr, *dfHi = nullptr, *dpHi = nullptr;
        std::vector<ptss_uchar4> host(nHi);
        const char* failed = nullptr;
        if (hipMalloc(&dfLo, n * sizeof(ptss_pixel_feature)) != hipSuccess || hipMalloc(&dfHi, nHi * sizeof(ptss_pixel_feature)) != hipSuccess ||
            hipMalloc(&dpHi, nHi * sizeof(ptss_uchar4)) != hipSuccess) {
            failed = "device buffers";
        } else {
            PTSS_HANDLE(ptss_render_features(ctx, (ptss_pixel_feature*)dfLo, NULL));
            PTSS_HANDLE(ptss_render_features_scaled(ctx, upscale, (ptss_pixel_feature*)dfHi, NULL));
            PTSS_HANDLE(ptss_upsample(ctx, (const ptss_uchar4*)devLo, (const ptss_pixel_feature*)dfLo, (const ptss_pixel_feature*)dfHi, &up,
                                      (ptss_uchar4*)dpHi, NULL, NULL));
            PTSS_HANDLE(ptss_synchronize(ctx));
            if (hipMemcpy(host.data(), dpHi, nHi * sizeof(ptss_uchar4), hipMemcpyDeviceToHost) != hipSuccess) failed = "read-back";
        }
        (void)hipFree(dfLo);   // (hipFree(nullptr) is a no-op)
        (void)hipFree(dfHi);
        (void)hipFree(dpHi);
        std::string name = out;
        const size_t dot = name.rfind(".tga");
        if (dot != std::string::npos && dot + 4 == name.size()) name.erase(dot);
        name += "_upscaled.tga";
        if (!failed && !writeTga(name.c_str(), host.data(), width * upscale, height * upscale)) failed = "cannot write the file";
        if (failed) fprintf(stderr, "--upscale: %s (%s)\n", failed, name.c_str());
        return failed ? 1 : 0;
    };

    bitmap.set_max_ticks(ticks);
    if (bake) {   // the loop of INTEGRATION.md §2g "Baking": atlas, seed, then per sample generate, trace, accumulate by texel; gutter fills; resolve
        // with --bake-view the spheres take part (ptss_surface_atlas_blocks); without it the atlas is ptss_surface_atlas' as before
        const bool view = bakeView >= 0;
        const ptss_triangle* tris = scene.trianglesVec.empty() ? nullptr : scene.trianglesVec.data();
        const size_t T = scene.trianglesVec.size();
        const ptss_sphere* sphs = view && !scene.spheresVec.empty() ? scene.spheresVec.data() : nullptr;
        const size_t S = sphs ? scene.spheresVec.size() : 0;
        const int maxSide = S > 0 ? (width / 2 < 64 ? width / 2 : 64) : (width < 64 ? width : 64);
        size_t K = 0;
        int atlasH = 0;
        if (T + S == 0 || (!view && T == 0) || maxSide < 1 ||
            ptsurf::atlasBlocks(tris, 0, T, sphs, 0, S, bakeTexels, 1, maxSide, width, nullptr, nullptr, nullptr, nullptr, 0, &atlasH, &K) != 0 || K == 0) {
            fprintf(stderr, "--bake: the scene has no triangles, or the atlas of %d columns does not fit 2^31 texels\n", width);
            return 2;
        }
        std::vector<ptss_surface_point> points(K);
        std::vector<uint32_t> texels(K);
        std::vector<ptss_surface_block> blocksTri(T), blocksSph(S);
        ptsurf::atlasBlocks(tris, 0, T, sphs, 0, S, bakeTexels, 1, maxSide, width, blocksTri.data(), blocksSph.data(), points.data(), texels.data(), K,
                            &atlasH, &K);
        const size_t P = (size_t)width * (size_t)atlasH;
        void *dPoints = nullptr, *dTexels = nullptr, *dRng = nullptr, *dRays = nullptr, *dRes = nullptr, *dMap[2] = {nullptr, nullptr}, *dMeans = nullptr;
        if (hipMalloc(&dPoints, K * sizeof(ptss_surface_point)) != hipSuccess || hipMalloc(&dTexels, K * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc(&dRng, K * sizeof(ptss_path_rng)) != hipSuccess || hipMalloc(&dRays, K * sizeof(ptss_ray_query)) != hipSuccess ||
            hipMalloc(&dRes, K * sizeof(ptss_path_result)) != hipSuccess || hipMalloc(&dMap[0], P * sizeof(ptss_linear_entry)) != hipSuccess ||
            hipMalloc(&dMap[1], P * sizeof(ptss_linear_entry)) != hipSuccess || hipMalloc(&dMeans, P * sizeof(ptss_history_entry)) != hipSuccess ||
            hipMemcpy(dPoints, points.data(), K * sizeof(ptss_surface_point), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dTexels, texels.data(), K * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemset(dMap[0], 0, P * sizeof(ptss_linear_entry)) != hipSuccess) {
            fprintf(stderr, "--bake: device buffers\n");
            return 1;
        }
        ptss_surface_params sp;
        sp.structSize = (unsigned int)sizeof(sp);
        sp.mode = PTSS_SURFACE_COSINE;
        sp.maxDistance = ptm::inf();
        sp.reserved = 0u;
        ptss_linear_params linearParams;
        PTSS_HANDLE(ptss_default_linear_params(&linearParams));
        PTSS_HANDLE(ptss_seed_path_rng(ctx, (ptss_path_rng*)dRng, K, seed, 0, 0, NULL));
        for (int s = 0; s < bakeSamples; ++s) {
            PTSS_HANDLE(ptss_generate_rays_surface(ctx, &sp, (const ptss_surface_point*)dPoints, K, 0, NULL, K, (ptss_path_rng*)dRng, (ptss_ray_query*)dRays,
                                                   NULL, NULL));
            PTSS_HANDLE(ptss_trace_paths(ctx, (const ptss_ray_query*)dRays, (ptss_path_rng*)dRng, (ptss_path_result*)dRes, K, bounces, NULL));
            PTSS_HANDLE(ptss_accumulate_paths_linear(ctx, (const ptss_path_result*)dRes, (const uint32_t*)dTexels, 0, K, (ptss_linear_entry*)dMap[0], P,
                                                     &linearParams, NULL));
        }
        int cur = 0;
        for (int pass = 0; pass < bakePasses; ++pass, cur = 1 - cur)
            PTSS_HANDLE(ptss_dilate_linear(ctx, (const ptss_linear_entry*)dMap[cur], width, atlasH, (ptss_linear_entry*)dMap[1 - cur], NULL));
        PTSS_HANDLE(ptss_resolve_linear(ctx, (const ptss_linear_entry*)dMap[cur], 0, P, &linearParams, (ptss_history_entry*)dMeans, NULL, NULL, NULL));
        PTSS_HANDLE(ptss_synchronize(ctx));
        unsigned long long rejected = 0;
        PTSS_HANDLE(ptss_surface_rejected(ctx, &rejected));
        std::vector<ptss_history_entry> means(P);
        if (hipMemcpy(means.data(), dMeans, P * sizeof(ptss_history_entry), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "--bake: read-back\n"); return 1; }
        const std::string name = out.empty() ? "lightmap.pfm" : out;
        if (!writePfm(name.c_str(), means.data(), width, atlasH)) { fprintf(stderr, "--bake: cannot write %s\n", name.c_str()); return 1; }
        printf("bake: atlas %d x %d, %zu texels of %zu triangles, %d samples, %d passes, rejected %llu\n", width, atlasH, K, T, bakeSamples, bakePasses,
               rejected);
        if (view) {   // the loop of INTEGRATION.md §2g "Looking a light map up": centre rays, closest hits, the lookup, the resolve
            for (char k : keys) moveCamera(data->camera, (unsigned char)k);
            ptss_film_camera fc;
            memset(&fc, 0, sizeof(fc));
            fc.structSize = (unsigned int)sizeof(fc);
            fc.kind = PTSS_FILM_PINHOLE;
            fc.camera = data->camera;
            fc.width = width;
            fc.height = height;
            fc.focusDistance = 1.f;
            fc.jitter = 0;
            ptss_lightmap_params lp;
            PTSS_HANDLE(ptss_default_lightmap_params(&lp));
            lp.atlasWidth = width;
            lp.atlasHeight = atlasH;
            lp.filter = bakeView;
            lp.flags = PTSS_LIGHTMAP_MODULATE | PTSS_LIGHTMAP_EMISSION;
            lp.numTriangleBlocks = (int)T;
            lp.numSphereBlocks = (int)S;
            const size_t n = (size_t)width * (size_t)height;
            void *dBt = nullptr, *dBs = nullptr, *dVRng = nullptr, *dVRays = nullptr, *dHits = nullptr, *dView = nullptr, *dVMeans = nullptr, *dInfo = nullptr;
            void* dChain = nullptr;   // --view-steps above 0: what each ray's chain did on the way
            if (viewSteps > 0 && hipMalloc(&dChain, n * sizeof(ptss_chain_result)) != hipSuccess) { fprintf(stderr, "--view-steps: device buffers\n"); return 1; }
            if (hipMalloc(&dBt, (T ? T : 1) * sizeof(ptss_surface_block)) != hipSuccess || hipMalloc(&dBs, (S ? S : 1) * sizeof(ptss_surface_block)) != hipSuccess ||
                hipMalloc(&dVRng, n * sizeof(ptss_path_rng)) != hipSuccess || hipMalloc(&dVRays, n * sizeof(ptss_ray_query)) != hipSuccess ||
                hipMalloc(&dHits, n * sizeof(ptss_ray_hit)) != hipSuccess || hipMalloc(&dView, n * sizeof(ptss_linear_entry)) != hipSuccess ||
                hipMalloc(&dVMeans, n * sizeof(ptss_history_entry)) != hipSuccess || hipMalloc(&dInfo, 4 * sizeof(uint32_t)) != hipSuccess ||
                hipMemcpy(dBt, blocksTri.data(), T * sizeof(ptss_surface_block), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemcpy(dBs, blocksSph.data(), S * sizeof(ptss_surface_block), hipMemcpyHostToDevice) != hipSuccess ||
                hipMemset(dVRng, 0, n * sizeof(ptss_path_rng)) != hipSuccess || hipMemset(dInfo, 0, 4 * sizeof(uint32_t)) != hipSuccess) {
                fprintf(stderr, "--bake-view: device buffers\n");
                return 1;
            }
            PTSS_HANDLE(ptss_generate_rays(ctx, &fc, 0, NULL, n, (ptss_path_rng*)dVRng, (ptss_ray_query*)dVRays, NULL));
            if (viewSteps > 0) {
                PTSS_HANDLE(ptss_intersect_chain(ctx, (const ptss_ray_query*)dVRays, n, viewSteps, NULL, (ptss_ray_hit*)dHits, (ptss_chain_result*)dChain, NULL));
                PTSS_HANDLE(ptss_lookup_lightmap_chain(ctx, &lp, &linearParams, T ? (const ptss_surface_block*)dBt : NULL,
                                                       S ? (const ptss_surface_block*)dBs : NULL, (const ptss_linear_entry*)dMap[cur],
                                                       (const ptss_ray_hit*)dHits, (const ptss_chain_result*)dChain, n, (ptss_linear_entry*)dView,
                                                       (uint32_t*)dInfo, NULL));
            } else {
                PTSS_HANDLE(ptss_intersect(ctx, (const ptss_ray_query*)dVRays, (ptss_ray_hit*)dHits, n, NULL));
                PTSS_HANDLE(ptss_lookup_lightmap(ctx, &lp, &linearParams, T ? (const ptss_surface_block*)dBt : NULL, S ? (const ptss_surface_block*)dBs : NULL,
                                                 (const ptss_linear_entry*)dMap[cur], (const ptss_ray_hit*)dHits, n, (ptss_linear_entry*)dView,
                                                 (uint32_t*)dInfo, NULL));
            }
            PTSS_HANDLE(ptss_resolve_linear(ctx, (const ptss_linear_entry*)dView, 0, n, &linearParams, (ptss_history_entry*)dVMeans, NULL, NULL, NULL));
            PTSS_HANDLE(ptss_synchronize(ctx));
            std::vector<ptss_history_entry> viewMeans(n);
            uint32_t info[4];
            if (hipMemcpy(viewMeans.data(), dVMeans, n * sizeof(ptss_history_entry), hipMemcpyDeviceToHost) != hipSuccess ||
                hipMemcpy(info, dInfo, sizeof(info), hipMemcpyDeviceToHost) != hipSuccess) {
                fprintf(stderr, "--bake-view: read-back\n");
                return 1;
            }
            std::string viewName = name;
            const size_t dot = viewName.rfind(".pfm");
            if (dot != std::string::npos && dot + 4 == viewName.size()) viewName.erase(dot);
            viewName += "_view.pfm";
            if (!writePfm(viewName.c_str(), viewMeans.data(), width, height)) { fprintf(stderr, "--bake-view: cannot write %s\n", viewName.c_str()); return 1; }
            printf("bake view: %d x %d, %s, %zu sphere blocks, filtered %u, empty %u, no block %u, rejected %u\n", width, height,
                   bakeView == PTSS_LIGHTMAP_NEAREST ? "nearest" : "bilinear", S, info[0], info[1], info[2], info[3]);
            if (viewSteps > 0) {
                std::vector<ptss_chain_result> rows(n);
                if (hipMemcpy(rows.data(), dChain, n * sizeof(ptss_chain_result), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "--view-steps: read-back\n"); return 1; }
                unsigned long long links = 0, behind = 0;
                for (const ptss_chain_result& c : rows) links += c.steps, behind += c.steps > 0u;
                printf("view steps: at most %d, %llu links followed, %llu of %zu pixels seen through a mirror or glass\n", viewSteps, links, behind, n);
                (void)hipFree(dChain);
            }
            for (void* d : {dBt, dBs, dVRng, dVRays, dHits, dView, dVMeans, dInfo}) (void)hipFree(d);
        }
        for (void* d : {dPoints, dTexels, dRng, dRays, dRes, dMap[0], dMap[1], dMeans}) (void)hipFree(d);
        PTSS_HANDLE(ptss_destroy(ctx));
        bitmap.free_resources();
        delete data;
        return 0;
    }
    if (temporal) {   // the loop of INTEGRATION.md: frames, features, reproject from the history kept at the previous pose, keep, move
        const size_t n = (size_t)width * (size_t)height;
        void *df[2] = {nullptr, nullptr}, *dh[2] = {nullptr, nullptr}, *dp = nullptr;
        for (int k = 0; k < 2; ++k)
            if (hipMalloc(&df[k], n * sizeof(ptss_pixel_feature)) != hipSuccess || hipMalloc(&dh[k], n * sizeof(ptss_history_entry)) != hipSuccess) {
                fprintf(stderr, "--temporal: device buffers\n");
                return 1;
            }
        if (hipMalloc(&dp, n * sizeof(ptss_uchar4)) != hipSuccess) { fprintf(stderr, "--temporal: device buffers\n"); return 1; }
        ptss_reproject_params rp;
        PTSS_HANDLE(ptss_default_reproject_params(&rp));
        ptss_camera keptCamera = data->camera;
        int cur = 0;
        for (size_t pose = 0; pose <= keys.size(); ++pose) {
            if (pose > 0) bitmap.push_key((unsigned char)keys[pose - 1]);
            bitmap.anim_and_exit((void (*)(uchar4*, void*, int))generateFrame, NULL, (void (*)(unsigned char, int, int))Key);
            const bool have = pose > 0;
            PTSS_HANDLE(ptss_render_features(ctx, (ptss_pixel_feature*)df[cur], NULL));
            PTSS_HANDLE(ptss_reproject(ctx, (const ptss_pixel_feature*)df[cur], have ? &keptCamera : NULL,
                                       have ? (const ptss_pixel_feature*)df[1 - cur] : NULL, have ? (const ptss_history_entry*)dh[1 - cur] : NULL, &rp,
                                       (ptss_history_entry*)dh[cur], NULL));
            keptCamera = data->camera;   // kept with its features and this output: the history of the next pose
            cur = 1 - cur;
        }
        ptss_denoise_params params;
        PTSS_HANDLE(ptss_default_denoise_params(&params));
        PTSS_HANDLE(ptss_denoise_history(ctx, (const ptss_history_entry*)dh[1 - cur], (const ptss_pixel_feature*)df[1 - cur], &params, (ptss_uchar4*)dp, NULL));
        PTSS_HANDLE(ptss_synchronize(ctx));
        std::vector<ptss_uchar4> host(n);
        if (hipMemcpy(host.data(), dp, n * sizeof(ptss_uchar4), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "--temporal: read-back\n"); return 1; }
        if (upscale != 0 && denoise == -2 && writeUpscaled(dp) != 0) return 1;
        for (int k = 0; k < 2; ++k) { (void)hipFree(df[k]); (void)hipFree(dh[k]); }
        (void)hipFree(dp);
        if (!writeTga(out.c_str(), host.data(), width, height)) fprintf(stderr, "--temporal: cannot write %s\n", out.c_str());
    } else if (!film.empty()) {   // the loop of INTEGRATION.md §2g: generate, trace, accumulate, once per tick
        *GPUAnimBitmap::get_bitmap_ptr() = &bitmap;   // (saveScreenshot reads the display buffer through it)
        for (char k : keys) moveCamera(data->camera, (unsigned char)k);
        PTSS_HANDLE(ptss_set_camera(ctx, &data->camera));
        ptss_film_camera fc;
        memset(&fc, 0, sizeof(fc));
        fc.structSize = (unsigned int)sizeof(fc);
        fc.kind = filmKind;
        fc.camera = data->camera;
        fc.width = width;
        fc.height = height;
        fc.lensRadius = lensRadius;
        fc.focusDistance = focusDistance;
        fc.jitter = 1;
        ptss_path_options pathOptions;
        PTSS_HANDLE(ptss_default_path_options(&pathOptions));
        if (refill) pathOptions.schedule = PTSS_PATHS_REFILL;
        const size_t n = (size_t)width * (size_t)height;
        void *dRng = nullptr, *dRays = nullptr, *dRes = nullptr, *dFilm = nullptr, *dHist = nullptr, *dFeat = nullptr, *dOut = nullptr;
        void *dMoments = nullptr, *dCdf = nullptr, *dIndex = nullptr, *dInfo = nullptr;   // --adaptive
        void *dLinear = nullptr, *dMeans = nullptr;   // --linear (with --filter dLinear holds ptss_splat_entry, the same 32 bytes per pixel)
        void* dPos = nullptr;                         // --filter
        void *dBins = nullptr, *dMeter = nullptr;     // --auto-exposure: one histogram per round, and the meter's state
        ptss_meter_params meterParams;
        PTSS_HANDLE(ptss_default_meter_params(&meterParams));
        if (meterKey > 0.f) meterParams.key = meterKey;
        if (meterRate >= 0.f) meterParams.rate = meterRate;
        ptss_linear_params linearParams;
        PTSS_HANDLE(ptss_default_linear_params(&linearParams));
        const bool filter = denoise != -2;
        if (hipMalloc(&dRng, n * sizeof(ptss_path_rng)) != hipSuccess || hipMalloc(&dRays, n * sizeof(ptss_ray_query)) != hipSuccess ||
            hipMalloc(&dRes, n * sizeof(ptss_path_result)) != hipSuccess || hipMalloc(&dFilm, n * sizeof(ptss_film_entry)) != hipSuccess ||
            hipMemset(dFilm, 0, n * sizeof(ptss_film_entry)) != hipSuccess ||
            (filter && (hipMalloc(&dHist, n * sizeof(ptss_history_entry)) != hipSuccess || hipMalloc(&dFeat, n * sizeof(ptss_pixel_feature)) != hipSuccess ||
                        hipMalloc(&dOut, n * sizeof(ptss_uchar4)) != hipSuccess))) {
            fprintf(stderr, "--film: device buffers\n");
            return 1;
        }
        size_t cdfEntries = 0;
        if (adaptive >= 0) {
            PTSS_HANDLE(ptss_plan_cdf_entries(n, &cdfEntries));
            if (hipMalloc(&dMoments, n * sizeof(unsigned long long)) != hipSuccess || hipMemset(dMoments, 0, n * sizeof(unsigned long long)) != hipSuccess ||
                hipMalloc(&dCdf, cdfEntries * sizeof(unsigned long long)) != hipSuccess || hipMalloc(&dIndex, n * sizeof(uint32_t)) != hipSuccess ||
                hipMalloc(&dInfo, sizeof(ptss_plan_info)) != hipSuccess) {
                fprintf(stderr, "--adaptive: device buffers\n");
                return 1;
            }
        }
        ptss_linear_plan_params linearPlan;
        PTSS_HANDLE(ptss_default_linear_plan_params(&linearPlan));
        if (adaptiveLinear >= 0) {   // (dMoments holds ptss_linear_moment here: --adaptive and --linear exclude each other)
            PTSS_HANDLE(ptss_plan_cdf_entries(n, &cdfEntries));
            if (hipMalloc(&dMoments, n * sizeof(ptss_linear_moment)) != hipSuccess || hipMemset(dMoments, 0, n * sizeof(ptss_linear_moment)) != hipSuccess ||
                hipMalloc(&dCdf, cdfEntries * sizeof(unsigned long long)) != hipSuccess || hipMalloc(&dIndex, n * sizeof(uint32_t)) != hipSuccess ||
                hipMalloc(&dInfo, sizeof(ptss_plan_info)) != hipSuccess) {
                fprintf(stderr, "--adaptive-linear: device buffers\n");
                return 1;
            }
            linearPlan.minSamples = ticks > 0 ? (uint32_t)ticks : 1u;
            if (linearPlan.maxSamples < linearPlan.minSamples) linearPlan.maxSamples = linearPlan.minSamples;
            if (adaptiveLinearThreshold >= 0.f) linearPlan.threshold = adaptiveLinearThreshold;
            if (adaptiveLinearFloor > 0.f) linearPlan.floor = adaptiveLinearFloor;
        }
        if (linear >= 0.f) {
            linearParams.exposure = linear;
            if (hipMalloc(&dLinear, n * sizeof(ptss_linear_entry)) != hipSuccess || hipMemset(dLinear, 0, n * sizeof(ptss_linear_entry)) != hipSuccess ||
                hipMalloc(&dMeans, n * sizeof(ptss_history_entry)) != hipSuccess) {
                fprintf(stderr, "--linear: device buffers\n");
                return 1;
            }
            static_assert(sizeof(ptss_splat_entry) == sizeof(ptss_linear_entry), "one film buffer serves both");
            if (!splat.empty() && hipMalloc(&dPos, n * sizeof(ptss_film_position)) != hipSuccess) { fprintf(stderr, "--filter: device buffers\n"); return 1; }
        }
        if (autoExposure) {   // every round meters into a histogram of its own, zeroed here: nothing is cleared between the rounds' launches
            const size_t rounds = (ticks > 0 ? (size_t)ticks : 1) * (carry ? 2 : 1) + (adaptiveLinear > 0 ? (size_t)adaptiveLinear : 0);
            if (hipMalloc(&dBins, rounds * PTSS_METER_BINS * sizeof(uint32_t)) != hipSuccess || hipMalloc(&dMeter, sizeof(ptss_meter_state)) != hipSuccess ||
                hipMemset(dBins, 0, rounds * PTSS_METER_BINS * sizeof(uint32_t)) != hipSuccess || hipMemset(dMeter, 0, sizeof(ptss_meter_state)) != hipSuccess ||
                hipDeviceSynchronize() != hipSuccess) {
                fprintf(stderr, "--auto-exposure: device buffers\n");
                return 1;
            }
        }
        void *dClean = nullptr, *dCleanFeat = nullptr, *dCleanWork = nullptr;   // --denoise-linear: the denoised film, the features, the workspace
        ptss_denoise_linear_params cleanParams;
        PTSS_HANDLE(ptss_default_denoise_linear_params(&cleanParams));
        if (denoiseLinearLevels >= 0) cleanParams.levels = denoiseLinearLevels;
        if (denoiseLinearSigma > 0.f) cleanParams.sigmaLuminance = denoiseLinearSigma;
        if (denoiseLinear) {
            size_t work = 0;
            PTSS_HANDLE(ptss_denoise_linear_workspace(width, height, &work));
            if (hipMalloc(&dClean, n * sizeof(ptss_linear_entry)) != hipSuccess || hipMalloc(&dCleanFeat, n * sizeof(ptss_pixel_feature)) != hipSuccess ||
                hipMalloc(&dCleanWork, work) != hipSuccess ||
                (!dMoments && (hipMalloc(&dMoments, n * sizeof(ptss_linear_moment)) != hipSuccess ||
                               hipMemset(dMoments, 0, n * sizeof(ptss_linear_moment)) != hipSuccess))) {
                fprintf(stderr, "--denoise-linear: device buffers\n");
                return 1;
            }
        }
        // --carry: the features of both poses, the seeded film and moments (swapped with the rounds' own after the call), the counters
        void *dCarryPrev = nullptr, *dCarryNow = nullptr, *dCarryFilm = nullptr, *dCarryMoments = nullptr, *dCarryInfo = nullptr;
        ptss_reproject_linear_params carryParams;
        PTSS_HANDLE(ptss_default_reproject_linear_params(&carryParams));
        if (carryHistory > 0) carryParams.maxHistory = (uint32_t)carryHistory;
        if (carry) {
            if (hipMalloc(&dCarryPrev, n * sizeof(ptss_pixel_feature)) != hipSuccess || hipMalloc(&dCarryNow, n * sizeof(ptss_pixel_feature)) != hipSuccess ||
                hipMalloc(&dCarryFilm, n * sizeof(ptss_linear_entry)) != hipSuccess || hipMalloc(&dCarryMoments, n * sizeof(ptss_linear_moment)) != hipSuccess ||
                hipMalloc(&dCarryInfo, sizeof(ptss_reproject_linear_info)) != hipSuccess ||
                hipMemset(dCarryInfo, 0, sizeof(ptss_reproject_linear_info)) != hipSuccess ||
                (!dMoments && (hipMalloc(&dMoments, n * sizeof(ptss_linear_moment)) != hipSuccess ||
                               hipMemset(dMoments, 0, n * sizeof(ptss_linear_moment)) != hipSuccess)) ||
                hipDeviceSynchronize() != hipSuccess) {
                fprintf(stderr, "--carry: device buffers\n");
                return 1;
            }
        }
        const bool keepMoments = adaptiveLinear >= 0 || denoiseLinear || carry;   // the rounds accumulate with stats
        // what the meter, the glare and the resolves read: the denoised film, a linear one whatever the rounds fill, or the rounds' own
        const void* shown = denoiseLinear ? dClean : dLinear;
        bool shownSplat = !denoiseLinear && dPos;
        // --upscale-linear: what is shown is the large film, made from the one above; its size, means and pixels
        size_t shownN = n;
        int shownW = width, shownH = height;
        void *dShownMeans = dMeans, *dShownPixels = bitmap.devPixels, *dShownHist = dHist;
        void *dBigFilm = nullptr, *dBigMeans = nullptr, *dBigPixels = nullptr, *dBigFeat = nullptr, *dSmallFeat = nullptr, *dBigInfo = nullptr;
        ptss_upsample_linear_params bigParams;
        PTSS_HANDLE(ptss_default_upsample_linear_params(&bigParams));
        const void* smallFilm = shown;
        const bool smallSplat = shownSplat;
        if (upscaleLinear != 0) {
            bigParams.factor = upscaleLinear;
            if (filmKind == PTSS_FILM_EQUIRECT) bigParams.flags |= PTSS_UPSAMPLE_LINEAR_WRAP_X;
            shownW = width * upscaleLinear, shownH = height * upscaleLinear;
            shownN = (size_t)shownW * (size_t)shownH;
            // the centre rays of the same film camera at both sizes (jitter 0 draws nothing; streams of their own all the same)
            void *dBigRng = nullptr, *dBigRays = nullptr;
            if (hipMalloc(&dBigFilm, shownN * sizeof(ptss_linear_entry)) != hipSuccess || hipMalloc(&dBigMeans, shownN * sizeof(ptss_history_entry)) != hipSuccess ||
                hipMalloc(&dBigPixels, shownN * sizeof(ptss_uchar4)) != hipSuccess || hipMalloc(&dBigFeat, shownN * sizeof(ptss_pixel_feature)) != hipSuccess ||
                hipMalloc(&dSmallFeat, n * sizeof(ptss_pixel_feature)) != hipSuccess || hipMalloc(&dBigInfo, sizeof(ptss_upsample_linear_info)) != hipSuccess ||
                hipMemset(dBigInfo, 0, sizeof(ptss_upsample_linear_info)) != hipSuccess || hipMalloc(&dBigRng, shownN * sizeof(ptss_path_rng)) != hipSuccess ||
                hipMalloc(&dBigRays, shownN * sizeof(ptss_ray_query)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
                fprintf(stderr, "--upscale-linear: device buffers\n");
                return 1;
            }
            PTSS_HANDLE(ptss_seed_path_rng(ctx, (ptss_path_rng*)dBigRng, shownN, seed, 0, 0, NULL));
            ptss_film_camera centre = fc;
            centre.jitter = 0;
            PTSS_HANDLE(ptss_generate_rays(ctx, &centre, 0, NULL, n, (ptss_path_rng*)dBigRng, (ptss_ray_query*)dBigRays, NULL));
            PTSS_HANDLE(ptss_ray_features(ctx, (const ptss_ray_query*)dBigRays, (ptss_pixel_feature*)dSmallFeat, n, NULL));
            centre.width = shownW, centre.height = shownH;
            PTSS_HANDLE(ptss_generate_rays(ctx, &centre, 0, NULL, shownN, (ptss_path_rng*)dBigRng, (ptss_ray_query*)dBigRays, NULL));
            PTSS_HANDLE(ptss_ray_features(ctx, (const ptss_ray_query*)dBigRays, (ptss_pixel_feature*)dBigFeat, shownN, NULL));
            PTSS_HANDLE(ptss_synchronize(ctx));
            (void)hipFree(dBigRng);
            (void)hipFree(dBigRays);
            shown = dBigFilm;
            shownSplat = false;
            dShownMeans = dBigMeans, dShownPixels = dBigPixels, dShownHist = nullptr;
        }
        auto upsampleFilm = [&]() -> int {
            PTSS_HANDLE(ptss_upsample_linear(ctx, smallFilm, smallSplat ? PTSS_FILM_SPLAT : PTSS_FILM_LINEAR, width, height,
                                             (const ptss_pixel_feature*)dSmallFeat, (const ptss_pixel_feature*)dBigFeat, &linearParams, &bigParams,
                                             (ptss_linear_entry*)dBigFilm, (ptss_upsample_linear_info*)dBigInfo, NULL));
            return 0;
        };
        auto denoiseFilm = [&]() -> int {
            PTSS_HANDLE(ptss_denoise_linear(ctx, dLinear, dPos ? PTSS_FILM_SPLAT : PTSS_FILM_LINEAR, width, height, (const ptss_linear_moment*)dMoments,
                                            (const ptss_pixel_feature*)dCleanFeat, &linearParams, &cleanParams, dCleanWork, (ptss_linear_entry*)dClean,
                                            NULL));
            return 0;
        };
        void* dPyramid = nullptr;   // --glare
        ptss_glare_params glareParams;
        PTSS_HANDLE(ptss_default_glare_params(&glareParams));
        if (glareStrength >= 0.f) glareParams.strength = glareStrength;
        if (glareThreshold >= 0.f) glareParams.threshold = glareThreshold;
        if (glareLevels >= 1) glareParams.levels = glareLevels;
        if (glare) {
            ptss_glare_level levels[PTSS_GLARE_MAX_LEVELS];
            size_t entries = 0;
            PTSS_HANDLE(ptss_glare_layout(shownW, shownH, glareParams.levels, levels, &entries));
            if (hipMalloc(&dPyramid, entries * sizeof(ptss_glare_entry)) != hipSuccess) { fprintf(stderr, "--glare: device buffers\n"); return 1; }
        }
        auto meteredResolve = [&]() -> int {   // the exposure is the state's, --linear's compensating
            if (shownSplat) {
                PTSS_HANDLE(ptss_resolve_splat_metered(ctx, (const ptss_splat_entry*)shown, 0, shownN, &linearParams, (const ptss_meter_state*)dMeter,
                                                       (ptss_history_entry*)dShownMeans, (ptss_uchar4*)dShownPixels, (ptss_history_entry*)dShownHist, NULL));
            } else {
                PTSS_HANDLE(ptss_resolve_linear_metered(ctx, (const ptss_linear_entry*)shown, 0, shownN, &linearParams, (const ptss_meter_state*)dMeter,
                                                        (ptss_history_entry*)dShownMeans, (ptss_uchar4*)dShownPixels, (ptss_history_entry*)dShownHist, NULL));
            }
            return 0;
        };
        auto meterRound = [&](int round) -> int {   // meter, update, metered resolve: the round's exposure never leaves the device
            uint32_t* bins = (uint32_t*)dBins + (size_t)round * PTSS_METER_BINS;
            if (denoiseLinear && denoiseFilm()) return 1;   // the meter reads the denoised film of this round
            if (upscaleLinear != 0 && upsampleFilm()) return 1;   // ... at the large size
            if (shownSplat) {
                PTSS_HANDLE(ptss_meter_splat(ctx, (const ptss_splat_entry*)shown, 0, shownN, bins, NULL));
            } else {
                PTSS_HANDLE(ptss_meter_linear(ctx, (const ptss_linear_entry*)shown, 0, shownN, bins, NULL));
            }
            PTSS_HANDLE(ptss_meter_exposure(ctx, bins, &linearParams, &meterParams, (ptss_meter_state*)dMeter, NULL));
            return meteredResolve();
        };
        PTSS_HANDLE(ptss_seed_path_rng(ctx, (ptss_path_rng*)dRng, n, seed, 0, 0, NULL));
        if (denoiseLinear) {   // the features of the pixel-centre rays (jitter 0 draws nothing: the streams stay what the rounds expect)
            fc.jitter = 0;
            PTSS_HANDLE(ptss_generate_rays(ctx, &fc, 0, NULL, n, (ptss_path_rng*)dRng, (ptss_ray_query*)dRays, NULL));
            PTSS_HANDLE(ptss_ray_features(ctx, (const ptss_ray_query*)dRays, (ptss_pixel_feature*)dCleanFeat, n, NULL));
            fc.jitter = 1;
        }
        auto centreFeatures = [&](void* features) -> int {   // (jitter 0 draws nothing: the streams stay what the rounds expect)
            fc.jitter = 0;
            PTSS_HANDLE(ptss_generate_rays(ctx, &fc, 0, NULL, n, (ptss_path_rng*)dRng, (ptss_ray_query*)dRays, NULL));
            PTSS_HANDLE(ptss_ray_features(ctx, (const ptss_ray_query*)dRays, (ptss_pixel_feature*)features, n, NULL));
            fc.jitter = 1;
            return 0;
        };
        auto carryFilm = [&]() -> int {   // the move of --carry: the film of the pose so far seeds the film of the next
            if (centreFeatures(dCarryPrev)) return 1;
            ptss_film_camera before = fc;
            for (char k : carryKeys) moveCamera(data->camera, (unsigned char)k);
            PTSS_HANDLE(ptss_set_camera(ctx, &data->camera));
            fc.camera = data->camera;
            if (centreFeatures(dCarryNow)) return 1;
            if (denoiseLinear && centreFeatures(dCleanFeat)) return 1;   // the denoiser is guided by the new pose's features from here on
            PTSS_HANDLE(ptss_reproject_linear(ctx, &fc, (const ptss_pixel_feature*)dCarryNow, NULL, &before, (const ptss_pixel_feature*)dCarryPrev, dLinear,
                                              dPos ? PTSS_FILM_SPLAT : PTSS_FILM_LINEAR, (const ptss_linear_moment*)dMoments, &linearParams, &carryParams,
                                              dCarryFilm, (ptss_linear_moment*)dCarryMoments, (ptss_reproject_linear_info*)dCarryInfo, NULL));
            std::swap(dLinear, dCarryFilm);
            std::swap(dMoments, dCarryMoments);
            if (!denoiseLinear) shown = dLinear;
            return 0;
        };
        for (int t = 0; t < (carry ? 2 * ticks : ticks); ++t) {
            if (carry && t == ticks && carryFilm()) return 1;
            if (dPos) {
                PTSS_HANDLE(ptss_generate_rays_positions(ctx, &fc, 0, NULL, n, (ptss_path_rng*)dRng, (ptss_ray_query*)dRays, (ptss_film_position*)dPos, NULL));
            } else {
                PTSS_HANDLE(ptss_generate_rays(ctx, &fc, 0, NULL, n, (ptss_path_rng*)dRng, (ptss_ray_query*)dRays, NULL));
            }
            PTSS_HANDLE(ptss_trace_paths_opt(ctx, (const ptss_ray_query*)dRays, (ptss_path_rng*)dRng, (ptss_path_result*)dRes, n, bounces, &pathOptions,
                                             NULL));
            if (dPos) {
                PTSS_HANDLE(ptss_splat_paths_homed(ctx, (const ptss_path_result*)dRes, (const ptss_film_position*)dPos, 0, n, (ptss_splat_entry*)dLinear,
                                                   width, height, &splatFilter, &linearParams, NULL));
                if (keepMoments) {   // the moments by home pixel, beside the filtered film
                    PTSS_HANDLE(ptss_accumulate_paths_linear_stats(ctx, (const ptss_path_result*)dRes, NULL, 0, n, NULL, (ptss_linear_moment*)dMoments, n,
                                                                   &linearParams, NULL));
                }
            } else if (keepMoments) {
                PTSS_HANDLE(ptss_accumulate_paths_linear_stats(ctx, (const ptss_path_result*)dRes, NULL, 0, n, (ptss_linear_entry*)dLinear,
                                                               (ptss_linear_moment*)dMoments, n, &linearParams, NULL));
            } else if (linear >= 0.f) {
                PTSS_HANDLE(ptss_accumulate_paths_linear(ctx, (const ptss_path_result*)dRes, NULL, 0, n, (ptss_linear_entry*)dLinear, n, &linearParams, NULL));
            } else if (adaptive >= 0) {
                PTSS_HANDLE(ptss_accumulate_paths_stats(ctx, (const ptss_path_result*)dRes, NULL, 0, n, (ptss_film_entry*)dFilm,
                                                        (unsigned long long*)dMoments, n, (ptss_uchar4*)bitmap.devPixels, (ptss_history_entry*)dHist, NULL));
            } else {
                PTSS_HANDLE(ptss_accumulate_paths(ctx, (const ptss_path_result*)dRes, NULL, 0, n, (ptss_film_entry*)dFilm, n, (ptss_uchar4*)bitmap.devPixels,
                                                  (ptss_history_entry*)dHist, NULL));
            }
            if (autoExposure && meterRound(t)) return 1;
        }
        if (adaptiveLinear >= 0) {   // the planned rounds on the linear film: ray slot i keeps stream i whatever pixel the plan gives it
            for (int t = 0; t <= adaptiveLinear; ++t) {   // (the last plan only reports what the rounds left)
                PTSS_HANDLE(ptss_plan_samples_linear(ctx, (const ptss_linear_moment*)dMoments, n, &linearParams, &linearPlan, n, (unsigned long long*)dCdf,
                                                     (uint32_t*)dIndex, (ptss_plan_info*)dInfo, NULL));
                if (t == adaptiveLinear) break;
                if (dPos) {
                    PTSS_HANDLE(ptss_generate_rays_positions(ctx, &fc, 0, (const uint32_t*)dIndex, n, (ptss_path_rng*)dRng, (ptss_ray_query*)dRays,
                                                             (ptss_film_position*)dPos, NULL));
                } else {
                    PTSS_HANDLE(ptss_generate_rays(ctx, &fc, 0, (const uint32_t*)dIndex, n, (ptss_path_rng*)dRng, (ptss_ray_query*)dRays, NULL));
                }
                PTSS_HANDLE(ptss_trace_paths_opt(ctx, (const ptss_ray_query*)dRays, (ptss_path_rng*)dRng, (ptss_path_result*)dRes, n, bounces, &pathOptions,
                                                 NULL));
                if (dPos) {   // planned rounds are not one sample per pixel: the scatter form, the moments by index pixel beside it
                    PTSS_HANDLE(ptss_splat_paths(ctx, (const ptss_path_result*)dRes, (const ptss_film_position*)dPos, n, (ptss_splat_entry*)dLinear, width,
                                                 height, &splatFilter, &linearParams, NULL));
                    PTSS_HANDLE(ptss_accumulate_paths_linear_stats(ctx, (const ptss_path_result*)dRes, (const uint32_t*)dIndex, 0, n, NULL,
                                                                   (ptss_linear_moment*)dMoments, n, &linearParams, NULL));
                } else {
                    PTSS_HANDLE(ptss_accumulate_paths_linear_stats(ctx, (const ptss_path_result*)dRes, (const uint32_t*)dIndex, 0, n,
                                                                   (ptss_linear_entry*)dLinear, (ptss_linear_moment*)dMoments, n, &linearParams, NULL));
                }
                if (autoExposure && meterRound((ticks > 0 ? ticks : 1) + t)) return 1;
            }
            PTSS_HANDLE(ptss_synchronize(ctx));
            ptss_plan_info info;
            if (hipMemcpy(&info, dInfo, sizeof(info), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "--adaptive-linear: read-back\n"); return 1; }
            printf("adaptive-linear: rounds %d totalWeight %llu activePixels %u unsampledPixels %u cappedPixels %u uniform %u\n", adaptiveLinear,
                   info.totalWeight, info.activePixels, info.unsampledPixels, info.cappedPixels, info.uniform);
        }
        if (adaptive >= 0) {   // the planned rounds: ray slot i keeps stream i whatever pixel the plan gives it
            ptss_plan_params plan;
            PTSS_HANDLE(ptss_default_plan_params(&plan));
            plan.minSamples = ticks > 0 ? (uint32_t)ticks : 1u;
            if (plan.maxSamples < plan.minSamples) plan.maxSamples = plan.minSamples;
            if (adaptiveThreshold >= 0.f) plan.threshold = adaptiveThreshold;
            for (int t = 0; t <= adaptive; ++t) {   // (the last plan only reports what the rounds left)
                PTSS_HANDLE(ptss_plan_samples(ctx, (const ptss_film_entry*)dFilm, (const unsigned long long*)dMoments, n, &plan, n,
                                              (unsigned long long*)dCdf, (uint32_t*)dIndex, (ptss_plan_info*)dInfo, NULL));
                if (t == adaptive) break;
                PTSS_HANDLE(ptss_generate_rays(ctx, &fc, 0, (const uint32_t*)dIndex, n, (ptss_path_rng*)dRng, (ptss_ray_query*)dRays, NULL));
                PTSS_HANDLE(ptss_trace_paths_opt(ctx, (const ptss_ray_query*)dRays, (ptss_path_rng*)dRng, (ptss_path_result*)dRes, n, bounces, &pathOptions,
                                                 NULL));
                PTSS_HANDLE(ptss_accumulate_paths_stats(ctx, (const ptss_path_result*)dRes, (const uint32_t*)dIndex, 0, n, (ptss_film_entry*)dFilm,
                                                        (unsigned long long*)dMoments, n, (ptss_uchar4*)bitmap.devPixels, (ptss_history_entry*)dHist, NULL));
            }
            PTSS_HANDLE(ptss_synchronize(ctx));
            ptss_plan_info info;
            if (hipMemcpy(&info, dInfo, sizeof(info), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "--adaptive: read-back\n"); return 1; }
            printf("adaptive: rounds %d totalWeight %llu activePixels %u unsampledPixels %u cappedPixels %u uniform %u\n", adaptive, info.totalWeight,
                   info.activePixels, info.unsampledPixels, info.cappedPixels, info.uniform);
        }
        if (carry) {
            PTSS_HANDLE(ptss_synchronize(ctx));
            ptss_reproject_linear_info info;
            if (hipMemcpy(&info, dCarryInfo, sizeof(info), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "--carry: read-back\n"); return 1; }
            printf("carry: seeded %llu offFilm %llu noTap %llu noVariance %llu\n", info.seeded, info.offFilm, info.noTap, info.noVariance);
        }
        if (linear >= 0.f) {   // the film resolved once: the screenshot's bytes, the filter's history, and the linear means as a PFM
            if (denoiseLinear && (!autoExposure || ticks <= 0) && denoiseFilm()) return 1;   // (with a meter the last round's denoised film stands)
            if (upscaleLinear != 0 && (!autoExposure || ticks <= 0) && upsampleFilm()) return 1;   // (... and its large film)
            if (autoExposure) {   // (the last round's metered resolve stands; without a round the new state's exposure, 0, shows black)
                if (ticks <= 0 && meteredResolve()) return 1;
                PTSS_HANDLE(ptss_synchronize(ctx));
                ptss_meter_state state;
                if (hipMemcpy(&state, dMeter, sizeof(state), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "--auto-exposure: read-back\n"); return 1; }
                printf("auto-exposure: exposure %.9g target %.9g meanLog2 %.9g updates %u metered %llu black %llu counted %llu sumLog %llu\n", state.exposure,
                       state.target, state.meanLog2, state.updates, state.metered, state.black, state.counted, state.sumLog);
            }
            if (toneCurve >= 0) {   // the finished film through the tone curve, with the meter's state and the glare pyramid where there are any
                const ptss_meter_state* state = autoExposure ? (const ptss_meter_state*)dMeter : NULL;
                ptss_tone_params tone;
                PTSS_HANDLE(ptss_default_tone_params(&tone));
                tone.curve = toneCurve;
                tone.transfer = toneSrgb ? PTSS_TRANSFER_SRGB : PTSS_TRANSFER_GAMMA22;
                tone.flags = toneLuminance ? PTSS_TONE_LUMINANCE : 0u;
                if (toneWhite > 0.f) tone.white = toneWhite;
                void* dToneTable = nullptr;
                if (hipMalloc(&dToneTable, ptss_tone_table_floats(tone.bits) * sizeof(float)) != hipSuccess) { fprintf(stderr, "--tone: device buffers\n"); return 1; }
                PTSS_HANDLE(ptss_tone_build(ctx, &tone, (float*)dToneTable, NULL));
                if (glare)
                    PTSS_HANDLE(ptss_glare_build(ctx, shown, shownSplat ? PTSS_GLARE_FILM_SPLAT : PTSS_GLARE_FILM_LINEAR, shownW, shownH, &linearParams,
                                                 &glareParams, (ptss_glare_entry*)dPyramid, NULL));
                PTSS_HANDLE(ptss_resolve_toned(ctx, shown, shownSplat ? PTSS_FILM_SPLAT : PTSS_FILM_LINEAR, 0, shownN, &linearParams, &tone,
                                               (const float*)dToneTable, state, shownW, shownH, glare ? &glareParams : NULL,
                                               glare ? (const ptss_glare_entry*)dPyramid : NULL, (ptss_history_entry*)dShownMeans, (uint32_t*)dShownPixels,
                                               (ptss_history_entry*)dShownHist, NULL));
                PTSS_HANDLE(ptss_synchronize(ctx));
                float flag = 1.f;   // T[K + 2]: 0 where the thresholds are in order
                if (hipMemcpy(&flag, (const float*)dToneTable + (1 << tone.bits) + 1, sizeof(float), hipMemcpyDeviceToHost) != hipSuccess || flag != 0.f) {
                    fprintf(stderr, "--tone: the table's thresholds are not in order\n");
                    return 1;
                }
                (void)hipFree(dToneTable);
            } else if (glare) {   // the pyramid of the finished film, and the resolve that adds it: at the meter's exposure where there is one
                const ptss_meter_state* state = autoExposure ? (const ptss_meter_state*)dMeter : NULL;
                PTSS_HANDLE(ptss_glare_build(ctx, shown, shownSplat ? PTSS_GLARE_FILM_SPLAT : PTSS_GLARE_FILM_LINEAR, shownW, shownH, &linearParams, &glareParams,
                                             (ptss_glare_entry*)dPyramid, NULL));
                if (shownSplat) {
                    PTSS_HANDLE(ptss_resolve_splat_glare(ctx, (const ptss_splat_entry*)shown, 0, shownN, &linearParams, shownW, shownH, &glareParams,
                                                         (const ptss_glare_entry*)dPyramid, state, (ptss_history_entry*)dShownMeans,
                                                         (ptss_uchar4*)dShownPixels, (ptss_history_entry*)dShownHist, NULL));
                } else {
                    PTSS_HANDLE(ptss_resolve_linear_glare(ctx, (const ptss_linear_entry*)shown, 0, shownN, &linearParams, shownW, shownH, &glareParams,
                                                          (const ptss_glare_entry*)dPyramid, state, (ptss_history_entry*)dShownMeans,
                                                          (ptss_uchar4*)dShownPixels, (ptss_history_entry*)dShownHist, NULL));
                }
            } else if (!autoExposure && shownSplat) {
                PTSS_HANDLE(ptss_resolve_splat(ctx, (const ptss_splat_entry*)shown, 0, shownN, &linearParams, (ptss_history_entry*)dShownMeans,
                                               (ptss_uchar4*)dShownPixels, (ptss_history_entry*)dShownHist, NULL));
            } else if (!autoExposure) {
                PTSS_HANDLE(ptss_resolve_linear(ctx, (const ptss_linear_entry*)shown, 0, shownN, &linearParams, (ptss_history_entry*)dShownMeans,
                                                (ptss_uchar4*)dShownPixels, (ptss_history_entry*)dShownHist, NULL));
            }
            PTSS_HANDLE(ptss_synchronize(ctx));
            std::vector<ptss_history_entry> means(shownN);
            if (hipMemcpy(means.data(), dShownMeans, shownN * sizeof(ptss_history_entry), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "--linear: read-back\n"); return 1; }
            if (upscaleLinear != 0) {   // the large image is this option's to write: the screenshot below is of the display buffer, at the small size
                ptss_upsample_linear_info info;
                std::vector<ptss_uchar4> host(shownN);
                if (hipMemcpy(&info, dBigInfo, sizeof(info), hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(host.data(), dBigPixels, shownN * sizeof(ptss_uchar4), hipMemcpyDeviceToHost) != hipSuccess) {
                    fprintf(stderr, "--upscale-linear: read-back\n");
                    return 1;
                }
                printf("upscale-linear: factor %d filtered %llu fallback %llu empty %llu\n", upscaleLinear, info.filtered, info.fallback, info.empty);
                if (!writeTga(out.c_str(), host.data(), shownW, shownH)) fprintf(stderr, "--upscale-linear: cannot write %s\n", out.c_str());
            }
            std::string name = out;
            const size_t dot = name.rfind(".tga");
            if (dot != std::string::npos && dot + 4 == name.size()) name.erase(dot);
            name += ".pfm";
            if (!writePfm(name.c_str(), means.data(), shownW, shownH)) fprintf(stderr, "--linear: cannot write %s\n", name.c_str());
        }
        if (filter && ticks > 0) {   // the features of the film's pixel centres, then the filter over the film's display values
            ptss_denoise_params params;
            PTSS_HANDLE(ptss_default_denoise_params(&params));
            if (denoise >= 0) params.levels = denoise;
            fc.jitter = 0;
            PTSS_HANDLE(ptss_generate_rays(ctx, &fc, 0, NULL, n, (ptss_path_rng*)dRng, (ptss_ray_query*)dRays, NULL));
            PTSS_HANDLE(ptss_ray_features(ctx, (const ptss_ray_query*)dRays, (ptss_pixel_feature*)dFeat, n, NULL));
            PTSS_HANDLE(ptss_denoise_history(ctx, (const ptss_history_entry*)dHist, (const ptss_pixel_feature*)dFeat, &params, (ptss_uchar4*)dOut, NULL));
            PTSS_HANDLE(ptss_synchronize(ctx));
            std::vector<ptss_uchar4> host(n);
            if (hipMemcpy(host.data(), dOut, n * sizeof(ptss_uchar4), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "--film --denoise: read-back\n"); return 1; }
            std::string name = out;
            const size_t dot = name.rfind(".tga");
            if (dot != std::string::npos && dot + 4 == name.size()) name.erase(dot);
            name += "_denoised.tga";
            if (!writeTga(name.c_str(), host.data(), width, height)) fprintf(stderr, "--film --denoise: cannot write %s\n", name.c_str());
        }
        PTSS_HANDLE(ptss_synchronize(ctx));
        for (void* p : {dRng, dRays, dRes, dFilm, dHist, dFeat, dOut, dMoments, dCdf, dIndex, dInfo, dLinear, dMeans, dPos, dBins, dMeter, dPyramid, dClean, dCleanFeat, dCleanWork, dCarryPrev, dCarryNow, dCarryFilm, dCarryMoments, dCarryInfo, dBigFilm, dBigMeans, dBigPixels, dBigFeat, dSmallFeat, dBigInfo}) (void)hipFree(p);
    } else {
        for (char k : keys) bitmap.push_key((unsigned char)k);
        bitmap.anim_and_exit((void (*)(uchar4*, void*, int))generateFrame, NULL, (void (*)(unsigned char, int, int))Key);
    }

    if (!quiet) printf("\n");
    if (!out.empty() && !temporal && upscaleLinear == 0) {
        char name[160];
        strncpy(name, out.c_str(), sizeof(name) - 1);
        name[sizeof(name) - 1] = 0;
        saveScreenshot(name, width, height);
    }
    if (denoise != -2 && film.empty()) {   // the denoised twin of the screenshot: features of the final camera, then the filter
        ptss_denoise_params params;
        PTSS_HANDLE(ptss_default_denoise_params(&params));
        if (denoise >= 0) params.levels = denoise;
        const size_t n = (size_t)width * (size_t)height;
        void *df = nullptr, *dp = nullptr;
        if (hipMalloc(&df, n * sizeof(ptss_pixel_feature)) != hipSuccess || hipMalloc(&dp, n * sizeof(ptss_uchar4)) != hipSuccess) {
            fprintf(stderr, "--denoise: device buffers\n");
            return 1;
        }
        if (specularSteps >= 0) {
            PTSS_HANDLE(ptss_render_features_specular(ctx, specularSteps, (ptss_pixel_feature*)df, NULL, NULL));
        } else {
            PTSS_HANDLE(ptss_render_features(ctx, (ptss_pixel_feature*)df, NULL));
        }
        PTSS_HANDLE(ptss_denoise(ctx, (const ptss_pixel_feature*)df, &params, (ptss_uchar4*)dp, NULL));
        PTSS_HANDLE(ptss_synchronize(ctx));
        std::vector<ptss_uchar4> host(n);
        if (hipMemcpy(host.data(), dp, n * sizeof(ptss_uchar4), hipMemcpyDeviceToHost) != hipSuccess) {
            fprintf(stderr, "--denoise: read-back\n");
            return 1;
        }
        if (upscale != 0 && writeUpscaled(dp) != 0) return 1;
        (void)hipFree(df);
        (void)hipFree(dp);
        std::string name = out;
        const size_t dot = name.rfind(".tga");
        if (dot != std::string::npos && dot + 4 == name.size()) name.erase(dot);
        name += "_denoised.tga";
        if (!writeTga(name.c_str(), host.data(), width, height)) fprintf(stderr, "--denoise: cannot write %s\n", name.c_str());
    }
    if (upscale != 0 && denoise == -2 && !temporal && writeUpscaled(bitmap.devPixels) != 0) return 1;
    if (!picks.empty()) {   // picking: the pixel-centre ray of the final camera through ptss_intersect
        std::vector<ptss_ray_query> q;
        for (const auto& p : picks) q.push_back(cameraRay(data->camera, width, height, p.first, p.second, 0.5f, 0.5f));
        std::vector<ptss_ray_hit> h(q.size());
        void *dq = nullptr, *dh = nullptr;
        if (hipMalloc(&dq, q.size() * sizeof(ptss_ray_query)) != hipSuccess || hipMalloc(&dh, h.size() * sizeof(ptss_ray_hit)) != hipSuccess ||
            hipMemcpy(dq, q.data(), q.size() * sizeof(ptss_ray_query), hipMemcpyHostToDevice) != hipSuccess) {
            fprintf(stderr, "--pick: device buffers\n");
            return 1;
        }
        PTSS_HANDLE(ptss_intersect(ctx, (const ptss_ray_query*)dq, (ptss_ray_hit*)dh, q.size(), NULL));
        PTSS_HANDLE(ptss_synchronize(ctx));
        if (hipMemcpy(h.data(), dh, h.size() * sizeof(ptss_ray_hit), hipMemcpyDeviceToHost) != hipSuccess) {
            fprintf(stderr, "--pick: read-back\n");
            return 1;
        }
        (void)hipFree(dq);
        (void)hipFree(dh);
        static const char* kinds[] = {"miss", "sphere", "triangle"};
        for (size_t i = 0; i < h.size(); ++i)
            printf("pick %d,%d: %s %d material %d distance %.9g point %.9g %.9g %.9g\n", picks[i].first, picks[i].second,
                   kinds[h[i].kind >= 0 && h[i].kind <= 2 ? h[i].kind : 0], h[i].primitive, h[i].materialIdx, h[i].distance, h[i].point.x,
                   h[i].point.y, h[i].point.z);
    }
    const unsigned long long rays = totalRayBounces(data);
    printf("%d ticks, %llu ray-bounces, last pass %.3f ms", ticks, rays, data->lastPassMs);
    if (gpus > 0) printf(", %d shard(s) on %s, gathered by %s", gpus, emulate ? "device 0" : "as many GPUs", emulate ? "device copies" : "ncclGather");
    printf("\n");

    // free (:731-740)
    if (gpus > 0) destroyShards(data);
    else PTSS_HANDLE(ptss_destroy(ctx));
    bitmap.free_resources();
    delete data;
    return 0;
}
