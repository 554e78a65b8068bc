// ptss_api_film.hip — the film of a path query and everything downstream of it that works on caller buffers: film, adaptive,
// linear, linear stats and splat accumulation with their plans; meter, glare, the resolves, tone, the linear denoiser, linear
// reproject and upsample; surface rays and dilate; the light-map lookups. Like the queries (ptss_api_query.hip) these calls run on
// the caller's stream and touch no frame state: of the context they read the device number, the default stream and images[0]
// (its thresholds and materials) at most, count into dTotal's film, splat and surface words (TotalWord), and write only their own
// counters, forms and last streams (ptss_context.h, second block).
#include "ptss_context.h"
#include "ptcamera.h"
#include "ptadaptive.h"
#include "ptlinstats.h"
#include "ptglare.h"
#include "pttone.h"
#include "ptlinup.h"
#include "ptsurface.h"
#include "ptlightmap.h"

extern "C" {

// ---- the film of a path query (ptss_film.hip) ----
// What the film calls share behind their own ctx and params checks, in the order each of them checks it: the film's size, n == 0 (nothing
// to do: PTSS_OK with go == false), the call's own verdict on its buffers (`badBuffers`: null first, then alignment; evaluated by the caller,
// reported here), n, firstPixel + n against the film where there is no index, the scene image where the call reads it, device and stream.
struct FilmCall {
    bool go = false;
    hipStream_t st = nullptr;
    uint32_t firstPixel = 0, n = 0, filmPixels = 0;   // firstPixel as the launch takes it: 0 with an index
    const float* quantTable = nullptr;                // the frame's own thresholds (frameBuffers); with a scene image only
};

static int filmCall(ptss_context* c, FilmCall* f, unsigned long long filmPixels, const char* filmTooLarge, size_t n, const char* badBuffers,
                    const uint32_t* dev_index, size_t firstPixel, bool readsImage, void* hipStream) {
    if (!fits31(filmPixels)) return fail(PTSS_ERANGE, filmTooLarge);
    if (n == 0) return PTSS_OK;
    if (badBuffers) return fail(PTSS_EINVAL, badBuffers);
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    if (!dev_index && (firstPixel > filmPixels || n > filmPixels - firstPixel)) return fail(PTSS_ERANGE, "firstPixel + n leaves the film");
    if (readsImage && !sceneImageOf(c)) return PTSS_EINVAL;
    HIP_TRY(hipSetDevice(c->cfg.device));
    *f = FilmCall{true, streamOf(c, hipStream), dev_index ? 0u : (uint32_t)firstPixel, (uint32_t)n, (uint32_t)filmPixels,
                  readsImage ? quantTableOf(c->images[0]) : nullptr};
    return PTSS_OK;
}

// a launch with an index may count rejected entries: ptss_film_rejected synchronises on its stream
static void noteFilmIndex(ptss_context* c, const uint32_t* dev_index, hipStream_t st) {
    if (dev_index) c->lastFilmIndex.note(st);
}

static int filmKindCheck(int filmKind) {
    return filmKind != PTSS_FILM_LINEAR && filmKind != PTSS_FILM_SPLAT ? fail(PTSS_EINVAL, "unknown film kind") : PTSS_OK;
}

static const char* const kNullBuffer = "null buffer with n > 0";

int ptss_generate_rays(ptss_context* c, const ptss_film_camera* film, size_t firstPixel, const uint32_t* dev_index, size_t n, ptss_path_rng* dev_rng,
                       ptss_ray_query* dev_rays, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptcam::cameraError(film)) return fail(PTSS_EINVAL, what);
    const char* bad = !dev_rng || !dev_rays ? kNullBuffer
                      : ((uintptr_t)dev_rays & 15u) || (((uintptr_t)dev_rng | (uintptr_t)dev_index) & 3u)
                          ? "rays must be 16-byte aligned, dev_rng and dev_index 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(filmCall(c, &f, (unsigned long long)film->width * (unsigned long long)film->height, "width * height must be below 2^31", n, bad, dev_index,
                    firstPixel, false, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchFilmRays(f.st, ptcam::filmOf(*film), f.firstPixel, dev_index, f.n, dev_rng, dev_rays, nullptr,
                                 c->dTotal + kFilmRejectedWord, &c->filmLaunches[0]));
    noteFilmIndex(c, dev_index, f.st);
    return PTSS_OK;
}

int ptss_accumulate_paths(ptss_context* c, const ptss_path_result* dev_results, const uint32_t* dev_index, size_t firstPixel, size_t n,
                          ptss_film_entry* dev_film, size_t filmPixels, ptss_uchar4* dev_pixels, ptss_history_entry* dev_history, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    const char* bad = !dev_results || !dev_film ? kNullBuffer
                      : (((uintptr_t)dev_results | (uintptr_t)dev_film | (uintptr_t)dev_history) & 15u) ||
                              (((uintptr_t)dev_index | (uintptr_t)dev_pixels) & 3u)
                          ? "results, film and history must be 16-byte aligned, dev_index and dev_pixels 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(filmCall(c, &f, filmPixels, "filmPixels must be below 2^31", n, bad, dev_index, firstPixel, true, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchFilmAccumulate(f.st, dev_results, dev_index, f.firstPixel, f.n, dev_film, f.filmPixels, dev_pixels, dev_history, f.quantTable,
                                       c->dTotal + kFilmRejectedWord, &c->filmLaunches[1]));
    noteFilmIndex(c, dev_index, f.st);
    return PTSS_OK;
}

int ptss_film_launches(const ptss_context* c, unsigned long long* out3) { return readLaunches(c, &ptss_context::filmLaunches, out3); }

int ptss_film_rejected(ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    return readBehind(c, c->lastFilmIndex, c->dTotal + kFilmRejectedWord, 1, out);
}

// ---- adaptive film sampling (ptss_adaptive.hip; csrc/ptadaptive.h). ----
int ptss_accumulate_paths_stats(ptss_context* c, const ptss_path_result* dev_results, const uint32_t* dev_index, size_t firstPixel, size_t n,
                                ptss_film_entry* dev_film, unsigned long long* dev_moments, size_t filmPixels, ptss_uchar4* dev_pixels,
                                ptss_history_entry* dev_history, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    const char* bad = !dev_results || !dev_film || !dev_moments ? kNullBuffer
                      : (((uintptr_t)dev_results | (uintptr_t)dev_film | (uintptr_t)dev_history) & 15u) ||
                              (((uintptr_t)dev_index | (uintptr_t)dev_pixels) & 3u) || ((uintptr_t)dev_moments & 7u)
                          ? "results, film and history must be 16-byte aligned, dev_moments 8-byte, dev_index and dev_pixels 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(filmCall(c, &f, filmPixels, "filmPixels must be below 2^31", n, bad, dev_index, firstPixel, true, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchStatsAccumulate(f.st, dev_results, dev_index, f.firstPixel, f.n, dev_film, dev_moments, f.filmPixels, dev_pixels, dev_history,
                                        f.quantTable, c->dTotal + kFilmRejectedWord, &c->adaptiveLaunches[0]));
    noteFilmIndex(c, dev_index, f.st);
    return PTSS_OK;
}

int ptss_default_plan_params(ptss_plan_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_plan_params);
    p->minSamples = 8u;
    p->maxSamples = ptad::kSampleLimit;
    p->threshold = 0.5f;
    return PTSS_OK;
}

int ptss_plan_cdf_entries(size_t filmPixels, size_t* entries) {
    if (!entries) return fail(PTSS_EINVAL, "entries is null");
    if (filmPixels == 0 || !fits31(filmPixels)) return fail(PTSS_ERANGE, "filmPixels must be in [1, 2^31)");
    *entries = (size_t)ptad::cdfEntries(filmPixels);
    return PTSS_OK;
}

// What the two plan calls share behind their own ctx and params checks, in this order: the film's size, n, n == 0 (nothing to do: PTSS_OK
// with go == false), the call's own verdict on its buffers (FilmCall's `badBuffers`), device and stream. FilmCall's firstPixel stays 0
static int planCall(ptss_context* c, FilmCall* f, size_t filmPixels, size_t n, const char* badBuffers, void* hipStream) {
    if (filmPixels == 0 || !fits31(filmPixels)) return fail(PTSS_ERANGE, "filmPixels must be in [1, 2^31)");
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    if (n == 0) return PTSS_OK;
    if (badBuffers) return fail(PTSS_EINVAL, badBuffers);
    HIP_TRY(hipSetDevice(c->cfg.device));
    *f = FilmCall{true, streamOf(c, hipStream), 0u, (uint32_t)n, (uint32_t)filmPixels, nullptr};
    return PTSS_OK;
}

int ptss_plan_samples(ptss_context* c, const ptss_film_entry* dev_film, const unsigned long long* dev_moments, size_t filmPixels,
                      const ptss_plan_params* params, size_t n, unsigned long long* dev_cdf, uint32_t* dev_index, ptss_plan_info* dev_info,
                      void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptad::paramsError(params)) return fail(PTSS_EINVAL, what);
    const char* bad = !dev_film || !dev_moments || !dev_cdf || !dev_index ? kNullBuffer
                      : ((uintptr_t)dev_film & 15u) || (((uintptr_t)dev_moments | (uintptr_t)dev_cdf | (uintptr_t)dev_info) & 7u) || ((uintptr_t)dev_index & 3u)
                          ? "film must be 16-byte aligned, dev_moments, dev_cdf and dev_info 8-byte, dev_index 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(planCall(c, &f, filmPixels, n, bad, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchPlanSamples(f.st, dev_film, dev_moments, f.filmPixels, *params, f.n, dev_cdf, dev_index, dev_info, &c->adaptiveLaunches[1]));
    return PTSS_OK;
}

int ptss_adaptive_launches(const ptss_context* c, unsigned long long* out2) { return readLaunches(c, &ptss_context::adaptiveLaunches, out2); }

// ---- the linear film (ptss_linear.hip; csrc/ptlinear.h). ----
int ptss_default_linear_params(ptss_linear_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_linear_params);
    p->scaleLog2 = 20;
    p->clampMax = 65536.f;
    p->exposure = 1.f;
    p->reserved = 0u;
    return PTSS_OK;
}

int ptss_accumulate_paths_linear(ptss_context* c, const ptss_path_result* dev_results, const uint32_t* dev_index, size_t firstPixel, size_t n,
                                 ptss_linear_entry* dev_film, size_t filmPixels, const ptss_linear_params* params, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlin::paramsError(params)) return fail(PTSS_EINVAL, what);
    const char* bad = !dev_results || !dev_film ? kNullBuffer
                      : (((uintptr_t)dev_results | (uintptr_t)dev_film) & 15u) || ((uintptr_t)dev_index & 3u)
                          ? "results and film must be 16-byte aligned, dev_index 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(filmCall(c, &f, filmPixels, "filmPixels must be below 2^31", n, bad, dev_index, firstPixel, true, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchLinearAccumulate(f.st, dev_results, dev_index, f.firstPixel, f.n, dev_film, nullptr, f.filmPixels, *params,
                                         c->dTotal + kFilmRejectedWord, &c->linearLaunches[0]));
    noteFilmIndex(c, dev_index, f.st);
    return PTSS_OK;
}

int ptss_linear_launches(const ptss_context* c, unsigned long long* out2) { return readLaunches(c, &ptss_context::linearLaunches, out2); }

// ---- adaptive sampling on the linear film (ptss_linear.hip, ptss_adaptive.hip; csrc/ptlinstats.h) ----
int ptss_default_linear_plan_params(ptss_linear_plan_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_linear_plan_params);
    p->minSamples = 8u;
    p->maxSamples = ptad::kSampleLimit;
    p->threshold = 0.02f;
    p->floor = 0.015625f;
    p->reserved[0] = p->reserved[1] = p->reserved[2] = 0u;
    return PTSS_OK;
}

int ptss_accumulate_paths_linear_stats(ptss_context* c, const ptss_path_result* dev_results, const uint32_t* dev_index, size_t firstPixel, size_t n,
                                       ptss_linear_entry* dev_film, ptss_linear_moment* dev_moments, size_t filmPixels,
                                       const ptss_linear_params* params, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlin::paramsError(params)) return fail(PTSS_EINVAL, what);
    const char* bad = !dev_results || !dev_moments ? kNullBuffer
                      : (((uintptr_t)dev_results | (uintptr_t)dev_film | (uintptr_t)dev_moments) & 15u) || ((uintptr_t)dev_index & 3u)
                          ? "results, film and moments must be 16-byte aligned, dev_index 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(filmCall(c, &f, filmPixels, "filmPixels must be below 2^31", n, bad, dev_index, firstPixel, true, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchLinearAccumulate(f.st, dev_results, dev_index, f.firstPixel, f.n, dev_film, dev_moments, f.filmPixels, *params,
                                         c->dTotal + kFilmRejectedWord, &c->linStatsLaunches[0]));
    noteFilmIndex(c, dev_index, f.st);
    return PTSS_OK;
}

int ptss_plan_samples_linear(ptss_context* c, const ptss_linear_moment* dev_moments, size_t filmPixels, const ptss_linear_params* params,
                             const ptss_linear_plan_params* plan, size_t n, unsigned long long* dev_cdf, uint32_t* dev_index,
                             ptss_plan_info* dev_info, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlin::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptls::paramsError(plan, params)) return fail(PTSS_EINVAL, what);
    const char* bad = !dev_moments || !dev_cdf || !dev_index ? kNullBuffer
                      : ((uintptr_t)dev_moments & 15u) || (((uintptr_t)dev_cdf | (uintptr_t)dev_info) & 7u) || ((uintptr_t)dev_index & 3u)
                          ? "moments must be 16-byte aligned, dev_cdf and dev_info 8-byte, dev_index 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(planCall(c, &f, filmPixels, n, bad, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchPlanSamplesLinear(f.st, dev_moments, f.filmPixels, *params, *plan, f.n, dev_cdf, dev_index, dev_info, &c->linStatsLaunches[1]));
    return PTSS_OK;
}

int ptss_linear_stats_launches(const ptss_context* c, unsigned long long* out2) { return readLaunches(c, &ptss_context::linStatsLaunches, out2); }

// ---- the filtered linear film (ptss_splat.hip; csrc/ptsplat.h). ----
int ptss_default_splat_filter(ptss_splat_filter* f) {
    if (!f) return fail(PTSS_EINVAL, "filter is null");
    f->structSize = (unsigned int)sizeof(ptss_splat_filter);
    f->kind = PTSS_SPLAT_TENT;
    f->radius = 1.f;
    f->alpha = 2.f;
    f->reserved = 0u;
    return PTSS_OK;
}

int ptss_generate_rays_positions(ptss_context* c, const ptss_film_camera* film, size_t firstPixel, const uint32_t* dev_index, size_t n,
                                 ptss_path_rng* dev_rng, ptss_ray_query* dev_rays, ptss_film_position* dev_positions, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptcam::cameraError(film)) return fail(PTSS_EINVAL, what);
    if (!dev_positions) return fail(PTSS_EINVAL, "dev_positions is null (ptss_generate_rays makes rays without positions)");
    const char* bad = !dev_rng || !dev_rays ? kNullBuffer
                      : ((uintptr_t)dev_rays & 15u) || ((uintptr_t)dev_positions & 7u) || (((uintptr_t)dev_rng | (uintptr_t)dev_index) & 3u)
                          ? "rays must be 16-byte aligned, dev_positions 8-byte, dev_rng and dev_index 4-byte aligned"
                          : nullptr;
    FilmCall f;
    RC_TRY(filmCall(c, &f, (unsigned long long)film->width * (unsigned long long)film->height, "width * height must be below 2^31", n, bad, dev_index,
                    firstPixel, false, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchFilmRays(f.st, ptcam::filmOf(*film), f.firstPixel, dev_index, f.n, dev_rng, dev_rays, dev_positions,
                                 c->dTotal + kFilmRejectedWord, &c->filmLaunches[0]));
    noteFilmIndex(c, dev_index, f.st);
    return PTSS_OK;
}

// what the two splat calls check in front of filmCall: ctx, filter, params, the film's sides
static int splatArguments(const ptss_context* c, const ptss_splat_filter* filter, const ptss_linear_params* params, int width, int height) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptspl::filterError(filter)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlin::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (width < 1 || height < 1 || width > ptspl::kMaxFilmSide || height > ptspl::kMaxFilmSide)
        return fail(PTSS_ERANGE, "width and height must be in [1, 2^22]");
    return PTSS_OK;
}

static const char* splatBuffersError(const ptss_path_result* dev_results, const ptss_film_position* dev_positions, const ptss_splat_entry* dev_film) {
    return !dev_results || !dev_positions || !dev_film ? kNullBuffer
           : (((uintptr_t)dev_results | (uintptr_t)dev_film) & 15u) || ((uintptr_t)dev_positions & 7u)
               ? "results and film must be 16-byte aligned, dev_positions 8-byte aligned"
               : nullptr;
}

int ptss_splat_paths(ptss_context* c, const ptss_path_result* dev_results, const ptss_film_position* dev_positions, size_t n,
                     ptss_splat_entry* dev_film, int width, int height, const ptss_splat_filter* filter, const ptss_linear_params* params,
                     void* hipStream) {
    RC_TRY(splatArguments(c, filter, params, width, height));
    FilmCall f;   // (positions take the place of an index: n is not bound by the film)
    RC_TRY(filmCall(c, &f, (unsigned long long)width * (unsigned long long)height, "width * height must be below 2^31", n,
                    splatBuffersError(dev_results, dev_positions, dev_film), reinterpret_cast<const uint32_t*>(dev_positions), 0, false, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchSplatScatter(f.st, dev_results, dev_positions, f.n, dev_film, width, height, *filter, *params, c->dTotal + kSplatCountersWord,
                                     &c->splatLaunches[0]));
    c->lastSplat.note(f.st);   // ptss_splat_stats reads the device counters behind it
    return PTSS_OK;
}

int ptss_splat_paths_homed(ptss_context* c, const ptss_path_result* dev_results, const ptss_film_position* dev_positions, size_t firstPixel, size_t n,
                           ptss_splat_entry* dev_film, int width, int height, const ptss_splat_filter* filter, const ptss_linear_params* params,
                           void* hipStream) {
    RC_TRY(splatArguments(c, filter, params, width, height));
    FilmCall f;
    RC_TRY(filmCall(c, &f, (unsigned long long)width * (unsigned long long)height, "width * height must be below 2^31", n,
                    splatBuffersError(dev_results, dev_positions, dev_film), nullptr, firstPixel, false, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchSplatHomed(f.st, dev_results, dev_positions, f.firstPixel, f.n, dev_film, width, height, *filter, *params,
                                   c->dTotal + kSplatCountersWord, &c->splatLaunches[1]));
    c->lastSplat.note(f.st);   // ptss_splat_stats reads the device counters behind it
    return PTSS_OK;
}

int ptss_splat_stats(ptss_context* c, unsigned long long* out5) {
    RC_TRY(readLaunches(c, &ptss_context::splatLaunches, out5));
    out5[3] = out5[4] = 0;
    return c->lastSplat.set ? readBehind(c, c->lastSplat, c->dTotal + kSplatCountersWord, 2, out5 + 3) : PTSS_OK;
}

// ---- the meter of the two linear films (ptss_meter.hip; csrc/ptmeter.h). ----
int ptss_default_meter_params(ptss_meter_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_meter_params);
    p->key = 0.18f;
    p->lowPermille = 100u;
    p->highPermille = 20u;
    p->rate = 1.f;
    p->minExposure = 1.f / 65536.f;
    p->maxExposure = 65536.f;
    p->reserved = 0u;
    return PTSS_OK;
}

// What the calls over a range of a film share behind their own ctx and params checks, in ptss_resolve_linear's order: count == 0 (nothing
// to do: PTSS_OK with go == false), the call's own verdict on its buffers (FilmCall's `badBuffers`), the range, the scene image where the
// call reads it, `writes` (a call none of whose outputs is there has nothing to do either, and does not touch the device), device and
// stream. FilmCall's firstPixel and n are the range; filmPixels stays 0
static int rangeCall(ptss_context* c, FilmCall* f, size_t firstPixel, size_t count, const char* badBuffers, bool readsImage, bool writes,
                     void* hipStream) {
    if (count == 0) return PTSS_OK;
    if (badBuffers) return fail(PTSS_EINVAL, badBuffers);
    if (!fits31(firstPixel) || !fits31(count) || !fits31(firstPixel + count)) return fail(PTSS_ERANGE, "firstPixel + count must be below 2^31");
    if (readsImage && !sceneImageOf(c)) return PTSS_EINVAL;
    if (!writes) return PTSS_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    *f = FilmCall{true, streamOf(c, hipStream), (uint32_t)firstPixel, (uint32_t)count, 0u, readsImage ? quantTableOf(c->images[0]) : nullptr};
    return PTSS_OK;
}

static int meterFilm(ptss_context* c, const void* dev_film, bool splat, size_t firstPixel, size_t count, uint32_t* dev_histogram, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    const char* bad = !dev_film || !dev_histogram ? "null film or histogram with count > 0"
                      : ((uintptr_t)dev_film & 15u) || ((uintptr_t)dev_histogram & 3u) ? "film must be 16-byte aligned, dev_histogram 4-byte aligned"
                                                                                         : nullptr;
    FilmCall f;
    RC_TRY(rangeCall(c, &f, firstPixel, count, bad, false, true, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchMeterHistogram(f.st, dev_film, splat, f.firstPixel, f.n, dev_histogram, &c->meterLaunches[0]));
    return PTSS_OK;
}

int ptss_meter_linear(ptss_context* c, const ptss_linear_entry* dev_film, size_t firstPixel, size_t count, uint32_t* dev_histogram, void* hipStream) {
    return meterFilm(c, dev_film, false, firstPixel, count, dev_histogram, hipStream);
}

int ptss_meter_splat(ptss_context* c, const ptss_splat_entry* dev_film, size_t firstPixel, size_t count, uint32_t* dev_histogram, void* hipStream) {
    return meterFilm(c, dev_film, true, firstPixel, count, dev_histogram, hipStream);
}

int ptss_meter_exposure(ptss_context* c, const uint32_t* dev_histogram, const ptss_linear_params* params, const ptss_meter_params* meter,
                        ptss_meter_state* dev_state, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlin::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptmeter::paramsError(meter)) return fail(PTSS_EINVAL, what);
    if (!dev_histogram || !dev_state) return fail(PTSS_EINVAL, "null histogram or state");
    if (((uintptr_t)dev_histogram & 3u) || ((uintptr_t)dev_state & 7u)) return fail(PTSS_EINVAL, "dev_histogram must be 4-byte aligned, dev_state 8-byte aligned");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchMeterExposure(streamOf(c, hipStream), dev_histogram, *params, *meter, dev_state, &c->meterLaunches[1]));
    return PTSS_OK;
}

int ptss_meter_launches(const ptss_context* c, unsigned long long* out3) { return readLaunches(c, &ptss_context::meterLaunches, out3); }

// ---- glare for the two linear films (ptss_glare.hip; csrc/ptglare.h). ----
int ptss_default_glare_params(ptss_glare_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_glare_params);
    p->levels = 6;
    p->mode = PTSS_GLARE_MIX;
    p->threshold = 0.f;
    p->strength = 0.1f;
    p->reserved = 0u;
    return PTSS_OK;
}

int ptss_glare_layout(int width, int height, int levels, ptss_glare_level out[8], size_t* entries) {
    if (!out || !entries) return fail(PTSS_EINVAL, "null argument");
    if (levels < 1 || levels > ptglare::kMaxLevels) return fail(PTSS_EINVAL, "levels must be in [1, 8]");
    if (const char* what = ptglare::sidesError(width, height)) return fail(PTSS_ERANGE, what);
    *entries = ptglare::layoutOf(width, height, levels, out);
    return PTSS_OK;
}

// what the glare calls check first: ctx, the film's parameters, the glare's, the film's kind and its sides
static int glareArguments(const ptss_context* c, const ptss_linear_params* params, const ptss_glare_params* glare, int filmKind, int width, int height) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlin::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptglare::paramsError(glare, *params)) return fail(PTSS_EINVAL, what);
    RC_TRY(filmKindCheck(filmKind));   // (PTSS_GLARE_FILM_* are PTSS_FILM_*)
    if (const char* what = ptglare::sidesError(width, height)) return fail(PTSS_ERANGE, what);
    return PTSS_OK;
}

int ptss_glare_build(ptss_context* c, const void* dev_film, int filmKind, int width, int height, const ptss_linear_params* params,
                     const ptss_glare_params* glare, ptss_glare_entry* dev_pyramid, void* hipStream) {
    RC_TRY(glareArguments(c, params, glare, filmKind, width, height));
    if (!dev_film || !dev_pyramid) return fail(PTSS_EINVAL, "null film or pyramid");
    if (((uintptr_t)dev_film | (uintptr_t)dev_pyramid) & 15u) return fail(PTSS_EINVAL, "film and pyramid must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchGlareBuild(streamOf(c, hipStream), dev_film, filmKind == PTSS_GLARE_FILM_SPLAT, width, height, *params, *glare, dev_pyramid,
                                   c->glareLaunches));
    return PTSS_OK;
}

int ptss_glare_launches(const ptss_context* c, unsigned long long* out3) { return readLaunches(c, &ptss_context::glareLaunches, out3); }

// ---- the denoiser of the two linear films (ptss_lindenoise.hip; csrc/ptlindn.h). ----
int ptss_default_denoise_linear_params(ptss_denoise_linear_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_denoise_linear_params);
    p->levels = 5;
    p->sigmaLuminance = 3.f;   // design choices, not measurements: three standard errors, and ptss_default_denoise_params' geometry
    p->sigmaNormal = 0.1f;
    p->sigmaDepth = 4.f;
    p->reserved[0] = p->reserved[1] = p->reserved[2] = 0u;
    return PTSS_OK;
}

int ptss_denoise_linear_workspace(int width, int height, size_t* bytes) {
    if (!bytes) return fail(PTSS_EINVAL, "bytes is null");
    if (const char* what = ptldn::sidesError(width, height)) return fail(PTSS_ERANGE, what);
    size_t off[4];
    *bytes = ptldn::workspaceLayout((size_t)width * (size_t)height, off);
    return PTSS_OK;
}

int ptss_denoise_linear(ptss_context* c, const void* dev_film, int filmKind, int width, int height, const ptss_linear_moment* dev_moments,
                        const ptss_pixel_feature* dev_features, const ptss_linear_params* params, const ptss_denoise_linear_params* denoise,
                        void* dev_workspace, ptss_linear_entry* dev_out, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlin::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptldn::paramsError(denoise)) return fail(PTSS_EINVAL, what);
    RC_TRY(filmKindCheck(filmKind));
    if (const char* what = ptldn::sidesError(width, height)) return fail(PTSS_ERANGE, what);
    if (!dev_film || !dev_moments || !dev_features || !dev_workspace || !dev_out) return fail(PTSS_EINVAL, "null film, moments, features, workspace or out");
    if (((uintptr_t)dev_film | (uintptr_t)dev_moments | (uintptr_t)dev_features | (uintptr_t)dev_workspace | (uintptr_t)dev_out) & 15u)
        return fail(PTSS_EINVAL, "film, moments, features, workspace and out must be 16-byte aligned");
    if ((const void*)dev_out == dev_film) return fail(PTSS_EINVAL, "dev_out must not be dev_film");
    size_t off[4];
    const size_t bytes = ptldn::workspaceLayout((size_t)width * (size_t)height, off);
    const uintptr_t ws = (uintptr_t)dev_workspace;
    if (((uintptr_t)dev_out >= ws && (uintptr_t)dev_out - ws < bytes) || ((uintptr_t)dev_film >= ws && (uintptr_t)dev_film - ws < bytes))
        return fail(PTSS_EINVAL, "film and out must not lie inside the workspace");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchLinearDenoise(streamOf(c, hipStream), dev_film, filmKind == PTSS_FILM_SPLAT, width, height, dev_moments, dev_features, *params,
                                      *denoise, c->linDenoiseForm, dev_workspace, dev_out, c->linDenoiseLaunches));
    return PTSS_OK;
}

int ptss_denoise_linear_launches(const ptss_context* c, unsigned long long* out2) { return readLaunches(c, &ptss_context::linDenoiseLaunches, out2); }

int ptss_debug_denoise_linear_form(ptss_context* c, int form) { return setForm(c, &ptss_context::linDenoiseForm, form, 0xff7u, "form must be 0, 1, 2 or 4 .. 11"); }

// ---- carrying the two linear films across a camera move (ptss_linreproject.hip; csrc/ptlinrp.h). ----
int ptss_default_reproject_linear_params(ptss_reproject_linear_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_reproject_linear_params);
    p->cosNormal = 0.9f;   // ptss_default_reproject_params' tests; a cap of 64 samples of history (design choices, not measurements)
    p->depthTolerance = 0.02f;
    p->minCoverage = 0.25f;
    p->maxHistory = 64u;
    p->reserved = 0u;
    return PTSS_OK;
}

int ptss_reproject_linear(ptss_context* c, const ptss_film_camera* now, const ptss_pixel_feature* dev_features_now,
                          const ptss_pixel_motion* dev_motion_now, const ptss_film_camera* prev, const ptss_pixel_feature* dev_features_prev,
                          const void* dev_film_prev, int filmKind, const ptss_linear_moment* dev_moments_prev, const ptss_linear_params* film,
                          const ptss_reproject_linear_params* params, void* dev_film_out, ptss_linear_moment* dev_moments_out,
                          ptss_reproject_linear_info* dev_info, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    // in the order of the header's list: null pointers, structSize and parameter ranges, the cameras, the film's parameters, the kind,
    // moments on one side only, alignment, overlap
    if (!now || !prev || !film || !params || !dev_features_now || !dev_features_prev || !dev_film_prev || !dev_film_out)
        return fail(PTSS_EINVAL, "null camera, parameters, features, previous film or output film");
    if (const char* what = ptlrp::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlrp::cameraError(now)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlrp::cameraError(prev)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlin::paramsError(film)) return fail(PTSS_EINVAL, what);
    RC_TRY(filmKindCheck(filmKind));
    if ((dev_moments_prev == nullptr) != (dev_moments_out == nullptr))
        return fail(PTSS_EINVAL, "dev_moments_prev and dev_moments_out must be given together or not at all");
    if (((uintptr_t)dev_features_now | (uintptr_t)dev_motion_now | (uintptr_t)dev_features_prev | (uintptr_t)dev_film_prev | (uintptr_t)dev_moments_prev |
         (uintptr_t)dev_film_out | (uintptr_t)dev_moments_out) & 15u)
        return fail(PTSS_EINVAL, "features, motion, films and moments must be 16-byte aligned");
    if ((uintptr_t)dev_info & 7u) return fail(PTSS_EINVAL, "dev_info must be 8-byte aligned");
    if (const char* what = ptlrp::buffersError(now, dev_features_now, prev, dev_features_prev, dev_film_prev, dev_moments_prev, dev_film_out, dev_moments_out))
        return fail(PTSS_EINVAL, what);
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchLinearReproject(streamOf(c, hipStream), *now, dev_features_now, dev_motion_now, *prev, dev_features_prev, dev_film_prev,
                                        filmKind == PTSS_FILM_SPLAT, dev_moments_prev, *film, *params, dev_film_out, dev_moments_out, dev_info,
                                        &c->linReprojectLaunches));
    return PTSS_OK;
}

int ptss_reproject_linear_launches(const ptss_context* c, unsigned long long* out) { return readLaunches(c, &ptss_context::linReprojectLaunches, out); }

// ---- upsampling the two linear films (ptss_linupsample.hip; csrc/ptlinup.h). ----
int ptss_default_upsample_linear_params(ptss_upsample_linear_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_upsample_linear_params);
    p->factor = 2;   // ptss_default_upsample_params' values (design choices, not measurements)
    p->sigmaNormal = 0.1f;
    p->sigmaDepth = 4.0f;
    p->flags = 0u;
    p->reserved = 0u;
    return PTSS_OK;
}

int ptss_upsample_linear(ptss_context* c, const void* dev_film_lo, int filmKind, int width, int height, const ptss_pixel_feature* dev_features_lo,
                         const ptss_pixel_feature* dev_features_hi, const ptss_linear_params* film, const ptss_upsample_linear_params* params,
                         ptss_linear_entry* dev_film_hi, ptss_upsample_linear_info* dev_info, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    // in the order of the header's list: null pointers, the parameters, the kind, the film's parameters, the sides, alignment, overlap
    if (!film || !params || !dev_film_lo || !dev_features_lo || !dev_features_hi || !dev_film_hi)
        return fail(PTSS_EINVAL, "null parameters, film, features or output film");
    if (const char* what = ptlup::paramsError(params)) return fail(PTSS_EINVAL, what);
    RC_TRY(filmKindCheck(filmKind));
    if (const char* what = ptlin::paramsError(film)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlup::sidesError(width, height, params->factor)) return fail(PTSS_ERANGE, what);
    if (((uintptr_t)dev_film_lo | (uintptr_t)dev_features_lo | (uintptr_t)dev_features_hi | (uintptr_t)dev_film_hi) & 15u)
        return fail(PTSS_EINVAL, "films and features must be 16-byte aligned");
    if ((uintptr_t)dev_info & 7u) return fail(PTSS_EINVAL, "dev_info must be 8-byte aligned");
    const size_t loBytes = 32 * (size_t)width * (size_t)height, hiBytes = loBytes * (size_t)params->factor * (size_t)params->factor;
    if (ptlup::rangesOverlap(dev_film_hi, hiBytes, dev_film_lo, loBytes)) return fail(PTSS_EINVAL, "dev_film_hi overlaps dev_film_lo");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchLinearUpsample(streamOf(c, hipStream), dev_film_lo, filmKind == PTSS_FILM_SPLAT, width, height, dev_features_lo, dev_features_hi,
                                       *film, *params, c->linUpsampleForm, dev_film_hi, dev_info, &c->linUpsampleLaunches));
    return PTSS_OK;
}

int ptss_upsample_linear_launches(const ptss_context* c, unsigned long long* out) { return readLaunches(c, &ptss_context::linUpsampleLaunches, out); }

int ptss_debug_upsample_linear_form(ptss_context* c, int form) { return setForm(c, &ptss_context::linUpsampleForm, form, 0x7u, "form must be 0, 1 or 2"); }

// ---- rays from surface points and the gutter fill (ptss_surface.hip; csrc/ptsurface.h). ----
int ptss_generate_rays_surface(ptss_context* c, const ptss_surface_params* params, const ptss_surface_point* dev_points, size_t numPoints,
                               size_t firstPoint, const uint32_t* dev_index, size_t n, ptss_path_rng* dev_rng, ptss_ray_query* dev_rays,
                               ptss_ray_hit* dev_surfels, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptsurf::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (!fits31(numPoints)) return fail(PTSS_ERANGE, "numPoints must be below 2^31");
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    if (n == 0) return PTSS_OK;
    if (!dev_points || !dev_rng || !dev_rays) return fail(PTSS_EINVAL, kNullBuffer);
    if ((((uintptr_t)dev_points | (uintptr_t)dev_rays | (uintptr_t)dev_surfels) & 15u) || (((uintptr_t)dev_rng | (uintptr_t)dev_index) & 3u))
        return fail(PTSS_EINVAL, "points, rays and surfels must be 16-byte aligned, dev_rng and dev_index 4-byte aligned");
    if (!dev_index && (firstPoint > numPoints || n > numPoints - firstPoint)) return fail(PTSS_ERANGE, "firstPoint + n leaves the points");
    const SceneImage* im = sceneImageOf(c);
    if (!im) return PTSS_EINVAL;
    HIP_TRY(hipSetDevice(c->cfg.device));
    hipStream_t st = streamOf(c, hipStream);
    HIP_TRY(ptss::launchSurfaceRays(st, im->dBlob, im->layout, *params, dev_points, (uint32_t)numPoints, dev_index ? 0u : (uint32_t)firstPoint, dev_index,
                                    (uint32_t)n, dev_rng, dev_rays, dev_surfels, c->dTotal + kSurfaceRejectedWord, &c->surfaceLaunches[0]));
    c->lastSurface.note(st);
    return PTSS_OK;
}

int ptss_dilate_linear(ptss_context* c, const ptss_linear_entry* dev_film, int width, int height, ptss_linear_entry* dev_out, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (!dev_film || !dev_out) return fail(PTSS_EINVAL, "null film");
    if (dev_film == dev_out) return fail(PTSS_EINVAL, "dev_out must not be dev_film");
    if (((uintptr_t)dev_film | (uintptr_t)dev_out) & 15u) return fail(PTSS_EINVAL, "films must be 16-byte aligned");
    if (const char* what = ptsurf::dilateSidesError(width, height)) return fail(PTSS_ERANGE, what);
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchDilateLinear(streamOf(c, hipStream), dev_film, width, height, c->dilateForm, dev_out, &c->surfaceLaunches[1]));
    return PTSS_OK;
}

int ptss_surface_launches(const ptss_context* c, unsigned long long* out2) { return readLaunches(c, &ptss_context::surfaceLaunches, out2); }

int ptss_surface_rejected(ptss_context* c, unsigned long long* out) {
    if (!c || !out) return fail(PTSS_EINVAL, "null argument");
    return readBehind(c, c->lastSurface, c->dTotal + kSurfaceRejectedWord, 1, out);
}

int ptss_debug_dilate_linear_form(ptss_context* c, int form) { return setForm(c, &ptss_context::dilateForm, form, 0x7u, "form must be 0, 1 or 2"); }

// ---- reading a baked light map back (ptss_lightmap.hip; csrc/ptlightmap.h). images[0]'s materials at most ----
int ptss_default_lightmap_params(ptss_lightmap_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    *p = ptss_lightmap_params{};
    p->structSize = (unsigned int)sizeof(*p);
    p->atlasWidth = p->atlasHeight = 1;
    p->filter = PTSS_LIGHTMAP_BILINEAR;
    return PTSS_OK;
}

// The one body behind both lookups. `chain` (ptss_lookup_lightmap_chain only): the chain rows whose throughput tints the FILTERED rows
// (ptlightmap.h step 6) — one more required buffer, one more alignment term and wording, one more overlap check
static int lookupLightmap(ptss_context* c, bool chain, const ptss_lightmap_params* params, const ptss_linear_params* film,
                          const ptss_surface_block* dev_blocksTri, const ptss_surface_block* dev_blocksSph, const ptss_linear_entry* dev_map,
                          const ptss_ray_hit* dev_hits, const ptss_chain_result* dev_chain, size_t n, ptss_linear_entry* dev_out, uint32_t* dev_info,
                          void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = ptlm::paramsError(params)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlin::paramsError(film)) return fail(PTSS_EINVAL, what);
    if (const char* what = ptlm::rangeError(params)) return fail(PTSS_ERANGE, what);
    if (!fits31(n)) return fail(PTSS_ERANGE, "n must be below 2^31");
    if (n == 0) return PTSS_OK;
    if (!dev_map || !dev_hits || (chain && !dev_chain) || !dev_out || (params->numTriangleBlocks > 0 && !dev_blocksTri) ||
        (params->numSphereBlocks > 0 && !dev_blocksSph))
        return fail(PTSS_EINVAL, kNullBuffer);
    if ((((uintptr_t)dev_blocksTri | (uintptr_t)dev_blocksSph | (uintptr_t)dev_map | (uintptr_t)dev_hits | (uintptr_t)dev_chain | (uintptr_t)dev_out) & 15u) ||
        ((uintptr_t)dev_info & 3u))
        return fail(PTSS_EINVAL, chain ? "blocks, map, hits, chain and out must be 16-byte aligned, dev_info 4-byte aligned"
                                       : "blocks, map, hits and out must be 16-byte aligned, dev_info 4-byte aligned");
    if (ptlrp::rangesOverlap(dev_out, 32 * n, dev_map, 32 * (size_t)params->atlasWidth * (size_t)params->atlasHeight))
        return fail(PTSS_EINVAL, "dev_out overlaps dev_map");
    if (chain && (ptlrp::rangesOverlap(dev_out, 32 * n, dev_chain, 32 * n) || ptlrp::rangesOverlap(dev_out, 32 * n, dev_hits, 48 * n)))
        return fail(PTSS_EINVAL, "dev_out overlaps dev_chain or dev_hits");
    const SceneImage* im = sceneImageOf(c);
    if (!im) return PTSS_EINVAL;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (chain)
        HIP_TRY(ptss::launchLookupLightmapChain(streamOf(c, hipStream), im->dBlob, im->layout, *params, *film, dev_blocksTri, dev_blocksSph, dev_map,
                                                dev_hits, dev_chain, (uint32_t)n, dev_out, dev_info, &c->lightmapChainLaunches));
    else
        HIP_TRY(ptss::launchLookupLightmap(streamOf(c, hipStream), im->dBlob, im->layout, *params, *film, dev_blocksTri, dev_blocksSph, dev_map, dev_hits,
                                           (uint32_t)n, c->lightmapForm, dev_out, dev_info, &c->lightmapLaunches));
    return PTSS_OK;
}

int ptss_lookup_lightmap(ptss_context* c, const ptss_lightmap_params* params, const ptss_linear_params* film, const ptss_surface_block* dev_blocksTri,
                         const ptss_surface_block* dev_blocksSph, const ptss_linear_entry* dev_map, const ptss_ray_hit* dev_hits, size_t n,
                         ptss_linear_entry* dev_out, uint32_t* dev_info, void* hipStream) {
    return lookupLightmap(c, false, params, film, dev_blocksTri, dev_blocksSph, dev_map, dev_hits, nullptr, n, dev_out, dev_info, hipStream);
}

int ptss_lookup_lightmap_chain(ptss_context* c, const ptss_lightmap_params* params, const ptss_linear_params* film,
                               const ptss_surface_block* dev_blocksTri, const ptss_surface_block* dev_blocksSph, const ptss_linear_entry* dev_map,
                               const ptss_ray_hit* dev_hits, const ptss_chain_result* dev_chain, size_t n, ptss_linear_entry* dev_out,
                               uint32_t* dev_info, void* hipStream) {
    return lookupLightmap(c, true, params, film, dev_blocksTri, dev_blocksSph, dev_map, dev_hits, dev_chain, n, dev_out, dev_info, hipStream);
}

int ptss_lightmap_chain_launches(const ptss_context* c, unsigned long long* out) { return readLaunches(c, &ptss_context::lightmapChainLaunches, out); }

int ptss_lightmap_launches(const ptss_context* c, unsigned long long* out) { return readLaunches(c, &ptss_context::lightmapLaunches, out); }

int ptss_debug_lightmap_form(ptss_context* c, int form) { return setForm(c, &ptss_context::lightmapForm, form, 0x7u, "form must be 0, 1 or 2"); }

// ---- the resolves of the two linear films (ptss_resolve.hip). ----
// The one body behind the six, each of which has checked ctx. In this order: the film's parameters (with `glare`: glareArguments), then
// rangeCall's checks — count == 0, the buffers, the range, the scene image, nothing to write. The buffers: `missing` is the caller's
// verdict on the pointers it requires, `nullText` and `alignText` are its own wordings; the alignment asked of a pointer is the same in
// every call, and a pointer a call does not have is null. With `glare` the range has to lie in the film as well, which is looked at
// once the buffers have passed. dev_state: the metered resolves' (required there: `missing`), a glare resolve's or nullptr
static int resolveLinearFilm(ptss_context* c, const void* dev_film, bool splat, size_t firstPixel, size_t count, const ptss_linear_params* params,
                             const ptss_meter_state* dev_state, const ptss::GlareResolveArgs* glare, bool missing, const char* nullText,
                             const char* alignText, ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels, ptss_history_entry* dev_history,
                             unsigned long long* launches, void* hipStream) {
    if (glare) {
        RC_TRY(glareArguments(c, params, glare->params, splat ? PTSS_GLARE_FILM_SPLAT : PTSS_GLARE_FILM_LINEAR, glare->width, glare->height));
    } else if (const char* what = ptlin::paramsError(params)) {
        return fail(PTSS_EINVAL, what);
    }
    const void* dev_pyramid = glare ? glare->pyramid : nullptr;
    const char* bad = missing ? nullText
                      : (((uintptr_t)dev_film | (uintptr_t)dev_pyramid | (uintptr_t)dev_linear | (uintptr_t)dev_history) & 15u) ||
                              ((uintptr_t)dev_state & 7u) || ((uintptr_t)dev_pixels & 3u)
                          ? alignText
                          : nullptr;
    if (glare && count != 0 && !bad) {
        const unsigned long long filmPixels = (unsigned long long)glare->width * (unsigned long long)glare->height;   // below 2^31
        if (firstPixel > filmPixels || count > filmPixels - firstPixel) return fail(PTSS_ERANGE, "firstPixel + count leaves the film");
    }
    FilmCall f;
    RC_TRY(rangeCall(c, &f, firstPixel, count, bad, true, dev_linear || dev_pixels || dev_history, hipStream));
    if (!f.go) return PTSS_OK;
    HIP_TRY(ptss::launchLinearFilmResolve(f.st, dev_film, splat, f.firstPixel, f.n, *params, dev_state, glare, f.quantTable, dev_linear, dev_pixels,
                                          dev_history, launches));
    return PTSS_OK;
}

static const char* const kResolveAlign = "film, linear and history must be 16-byte aligned, dev_pixels 4-byte aligned";
static const char* const kResolveMeteredAlign = "film, linear and history must be 16-byte aligned, dev_state 8-byte, dev_pixels 4-byte aligned";
static const char* const kResolveGlareAlign =
    "film, pyramid, linear and history must be 16-byte aligned, dev_state 8-byte, dev_pixels 4-byte aligned";

int ptss_resolve_linear(ptss_context* c, const ptss_linear_entry* dev_film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                        ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels, ptss_history_entry* dev_history, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    return resolveLinearFilm(c, dev_film, false, firstPixel, count, params, nullptr, nullptr, !dev_film, "null film with count > 0", kResolveAlign,
                             dev_linear, dev_pixels, dev_history, &c->linearLaunches[1], hipStream);
}

int ptss_resolve_splat(ptss_context* c, const ptss_splat_entry* dev_film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                       ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels, ptss_history_entry* dev_history, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    return resolveLinearFilm(c, dev_film, true, firstPixel, count, params, nullptr, nullptr, !dev_film, "null film with count > 0", kResolveAlign,
                             dev_linear, dev_pixels, dev_history, &c->splatLaunches[2], hipStream);
}

int ptss_resolve_linear_metered(ptss_context* c, const ptss_linear_entry* dev_film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                                const ptss_meter_state* dev_state, ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels,
                                ptss_history_entry* dev_history, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    return resolveLinearFilm(c, dev_film, false, firstPixel, count, params, dev_state, nullptr, !dev_film || !dev_state,
                             "null film or state with count > 0", kResolveMeteredAlign, dev_linear, dev_pixels, dev_history,
                             &c->meterLaunches[2], hipStream);
}

int ptss_resolve_splat_metered(ptss_context* c, const ptss_splat_entry* dev_film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                               const ptss_meter_state* dev_state, ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels,
                               ptss_history_entry* dev_history, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    return resolveLinearFilm(c, dev_film, true, firstPixel, count, params, dev_state, nullptr, !dev_film || !dev_state,
                             "null film or state with count > 0", kResolveMeteredAlign, dev_linear, dev_pixels, dev_history,
                             &c->meterLaunches[2], hipStream);
}

int ptss_resolve_linear_glare(ptss_context* c, const ptss_linear_entry* dev_film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                              int width, int height, const ptss_glare_params* glare, const ptss_glare_entry* dev_pyramid,
                              const ptss_meter_state* dev_state, ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels,
                              ptss_history_entry* dev_history, void* hipStream) {
    const ptss::GlareResolveArgs g{width, height, glare, dev_pyramid};
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    return resolveLinearFilm(c, dev_film, false, firstPixel, count, params, dev_state, &g, !dev_film || !dev_pyramid,
                             "null film or pyramid with count > 0", kResolveGlareAlign, dev_linear, dev_pixels, dev_history,
                             &c->glareLaunches[2], hipStream);
}

int ptss_resolve_splat_glare(ptss_context* c, const ptss_splat_entry* dev_film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                             int width, int height, const ptss_glare_params* glare, const ptss_glare_entry* dev_pyramid,
                             const ptss_meter_state* dev_state, ptss_history_entry* dev_linear, ptss_uchar4* dev_pixels,
                             ptss_history_entry* dev_history, void* hipStream) {
    const ptss::GlareResolveArgs g{width, height, glare, dev_pyramid};
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    return resolveLinearFilm(c, dev_film, true, firstPixel, count, params, dev_state, &g, !dev_film || !dev_pyramid,
                             "null film or pyramid with count > 0", kResolveGlareAlign, dev_linear, dev_pixels, dev_history,
                             &c->glareLaunches[2], hipStream);
}

// ---- tone curves for the two linear films (ptss_tone.hip; csrc/pttone.h). ----
int ptss_default_tone_params(ptss_tone_params* p) {
    if (!p) return fail(PTSS_EINVAL, "params is null");
    p->structSize = (unsigned int)sizeof(ptss_tone_params);
    p->curve = PTSS_TONE_FILMIC;   // design choices, not measurements: a common filmic fit, the display's own transfer, the TGA's depth
    p->transfer = PTSS_TRANSFER_SRGB;
    p->bits = 8;
    p->flags = 0u;
    p->white = 4.0f;
    p->filmic[0] = 2.51f, p->filmic[1] = 0.03f, p->filmic[2] = 2.43f, p->filmic[3] = 0.59f, p->filmic[4] = 0.14f;
    p->reserved = 0u;
    return PTSS_OK;
}

size_t ptss_tone_table_floats(int bits) { return (bits == 8 || bits == 10) ? (size_t)pttone::tableFloats(bits) : 0; }

int ptss_tone_build(ptss_context* c, const ptss_tone_params* tone, float* dev_table, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    if (const char* what = pttone::paramsError(tone)) return fail(PTSS_EINVAL, what);
    if (!dev_table) return fail(PTSS_EINVAL, "dev_table is null");
    if ((uintptr_t)dev_table & 15u) return fail(PTSS_EINVAL, "dev_table must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->cfg.device));
    HIP_TRY(ptss::launchToneBuild(streamOf(c, hipStream), *tone, dev_table, &c->toneLaunches[0]));
    return PTSS_OK;
}

int ptss_resolve_toned(ptss_context* c, const void* dev_film, int filmKind, size_t firstPixel, size_t count, const ptss_linear_params* params,
                       const ptss_tone_params* tone, const float* dev_table, const ptss_meter_state* dev_state, int width, int height,
                       const ptss_glare_params* glare, const ptss_glare_entry* dev_pyramid, ptss_history_entry* dev_linear, uint32_t* dev_pixels,
                       ptss_history_entry* dev_history, void* hipStream) {
    if (!c) return fail(PTSS_EINVAL, "ctx is null");
    RC_TRY(filmKindCheck(filmKind));
    if (glare)
        RC_TRY(glareArguments(c, params, glare, filmKind, width, height));
    else if (const char* what = ptlin::paramsError(params))
        return fail(PTSS_EINVAL, what);
    if (const char* what = pttone::paramsError(tone)) return fail(PTSS_EINVAL, what);
    if (!glare && dev_pyramid) return fail(PTSS_EINVAL, "a pyramid needs its glare parameters");
    const bool missing = !dev_film || !dev_table || (glare && !dev_pyramid);
    const char* bad = missing ? "null film, table or pyramid with count > 0"
                      : (((uintptr_t)dev_film | (uintptr_t)dev_table | (uintptr_t)dev_pyramid | (uintptr_t)dev_linear | (uintptr_t)dev_history) & 15u) ||
                              ((uintptr_t)dev_state & 7u) || ((uintptr_t)dev_pixels & 3u)
                          ? "film, table, pyramid, linear and history must be 16-byte aligned, dev_state 8-byte, dev_pixels 4-byte aligned"
                          : nullptr;
    if (glare && count != 0 && !bad) {
        const unsigned long long filmPixels = (unsigned long long)width * (unsigned long long)height;   // below 2^31
        if (firstPixel > filmPixels || count > filmPixels - firstPixel) return fail(PTSS_ERANGE, "firstPixel + count leaves the film");
    }
    FilmCall f;
    RC_TRY(rangeCall(c, &f, firstPixel, count, bad, true, dev_linear || dev_pixels || dev_history, hipStream));
    if (!f.go) return PTSS_OK;
    const ptss::GlareResolveArgs g{width, height, glare, dev_pyramid};
    HIP_TRY(ptss::launchTonedResolve(f.st, dev_film, filmKind == PTSS_FILM_SPLAT, f.firstPixel, f.n, *params, *tone, dev_table, dev_state,
                                     glare ? &g : nullptr, c->toneForm, dev_linear, dev_pixels, dev_history, &c->toneLaunches[1]));
    return PTSS_OK;
}

int ptss_tone_launches(const ptss_context* c, unsigned long long* out2) { return readLaunches(c, &ptss_context::toneLaunches, out2); }

int ptss_debug_tone_form(ptss_context* c, int form) { return setForm(c, &ptss_context::toneForm, form, 0x7u, "form must be 0, 1 or 2"); }

}  // extern "C"
