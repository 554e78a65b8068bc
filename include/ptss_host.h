/* ptss_host.h — C entry points of libptss_host.so: the HOST-ONLY half of the boundary (no HIP).
 *
 * It exposes the C++ host mirror of the reference (class Scene, CudaTracer/Scene.h:5-27;
 * moveCamera, CudaTracer/CudaTracer.cu:822-870; saveScreenshot, :795-813) to non-C++ callers
 * (the Python test/bench harness), plus read-only probes of the deterministic math and RNG
 * that the device code is built from, so they can be pinned on a machine without a GPU.
 * Every function returns 0 on success and a negative PTSS_HOST_E* code otherwise.
 */
#ifndef PTSS_HOST_H
#define PTSS_HOST_H

#include "ptss_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PTSS_HOST_OK 0
#define PTSS_HOST_EINVAL (-1)
#define PTSS_HOST_EIO (-2)
#define PTSS_HOST_ERANGE (-3) /* a size outside what the call serves (ptss_probe_upsample_linear) */

typedef struct ptss_scene ptss_scene; /* owns a C++ Scene */

/* Scene::buildPreset — "default" is Scene::build() (Scene.cpp:17-32); the rest: SURVEY.md §9.6. */
int ptss_scene_create(const char* preset, ptss_scene** out);
void ptss_scene_destroy(ptss_scene* s);
/* Borrowed pointers into the scene's vectors (Scene.h:11-15); valid until destroy. */
int ptss_scene_describe(const ptss_scene* s, ptss_scene_desc* out);

/* Scene::addObjModel — a Wavefront OBJ file (v, vn, f in the i, i/j, i//k, i/j/k forms, negative indices relative; polygons
 * fan-triangulated; vt, o, g, s, usemtl, mtllib and comments ignored) appended to the scene's triangles with materialIdx.
 * mat4x4: 16 floats, ROW-major (row r = mat4x4[4r .. 4r + 3]), applied to positions (normals: its inverse transpose); NULL =
 * identity. *added (may be NULL) = triangles appended. PTSS_HOST_EIO: the file cannot be read; PTSS_HOST_EINVAL: a malformed
 * line, an index out of range, a non-finite number, or materialIdx outside the scene's materials. On any error the scene is
 * unchanged. Pointers from an earlier ptss_scene_describe may be invalidated: describe again. */
int ptss_scene_add_obj(ptss_scene* s, const char* path, const float* mat4x4, int materialIdx, size_t* added);

/* Camera() defaults (RenderStructs.h:51-52) and moveCamera (CudaTracer.cu:822-870):
 * key is the reference's key code ('w','a','s','d','q','e','f','h','g','t'); *moved = 1 if handled. */
int ptss_camera_default(ptss_camera* out);
int ptss_camera_move(ptss_camera* cam, unsigned char key, int* moved);
/* The eye ray through (x + jx, y + jy) of a width x height frame, built with bounce 0's operations (computeEyeRay,
 * CudaTracer.cu:321-343), tmax = +inf. With (jx, jy) = the pixel's two RNG uniforms it is the frame's own eye ray; (0.5, 0.5)
 * is the pixel centre. */
int ptss_camera_ray(const ptss_camera* cam, int width, int height, int x, int y, float jx, float jy, ptss_ray_query* out);

/* saveScreenshot (CudaTracer.cu:795-813): 18-byte header, type 2, 24-bit BGR, bottom-up rows,
 * from a host copy of the RGBA display buffer (row 0 = bottom, as GPUAnimBitmap draws it). */
int ptss_write_tga(const char* filename, const ptss_uchar4* rgba, int width, int height);

/* Pixel-tile ownership used for multi-GPU sharding (north_star): rows are dealt to
 * ranks in bands of band_rows. Returns the number of rows rank owns; fills rows[] (may be NULL). */
int ptss_tile_rows(int height, int band_rows, int rank, int world, int* rows, int cap);

/* Probes (tests only). op: 0 sin, 1 cos, 2 tan, 3 atan, 4 log, 5 exp, 6 pow(x,y), 7 sqrt */
int ptss_probe_math(int op, const float* x, const float* y, float* out, size_t n);
/* The vector layer of csrc/ptmath.h (its pinned fma chains), n cases of 12 floats in and 4 floats out each. op (operands -> results;
 * quaternions as x, y, z, w; results an operation does not have are +0; csrc/ptvecops.h is the one statement of this table, compiled
 * here and into the device side of tests/csrc/math_identity.hip): 0 dot(in[0..2], in[3..5]) -> out[0]; 1 cross(in[0..2], in[3..5]) ->
 * out[0..2]; 2 in[0..2] / in[3]; 3 madd(v = in[0..2], s = in[3], o = in[4..6]); 4 madd(a = in[0..2], b = in[3..5], o = in[6..8]);
 * 5 rotate(q = in[0..3], v = in[4..6]); 6 mul(p = in[0..3], q = in[4..7]) -> out[0..3]; 7 normalize(in[0..2]); 8 normalize(q =
 * in[0..3]) -> out[0..3]; 9 length(in[0..2]) -> out[0]. PTSS_HOST_EINVAL: a null pointer or an op outside 0..9. */
int ptss_probe_vector(int op, const float* in, float* out, size_t n);
/* The range facts behind the guard-free fast paths of the shading code (csrc/ptmath.h; tests/test_guard_ranges.py).
 * ptss_probe_guard: out[i] = 1 or 0 for x[i] under op 0 fast_numerator, 1 fast_divisor, 2 fast_rcp_operand, 3 in_light_window (the
 * one-compare integer form of kLightD2Lo <= x < kLightD2Hi). ptss_probe_guard_constants: out9 = kSqrtLo, kSqrtHi, kRcpLo, kRcpHi,
 * kDivLo, kDivHi, kLightD2Lo, kLightD2Hi, kFourPi. ptss_probe_scene_guard_flags: what ptss_create decides for a scene
 * (csrc/ptpack.h sceneGuardFlags; the bits of ptss_guard_flags). */
int ptss_probe_guard(int op, const float* x, unsigned int* out, size_t n);
int ptss_probe_guard_constants(float* out9);
int ptss_probe_scene_guard_flags(const ptss_scene_desc* scene, unsigned int* out);
/* 8-bit tone-mapped sample of a radiance value, literal (CudaTracer.cu:72-85), and the 257 thresholds T[0..256] of its
 * table form (csrc/ptquant.h): T[k] = smallest float whose sample is >= k (T[0] = -inf, T[256] = NaN). Returns PTSS_HOST_EINVAL if not monotone. */
int ptss_probe_quantize(const float* x, unsigned int* out, size_t n);
int ptss_probe_quant_table(float* out257);
/* Triangle::intersectRay (Primitives.h:25-83) for n (triangle {v0, e1, e2}, origin, direction, running distance) tuples, in the
 * general form and in the edge-class form the kernels pick for that triangle (csrc/pttri.h); primary != 0: with the
 * camera-origin precomputes of bounce 0. cls[i] = the class; per form six floats: accepted (0/1), dist, b0, b1, b2, det. */
int ptss_probe_triangle_forms(const float* tri9, const float* o3, const float* d3, const float* limit, int primary, size_t n, int* cls,
                              float* general6, float* classed6);
/* Pixel order of a tile (csrc/ptlocate.h — the very functions bounce 0 calls): for each of the n strips of 64 consecutive local
 * pixels that start at firstBegin, firstBegin + 1, ..., the frame position {x, gy, globalIndex} of every pixel of the strip as the
 * per-wave form gives it (wave3: waveOrigin + laneCoord, or locate per pixel where the strip crosses more than one row end) and as
 * locate() gives it (lane3), 64 x 3 ints per strip; fast[i] = 1 where strip i took the per-wave form. */
int ptss_probe_wave_locate(int width, int rank, int world, int bandRows, unsigned int firstBegin, size_t n, int* wave3, int* lane3, int* fast);
/* The strip words of bounce 0 (csrc/ptstrip.h — the very functions stripMaskKernel calls, compiled for the host): packs `scene` as
 * ptss_create does and fills masks[0 .. *numStrips) with the word of every 64-pixel strip of the local pixel plane of rank `rank` of
 * `world` (bands of bandRows rows of a width x height frame) under `camera`: bits 0-31 the stored spheres, bits 32-63 the stored
 * triangles the strip's eye rays can reach. *enabled = 1 where ptss_generate_frame would hand the words to bounce 0 (a plain,
 * bounded, edge-classed image of at most 32 spheres and 32 triangles, the camera in range), else 0 and every word all ones.
 * triPos (may be NULL) receives the stored position of each of the scene's triangles; spheres are stored in the caller's order.
 * capacity: words `masks` can hold; PTSS_HOST_EINVAL when that is too few. */
int ptss_probe_strip_masks(const ptss_scene_desc* scene, const ptss_camera* camera, int width, int height, int bandRows, int rank, int world,
                           unsigned long long* masks, size_t capacity, size_t* numStrips, int* enabled, int* triPos);
/* The mesh image's leaf / group bound (csrc/ptmesh.h — the very predicate the kernels evaluate): builds ONE bound around the
 * ntri triangles {v0, e1, e2} (nine floats each, as stored) and answers for each of n rays (origin, direction) whether it may be
 * accepted by a triangle inside (out[i] = 1) or provably is not (0). The predicate holds for |d|^2 within 1e-5 of 1 and a
 * finite origin; margin scales its inflation term (1 = the kernels'; smaller values exist to show that a test can catch an
 * under-inflated bound). bound12 (may be NULL) receives the bound's three rows. */
int ptss_probe_mesh_bound(const float* tri9, size_t ntri, const float* o3, const float* d3, size_t n, float margin, int* out, float* bound12);
/* The REFIT of the mesh image's bounds on the host (csrc/ptmesh.h refitBound — the very arithmetic and reduction shape of
 * meshRefitKernel, ptss_update_triangles): tri9 holds ntri triangles {v0, e1, e2} in STORED order; bounds12 receives 12 floats
 * per bound, the ceil(ntri / 16) leaves first, then the ceil(leaves / 16) groups — what ptss_read_triangle_bounds returns after a
 * refit, bit for bit. */
int ptss_probe_mesh_refit(const float* tri9, size_t ntri, float* bounds12);
/* The kd order of n triangles as ptss_resort_triangles rebuilds it (csrc/ptorder.h — the very centroid, key, axis and split code
 * the kernels run, level by level): position[i] = the stored position of original index i. Only the vertices are read; they must
 * be finite. Every 16 consecutive positions hold what the packer's kd order (csrc/ptpack.h) puts into that leaf; inside a leaf the
 * original indices ascend. PTSS_HOST_EINVAL: a null pointer, n = 0 or n > 2^20. */
int ptss_probe_kd_order(const ptss_triangle* triangles, size_t n, int* position);
/* The same rule with float codes that keep -0.0 below +0.0 — NOT the packer's order, whose comparator ties the two zeros: it exists
 * so that a test can show that the canonical zero of ptss_probe_kd_order matters (tests/test_resort_cpu.py). */
int ptss_probe_kd_order_signed_zero(const ptss_triangle* triangles, size_t n, int* position);
/* The scene image ptss_create builds for a scene (csrc/ptpack.h — the very packer libptss.so runs): image `image` (0 or 1) of the
 * *numImages (1 or 2) the scene gets with cfg.everySphereLoop = everySphereLoop (0 or 1). *inLds: 1 if the image is staged in LDS.
 * layout (may be NULL) receives the image's SceneLayout (csrc/ptscene.h) as raw bytes; layoutBytes must be its size (140).
 * *blobWords = the image's float words (four per row); blob (may be NULL: a size query) receives them if blobCapacity, in words,
 * suffices. Every out pointer may be NULL; with layout, blob, inLds and blobWords all NULL nothing is packed (the count alone).
 * PTSS_HOST_EINVAL: a null or invalid scene, a flag or an image index out of range (*numImages is set), a wrong layoutBytes, or a
 * blob too small (*blobWords is set). */
int ptss_probe_pack_scene(const ptss_scene_desc* scene, int everySphereLoop, int image, int* numImages, int* inLds, void* layout,
                          size_t layoutBytes, float* blob, size_t blobCapacity, size_t* blobWords);
/* ptmesh.h mayTouch for n rays against ONE given bound (12 floats), margin as in ptss_probe_mesh_bound. */
int ptss_probe_mesh_touch(const float* bound12, const float* o3, const float* d3, size_t n, float margin, int* out);
/* ptss_denoise on the host (csrc/ptdenoise.h — the very per-tap weights and accumulation order the kernel evaluates): accum = 3
 * uint32 per pixel, features = width * height entries, row-major. out_rgba (4 bytes per pixel) and out_float (3 floats per pixel, the
 * filtered value before the byte conversion) may each be NULL. PTSS_HOST_EINVAL: a null input, a non-positive size, a wrong
 * structSize or levels outside 0..6. */
int ptss_probe_denoise(const uint32_t* accum, float inverseTicks, const ptss_pixel_feature* features, int width, int height,
                       const ptss_denoise_params* params, unsigned char* out_rgba, float* out_float);
/* The same passes with float colours as input (ptss_denoise_history on the host): the r, g, b of width * height history entries. */
int ptss_probe_denoise_history(const ptss_history_entry* history, const ptss_pixel_feature* features, int width, int height,
                               const ptss_denoise_params* params, unsigned char* out_rgba, float* out_float);
/* ptss_upsample on the host (csrc/ptupsample.h — the very tap geometry, weights and accumulation order the kernel evaluates), with
 * the device call's argument checks: lo_rgba = 4 bytes per pixel of a width x height image, features_lo its features, features_hi
 * those of the params->factor times larger frame, all row-major. out_rgba: 4 bytes per hi-res pixel; out_float4 (may be NULL): r, g,
 * b before the byte conversion and the taps' weight sum. PTSS_HOST_EINVAL: a null required pointer, a non-positive size, a hi-res
 * frame of 2^31 pixels or more, out_rgba == lo_rgba, or parameters ptss_upsample refuses. */
int ptss_probe_upsample(const unsigned char* lo_rgba, const ptss_pixel_feature* features_lo, int width, int height,
                        const ptss_pixel_feature* features_hi, const ptss_upsample_params* params, unsigned char* out_rgba, float* out_float4);
/* The tap geometry of one axis (csrc/ptupsample.h axisOf) for hi-res coordinate X at `factor`: *x0 the lower tap (-1 .. size - 1),
 * *k the centre's distance from it in half hi-res pixels, *fx = k / (2 factor), the weight of tap x0 + 1. PTSS_HOST_EINVAL: X < 0,
 * a factor outside 1 .. 4 or a null pointer. */
int ptss_probe_upsample_axis(int X, int factor, int* x0, int* k, float* fx);
/* ptss_reproject on the host (csrc/ptreproject.h — the very arithmetic the kernel evaluates), with the device call's argument
 * checks: accum = 3 uint32 per pixel, n = samples per pixel behind it, the features of both cameras and the previous history
 * row-major, width * height entries each. history_prev = NULL: no history (camera_prev and features_prev are then ignored).
 * PTSS_HOST_EINVAL: a null required pointer, a non-positive size, n < 0, out == history_prev, or parameters ptss_reproject refuses. */
int ptss_probe_reproject(const uint32_t* accum, float inverseTicks, int n, const ptss_camera* camera_now, const ptss_camera* camera_prev,
                         int width, int height, const ptss_pixel_feature* features_now, const ptss_pixel_feature* features_prev,
                         const ptss_history_entry* history_prev, const ptss_reproject_params* params, ptss_history_entry* out);
/* ptss_reproject_motion on the host: ptss_probe_reproject with the world point of every hit pixel taken from motion_now (width *
 * height rows, required), and the same refusals. */
int ptss_probe_reproject_motion(const uint32_t* accum, float inverseTicks, int n, const ptss_camera* camera_now, const ptss_camera* camera_prev,
                                int width, int height, const ptss_pixel_feature* features_now, const ptss_pixel_motion* motion_now,
                                const ptss_pixel_feature* features_prev, const ptss_history_entry* history_prev,
                                const ptss_reproject_params* params, ptss_history_entry* out);
/* The motion row of ptss_render_features_motion on the host (csrc/ptmotion.h — the very arithmetic the kernel evaluates), for n
 * rays: direction and origin of rays[i], and kind / primitive / distance / w1 / w2 of hits[i] (what ptss_intersect returned for that
 * ray); triangles_prev: `count` records, the previous pose of triangles first .. first + count - 1 of a scene of numTriangles.
 * count = 0: nothing moved (triangles_prev may be NULL). PTSS_HOST_EINVAL: a null rays, hits or out with n > 0, a null
 * triangles_prev with count > 0, or, with count > 0, a range that leaves [0, numTriangles). */
int ptss_probe_motion(const ptss_ray_query* rays, const ptss_ray_hit* hits, size_t n, const ptss_triangle* triangles_prev, size_t first,
                      size_t count, size_t numTriangles, ptss_pixel_motion* out);
/* One step of ptss_render_features_specular's chain on the host (csrc/ptspecular.h — the very arithmetic the kernel evaluates), for
 * n rays: direction of rays[i], and kind / point / normal / materialIdx of hits[i] (what ptss_intersect returned for that ray).
 * follows[i] = 1 when the chain continues through the hit's material (a mirror, or glass that refracts or reflects totally), and
 * next[i] is then the continued ray with tmax = +inf and pad = 0; follows[i] = 0 (a miss, a terminal material, total internal reflection
 * without a specular lobe, a direction that is not finite) leaves next[i] untouched. PTSS_HOST_EINVAL: a null pointer with n > 0, or a
 * hit whose materialIdx is outside [0, numMaterials) (nothing has then been written). */
int ptss_probe_specular_step(const ptss_ray_query* rays, const ptss_ray_hit* hits, size_t n, const ptss_material* materials, size_t numMaterials,
                             ptss_ray_query* next, int* follows);
/* One link of ptss_intersect_chain on the host (csrc/ptspecular.h ptsp::step and ptsp::linkFactor):
 * ptss_probe_specular_step — the same arguments, refusals, and the very bytes of next and follows — plus factors[i], the factor by which
 * the followed link multiplies the radiance (the followed lobe's probability in the reference's scatter times its weight there):
 * specularColor * specAvg for a mirror with the pure-reflection flag, specularColor * (specAvg * F) for one without and for glass in
 * total internal reflection, refrAvg * (1 - F) in every channel for a refracted link, F the Fresnel reflectance of the incidence.
 * follows[i] = 0 leaves factors[i] untouched. A null factors with n > 0 is refused too. */
int ptss_probe_specular_link(const ptss_ray_query* rays, const ptss_ray_hit* hits, size_t n, const ptss_material* materials, size_t numMaterials,
                             ptss_ray_query* next, int* follows, ptss_vec3* factors);
/* The class csrc/ptspecular.h gives a material: 0 terminal, 1 transmit, 2 mirror; -1 for a null pointer. */
int ptss_probe_specular_class(const ptss_material* material);
/* XORWOW state after curand_init(seed, subsequence, 0): out6 = v0..v4, d. */
int ptss_probe_rng_init(unsigned long long seed, unsigned int subsequence, unsigned int* out6);
/* n raw draws and the matching (0,1] floats from a state; state advanced in place. */
int ptss_probe_rng_draw(unsigned int* state6, unsigned int* raw, float* uni, size_t n);
/* The 32 subsequence jump matrices A^(2^(67+k)) as 32*160*5 words (images of unit vectors). */
int ptss_probe_rng_jump_table(unsigned int* out, size_t words);
/* ptss_generate_rays on the host (csrc/ptcamera.h — the very operations the kernel evaluates, in their order; this build is the
 * specification): rays[i] = the eye ray of film pixel index ? index[i] : firstPixel + i from stream rng[i], advanced in place by the
 * model's draws (pinhole 2, thin lens 4, equirect 2; jitter = 0: none). An index entry >= width * height writes nothing and is counted
 * in *rejected (may be NULL; set, not added to). PTSS_HOST_EINVAL: whatever ptss_generate_rays refuses, alignment aside. */
int ptss_probe_film_rays(const ptss_film_camera* film, size_t firstPixel, const uint32_t* index /* may be NULL */, size_t n,
                         ptss_path_rng* rng /* in/out */, ptss_ray_query* rays, unsigned long long* rejected);
/* ptss_accumulate_paths on the host, with the LITERAL tone map (csrc/ptquant.h quantize_literal; CudaTracer.cu:72-85): the sums of all
 * n rays first, duplicates included, then every touched pixel resolved into pixels and history (each may be NULL) from its final sums.
 * *rejected (may be NULL; set, not added to): index entries >= filmPixels. PTSS_HOST_EINVAL: whatever ptss_accumulate_paths refuses,
 * alignment aside. */
int ptss_probe_accumulate(const ptss_path_result* results, const uint32_t* index /* may be NULL */, size_t firstPixel, size_t n,
                          ptss_film_entry* film, size_t filmPixels, ptss_uchar4* pixels, ptss_history_entry* history,
                          unsigned long long* rejected);

/* ptss_accumulate_paths_stats on the host, with the LITERAL tone map: ptss_probe_accumulate's film, pixels and history, and
 * moments[p] += qr^2 + qg^2 + qb^2 of every ray kept (csrc/ptadaptive.h squares). PTSS_HOST_EINVAL: ptss_probe_accumulate's, or a
 * null moments with n > 0. */
int ptss_probe_accumulate_stats(const ptss_path_result* results, const uint32_t* index /* may be NULL */, size_t firstPixel, size_t n,
                                ptss_film_entry* film, unsigned long long* moments, size_t filmPixels, ptss_uchar4* pixels,
                                ptss_history_entry* history, unsigned long long* rejected);
/* ptss_plan_samples on the host (csrc/ptadaptive.h — the very operations the kernels evaluate; this build is the specification):
 * cdf[0 .. filmPixels) the running sums of the weights, index[0 .. n) the plan, *info (may be NULL) what it found.
 * PTSS_HOST_EINVAL: whatever ptss_plan_samples refuses, alignment aside. */
int ptss_probe_plan_samples(const ptss_film_entry* film, const unsigned long long* moments, size_t filmPixels, const ptss_plan_params* params,
                            size_t n, unsigned long long* cdf, uint32_t* index, ptss_plan_info* info);
/* The weight csrc/ptadaptive.h gives one pixel (the plan's first step) and target i of n over a total (its third). */
uint32_t ptss_probe_plan_weight(const ptss_film_entry* entry, unsigned long long moment, const ptss_plan_params* params);
unsigned long long ptss_probe_plan_target(unsigned long long i, unsigned long long n, unsigned long long total);

/* ptss_accumulate_paths_linear on the host (csrc/ptlinear.h — the very operations the kernels evaluate; this build is the
 * specification): every ray's fixed-point sample added to film[p], duplicates included. *rejected (may be NULL; set, not added to):
 * index entries >= filmPixels. PTSS_HOST_EINVAL: whatever ptss_accumulate_paths_linear refuses, alignment aside. */
int ptss_probe_accumulate_linear(const ptss_path_result* results, const uint32_t* index /* may be NULL */, size_t firstPixel, size_t n,
                                 ptss_linear_entry* film, size_t filmPixels, const ptss_linear_params* params, unsigned long long* rejected);
/* ptss_accumulate_paths_linear_stats on the host (csrc/ptlinstats.h — the very operations the kernels evaluate; this build is the
 * specification): the same arguments over host memory, film may be NULL. PTSS_HOST_EINVAL: whatever the device call refuses, alignment
 * aside. */
int ptss_probe_accumulate_linear_stats(const ptss_path_result* results, const uint32_t* index /* may be NULL */, size_t firstPixel, size_t n,
                                       ptss_linear_entry* film /* may be NULL */, ptss_linear_moment* moments, size_t filmPixels,
                                       const ptss_linear_params* params, unsigned long long* rejected);
/* ptss_plan_samples_linear on the host: cdf needs filmPixels entries here. ptss_probe_linear_plan_weight: the weight of one moment row,
 * 0xffffffff for refused parameters. */
int ptss_probe_plan_samples_linear(const ptss_linear_moment* moments, size_t filmPixels, const ptss_linear_params* params,
                                   const ptss_linear_plan_params* plan, size_t n, unsigned long long* cdf, uint32_t* index,
                                   ptss_plan_info* info /* may be NULL */);
uint32_t ptss_probe_linear_plan_weight(const ptss_linear_moment* moment, const ptss_linear_params* params, const ptss_linear_plan_params* plan);
/* ptss_resolve_linear on the host, with the LITERAL tone map (like ptss_probe_accumulate it needs no thresholds): pixels firstPixel ..
 * firstPixel + count of film into linear, pixels and history (each may be NULL). PTSS_HOST_EINVAL: whatever ptss_resolve_linear
 * refuses, alignment aside. */
int ptss_probe_resolve_linear(const ptss_linear_entry* film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                              ptss_history_entry* linear, ptss_uchar4* pixels, ptss_history_entry* history);

/* ptss_generate_rays_positions on the host: ptss_probe_film_rays' arguments, rays and streams, and positions[i] = where the sample
 * lies on the film (csrc/ptcamera.h samplePosition: the x + jx, y + jy the ray is made from); {NaN, NaN} for an index entry that leaves
 * the film. PTSS_HOST_EINVAL: ptss_probe_film_rays', or null positions. */
int ptss_probe_film_positions(const ptss_film_camera* film, size_t firstPixel, const uint32_t* index /* may be NULL */, size_t n,
                              ptss_path_rng* rng /* in/out */, ptss_ray_query* rays, ptss_film_position* positions,
                              unsigned long long* rejected);
/* ptss_splat_paths on the host (csrc/ptsplat.h — the very operations the kernels evaluate; this build is the specification): a
 * straight loop over samples and their taps. firstPixel == NULL: the scatter form's drop rule (a coordinate that is not finite or outside
 * [-R, extent + R]); else sample i is homed at pixel *firstPixel + i and a sample outside its home's closed square is dropped
 * (ptss_splat_paths_homed). *dropped and *clamped (each may be NULL; set, not added to): samples dropped, and samples kept with a channel
 * that was NaN or above clampMax. PTSS_HOST_EINVAL: whatever the two calls refuse, alignment aside. */
int ptss_probe_splat_paths(const ptss_path_result* results, const ptss_film_position* positions, const size_t* firstPixel /* may be NULL */,
                           size_t n, ptss_splat_entry* film, int width, int height, const ptss_splat_filter* filter,
                           const ptss_linear_params* params, unsigned long long* dropped, unsigned long long* clamped);
/* ptss_resolve_splat on the host, with the LITERAL tone map: ptss_probe_resolve_linear's outputs from a filtered film. */
int ptss_probe_resolve_splat(const ptss_splat_entry* film, size_t firstPixel, size_t count, const ptss_linear_params* params,
                             ptss_history_entry* linear, ptss_uchar4* pixels, ptss_history_entry* history);

/* The meter on the host (csrc/ptmeter.h — the very operations the kernels evaluate; this build is the specification).
 * ptss_probe_meter_bin: the bin of one film entry given as its four 64-bit words (splat = 0: a ptss_linear_entry, the low half of word 3
 * its samples; else a ptss_splat_entry); *bin = -1 for a pixel that is not metered; *luminance (may be NULL): Y, 0 where not metered. */
int ptss_probe_meter_bin(const unsigned long long* entry4, int splat, int* bin, unsigned long long* luminance);
/* ptss_meter_linear / ptss_meter_splat on the host: a straight loop over pixels firstPixel .. firstPixel + count, added to histogram.
 * PTSS_HOST_EINVAL: whatever the calls refuse, alignment aside. */
int ptss_probe_meter_linear(const ptss_linear_entry* film, size_t firstPixel, size_t count, uint32_t* histogram);
int ptss_probe_meter_splat(const ptss_splat_entry* film, size_t firstPixel, size_t count, uint32_t* histogram);
/* ptss_meter_exposure on the host: one update of *state. PTSS_HOST_EINVAL: whatever ptss_meter_exposure refuses, alignment aside. */
int ptss_probe_meter_exposure(const uint32_t* histogram, const ptss_linear_params* params, const ptss_meter_params* meter,
                              ptss_meter_state* state /* in/out */);

/* Glare on the host (csrc/ptglare.h — the very operations the kernels evaluate; this build is the specification).
 * ptss_glare_layout: ptss.h's, with PTSS_HOST_EINVAL for every refusal.
 * ptss_probe_glare_build: ptss_glare_build as straight loops: the downs level by level, then the ups in place from the coarsest level.
 * film: width * height entries of 32 B, a ptss_splat_entry where filmKind is PTSS_GLARE_FILM_SPLAT; pyramid: the entries
 * ptss_glare_layout counts, all of them written. PTSS_HOST_EINVAL: whatever ptss_glare_build refuses, alignment aside. */
int ptss_glare_layout(int width, int height, int levels, ptss_glare_level out[8], size_t* entries);
int ptss_probe_glare_build(const void* film, int filmKind, int width, int height, const ptss_linear_params* params,
                           const ptss_glare_params* glare, ptss_glare_entry* pyramid);
/* ptss_resolve_linear_glare / ptss_resolve_splat_glare on the host, with the literal tone map: pixels firstPixel .. firstPixel + count.
 * state may be NULL (the exposure is params->exposure), linear / pixels / history each may be NULL. */
int ptss_probe_resolve_glare(const void* film, int filmKind, size_t firstPixel, size_t count, const ptss_linear_params* params, int width,
                             int height, const ptss_glare_params* glare, const ptss_glare_entry* pyramid, const ptss_meter_state* state,
                             ptss_history_entry* linear, ptss_uchar4* pixels, ptss_history_entry* history);

/* Tone curves on the host (csrc/pttone.h — the very operations the kernels evaluate; this build is the specification).
 * ptss_probe_tone_build: ptss_tone_build on the host. table: ptss_tone_table_floats(params->bits) = 2^bits + 4 floats, all written: T[0] =
 * -inf, the thresholds T[1 .. K] (K = 2^bits - 1), T[K + 1] = NaN, T[K + 2] = 0 (1 where the thresholds are not in order: the call then
 * returns PTSS_HOST_ERANGE), T[K + 3] = T[K + 4] = NaN.
 * ptss_probe_tone_value: the literal display value transfer(curve(x)) of the parameters' own curve, whatever their flags.
 * ptss_probe_tone_level: the level of x by the table: the number of k in 1 .. K with x >= table[k].
 * ptss_probe_resolve_toned: ptss_resolve_toned on the host, over either film kind: pixels firstPixel .. firstPixel + count, one 32-bit word
 * per pixel in `pixels`. state may be NULL; glare and pyramid are both NULL or both given, width and height are read only then; linear /
 * pixels / history each may be NULL. PTSS_HOST_EINVAL: whatever the device calls refuse, alignment aside. */
int ptss_probe_tone_build(const ptss_tone_params* params, float* table);
int ptss_probe_tone_value(const ptss_tone_params* params, const float* x, float* v, size_t n);
int ptss_probe_tone_level(const float* table, int bits, const float* x, uint32_t* level, size_t n);
int ptss_probe_resolve_toned(const void* film, int filmKind, size_t firstPixel, size_t count, const ptss_linear_params* params,
                             const ptss_tone_params* tone, const float* table, const ptss_meter_state* state, int width, int height,
                             const ptss_glare_params* glare, const ptss_glare_entry* pyramid, ptss_history_entry* linear, uint32_t* pixels,
                             ptss_history_entry* history);

/* The denoiser of the two linear films on the host (csrc/ptlindn.h — the very operations the kernels evaluate; this build is the
 * specification). ptss_probe_denoise_linear: ptss_denoise_linear as straight loops over host memory, without a workspace. out: width *
 * height entries, all written. out_plane (may be NULL): width * height rows {c.r, c.g, c.b, v} of the last plane the call computed —
 * what the last pass made before its finish, or with levels = 0 what prepare made; an empty pixel's row is {0, 0, 0, -1}. On the
 * device, the plane in front of the last pass is therefore this call's out_plane with one level less. PTSS_HOST_EINVAL: whatever
 * ptss_denoise_linear refuses, alignment aside (out == film included).
 * ptss_probe_denoise_linear_finish: the finish of one pixel by itself — the output row (four 64-bit words of a ptss_linear_entry) of
 * a pixel whose filtered colour is rgb[0..2] and whose film entry has word3 as its fourth word. */
int ptss_probe_denoise_linear(const void* film, int filmKind, int width, int height, const ptss_linear_moment* moments,
                              const ptss_pixel_feature* features, const ptss_linear_params* params, const ptss_denoise_linear_params* denoise,
                              ptss_linear_entry* out, float* out_plane /* may be NULL */);
int ptss_probe_denoise_linear_finish(const float* rgb, unsigned long long word3, int filmKind, const ptss_linear_params* params,
                                     unsigned long long* out4);

/* Carrying the two linear films across a camera move on the host (csrc/ptlinrp.h — the very operations the kernel evaluates; this
 * build is the specification). ptss_probe_reproject_linear: ptss_reproject_linear as a straight loop over host memory; info (may be
 * NULL) is added to, as on the device. PTSS_HOST_EINVAL: whatever ptss_reproject_linear refuses, alignment aside.
 * ptss_probe_reproject_linear_finish: steps 4's rounding to 6 for one pixel by themselves — the reprojected mean h[0..2], the
 * interpolated count w and (hasVariance != 0) the interpolated per-sample variance s2 -> the film row and the moment row, four 64-bit
 * words each; a K of 0 gives two all-zero rows. Returns PTSS_HOST_EINVAL for a null pointer, refused params, or an s2 that is
 * negative, NaN or above 2^80 (the lookup clamps it). */
int ptss_probe_reproject_linear(const ptss_film_camera* now, const ptss_pixel_feature* features_now, const ptss_pixel_motion* motion_now,
                                const ptss_film_camera* prev, const ptss_pixel_feature* features_prev, const void* film_prev, int filmKind,
                                const ptss_linear_moment* moments_prev, const ptss_linear_params* film,
                                const ptss_reproject_linear_params* params, void* film_out, ptss_linear_moment* moments_out,
                                ptss_reproject_linear_info* info);
int ptss_probe_reproject_linear_finish(const float* h, float w, int hasVariance, float s2, int filmKind, const ptss_linear_params* film,
                                       const ptss_reproject_linear_params* params, unsigned long long* film4, unsigned long long* moment4);

/* Upsampling the two linear films on the host (csrc/ptlinup.h — the very operations the kernels evaluate; this build is the
 * specification): ptss_upsample_linear as a straight loop over host memory; info (may be NULL) is added to, as on the device.
 * PTSS_HOST_EINVAL / PTSS_HOST_ERANGE: whatever ptss_upsample_linear refuses with PTSS_EINVAL / PTSS_ERANGE, alignment aside. */
int ptss_probe_upsample_linear(const void* film_lo, int filmKind, int width, int height, const ptss_pixel_feature* features_lo,
                               const ptss_pixel_feature* features_hi, const ptss_linear_params* film, const ptss_upsample_linear_params* params,
                               ptss_linear_entry* film_hi, ptss_upsample_linear_info* info);

/* Rays from surface points and the gutter fill on the host (csrc/ptsurface.h — the very operations the kernels evaluate; this build is
 * the specification). ptss_probe_surface_rays: ptss_generate_rays_surface over the caller's own records — e1 = v1 - v0
 * and e2 = v2 - v0 and radius * radius formed as the packer forms them — with the same remaining arguments and outputs; *rejected (may
 * be NULL) is SET to the entries dropped. ptss_probe_dilate_linear: ptss_dilate_linear as a straight loop. PTSS_HOST_EINVAL /
 * PTSS_HOST_ERANGE: whatever the device calls refuse with PTSS_EINVAL / PTSS_ERANGE, alignment aside.
 *
 * ptss_surface_atlas (host only; a convenience, not a kernel): the texels of a light map over triangles[first .. first + count).
 * Triangle t gets a square block of side s = clamp(ceil(longestEdge * texelsPerUnit), minSide, maxSide) (a longest edge that is not a
 * number gives minSide); the blocks are shelf-packed left to right in the caller's order into atlasWidth columns with one empty texel
 * between blocks and between shelves; the texels (i, j) of a block with i + j <= s - 1 each get one surface point strictly inside
 * the triangle, a = (3 i + 1) / (3 s), b = (3 j + 1) / (3 s) — the centroid of the texel's lower-left half, so a + b <= 1 - 1 / (3 s).
 * points[k] / texels[k] (each may be NULL: count only; capacity entries at most are written): the point and the number
 * y * atlasWidth + x of its texel, in the caller's triangle order, rows of a block bottom up. *atlasHeight (may be NULL): the rows
 * used; *numPoints: the points there are, whatever the capacity. PTSS_HOST_EINVAL: null triangles with count > 0, a null numPoints,
 * texelsPerUnit not a positive finite number, minSide < 1, maxSide < minSide, maxSide > 4096 or maxSide > atlasWidth; PTSS_HOST_ERANGE:
 * first + count at or above 2^30 (the surface encoding), an atlas of 2^31 texels or more. */
int ptss_probe_surface_rays(const ptss_triangle* triangles, size_t numTriangles, const ptss_sphere* spheres, size_t numSpheres,
                            const ptss_surface_params* params, const ptss_surface_point* points, size_t numPoints, size_t firstPoint,
                            const uint32_t* index /* may be NULL */, size_t n, ptss_path_rng* rng, ptss_ray_query* rays,
                            ptss_ray_hit* surfels /* may be NULL */, unsigned long long* rejected);
int ptss_probe_dilate_linear(const ptss_linear_entry* film, int width, int height, ptss_linear_entry* out);
int ptss_surface_atlas(const ptss_triangle* triangles, size_t first, size_t count, float texelsPerUnit, int minSide, int maxSide, int atlasWidth,
                       ptss_surface_point* points, uint32_t* texels, size_t capacity, int* atlasHeight, size_t* numPoints);

/* Light maps read back (csrc/ptlightmap.h, csrc/ptsurface.h).
 *
 * ptss_surface_atlas_blocks (host only; a convenience like ptss_surface_atlas): the same atlas, with the blocks named and continued
 * over spheres[firstSphere .. firstSphere + numSpheres) (may be NULL with 0). The triangles come first and are packed by
 * ptss_surface_atlas' rule — with numSpheres = 0 the points, texels, height and count are that function's —; the spheres continue on
 * the same shelves with the same one-texel gaps: sphere k gets h = clamp(ceil(pi * radius * texelsPerUnit), minSide, maxSide) rows
 * (not a number: minSide) and w = 2 h columns, and every texel (i, j) of its block the point {surface = k, a = (i + 0.5) / w,
 * b = (j + 0.5) / h, flags = 0} — ptss_surface_point's longitude and latitude fractions — rows bottom up, after all triangle points.
 * blocksTri[count], blocksSph[numSpheres] (each may be NULL): where each primitive's block lies; the texel of a block's (i, j) is
 * (y + j) * atlasWidth + x + i. Refused as ptss_surface_atlas refuses, and PTSS_HOST_EINVAL null spheres with numSpheres > 0 or
 * 2 * maxSide > atlasWidth when numSpheres > 0, PTSS_HOST_ERANGE firstSphere + numSpheres at or above 2^30.
 *
 * ptss_probe_lookup_lightmap: ptss_lookup_lightmap over the caller's own records — materials[numMaterials] stand for the scene image's
 * (may be NULL with 0) — with the same remaining arguments and outputs; info (may be NULL): four counts ADDED to. The specification of
 * the device's rows. PTSS_HOST_EINVAL / PTSS_HOST_ERANGE: whatever the device call refuses with PTSS_EINVAL / PTSS_ERANGE, alignment
 * aside. */
int ptss_surface_atlas_blocks(const ptss_triangle* triangles, size_t firstTriangle, size_t numTriangles, const ptss_sphere* spheres,
                              size_t firstSphere, size_t numSpheres, float texelsPerUnit, int minSide, int maxSide, int atlasWidth,
                              ptss_surface_block* blocksTri, ptss_surface_block* blocksSph, ptss_surface_point* points, uint32_t* texels,
                              size_t capacity, int* atlasHeight, size_t* numPoints);
int ptss_probe_lookup_lightmap(const ptss_material* materials, size_t numMaterials, const ptss_lightmap_params* params,
                               const ptss_linear_params* film, const ptss_surface_block* blocksTri, const ptss_surface_block* blocksSph,
                               const ptss_linear_entry* map, const ptss_ray_hit* hits, size_t n, ptss_linear_entry* out, uint32_t* info);
/* ptss_lookup_lightmap_chain over the caller's own records (csrc/ptlightmap.h step 6): ptss_probe_lookup_lightmap with
 * chain[n], whose throughput tints every FILTERED row — clamped into [0, 1], not a number: 0. The specification of the device's rows.
 * Also PTSS_HOST_EINVAL: a null chain with n > 0, out overlapping chain or hits. */
int ptss_probe_lookup_lightmap_chain(const ptss_material* materials, size_t numMaterials, const ptss_lightmap_params* params,
                                     const ptss_linear_params* film, const ptss_surface_block* blocksTri, const ptss_surface_block* blocksSph,
                                     const ptss_linear_entry* map, const ptss_ray_hit* hits, const ptss_chain_result* chain, size_t n,
                                     ptss_linear_entry* out, uint32_t* info);

#ifdef __cplusplus
}
#endif
#endif
