/*
 * pt_host.h -- C ABI of the host layer (libpt_host.so) for FFI callers (Python ctypes, tests).
 *
 * Wraps the C++ drop-in API of pathtracer_amd.hpp:
 *   pth_scene_*    SceneLoader.cpp:124-348 + BVH::build (BVH.cpp:5-228) + CpuHittable
 *                  (Hittable.cpp:115-190) without a GPU: parse, transform, build, inspect;
 *   pth_renderer_* the reference's Pathtracer class (Pathtracer.h:12-68) bound to one GPU (or a
 *                  row tile of the image), with loadScene() semantics for scene files.
 * Errors never terminate the process here: calls return PT_ERR_* (see pt_hip.h) and
 * pth_last_error() holds the message of the calling thread.
 */
#ifndef PT_HOST_H
#define PT_HOST_H

#include "pt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pth_scene pth_scene;
typedef struct pth_renderer pth_renderer;

PT_API const char *pth_last_error(void);

/* Scene file -> objects (file order), BVH (leaf size 4), camera for a width x height image,
 * textures decoded on the host (handle = load order, failures get handle 0 and no slot). */
PT_API int pth_scene_load(const char *path, uint32_t width, uint32_t height, pth_scene **out);
PT_API void pth_scene_free(pth_scene *scene);

/* Host-side wall time of the load: JSON parse + transforms (SceneLoader.cpp:124-348) and the SAH
 * BVH build (BVH.cpp:66-228; multi-threaded over independent subtrees, identical layout). */
PT_API int pth_scene_timing(const pth_scene *scene, double *parse_ms, double *bvh_ms);
PT_API uint32_t pth_scene_object_count(const pth_scene *scene);
PT_API uint32_t pth_scene_node_count(const pth_scene *scene);
PT_API uint32_t pth_scene_bvh_depth(const pth_scene *scene);
/* objects in file order as device records, plus their world AABBs (min xyz, max xyz) */
PT_API int pth_scene_objects(const pth_scene *scene, pt_hittable *objects, float *aabbs);
/* BVH nodes and the reordered primitives referenced by the leaves */
PT_API int pth_scene_bvh(const pth_scene *scene, pt_bvh_node *nodes, pt_hittable *prims);
PT_API int pth_scene_camera(const pth_scene *scene, pt_camera *camera);
PT_API uint32_t pth_scene_skybox(const pth_scene *scene);
PT_API uint32_t pth_scene_texture_count(const pth_scene *scene);
PT_API int pth_scene_texture_info(const pth_scene *scene, uint32_t handle, uint32_t *width, uint32_t *height);
PT_API int pth_scene_texture_data(const pth_scene *scene, uint32_t handle, float *rgba);

/* Camera ctor (Camera.inl:4-23, fovy in radians) and SceneLoader's degree conversion. */
PT_API int pth_camera_make(const float *position, const float *lookat, const float *up, float fovy_radians, float aspect,
                           pt_camera *out);

/* Camera::rotate / Camera::translate (Camera.inl:30-52) on a camera record, in place: the
 * interactive controls of main.cpp:330-376 (the reference resets the accumulation after either). */
PT_API int pth_camera_rotate(pt_camera *cam, float pitch, float yaw, float roll);
PT_API int pth_camera_translate(pt_camera *cam, float x, float y, float z);
PT_API float pth_radians(float degrees);

/* Pathtracer on `device`, covering rows y = row_offset + k * row_stride. */
PT_API int pth_renderer_create(uint32_t width, uint32_t height, int device, uint32_t row_offset, uint32_t row_stride,
                               pth_renderer **out);
/* Pathtracer on `device`, covering the row bands b = band_offset + k * band_stride of band_rows
 * rows each (pt_create_banded). */
PT_API int pth_renderer_create_banded(uint32_t width, uint32_t height, int device, uint32_t band_rows,
                                      uint32_t band_offset, uint32_t band_stride, pth_renderer **out);
/* Pathtracer over several GPUs of this process (pt_group_*): the image data calls return the full
 * image, gathered on devices[0] over RCCL; pth_renderer_gather_ms = wall time of the last gather. */
PT_API int pth_renderer_create_group(uint32_t width, uint32_t height, int ndev, const int *devices, uint32_t band_rows,
                                     pth_renderer **out);
PT_API float pth_renderer_gather_ms(const pth_renderer *r);
PT_API void pth_renderer_destroy(pth_renderer *r);
/* loadScene(pathtracer, params) for a scene file; fills the camera (aspect = width / height). */
PT_API int pth_renderer_load_scene(pth_renderer *r, const char *path, pt_camera *camera);
/* loadSceneMoved / Pathtracer::setSceneMoved for a scene file whose objects moved since the renderer's last scene:
 * the temporal history survives and the next pth_renderer_temporal / _temporal_moments reprojects through the
 * objects' motion (pt_set_scene_moved, rule 7 of pt_hip.h; single device).  previous_object: one entry per object
 * of the file, the index that object had in the last scene's file order or 0xffffffff for a new one; NULL: object
 * k was object k, and PT_ERR_ARG naming both counts when they differ.  The renderer keeps the last scene's objects
 * and where its BVH put them; it builds the new BVH, turns the correspondences into the per-primitive table with
 * prev_index in the last BVH's order, and calls pt_set_scene_moved.  A texture of the file whose pixels are already
 * loaded keeps its handle (so an unchanged texture or sky ends nothing); one whose pixels changed is uploaded and
 * ends the history.  Without an earlier scene the call is pth_renderer_load_scene.  One move per temporal step: a
 * second call before the next temporal step ends the history.
 * pth_renderer_holds_motion: pt_holds_motion.  pth_renderer_motion_table: the table of the last successful move
 * (borrowed pointers, valid until the next scene call; returns the primitive count, 0 when there is none). */
PT_API int pth_renderer_load_scene_moved(pth_renderer *r, const char *path, const uint32_t *previous_object,
                                         pt_camera *camera);
PT_API int pth_renderer_holds_motion(const pth_renderer *r);
PT_API uint32_t pth_renderer_motion_table(const pth_renderer *r, const float **rows, const uint32_t **prev_index);
/* Moving objects without a rebuild (Pathtracer::moveObjects; pt_move_primitives and rule 10 of pt_hip.h).  object:
 * `count` distinct indices into the last scene's objects (the file's order); position, rotation (radians, as the
 * CpuHittable constructor takes it) and scale: count x 3 floats, the objects' new transforms.  Type and material stay
 * what the object has.  The temporal history is kept as pth_renderer_load_scene_moved keeps it, and
 * pth_renderer_motion_table answers as after it.  Refused with nothing changed: a device group or no scene
 * (PT_ERR_STATE), count 0, a null array, an index out of range or given twice, a transform whose inverse is not finite
 * (PT_ERR_ARG). */
PT_API int pth_renderer_move_objects(pth_renderer *r, uint32_t count, const uint32_t *object, const float *position,
                                     const float *rotation, const float *scale);
/* Pathtracer::rebuildScene: a fresh SAH build of the current objects, the history kept (a move onto themselves). */
PT_API int pth_renderer_rebuild_scene(pth_renderer *r);
/* The transforms the current objects were made with, count x 3 floats each (null arrays are skipped); returns the
 * number of objects. */
PT_API uint32_t pth_renderer_object_transforms(const pth_renderer *r, float *position, float *rotation, float *scale);
/* hipEvent milliseconds of the last move's kernels (pt_read_refit_timing). */
PT_API int pth_renderer_refit_timing(pth_renderer *r, float *ms);
/* The tree this renderer holds, which mirrors the device's: after pth_renderer_move_objects the refitted one.  The
 * counts are always written; null arrays are skipped. */
PT_API int pth_renderer_bvh(const pth_renderer *r, pt_bvh_node *nodes, pt_hittable *prims, uint32_t *node_count,
                            uint32_t *prim_count);
/* Rule 10 of pt_hip.h on the host, in place (ptamd::refitBoxes): boxes = prim_count x 6 floats.  PT_ERR_ARG, with
 * nothing changed, when the nodes are no tree over the primitives or a box is not finite or not ordered.  Pure CPU. */
PT_API int pth_refit_boxes(pt_bvh_node *nodes, uint32_t node_count, const float *boxes, uint32_t prim_count);
/* Rule 7's map for `count` objects from their records in two scenes; pure CPU, no HIP call.  With the world->object
 * rows [A | b] of prev[i] and cur[i] (inv_transform_rows), T_i = [inverse(A_prev) A_cur | inverse(A_prev) (b_cur -
 * b_prev)] takes a world point on the object now to where that object point was.  Computed in float64 from the
 * float32 words, in exactly these operations (tests/motion_model.py restates them), a = A_prev, c = A_cur:
 *   cofactors  C00 = a11*a22 - a12*a21   C01 = a12*a20 - a10*a22   C02 = a10*a21 - a11*a20
 *              C10 = a02*a21 - a01*a22   C11 = a00*a22 - a02*a20   C12 = a01*a20 - a00*a21
 *              C20 = a01*a12 - a02*a11   C21 = a02*a10 - a00*a12   C22 = a00*a11 - a01*a10
 *   det = (a00*C00 + a01*C01) + a02*C02;   inv[r][k] = C[k][r] / det          (one division per element)
 *   T[r][k] = (inv[r][0]*c[0][k] + inv[r][1]*c[1][k]) + inv[r][2]*c[2][k]      for k = 0..2, summed left to right
 *   d[k] = b_cur[k] - b_prev[k];   T[r][3] = (inv[r][0]*d[0] + inv[r][1]*d[1]) + inv[r][2]*d[2]
 * each T word rounded once to float32.  rows = count x 12 floats; valid[i] = 1, or 0 when a word of T_i is not
 * finite: the caller then sets prev_index = 0xffffffff for it. */
PT_API int pth_motion_table(const pt_hittable *prev, const pt_hittable *cur, uint32_t count, float *rows, uint32_t *valid);
/* `chunks` x Pathtracer::render(camera, spp, ignore_history && first) in one launch. */
PT_API int pth_renderer_render(pth_renderer *r, const pt_camera *camera, uint32_t spp, uint32_t chunks, int ignore_history);
/* Pathtracer::renderAdaptive (pt_render_adaptive, pt_hip.h; single device).  Afterwards
 * pth_renderer_hdr / pth_renderer_image divide every pixel by its own number of calls, and
 * pth_renderer_render with ignore_history = 0 returns PT_ERR_STATE until a render with
 * ignore_history != 0 starts a uniform buffer again.  pth_renderer_adaptive: 1 while the buffer holds
 * an adaptive render. */
PT_API int pth_renderer_render_adaptive(pth_renderer *r, const pt_camera *camera, const pt_adaptive_params *params,
                                        pt_adaptive_result *result);
PT_API int pth_renderer_adaptive(const pth_renderer *r);
/* Pathtracer::renderFeatures / featurePlane / denoise (pt_render_features, pt_denoise, pt_hip.h; single
 * device).  pth_renderer_feature_plane: plane 0..2, a borrowed pointer (rows x width float4) valid until
 * the next call, null on error.  pth_renderer_denoise: with auto_sigma != 0 params->sigma_color is not
 * read: the host computes it (PT_DENOISE_DEFAULT_SIGMA_FACTOR x the median luminance of the kept pixels);
 * sigma_used (optional) receives the value the filter ran with.  Afterwards pth_renderer_hdr /
 * pth_renderer_image return the denoised image, and pth_renderer_denoised is 1, until the next render or
 * scene change; the accumulation is not touched. */
PT_API int pth_renderer_features(pth_renderer *r, const pt_camera *camera);
PT_API const float *pth_renderer_feature_plane(pth_renderer *r, uint32_t plane);
PT_API int pth_renderer_denoise(pth_renderer *r, const pt_denoise_params *params, int auto_sigma, float *sigma_used);
PT_API int pth_renderer_denoised(const pth_renderer *r);
/* Pathtracer::temporal / getTemporalHDRImageData (pt_temporal, pt_hip.h; single device): one step of temporal
 * reprojection with the planes of the last pth_renderer_features; history_used (optional) receives whether a
 * previous history was used.  pth_renderer_temporal_hdr: the image, a borrowed pointer (rows x width float4,
 * w = the history length) valid until the next call, null on error.  pth_renderer_hdr / pth_renderer_image
 * are not changed by either. */
PT_API int pth_renderer_temporal(pth_renderer *r, const pt_temporal_params *params, int reset, int *history_used);
PT_API const float *pth_renderer_temporal_hdr(pth_renderer *r);
/* Pathtracer::temporalMoments / temporalVariance / denoiseVariance (pt_temporal_moments, pt_denoise_variance,
 * pt_hip.h; single device).  pth_renderer_temporal_variance: a borrowed pointer (rows x width floats) valid
 * until the next call, null on error.  After pth_renderer_denoise_variance pth_renderer_hdr /
 * pth_renderer_image return the filtered image, and pth_renderer_denoised is 1, as after pth_renderer_denoise. */
PT_API int pth_renderer_temporal_moments(pth_renderer *r, const pt_temporal_params *params,
                                         const pt_variance_params *variance, int reset, int *history_used);
PT_API const float *pth_renderer_temporal_variance(pth_renderer *r);
PT_API int pth_renderer_denoise_variance(pth_renderer *r, const pt_vdenoise_params *params);
/* Pathtracer::denoiseVariance(options, feedbackLevel) / temporalHistory (pt_denoise_variance_feedback,
 * pt_read_temporal_history, pt_hip.h; single device).  pth_renderer_temporal_history: a borrowed pointer
 * (rows x width float4) valid until the next call, null on error. */
PT_API int pth_renderer_denoise_variance_feedback(pth_renderer *r, const pt_vdenoise_params *params,
                                                  const pt_vfeedback_params *feedback);
PT_API const float *pth_renderer_temporal_history(pth_renderer *r, uint32_t plane);
/* Pathtracer::denoiseAdaptive / adaptiveVariance (pt_denoise_adaptive, pt_read_adaptive_variance, pt_hip.h; single
 * device).  After pth_renderer_denoise_adaptive the image calls return the filtered image, as after
 * pth_renderer_denoise_variance.  pth_renderer_adaptive_variance: a borrowed pointer (rows x width floats) valid
 * until the next call, null on error. */
PT_API int pth_renderer_denoise_adaptive(pth_renderer *r, const pt_adaptive_variance_params *variance,
                                         const pt_vdenoise_params *params);
PT_API const float *pth_renderer_adaptive_variance(pth_renderer *r);
/* Pathtracer::despike / despikeCount (pt_despike, pt_read_despike_count, pt_hip.h; single device).  After
 * pth_renderer_despike the image calls return the despiked image and pth_renderer_denoise filters it, until the next
 * render, features call or scene change.  params->min_neighbors 0 = the default (3, raised to rank and lowered to the
 * window's taps).  pth_renderer_despike_count: the pixels clamped, into *count. */
PT_API int pth_renderer_despike(pth_renderer *r, const pt_despike_params *params);
PT_API int pth_renderer_despike_count(pth_renderer *r, uint32_t *count);
/* Pathtracer::upsample / upsampleCounts (pt_upsample, pt_read_upsample_counts, pt_hip.h; single device): `hi`
 * reconstructs its frame from the image of `lo`.  source: PT_UPSAMPLE_*, or 0xffffffff = what lo's image calls return.
 * Afterwards hi's image calls return the upsampled image, until its next render, filter call or scene change.
 * pth_renderer_upsample_counts: the pixels that needed the wider ring and those that took the nearest low pixel. */
PT_API int pth_renderer_upsample(pth_renderer *hi, pth_renderer *lo, uint32_t source, const pt_upsample_params *params);
PT_API int pth_renderer_upsample_counts(pth_renderer *r, uint32_t *counts);
/* Pathtracer::upsample(lo, planes, options) (pt_upsample_resolve, rule 9 of pt_hip.h): the same onto the feature
 * planes of `planes`, a renderer at exactly 2, 3 or 4 times hi's width and height, each pixel of `hi` the mean over
 * its factor x factor first-hit samples.  `hi` needs neither features nor a render. */
PT_API int pth_renderer_upsample_resolve(pth_renderer *hi, pth_renderer *planes, pth_renderer *lo, uint32_t source,
                                         const pt_upsample_params *params);
PT_API float pth_renderer_timing(const pth_renderer *r);
PT_API uint32_t pth_renderer_frames(const pth_renderer *r);
PT_API uint32_t pth_renderer_local_rows(const pth_renderer *r);
/* getHDRImageData / getImageData: borrowed pointers, valid until the next call */
PT_API const float *pth_renderer_hdr(pth_renderer *r);
PT_API const uint8_t *pth_renderer_image(pth_renderer *r);
PT_API pt_context *pth_renderer_context(pth_renderer *r);   /* devices[0]'s context for a group */
PT_API pt_group *pth_renderer_group(pth_renderer *r);       /* null unless multi-device */

/* Output files (main.cpp:180-199 semantics: rows flipped vertically when flip != 0). */
PT_API int pth_write_png(const char *path, uint32_t width, uint32_t height, const uint8_t *rgba, int flip);
PT_API int pth_write_hdr(const char *path, uint32_t width, uint32_t height, const float *rgba, int flip);

#ifdef __cplusplus
}
#endif

#endif /* PT_HOST_H */
