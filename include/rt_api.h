/*
 * rt_api.h — C ABI of the MI355X renderer (librtamd.so).
 *
 * This is the drop-in for the reference's GPU operator boundary: the GL compute
 * program, its SSBO bindings, its uniforms and glDispatchCompute. Each entry
 * point names the reference call it replaces. Plain pointers and sizes only;
 * every function returns an int status (RT_OK = 0, negative on error) and never
 * throws across the boundary (the reference prints shader errors and carries
 * on, src/computeShader.hpp:64-79; here the caller gets a code).
 *
 * Threading: one rt_ctx per device. A context is not thread-safe; different
 * contexts may be driven from different threads. All work of a context is
 * ordered on one HIP stream (its own, or the caller's via rt_set_stream).
 */
#ifndef RT_API_H
#define RT_API_H

#include <stddef.h>
#include <stdint.h>
#include "rt_flat.h"

#ifdef __cplusplus
extern "C" {
#endif

struct rt_ctx; /* opaque: one per device */

enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID = -1,   /* bad argument (null pointer, negative size, bad rows)   */
    RT_ERR_DEVICE = -2,    /* a HIP runtime call failed                              */
    RT_ERR_NO_MEMORY = -3, /* device allocation failed                               */
    RT_ERR_NO_SCENE = -4,  /* dispatch before rt_upload_scene / camera / light       */
    RT_ERR_BVH = -5,       /* node/index arrays are out of range or too deep         */
    RT_ERR_NO_DEVICE = -6, /* no HIP device with that ordinal                        */
    RT_ERR_COMM = -7,      /* an RCCL call failed (rt_group.h)                       */
    RT_ERR_TIMEOUT = -8    /* a group's frames did not finish in time (rt_group.h)   */
};

/* Uniforms of gpu_shader.comp:126-130, set by src/main.cpp:357-361.
 * Applied AT the next dispatch (the reference sets them after the dispatch, so
 * its frame k uses frame k-1's values and frame 0 uses zeros). */
typedef struct rt_params {
    float resX, resY;        /* screenRes; pixel NDC and background use these        */
    int maxBounces;          /* closest-hit bounces per pixel, >= 0                  */
    int useBVH;              /* 1: BVH traversal branch, 0: brute-force branch       */
    int useFresnel;          /* Fresnel-weighted reflections                         */
    int useMollerTrumbore;   /* triangle test: 1 Moller-Trumbore, 0 barycentric      */
} rt_params;

/* Traversal kernel variants (all produce the same image). */
enum rt_kernel {
    RT_KERNEL_AUTO = 0,      /* pick the fastest for the uploaded scene               */
    RT_KERNEL_LANE = 1,      /* one ray per lane, per-lane LDS stack (reference walk) */
    RT_KERNEL_PACKET = 2,    /* wave64 packet walk, wave-uniform stack + active mask  */
    RT_KERNEL_ACCEL = 3,     /* packet walk + exact-result leaf accelerator (default  */
                             /* for BVH + barycentric; falls back to PACKET otherwise)*/
    RT_KERNEL_LIGHTS = 4,    /* reported only (rt_accel_info::last_kernel): the frame */
                             /* of two or more lights over the accelerator            */
                             /* (rt_set_lights); rt_set_kernel does not take it       */
    RT_KERNEL_SOFT = 5       /* reported only: the frame of area lights over the      */
                             /* accelerator (rt_set_soft_shadows); rt_set_kernel does */
                             /* not take it                                           */
};

/* Accelerator statistics of the uploaded scene (rt_accel_info). */
typedef struct rt_accel_info {
    int built;               /* 1 if the accelerator is in use for this scene         */
    int local_nodes;         /* local BVH nodes inside large reference leaves         */
    int local_leaves;
    int bounded_prims;       /* shapes under a conservative box                       */
    int always_prims;        /* shapes tested whenever their leaf is entered          */
    int max_stack;           /* worst-case wave stack entries                          */
    int last_kernel;         /* rt_kernel of the latest render dispatch               */
    int scene_tree;          /* 1 if the scene tree is built (rt_set_tree)             */
    int scene_nodes;         /* its wide nodes                                         */
    int scene_items;         /* its leaves (shapes of one reference leaf each)         */
    int scene_height;        /* its binary height                                      */
    int tree_nested;         /* the reference tree's child boxes lie in their parents' */
    int record_bytes;        /* device records the accelerated kernel reads: nodes,   */
                             /* items, shapes, materials (its compulsory scene bytes)  */
} rt_accel_info;

/* Work counted on the reference's own traversal (gpu_shader.comp:380-430 and
 * :523-580) — what the reference shader would load. Filled by
 * rt_collect_stats; used for Mrays/s and the algorithmic-bytes roofline. */
typedef struct rt_stats {
    uint64_t pixels;              /* pixels shaded                                  */
    uint64_t closest_rays;        /* closest-hit traversals (primary + reflection)  */
    uint64_t shadow_rays;         /* shadow traversals                              */
    uint64_t node_visits;         /* FlatNode records popped and box-tested         */
    uint64_t bvh_tests[4];        /* leaf primitive tests by type (BVH branch)      */
    uint64_t brute_tests[4];      /* primitive tests by type (brute-force branch)   */
    uint64_t closest_updates;     /* closest-hit record updates (material fetches)  */
    uint64_t hits;                /* bounces that hit a shape                       */
} rt_stats;

/* ComputeShader("gpu_shader.comp") + the RGBA32F image (src/computeShader.hpp:30-83,
 * src/main.cpp:182-195). Selects HIP device `device`. */
int rt_create(struct rt_ctx** out, int device);
int rt_destroy(struct rt_ctx* ctx);

/* Order all work of the context on a caller stream (hipStream_t; NULL = own stream). */
int rt_set_stream(struct rt_ctx* ctx, void* hip_stream);

/* SSBO 3 (shapes), 4 (nodes), 5 (bvhIndices) (src/main.cpp:256-275). The root
 * is node N-1 as in gpu_shader.comp:386. Copies to HBM and re-lays the records
 * out for the kernels; the caller keeps ownership. N == 0 is allowed (the BVH
 * branch then sees no shape). Returns RT_ERR_BVH for child/index out of range. */
int rt_upload_scene(struct rt_ctx* ctx, const FlatShape* shapes, int num_shapes,
                    const FlatNode* nodes, int num_nodes, const int* indices, int num_indices);

/* Partial re-upload of shapes [first, first+count) (glBufferSubData in updateScene,
 * src/main.cpp:981-992). Node boxes are not touched (the reference's are not either,
 * until it re-uploads them). The host array may be reused when the call returns. */
int rt_update_shapes(struct rt_ctx* ctx, int first, int count, const FlatShape* shapes);

/* Re-upload of all nodes with the same topology (src/main.cpp:340-345, after
 * updateBVH + serializeBVH); RT_ERR_BVH if the topology differs.
 *
 * Both calls only write the context's host copies and return; the next operation
 * that reads the device scene (a dispatch, rt_collect_stats, rt_read_nodes,
 * rt_build_lbvh, rt_animate) applies everything written since as ONE device refit
 * on the context's stream: the moved shapes' records, the boxes of the accelerator
 * above them, and every copy of the node boxes. So the reference's loop -- one
 * rt_update_shapes per animated record, then one rt_update_nodes -- costs one small
 * kernel per frame, not one rebuild per call. The accelerator is rebuilt on the host
 * only when a moved shape's kind of bound changed (the frame is exact before that
 * too: the refit enters every box above it) or the new node boxes no longer nest
 * (the scene tree's condition, rt_set_tree). rt_debug_refits / rt_debug_anim_rebuilds
 * count the two outcomes. */
int rt_update_nodes(struct rt_ctx* ctx, const FlatNode* nodes, int num_nodes);

/* Device-side animation. Replaces the reference's
 * per-frame CPU path: updateScene + updateBVH + serializeBVH + the two
 * glBufferSubData calls (src/main.cpp:336-346, 981-992, 1068-1077).
 *
 * rt_set_animated marks the shapes the host animates: the reference's
 * animatedIndices / Shape::animated (src/main.cpp:120, 600-616, 706-708).
 * ids must be distinct and in [0, num_shapes); count 0 clears the set.
 * The set holds until the next rt_upload_scene.
 *
 * rt_animate uploads their new records: shapes[i] is shape ids[i]. On the
 * device it then grows every node whose shape set lists an animated shape to
 * include the shape, exactly as updateBVH does. That means the leaf and every
 * node above it, growToInclude (src/BoundingBox.hpp:44-95), grow-only.
 * The accelerator's conservative boxes are refit along with the node boxes, in
 * one kernel launch per call (with any rt_update_shapes / rt_update_nodes pending).
 * A moved shape whose kind of bound changes (a triangle that becomes too thin to
 * bound, a sphere whose radius becomes infinite) is entered through every box
 * above it until the host rebuilds the accelerator, which the refit requests.
 * The frame is identical either way. The host array may be reused when the call
 * returns. RT_ERR_INVALID if no set is marked.
 *
 * rt_read_nodes copies the current node records to the host, including the
 * boxes rt_animate grew. num_nodes must match the scene's node count. */
int rt_set_animated(struct rt_ctx* ctx, const int* ids, int count);
int rt_animate(struct rt_ctx* ctx, const FlatShape* shapes);
int rt_read_nodes(struct rt_ctx* ctx, FlatNode* nodes, int num_nodes);

/* SSBO 2 and 1 (src/main.cpp:328-334). */
int rt_set_camera(struct rt_ctx* ctx, const FlatCamera* camera);
int rt_set_light(struct rt_ctx* ctx, const FlatLight* light);

/* More than one point light (an extension: the reference shader has one).
 *
 * rt_set_lights copies `count` records (1..RT_MAX_LIGHTS) and applies them at the next
 * dispatch, as rt_set_light does; it replaces the whole set. rt_set_light(l) is
 * rt_set_lights(l, 1), so a host that sets its light every frame (rth_render_loop*) keeps
 * rendering one light. rt_get_lights copies min(cap, count) records to `lights` and the set's
 * size to `*count`; either pointer may be NULL (cap is not read when `lights` is NULL); a
 * context that never had a light reports 0. RT_ERR_INVALID for a NULL context, for NULL
 * `lights` or a count outside 1..RT_MAX_LIGHTS in rt_set_lights, and for a negative cap; the
 * previous set stays in force.
 *
 * Definition. A pixel is the reference shader's main() except the light term `pc` of a bounce
 * that hit something. Every operation is float32 and none is contracted. With the hit point
 * hp, the normal hn, the material m, the incoming direction ray.d and the shadow offset off of
 * the branch (1e-3 with useBVH, 1e-5 for the brute-force branch), for light i = 0 .. L-1, in
 * order:
 *   - the shadow ray has origin hp + hn * off (the same for every light) and direction
 *     normalize(pos_i - hp); it is blocked by an INNER hit nearer than
 *     min(dist(pos_i, hp), 1e20f): the reference's shadow ray, with light i;
 *   - term_i = phong(hp, hn, ray.d, pos_i, color_i, m), times 0.3f if blocked: the
 *     reference's pc, with light i.
 * Then pc = term_0, and pc = pc + term_i per component for i = 1 .. L-1, left to right. The
 * rest of the bounce uses that pc exactly as the shader does: acc += att * pc, the mirror
 * ray, Fresnel's second acc term, att. Phong's ambient term is per light (ambient * color_i /
 * dist(pos_i, hp), gpu_shader.comp:331-361), so each light brings its own ambient. L = 1 is
 * the reference's pixel, bit for bit, and runs exactly the kernels it ran before this call
 * existed.
 *
 * The set applies to every frame dispatch (rt_dispatch, rt_dispatch_rows, _fmt, _ex) in every
 * pixel and surface format, to frames under rt_set_samples and rt_set_adaptive, and to
 * rt_shade_rays / rt_shade_rays_host. It does not enter rt_trace_*, rt_dispatch_gbuffer,
 * rt_dispatch_ao or rt_camera_rays. rt_collect_stats* keeps counting the reference's
 * one-light frame, with light 0. An rt_group's frames keep their one light
 * (rt_group_set_light sets one).
 *
 * Frames and ray lists of two or more lights run in kernels of their own: over the
 * accelerator (rt_accel_info::last_kernel reports RT_KERNEL_LIGHTS for a frame) camera rays
 * and their L shadow rays walk as wave64 packets, later bounces per lane; RT_KERNEL_LANE /
 * RT_KERNEL_PACKET, contexts without a usable accelerator and far cameras take the literal
 * per-pixel loop (last_kernel reports RT_KERNEL_LANE). Both write the same bytes. For
 * rt_set_samples such a frame is one the accelerated kernel does not render: the sample
 * frame goes to the context's scratch surface and a filter pass writes the output (the
 * adaptive filter under rt_set_adaptive). The cost order (rt_set_schedule), latency mode,
 * tail compaction (rt_set_tail) and rt_set_walk do not apply to these frames.
 * rt_kernel_times gets one entry per dispatch and rt_sync_frame's marker follows the frame,
 * as for any frame. */
enum { RT_MAX_LIGHTS = 8 };
int rt_set_lights(struct rt_ctx* ctx, const FlatLight* lights, int count);
int rt_get_lights(struct rt_ctx* ctx, FlatLight* lights, int cap, int* count);

/* Area lights: soft shadows from K shadow rays per light (an extension: the reference shader's
 * lights are points and its shadows hard edges).
 *
 * rt_set_soft_shadows gives light i of the set in force (rt_set_lights / rt_set_light) the
 * radius radii[i], i < count; lights with index >= count have radius 0. count is
 * 0..RT_MAX_LIGHTS, every radius finite and >= 0, `samples` is K, 1..RT_MAX_SHADOW_SAMPLES.
 * count == 0 (radii may be NULL, samples is not read) turns the feature off; off is the default.
 * The setting belongs to the context, like rt_set_samples: it is applied at the next dispatch
 * and survives rt_set_lights, rt_set_light and rt_upload_scene. rt_get_soft_shadows mirrors
 * rt_get_lights: min(cap, count) radii to `radii`, the count to `*count`, K to `*samples` (0
 * while the feature is off); any pointer may be NULL, cap is not read when `radii` is NULL.
 * RT_ERR_INVALID for a NULL context, NULL radii with count > 0, a count outside
 * 0..RT_MAX_LIGHTS, samples outside 1..RT_MAX_SHADOW_SAMPLES when count > 0, a negative, NaN or
 * infinite radius, and a negative cap; the previous setting stays in force.
 *
 * When it is active. A dispatch or ray list is soft iff some light i < L (L the light set's
 * size) has radius[i] > 0. One that is not soft runs exactly the kernels it runs without this
 * call, byte for byte; a soft one runs kernels of its own, for L = 1 as well.
 *
 * Definition. A soft pixel is rt_set_lights' pixel except for the shadow factor of each light.
 * Every operation is float32, in the order written, and none is contracted. At a bounce, with
 * the hit point hp, the normal hn and the shadow origin so = hp + hn * off (unchanged: 1e-3
 * with useBVH, 1e-5 on the brute-force branch), for light i with position pos_i, radius R_i:
 *   - R_i == 0: one shadow ray, exactly rt_set_lights' ray. K_i = 1, and b_i is 1 if the ray
 *     is blocked, else 0.
 *   - R_i > 0: K_i = K, and b_i is the number of blocked sample rays k = 0..K-1. Sample ray k:
 *     1. w = normalize(pos_i - hp), the hard shadow ray's direction, the same expression.
 *     2. The tangent frame (t, u) about w is step 2 of rt_dispatch_ao's definition with
 *        nf := w (no facing flip):
 *          sg = copysignf(1, w.z)
 *          a  = -1.0f / (sg + w.z)
 *          b  = (w.x*w.y)*a
 *          t  = (1.0f + sg*((w.x*w.x)*a), sg*b, -(sg*w.x))
 *          u  = (b, sg + (w.y*w.y)*a, -w.y)
 *     3. The rotation is (c, sn) = ROT[j] of rt_dispatch_ao's table, with
 *          j = (((bits(hp.x) ^ bits(hp.y) ^ bits(hp.z)) * 0x9E3779B1u) mod 2^32) >> 28.
 *        j comes from the hit point, not from the pixel: a ray list and a frame agree, and so
 *        do reflected hits.
 *     4. The disc point comes from D[k].x, D[k].y of rt_dispatch_ao's table (the x, y of
 *        cosine-weighted hemisphere points are uniform on the unit disc):
 *          lx = c*D[k].x - sn*D[k].y
 *          ly = sn*D[k].x + c*D[k].y
 *          rx = R_i*lx
 *          ry = R_i*ly
 *     5. The sample point, per component: s.c = pos_i.c + ((t.c*rx) + (u.c*ry)). It lies on a
 *        disc of radius R_i about the light that faces the hit.
 *     6. The ray has origin so and direction normalize(s - hp). It is blocked by an INNER hit
 *        nearer than min(dist(s, hp), 1e20f): the hard ray's test with s in place of pos_i.
 *   - term_i = phong(hp, hn, ray.d, pos_i, color_i, m): Phong uses the centre, once per light.
 *     If b_i > 0, term_i is multiplied by 1.0f - 0.7f * ((float)b_i / (float)K_i). For
 *     b_i == K_i that factor is 1.0f - 0.7f, in float32 exactly 0.3f: a fully blocked light
 *     has the hard shadow's bits.
 * Then pc = term_0, and pc = pc + term_i left to right; the rest of the bounce is the shader's.
 *
 * Limits. The penumbra is K discrete levels, dithered by a hash of the hit point: noise, not a
 * pattern, and rt_set_samples averages it. The disc is not clipped against the surface's
 * horizon.
 *
 * It applies to every frame dispatch form in every pixel and surface format, to frames under
 * rt_set_samples and rt_set_adaptive (such a frame is one the accelerated kernel does not
 * render, as with lights: a scratch sample frame, then the filter or adaptive filter pass) and
 * to rt_shade_rays / rt_shade_rays_host. It does not enter rt_trace_*, rt_dispatch_gbuffer,
 * rt_dispatch_ao, rt_camera_rays, rt_collect_stats* or an rt_group's frames. The cost order,
 * latency mode, rt_set_tail and rt_set_walk do not apply to soft frames. rt_kernel_times gets
 * one entry per dispatch and rt_sync_frame's marker follows the frame;
 * rt_accel_info::last_kernel reports RT_KERNEL_SOFT over the accelerator (camera rays and all
 * their sample rays walk as wave64 packets, later bounces per lane) and RT_KERNEL_LANE for the
 * literal loop (RT_KERNEL_LANE / RT_KERNEL_PACKET, contexts without a usable accelerator, far
 * cameras). Both write the same bytes. */
enum { RT_MAX_SHADOW_SAMPLES = 64 };
int rt_set_soft_shadows(struct rt_ctx* ctx, const float* radii, int count, int samples);
int rt_get_soft_shadows(struct rt_ctx* ctx, float* radii, int cap, int* count, int* samples);

/* The five uniforms (src/main.cpp:357-361). */
int rt_set_params(struct rt_ctx* ctx, const rt_params* params);

/* Kernel variant; RT_KERNEL_AUTO by default. */
int rt_set_kernel(struct rt_ctx* ctx, int kernel);

/* glDispatchCompute(W,H,1) + glMemoryBarrier (src/main.cpp:352-354) into the
 * context's own W x H surface (RGBA32F, or the format of rt_set_surface_format), rows
 * [y0, y1). Stream-ordered, async. */
int rt_dispatch(struct rt_ctx* ctx, int width, int height, int y0, int y1);

/* Same into a caller-owned device surface (for tiling and RCCL gathers).
 * Row-stripe mapping: output row r (0-based, r < out_rows) holds image row
 *   y = y0 + (r / stripe) * stripe * step + (r % stripe)
 * so step = 1 renders the contiguous band [y0, y0+out_rows) and step = P with
 * y0 = k*stripe renders the k-th of P interleaved stripe sets. Rows with
 * y >= height are left untouched. `pitch` is in bytes (>= 16*width). */
int rt_dispatch_rows(struct rt_ctx* ctx, int width, int height, int y0, int stripe,
                     int step, int out_rows, float* dst, size_t pitch);

/* rt_dispatch_rows with an output format: RT_FORMAT_RGBA32F (16 B per pixel, as
 * the reference's image2D rgba32f) or RT_FORMAT_RGB32F (12 B per pixel, packed;
 * the alpha the reference stores is always 1, gpu_shader.comp:437,623). The
 * multi-GPU gather (rt_group.h) sends RGB32F: 25 % fewer bytes over xGMI.
 * pitch >= 12*width and 4-byte aligned for RGB32F.
 * RT_FORMAT_RGBA32F_IMAGE: RGBA32F written at each row's IMAGE row y, not at its
 * compact row r: dst is the whole width x height surface (pitch >= 16*width),
 * and rows the call does not render are left untouched. rt_group's rank 0
 * renders its stripes straight into the gathered frame this way.
 *
 * Display formats: what a host that shows, encodes or saves the frame wants, converted in
 * the render kernel's registers (and in the filter kernel of rt_set_samples), so nothing but
 * the small pixel is written or read back. `dst` keeps its type but is a byte surface here.
 * Per channel c, the float32 value the RGBA32F frame of the same dispatch would hold:
 *   RT_FORMAT_RGBA8   4 B  q = (int)rintf(fminf(fmaxf(c, 0), 1) * 255.0f): the product in
 *                          float32, rounded to nearest even; NaN gives 0.
 *   RT_FORMAT_SRGBA8  4 B  R, G, B sRGB-encoded, alpha as RGBA8: q = the number of k in
 *                          1..255 with clamp(c) >= T[k] (NaN gives 0), where T[k] is the
 *                          float32 nearest to eotf((k - 0.5) / 255) evaluated in double,
 *                          eotf(x) = x / 12.92 for x <= 0.04045, else ((x + 0.055) / 1.055)^2.4.
 *                          The table (rt_srgb_thresholds, csrc/srgb_table.h, generated by
 *                          tools/gen_srgb_table.py) is the definition: the frame agrees with
 *                          it for every float32 input.
 *   RT_FORMAT_RGBA16F 8 B  IEEE float32 -> float16, round to nearest even, all four
 *                          channels; no clamp, overflow becomes inf, NaN stays NaN.
 * Bytes in memory are R, G, B, A (a little-endian dword R | G<<8 | B<<16 | A<<24). The
 * frame's alpha is exactly 1: 255, or 0x3C00 for RGBA16F. Rows are compact, as for
 * RT_FORMAT_RGBA32F (row r of dst; there is no image-row variant). RGBA8 / SRGBA8:
 * pitch >= 4*width, dst and pitch 4-byte aligned; RGBA16F: pitch >= 8*width, dst and pitch
 * 8-byte aligned. Anything else, an unknown format included, is RT_ERR_INVALID before
 * anything is launched. With rt_set_samples the stored pixel is the conversion of the
 * float32 box-filtered value defined there. No tone mapping beyond the clamp, no dither. */
enum rt_format {
    RT_FORMAT_RGBA32F = 0, RT_FORMAT_RGB32F = 1, RT_FORMAT_RGBA32F_IMAGE = 2,
    RT_FORMAT_RGBA8 = 3, RT_FORMAT_SRGBA8 = 4, RT_FORMAT_RGBA16F = 5
};
int rt_dispatch_rows_fmt(struct rt_ctx* ctx, int width, int height, int y0, int stripe, int step, int out_rows,
                         float* dst, size_t pitch, int format);

/* rt_dispatch_rows_fmt with the stripe spacing in rows: compact row r is image
 * row y0 + (r / stripe) * period + r % stripe (period >= stripe; the forms above
 * are period = stripe * step). Lets one rank own a wider stripe than the others
 * in the same period (rt_group_set_root_share). */
int rt_dispatch_rows_ex(struct rt_ctx* ctx, int width, int height, int y0, int stripe, int period, int out_rows,
                        float* dst, size_t pitch, int format);

/* Supersampling: every pixel is the mean of n x n samples on the regular sub-pixel grid.
 * n in {1, 2, 4, 8}; 1 (default) is today's frame. RT_ERR_INVALID for any other n.
 *
 * Applied at the next dispatch, and to every dispatch form (rt_dispatch, rt_dispatch_rows,
 * _fmt, _ex; every format, any y0 / stripe / period / out_rows). The caller's width,
 * height, rows, pitch and rt_params keep their meaning: they describe the OUTPUT frame.
 * The samples are the pixels of the one-sample frame with width, height, y0, stripe,
 * period, out_rows, resX and resY all multiplied by n (the reference's pixel NDC is
 * 2x/resX - 1 and its background y/resY, so that frame's pixels are exactly the n x n
 * regular sub-pixel grid of this one). The filter is fixed, per channel (alpha included)
 * in float32: log2 n rounds along x, each a[i] = a[2i] + a[2i+1]; then log2 n such rounds
 * along y; then one multiply by 1/n^2 (exact). Alpha stays exactly 1. So the frame is that
 * box filter of the renderer's own n*W x n*H frame, bit for bit, for every kernel variant
 * and every other setting.
 *
 * A dispatch whose sample frame breaks a limit of the one-sample dispatch (more than 65535
 * rows of 8x8 tiles, width * rows >= 2^32 samples, a scaled value that overflows int) is
 * refused with RT_ERR_INVALID before anything is launched.
 *
 * Frames the accelerated kernel renders (RT_KERNEL_ACCEL in rt_accel_info::last_kernel)
 * average each n x n block inside the render kernel's store: an 8x8 tile of samples is
 * one wave, so nothing but the output frame is written. Such frames render without ray
 * compaction (rt_set_tail is ignored for them), and latency mode splits a heavy tile only
 * into bands of whole blocks. Every other frame (RT_KERNEL_LANE, RT_KERNEL_PACKET, no
 * usable accelerator, a far camera) renders the sample frame into a surface the context
 * keeps between frames and filters it with a second small kernel.
 *
 * rt_collect_stats* is not affected: it counts the one-sample frame it is given. A host
 * that wants the sample frame's ray counts collects them at n*W x n*H with resX, resY
 * times n. Group frames (rt_group.h) stay one sample per pixel. */
int rt_set_samples(struct rt_ctx* ctx, int n);

/* Adaptive supersampling: with rt_set_samples n > 1, take the n x n samples only where
 * neighbouring pixels of the one-sample frame disagree.
 *
 * threshold < 0 (default -1): off. threshold >= 0 (+inf allowed): on. NaN: RT_ERR_INVALID,
 * and the previous setting stays. Applies at the next dispatch, to every dispatch form and
 * format, when rt_set_samples n > 1; with n == 1 it changes nothing.
 *
 * Two frames define the result, both float32, before any format conversion:
 *   B  the frame this dispatch would write with rt_set_samples(1);
 *   S  the frame it would write with rt_set_samples(n) and adaptive off;
 * over the dispatch's own pixels: compact rows r in [0, out_rows) whose image row y(r) is
 * below height, and x in [0, width).
 *
 * Neighbours of (r, x): (r, x +- 1) where that x is inside the frame, and (r +- 1, x) where
 * that compact row is one of the dispatch's own pixels and its image row is exactly
 * y(r) +- 1. So a full frame has the usual 4-neighbourhood, and a stripe's first and last
 * rows have no neighbour across the gap to the next stripe.
 *
 * A pixel p is refined iff, for some neighbour q and some channel c of R, G, B,
 * !(fabsf(B(p).c - B(q).c) <= threshold), the subtraction being one float32 operation. A NaN
 * therefore refines, and both pixels of a contrasting pair refine. Each pixel is S(p) if
 * refined and B(p) otherwise, then goes through the dispatch's format conversion as ever;
 * alpha is exactly 1. So every pixel holds one of two values the renderer already defines,
 * and the threshold only decides which: +inf gives B exactly, a threshold below every
 * contrast gives S exactly. (B(p) is also sample (0, 0) of p's block.)
 *
 * Limit: a feature thinner than a pixel between two pixels of equal colour is not found.
 *
 * Frames the accelerated kernel renders take the fast path: B as an ordinary one-sample
 * dispatch (latency mode, cost order and rt_set_tail apply to it) into a surface the context
 * keeps, one small kernel that writes the unrefined pixels and lists the refined ones, and
 * one that shades the listed pixels' samples; the host reads nothing in between, the dispatch
 * stays asynchronous. Every other frame (RT_KERNEL_LANE, RT_KERNEL_PACKET, no usable
 * accelerator, a far camera) renders the whole sample frame as for rt_set_samples and picks
 * per pixel in the filter kernel: the same image, exact for every kernel variant, and not
 * faster than full supersampling.
 *
 * rt_collect_stats*, rt_trace_*, rt_group frames, the cost order and
 * rt_accel_info::last_kernel (the kernel that rendered B) are unaffected. One rt_kernel_times
 * entry covers all passes of the dispatch, and rt_sync_frame's marker follows the last. */
int rt_set_adaptive(struct rt_ctx* ctx, float threshold);

/* Pixels of the last dispatch that ran adaptively: how many were refined, how many it wrote
 * (either pointer may be NULL). Waits for that dispatch. RT_ERR_INVALID if no dispatch of
 * this context ran adaptively. */
int rt_adaptive_stats(struct rt_ctx* ctx, uint64_t* refined, uint64_t* pixels);

/* glMemoryBarrier + wait: blocks until the context's stream is drained. */
int rt_sync(struct rt_ctx* ctx);

/* The wait of the reference's render loop (src/main.cpp:290-462: dispatch, barrier, draw,
 * swap): blocks until the last dispatch's frame is complete -- its image and every upload
 * issued before it. Scheduling work the renderer queued behind the frame for the next one
 * (a latency-mode cost frame's tile order) may still be running; the next dispatch on the
 * same stream runs after it. Work the host enqueued after that dispatch is not waited for
 * (use rt_sync); when there is no such frame marker it is rt_sync. */
int rt_sync_frame(struct rt_ctx* ctx);

/* Read the context surface back to host memory: `height` rows of `pitch` bytes.
 * width/height state the destination's size and must equal the surface's (the
 * last rt_dispatch's W x H), so a short buffer is refused, never overrun.
 * RT_ERR_INVALID when the surface is not RGBA32F (rt_set_surface_format): use
 * rt_read_surface. */
int rt_read_image(struct rt_ctx* ctx, float* host_dst, size_t pitch, int width, int height);

/* Device pointer and pitch of the context surface (zero-copy hand-off), in the
 * surface's format. */
int rt_device_image(struct rt_ctx* ctx, void** ptr, size_t* pitch);

/* The format of the context's own surface: RT_FORMAT_RGBA32F (default), RT_FORMAT_RGBA8,
 * RT_FORMAT_SRGBA8 or RT_FORMAT_RGBA16F; any other value is RT_ERR_INVALID. Applies at the
 * next rt_dispatch, which reallocates the surface (pitched at the format's row bytes,
 * zero-filled) when the format, width or height changed; until then the surface, and what
 * rt_read_image / rt_read_surface / rt_device_image see, stay as they are.
 * rt_surface_format returns the format set here. */
int rt_set_surface_format(struct rt_ctx* ctx, int format);
int rt_surface_format(struct rt_ctx* ctx, int* format);

/* rt_read_image for whatever format the surface has: `height` rows of `pitch` bytes,
 * pitch >= bytes per pixel * width. width/height must equal the surface's, so a short
 * buffer is refused, never overrun. A 1920x1080 RGBA8 frame is 8.3 MB against 33.2 MB. */
int rt_read_surface(struct rt_ctx* ctx, void* host_dst, size_t pitch, int width, int height);

/* The table T[1..255] that defines RT_FORMAT_SRGBA8, as 255 floats: out255[k - 1] = T[k].
 * Needs no device. */
int rt_srgb_thresholds(float* out255);

/* Runs the counting variant of the reference traversal over the same rows as
 * rt_dispatch_rows and returns the totals (synchronous; not for timed loops). */
int rt_collect_stats(struct rt_ctx* ctx, int width, int height, int y0, int stripe,
                     int step, int out_rows, rt_stats* out);
/* The same over rt_dispatch_rows_ex's rows. */
int rt_collect_stats_ex(struct rt_ctx* ctx, int width, int height, int y0, int stripe,
                        int period, int out_rows, rt_stats* out);

/* Record the device-time events around each render dispatch (default 1), which
 * rt_kernel_times / rt_last_kernel_ms read. Each is a timestamped marker on the
 * stream, and a host that waits for every frame pays for them (~4 us per waited
 * car frame, tools/group_cost.py). 0: no events; rt_kernel_times then reports
 * no dispatches. Same image either way. */
int rt_set_kernel_timing(struct rt_ctx* ctx, int on);

/* Device time of the last render kernel in ms (HIP events on the context stream). */
int rt_last_kernel_ms(struct rt_ctx* ctx, float* ms);

/* Device times (ms) of the render dispatches issued since the previous call
 * (up to 1024 are kept), written to ms[0..min(n,cap)). Returns n >= 0 and
 * restarts the record. Waits for those dispatches to finish. */
int rt_kernel_times(struct rt_ctx* ctx, float* ms, int cap);

/* Accelerated kernel: bounces with depth >= lane_from_depth walk one ray per
 * lane (LDS stack) instead of one packet per wave; 0 = all bounces per lane,
 * >= maxBounces = all packet. Default (auto): 1 -- camera rays and their shadow
 * rays walk as packets (coherent), reflections per lane (measured fastest on
 * configs 2, 3 and 5) -- and all packets for Moller-Trumbore frames over
 * reference trees of fewer than 1024 nodes. -1 restores that automatic policy.
 * Same image for every value. */
int rt_set_walk(struct rt_ctx* ctx, int lane_from_depth);

/* Tile dispatch order of the accelerated kernel. RT_SCHED_ROWS: row-major.
 * RT_SCHED_COST (default): a dispatch records each 8x8 tile's duration (its
 * wave's wall time, in 40 ns units; every 16th frame once the order exists),
 * and the next dispatch with the same tile count starts the tiles in
 * decreasing order of those durations (longest first), so the frame is not
 * left waiting on expensive tiles that started late. The order only changes
 * when pixels are computed, never their values. RT_SCHED_COST_XCD: the same
 * longest-first order, with each bucket of equal cost split into 8 screen
 * bands, one per XCD (workgroups are dealt to the XCDs round-robin), so each
 * XCD's L2 holds the records of one band at a time. */
enum rt_schedule { RT_SCHED_ROWS = 0, RT_SCHED_COST = 1, RT_SCHED_COST_XCD = 2 };
int rt_set_schedule(struct rt_ctx* ctx, int mode);

/* Latency mode, for a host that waits for each frame before the next (the
 * reference's own loop, src/main.cpp:290-462) rather than keeping frames in
 * flight. 1: the accelerated kernel's instance with split walks in sparse
 * waves (idle lanes help a tile's few live rays) and, on frames not already
 * split, the heaviest tiles of the cost order as several waves each: 1/200 as
 * two (four for all-packet frames such as Moller-Trumbore's), and on frames of
 * few tiles per CU (a rank's share of a strong multi-GPU frame) 1/25 as eight or
 * sixteen. A dispatch whose camera moved since the last one re-ranks the tiles
 * after every frame (whole-tile wall times, each tile ranked by the largest
 * within one tile). Shortens one frame (car: -18 %) and costs throughput when
 * frames overlap. Frames of more than 12 tiles per wave slot (49,152 8x8 tiles
 * on 256 CUs: 3840x2160 has 129,600) render as in the default mode, which is
 * faster for them. 0 (default): off. Same image either way. */
int rt_set_latency_mode(struct rt_ctx* ctx, int on);

/* Ray compaction in the accelerated kernel: the rays still alive after bounce
 * from_bounce - 1 are queued per 64x64-pixel region, and a second kernel runs
 * their remaining bounces 64 rays to a wave instead of in their half-empty tile
 * waves. 0 = off; RT_TAIL_AUTO (default) = from bounce 2 on scenes whose scene
 * tree has at least 8,192 items (the 100k-triangle config: -5 %), off otherwise
 * (the car: the extra kernel costs more than it saves). Same image for every
 * value (the bounces' arithmetic is the same; a ray's walk does not depend on
 * its wave's other rays). */
enum { RT_TAIL_AUTO = -1 };
int rt_set_tail(struct rt_ctx* ctx, int from_bounce);

/* Opt-in device BVH build (lbvh.hip). Builds a linear
 * BVH (Karras 2012: Morton codes of the shapes' split() centres, radix sort,
 * one shape per leaf) on the GPU over the current shapes, in the FlatNode /
 * bvhIndices layout (root at N-1 = 2S-2, node boxes = the reference's
 * BoundingBox of their shapes), and adopts it as if the host had passed it to
 * rt_upload_scene (which also clears the animated set). It replaces the
 * reference builder's tree (src/main.cpp:1111-1193), so frames are the
 * reference shader's frames over THIS tree: read it back with rt_scene_size,
 * rt_read_nodes and rt_read_indices to reproduce them elsewhere.
 * *device_ms (optional) = device time of the build kernels. */
int rt_build_lbvh(struct rt_ctx* ctx, float* device_ms);
int rt_scene_size(struct rt_ctx* ctx, int* num_shapes, int* num_nodes, int* num_indices);
int rt_read_indices(struct rt_ctx* ctx, int* indices, int num_indices);

/* Which tree the accelerated kernel walks. RT_TREE_SCENE (default): when the
 * reference tree's child boxes nest in their parents' boxes, rays whose slab
 * values cannot be NaN walk one SAH tree over all reference leaves' shapes,
 * testing each leaf's own exact box before its shapes (the nesting makes that
 * test equivalent to the reference's walk down to the leaf); other rays walk the
 * reference tree. Animated and updated scenes keep the scene tree: the refit
 * (rt_animate, rt_update_shapes / rt_update_nodes) refits its boxes and items,
 * and node boxes that stop nesting rebuild the accelerator without it.
 * RT_TREE_REFERENCE: every ray walks the reference tree. Same image either way. */
enum rt_tree { RT_TREE_REFERENCE = 0, RT_TREE_SCENE = 1 };
int rt_set_tree(struct rt_ctx* ctx, int mode);

/* Ray queries over the uploaded scene: picking, line of sight, distance along a ray.
 *
 * Every ray gets the answer of the reference's BVH branch (gpu_shader.comp:380-430) over
 * the context's current tree and shapes: the closest INNER hit by distance, strict "<" in
 * the reference's walk order, so ties go to the first shape the reference would find.
 * rt_params::useBVH does not matter to a query; useMollerTrumbore selects the triangle
 * test as for the next dispatch (barycentric if no params were ever set). Camera, light,
 * bounces, Fresnel and rt_set_samples do not enter. rt_set_kernel and rt_set_tree apply
 * as they do to frames: the accelerated walk (its Moller-Trumbore form for MT queries), or
 * the literal reference walk for RT_KERNEL_LANE / RT_KERNEL_PACKET and scenes without an
 * accelerator. Same answers either way. Rays are walked in the order given, 64 consecutive
 * rays to a wave: coherent neighbours are faster.
 *
 * A query reads the device scene: like a dispatch it first applies pending
 * rt_update_shapes / rt_update_nodes / rt_animate work as one refit, so it sees the scene
 * the next frame would see. It does not touch the context surface, rt_accel_info::
 * last_kernel, the record of rt_kernel_times / rt_last_kernel_ms, rt_sync_frame's frame
 * marker or the tile cost order.
 *
 * RT_TRACE_CLOSEST fills shape and distance, and occluded = (shape >= 0 && distance <
 * limit). RT_TRACE_ANY is the shadow walk: it stops at the first INNER hit nearer than
 * limit, fills occluded only and writes shape = -1, distance = 1e20f. */
typedef struct rt_ray {      /* 32 bytes, 16-byte aligned */
    float origin[3];
    float limit;             /* occlusion limit: a distance from the origin, as the shader's light distance */
    float dir[3];            /* any length; need not be normalised */
    int   reserved;          /* 0 */
} rt_ray;

typedef struct rt_hit {      /* 16 bytes */
    int   shape;             /* index into the uploaded FlatShape array, -1 = miss */
    float distance;          /* the reference's distance(origin, hit point); 1e20f on a miss */
    int   occluded;          /* 1 if an INNER hit lies nearer than rt_ray::limit, else 0 */
    int   reserved;          /* 0 */
} rt_hit;

enum rt_trace_mode { RT_TRACE_CLOSEST = 0, RT_TRACE_ANY = 1 };

RT_STATIC_ASSERT(sizeof(rt_ray) == 32 && offsetof(rt_ray, limit) == 12 && offsetof(rt_ray, dir) == 16, "rt_ray");
RT_STATIC_ASSERT(sizeof(rt_hit) == 16 && offsetof(rt_hit, distance) == 4 && offsetof(rt_hit, occluded) == 8, "rt_hit");

/* dev_rays / dev_hits are device pointers, 16-byte aligned; stream-ordered on the context's
 * stream, asynchronous. RT_ERR_INVALID: a null pointer with n > 0, n < 0, an unknown mode,
 * a misaligned pointer. RT_ERR_NO_SCENE before rt_upload_scene. n == 0 launches nothing.
 * A scene without nodes answers every ray with a miss. */
int rt_trace_rays(struct rt_ctx* ctx, const rt_ray* dev_rays, int n, rt_hit* dev_hits, int mode);

/* The same with host pointers, staged through buffers the context keeps between calls;
 * returns when the hits are in `hits`. */
int rt_trace_rays_host(struct rt_ctx* ctx, const rt_ray* rays, int n, rt_hit* hits, int mode);

/* Picking: RT_TRACE_CLOSEST with an infinite limit for the camera ray of each pixel
 * (xy[2i], xy[2i+1]) of a width x height frame, generated on the device exactly as a
 * dispatch generates it (current camera, rt_params::resX / resY). Host pointers;
 * synchronous. RT_ERR_NO_SCENE without a camera or params, RT_ERR_INVALID for a pixel
 * outside the frame. */
int rt_trace_pixels(struct rt_ctx* ctx, int width, int height, const int* xy, int n, rt_hit* hits);

/* Geometry buffer: per pixel, the shape under it, its depth, the surface normal and the hit
 * point -- what a host needs to composite raster content over the traced image, to outline
 * or mask shapes, or for screen-space effects. One kernel of its own walks the camera rays
 * of whole 8x8 tiles as wave64 packets; no ray or hit list crosses the bus.
 *
 * Planes. Each plane is a caller surface with its own pitch in bytes; a NULL pointer means
 * the plane is not wanted (at least one must be given).
 *
 * Rows. The compact rows of rt_dispatch_rows_ex: row r in [0, out_rows) of every plane is
 * image row y(r) = y0 + (r / stripe) * period + r % stripe. A row with y(r) >= height is left
 * untouched in every plane. Within a row only the first `width` pixels are written (4*width
 * or 16*width bytes); not one byte after them is touched.
 *
 * What a pixel holds. For pixel (x, y), take the camera ray a dispatch generates (current
 * camera, rt_params::resX / resY, NDC 2x/resX - 1, 1 - 2y/resY) and the answer
 * rt_trace_pixels gives for it: the closest INNER hit of the reference's BVH branch over the
 * context's current tree and shapes, ties to the first shape in the reference's walk order.
 *   shape     int32 index into the uploaded FlatShape array; -1 on a miss.
 *   depth     float32 rt_hit::distance, the shader's distance(origin, hit); 1e20f on a miss.
 *   position  (p.x, p.y, p.z, 1.0f) with p = origin + t * dir, the hit point the shader
 *             shades (the point get_intersection returns); (0, 0, 0, 0) on a miss, so w is
 *             a hit mask.
 *   normal    (n.x, n.y, n.z, 0.0f) with n = getNormalFromShape at p: for a sphere
 *             n = v * (1.0f / sqrtf((v.x*v.x + v.y*v.y) + v.z*v.z)) with v = p - centre, all
 *             in float32; for a plane, wall or triangle the record's planeNormal, its bits
 *             unchanged; (0, 0, 0, 0) on a miss. The normal is not flipped towards the
 *             viewer: it is the value the shading uses.
 * Every value is exact: the same bits from every kernel variant.
 *
 * What applies: useMollerTrumbore, rt_set_kernel and rt_set_tree, exactly as they do to
 * rt_trace_pixels. What does not enter: useBVH, light, bounces, Fresnel, rt_set_samples,
 * rt_set_adaptive, latency mode, schedule and tail. With rt_set_samples(n) the buffer
 * describes sample (0, 0) of each pixel: the frame B of rt_set_adaptive.
 *
 * Like a query, the call first applies pending rt_update_shapes / rt_update_nodes /
 * rt_animate work as one refit. It leaves alone the surface, rt_accel_info::last_kernel, the
 * record of rt_kernel_times / rt_last_kernel_ms, rt_sync_frame's marker, the tile cost order
 * and rt_adaptive_stats.
 *
 * Errors, returned before anything is launched. RT_ERR_INVALID: out == NULL; all four
 * planes NULL; width, height or stripe <= 0, y0 or out_rows < 0, period < stripe (as
 * rt_dispatch_rows_ex); a shape or depth pitch below 4*width or not 4-byte aligned; a normal
 * or position pitch below 16*width or not 16-byte aligned; a misaligned plane pointer (4
 * bytes for shape and depth, 16 for normal and position); a limit of the one-sample dispatch
 * broken (more than 65,535 rows of 8x8 tiles, width * out_rows >= 2^32). RT_ERR_NO_SCENE
 * without a scene, camera or params, as for rt_trace_pixels. out_rows == 0 is RT_OK and
 * launches nothing. A scene without nodes makes every pixel a miss.
 *
 * Group frames (rt_group.h) have no geometry buffer. A view-space depth is
 * dot(position - camera.Position, camera.Front); there is no plane for it. */
typedef struct rt_gbuffer {          /* planes; a NULL pointer = plane not wanted */
    int*   shape;    size_t shape_pitch;     /*  4 B / pixel */
    float* depth;    size_t depth_pitch;     /*  4 B / pixel */
    float* normal;   size_t normal_pitch;    /* 16 B / pixel */
    float* position; size_t position_pitch;  /* 16 B / pixel */
} rt_gbuffer;

RT_STATIC_ASSERT(sizeof(rt_gbuffer) == 8 * sizeof(void*) && offsetof(rt_gbuffer, shape_pitch) == sizeof(void*) &&
                 offsetof(rt_gbuffer, depth) == 2 * sizeof(void*) && offsetof(rt_gbuffer, normal) == 4 * sizeof(void*) &&
                 offsetof(rt_gbuffer, position) == 6 * sizeof(void*) &&
                 offsetof(rt_gbuffer, position_pitch) == 7 * sizeof(void*), "rt_gbuffer");

/* Device pointers; stream-ordered on the context's stream, asynchronous. */
int rt_dispatch_gbuffer(struct rt_ctx* ctx, int width, int height, int y0, int stripe, int period,
                        int out_rows, const rt_gbuffer* out);

/* Host pointers, the whole frame (rows [0, height)), staged through buffers the context keeps
 * between calls; returns when the planes are in host memory. Pointers and pitches are checked
 * as above. */
int rt_gbuffer_host(struct rt_ctx* ctx, int width, int height, const rt_gbuffer* host_out);

/* Ambient occlusion: per pixel, how many of `rays` fixed hemisphere rays about the visible
 * surface's normal are blocked within `radius`. A host multiplies its ambient term by the
 * visibility plane. One kernel of its own finds the camera hit, builds the
 * rays and walks them; no ray, hit or geometry plane crosses the bus. Nothing in a frame
 * dispatch changes: applying the term is the host's.
 *
 * Planes, rows, what applies, what does not enter, pending updates and what is left alone:
 * exactly as rt_dispatch_gbuffer above (rows y(r) >= height untouched; of a row only the first
 * `width` pixels are written, `width` bytes of count and 4*width bytes of visibility, not one
 * byte after them). With rt_set_samples(n) the planes describe sample (0, 0).
 *
 * Definition of a pixel. Every operation is float32, in the order written, none contracted.
 * Take rt_dispatch_gbuffer's values of pixel (x, y): shape, position p and normal n; and the
 * camera ray's direction d as a dispatch generates it. A miss (shape -1) has count 0 and
 * visibility 1.0f. Otherwise:
 *  1. Facing. s = (n.x*d.x + n.y*d.y) + n.z*d.z; nf = s > 0 ? -n : n (a NaN keeps n).
 *  2. Frame. sg = copysignf(1, nf.z); a = -1.0f / (sg + nf.z); b = (nf.x*nf.y)*a;
 *       t = (1.0f + sg*((nf.x*nf.x)*a), sg*b, -(sg*nf.x));
 *       u = (b, sg + (nf.y*nf.y)*a, -nf.y).
 *  3. Tables (csrc/ao_table.h, written by tools/gen_ao_table.py, returned by rt_ao_table; the
 *     tables are the definition, as the thresholds are for RT_FORMAT_SRGBA8).
 *       D[k], k = 0..63: cosine-weighted Halton points; with u1 the radical inverse of k + 1 in
 *       base 2 and u2 that in base 3, D[k] = (sqrt(u1) cos 2 pi u2, sqrt(u1) sin 2 pi u2,
 *       sqrt(1 - u1)) in double, rounded to float32. Ray count K uses D[0..K-1].
 *       ROT[j], j = 0..15: (cos, sin) of 2 pi ((7 j) mod 16) / 16 in double, rounded to float32.
 *  4. Rotation per pixel (interleaved sampling; a 4x4 blur by the host removes the pattern).
 *     j = (x & 3) + 4*(y & 3) on image coordinates, (c, sn) = ROT[j];
 *       lx = c*D[k].x - sn*D[k].y; ly = sn*D[k].x + c*D[k].y; lz = D[k].z.
 *  5. Ray k. Origin p + nf*bias per component (one multiply, one add: the shader's shadow
 *     origin); direction per component (t.c*lx + u.c*ly) + nf.c*lz; limit radius.
 *  6. count = the number of k < rays whose ray is occluded in the sense of RT_TRACE_ANY: an
 *     INNER hit nearer than min(radius, 1e20f). visibility = (float)(rays - count) /
 *     (float)rays, one IEEE division.
 * Every value is exact: the same bytes from every kernel variant, and count equals the sum of
 * rt_trace_rays(RT_TRACE_ANY) over these rays.
 *
 * Errors, returned before anything is launched. RT_ERR_INVALID: everything
 * rt_dispatch_gbuffer refuses about ctx, width, height, y0, stripe, period and out_rows;
 * params or out NULL; rays outside 1..64; radius NaN or <= 0 (+inf is allowed); bias NaN,
 * negative or infinite; reserved != 0; both planes NULL; count_pitch < width; a visibility
 * pointer or pitch not 4-byte aligned, or visibility_pitch < 4*width. RT_ERR_NO_SCENE as for
 * the geometry buffer. out_rows == 0 is RT_OK and launches nothing. */
typedef struct rt_ao_params {
    int rays;        /* K, 1..64 */
    float radius;    /* occlusion distance, > 0, may be +inf */
    float bias;      /* origin offset along the facing normal, >= 0, finite */
    int reserved;    /* 0 */
} rt_ao_params;

typedef struct rt_ao {               /* planes; a NULL pointer = plane not wanted, at least one */
    uint8_t* count;      size_t count_pitch;       /* 1 B / pixel: occluded rays, 0..rays */
    float*   visibility; size_t visibility_pitch;  /* 4 B / pixel: (float)(rays - count) / (float)rays */
} rt_ao;

RT_STATIC_ASSERT(sizeof(rt_ao_params) == 16 && offsetof(rt_ao_params, radius) == 4 &&
                 offsetof(rt_ao_params, bias) == 8 && offsetof(rt_ao_params, reserved) == 12, "rt_ao_params");
RT_STATIC_ASSERT(sizeof(rt_ao) == 4 * sizeof(void*) && offsetof(rt_ao, count_pitch) == sizeof(void*) &&
                 offsetof(rt_ao, visibility) == 2 * sizeof(void*) &&
                 offsetof(rt_ao, visibility_pitch) == 3 * sizeof(void*), "rt_ao");

/* Device pointers; stream-ordered on the context's stream, asynchronous. */
int rt_dispatch_ao(struct rt_ctx* ctx, int width, int height, int y0, int stripe, int period, int out_rows,
                   const rt_ao_params* params, const rt_ao* out);

/* Host pointers, the whole frame (rows [0, height)), staged through buffers the context keeps
 * between calls; returns when the planes are in host memory. Checked as above. */
int rt_ao_host(struct rt_ctx* ctx, int width, int height, const rt_ao_params* params, const rt_ao* host_out);

/* The defining tables: D as 64 x 3 floats, ROT as 16 x 2; either pointer may be NULL. Needs no
 * device and no context. */
int rt_ao_table(float* dirs64x3, float* rot16x2);

/* Shaded rays: the frame's shading for rays the caller gives -- a second eye, the six faces of
 * a probe, a fisheye or orthographic view, a lens, a sparse or foveated pattern, a mirror or
 * portal view. A dispatch aims its rays with one pinhole camera (getRay,
 * gpu_shader.comp:155-168); here the host aims them, and everything after the camera ray is the
 * frame's: closest hit, Phong, the hard shadow, mirror bounces, Fresnel.
 *
 * Definition. Pixel i is the value main() of the reference shader (gpu_shader.comp:432-624)
 * computes when its camera ray is ray i: acc = 0, att = 1, then up to maxBounces bounces; on a
 * miss at any bounce the background mix((0.05, 0.07, 0.1), (0.5, 0.7, 1.0), sky) with that ray's
 * own `sky` (a frame computes the same expression with sky = (float)y / resY); alpha exactly 1.
 * The direction is used as given, without normalisation: in the walk, in reflect and as Phong's
 * view vector (the shading assumes unit length; a direction of another length is shaded as the
 * shader would shade it). A ray whose origin, direction and sky are bit-equal to what a dispatch
 * generates for pixel (x, y) gets that pixel's bits, from every kernel variant.
 *
 * Formats. RT_FORMAT_RGBA32F (16 B per pixel, dev_pixels 16-byte aligned), RT_FORMAT_RGB32F
 * (12 B, 4-byte aligned), RT_FORMAT_RGBA8 and RT_FORMAT_SRGBA8 (4 B, 4-byte aligned),
 * RT_FORMAT_RGBA16F (8 B, 8-byte aligned), with the conversions rt_dispatch_rows_fmt defines.
 * Pixels are compact: pixel i at i * bytes per pixel, and not one byte after pixel n - 1 is
 * written. RT_FORMAT_RGBA32F_IMAGE and unknown formats are RT_ERR_INVALID.
 *
 * What applies: maxBounces, useBVH, useFresnel and useMollerTrumbore (the brute-force branch's
 * 1e-5 shadow offset included), the light, rt_set_kernel and rt_set_tree. What does not enter:
 * the camera, resX and resY, rt_set_samples, rt_set_adaptive, latency mode, schedule, tail and
 * rt_set_walk. Rays are shaded in the order given, 64 consecutive rays to a wave: neighbours
 * that point the same way are faster ("Your own camera"). The call never
 * reorders rays.
 *
 * Like a query, the call first applies pending rt_update_shapes / rt_update_nodes / rt_animate
 * work as one refit. It leaves alone the context surface, rt_accel_info::last_kernel, the record
 * of rt_kernel_times / rt_last_kernel_ms, rt_sync_frame's marker, the tile cost order and
 * rt_adaptive_stats. Overlapping ray and pixel buffers are undefined.
 *
 * Errors, returned before anything is launched. RT_ERR_INVALID: a NULL context, n < 0, a NULL
 * pointer with n > 0, a bad format, a misaligned device pointer (rays 16 bytes, pixels as
 * above). RT_ERR_NO_SCENE without a scene, a light or params; a camera is not needed. n == 0 is
 * RT_OK and launches nothing. A scene without nodes gives every ray its background (with
 * maxBounces > 0). */
typedef struct rt_view_ray {   /* 32 bytes, 16-byte aligned */
    float origin[3];
    float sky;                 /* background parameter: the value a frame uses as y / resY */
    float dir[3];              /* used as given; the shading assumes unit length */
    int   reserved;            /* 0 */
} rt_view_ray;

RT_STATIC_ASSERT(sizeof(rt_view_ray) == 32 && offsetof(rt_view_ray, sky) == 12 && offsetof(rt_view_ray, dir) == 16 &&
                 offsetof(rt_view_ray, reserved) == 28, "rt_view_ray");

/* Device pointers; stream-ordered on the context's stream, asynchronous. */
int rt_shade_rays(struct rt_ctx* ctx, const rt_view_ray* dev_rays, int n, void* dev_pixels, int format);

/* Host pointers (any alignment), staged through buffers the context keeps between calls;
 * returns when the pixels are in host memory. */
int rt_shade_rays_host(struct rt_ctx* ctx, const rt_view_ray* rays, int n, void* pixels, int format);

/* The generator a host starts from and perturbs: for y in [y0, y0 + rows) and x in [0, width),
 * record (y - y0) * width + x holds the origin and direction a dispatch of a width x height
 * frame generates for pixel (x, y), bit for bit (current camera, rt_params::resX / resY),
 * sky = (float)y / resY (one IEEE division) and reserved = 0. So rt_shade_rays over the list is
 * the frame's rows [y0, y0 + rows). RT_ERR_INVALID: width, height or rows <= 0, y0 < 0,
 * y0 + rows > height (the list has no holes), a NULL pointer, a device pointer not 16-byte
 * aligned, width * rows >= 2^31. RT_ERR_NO_SCENE without a camera or params; an uploaded scene
 * is not needed. The device form is stream-ordered and asynchronous; the host form returns when
 * the records are in host memory. */
int rt_camera_rays(struct rt_ctx* ctx, int width, int height, int y0, int rows, rt_view_ray* dev_rays);
int rt_camera_rays_host(struct rt_ctx* ctx, int width, int height, int y0, int rows, rt_view_ray* rays);

/* Accelerator statistics for the uploaded scene. */
int rt_accel_info_get(struct rt_ctx* ctx, rt_accel_info* out);

/* Human-readable status string. */
const char* rt_status_string(int status);

#ifdef __cplusplus
}
#endif

#endif /* RT_API_H */
