/*
 * rt_api.h — C-ABI drop-in boundary for the render-loop hot path of
 * SakibSaikia/CPURayTracer (src/spheres), MI355X-native implementation.
 *
 * The reference has no FFI: the replaceable statements are the two Parallel-STL
 * algorithms inside SpheresApp::DrawBitmap
 *     std::for_each(par, rays, hdr[id] += GetHitColor(ray,0) * exposure)   spheres-app.cpp:177-184
 *     std::transform(par, hdr -> ldr: /n, ACES, gamma, XMStoreColor)       spheres-app.cpp:196-214
 * plus the serial ray generation feeding them (GenerateRays, spheres-app.cpp:132-161).
 * This header is what a binding for that path binds: plain C types, caller-owned
 * host buffers, device memory owned by the handle.  Every entry point returns an
 * int status (RT_OK == 0); rt_last_error() returns the message for the calling
 * thread.  Calls on one handle are serialised by the caller; one handle per device.
 *
 * The library behind this header is librt_hip.so (cpuraytracer_amd/csrc/): hand
 * written HIP for gfx950.  There is NO CPU fallback: rt_create fails loudly when
 * no HIP device is present.  The CPU restatement used for parity checks lives in
 * oracle/ behind oracle/oracle_api.h and shares only the POD records below.
 */
#ifndef RT_API_H
#define RT_API_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_API_VERSION 2 /* 2: rt_scene_upload takes the LIST of lights (spheres-app.h:38 m_lights), not one sun */

enum rt_status {
    RT_OK = 0,
    RT_ERR_NO_DEVICE = 1,     /* no HIP device / ordinal out of range              */
    RT_ERR_INVALID_ARG = 2,   /* null pointer, zero size, bad range                */
    RT_ERR_NO_SCENE = 3,      /* rt_render before rt_scene_upload                  */
    RT_ERR_HIP = 4,           /* a HIP runtime call failed (see rt_last_error)     */
    RT_ERR_OUT_OF_MEMORY = 5,
    RT_ERR_SEQUENCE = 6       /* sample range does not continue the accumulation   */
};

/* ------------------------------------------------------------------ records */

/* Sphere — common-lib/ray-tracing.h:53-57 (center, radius); material i belongs to sphere i. */
typedef struct rt_sphere {
    float cx, cy, cz, r;
} rt_sphere; /* 16 B */

/* Material kinds — common-lib/material.h:21,37,54,70 */
enum rt_material_type {
    RT_MAT_DIELECTRIC_OPAQUE = 0,
    RT_MAT_METAL = 1,
    RT_MAT_DIELECTRIC_TRANSPARENT = 2,
    RT_MAT_EMISSIVE = 3
};

/* Texture kinds — common-lib/texture.h:12,22 */
enum rt_texture_type {
    RT_TEX_CONST = 0,
    RT_TEX_CHECKER = 1
};

/* Material + its (single) texture, flattened.  Colours are the values the
 * reference holds after XMLoadColor(XMCOLOR) (texture.cpp:5,16-17): byte * (1/255).
 *
 * The material domain -- what rt_scene_upload (every sphere's record and the sky's) and rt_unit_scatter accept; anything else is
 * RT_ERR_INVALID_ARG with a message naming the sphere (or "the sky") and the field:
 *   - type <= 3 and tex_type <= 1 (the enums above);
 *   - the fields the record's type reads are finite: smoothness for types 0, 1, 2; ior for type 2; luminance for type 3; rgb0
 *     for types 0, 1, 3; rgb1 and tiling only under a checker texture, on types 0, 1, 3 (a glass sphere has no texture).  Fields
 *     the type does not read are NOT inspected: callers leave them unset;
 *   - under a checker texture |tiling| <= 2^30: CheckerTexture::Evaluate (texture.cpp:20-33) forms (int)(tiling * u) with
 *     u = 0.5 n + 0.5, |n| within a few ulp of 1, and beyond int that conversion is undefined in C++ (x86 and gfx950 give
 *     different values).
 * Colours off the byte grid are accepted: they lie outside the parity contract with the reference (which can only hold bytes)
 * and take the 48-byte records on the device. */
typedef struct rt_material {
    uint32_t type;       /* rt_material_type                                         */
    uint32_t tex_type;   /* rt_texture_type (opaque: albedo, metal: reflectance)     */
    float smoothness;    /* m_smoothness (replicated scalar)                         */
    float ior;           /* DielectricTransparent::m_ior                             */
    float tiling;        /* CheckerTexture::m_tilingScale                            */
    float rgb0[3];       /* ConstTexture colour / checker colour 0                   */
    float rgb1[3];       /* checker colour 1                                         */
    float luminance;     /* Emissive::m_luminance                                    */
} rt_material; /* 48 B */

/* Camera members after Camera::Camera — common-lib/camera.h:14-19, camera.cpp:3-28 */
typedef struct rt_camera {
    float origin[4];              /* m_origin            */
    float x[4];                   /* m_x = halfWidth*u   */
    float y[4];                   /* m_y = halfHeight*v  */
    float origin_image_plane[4];  /* m_originImagePlane  */
    float aperture;               /* m_aperture          */
    float focal_length;           /* m_focalLength       */
} rt_camera; /* 72 B */

/* DirectionalLight members — common-lib/light.h:18-21, light.cpp:4-9 */
typedef struct rt_light {
    float direction[3];  /* normalised */
    float color[3];      /* XMLoadColor of the ctor colour */
    float luminance;
} rt_light; /* 28 B */

/* Rows of the W x H image this call renders.  The row range
 * [first_row, first_row+num_rows) is cut into blocks of block_rows rows; the
 * call owns the blocks b with b % nshards == shard (cyclic: cost is strongly
 * row dependent).  Owned rows, in increasing order, are the "local rows" of the
 * HDR/LDR strip.  {0, H, H, 0, 1} is the whole image. */
typedef struct rt_rowset {
    uint32_t first_row;
    uint32_t num_rows;
    uint32_t block_rows;
    uint32_t shard;
    uint32_t nshards;
} rt_rowset;

/* Counters a render call returns; traversals must equal the oracle's count. */
typedef struct rt_stats {
    uint64_t samples;      /* (pixel, s) paths traced                               */
    uint64_t traversals;   /* ray-vs-whole-list scans: closest-hit + shadow         */
    uint64_t segments;     /* closest-hit scans only (= ray segments)               */
    double ms_render;      /* HIP-event time of the trace kernel(s)                 */
    double ms_accumulate;  /* HIP-event time of the ordered accumulate kernel       */
    double ms_resolve;     /* HIP-event time of the last rt_resolve                 */
    uint32_t local_rows;   /* rows in this shard's strip                            */
    uint32_t passes;       /* sample-range passes the call was split into           */
} rt_stats;

typedef struct rt_ctx rt_ctx;

/* ------------------------------------------------------------- life cycle */

const char* rt_last_error(void);
int rt_api_version(void);

/* One context per device ordinal.  Fails with RT_ERR_NO_DEVICE when there is no GPU. */
int rt_create(int device_ordinal, rt_ctx** out);
void rt_destroy(rt_ctx* ctx);

/* Launch on a caller-provided hipStream_t (e.g. a torch stream); NULL restores the context's own stream.
 * Everything the context enqueues from here on goes to that stream, and the entries that hand data to the host wait for it.
 * Order: work queued on the previous stream -- a pending batch and frames in flight are settled there first -- is ordered before
 * work queued on the new one: the new stream waits on the device for an event recorded at the end of the old one; the host does
 * not wait for it.  So an accumulation, the feature strips and the temporal history continue across the call (planes traced ahead and the
 * tiles' work order are dropped, as documented at rt_set_frame_lookahead).  The handle already in force changes no result.
 * The previous stream must still exist at the call: set another stream (or NULL) before destroying one the context was given.
 * A handle of 0 selects the context's own stream, which is created hipStreamNonBlocking: the legacy default stream -- the handle
 * of torch's default stream -- cannot be chosen, and work on it is not ordered with the context's.  Hand over a stream that was
 * created (torch.cuda.Stream()). */
int rt_set_stream(rt_ctx* ctx, void* hip_stream);

/* Upper bound for the per-sample workspace in bytes (default: min(64 GiB, half of the
 * device's free memory) — sized for 288 GB of HBM, so BASELINE configs 3 and 5 are one
 * pass on one GPU; env RT_WORKSPACE_GIB overrides).  A render whose W*rows*(s1-s0)*12 bytes
 * exceed it is split into sample-range passes that run back to back on the stream. */
int rt_set_workspace_limit(rt_ctx* ctx, uint64_t bytes);

/* ------------------------------------------------------------------ scene */

/* Replaces SpheresApp::InitScene's products (spheres-app.cpp:51-130): n spheres with
 * their materials, the camera (InitCamera, :35-49), the sun, the sky Emissive
 * material and exposureAdjustment = 2^m_exposure (:174). */
/* Limit: the clustered scan table (groups of four, padded) must stay below 65,536 entries
 * — about 65,000 spheres — because work lists, the shadow index and the closest-hit keys
 * carry entry ids in 16 bits; larger scenes are rejected here with RT_ERR_INVALID_ARG. */
/* Radii: any finite value.  r < 0 is the reference's hollow sphere (Sphere::Intersect tests r * r and divides the normal by
 * r, ray-tracing.cpp:48, :62, :75: the same surface as |r| with the normal turned inward) and r == 0 its degenerate point; both
 * render as the reference renders them.  Every acceleration table (group and leaf bounds, hierarchy, cell grid, shadow
 * index, per-tile tables) encloses |r|.  A centre or radius that is NaN or infinite is rejected with RT_ERR_INVALID_ARG
 * and a message naming the sphere: no bound can be built from it. */
/* lights: SpheresApp::m_lights (spheres-app.h:38, filled at spheres-app.cpp:129) as flat records, in list order -- the order
 * Material::Shade adds their contributions in (material.cpp:4-13); 0 <= n_lights <= RT_MAX_LIGHTS (lights may be NULL when
 * n_lights == 0: Shade then returns zero and no shadow ray is cast).  Every light answers its any-hit shadow query through
 * an exact footprint index of its own; a light below the horizon of a surface contributes nDotL = 0 exactly as in
 * the reference.  One light (the reference's scene) runs the single-light kernel path unchanged. */
/* materials and sky: inside the material domain (rt_material above).  Like a sphere that is not finite, a record outside it is
 * refused before any side effect: the previous scene and pending frames stay as they were. */
#define RT_MAX_LIGHTS 8
int rt_scene_upload(rt_ctx* ctx, const rt_sphere* spheres, const rt_material* materials, uint32_t n,
                    const rt_camera* camera, const rt_light* lights, uint32_t n_lights, const rt_material* sky,
                    float exposure_scale);

/* Moves the camera of the uploaded scene without an upload: no scene preparation, no table copied, no host wait of its own (the
 * only waits are those that rendering a pending batch implies).  Everything else on the device -- scene tables, lights, sky,
 * exposure -- stays.
 * Equivalence: after a successful rt_set_camera(ctx, C) everything the context computes is, bit for bit, what it computes after an
 * rt_scene_upload of the same spheres, materials, lights, sky and exposure with camera C: rt_render under every progressive mode
 * (HDR, LDR, moments, rt_stats' counters, the kernel variant of rt_unit_last_trace_launch), the per-tile masks and lists of the unit
 * entries, rt_render_features, the denoise family (picture, history, target) and the unit entries.
 * Voids exactly what the upload voids: the accumulation (the next rt_render must start at s0 == 1; one that continues is
 * RT_ERR_SEQUENCE), planes traced ahead, frames in flight under pipelining, every per-tile table (masks, sphere lists, work order,
 * empty-list flags and their count: all functions of the camera), the feature strips and the denoise snapshot.  A pending batch was
 * asked of the old camera and is rendered first; its errors surface here.
 * Keeps the sampler flags, the noise switch, the three progressive settings, the stream and the temporal history: the next temporal
 * call reprojects from the history's camera into C, as it does after an upload.
 * Same record: a record whose 14 floats that the renderer reads -- three components each of origin, x, y and origin_image_plane,
 * aperture, focal_length -- equal the current ones as bit patterns changes nothing and voids nothing (rt_set_sampler's precedent): a
 * running accumulation continues, a pending batch stays pending.  The fourth components are neither read nor compared.
 * Refused before any side effect: a null argument (RT_ERR_INVALID_ARG); no scene uploaded (RT_ERR_NO_SCENE); any of the 14 floats
 * not finite (RT_ERR_INVALID_ARG, the message names the field).  This is the one place where the two differ: rt_scene_upload keeps
 * accepting every camera record it accepted before, finite or not.  A refused call changes nothing. */
int rt_set_camera(rt_ctx* ctx, const rt_camera* camera);
/* The record of the last rt_scene_upload or (changing) rt_set_camera, all 72 bytes.  RT_ERR_NO_SCENE before any upload. */
int rt_get_camera(rt_ctx* ctx, rt_camera* out);

/* Shading edits: new materials and sky, new light colours and luminances, a new exposure for the uploaded scene, without an upload.
 * No scene preparation, no host wait of their own, no device memory allocated or freed.  Clustering, bounds, hierarchy, cell grid and
 * every shadow index are functions of the spheres and the light directions alone and stay as they are.
 * Equivalence: after a successful call everything the context computes is, bit for bit, what it computes after an rt_scene_upload of
 * the same spheres, camera and light directions with the new materials and sky, light colours and luminances, or exposure: rt_render
 * under every progressive mode (HDR, LDR, moments, rt_stats' counters, the kernel variant of rt_unit_last_trace_launch -- an edit after
 * which the materials pack into 16 bytes, or no longer do, takes the variant the upload takes), the per-tile unit entries,
 * rt_render_features and the denoise family (picture, history, target).
 * Void and keep: exactly what rt_set_camera voids and keeps -- the accumulation (a continuing rt_render is RT_ERR_SEQUENCE), planes
 * traced ahead, frames in flight, every per-tile table (the work order reads the material types, the constant sample of the empty-list
 * tiles reads sky and exposure), the feature strips and the denoise snapshot are void; a pending batch is rendered first, under the
 * old values, and its errors surface here; scene tables, camera, sampler flags, noise switch, progressive settings, stream and the
 * temporal history stay.  The history's validation never looks at colour: see rt_temporal_forget.
 * Same values: records equal to the current ones as bit patterns change nothing and void nothing (rt_set_camera's precedent).
 * Compared are all 48 bytes of every material record and of the sky's (the device tables hold the records whole), colour and
 * luminance of every light, the exposure.
 * Waits: the new tables travel through pinned memory the context owns, two sets used in turn; a call waits for the host only where
 * the copies of the edit before the previous one have not run yet.  rt_set_lights and rt_set_exposure never wait.
 * Refused before any side effect, a refused call changes nothing:
 *   - a null argument: RT_ERR_INVALID_ARG (lights may be NULL where n_lights == 0); no scene uploaded: RT_ERR_NO_SCENE;
 *   - rt_set_materials: n other than the uploaded sphere count; a record or the sky outside the material domain (rt_material above;
 *     the message names the sphere, or "the sky", and the field): RT_ERR_INVALID_ARG;
 *   - rt_set_lights: n_lights other than the uploaded count; a direction that differs as a bit pattern from the uploaded one -- the
 *     light's shadow index is built for its direction, a direction change needs an upload; a colour or luminance that is not finite:
 *     RT_ERR_INVALID_ARG;
 *   - rt_set_exposure: an exposure that is not finite: RT_ERR_INVALID_ARG.
 * Like rt_set_camera they are stricter than the upload in one place: rt_scene_upload keeps accepting light colours, luminances and
 * exposures that are not finite.
 * rt_set_lights and directions: a direction change goes through rt_turn_lights below.  After a turn, "the uploaded direction" above
 * reads "the direction set last": rt_set_lights compares with what rt_get_lights returns. */
int rt_set_materials(rt_ctx* ctx, const rt_material* materials, uint32_t n, const rt_material* sky);
int rt_set_lights(rt_ctx* ctx, const rt_light* lights, uint32_t n_lights);
int rt_set_exposure(rt_ctx* ctx, float exposure_scale);

/* Turns the lights of the uploaded scene without an upload: whole records, i.e. direction, colour and luminance of every light, as ONE
 * event (a sun that reddens while it sets is one call and one void per frame).  Of everything an upload prepares, a direction reaches
 * the shadow indices alone -- light 0's, one per further light, light 0's far tier -- and those are rebuilt on the host over the
 * layout kept from the upload, under the preparation options the upload used (the environment is not read again).  No clustering,
 * bounds, hierarchy or cell grid is built, no device memory allocated or freed, the stream is never synchronised.
 * Equivalence: after a successful call everything the context computes is, bit for bit, what it computes after an rt_scene_upload of
 * the same spheres, materials, camera, sky and exposure with the new lights: rt_render under every progressive mode (HDR, LDR, moments,
 * rt_stats' counters), the trace variant and LDS image of rt_unit_last_trace_launch -- they change with the index's size and with an
 * index switching on or off -- rt_unit_last_trace_far_state, rt_unit_shadow and rt_unit_shadow_tier, the per-tile unit entries,
 * rt_render_features and the denoise family with its history and target.
 * A finite direction that is no direction (length outside (0.5, 2)) is accepted, as the upload accepts it: that light gets no index
 * and its shadow rays take the scan; a later turn to a direction switches the index on again.
 * Void and keep: exactly what rt_set_camera voids and keeps; a pending batch is rendered first, under the old lights.  The temporal
 * history survives and its validation never looks at colour: after a turn EVERY shadow in it is stale.  The remedy is the caller's --
 * rt_temporal_reset, or rt_temporal_forget of what it knows moved.
 * Same values: records equal to the current ones as bit patterns -- direction, colour and luminance of every light -- are no event.
 * Waits: as rt_set_materials -- two staging sets in turn; the host waits only where the copies of the edit before the previous one
 * have not run yet.
 * Refused before any side effect, a refused call changes nothing: a null argument (lights may be NULL where n_lights == 0):
 * RT_ERR_INVALID_ARG; no scene uploaded: RT_ERR_NO_SCENE; n_lights other than the uploaded count: RT_ERR_INVALID_ARG; a direction
 * component, colour or luminance that is not finite: RT_ERR_INVALID_ARG (stricter than the upload, like the other setters). */
int rt_turn_lights(rt_ctx* ctx, const rt_light* lights, uint32_t n_lights);
/* The lights the context renders with now: the records of the last rt_scene_upload, rt_set_lights or rt_turn_lights that changed them.
 * *n_lights receives their count; with capacity == 0 nothing else is written (out may be NULL), else capacity must be at least the
 * count (RT_ERR_INVALID_ARG) and out[0 .. count) receives the records.  RT_ERR_NO_SCENE before any upload. */
int rt_get_lights(rt_ctx* ctx, rt_light* out, uint32_t capacity, uint32_t* n_lights);

/* ----------------------------------------------------------------- render */

/* Replaces GenerateRays + the for_each(par) trace loop for sample indices s in
 * [s0, s1) (1-based like m_sampleCount, spheres-app.cpp:168) over the rows in rs.
 * hdr[pixel] += GetHitColor(ray(i,j,s), 0) * exposure, added in increasing s
 * (spheres-app.cpp:182-183).  The HDR strip persists in the context: a call with
 * s0 == 1 (or after rt_clear) starts a new accumulation, a call whose s0 equals
 * the previous s1 continues it (progressive refinement, app.h:26 + spheres-app.h:42).
 * Material random draws come from a per-(pixel,s) xoshiro128** stream seeded from
 * (seed, global pixel id, s) — see DESIGN.md "RNG contract".  With out_stats == NULL the call only enqueues work
 * on the context's stream (no host wait); with out_stats it waits for the kernels to read their timers.
 * A call that fails part-way voids the accumulation: the next call must start again at s0 == 1. */
int rt_render(rt_ctx* ctx, uint32_t W, uint32_t H, rt_rowset rs, uint32_t s0, uint32_t s1,
              uint32_t max_depth, uint64_t seed, rt_stats* out_stats);

/* Sampler variants.  Default 0 = the reference's own mappings: HaltonSampleHemisphere is uniform
 * in solid angle (quasi-random.cpp:36-50: z = u1, r = sqrt(1 - u1^2); NOT cosine weighted, and the caller applies
 * no pdf) and HaltonSampleDisk takes r = u (quasi-random.cpp:52-61: NOT sqrt'ed, centre-weighted lens).  The flags
 * select the textbook mappings instead, with the same draws in the same order:
 *   RT_SAMPLER_COSINE_HEMISPHERE  r = sqrt(u1), z = sqrt(1 - u1), phi = 2 pi u2   (DielectricOpaque diffuse bounce)
 *   RT_SAMPLER_SQRT_DISK          r = sqrt(u)                                     (lens offsets, GenerateRays :152)
 * Takes effect at the next accumulation (rt_render with s0 == 1); changing it voids a running one. */
#define RT_SAMPLER_COSINE_HEMISPHERE 1u
#define RT_SAMPLER_SQRT_DISK 2u
int rt_set_sampler(rt_ctx* ctx, uint32_t flags);

/* Frame pipelining for progressive use — the reference's only mode: OnRender adds ONE sample per pixel per frame
 * (spheres-app.cpp:163-184, app.cpp:56-76).  A 1-spp frame is 0.13 ms of work followed by the tail of its few 51-segment
 * paths.  With depth > 0, an rt_render call that passes out_stats == NULL returns with up to `depth` of the newest calls'
 * sample planes still in flight: its kernel ends when nothing is left to start and carries the unfinished paths into the
 * next call's kernel.  Planes are added to the HDR strip strictly in sample order as they complete, so after a flush the
 * strip equals the one-shot render bit for bit.  While frames are in flight rt_resolve(ctx, 0) divides by the number of
 * samples actually in the strip (rt_committed_samples), and rt_download / rt_copy_to_device hand out that strip.
 * rt_synchronize, a call with statistics and rt_set_frame_pipelining itself settle everything first.  depth 0 = off.
 * SCOPE: the carrying kernel exists for scenes whose tables fit LDS with the matrix-core filter (up to 128 groups of four
 * spheres, i.e. about 500 spheres: the reference's cover scene and everything smaller).  Larger scenes -- the cell-grid and
 * bounds-hierarchy scans (10,000-sphere class) -- and contexts created under non-default launch knobs render every call
 * UNPIPELINED: same results, each call runs its own paths to their end before the next one starts. */
int rt_set_frame_pipelining(rt_ctx* ctx, uint32_t depth);
/* Frame batching for progressive use: a 1-spp frame is less work than the three launches it takes.  With frames > 1, rt_render
 * calls that pass out_stats == NULL and continue each other (same image, row set, depth and seed; s0 == the previous s1) are
 * only RECORDED until `frames` sample planes are pending; then ONE launch renders them all, and the planes are added to the
 * HDR strip in sample order as always -- the strip equals what the separate calls would have produced, bit for bit.  Until
 * then rt_resolve / rt_download / rt_copy_to_device hand out the samples committed so far (rt_committed_samples; when nothing
 * is committed yet they render the pending frames first).  rt_synchronize, a call with statistics, a call that does not
 * continue the batch, rt_scene_upload, rt_set_stream and rt_set_frame_batch itself render what is pending first; errors of
 * deferred calls surface there.  Not combined with rt_set_frame_pipelining (depth > 0 takes precedence).  frames == 1: off. */
int rt_set_frame_batch(rt_ctx* ctx, uint32_t frames);
/* Render-AHEAD for progressive use (round 4): with frames > 1, an rt_render call that passes out_stats == NULL traces, with its ONE
 * launch, its own sample planes AND the planes of the next calls (`frames` planes in all), but adds only its own to the HDR strip;
 * the calls that continue it (same image, row set, depth and seed; s0 == the previous s1) find their planes traced and only add
 * them, in sample order -- one small kernel.  The strip always holds EXACTLY the samples of the calls made (display lag 0: what
 * rt_resolve / rt_download hand out after call f is the one-shot render of samples 1..f, bit for bit), the launch and its tail are
 * paid once per `frames` calls, and the first call of each group takes the group's time.  A call that does not continue, a call
 * with statistics, rt_scene_upload, rt_clear, rt_set_stream drop what was traced ahead (nothing of it ever reached the strip).
 * Why not one frame per launch at full rate: a path is up to 51 dependent scans of ~10 us, five 1200x800 1-spp frames' worth of
 * bulk-rate work, so a frame's last sample cannot exist before ~5 later frames have been started (interactive mode).
 * Takes precedence below rt_set_frame_batch and rt_set_frame_pipelining (either of them on: ignored).  frames == 1: off. */
int rt_set_frame_lookahead(rt_ctx* ctx, uint32_t frames);
/* Samples per pixel in the HDR strip right now (waits for the stream). */
int rt_committed_samples(rt_ctx* ctx, uint32_t* out);

/* Forget the accumulated HDR strip and sample count (and, with rt_set_noise_estimate on, the strip of second moments). */
int rt_clear(rt_ctx* ctx);

/* ---------------------------------------------------------- noise estimate
 * How converged is a pixel?  With the switch on, an accumulation keeps, next to the HDR strip, a strip sq of W*local_rows*3
 * floats: for every sample plane added to hdr, in the same increasing-s order and for c in r, g, b,
 *     sq[c] = sq[c] + (v[c] * v[c])      -- the product rounded to binary32 first, the add second, never fused.
 * The HDR strip has the same bits with the switch on or off; off, exactly the kernels of before are launched.  Like rt_set_sampler
 * the switch takes effect at the next accumulation (rt_render with s0 == 1) and changing it voids a running one; default off.
 * rt_clear, a failed pass and rt_scene_upload void sq together with hdr.  Frame batching and render-ahead keep sq in step with hdr.
 * FRAME PIPELINING WITH THE SWITCH ON RENDERS EVERY CALL UNPIPELINED (same results; the fallback large scenes already take): the
 * carrying kernel's commit adds no second moments.  Moments are per context: a multi-GPU gather of sq is the caller's, and
 * rt_copy_moments_to_device is what feeds it (rt_denoise_shards below filters the gathered parts). */
int rt_set_noise_estimate(rt_ctx* ctx, int on);
/* Copy sq to host: W*local_rows*3 floats.  RT_ERR_SEQUENCE when the switch is off or nothing is accumulated. */
int rt_download_moments(rt_ctx* ctx, float* sq_rgb);
/* Same, device to device into caller-owned device memory (the buffer a gather of the shards sends).  Asynchronous on the context's
 * stream; pending batches are settled and the errors are as for rt_download_moments. */
int rt_copy_moments_to_device(rt_ctx* ctx, void* dev_sq);
/* Per-pixel standard error of the accumulated MEAN after n = the samples in the strip (n >= 2, else RT_ERR_SEQUENCE; also when the
 * switch is off or nothing is accumulated).  binary64, only + - * / and comparisons, in this order (DESIGN.md "Noise estimate"):
 *     for c in r,g,b:  S = (double)hdr[c];  Q = (double)sq[c];  mean_c = S / n
 *                      var_c = (Q - S * mean_c) / (n - 1);   if !(var_c > 0) var_c = 0
 *     V = (var_r + var_g) + var_b;   M = (mean_r + mean_g) + mean_b;   abs2 = V / n;   d = M + (double)floor
 *     out[0] = sqrt32((float)abs2)               standard error of the pixel mean, HDR units, channels summed
 *     out[1] = sqrt32((float)(abs2 / (d * d)))   the same, relative to the pixel's brightness (floor keeps dark pixels finite)
 * sqrt32 = the correctly rounded binary32 square root (rt_unit_math op 7).  out_abs_rel: 2 floats per pixel, host memory.  A pixel
 * with M + floor == 0 gets a non-finite out[1] and is reported so (a NaN's sign and payload are unspecified).  Pending batches are
 * settled as rt_resolve settles them; planes traced ahead are not in the strips. */
int rt_noise_map(rt_ctx* ctx, float floor, float* out_abs_rel);
/* Order-independent summary of that map's relative error: out_counts[k] = pixels with rel > thresholds[k] (n_thr <= 8; a non-finite
 * rel counts as above every threshold), *out_max_rel = the largest finite rel (0 when there is none; may be NULL).  Reduced on the
 * device with integer atomics only, so repeated calls give identical answers.  Same sequencing as rt_noise_map. */
int rt_noise_summary(rt_ctx* ctx, float floor, const float* thresholds, uint32_t n_thr, uint32_t* out_counts, float* out_max_rel);

/* --------------------------------------------------------- feature buffers
 * First-hit albedo, normal, depth, coverage and object id (DESIGN.md "Feature buffers"; csrc/rt_features.h): what denoisers, edge-aware
 * filters, compositing and picking take beside the colour.  For a pixel (i, j) and a sample index s the ray is exactly the path's
 * primary ray (GenerateRays + Camera::GetRay with the context's sampler flags: RT_SAMPLER_SQRT_DISK moves the lens offsets here too)
 * and the hit is the contract's closest hit (the list scan's result).  The sample's feature vector v[8] and id:
 *     hit, OPAQUE / METAL / EMISSIVE  v[0..2] = Texture::Evaluate(uv) of the material's texture, uv = (0.5 n.x + 0.5, 0.5 n.z + 0.5)
 *     hit, TRANSPARENT                v[0..2] = (1, 1, 1)
 *         either way                  v[3..5] = the hit normal (pos - c) / r (signed r, as the path uses it), v[6] = t, v[7] = 1,
 *                                     id = the sphere's index in the uploaded list
 *     miss                            v[0..2] = the sky material's texture at uv (0, 0) (Emit(Payload{})'s colour without the luminance),
 *                                     v[3..7] = 0, id = 0xffffffff
 * The context keeps a strip feat[pixel][8] of binary32 sums, feat[c] = feat[c] + v[c] added in increasing s, and id[pixel], the id of
 * the sample added last; pixels are the local pixels of the row set, in the order of the HDR strip.
 * Sequencing mirrors rt_render but is INDEPENDENT of the HDR accumulation: a call with s0 == 1, or the first call after
 * rt_clear_features, starts an accumulation; a call with s0 == the previous s1 and the same W, H and row set continues it (same bits
 * as one call over the whole range); anything else is RT_ERR_SEQUENCE.  rt_scene_upload voids the strips, and so does an
 * rt_set_sampler that changes the flags.  rt_clear, rt_render, rt_resolve and the three progressive switches neither read nor change
 * them, and the feature calls leave everything rt_render relies on untouched (they keep ray-generation tables of their own).
 * With out_ms == NULL the call only enqueues work on the context's stream; else it waits and returns the HIP-event time. */
int rt_render_features(rt_ctx* ctx, uint32_t W, uint32_t H, rt_rowset rs, uint32_t s0, uint32_t s1, double* out_ms);
/* Samples per pixel in the feature strips (0: nothing accumulated). */
int rt_feature_samples(rt_ctx* ctx, uint32_t* out);
/* Copy the raw sums to host.  feat8: W*local_rows*8 floats; ids: W*local_rows values.  Either pointer may be NULL.
 * RT_ERR_SEQUENCE when nothing is accumulated. */
int rt_download_features(rt_ctx* ctx, float* feat8, uint32_t* ids);
/* Same, device to device into caller-owned device memory.  Asynchronous on the context's stream. */
int rt_copy_features_to_device(rt_ctx* ctx, void* dev_feat8, void* dev_ids);
/* Forget the feature strips; the next rt_render_features starts an accumulation at any s0. */
int rt_clear_features(rt_ctx* ctx);

/* ----------------------------------------------------------------- denoise
 * Feature-guided edge-avoiding a-trous filter of the accumulated picture (DESIGN.md "Denoise"; csrc/rt_denoise.h): the consumer of the
 * noise estimate and of the feature buffers.  Everything is binary32, only + - * / and comparisons in exactly this order and
 * association, never fused; division is the correctly rounded one; the one square root is the noise estimate's.
 * Inputs: hdr, sq after n >= 2 samples; feat after m >= 1 samples; W x rows the strip of a CONTIGUOUS row set (nshards == 1: the
 * local rows of a cyclic row set are not neighbours in the image).  Per pixel p:
 *     c0[k] = hdr[k] / (float)n   k = r, g, b       sigma = rt_noise_map's out[0] with floor = 0;  v0 = sigma * sigma
 *     g[k]  = feat[k] / (float)m  k = 0..7 (albedo 3, normal 3, depth, coverage)
 * Level l = 0 .. levels-1, step = 1 << l: taps a = 0..4 outer (dy = (a-2) step), b = 0..4 inner (dx = (b-2) step), h = {1/16, 1/4,
 * 3/8, 1/4, 1/16}; a tap outside the strip is skipped (adds nothing, takes no slot); the sums start at +0; for tap q of pixel p
 *     dn = gp[3..5]-gq[3..5];  xn = k_normal   * ((dn0*dn0 + dn1*dn1) + dn2*dn2)
 *     da = gp[0..2]-gq[0..2];  xa = k_albedo   * ((da0*da0 + da1*da1) + da2*da2)
 *     dz = gp[6]-gq[6];  zm = max(gp[6], gq[6]);   xz = k_depth * ((dz*dz) / (zm*zm + 1e-12f))
 *     dc = gp[7]-gq[7];        xc = k_coverage * (dc*dc)
 *     dl = cp - cq;            xl = k_colour   * (((dl0*dl0 + dl1*dl1) + dl2*dl2) / ((vp + vq) + var_floor))
 *     x  = (((xn + xz) + xa) + xc) + xl;       ww = (h[a]*h[b]) / (1.0f + x)
 *     sc[k] = sc[k] + ww*cq[k];    sv = sv + (ww*ww)*vq;    sw = sw + ww
 * and after the 25 taps c'[k] = sc[k] / sw, v' = sv / (sw*sw) (the centre tap makes sw > 0).  c, v at every tap of a level are the
 * previous level's (two buffers, never in place); the guides never change.  Output: den[p][3] = c and den_var[p] = v after the last
 * level -- means, not sums.  Pixels whose inputs are all finite are covered; a NaN's sign and payload are not. */
typedef struct rt_denoise_params {
    uint32_t levels;                                           /* 1..5; default 3                                      */
    float k_normal, k_depth, k_albedo, k_coverage, k_colour;   /* defaults 16, 400, 64, 16, 1; each finite and >= 0    */
    float var_floor;                                           /* default 1e-6f; finite and > 0                        */
} rt_denoise_params;
int rt_denoise_default_params(rt_denoise_params* out);  /* needs no GPU */
/* Filters the strips as they are now into strips of the denoiser's own, and tonemaps the result (the resolve with n_samples = 1) into
 * an LDR buffer of its own.  params == NULL: the defaults; parameters outside their domain: RT_ERR_INVALID_ARG.  Needs the noise
 * estimate on and n >= 2 samples accumulated (pending batches are settled as rt_noise_map settles them; planes traced ahead are not in
 * the strips), and feature strips with at least one sample of the same W, H and row set as the picture: else RT_ERR_SEQUENCE.  A row set
 * with nshards != 1 is RT_ERR_INVALID_ARG (gather the shards and call rt_denoise_shards).  Reads hdr, sq and feat; changes none of them, nor ldr, nor any sequencing state: a render
 * that continues afterwards ends on the bits it would have had.  The result is a snapshot that stays until the next rt_denoise or
 * rt_scene_upload.  With out_ms == NULL the call only enqueues work on the context's stream; else it waits and returns the HIP-event
 * time.  env RT_DENOISE_STAGE, read per call: 0 = no level stages its taps in LDS, 1 = every level whose tile and halo fit does (same
 * bits either way; unset: the measured cut). */
int rt_denoise(rt_ctx* ctx, const rt_denoise_params* params, double* out_ms);
/* Copy the result to host.  rgb: W*rows*3 floats; var: W*rows floats; ldr: W*rows*3 bytes.  Any pointer may be NULL.
 * RT_ERR_SEQUENCE before any rt_denoise (or after rt_scene_upload voided it). */
int rt_download_denoised(rt_ctx* ctx, float* rgb, float* var, uint8_t* ldr);
/* Same, device to device into caller-owned device memory.  Asynchronous on the context's stream. */
int rt_copy_denoised_to_device(rt_ctx* ctx, void* dev_rgb, void* dev_var, void* dev_ldr);
/* The same filter over a picture that was rendered in row shards (rt_rowset with nshards > 1, e.g. one shard per GPU) and gathered
 * onto this context's device: part s holds shard s's hdr, sq and feat strips, each part padded to rows_max rows, the parts back to
 * back -- the layout an equal-count gather of the shards' strips leaves.  Row j of the W x rs.num_rows image (j counted from
 * rs.first_row) is local row lr of part s with (s, lr) = rt_rowset_locate(rs, j); the rows lr >= local_rows(s) of a part are the
 * gather's padding and are never read. */
typedef struct rt_shard_parts {
    const void* hdr;   /* device: [nshards][rows_max * W * 3] float32 sums, as the equal-count gather leaves them */
    const void* sq;    /* device: same shape                                                                    */
    const void* feat;  /* device: [nshards][rows_max * W * 8] float32 sums; 16-byte aligned                     */
    uint32_t W, rows_max;
    rt_rowset rs;      /* first_row, num_rows, block_rows, nshards of the sharding; rs.shard ignored            */
    uint32_t n, m;     /* samples in hdr / sq (>= 2), samples in feat (>= 1)                                    */
} rt_shard_parts;
/* Filters that image into the context's own denoise strips, in image order, and tonemaps it: rt_download_denoised,
 * rt_copy_denoised_to_device and rt_unit_denoise_forms then serve the result exactly as after rt_denoise.  The arithmetic, the
 * parameters (NULL: the defaults), RT_DENOISE_STAGE, out_ms and the snapshot's lifetime are rt_denoise's: the result has the bits
 * rt_denoise gives in one context that rendered the whole image.  The parts are read by a prepare pass of their own, which looks every
 * row up through the mapping; no assembled copy of the inputs is made.  Needs no scene and no accumulation in ctx, and reads and
 * changes nothing of the context's render, noise or feature state.  A null pointer; W, rs.num_rows, rs.nshards or rs.block_rows of 0
 * (or an image beyond 2^31 pixels or 524,280 rows); rows_max below the largest shard's rows; feat not 16-byte aligned; parameters
 * outside their domain: RT_ERR_INVALID_ARG.  n < 2 or m == 0: RT_ERR_SEQUENCE.  A refused call keeps the previous snapshot. */
int rt_denoise_shards(rt_ctx* ctx, const rt_shard_parts* parts, const rt_denoise_params* params, double* out_ms);

/* ----------------------------------------------------------------- temporal accumulation
 * The temporal half of the denoiser (DESIGN.md "Temporal accumulation"; csrc/rt_temporal.h): the prepare pass's state (c.rgb, v) of the
 * previous call -- the HISTORY -- is reprojected into the current camera, validated against the guides and blended into this call's
 * state before the levels run.  Binary32 only, + - * / and comparisons in exactly this order, never fused, correctly rounded division
 * and square root (sqrt_rn), dot(a, b) = (a0*b0 + a1*b1) + a2*b2.  For pixel (x, y) of the image (y = rs.first_row + local row), with
 * c, v, g as rt_denoise prepares them, id the feature strips' id, C the current camera, C' the history's, w = C.origin_image_plane -
 * C.origin (w' likewise), and ch, vh, gh, idh, lenh the history's pixel:
 *     u = ((float)x + 0.5f) / (float)W;   vv = ((float)y + 0.5f) / (float)H;   nx = 2.f*u - 1.f;   ny = -2.f*vv + 1.f
 *     d[k] = (w[k] + nx*C.x[k]) + ny*C.y[k];      cov = g[7]
 *     cov > 0:  z = g[6] / cov;  s = z / sqrt_rn(dot(d,d));  P[k] = C.origin[k] + s*d[k];  q[k] = P[k] - C'.origin[k];
 *               dist = sqrt_rn(dot(q,q))          else: q = d (the sky is reprojected by its direction)
 *     zw = dot(q,w') / dot(w',w');                                                       reject unless zw > 0
 *     px = (dot(q,C'.x) / dot(C'.x,C'.x)) / zw;   py = (dot(q,C'.y) / dot(C'.y,C'.y)) / zw
 *     fx = ((px + 1.f) * 0.5f) * (float)W;        fy = ((1.f - py) * 0.5f) * (float)H
 *     reject unless 0 <= fx < W and first_row <= fy < first_row + num_rows;   xi = (uint32)fx;  yi = (uint32)fy
 * The history's pixel is the one at (xi, yi) -- nearest pixel, no interpolation.  The pixel is accepted when all of these hold:
 *     lenh >= 1;   id == idh (with use_id);   |cov - gh[7]| <= coverage_tol;   dn = g[3..5] - gh[3..5], dot(dn,dn) <= normal_tol;
 *     cov > 0:  gh[7] > 0, and with zh = gh[6]/gh[7], dz = dist - zh, zm = max(dist, zh):  dz*dz <= (depth_tol*depth_tol) * (zm*zm)
 *     cov == 0: gh[7] == 0
 * Accepted: L = (float)min(lenh, max_history - 1), a = 1.f / (L + 1.f), c'[k] = a*c[k] + (1.f - a)*ch[k],
 * v' = (a*a)*v + ((1.f - a)*(1.f - a))*vh, len' = min(lenh, max_history - 1) + 1, target = (yi - first_row)*W + xi.
 * Rejected (a NaN in any test rejects): c' = c, v' = v, len' = 1, target = 0xffffffff.  (c', v') is the input of level 0 and, with g, id
 * and len', the new history; C becomes the history's camera. */
typedef struct rt_temporal_params {
    uint32_t max_history;   /* 1..64, default 2; 1 = never blend                 */
    uint32_t use_id;        /* default 1                                          */
    float depth_tol;        /* default 0.1f;  finite, >= 0                        */
    float normal_tol;       /* default 0.1f;  finite, >= 0                        */
    float coverage_tol;     /* default 0.25f; finite, >= 0                        */
} rt_temporal_params;
int rt_temporal_default_params(rt_temporal_params* out);  /* needs no GPU */
/* rt_denoise with the temporal step in its prepare pass.  Preconditions, refusals, params, out_ms, RT_DENOISE_STAGE and the snapshot
 * (rt_download_denoised, rt_copy_denoised_to_device, rt_unit_denoise_forms) are rt_denoise's; tparams == NULL: the defaults, outside
 * their domain: RT_ERR_INVALID_ARG; so is a picture wider or taller than 2^24.  The current camera is rt_get_camera's.  Changes
 * none of hdr, sq, feat, the ids or ldr, nor any sequencing state.  The history is state of its own: it survives rt_set_camera (a
 * camera move) and rt_scene_upload (keeping object ids stable across uploads is the caller's business, use_id = 0 otherwise), is dropped by
 * rt_temporal_reset and rt_destroy, and a call whose W, H or row set differ from the history's starts from an empty one -- on an
 * empty history the call gives rt_denoise's bits.  A refused call keeps history and snapshot.  rt_denoise and rt_denoise_shards
 * neither read nor change the history. */
int rt_denoise_temporal(rt_ctx* ctx, const rt_denoise_params* params, const rt_temporal_params* tparams, double* out_ms);
int rt_temporal_reset(rt_ctx* ctx);
/* The history as the last rt_denoise_temporal left it: state4 = W*rows*4 floats (c'.rgb, v'), len and target = W*rows words each.  Any
 * pointer may be NULL.  RT_ERR_SEQUENCE while the history is empty. */
int rt_download_temporal(rt_ctx* ctx, float* state4, uint32_t* len, uint32_t* target);
/* Forget what the history knows about some objects: every pixel of the current history whose stored id is one of ids[0 .. n_ids) gets
 * len = 0, so that the next temporal call of either fetch, contiguous or sharded, treats it exactly as a pixel with no history (the
 * nearest fetch's length test fails, a bilinear tap does not take part): len' = 1, target 0xffffffff, the state the frame's own.  What a
 * caller does after recolouring a sphere (rt_set_materials), since the history's validation tests id, depth, normal and coverage,
 * never colour.  0xffffffff names the sky; ids at or above the sphere count (without a scene: at or above 65536) are accepted and
 * match nothing.  Everything else of the history -- state, guides, ids, other pixels' len, its camera -- is untouched.
 * Stream-ordered, no host wait (more than 16 ids travel as a table through the edits' pinned memory, with its rule).  n_ids == 0 or an
 * empty history: RT_OK, nothing happens.  A null context, or null ids with n_ids > 0: RT_ERR_INVALID_ARG.  Needs no scene. */
int rt_temporal_forget(rt_ctx* ctx, const uint32_t* ids, uint32_t n_ids);
/* The way the history is fetched, chosen per call.  RT_TEMPORAL_FETCH_NEAREST is everything above.  RT_TEMPORAL_FETCH_BILINEAR reads
 * the four pixels whose centres surround the reprojected point, so that a sample k calls old is not up to k/2 pixels off.  For a point
 * the reprojection accepts (fx, fy, xi, yi, dist as above), in the same arithmetic:
 *   rx = fx - (float)xi (exact);  rx >= 0.5f: x0 = xi, tx = rx - 0.5f;  else: x0 = xi - 1 (may be -1), tx = rx + 0.5f;  ry, y0, ty likewise
 *   taps in the order (i, j) = (0,0) (1,0) (0,1) (1,1):  qx = x0 + i, qy = y0 + j,  w = (i ? tx : 1.f - tx) * (j ? ty : 1.f - ty)
 *   a tap takes part iff 0 <= qx < W, first_row <= qy < first_row + num_rows, w > 0.f and it passes the validation above (the current
 *   pixel against the history's pixel q, with the same dist) -- a tap that does not is never added, so an Inf or NaN there reaches nothing:
 *     sc[k] = sc[k] + w*ch(q)[k];  sv = sv + (w*w)*vh(q);  sw = sw + w;  lmin = min(lmin, lenh(q))        (sums start at +0)
 *   accepted iff sw > 0.f: ch[k] = sc[k]/sw, vh = sv/(sw*sw) (the filter's own rule for a weighted mean's variance), lenh = lmin, and the
 *   blend above; target = the index of the participating tap of the greatest w, the first in tap order on a tie.  Rejected: as above.
 * The history is the same state whichever fetch wrote it: calls may alternate. */
enum { RT_TEMPORAL_FETCH_NEAREST = 1, RT_TEMPORAL_FETCH_BILINEAR = 4 };
/* rt_temporal_default_params for a fetch: 1 gives its values, 4 the same tolerances with max_history = 3 (docs/EXPERIMENTS.md: the
 * best row of the fetch x max_history grid).  Any other fetch: RT_ERR_INVALID_ARG.  Needs no GPU. */
int rt_temporal_default_params_fetch(uint32_t fetch, rt_temporal_params* out);
/* rt_denoise_temporal with the fetch chosen: its preconditions, refusals, snapshot and history lifetime, every refusal before the first
 * change.  tparams == NULL: that fetch's defaults.  fetch neither 1 nor 4: RT_ERR_INVALID_ARG.  Fetch 1 gives rt_denoise_temporal's bits. */
int rt_denoise_temporal_fetch(rt_ctx* ctx, const rt_denoise_params* params, const rt_temporal_params* tparams, uint32_t fetch, double* out_ms);
/* Temporal accumulation for a picture that was rendered in row shards and gathered onto this context's device (rt_denoise_shards
 * above): the gathered parts, the shards' feature ids in the same layout, and what the reprojection needs of the picture they are rows
 * of -- the image's height and the camera the shards were rendered with (every shard renders with the same one). */
typedef struct rt_shard_frame {
    rt_shard_parts parts;   /* as rt_denoise_shards reads it */
    const void* ids;        /* device: [nshards][rows_max * W] uint32, the shards' feature ids, padded like the other parts */
    uint32_t H;             /* height of the whole image; parts.rs.first_row + parts.rs.num_rows <= H */
    rt_camera camera;       /* the camera the shards were rendered with */
} rt_shard_frame;
/* rt_denoise_temporal_fetch over the parts: den, den_var, the LDR, the new history (state, guides, ids, len) and target have the bits
 * rt_denoise_temporal_fetch gives in one context that rendered rows [first_row, first_row + num_rows) of the W x H image contiguously
 * with that camera; target counts in image order, (yi - first_row)*W + xi.  The prepare pass reads the current frame through the row
 * mapping (rt_rowset_locate) and reads and writes the history in image order; the padding rows are never read, and no assembled copy
 * of the inputs is made.  Like rt_denoise_shards the call needs no scene and no accumulation in ctx and reads and changes nothing of
 * the context's render, noise or feature state.
 * The history is the context's one history, with rt_denoise_temporal's lifetime (it survives rt_scene_upload; rt_temporal_reset and
 * rt_destroy drop it); rt_download_temporal, rt_download_denoised, rt_copy_denoised_to_device and rt_unit_denoise_forms serve the call
 * as they serve rt_denoise_temporal_fetch.  Its picture is W, H and parts.rs with shard = 0, compared field by field with the
 * history's: a call with nshards = 1 whose W, H, first_row, num_rows and block_rows are a contiguous call's continues that call's
 * history, and the reverse (the whole image is {0, H, H, 0, 1}); any other difference -- another sharding of the same rows too --
 * starts from an empty history, on which the result has rt_denoise_shards' bits.  The fetches may alternate.
 * Refused with RT_ERR_INVALID_ARG: everything rt_denoise_shards refuses so; ids null or not 4-byte aligned; H < first_row + num_rows;
 * W or H above 2^24; fetch neither 1 nor 4; tparams outside their domain (NULL: that fetch's defaults); a camera whose origin, x, y,
 * origin_image_plane (three components each), aperture or focal_length is not finite.  n < 2 or m == 0: RT_ERR_SEQUENCE.  Every refusal
 * comes before the first change: a refused call keeps history and snapshot. */
int rt_denoise_shards_temporal(rt_ctx* ctx, const rt_shard_frame* frame, const rt_denoise_params* params, const rt_temporal_params* tparams,
                               uint32_t fetch, double* out_ms);

/* ----------------------------------------------------------------- spatial variance estimate
 * Where the filter's v0 comes from, chosen per call (csrc/rt_denoise.h).  RT_VARIANCE_MOMENTS is everything above: the
 * strip of second moments, which needs rt_set_noise_estimate(1) and n >= 2.  RT_VARIANCE_SPATIAL takes v0 from the picture itself -- the
 * guide-weighted variance of c0 over the (2R+1)^2 window around the pixel -- and so runs at ONE sample per pixel, with the noise switch
 * off and with frames in flight.  The arithmetic rules are the denoiser's (binary32; only + - * / and comparisons in this order and
 * association; never fused; correctly rounded division).  c0[k] = hdr[k] / (float)n and g = feat / (float)m as above; sq is not read.
 * For pixel p, R = radius: taps a = 0..2R outer (dy = a - R), b = 0..2R inner (dx = b - R), the centre included; a tap outside the strip
 * is skipped (adds nothing, never clamped); the sums start at +0; for tap q
 *     xn, xa, xz, xc   the four guide terms of the filter's tap above (same expressions, the call's k_normal, k_albedo, k_depth, k_coverage)
 *     x  = ((xn + xz) + xa) + xc;            w = 1.0f / (1.0f + x)
 *     s1[k] = s1[k] + w*cq[k];   s2[k] = s2[k] + w*(cq[k]*cq[k]);   sw = sw + w        k = r, g, b
 * and after the taps mu[k] = s1[k]/sw; e[k] = s2[k]/sw; d[k] = e[k] - mu[k]*mu[k]; if !(d[k] > 0) d[k] = 0;  v0 = (d[0] + d[1]) + d[2]
 * (the centre has w = 1, so sw >= 1).  The pixel's state is (c0, v0); from there everything is unchanged: the temporal validation and
 * blend, the levels and den_var, the tonemap, the snapshot and its readers, RT_DENOISE_STAGE, rt_unit_denoise_forms, and the history's
 * layout, key and lifetime.  Calls may alternate sources and fetches over one history.  Pixels whose inputs are all finite are covered; a
 * NaN's sign and payload are not. */
enum { RT_VARIANCE_MOMENTS = 0, RT_VARIANCE_SPATIAL = 1 };
typedef struct rt_variance_params {
    uint32_t source;   /* default RT_VARIANCE_MOMENTS */
    uint32_t radius;   /* 1..3, window (2R+1)^2, default 1 (docs/EXPERIMENTS.md: the grid); read only under RT_VARIANCE_SPATIAL */
} rt_variance_params;
int rt_variance_default_params(rt_variance_params* out);   /* needs no GPU */
/* rt_denoise and rt_denoise_temporal_fetch with the variance source chosen.  vparams == NULL or source == RT_VARIANCE_MOMENTS: exactly
 * those two entries -- preconditions, refusals, bits and history.  Under RT_VARIANCE_SPATIAL: a picture accumulated with n >= 1 samples
 * in the strip, n being the count rt_resolve(ctx, 0) and rt_download see (pending batches are settled as they settle them; planes traced
 * ahead are not in the strip; with frames in flight it is rt_committed_samples, read on the device); nothing accumulated is
 * RT_ERR_SEQUENCE.  The noise switch may be off, and the call settles nothing that rt_resolve would not: pipelined frames stay in flight.
 * Feature strips, the nshards rule and the row limits are rt_denoise's.  radius outside 1..3 under SPATIAL, or an unknown source:
 * RT_ERR_INVALID_ARG.  Every refusal comes before the first change: history and snapshot stay.  The sharded entries (rt_denoise_shards,
 * rt_denoise_shards_temporal) are unchanged; their forms with the source chosen follow. */
int rt_denoise_variance(rt_ctx* ctx, const rt_denoise_params* params, const rt_variance_params* vparams, double* out_ms);
int rt_denoise_temporal_variance(rt_ctx* ctx, const rt_denoise_params* params, const rt_temporal_params* tparams, uint32_t fetch,
                                 const rt_variance_params* vparams, double* out_ms);
/* rt_denoise_shards and rt_denoise_shards_temporal with the variance source chosen: a picture rendered in row shards at ONE sample per
 * pixel, gathered, filtered and accumulated on one device.  vparams is checked first.  vparams == NULL or source == RT_VARIANCE_MOMENTS:
 * exactly those two entries -- preconditions, refusals, messages, bits and history.  Under RT_VARIANCE_SPATIAL parts->sq is not
 * inspected and may be NULL (the gather need not carry the second moments: 11 words per pixel, 12 with ids, instead of 14 or 15), and
 * parts->n >= 1 suffices (n == 0: RT_ERR_SEQUENCE); m, the shape, alignment, row limits, camera, fetch and tparams rules are those of the
 * two entries; a radius outside 1..3 or an unknown source is RT_ERR_INVALID_ARG.  Every refusal comes before the first change: history
 * and snapshot stay.  The spatial pass reads hdr and feat of image pixel (x, y) through the row mapping; its window is the IMAGE's, so it
 * crosses shard and block boundaries as if there were none, and a part's padding rows are never read.  Bits: those of
 * rt_denoise_variance / rt_denoise_temporal_variance in one context that rendered rows [first_row, first_row + num_rows) of the W x H
 * image contiguously with that camera -- den, den_var, LDR, the new history (state, guides, ids, len) and target.  The history is the
 * context's one history with rt_denoise_shards_temporal's key and lifetime: nshards == 1 with a contiguous call's rows continues that
 * call's history and the reverse, and sources and fetches may alternate over it.  The snapshot's readers, RT_DENOISE_STAGE,
 * rt_unit_denoise_forms and out_ms are unchanged.  Like the entries above the calls need no scene and no accumulation in ctx, and touch
 * nothing of its render, noise or feature state. */
int rt_denoise_shards_variance(rt_ctx* ctx, const rt_shard_parts* parts, const rt_denoise_params* params, const rt_variance_params* vparams,
                               double* out_ms);
int rt_denoise_shards_temporal_variance(rt_ctx* ctx, const rt_shard_frame* frame, const rt_denoise_params* params, const rt_temporal_params* tparams,
                                        uint32_t fetch, const rt_variance_params* vparams, double* out_ms);

/* Replaces the transform(par) tonemap (spheres-app.cpp:186-214): hdr / n_samples,
 * ACES fit, gamma 1/2.2, XMStoreColor.  n_samples == 0 uses the accumulated count. */
int rt_resolve(rt_ctx* ctx, uint32_t n_samples);
/* HIP-event time of the last rt_resolve kernel, milliseconds. */
double rt_last_resolve_ms(rt_ctx* ctx);

/* Copy the strip to host.  hdr_rgb: W*local_rows*3 floats; ldr_rgb: W*local_rows*3
 * bytes (R,G,B of the XMCOLOR).  Either pointer may be NULL. */
int rt_download(rt_ctx* ctx, float* hdr_rgb, uint8_t* ldr_rgb);

/* Same, device to device into caller-owned device memory (e.g. a torch tensor that
 * feeds the RCCL gather).  Asynchronous on the context's stream. */
int rt_copy_to_device(rt_ctx* ctx, void* dev_hdr_rgb, void* dev_ldr_rgb);

/* Block until everything queued on the context's stream has finished. */
int rt_synchronize(rt_ctx* ctx);

/* Global row index of local row lr under rs (pure host arithmetic; no GPU). */
uint32_t rt_rowset_local_rows(rt_rowset rs);
uint32_t rt_rowset_global_row(rt_rowset rs, uint32_t local_row);
/* The inverse: which shard owns row image_row of the row range (counted from rs.first_row, < rs.num_rows) and which of its local rows
 * that is; rs.shard is ignored.  rt_rowset_global_row({.., shard = *shard, ..}, *local_row) == rs.first_row + image_row.  A null
 * pointer, block_rows or nshards of 0, or a row beyond the range: RT_ERR_INVALID_ARG.  Pure host arithmetic; no GPU.  The same
 * source (csrc/rt_rowset_map.h) is what the kernel of rt_denoise_shards finds its rows with. */
int rt_rowset_locate(rt_rowset rs, uint32_t image_row, uint32_t* shard, uint32_t* local_row);

/* --------------------------------------------------- unit-level entry points
 * Batched, device-evaluated pieces of the path, so that each reference function
 * has a GPU-vs-oracle known-answer test (tests/test_gpu_parity.py).  All buffers
 * are host memory; n elements. */

/* Random::HaltonSample — quasi-random.cpp:3-16 */
int rt_unit_halton(rt_ctx* ctx, const uint32_t* index, uint32_t base, uint32_t n, float* out);
/* op 0: sin, 1: cos, 2: pow(x,y), 3: tan — the shared elementary-function contract; 4: the refined reciprocal and
 * 5: the guarded Markstein quotient x/y of the hit processing (both must equal IEEE division); 6: plain x/y on the device;
 * 7: the path's square root (guarded fast form), 8: its fast form alone (x in [2^-80, inf)), 9: the compiler's sqrtf on the
 * device -- all three must equal the IEEE square root */
int rt_unit_math(rt_ctx* ctx, uint32_t op, const float* x, const float* y, uint32_t n, float* out);
/* ops 0 to 3 of rt_unit_math from the same source compiled for the host (csrc/rt_device_math.h).  y may be NULL except for op 2.
 * Needs no GPU. */
int rt_unit_math_host(uint32_t op, const float* x, const float* y, uint32_t n, float* out);
/* GenerateRays for chosen pixels: (i,j,s) -> origin xyz, direction xyz (6 floats each) */
int rt_unit_primary_rays(rt_ctx* ctx, uint32_t W, uint32_t H, const uint32_t* ijs /*3 per ray*/,
                         uint32_t n, float* out_rays);
/* Closest hit over the uploaded scene: rays (6 floats) -> t, index (as float bits), pos xyz,
 * normal xyz, uv (10 floats each; index < 0 == miss) */
int rt_unit_closest_hit(rt_ctx* ctx, const float* rays, uint32_t n, float* out_hits);
/* Per-sample radiance*exposure for chosen (i,j,s): 3 floats each + traversal count */
int rt_unit_trace(rt_ctx* ctx, uint32_t W, uint32_t H, const uint32_t* ijs, uint32_t n,
                  uint32_t max_depth, uint64_t seed, float* out_rgb, uint32_t* out_traversals);

/* Camera::GetRay (camera.cpp:30-48) for (uv.x, uv.y, offset.x, offset.y) quadruples -> origin xyz, direction xyz */
int rt_unit_camera_rays(rt_ctx* ctx, const rt_camera* camera, const float* uv_offset, uint32_t n, float* out_rays);
/* Material::Scatter (material.cpp:20-164) + Emit + unoccluded DirectionalLight::Shade (light.cpp:21-40) for one
 * material record.  in: ray direction 3, hit pos 3, hit normal 3, three uniforms consumed in call order (12 floats);
 * out: scattered flag, attenuation 3, scattered direction 3, draws consumed, Emit+Shade 3 (11 floats). */
int rt_unit_scatter(rt_ctx* ctx, const rt_material* material, const rt_light* sun, const float view_origin[3],
                    const float* in, uint32_t n, float* out);  /* uses the context's sampler flags; the record must be inside the material domain */
/* Host-only view of the clustered storage rt_scene_upload builds for the scan (groups of four spheres with a
 * conservative bounding sphere each).  orig: 4 entries per group, 0xffffffff = padding;
 * bounds: Cx, Cy, Cz, |C|^2 - Rf^2 per group.  cap_groups == 0 only queries *n_groups.  Needs no GPU. */
int rt_unit_layout(const rt_sphere* spheres, uint32_t n, uint32_t cap_groups, uint32_t* n_groups, uint32_t* orig, float* bounds);
/* ... and which closest-hit scan that storage is laid out for: out[0] = 0 flat matrix-core filter (<= 128 groups), 1 cell grid,
 * 2 bounds hierarchy; out[1], out[2] = grid cells along its two axes (0 otherwise); out[3] = big spheres tested for every ray;
 * out[4] = levels of bounds.  Needs no GPU. */
int rt_unit_layout_info(const rt_sphere* spheres, uint32_t n, uint32_t out[5]);
/* The cell-grid scan's walk as SHIPPED (csrc/rt_scan.h grid_segment_slope + grid_slab_rows, compiled for the host from the same
 * source the kernels use): for n segments (su, sv, eu, ev, D: 5 floats each, grid coordinates) and slabs iu, the rows [r0, r1] of
 * slab iu the walk visits (r0 > r1: none) and the entry parameter sEnter.  out_rows: 2 ints per query.  Needs no GPU. */
int rt_unit_grid_rows(const float* segments, const int32_t* iu, uint32_t n, int32_t nv, int32_t* out_rows, float* out_s_enter);
/* The cell grid rt_scene_upload would build for these spheres.  out_u[0] = 1: the scene selects the cell-grid scan (else nothing more
 * is written); out_u[1..4] = cells along u and v, the scene axes (0 x, 1 y, 2 z) that are u and v.  out_f[0..3] = the grid's origin
 * along u and v, 1 / cell size, and the walk's dilation max|r| / cell size of the small spheres (the kernel adds its rounding reach
 * and slack); out_f[4..9] = lo.xyz, hi.xyz of the box around the small spheres, radii |r| included, to which rays are clipped.
 * home_cell (n ints, may be null): cell iu * nv + iv whose run of scan entries holds each sphere, -1 for a big sphere (tested for every
 * ray).  Needs no GPU. */
int rt_unit_grid_info(const rt_sphere* spheres, uint32_t n, uint32_t out_u[5], float out_f[10], int32_t* home_cell);
/* Candidate masks of the primary rays (csrc/rt_tile_mask.h), as rt_render builds them for the uploaded scene when an accumulation of a
 * W x H image over row set rs starts: 8 words per full tile of 64 consecutive local pixels -- [0..3] the flat scan's candidate words
 * (bit N from the top of word k = group kBase[k] + N + (N & 16), kBase = 0, 64, 16, 80), [4] bit 0 = the tile has a mask (else it keeps
 * the matrix-core filter), [5] = candidate groups.  *n_tiles = 0: this scene / these settings use no masks.  group_of_sphere (by
 * original sphere index, may be null): the group each sphere belongs to.  scans (may be null): [0] blocks of 64 fresh paths (host arithmetic) and [1]
 * the scans that took a mask (counted by the kernel), in the last rt_render that launched a trace kernel of its own. */
int rt_unit_tile_masks(rt_ctx* ctx, uint32_t W, uint32_t H, rt_rowset rs, uint32_t cap_tiles, uint32_t* n_tiles, uint32_t* words,
                       uint32_t cap_spheres, uint32_t* group_of_sphere, uint64_t scans[2]);
/* ... the same masks evaluated on the host from the same source (candidate limit given).  Needs no GPU. */
int rt_unit_tile_masks_host(const rt_sphere* spheres, uint32_t n, const rt_camera* camera, uint32_t W, uint32_t H, rt_rowset rs, uint32_t limit,
                            uint32_t cap_tiles, uint32_t* n_tiles, uint32_t* words, uint32_t* group_of_sphere);
/* Sphere lists of the tiles' primary rays (csrc/rt_tile_mask.h), as the device built them for the strip rs of a W x H image under the
 * current RT_PRIMARY_MASK_LIMIT / RT_PRIMARY_SPHERES: 64 16-bit values per full tile, [0] = the number of listed scan entries or
 * 0xffff (the tile has no list: no mask, or more reachable spheres than the limit), [1 + k] = the k-th listed scan entry, ascending.
 * A tile with a list resolves the scan of its 64 fresh primary rays directly against the listed spheres.  *n_tiles = 0: no lists
 * (this scene / these settings).  scans (may be null): [0] blocks of 64 fresh paths, [1] scans that took a tile's mask or list (as
 * rt_unit_tile_masks reports), [2] those resolved directly from a sphere list, in the last rt_render that launched a trace kernel of its own. */
int rt_unit_tile_spheres(rt_ctx* ctx, uint32_t W, uint32_t H, rt_rowset rs, uint32_t cap_tiles, uint32_t* n_tiles, uint16_t* lists, uint64_t scans[3]);
/* The kernel's own count of tile-planes (64 fresh paths of one full tile at one sample) that were finished without rays because the
 * tile's sphere list is empty (csrc/rt_kernels.h kSky), in the last rt_render that launched a trace kernel of its own; they are part
 * of scans[2] above.  0 with RT_SKY_SKIP=0. */
int rt_unit_sky_planes(rt_ctx* ctx, uint64_t* planes);
/* Full tiles the last rt_render that launched a trace kernel of its own kept OUT of its queue because their sphere list is empty: the
 * launch covered only the other tiles, the accumulation added the constant sky sample for these, and the counters above were given
 * these tiles' share by the host.  0 whenever every tile was queued: the tiles' number had not reached the host yet (it is copied
 * asynchronously where the tables are built and never waited for, so the first rt_render of a picture reports 0), RT_SKY_EXCLUDE=0,
 * RT_SKY_SKIP=0, RT_TILE_ORDER=0, too few tiles for a work order, a partial last tile, frame pipelining. */
int rt_unit_sky_excluded(rt_ctx* ctx, uint32_t* tiles);
/* The work order of the full tiles (csrc/rt_kernels.h, "work order of the tiles"), which rt_render builds where an accumulation of a
 * picture with at least 2 x compute-units full tiles starts (RT_TILE_ORDER=0: never) and whose trace launches take their tiles through.
 * The contract of the order, for a strip of npix = W x local rows pixels, tile t = local pixels [64 t, 64 t + 64) in row-major order of
 * the strip (a tile may straddle two rows), nFull = npix / 64 full tiles:
 *   - pilots: three primary rays per full tile, those of its local pixels 64 t, 64 t + 32 and 64 t + 63 (first, middle, last), each at
 *     sample 1: pixel (i, j) = (p mod W, rt_rowset_global_row(rs, p / W)), the ray rt_unit_primary_rays gives for (i, j, 1) under the
 *     context's sampler flags (jitter and lens sample included).  Their first hits are rt_unit_closest_hit's.
 *   - pilot class of a tile: the largest over its three pilots of 0 nothing hit, 3 RT_MAT_DIELECTRIC_TRANSPARENT, 2 RT_MAT_METAL, 1 any
 *     other material (the type of the sphere hit first).
 *   - neighbour rule: a tile whose pilot class is below 3 gets 3 if one of six pixels lies in a FULL tile of pilot class 3 -- with
 *     f = 64 t the local pixels f - 64, f + 64 (the tiles before and after), f - W, f - W + 63 (above its first and its last pixel),
 *     f + W, f + W + 63 (below them); a pixel before the strip, or in the partial last tile or beyond, counts for nothing.  The rule
 *     reads pilot classes only: it does not propagate.
 *   - stored class: 0 for a flagged tile, else 1 + the class after the rule (1 nothing hit, 2 other, 3 metal, 4 glass).  A tile is
 *     flagged iff its sphere list (rt_unit_tile_spheres) is EMPTY, where the picture has lists and RT_SKY_SKIP and RT_SKY_EXCLUDE are
 *     on; the flag is applied AFTER the rule, so a flagged tile next to glass stays 0 -- and is never a source of the rule itself.
 *   - order: the stable sort of 0 .. nFull - 1 by DESCENDING stored class -- a permutation that ends with exactly the flagged tiles.
 *
 * rt_unit_tile_order, source 0: builds all of that afresh for the strip rs of a W x H image -- pilot rays, the production closest-hit
 * scan, the flags, classes, the sort: the very launches rt_render makes, into buffers of the call's own -- for ANY nFull >= 1 (the
 * 2 x compute-units threshold is a scheduling decision, not part of what the kernels compute) and whatever RT_TILE_ORDER says.  Masks
 * and lists are obtained as rt_unit_tile_spheres obtains them, under the knobs of the moment, and like it the call may rebuild the mask
 * tables for this picture; the order, flags and count the context keeps for its running accumulation are not touched.  source 1: copies
 * out what the context keeps for its running accumulation of exactly this picture; *n_tiles = 0 where it keeps no order (too few tiles,
 * RT_TILE_ORDER=0, another picture, nothing rendered since an upload, a camera move or a shading edit).
 * Out, each where the pointer is not null and for *n_tiles = nFull tiles: pilot_rays 18 floats per tile (origin xyz, direction xyz of
 * the three pilots), classes and flags one byte per tile (flags 0 / 1), order one word per tile, info[0] = the number of flagged tiles,
 * info[1..3] = the bits of the flagged tiles' constant sample (sky x exposure); without flags, flags and info read 0.  nFull == 0:
 * RT_OK with *n_tiles = 0.  Refused: a null context or n_tiles, W or H of 0, source > 1, a bad row set (RT_ERR_INVALID_ARG); no scene
 * (RT_ERR_NO_SCENE); cap_tiles below *n_tiles with any of the four arrays asked for (RT_ERR_INVALID_ARG, *n_tiles is written).  The
 * context's stream has run dry when the call returns. */
int rt_unit_tile_order(rt_ctx* ctx, uint32_t W, uint32_t H, rt_rowset rs, uint32_t source, uint32_t cap_tiles, uint32_t* n_tiles, float* pilot_rays,
                       uint8_t* classes, uint8_t* flags, uint32_t* order, uint32_t info[4]);
/* The sort alone: the production rt_tile_order_kernel, launched as rt_render launches it (one workgroup of 1024 threads), over n_tiles
 * stored classes given by the caller.  order_out: n_tiles + 64 words -- the order, then 64 guard words the entry set to 0xffffffff behind
 * the kernel's destination and copied back with it (a test checks that they are intact).  Needs no scene; touches nothing the context
 * keeps.  A null pointer, n_tiles == 0 or a class of 5 or more: RT_ERR_INVALID_ARG. */
int rt_unit_tile_order_sort(rt_ctx* ctx, const uint8_t* classes, uint32_t n_tiles, uint32_t* order_out);
/* ... the same lists evaluated on the host from the same source (both limits given).  entry_of_sphere (by original sphere index, may be
 * null): the scan entry of each sphere.  Needs no GPU. */
int rt_unit_tile_spheres_host(const rt_sphere* spheres, uint32_t n, const rt_camera* camera, uint32_t W, uint32_t H, rt_rowset rs, uint32_t mask_limit,
                              uint32_t sphere_limit, uint32_t cap_tiles, uint32_t* n_tiles, uint16_t* lists, uint32_t* entry_of_sphere);
/* ... and the cone of the primary rays of pixels i0..i1 of row j: out = camera origin 3, axis D = Fc - origin 3, rhoL, rhoF, valid.
 * Every point (1 - l) O + l F of such a ray lies within |1 - l| rhoL + l rhoF of origin + l D.  Needs no GPU. */
int rt_unit_tile_cone(const rt_camera* camera, uint32_t W, uint32_t H, uint32_t i0, uint32_t i1, uint32_t j, double out[9]);
/* The estimate of rt_noise_map for given strips (3 floats per pixel each), from the same source compiled for the host (csrc/rt_noise.h):
 * out = 2 floats per pixel.  n < 2: RT_ERR_SEQUENCE.  Needs no GPU. */
int rt_unit_noise_estimate_host(const float* hdr, const float* sq, uint32_t npix, uint32_t n, float floor, float* out);
/* The per-sample step of the feature buffers for n hit records of rt_unit_closest_hit's format (hits10[1] = the original sphere index
 * as bits, < 0 = miss), from the same source compiled for the host (csrc/rt_features.h): out8 = v[8] per record, out_ids = its id.
 * materials: by original sphere index (an index >= n_materials is RT_ERR_INVALID_ARG).  Needs no GPU. */
int rt_unit_features_host(const rt_material* materials, uint32_t n_materials, const rt_material* sky, const float* hits10, uint32_t n,
                          float* out8, uint32_t* out_ids);
/* The filter of rt_denoise for given strips (hdr, sq: 3 floats per pixel after n samples; feat8: 8 floats per pixel after m samples; W x
 * rows pixels), from the same source compiled for the host (csrc/rt_denoise.h): out_rgb = 3 floats, out_var = 1 float per pixel.
 * params == NULL: the defaults.  A null buffer, an empty strip or parameters outside their domain: RT_ERR_INVALID_ARG; n < 2 or m == 0:
 * RT_ERR_SEQUENCE.  Needs no GPU. */
int rt_unit_denoise_host(const float* hdr, const float* sq, uint32_t n, const float* feat8, uint32_t m, uint32_t W, uint32_t rows,
                         const rt_denoise_params* params, float* out_rgb, float* out_var);
/* The filter of rt_denoise_shards for given parts, from the same sources compiled for the host (csrc/rt_rowset_map.h, csrc/rt_denoise.h).
 * hdr, sq, feat8: host memory in the layout of rt_shard_parts; of *shape the pointers are ignored, everything else is read as
 * rt_denoise_shards reads it.  out_rgb = 3 floats, out_var = 1 float per pixel of the W x rs.num_rows image, in image order.  The
 * padding rows are never read.  Refusals as rt_denoise_shards'.  Needs no GPU. */
int rt_unit_denoise_shards_host(const float* hdr, const float* sq, const float* feat8, const rt_shard_parts* shape, const rt_denoise_params* params,
                                float* out_rgb, float* out_var);
/* One frame step of rt_denoise_temporal plus the levels, from the same sources compiled for the host (csrc/rt_temporal.h,
 * csrc/rt_denoise.h), over plain arrays and two camera records: hdr, sq, feat8, ids the strip of rows [first_row, first_row + num_rows)
 * of the W x H image after n and m samples; camera the current record, hist_camera the history's; hist_state4 (4 floats per pixel),
 * hist_guides8 (8), hist_ids and hist_len the history's strips -- hist_len == NULL is an empty history, and the other four are then not
 * read.  Out, each where the pointer is not null: out_rgb (3 floats per pixel) and out_var = den and den_var; out_state4, out_guides8,
 * out_len = the new history (its ids are `ids`, its camera `camera`); out_target.  params, tparams == NULL: the defaults.  Refusals as
 * rt_unit_denoise_host's and rt_denoise_temporal's.  Needs no context and no GPU. */
int rt_unit_temporal_host(const float* hdr, const float* sq, uint32_t n, const float* feat8, uint32_t m, const uint32_t* ids, uint32_t W, uint32_t H,
                          uint32_t first_row, uint32_t num_rows, const rt_camera* camera, const rt_camera* hist_camera, const float* hist_state4,
                          const float* hist_guides8, const uint32_t* hist_ids, const uint32_t* hist_len, const rt_denoise_params* params,
                          const rt_temporal_params* tparams, float* out_rgb, float* out_var, float* out_state4, float* out_guides8, uint32_t* out_len,
                          uint32_t* out_target);
/* rt_unit_temporal_host with the fetch chosen (tparams == NULL: that fetch's defaults; fetch neither 1 nor 4: RT_ERR_INVALID_ARG): the
 * twin of rt_denoise_temporal_fetch.  Fetch 1 gives rt_unit_temporal_host's bits. */
int rt_unit_temporal_host_fetch(const float* hdr, const float* sq, uint32_t n, const float* feat8, uint32_t m, const uint32_t* ids, uint32_t W, uint32_t H,
                                uint32_t first_row, uint32_t num_rows, const rt_camera* camera, const rt_camera* hist_camera, const float* hist_state4,
                                const float* hist_guides8, const uint32_t* hist_ids, const uint32_t* hist_len, const rt_denoise_params* params,
                                const rt_temporal_params* tparams, uint32_t fetch, float* out_rgb, float* out_var, float* out_state4, float* out_guides8,
                                uint32_t* out_len, uint32_t* out_target);
/* The twin of rt_denoise_shards_temporal, from the same sources compiled for the host (csrc/rt_rowset_map.h, csrc/rt_temporal.h,
 * csrc/rt_denoise.h).  hdr, sq, feat8, ids: host memory in the layout of rt_shard_frame; of *shape the pointers are ignored, everything
 * else -- the camera too -- is read as rt_denoise_shards_temporal reads it.  The history's strips and every output are as
 * rt_unit_temporal_host_fetch's, in image order, W x rs.num_rows pixels (the new history's ids are the parts' ids in image order, its
 * camera shape->camera).  The padding rows are never read.  Refusals as rt_denoise_shards_temporal's and rt_unit_temporal_host_fetch's.
 * Needs no context and no GPU. */
int rt_unit_temporal_shards_host(const float* hdr, const float* sq, const float* feat8, const uint32_t* ids, const rt_shard_frame* shape,
                                 const rt_camera* hist_camera, const float* hist_state4, const float* hist_guides8, const uint32_t* hist_ids,
                                 const uint32_t* hist_len, const rt_denoise_params* params, const rt_temporal_params* tparams, uint32_t fetch,
                                 float* out_rgb, float* out_var, float* out_state4, float* out_guides8, uint32_t* out_len, uint32_t* out_target);
/* rt_unit_denoise_host with the variance source chosen: the twin of rt_denoise_variance.  vparams == NULL or RT_VARIANCE_MOMENTS:
 * rt_unit_denoise_host's refusals and bits.  Under RT_VARIANCE_SPATIAL sq may be NULL (it is not read) and n >= 1 suffices (n == 0:
 * RT_ERR_SEQUENCE); a radius outside 1..3 or an unknown source: RT_ERR_INVALID_ARG.  out_state4 (may be NULL): the prepared (c0, v0), 4
 * floats per pixel, as the levels read it.  Needs no GPU. */
int rt_unit_denoise_variance_host(const float* hdr, const float* sq, uint32_t n, const float* feat8, uint32_t m, uint32_t W, uint32_t rows,
                                  const rt_denoise_params* params, const rt_variance_params* vparams, float* out_rgb, float* out_var, float* out_state4);
/* rt_temporal_forget on the host, from the same membership rule (csrc/rt_forget.h), in place: len[p] = 0 for every p < npix whose
 * ids[p] is one of forget_ids[0 .. n_ids); 0xffffffff names the sky, ids at or above n_spheres match nothing.  npix > 0 with len or
 * ids NULL, or n_ids > 0 with forget_ids NULL: RT_ERR_INVALID_ARG.  Needs no GPU. */
int rt_unit_temporal_forget_host(uint32_t* len, const uint32_t* ids, uint32_t npix, uint32_t n_spheres, const uint32_t* forget_ids, uint32_t n_ids);
/* rt_unit_temporal_host_fetch with the variance source chosen: the twin of rt_denoise_temporal_variance, sq and n as above. */
int rt_unit_temporal_variance_host(const float* hdr, const float* sq, uint32_t n, const float* feat8, uint32_t m, const uint32_t* ids, uint32_t W, uint32_t H,
                                   uint32_t first_row, uint32_t num_rows, const rt_camera* camera, const rt_camera* hist_camera, const float* hist_state4,
                                   const float* hist_guides8, const uint32_t* hist_ids, const uint32_t* hist_len, const rt_denoise_params* params,
                                   const rt_temporal_params* tparams, uint32_t fetch, const rt_variance_params* vparams, float* out_rgb, float* out_var,
                                   float* out_state4, float* out_guides8, uint32_t* out_len, uint32_t* out_target);
/* rt_unit_denoise_shards_host and rt_unit_temporal_shards_host with the variance source chosen: the twins of rt_denoise_shards_variance
 * and rt_denoise_shards_temporal_variance.  vparams == NULL or RT_VARIANCE_MOMENTS: those twins' refusals and bits.  Under
 * RT_VARIANCE_SPATIAL sq may be NULL and shape's n >= 1 suffices, as above.  out_state4 (may be NULL) of the first: the prepared (c0, v0)
 * in image order.  Need no GPU. */
int rt_unit_denoise_shards_variance_host(const float* hdr, const float* sq, const float* feat8, const rt_shard_parts* shape, const rt_denoise_params* params,
                                         const rt_variance_params* vparams, float* out_rgb, float* out_var, float* out_state4);
int rt_unit_temporal_shards_variance_host(const float* hdr, const float* sq, const float* feat8, const uint32_t* ids, const rt_shard_frame* shape,
                                          const rt_camera* hist_camera, const float* hist_state4, const float* hist_guides8, const uint32_t* hist_ids,
                                          const uint32_t* hist_len, const rt_denoise_params* params, const rt_temporal_params* tparams, uint32_t fetch,
                                          const rt_variance_params* vparams, float* out_rgb, float* out_var, float* out_state4, float* out_guides8,
                                          uint32_t* out_len, uint32_t* out_target);
/* Which form each level of the last rt_denoise, rt_denoise_shards, rt_denoise_temporal or rt_denoise_shards_temporal took: out[l] = 0 the level did not run, 1 its taps were read from
 * global memory, 2 from a tile staged in LDS. */
int rt_unit_denoise_forms(rt_ctx* ctx, uint32_t out[5]);
/* The shadow index rt_scene_upload would build for light `light` of the list, under the environment of the moment.
 * out_u: [0] 1 = the index is enabled (else nothing more is valid: every shadow ray of this light is answered over every scan
 * entry), [1] nx, [2] ny, [3] elements of cell_start (nx * ny + 1), [4] of entries, [5] of global, [6] scan entries (elements of orig),
 * [7] 1 = the scan's tables stay in global memory (cell grid, hierarchy).  out_f: e1 3, e2 3, u0, v0, 1 / cell size, p0sq.
 * cell_start, entries, global (16-bit scan-entry ids) and orig (original sphere index of every scan entry, 0xffffffff = padding) are
 * written where the pointer is not null; a capacity below the count is RT_ERR_INVALID_ARG.  Needs no GPU. */
int rt_unit_shadow_index_host(const rt_sphere* spheres, uint32_t n, const rt_light* lights, uint32_t n_lights, uint32_t light, uint32_t out_u[8],
                              float out_f[10], uint32_t cap_cells, uint16_t* cell_start, uint32_t cap_entries, uint16_t* entries,
                              uint32_t cap_global, uint16_t* global, uint32_t cap_orig, uint32_t* orig);
/* The shadow question of the hit processing for n_points points (3 floats each) and that light, answered on the host by the source the
 * kernels compile (csrc/rt_shade.h shadow_query and any_hit_all over the tables above): one byte per point, bit 0 = occluded, bit 1 =
 * answered over every scan entry (the index is off, or |p|^2 > p0sq) and not from the index.  Needs no GPU. */
int rt_unit_shadow_query_host(const rt_sphere* spheres, uint32_t n, const rt_light* lights, uint32_t n_lights, uint32_t light,
                              const float* points, uint32_t n_points, uint8_t* out);
/* ... and by the device, over the tables rt_scene_upload put there for the uploaded scene (light 0: the launch parameters' index,
 * lights 1 ..: their records): the same byte per point.  glob_in_lds != 0: the index's global list is walked from a copy of
 * (spheres, ids) in LDS, staged as the trace kernel stages it; 0: from its id list in global memory. */
int rt_unit_shadow(rt_ctx* ctx, uint32_t light, const float* points, uint32_t n, uint32_t glob_in_lds, uint8_t* out);
/* What the launcher decides for n trace launches, with no context and no device (csrc/host/rt_launch_plan.h): the LDS image, the
 * launch parameters that describe it, the grid and the kernel variant.  cases: 28 words each --
 *   [0] scan entries (n_padded)  [1] hierarchy levels (1..6)  [2] nodes of the top level  [3] first node of the top level
 *   [4] scene bits: 1 laid out for the cell grid, 2 has quantised bounds, 4 light 0 has a shadow index, 8 has packed materials
 *   [5] [6] grid cells nu, nv  [7] [8] shadow index cells nx, ny  [9] its entries  [10] its global entries  [11] lights
 *   [12] CUs  [13] blocks per CU (1..8)  [14] threads per block (a multiple of 64, <= 1024)
 *   [15] setting bits: 1 RT_SCAN=mfma, 2 RT_MATS_LDS, 4 RT_RAY_CACHE, 8 RT_STASH, 16 RT_TREE_LDS, 32 RT_FORCE_GLOBAL_TABLES
 *   [16] RT_MATS16  [17] RT_MATS_L2  [18] RT_STASH_CAP  [19] RT_STASH_PROCESS  [20] RT_GRID_QUANT  [21] RT_GRID_SG_LDS  [22] RT_QUEUE_BLOCK
 *   [23] RT_QUEUE_STATIC  [24] paths  [25] max_depth  [26] 0 = ordinary launch, 1 = the frame-pipelining launch  [27] 0
 * plans: 28 words each --
 *   [0] RT_OK or the error code of a refused launch  [1] which refusal: 1 too many scan entries, 2 no pipelining for this scene,
 *       3..5 internal (materials through L2 / shadow index in LDS / quantised bounds, each without the hit stash); after a refusal
 *       only [26] and [27] are valid besides
 *   [2] blocks  [3] dynamic LDS bytes  [4..9] the parts RT_VERBOSE prints: work lists, tables, one-sphere bounds, filter operands,
 *       shadow index, hierarchy
 *   [10] bits: 1 hierarchy scan, 2 flat scan, 4 cell-grid scan, 8 ... with every table in LDS, 16 scan tables in LDS, 32 path cache,
 *        64 the kernel finishes empty-list planes itself, 128 ([26] = 1) the scene gets the pipelining variant
 *   [11] mats_in_lds  [12] mats16_mode  [13] sg_glob16  [14] sg_in_lds  [15] tree_in_lds  [16] grid_in_lds  [17] ray_cache_off16
 *   [18] ray_cache_stride16  [19] stash_cap  [20] stash_process  [21] queue_block  [22] static_blocks  [23] dyn_begin  [24] dyn_blocks
 *       ([21..24]: 0 for the pipelining launch, whose caller sets them)
 *   [25] the kernel: bit 0 the _lights twin, 1 kLds, 2-3 kThreads (0 = 256, 1 = 512, 2 = 1024), 4-5 kScan, 6 kCache, 7 kHitLds, 8 kCarry,
 *        9 kStash, 10 kMatsL2, 11 kSgLds, 12 kGridQ, 31 the variant is instantiated
 *   [26] the unit kernels' scan (rt_unit_closest_hit, rt_render_features): bit 0 kLds, 1-2 kScan, 3 tree_in_lds, 4 instantiated
 *   [27] ... and their dynamic LDS bytes
 * A case no context or scene can be ([13], [14], [1] out of range, cells beyond 65,535 a side, unknown bits) is RT_ERR_INVALID_ARG.
 * Needs no GPU. */
int rt_unit_launch_plan(const uint32_t* cases, uint32_t n, uint32_t* plans);
/* The launcher's own account of the most recent trace-kernel launch of this context, in exactly the words above: case_words = the
 * inputs it gathered from the uploaded scene, the context's settings and the RT_* knobs of that moment, plan_words = the plan it
 * applied ([25] the kernel that ran, [21..24] its queue cut, [2] its blocks); either may be null.  Ordinary, path-list and
 * frame-pipelining launches alike (a render call may make several: the last one counts).  Feeding case_words to rt_unit_launch_plan
 * returns plan_words.  *launches (may be null) = trace-kernel launches since rt_create.  Before the first launch: RT_ERR_SEQUENCE
 * (*launches = 0 is still written, the words are not); a null context: RT_ERR_INVALID_ARG (nothing is written).  Waits for nothing: the
 * words are known when the launch is made. */
int rt_unit_last_trace_launch(rt_ctx* ctx, uint32_t case_words[28], uint32_t plan_words[28], uint32_t* launches);
/* The variants of the trace kernel the library instantiates (csrc/rt_trace_variants.h), in list order, each as word [25] above in its
 * single-light form (bit 0 clear, bit 31 set); every one exists a second time as its _lights twin (bit 0 set).  *n = their number (55);
 * cap == 0 only queries it, a smaller capacity than *n is RT_ERR_INVALID_ARG.  Needs no GPU. */
int rt_unit_trace_variants(uint32_t* kernel_words, uint32_t cap, uint32_t* n);
/* ... and those of them that exist once more WITHOUT far-hit state (csrc/rt_trace_variants.h RT_TRACE_LEAN_VARIANTS): the
 * same words, a subset of the list above (3: the flat hit-stash rows), each again with its _lights twin -- six functions behind the 110.
 * A lean kernel is its row's kernel for picture launches, not another row: the plan, its words and word [25] are the row's.  Same
 * argument rules.  Needs no GPU. */
int rt_unit_trace_lean_variants(uint32_t* kernel_words, uint32_t cap, uint32_t* n);
/* Whether the most recent trace-kernel launch of this context ran its row's lean function (*lean = 1) or the one with far-hit state
 * (0): what rt_unit_last_trace_launch's words cannot say, since both are the same row.  Same refusals as that entry. */
int rt_unit_last_trace_far_state(rt_ctx* ctx, uint32_t* lean);
/* The launcher's rule for that choice (csrc/host/rt_launch_plan.h FarStateLean), with no context and no device: *lean = 1 when the
 * launch that case_words (28 words, as above) describe takes the lean function, given whether it traces an explicit path list, wants
 * per-path traversal counts (rt_unit_trace does both), whether the context builds shadow indices (RT_SHADOW_GRID is not 0) and whether
 * RT_FAR_STATE=1 forces the far-hit state.  A case rt_unit_launch_plan refuses as impossible is RT_ERR_INVALID_ARG. */
int rt_unit_far_state_plan(const uint32_t* case_words, uint32_t path_list, uint32_t trav_out, uint32_t shadow_grid, uint32_t force_full, uint32_t* lean);
/* The three shadow entries above with the index chosen: tier 1 = the light's index (what the entries above answer), tier 2 (light 0
 * only; anything else is RT_ERR_INVALID_ARG) = light 0's SECOND index, built like the first for the hit points beyond its radius and
 * kept in global memory.  rt_unit_shadow_index_host_tier hands out that index's tables (out_f[9] = the square of ITS
 * radius; out_u[0] = 0: the scene has none).  The two query entries then answer as the kernels without far-hit state ask: the first
 * index within its radius, the second one within its own (bit 2 set, bit 1 clear), else every scan entry (bit 1 set). */
int rt_unit_shadow_index_host_tier(const rt_sphere* spheres, uint32_t n, const rt_light* lights, uint32_t n_lights, uint32_t light, uint32_t tier,
                                   uint32_t out_u[8], float out_f[10], uint32_t cap_cells, uint16_t* cell_start, uint32_t cap_entries, uint16_t* entries,
                                   uint32_t cap_global, uint16_t* global, uint32_t cap_orig, uint32_t* orig);
int rt_unit_shadow_query_host_tier(const rt_sphere* spheres, uint32_t n, const rt_light* lights, uint32_t n_lights, uint32_t light, uint32_t tier,
                                   const float* points, uint32_t n_points, uint8_t* out);
int rt_unit_shadow_tier(rt_ctx* ctx, uint32_t light, uint32_t tier, const float* points, uint32_t n, uint32_t glob_in_lds, uint8_t* out);
/* The resolve of spheres-app.cpp:196-214 for given HDR triples -> R,G,B bytes */
int rt_unit_tonemap(rt_ctx* ctx, const float* hdr_rgb, uint32_t n, uint32_t n_samples, uint8_t* out_rgb);

#ifdef __cplusplus
}
#endif
#endif /* RT_API_H */
