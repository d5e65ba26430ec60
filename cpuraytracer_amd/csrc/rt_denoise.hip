// rt_denoise.hip -- the denoiser's kernels and their launcher (DESIGN.md "Denoise"; arithmetic: rt_denoise.h).  A translation unit
// of its own: rt_capi.hip calls rtdn::Launch (host/rt_denoise_launch.h) and holds none of this device code.
#include <hip/hip_runtime.h>

#include "host/rt_denoise_launch.h"

namespace rtd {

// The three pieces every prepare pass is made of.  The inputs of a pixel of the current frame, read where they lie (p): hdr and sq as
// three floats each, feat as two float4 -- what denoise_prepare forms the state (c.rgb, v) and the guides from ...
__device__ __forceinline__ void load_pixel(const float* __restrict__ hdr, const float* __restrict__ sq, const float4* __restrict__ feat, const size_t p,
                                           float h[3], float q[3], float f[8]) {
    h[0] = hdr[3 * p], h[1] = hdr[3 * p + 1], h[2] = hdr[3 * p + 2];
    q[0] = sq[3 * p], q[1] = sq[3 * p + 1], q[2] = sq[3 * p + 2];
    const float4 fa = feat[2 * p], fb = feat[2 * p + 1];
    f[0] = fa.x, f[1] = fa.y, f[2] = fa.z, f[3] = fa.w, f[4] = fb.x, f[5] = fb.y, f[6] = fb.z, f[7] = fb.w;
}
// ... a prepared pixel written in image order (o): the state as one float4, the guides as two float4 planes ...
__device__ __forceinline__ void store_pixel(float4* __restrict__ state, float4* __restrict__ g0, float4* __restrict__ g1, const size_t o,
                                            const DenoiseState& s, const float g[8]) {
    state[o] = make_float4(s.c[0], s.c[1], s.c[2], s.v);
    g0[o] = make_float4(g[0], g[1], g[2], g[3]);
    g1[o] = make_float4(g[4], g[5], g[6], g[7]);
}
// ... and where the current-frame inputs of IMAGE pixel pix lie in the gathered parts of a row-sharded picture: in the part and the
// local row that hold its row (rt_rowset_map.h).  A row is contiguous inside its part, so the lanes of a wave still read contiguous
// segments.  Rows of a part beyond its shard's own (the gather's padding) belong to no image row and are never read.  The result is
// < nshards * rowsMax * W: lr < rowsMax for every row of the range (rowset_max_shard_rows, checked by the caller).
__device__ __forceinline__ size_t parts_source(const rtdn::ShardLayout& L, const uint32_t W, const uint32_t pix) {
    const uint32_t y = pix / W, x = pix - y * W;
    uint32_t shard, lr;
    rowset_locate(L.blockRows, L.nshards, y, shard, lr);
    return ((size_t)shard * L.rowsMax + lr) * W + x;
}

// One pass, a thread per pixel of the strip (kParts: of the IMAGE, its inputs read through the mapping): state, g0, g1 in image order,
// so the levels run on them unchanged.
template <bool kParts>
__device__ __forceinline__ void prepare_pass(const float* __restrict__ hdr, const float* __restrict__ sq, const float4* __restrict__ feat, uint32_t W,
                                             uint32_t npix, const rtdn::ShardLayout& L, uint32_t n, uint32_t m, float4* __restrict__ state,
                                             float4* __restrict__ g0, float4* __restrict__ g1) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    DenoiseState s;
    float g[8];
    float h[3], q[3], f[8];
    load_pixel(hdr, sq, feat, kParts ? parts_source(L, W, pix) : (size_t)pix, h, q, f);
    denoise_prepare(h, q, n, f, m, s, g);
    store_pixel(state, g0, g1, pix, s, g);
}

__global__ void __launch_bounds__(256) rt_denoise_prepare_kernel(const float* __restrict__ hdr, const float* __restrict__ sq,
                                                                 const float4* __restrict__ feat, uint32_t npix, uint32_t n, uint32_t m,
                                                                 float4* __restrict__ state, float4* __restrict__ g0, float4* __restrict__ g1) {
    prepare_pass<false>(hdr, sq, feat, 0u, npix, rtdn::ShardLayout{}, n, m, state, g0, g1);
}

__global__ void __launch_bounds__(256) rt_denoise_prepare_shards_kernel(const float* __restrict__ hdr, const float* __restrict__ sq,
                                                                        const float4* __restrict__ feat, uint32_t W, uint32_t npix, uint32_t rowsMax,
                                                                        uint32_t blockRows, uint32_t nshards, uint32_t n, uint32_t m,
                                                                        float4* __restrict__ state, float4* __restrict__ g0, float4* __restrict__ g1) {
    prepare_pass<true>(hdr, sq, feat, W, npix, rtdn::ShardLayout{rowsMax, blockRows, nshards}, n, m, state, g0, g1);
}

__device__ __forceinline__ void unpack(const float4 s, const float4 a, const float4 b, DenoiseState& st, float g[8]) {
    st.c[0] = s.x; st.c[1] = s.y; st.c[2] = s.z; st.v = s.w;
    g[0] = a.x; g[1] = a.y; g[2] = a.z; g[3] = a.w;
    g[4] = b.x; g[5] = b.y; g[6] = b.z; g[7] = b.w;
}

// The temporal form of the prepare pass (rt_temporal.h): a thread owns pixel pix of the strip, forms its state and guides, reprojects
// it into the history's camera, reads the history there, validates, blends and writes the blended state, the guides, the id, the
// length and the target into the NEXT history set.  The history sets, target and every write are in image order; the current-frame
// reads and every write are contiguous row segments.  Nothing of the set that is read is written: a pixel reads other pixels' history.
struct TemporalArgs {
    const float* __restrict__ hdr;
    const float* __restrict__ sq;
    const float4* __restrict__ feat;
    const uint32_t* __restrict__ ids;
    uint32_t npix, n, m, hasPrev;
    TemporalGeom G;
    TemporalCam C, Cp;
    TemporalParams T;
    const float4* __restrict__ hS;
    const float4* __restrict__ hG0;
    const float4* __restrict__ hG1;
    const uint32_t* __restrict__ hId;
    const uint32_t* __restrict__ hLen;
    float4* __restrict__ oS;
    float4* __restrict__ oG0;
    float4* __restrict__ oG1;
    uint32_t* __restrict__ oId;
    uint32_t* __restrict__ oLen;
    uint32_t* __restrict__ target;
};
// What the two other kinds of input add to the arguments.  Prepared: the planes a spatial prepare pass (rt_denoise_prepare_spatial_kernel
// below) wrote, in image order -- (c0, v0) and g are read there, hdr, sq and feat are not read.  Parts: the layout of the gathered
// parts, where hdr, sq, feat and ids of the current frame are read through parts_source.
struct PreparedPlanes {
    const float4* __restrict__ s;
    const float4* __restrict__ g0;
    const float4* __restrict__ g1;
};
struct TemporalPreparedArgs {
    TemporalArgs A;
    PreparedPlanes Q;
};
struct TemporalShardArgs {
    TemporalArgs A;
    rtdn::ShardLayout L;
};
struct TemporalPreparedShardArgs {  // both: the planes lie in image order, only the frame's ids are read through the mapping
    TemporalArgs A;
    PreparedPlanes Q;
    rtdn::ShardLayout L;
};

// The pass has one body per fetch, called by the eight kernels with pix, the pixel of the strip they guard (pix < npix), and p, where
// its current-frame inputs lie: pix itself, or parts_source(pix) -- strips and parts differ in nothing else.  kPrepared: the pixel's
// state and guides are read from the spatial pass's planes instead of formed from hdr, sq and feat.  A body begins with the pixel's id,
// state and guides, ends with the writes into the next history set (temporal_end) and holds the history's answer in between.  The
// two bodies, their beginnings and the kernels' guards are written out, not shared further: with them in shared functions four of the
// six kernels were compiled to other instruction streams than the separately written kernels they replace
// (profiles/denoise_refactor_codegen.txt); as they stand those six have those streams, and the two that are both prepared and parts
// (profiles/denoise_shards_spatial_codegen.txt) left them alone.

__device__ __forceinline__ void temporal_end(const TemporalArgs& A, const uint32_t pix, const DenoiseState& s, const float g[8], const uint32_t id,
                                             const uint32_t len, const uint32_t target) {
    store_pixel(A.oS, A.oG0, A.oG1, pix, s, g);
    A.oId[pix] = id;
    A.oLen[pix] = len;
    A.target[pix] = target;
}

// The nearest fetch: one gathered read of a float4 state, two float4 guide planes, an id and a length; neighbouring lanes are neighbouring pixels,
// so under small motion the gather is a row segment shifted by a few pixels.  q < npix by temporal_reproject's bounds (xi < W,
// yi - first_row < num_rows).
template <bool kPrepared>
__device__ __forceinline__ void temporal_prepare_nearest(const TemporalArgs& A, const PreparedPlanes& Q, const uint32_t pix, const size_t p) {
    DenoiseState s;
    float g[8];
    uint32_t id;
    if (kPrepared) {  // the pixel's state and guides as the spatial pass left them
        id = A.ids[p];
        unpack(Q.s[pix], Q.g0[pix], Q.g1[pix], s, g);
    } else {
        float h[3], q3[3], f[8];
        load_pixel(A.hdr, A.sq, A.feat, p, h, q3, f);
        id = A.ids[p];
        denoise_prepare(h, q3, A.n, f, A.m, s, g);
    }
    uint32_t len = 1u, target = kTemporalNoTarget;
    if (A.hasPrev) {
        const uint32_t ly = pix / A.G.W, x = pix - ly * A.G.W;
        uint32_t xi = 0, yi = 0;
        float dist = 0.f;
        if (temporal_reproject(A.G, A.C, A.Cp, x, A.G.first_row + ly, g, xi, yi, dist)) {
            const uint32_t q = (yi - A.G.first_row) * A.G.W + xi;
            const float4 hs = A.hS[q], ha = A.hG0[q], hb = A.hG1[q];
            const uint32_t idh = A.hId[q], lenh = A.hLen[q];
            DenoiseState sh;
            float gh[8];
            unpack(hs, ha, hb, sh, gh);
            const bool ok = temporal_validate(A.T, g, id, dist, gh, idh, lenh);
            len = temporal_blend(A.T, ok, s, sh, lenh);
            if (ok) target = q;
        }
    }
    temporal_end(A, pix, s, g, id, len, target);
}

// The bilinear fetch (rt_temporal.h): the history is read at the four pixels around the reprojected point.  The two taps of a row are adjacent
// (32 bytes per float4 plane) and under small motion a wave's taps are two row segments its lanes share.  All four taps' loads are
// issued before the first is used: a tap outside the strip loads the pixel's own index instead (pix < npix, a contiguous read) and what
// it loaded is dropped, so no load waits for a test and none leaves the arrays -- a tap inside has its index < npix by
// temporal_tap_index.  Only taps that take part are added (temporal_gather_tap).
template <bool kPrepared>
__device__ __forceinline__ void temporal_prepare_bilinear(const TemporalArgs& A, const PreparedPlanes& Q, const uint32_t pix, const size_t p) {
    DenoiseState s;
    float g[8];
    uint32_t id;
    if (kPrepared) {  // the pixel's state and guides as the spatial pass left them
        id = A.ids[p];
        unpack(Q.s[pix], Q.g0[pix], Q.g1[pix], s, g);
    } else {
        float h[3], q3[3], f[8];
        load_pixel(A.hdr, A.sq, A.feat, p, h, q3, f);
        id = A.ids[p];
        denoise_prepare(h, q3, A.n, f, A.m, s, g);
    }
    uint32_t len = 1u, target = kTemporalNoTarget;
    if (A.hasPrev) {
        const uint32_t ly = pix / A.G.W, x = pix - ly * A.G.W;
        uint32_t xi = 0, yi = 0;
        float fx = 0.f, fy = 0.f, dist = 0.f;
        if (temporal_reproject_point(A.G, A.C, A.Cp, x, A.G.first_row + ly, g, fx, fy, xi, yi, dist)) {
            TemporalTaps B;
            temporal_taps(fx, fy, xi, yi, B);
            bool in[4];
            uint32_t q[4];
            float4 hs[4], ha[4], hb[4];
            uint32_t idh[4], lenh[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                q[k] = pix;
                in[k] = temporal_tap_index(A.G, B, k, q[k]);
                const uint32_t r = in[k] ? q[k] : pix;
                hs[k] = A.hS[r];
                ha[k] = A.hG0[r];
                hb[k] = A.hG1[r];
                idh[k] = A.hId[r];
                lenh[k] = A.hLen[r];
            }
            TemporalGather S;
            temporal_gather_begin(S);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float w = temporal_tap_weight(B, k);
                if (!(in[k] && w > 0.f)) continue;
                DenoiseState st;
                float gh[8];
                unpack(hs[k], ha[k], hb[k], st, gh);
                if (!temporal_validate(A.T, g, id, dist, gh, idh[k], lenh[k])) continue;
                temporal_gather_tap(S, w, st, lenh[k], q[k]);
            }
            DenoiseState sh{};
            uint32_t lh = 0u;
            const bool ok = temporal_gather_finish(S, sh, lh);
            len = temporal_blend(A.T, ok, s, sh, lh);
            if (ok) target = S.target;
        }
    }
    temporal_end(A, pix, s, g, id, len, target);
}

__global__ void __launch_bounds__(256) rt_denoise_prepare_temporal_kernel(const TemporalArgs A) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= A.npix) return;
    temporal_prepare_nearest<false>(A, PreparedPlanes{}, pix, pix);
}
__global__ void __launch_bounds__(256) rt_denoise_prepare_temporal_bilinear_kernel(const TemporalArgs A) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= A.npix) return;
    temporal_prepare_bilinear<false>(A, PreparedPlanes{}, pix, pix);
}
__global__ void __launch_bounds__(256) rt_denoise_prepared_temporal_kernel(const TemporalPreparedArgs S) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= S.A.npix) return;
    temporal_prepare_nearest<true>(S.A, S.Q, pix, pix);
}
__global__ void __launch_bounds__(256) rt_denoise_prepared_temporal_bilinear_kernel(const TemporalPreparedArgs S) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= S.A.npix) return;
    temporal_prepare_bilinear<true>(S.A, S.Q, pix, pix);
}
__global__ void __launch_bounds__(256) rt_denoise_prepare_shards_temporal_kernel(const TemporalShardArgs S) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= S.A.npix) return;
    temporal_prepare_nearest<false>(S.A, PreparedPlanes{}, pix, parts_source(S.L, S.A.G.W, pix));
}
__global__ void __launch_bounds__(256) rt_denoise_prepare_shards_temporal_bilinear_kernel(const TemporalShardArgs S) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= S.A.npix) return;
    temporal_prepare_bilinear<false>(S.A, PreparedPlanes{}, pix, parts_source(S.L, S.A.G.W, pix));
}
__global__ void __launch_bounds__(256) rt_denoise_prepared_shards_temporal_kernel(const TemporalPreparedShardArgs S) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= S.A.npix) return;
    temporal_prepare_nearest<true>(S.A, S.Q, pix, parts_source(S.L, S.A.G.W, pix));
}
__global__ void __launch_bounds__(256) rt_denoise_prepared_shards_temporal_bilinear_kernel(const TemporalPreparedShardArgs S) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= S.A.npix) return;
    temporal_prepare_bilinear<true>(S.A, S.Q, pix, parts_source(S.L, S.A.G.W, pix));
}

// One level.  Thread (tx, ty) of the 32 x 8 workgroup owns pixel (32 bx + tx, 8 by + ty); its 25 taps lie (a - 2) step rows and
// (b - 2) step columns away, a outer, b inner; a tap outside the strip is skipped, never clamped.
//   kStaged: the tile and its 2 step halo go into LDS first as three planes of float4 with contiguous rows (a wave stages two rows
//            of 32 at a time, and later reads 64 consecutive 16-byte slots per tap); slots of pixels outside the strip are never
//            written and never read.  One barrier.
//   else:    the taps are read from global memory: lanes are neighbouring pixels and the offset is uniform, so every read is a
//            contiguous row segment.
//   kLast:   the result goes to the packed den / den_var strips instead of the next level's state.
template <bool kStaged, bool kLast>
__global__ void __launch_bounds__(256) rt_atrous_kernel(const float4* __restrict__ state, const float4* __restrict__ g0, const float4* __restrict__ g1,
                                                        uint32_t W, uint32_t rows, uint32_t step, const DenoiseParams P, float4* __restrict__ out,
                                                        float* __restrict__ den, float* __restrict__ denVar) {
    extern __shared__ float4 tileLds[];
    const uint32_t tx = threadIdx.x & (rtdn::kTileW - 1u), ty = threadIdx.x / rtdn::kTileW;
    const int x0 = (int)(blockIdx.x * rtdn::kTileW), y0 = (int)(blockIdx.y * rtdn::kTileH);
    const int x = x0 + (int)tx, y = y0 + (int)ty;
    const int halo = 2 * (int)step;
    const uint32_t tw = rtdn::kTileW + 4u * step, th = rtdn::kTileH + 4u * step;
    float4* ldsS = tileLds;
    float4* ldsA = tileLds + tw * th;
    float4* ldsB = tileLds + 2u * tw * th;
    if (kStaged) {
        for (uint32_t ly = ty; ly < th; ly += rtdn::kTileH) {
            const int gy = y0 - halo + (int)ly;
            if (gy < 0 || gy >= (int)rows) continue;
            for (uint32_t lx = tx; lx < tw; lx += rtdn::kTileW) {
                const int gx = x0 - halo + (int)lx;
                if (gx < 0 || gx >= (int)W) continue;
                const size_t q = (size_t)gy * W + (size_t)gx;
                const uint32_t slot = ly * tw + lx;
                ldsS[slot] = state[q];
                ldsA[slot] = g0[q];
                ldsB[slot] = g1[q];
            }
        }
        __syncthreads();
    }
    if (x >= (int)W || y >= (int)rows) return;
    const size_t p = (size_t)y * W + (size_t)x;
    DenoiseState sp;
    float gp[8];
    if (kStaged) {
        const uint32_t slot = (ty + (uint32_t)halo) * tw + tx + (uint32_t)halo;
        unpack(ldsS[slot], ldsA[slot], ldsB[slot], sp, gp);
    } else {
        unpack(state[p], g0[p], g1[p], sp, gp);
    }
    DenoiseSums S;
    denoise_begin(S);
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        const int dy = (a - 2) * (int)step;
        const int qy = y + dy;
        if (qy < 0 || qy >= (int)rows) continue;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            const int dx = (b - 2) * (int)step;
            const int qx = x + dx;
            if (qx < 0 || qx >= (int)W) continue;
            DenoiseState sq;
            float gq[8];
            if (kStaged) {
                const uint32_t slot = (uint32_t)((int)ty + halo + dy) * tw + (uint32_t)((int)tx + halo + dx);
                unpack(ldsS[slot], ldsA[slot], ldsB[slot], sq, gq);
            } else {
                const size_t q = (size_t)qy * W + (size_t)qx;
                unpack(state[q], g0[q], g1[q], sq, gq);
            }
            denoise_tap(P, denoise_h(a) * denoise_h(b), sp, gp, sq, gq, S);
        }
    }
    DenoiseState r;
    denoise_finish(S, r);
    if (kLast) {
        den[3 * p] = r.c[0];
        den[3 * p + 1] = r.c[1];
        den[3 * p + 2] = r.c[2];
        denVar[p] = r.v;
    } else {
        out[p] = make_float4(r.c[0], r.c[1], r.c[2], r.v);
    }
}

// The prepare pass of the spatial variance source (rt_denoise.h).  The a-trous kernel's geometry: thread (tx, ty) of the
// 32 x 8 workgroup owns pixel (32 bx + tx, 8 by + ty).  The workgroup forms c0 = hdr / n and g = feat / m of its tile and a halo of kR
// pixels ONCE while staging them into LDS -- three planes of float4 with contiguous rows, (c0, unused), (g 0..3), (g 4..7): 48 bytes per
// pixel, (32 + 2 kR) x (8 + 2 kR) pixels, 25,536 bytes at kR = 3 -- and after one barrier every thread runs its (2 kR + 1)^2 taps from
// there, a outer, b inner.  A tap outside the strip is skipped, never clamped; slots of pixels outside the strip are never written and
// never read.  sq is not read.  committed (rt_resolve's rule): with frames in flight the strip's sample count is a word only the device
// knows.  Writes state (c0, v0), g0, g1 in image order, as rt_denoise_prepare_kernel does.
template <int kR>
__global__ void __launch_bounds__(256) rt_denoise_prepare_spatial_kernel(const float* __restrict__ hdr, const float4* __restrict__ feat, uint32_t W,
                                                                         uint32_t rows, uint32_t n, uint32_t m, const uint32_t* __restrict__ committed,
                                                                         const DenoiseParams P, float4* __restrict__ state, float4* __restrict__ g0,
                                                                         float4* __restrict__ g1) {
    constexpr uint32_t tw = rtdn::kTileW + 2u * kR, th = rtdn::kTileH + 2u * kR;
    __shared__ float4 ldsC[tw * th];
    __shared__ float4 ldsA[tw * th];
    __shared__ float4 ldsB[tw * th];
    const uint32_t tx = threadIdx.x & (rtdn::kTileW - 1u), ty = threadIdx.x / rtdn::kTileW;
    const int x0 = (int)(blockIdx.x * rtdn::kTileW), y0 = (int)(blockIdx.y * rtdn::kTileH);
    const int x = x0 + (int)tx, y = y0 + (int)ty;
    if (committed) n = *committed > 0u ? *committed : 1u;
    for (uint32_t ly = ty; ly < th; ly += rtdn::kTileH) {
        const int gy = y0 - kR + (int)ly;
        if (gy < 0 || gy >= (int)rows) continue;
        for (uint32_t lx = tx; lx < tw; lx += rtdn::kTileW) {
            const int gx = x0 - kR + (int)lx;
            if (gx < 0 || gx >= (int)W) continue;
            const size_t q = (size_t)gy * W + (size_t)gx;
            const float h[3] = {hdr[3 * q], hdr[3 * q + 1], hdr[3 * q + 2]};
            const float4 fa = feat[2 * q], fb = feat[2 * q + 1];
            const float f[8] = {fa.x, fa.y, fa.z, fa.w, fb.x, fb.y, fb.z, fb.w};
            float c[3], g[8];
            denoise_prepare_mean(h, n, f, m, c, g);
            const uint32_t slot = ly * tw + lx;
            ldsC[slot] = make_float4(c[0], c[1], c[2], 0.0f);
            ldsA[slot] = make_float4(g[0], g[1], g[2], g[3]);
            ldsB[slot] = make_float4(g[4], g[5], g[6], g[7]);
        }
    }
    __syncthreads();
    if (x >= (int)W || y >= (int)rows) return;
    const uint32_t centre = (ty + (uint32_t)kR) * tw + tx + (uint32_t)kR;
    DenoiseState sp;
    float gp[8];
    unpack(ldsC[centre], ldsA[centre], ldsB[centre], sp, gp);
    SpatialSums S;
    spatial_begin(S);
#pragma unroll
    for (int a = 0; a <= 2 * kR; ++a) {
        const int dy = a - kR;
        const int qy = y + dy;
        if (qy < 0 || qy >= (int)rows) continue;
#pragma unroll
        for (int b = 0; b <= 2 * kR; ++b) {
            const int dx = b - kR;
            const int qx = x + dx;
            if (qx < 0 || qx >= (int)W) continue;
            const uint32_t slot = (uint32_t)((int)ty + kR + dy) * tw + (uint32_t)((int)tx + kR + dx);
            DenoiseState sq;
            float gq[8];
            unpack(ldsC[slot], ldsA[slot], ldsB[slot], sq, gq);
            spatial_tap(P, gp, sq.c, gq, S);
        }
    }
    const size_t p = (size_t)y * W + (size_t)x;
    state[p] = make_float4(sp.c[0], sp.c[1], sp.c[2], spatial_finish(S));
    g0[p] = make_float4(gp[0], gp[1], gp[2], gp[3]);
    g1[p] = make_float4(gp[4], gp[5], gp[6], gp[7]);
}

// The same pass over the gathered parts of a row-sharded picture: W x rows is the IMAGE's row range, and while staging, image row gy is
// read where the mapping puts it (rt_rowset_map.h) -- a wave stages two rows, which may come from two parts, each a contiguous segment
// of its part.  A row or column outside the range is skipped BEFORE it is located: a part's padding rows (lr >= its shard's rows)
// belong to no image row and are never read; row + gx < nshards * rowsMax * W as in parts_source.  n is the call's: the parts are a
// snapshot, there is no committed word.  Everything after the barrier -- tile, halo, LDS planes, tap order, writes in image order -- is
// the kernel above, written out a second time: as one shared body the three kernels above were compiled to other register numbers and
// instruction orders than the parent's (profiles/denoise_shards_spatial_codegen.txt).
template <int kR>
__global__ void __launch_bounds__(256) rt_denoise_prepare_spatial_shards_kernel(const float* __restrict__ hdr, const float4* __restrict__ feat, uint32_t W,
                                                                                uint32_t rows, uint32_t n, uint32_t m, const rtdn::ShardLayout L,
                                                                                const DenoiseParams P, float4* __restrict__ state, float4* __restrict__ g0,
                                                                                float4* __restrict__ g1) {
    constexpr uint32_t tw = rtdn::kTileW + 2u * kR, th = rtdn::kTileH + 2u * kR;
    __shared__ float4 ldsC[tw * th];
    __shared__ float4 ldsA[tw * th];
    __shared__ float4 ldsB[tw * th];
    const uint32_t tx = threadIdx.x & (rtdn::kTileW - 1u), ty = threadIdx.x / rtdn::kTileW;
    const int x0 = (int)(blockIdx.x * rtdn::kTileW), y0 = (int)(blockIdx.y * rtdn::kTileH);
    const int x = x0 + (int)tx, y = y0 + (int)ty;
    for (uint32_t ly = ty; ly < th; ly += rtdn::kTileH) {
        const int gy = y0 - kR + (int)ly;
        if (gy < 0 || gy >= (int)rows) continue;
        uint32_t shard, lr;  // located once per staged row: one division chain per row, not one per lane
        rowset_locate(L.blockRows, L.nshards, (uint32_t)gy, shard, lr);
        const size_t row = ((size_t)shard * L.rowsMax + lr) * W;
        for (uint32_t lx = tx; lx < tw; lx += rtdn::kTileW) {
            const int gx = x0 - kR + (int)lx;
            if (gx < 0 || gx >= (int)W) continue;
            const size_t q = row + (size_t)gx;
            const float h[3] = {hdr[3 * q], hdr[3 * q + 1], hdr[3 * q + 2]};
            const float4 fa = feat[2 * q], fb = feat[2 * q + 1];
            const float f[8] = {fa.x, fa.y, fa.z, fa.w, fb.x, fb.y, fb.z, fb.w};
            float c[3], g[8];
            denoise_prepare_mean(h, n, f, m, c, g);
            const uint32_t slot = ly * tw + lx;
            ldsC[slot] = make_float4(c[0], c[1], c[2], 0.0f);
            ldsA[slot] = make_float4(g[0], g[1], g[2], g[3]);
            ldsB[slot] = make_float4(g[4], g[5], g[6], g[7]);
        }
    }
    __syncthreads();
    if (x >= (int)W || y >= (int)rows) return;
    const uint32_t centre = (ty + (uint32_t)kR) * tw + tx + (uint32_t)kR;
    DenoiseState sp;
    float gp[8];
    unpack(ldsC[centre], ldsA[centre], ldsB[centre], sp, gp);
    SpatialSums S;
    spatial_begin(S);
#pragma unroll
    for (int a = 0; a <= 2 * kR; ++a) {
        const int dy = a - kR;
        const int qy = y + dy;
        if (qy < 0 || qy >= (int)rows) continue;
#pragma unroll
        for (int b = 0; b <= 2 * kR; ++b) {
            const int dx = b - kR;
            const int qx = x + dx;
            if (qx < 0 || qx >= (int)W) continue;
            const uint32_t slot = (uint32_t)((int)ty + kR + dy) * tw + (uint32_t)((int)tx + kR + dx);
            DenoiseState sq;
            float gq[8];
            unpack(ldsC[slot], ldsA[slot], ldsB[slot], sq, gq);
            spatial_tap(P, gp, sq.c, gq, S);
        }
    }
    const size_t p = (size_t)y * W + (size_t)x;
    state[p] = make_float4(sp.c[0], sp.c[1], sp.c[2], spatial_finish(S));
    g0[p] = make_float4(gp[0], gp[1], gp[2], gp[3]);
    g1[p] = make_float4(gp[4], gp[5], gp[6], gp[7]);
}

}  // namespace rtd

namespace rtdn {

// A state and its two guide planes as the kernels take them.
struct Planes {
    float4 *s, *g0, *g1;
};
static Planes PlanesOf(void* state, void* const guide[2]) { return Planes{static_cast<float4*>(state), static_cast<float4*>(guide[0]), static_cast<float4*>(guide[1])}; }

// The spatial prepare pass into the three planes (radius 1..3: the caller's check).  parts: NULL, or the layout the inputs are read
// through (the parts form takes n from the strips: committed is not read).
static int LaunchPrepareSpatial(hipStream_t st, const Strips& s, const ShardLayout* parts, const rtd::DenoiseParams& P, uint32_t radius, const uint32_t* committed,
                                const Planes& o) {
    const dim3 grid((s.W + kTileW - 1u) / kTileW, (s.rows + kTileH - 1u) / kTileH);
    const float4* feat = reinterpret_cast<const float4*>(s.feat);
    if (radius < 1u || radius > 3u) return (int)hipErrorInvalidValue;
    if (parts && radius == 1u)
        hipLaunchKernelGGL((rtd::rt_denoise_prepare_spatial_shards_kernel<1>), grid, dim3(256), 0, st, s.hdr, feat, s.W, s.rows, s.n, s.m, *parts, P, o.s, o.g0, o.g1);
    else if (parts && radius == 2u)
        hipLaunchKernelGGL((rtd::rt_denoise_prepare_spatial_shards_kernel<2>), grid, dim3(256), 0, st, s.hdr, feat, s.W, s.rows, s.n, s.m, *parts, P, o.s, o.g0, o.g1);
    else if (parts)
        hipLaunchKernelGGL((rtd::rt_denoise_prepare_spatial_shards_kernel<3>), grid, dim3(256), 0, st, s.hdr, feat, s.W, s.rows, s.n, s.m, *parts, P, o.s, o.g0, o.g1);
    else if (radius == 1u)
        hipLaunchKernelGGL((rtd::rt_denoise_prepare_spatial_kernel<1>), grid, dim3(256), 0, st, s.hdr, feat, s.W, s.rows, s.n, s.m, committed, P, o.s, o.g0, o.g1);
    else if (radius == 2u)
        hipLaunchKernelGGL((rtd::rt_denoise_prepare_spatial_kernel<2>), grid, dim3(256), 0, st, s.hdr, feat, s.W, s.rows, s.n, s.m, committed, P, o.s, o.g0, o.g1);
    else if (radius == 3u)
        hipLaunchKernelGGL((rtd::rt_denoise_prepare_spatial_kernel<3>), grid, dim3(256), 0, st, s.hdr, feat, s.W, s.rows, s.n, s.m, committed, P, o.s, o.g0, o.g1);
    else
        return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

// The levels over the prepared state and guides of a W x rows picture in image order.
// (first: level 0's input -- the strips' own state[0] and guides, or the temporal form's new history, which no level may overwrite)
static int LaunchLevels(hipStream_t st, const Strips& s, const Planes& first, const rtd::DenoiseParams& P, int stageKnob, uint32_t forms[rtd::kDenoiseMaxLevels]) {
    float4* state[2] = {static_cast<float4*>(s.state[0]), static_cast<float4*>(s.state[1])};
    const float4 *g0 = first.g0, *g1 = first.g1;
    hipError_t e = hipSuccess;
    const dim3 grid((s.W + kTileW - 1u) / kTileW, (s.rows + kTileH - 1u) / kTileH);
    for (uint32_t l = 0; l < P.levels; ++l) {
        const uint32_t step = 1u << l;
        const bool staged = Staged(step, stageKnob), last = l + 1u == P.levels;
        const size_t lds = staged ? StageBytes(step) : 0;
        const float4* in = l == 0 ? first.s : state[l & 1u];
        float4* out = state[(l + 1u) & 1u];
        if (staged && last)
            hipLaunchKernelGGL((rtd::rt_atrous_kernel<true, true>), grid, dim3(256), lds, st, in, g0, g1, s.W, s.rows, step, P, out, s.den, s.denVar);
        else if (staged)
            hipLaunchKernelGGL((rtd::rt_atrous_kernel<true, false>), grid, dim3(256), lds, st, in, g0, g1, s.W, s.rows, step, P, out, s.den, s.denVar);
        else if (last)
            hipLaunchKernelGGL((rtd::rt_atrous_kernel<false, true>), grid, dim3(256), lds, st, in, g0, g1, s.W, s.rows, step, P, out, s.den, s.denVar);
        else
            hipLaunchKernelGGL((rtd::rt_atrous_kernel<false, false>), grid, dim3(256), lds, st, in, g0, g1, s.W, s.rows, step, P, out, s.den, s.denVar);
        e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
        forms[l] = staged ? kFormStaged : kFormDirect;
    }
    return 0;
}

static rtd::TemporalArgs TemporalArgsOf(const Strips& s, const Temporal& t) {
    rtd::TemporalArgs A{};
    A.hdr = s.hdr;
    A.sq = s.sq;
    A.feat = reinterpret_cast<const float4*>(s.feat);
    A.ids = t.ids;
    A.npix = s.W * s.rows;
    A.n = s.n;
    A.m = s.m;
    A.hasPrev = t.hasPrev ? 1u : 0u;
    A.G = t.geom;
    A.C = t.cam;
    A.Cp = t.camPrev;
    A.T = t.params;
    const Planes h = PlanesOf(t.prev.state, t.prev.guide), o = PlanesOf(t.next.state, t.next.guide);
    A.hS = h.s;
    A.hG0 = h.g0;
    A.hG1 = h.g1;
    A.hId = t.prev.ids;
    A.hLen = t.prev.len;
    A.oS = o.s;
    A.oG0 = o.g0;
    A.oG1 = o.g1;
    A.oId = t.next.ids;
    A.oLen = t.next.len;
    A.target = t.target;
    return A;
}

int Launch(void* stream, const Job& j, const rtd::DenoiseParams& P, int stageKnob, uint32_t forms[rtd::kDenoiseMaxLevels]) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Strips& s = j.strips;
    const uint32_t npix = s.W * s.rows;
    const dim3 grid((npix + 255u) / 256u), block(256);
    for (uint32_t l = 0; l < rtd::kDenoiseMaxLevels; ++l) forms[l] = kFormNone;
    const Planes own = PlanesOf(s.state[0], s.guide);
    Planes first = own;  // what the levels start from: the pass's outputs
    if (j.spatialRadius != 0)
        if (const int e = LaunchPrepareSpatial(st, s, j.parts, P, j.spatialRadius, j.committed, own)) return e;
    if (j.temporal) {
        const rtd::TemporalArgs A = TemporalArgsOf(s, *j.temporal);
        const bool bilinear = j.temporal->fetch == rtd::kTemporalFetchBilinear;
        if (j.parts && j.spatialRadius != 0)
            hipLaunchKernelGGL((bilinear ? rtd::rt_denoise_prepared_shards_temporal_bilinear_kernel : rtd::rt_denoise_prepared_shards_temporal_kernel), grid, block, 0,
                               st, rtd::TemporalPreparedShardArgs{A, {own.s, own.g0, own.g1}, *j.parts});
        else if (j.parts)
            hipLaunchKernelGGL((bilinear ? rtd::rt_denoise_prepare_shards_temporal_bilinear_kernel : rtd::rt_denoise_prepare_shards_temporal_kernel), grid, block, 0, st,
                               rtd::TemporalShardArgs{A, *j.parts});
        else if (j.spatialRadius != 0)
            hipLaunchKernelGGL((bilinear ? rtd::rt_denoise_prepared_temporal_bilinear_kernel : rtd::rt_denoise_prepared_temporal_kernel), grid, block, 0, st,
                               rtd::TemporalPreparedArgs{A, {own.s, own.g0, own.g1}});
        else
            hipLaunchKernelGGL((bilinear ? rtd::rt_denoise_prepare_temporal_bilinear_kernel : rtd::rt_denoise_prepare_temporal_kernel), grid, block, 0, st, A);
        first = Planes{A.oS, A.oG0, A.oG1};
    } else if (j.parts && j.spatialRadius == 0) {
        hipLaunchKernelGGL(rtd::rt_denoise_prepare_shards_kernel, grid, block, 0, st, s.hdr, s.sq, reinterpret_cast<const float4*>(s.feat), s.W, npix,
                           j.parts->rowsMax, j.parts->blockRows, j.parts->nshards, s.n, s.m, own.s, own.g0, own.g1);
    } else if (j.spatialRadius == 0) {
        hipLaunchKernelGGL(rtd::rt_denoise_prepare_kernel, grid, block, 0, st, s.hdr, s.sq, reinterpret_cast<const float4*>(s.feat), npix, s.n, s.m, own.s, own.g0,
                           own.g1);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return LaunchLevels(st, s, first, P, stageKnob, forms);
}

}  // namespace rtdn
