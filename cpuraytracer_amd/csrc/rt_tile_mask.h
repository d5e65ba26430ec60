// rt_tile_mask.h -- per-tile candidate masks for the flat scan's PRIMARY rays (DESIGN.md §5.2 "tile masks").
//
// The 64 primary rays a wave generates together are one tile of the sample buffer (64 consecutive local pixels) at one
// sample index.  Which groups such a ray can reach is a property of (scene, camera, image size, row set), not of the
// sample: rt_tile_mask_kernel evaluates it once per accumulation start and the scan of a fresh tile takes the four bitmap
// words from the table instead of running the matrix-core filter (rt_scan.h scan_list_mfma, tileMask).
//
// Soundness.  Camera::GetRay (rt_params.h camera_get_ray): the origin is O = camO + rdx mx + rdy my with
// |(rdx, rdy)| <= 0.5 |aperture| for every lens point of the unit disc, so |O - camO| <= rhoL = 0.5 |aperture| max(|mx|, |my|)
// sqrt(2); the ray passes through F = camO + focal normalize(pp - camO), pp on the run's patch of the image plane.  For a
// run of pixels of one row, Fc is the focal point of the patch's centre and rhoF = max |F - Fc| over the corners of the
// patch widened by one pixel on every side: the directions within a given angle of the centre's form a cone, whose
// section with the image plane is convex, so the largest angle over the (convex) patch is at a corner, and |F - Fc| grows
// with the angle.  The point of the ray at parameter lambda >= 0, (1 - lambda) O + lambda F, then lies within
// |1 - lambda| rhoL + lambda rhoF of the axis point camO + lambda (Fc - camO).  A group's bound (C, R) can hold a point of
// such a ray only if  |C - axis(lambda)| <= R + |1 - lambda| rhoL + lambda rhoF  for some lambda >= 0.  Both sides are
// non-negative and the right side is linear on [0, 1] and on [1, inf), so on each piece the condition is a quadratic
// inequality q(lambda) <= 0 whose minimum is at an end of the piece or at the vertex: closed form, evaluated in f64.
// R is the filter's own inflated radius Rf (the host folds the exact path's rounding into it), plus the
// bound of the filter's per-ray term 2 K eps |o|^2 at |o| <= |camO| + rhoL, plus a geometric slack of 1e-3 Rf +
// 1e-4 (|camO| + |C| + Rf) -- three orders of magnitude above the f32 rounding of the ray generation, which this f64
// restatement does not reproduce.  Every comparison is written so that a NaN sets the bit; a degenerate camera (focal <= 0,
// a zero basis vector, a patch behind the centre direction) yields "no mask" for the tile.
#pragma once

#include <stdint.h>

#include "../../include/rt_api.h"
#include "rt_device_math.h"

namespace rtd {

// per tile: cw0..cw3 | flags (bit 0: valid) | candidate groups (read by tests and reports only) | two words of padding, so that a
// tile's record is one aligned 32-byte piece
constexpr uint32_t kTileMaskWords = 8;
// Tiles with more candidate groups than this keep the matrix-core filter: there the per-ray filter, which finds 1-2 groups per ray,
// is cheaper than phase A over a long common list.  Measured (profiles/primary_mask_ab.txt; ms of C2 / C4): limit 4: 11.89 / 100.0,
// 8: 11.67 / 99.4, 12: 11.66 / 98.9, 16: 11.65 / 100.2, 48 (every tile masked): 11.75 / 100.9.  At 16, 2.4 % of C2's tiles and
// 6.3 % of C4's fall back; at 12, 19 % of C2's would.
constexpr uint32_t kTileMaskLimitDefault = 16;
constexpr double kTileMaskPerRay = 2.0 * 4096.0 * 5.9604644775390625e-8;  // 2 K eps (rt_scan.h kMarginK)

struct TileMaskCam {
    float cam_o[3], cam_x[3], cam_y[3], cam_oip[3];
    float aperture, focal;
    uint32_t W, H;
};

template <class A>
RT_DEV TileMaskCam tile_mask_cam(const A& o, const A& x, const A& y, const A& oip, float aperture, float focal, uint32_t W, uint32_t H) {
    TileMaskCam c;
    for (int k = 0; k < 3; ++k) {
        c.cam_o[k] = o[k]; c.cam_x[k] = x[k]; c.cam_y[k] = y[k]; c.cam_oip[k] = oip[k];
    }
    c.aperture = aperture; c.focal = focal; c.W = W; c.H = H;
    return c;
}
// flags word of a tile's record: bit 0 = the tile has a mask (the construction applied and the mask is not too loose to pay)
RT_DEV uint32_t tile_mask_flags(bool bad, uint32_t candidates, uint32_t limit) { return (!bad && candidates <= limit) ? 1u : 0u; }

struct TileCone {
    double o[3], D[3];   // axis(lambda) = o + lambda D, D = Fc - camO
    double rhoL, rhoF, normO;
    bool ok;
};

RT_DEV double tm_len3(const double v[3]) { return __builtin_sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// focal point of image-plane coordinates (uvx, uvy), relative to camO; false when the direction is degenerate
RT_DEV bool tm_focal_offset(const TileMaskCam& c, double uvx, double uvy, double out[3]) {
    const double ndcx = 2.0 * uvx - 1.0, ndcy = -2.0 * uvy + 1.0;
    double v[3];
    for (int k = 0; k < 3; ++k) v[k] = ((double)c.cam_oip[k] + ndcx * (double)c.cam_x[k] + ndcy * (double)c.cam_y[k]) - (double)c.cam_o[k];
    const double l = tm_len3(v);
    if (!(l > 0.0) || !(l < 1e300)) return false;
    for (int k = 0; k < 3; ++k) out[k] = (double)c.focal * v[k] / l;
    return true;
}

// The cone of every primary ray of the pixels i0..i1 (inclusive) of global row j.
RT_DEV TileCone tile_run_cone(const TileMaskCam& c, uint32_t i0, uint32_t i1, uint32_t j) {
    TileCone t;
    t.ok = false;
    t.rhoL = t.rhoF = t.normO = 0.0;
    for (int k = 0; k < 3; ++k) t.o[k] = t.D[k] = 0.0;
    const double W = (double)c.W, H = (double)c.H;
    const double mx[3] = {(double)c.cam_x[0], (double)c.cam_x[1], (double)c.cam_x[2]};
    const double my[3] = {(double)c.cam_y[0], (double)c.cam_y[1], (double)c.cam_y[2]};
    const double lx = tm_len3(mx), ly = tm_len3(my);
    if (!(c.focal > 0.f) || !(lx > 0.0) || !(ly > 0.0) || !(W > 0.0) || !(H > 0.0)) return t;
    const double u0 = ((double)i0 - 1.0) / W, u1 = ((double)i1 + 2.0) / W;
    const double v0 = ((double)j - 1.0) / H, v1 = ((double)j + 2.0) / H;
    if (!tm_focal_offset(c, 0.5 * (u0 + u1), 0.5 * (v0 + v1), t.D)) return t;
    double rho = 0.0;
    for (int q = 0; q < 4; ++q) {
        double f[3];
        if (!tm_focal_offset(c, (q & 1) ? u1 : u0, (q & 2) ? v1 : v0, f)) return t;
        if (!(f[0] * t.D[0] + f[1] * t.D[1] + f[2] * t.D[2] > 0.0)) return t;  // more than a right angle from the centre
        const double d[3] = {f[0] - t.D[0], f[1] - t.D[1], f[2] - t.D[2]};
        const double l = tm_len3(d);
        if (!(l <= rho)) rho = l;  // (a NaN sticks)
    }
    const double ap = c.aperture < 0.f ? -(double)c.aperture : (double)c.aperture;
    t.rhoL = 0.5 * ap * (lx > ly ? lx : ly) * 1.4142135623730951;
    t.rhoF = rho;
    for (int k = 0; k < 3; ++k) t.o[k] = (double)c.cam_o[k];
    t.normO = tm_len3(t.o);
    t.ok = t.rhoL == t.rhoL && t.rhoF == t.rhoF && t.rhoL < 1e300 && t.rhoF < 1e300 && t.normO < 1e300;
    return t;
}

// Reach of the cone's rays at parameter lambda: every point (1 - lambda) O + lambda F lies this close to axis(lambda).
RT_DEV double tile_cone_reach(const TileCone& t, double lambda) { return (lambda < 1.0 ? 1.0 - lambda : lambda - 1.0) * t.rhoL + lambda * t.rhoF; }

// min over the piece [l0, l1] (l1 < 0: unbounded) of |w - lambda D|^2 - (alpha + beta lambda)^2 is <= 0 (or not provably > 0)
RT_DEV bool tm_piece_reached(double DD, double wD, double ww, double alpha, double beta, double l0, double l1) {
    const double A2 = DD - beta * beta, B = wD + alpha * beta, C0 = ww - alpha * alpha;
    const double q0 = (A2 * l0 - 2.0 * B) * l0 + C0;
    if (!(q0 > 0.0)) return true;
    if (l1 >= 0.0) {
        const double q1 = (A2 * l1 - 2.0 * B) * l1 + C0;
        if (!(q1 > 0.0)) return true;
    } else if (!(A2 > 0.0)) {
        return true;  // the reach grows at least as fast as the axis moves away
    }
    if (A2 > 0.0) {
        const double lv = B / A2;
        if (lv > l0 && (l1 < 0.0 || lv < l1)) {
            const double qv = C0 - B * lv;
            if (!(qv > 0.0)) return true;
        }
    }
    return false;
}

// The filter radius of a group bound (Cx, Cy, Cz, |C|^2 - Rf^2) as the masks use it (header comment).
RT_DEV double tile_group_radius(const TileCone& t, const float b[4]) {
    const double C[3] = {(double)b[0], (double)b[1], (double)b[2]};
    const double cc = C[0] * C[0] + C[1] * C[1] + C[2] * C[2];
    double rf2 = cc - (double)b[3];
    if (!(rf2 > 0.0)) rf2 = 0.0;
    const double rf = __builtin_sqrt(rf2), omax = t.normO + t.rhoL;
    return __builtin_sqrt(rf2 + kTileMaskPerRay * omax * omax) + 1e-3 * rf + 1e-4 * (t.normO + __builtin_sqrt(cc) + rf);
}

// May a primary ray of the cone have a point inside the group's bound?
RT_DEV bool tile_cone_reaches(const TileCone& t, const float b[4]) {
    const double R = tile_group_radius(t, b);
    const double w[3] = {(double)b[0] - t.o[0], (double)b[1] - t.o[1], (double)b[2] - t.o[2]};
    const double DD = t.D[0] * t.D[0] + t.D[1] * t.D[1] + t.D[2] * t.D[2];
    const double wD = w[0] * t.D[0] + w[1] * t.D[1] + w[2] * t.D[2];
    const double ww = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    if (!(R == R) || !(ww == ww)) return true;
    return tm_piece_reached(DD, wD, ww, R + t.rhoL, t.rhoF - t.rhoL, 0.0, 1.0) ||
           tm_piece_reached(DD, wD, ww, R - t.rhoL, t.rhoF + t.rhoL, 1.0, -1.0);
}

// Group g of tile `tile` (local pixels 64 tile .. 64 tile + 63 of a strip of width W under row set rs): 1 = candidate,
// 0 = no primary ray of the tile reaches it, -1 = the construction does not apply (no mask for this tile).  A tile that
// wraps a row end, or whose rows are not adjacent, is the union of its row runs.
RT_DEV int tile_group_reached(const TileMaskCam& c, const rt_rowset& rs, uint32_t tile, const float b[4]) {
    const uint32_t p0 = tile << 6, p1 = p0 + 63u;
    int reached = 0;
    for (uint32_t lr = p0 / c.W; lr <= p1 / c.W; ++lr) {
        const uint32_t r0 = lr * c.W;
        const uint32_t i0 = (p0 > r0 ? p0 : r0) - r0, i1 = (p1 < r0 + c.W - 1u ? p1 : r0 + c.W - 1u) - r0;
        const uint32_t lb = lr / rs.block_rows;
        const uint32_t j = rs.first_row + (lb * rs.nshards + rs.shard) * rs.block_rows + (lr - lb * rs.block_rows);
        const TileCone t = tile_run_cone(c, i0, i1, j);
        if (!t.ok) return -1;
        if (tile_cone_reaches(t, b)) reached = 1;
    }
    return reached;
}

// ---------------------------------------------------------------- per-tile sphere lists (DESIGN.md §5.2 "sphere lists")
// For a tile with a mask, the SCAN ENTRIES (spheres, not groups) a primary ray of the tile can reach: the same cone test on the
// entry's one-sphere bound, which is the sphere-level filter's own (rt_scan.h kMarginKLeaf: centre, |c|^2 - rf^2 with the exact
// path's rounding folded into rf), with the per-ray term and the geometric slack of tile_group_radius -- whose per-ray term is the
// group level's 2 * 4096 eps |o|^2, above the one-sphere level's 2 * 64 eps |o|^2.  Only members of the tile's candidate groups are
// tested (a sphere with an accepted root has its group's bit set: the masks' soundness) and padding entries (orig = 0xffffffff)
// are never listed.  The scan of such a tile tests each of its 64 rays against the listed spheres directly (rt_scan.h
// scan_tile_spheres) -- no candidate words, no pooled resolve.  A record is kTileSphereHalfs 16-bit values, 128 bytes: [0] = the
// count, or kTileSphereNone (no list: no mask, or more spheres than the limit); [1 + k] = the k-th entry, ascending.
constexpr uint32_t kTileSphereHalfs = 64;
constexpr uint32_t kTileSphereMax = kTileSphereHalfs - 1u;  // the most a record holds (and a lane per entry in the scan)
constexpr uint32_t kTileSphereNone = 0xffffu;
// Tiles with more listed spheres than this keep the masked pooled resolve.  Measured (profiles/primary_spheres_ab.txt; ms of C2 / C4,
// parent 11.74 / 100.04): limit 0 (off): 11.79 / 100.41, 8: 11.01 / 94.46, 16: 10.57 / 90.67, 24: 10.48 / 89.03, 32: 10.48 / 88.96,
// 63: 10.50 / 88.87.  The direct loop costs ~45 issue slots per listed sphere at 64 of 64 lanes, so long lists still beat the pools.
constexpr uint32_t kTileSphereLimitDefault = 24;

// Is scan entry e (one-sphere bound lb, original index og) listed for the tile?  groupReached: tile_group_reached of its group.
RT_DEV bool tile_entry_listed(const TileMaskCam& c, const rt_rowset& rs, uint32_t tile, int groupReached, uint32_t og, const float lb[4]) {
    if (groupReached <= 0 || og == 0xffffffffu) return false;
    return tile_group_reached(c, rs, tile, lb) != 0;
}

// Where group g sits in the scan's candidate words (rt_scan.h: bit N from the top of word k is group kBase[k] + N + (N & 16),
// kBase = 0, 64, 16, 80).
RT_DEV void tile_mask_slot(uint32_t g, uint32_t& word, uint32_t& bit) {
    const uint32_t r = g & 63u, q = r >> 4;
    word = (g >> 6) + 2u * (q & 1u);
    bit = 0x80000000u >> ((r & 15u) + 16u * (q >> 1));
}

}  // namespace rtd
