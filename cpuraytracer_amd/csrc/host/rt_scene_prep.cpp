// rt_scene_prep.cpp -- scene preparation on the host (rt_scene_prep.h) and the C entries of include/rt_api.h that need no
// device.  Plain C++17, compiled with -ffp-contract=off like the kernels: every table below is a function of the input's bits.
#include "rt_scene_prep.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "../rt_features.h"
#include "../rt_noise.h"
#include "../rt_tile_mask.h"

namespace rtprep {

namespace {
thread_local std::string g_err;
F4 MakeF4(float x, float y, float z, float w) { return F4{x, y, z, w}; }
}  // namespace

int Fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
const char* LastError() { return g_err.c_str(); }

uint32_t EnvU32(const char* name, uint32_t dflt) {
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    return (uint32_t)std::strtoul(v, nullptr, 10);
}

PrepOptions PrepOptions::FromEnv() {
    PrepOptions o;
    o.treeTop = EnvU32("RT_TREE_TOP", 128);
    if (o.treeTop < 4 || o.treeTop > 128) o.treeTop = 128u;
    o.shadowGrid = EnvU32("RT_SHADOW_GRID", 1) != 0;
    o.shadowCellsGlobal = EnvU32("RT_SHADOW_CELLS", 256u);
    o.sgSph = EnvU32("RT_SG_SPH", 0u) != 0u;
    if (const char* e = std::getenv("RT_SINGLE_DIRECT")) o.singleDirect = std::atoi(e) != 0;
    if (const char* e = std::getenv("RT_GRID_DENSITY")) o.gridDensity = std::max(0.1, std::atof(e));
    if (const char* g = std::getenv("RT_GRID")) {
        o.grid = g[0] != '0';
        o.gridForce = g[0] == '2';
    }
    o.bigApart = std::getenv("RT_ALWAYS_BIG") == nullptr;
    o.treeBox = std::getenv("RT_TREE_BOX_OFF") == nullptr;
    return o;
}

uint32_t RowsetLocalRows(rt_rowset rs) {
    if (rs.block_rows == 0 || rs.nshards == 0 || rs.shard >= rs.nshards) return 0;
    uint32_t rows = 0;
    const uint32_t nblocks = (rs.num_rows + rs.block_rows - 1) / rs.block_rows;
    for (uint32_t b = rs.shard; b < nblocks; b += rs.nshards) {
        const uint32_t r0 = b * rs.block_rows;
        const uint32_t left = rs.num_rows - r0;
        rows += left < rs.block_rows ? left : rs.block_rows;
    }
    return rows;
}

// ---------------------------------------------------------------------------------- scene layout

// The spheres as the bounds see them: radius |r|.  A negative radius is legal input (the reference's Sphere::Intersect tests r * r
// and divides the normal by r: the inward normal of a hollow sphere), and the surface it describes is that of |r|.  Everything below
// that ENCLOSES a sphere or compares sphere sizes (BoundOf, EnclosingRadius, BoxOf, the grid builder, the big-sphere split, the
// shadow index) reads this copy; the scan entry's r * r has the same bits either way, and the radius table the normals divide by
// is filled from the caller's signed radii (PrepareScene).
static std::vector<rt_sphere> WithAbsRadii(const rt_sphere* sp, uint32_t n) {
    std::vector<rt_sphere> out(sp, sp + n);
    for (rt_sphere& s : out) s.r = std::fabs(s.r);
    return out;
}

bool AllFinite(const rt_sphere* sp, uint32_t n, uint32_t* which) {
    for (uint32_t k = 0; k < n; ++k)
        if (!std::isfinite(sp[k].cx) || !std::isfinite(sp[k].cy) || !std::isfinite(sp[k].cz) || !std::isfinite(sp[k].r)) {
            if (which) *which = k;
            return false;
        }
    return true;
}

const char* MaterialFault(const rt_material& m) {
    if (m.type > 3u) return "type";
    if (m.tex_type > 1u) return "tex_type";
    const bool glass = m.type == RT_MAT_DIELECTRIC_TRANSPARENT, emissive = m.type == RT_MAT_EMISSIVE;
    if (!emissive && !std::isfinite(m.smoothness)) return "smoothness";
    if (glass && !std::isfinite(m.ior)) return "ior";
    if (emissive && !std::isfinite(m.luminance)) return "luminance";
    if (glass) return nullptr;  // a glass sphere has no texture
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(m.rgb0[k])) return "rgb0";
    if (m.tex_type != RT_TEX_CHECKER) return nullptr;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(m.rgb1[k])) return "rgb1";
    // (int)(tiling * u) with u = 0.5 n + 0.5, |n| within a few ulp of 1: the product stays inside int (NaN fails the comparison)
    if (!(std::fabs(m.tiling) <= 1073741824.0f)) return "tiling";
    return nullptr;
}

bool MaterialsInDomain(const rt_material* mats, uint32_t n, uint32_t* which, const char** field) {
    for (uint32_t k = 0; k < n; ++k)
        if (const char* f = MaterialFault(mats[k])) {
            if (which) *which = k;
            if (field) *field = f;
            return false;
        }
    return true;
}

std::string MaterialFaultMessage(const char* who, const std::string& what, const rt_material& m, const char* field) {
    std::string why;
    if (!std::strcmp(field, "type")) why = "type = " + std::to_string(m.type) + " (rt_material_type is 0..3)";
    else if (!std::strcmp(field, "tex_type")) why = "tex_type = " + std::to_string(m.tex_type) + " (rt_texture_type is 0..1)";
    else if (!std::strcmp(field, "tiling")) why = "tiling is not finite or beyond 2^30 in magnitude";
    else why = std::string(field) + " is not finite";
    return std::string(who) + ": the material of " + what + " is outside the material domain: " + why;
}

// Conservative bounding sphere of a set of spheres, in the filter's (C, |C|^2 - Rf^2) form.
static F4 BoundOf(const rt_sphere* sp, const std::vector<uint32_t>& ids, float* normOut, float marginK) {
    if (ids.empty()) return MakeF4(0.f, 0.f, 0.f, 1e30f);  // never a candidate
    const double kEps = (double)marginK * 5.9604644775390625e-08;  // K * eps: K is that of the unit testing this bound (rt_scan.h)
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (uint32_t k : ids) {
        const double c[3] = {sp[k].cx, sp[k].cy, sp[k].cz};
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], c[a] - (double)sp[k].r);
            hi[a] = std::max(hi[a], c[a] + (double)sp[k].r);
        }
    }
    // centre: the enclosing radius max_i(|c_i - C| + r_i) is convex in C, so a pattern search from the box centre
    // (axis steps, halved when none improves) finds the near-minimal enclosing sphere, typically 5-15 % smaller than the
    // box-centred one.  Any centre is valid: R below is measured from the centre actually used.  The bound centre is the
    // FLOAT the device will use, so its rounding is inside s_i below.
    double cc[3] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])};
    if (ids.size() > 1) {
        auto reachOf = [&](const double c[3]) {
            double far = 0.0;
            for (uint32_t k : ids) {
                const double dx = sp[k].cx - c[0], dy = sp[k].cy - c[1], dz = sp[k].cz - c[2];
                far = std::max(far, std::sqrt(dx * dx + dy * dy + dz * dz) + (double)sp[k].r);
            }
            return far;
        };
        double best = reachOf(cc);
        double step = 0.25 * best;
        for (int it = 0; it < 400 && step > 1e-7 * best; ++it) {
            bool improved = false;
            for (int ax = 0; ax < 3; ++ax)
                for (int sgn = -1; sgn <= 1; sgn += 2) {
                    double t[3] = {cc[0], cc[1], cc[2]};
                    t[ax] += sgn * step;
                    const double r = reachOf(t);
                    if (r < best) {
                        best = r;
                        cc[0] = t[0]; cc[1] = t[1]; cc[2] = t[2];
                        improved = true;
                    }
                }
            if (!improved) step *= 0.5;
        }
    }
    const float Cf[3] = {(float)cc[0], (float)cc[1], (float)cc[2]};
    double R = 0, smax = 0;
    for (uint32_t k : ids) {
        const double dx = sp[k].cx - (double)Cf[0], dy = sp[k].cy - (double)Cf[1], dz = sp[k].cz - (double)Cf[2];
        const double si = std::sqrt(dx * dx + dy * dy + dz * dz);
        smax = std::max(smax, si);
        R = std::max(R, si + (double)sp[k].r);
    }
    const double C2 = (double)Cf[0] * Cf[0] + (double)Cf[1] * Cf[1] + (double)Cf[2] * Cf[2];
    const double Cn = std::sqrt(C2);
    const double Rf2 = R * R * (1.0 + 1e-5) + 0.01 * smax * smax + kEps * (2.0 * (Cn + R) * (Cn + R) + R * R);
    float w = (float)(C2 - Rf2);
    w = std::nextafterf(std::nextafterf(w, -INFINITY), -INFINITY);  // err towards "more candidates"
    if (normOut) *normOut = std::max(*normOut, (float)((Cn + R) * 1.001));
    return MakeF4(Cf[0], Cf[1], Cf[2], w);
}

// Enclosing radius of a set of spheres about its near-optimal centre (the same pattern search BoundOf uses).
static double EnclosingRadius(const rt_sphere* sp, const uint32_t* ids, size_t n) {
    if (n == 0) return 0.0;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (size_t q = 0; q < n; ++q) {
        const rt_sphere& s = sp[ids[q]];
        const double c[3] = {s.cx, s.cy, s.cz};
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], c[a] - (double)s.r);
            hi[a] = std::max(hi[a], c[a] + (double)s.r);
        }
    }
    double cc[3] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])};
    auto reachOf = [&](const double c[3]) {
        double far = 0.0;
        for (size_t q = 0; q < n; ++q) {
            const rt_sphere& s = sp[ids[q]];
            const double dx = s.cx - c[0], dy = s.cy - c[1], dz = s.cz - c[2];
            far = std::max(far, std::sqrt(dx * dx + dy * dy + dz * dz) + (double)s.r);
        }
        return far;
    };
    double best = reachOf(cc);
    if (n == 1) return best;
    double step = 0.25 * best;
    for (int it = 0; it < 60 && step > 1e-4 * best; ++it) {
        bool improved = false;
        for (int ax = 0; ax < 3; ++ax)
            for (int sgn = -1; sgn <= 1; sgn += 2) {
                double t[3] = {cc[0], cc[1], cc[2]};
                t[ax] += sgn * step;
                const double r = reachOf(t);
                if (r < best) { best = r; cc[0] = t[0]; cc[1] = t[1]; cc[2] = t[2]; improved = true; }
            }
        if (!improved) step *= 0.5;
    }
    return best;
}

// Local refinement of the k-d groups: for pairs of spatially neighbouring groups, redistribute their (at most eight)
// members into two groups of the same sizes when that lowers R1^2 + R2^2 (the filter's candidate count per ray is
// proportional to the summed squared bound radii).  Groups keep their positions in the list, so the hierarchy above
// them (consecutive quadruples) stays spatially coherent.  Skipped for very large scenes (upload time).
static void RefineGroups(const rt_sphere* sp, std::vector<std::vector<uint32_t>>& groups) {
    const size_t G = groups.size();
    if (G < 2 || G > 4096) return;
    std::vector<double> R(G, 0.0);
    std::vector<std::array<double, 3>> C(G);
    auto update = [&](size_t g) {
        R[g] = EnclosingRadius(sp, groups[g].data(), groups[g].size());
        double c[3] = {0, 0, 0};
        for (uint32_t k : groups[g]) { c[0] += sp[k].cx; c[1] += sp[k].cy; c[2] += sp[k].cz; }
        const double inv = groups[g].empty() ? 0.0 : 1.0 / (double)groups[g].size();
        C[g] = {c[0] * inv, c[1] * inv, c[2] * inv};
    };
    for (size_t g = 0; g < G; ++g) update(g);
    for (int sweep = 0; sweep < 4; ++sweep) {
        bool any = false;
        for (size_t g = 0; g < G; ++g) {
            if (groups[g].size() < 2) continue;  // singletons (big spheres) and padding stay as they are
            for (size_t h = g + 1; h < G; ++h) {
                if (groups[h].size() < 2) continue;
                const double dx = C[g][0] - C[h][0], dy = C[g][1] - C[h][1], dz = C[g][2] - C[h][2];
                const double reachSum = R[g] + R[h];
                if (dx * dx + dy * dy + dz * dz > reachSum * reachSum) continue;  // bounds do not even touch
                const size_t ng = groups[g].size(), nh = groups[h].size(), nt = ng + nh;
                uint32_t all[8];
                for (size_t q = 0; q < ng; ++q) all[q] = groups[g][q];
                for (size_t q = 0; q < nh; ++q) all[ng + q] = groups[h][q];
                double bestCost = R[g] * R[g] + R[h] * R[h];
                uint32_t bestMask = 0;
                for (uint32_t mask = 1; mask < (1u << nt); ++mask) {
                    if ((size_t)__builtin_popcount(mask) != ng || !(mask & 1u)) continue;  // member 0 stays in g: no mirror splits
                    uint32_t a[8], b[8];
                    size_t na = 0, nb = 0;
                    for (size_t q = 0; q < nt; ++q) ((mask >> q) & 1u ? a[na++] : b[nb++]) = all[q];
                    const double ra = EnclosingRadius(sp, a, na);
                    if (ra * ra >= bestCost) continue;
                    const double rb = EnclosingRadius(sp, b, nb);
                    const double cost = ra * ra + rb * rb;
                    if (cost < bestCost * (1.0 - 1e-9)) { bestCost = cost; bestMask = mask; }
                }
                if (bestMask != 0 && bestMask != ((1u << ng) - 1u)) {
                    std::vector<uint32_t> a, b;
                    for (size_t q = 0; q < nt; ++q) ((bestMask >> q) & 1u ? a : b).push_back(all[q]);
                    groups[g] = a;
                    groups[h] = b;
                    update(g);
                    update(h);
                    any = true;
                }
            }
        }
        if (!any) break;
    }
}

// Box around a set of spheres (radii included) and the constants of the per-ray padding (rt_scan.h): treeBox[0..5] = lo, hi,
// [6] = max |coordinate|, [7] = 3 A^2 (A = max |c| + r), [8] = 1 / (2 r_min).
static bool BoxOf(const rt_sphere* sp, const std::vector<uint32_t>& ids, float treeBox[9]) {
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    double A = 0.0, rmin = 1e300;
    for (uint32_t k : ids) {
        const double c[3] = {sp[k].cx, sp[k].cy, sp[k].cz};
        A = std::max(A, std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) + (double)sp[k].r);
        rmin = std::min(rmin, (double)sp[k].r);
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], c[a] - (double)sp[k].r * (1.0 + 1e-5));
            hi[a] = std::max(hi[a], c[a] + (double)sp[k].r * (1.0 + 1e-5));
        }
    }
    if (!(lo[0] <= hi[0])) return false;
    double am = 0;
    for (int a = 0; a < 3; ++a) {
        treeBox[a] = std::nextafterf((float)lo[a], -INFINITY);
        treeBox[3 + a] = std::nextafterf((float)hi[a], INFINITY);
        am = std::max(am, std::max(std::fabs(lo[a]), std::fabs(hi[a])));
    }
    treeBox[6] = (float)(am * 1.001);
    treeBox[7] = (float)(3.0 * A * A * 1.001);
    treeBox[8] = (float)(1.001 / (2.0 * rmin));
    return true;
}

// Cell-grid layout (rt_scan.h scan_list_grid) for a scene of at most eight big spheres and a layer of many small ones: the big
// spheres keep the leading one-sphere groups (entries 4q; every ray tests them exactly), the small spheres follow SORTED BY
// HOME CELL of a uniform grid over the two long axes of their box -- cell = iu * nv + iv, so a run of cells of one u-slab is a
// run of scan entries -- about one sphere per cell, at most 254 x 254 cells.  false: the scene does not suit (the caller builds
// the bounds hierarchy instead).
static bool BuildGridLayout(const rt_sphere* sp, const std::vector<uint32_t>& big, const std::vector<uint32_t>& small, double density, SceneLayout& L) {
    if (big.size() > 8 || small.size() < 256) return false;
    if (!BoxOf(sp, small, L.treeBox)) return false;
    const double ext[3] = {(double)L.treeBox[3] - L.treeBox[0], (double)L.treeBox[4] - L.treeBox[1], (double)L.treeBox[5] - L.treeBox[2]};
    int w = 0;
    if (ext[1] < ext[w]) w = 1;
    if (ext[2] < ext[w]) w = 2;
    const int axU = (w + 1) % 3, axV = (w + 2) % 3;
    double rmax = 0;
    for (uint32_t k : small) rmax = std::max(rmax, (double)sp[k].r);
    // density: spheres per cell aimed at (measured on grid10k: 0.5 -5 %, 0.75 -4 %, 1.5 -4 %, 2.5 -8 %, 4 -12 % against 1.0)
    double h = std::sqrt(std::max(ext[axU] * ext[axV], 1e-30) * density / (double)small.size());
    h = std::max(h, 2.5 * rmax);                                  // a sphere's neighbourhood stays within one cell of its home
    h = std::max(h, std::max(ext[axU], ext[axV]) / 250.0);         // at most 254 cells per axis
    const float g0u = L.treeBox[axU] - (float)(0.01 * h), g0v = L.treeBox[axV] - (float)(0.01 * h);
    const float invH = (float)(1.0 / h);
    const uint32_t nu = (uint32_t)std::floor(((double)L.treeBox[3 + axU] - g0u) * invH) + 2u;
    const uint32_t nv = (uint32_t)std::floor(((double)L.treeBox[3 + axV] - g0v) * invH) + 2u;
    if (nu > 254u || nv > 254u || (size_t)nu * nv > 60000u) return false;
    auto coord = [&](uint32_t k, int ax) { return ax == 0 ? sp[k].cx : (ax == 1 ? sp[k].cy : sp[k].cz); };
    std::vector<std::pair<uint32_t, uint32_t>> keyed;  // (home cell, sphere)
    keyed.reserve(small.size());
    for (uint32_t k : small) {
        // the device forms (x - g0) * invH in float; the host's double value differs by < 1e-4 cells, inside the walk's slack
        const double fu = ((double)coord(k, axU) - (double)g0u) * (double)invH, fv = ((double)coord(k, axV) - (double)g0v) * (double)invH;
        const uint32_t iu = (uint32_t)std::min(std::max(std::floor(fu), 0.0), (double)(nu - 1u));
        const uint32_t iv = (uint32_t)std::min(std::max(std::floor(fv), 0.0), (double)(nv - 1u));
        keyed.push_back({iu * nv + iv, k});
    }
    std::stable_sort(keyed.begin(), keyed.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.first < b.first; });
    {   // a uniform grid suits a uniform layer: when the spheres are clumped (the average sphere shares its cell with more than
        // five others; a Poisson layer at one sphere per cell has one) a ray through a clump would test hundreds of spheres per
        // cell -- measured 3x slower than the bounds hierarchy on 1,500 spheres in a 3 x 3 patch of a 200 x 200 layer -- so the
        // hierarchy takes such scenes
        double sumSq = 0.0;
        for (size_t q = 0; q < keyed.size();) {
            size_t e = q;
            while (e < keyed.size() && keyed[e].first == keyed[q].first) ++e;
            sumSq += (double)(e - q) * (double)(e - q);
            q = e;
        }
        if (sumSq / (double)keyed.size() > 6.0) return false;
    }
    std::vector<std::vector<uint32_t>> groups;
    for (uint32_t k : big) groups.push_back({k});
    while (groups.size() & 3u) groups.push_back({});
    const uint32_t base = (uint32_t)groups.size() * 4u;  // first entry of the sorted small spheres
    for (size_t q = 0; q < keyed.size(); q += 4) {
        std::vector<uint32_t> g;
        for (size_t m = q; m < std::min(q + 4, keyed.size()); ++m) g.push_back(keyed[m].second);
        groups.push_back(g);
    }
    while (groups.size() & 3u) groups.push_back({});
    if (groups.size() * 4 + 4 >= 65536) return false;
    L.nGroups = (uint32_t)groups.size();
    const F4 never = MakeF4(0.f, 0.f, 0.f, -1e30f);
    L.scan.assign((size_t)L.nGroups * 4 + 4, never);
    L.orig.assign((size_t)L.nGroups * 4 + 4, 0xffffffffu);
    for (uint32_t gi = 0; gi < L.nGroups; ++gi)
        for (size_t m = 0; m < groups[gi].size(); ++m) {
            const uint32_t k = groups[gi][m];
            L.scan[(size_t)gi * 4 + m] = MakeF4(sp[k].cx, sp[k].cy, sp[k].cz, sp[k].r * sp[k].r);
            L.orig[(size_t)gi * 4 + m] = k;
        }
    L.gridCellStart.assign((size_t)nu * nv + 1, 0);
    {
        size_t q = 0;
        for (uint32_t c = 0; c <= nu * nv; ++c) {
            while (q < keyed.size() && keyed[q].first < c) ++q;
            L.gridCellStart[c] = (uint16_t)(base + q);
        }
    }
    L.singleMask[0] = L.singleMask[1] = 0ull;
    L.leaf.assign(L.scan.size(), BoundOf(sp, {}, nullptr, rtd::kMarginKLeaf));
    L.boundNorm = 0.f;
    for (size_t e = 0; e < L.orig.size(); ++e)
        if (L.orig[e] != 0xffffffffu) L.leaf[e] = BoundOf(sp, {L.orig[e]}, e >= base ? &L.boundNorm : &L.gridBigNorm, rtd::kMarginKLeaf);
    L.nAlways = (uint32_t)big.size();
    // one level of group bounds for rt_unit_layout's readers (the scan does not use them); the big spheres' groups are out of it
    L.tree.clear();
    L.nLevels = 1;
    L.levelOff[0] = 0;
    L.levelCnt[0] = L.nGroups;
    for (uint32_t gi = 0; gi < L.nGroups; ++gi) {
        float norm = 0.f;
        L.tree.push_back(gi < L.nAlways ? BoundOf(sp, {}, nullptr, rtd::kMarginKValu) : BoundOf(sp, groups[gi], &norm, rtd::kMarginKValu));
    }
    L.treeBoxOn = true;
    L.gridOn = true;
    L.gridNu = nu; L.gridNv = nv; L.gridAxU = (uint32_t)axU; L.gridAxV = (uint32_t)axV;
    L.gridG0u = g0u; L.gridG0v = g0v; L.gridInvH = invH; L.gridRmaxOverH = (float)(rmax * (double)invH * 1.0001);
    {   // Quantised bounds (rt_scan.h GridQuant): the device's four fmas, evaluated here with fmaf on the same constants, give the
        // bound centre C' bit for bit; the radius class covers r_i plus the sphere's own offset |C' - c_i|.
        const float hF = (float)h, su = hF / 256.f;
        const float uBase0 = g0u + 0.5f * su, vBase = g0v + 0.5f * su;
        double wlo = 1e300, whi = -1e300;
        for (uint32_t k : small) {
            wlo = std::min(wlo, (double)coord(k, w));
            whi = std::max(whi, (double)coord(k, w));
        }
        const float wstep = (float)((whi - wlo) / 16.0 * 1.0001 + 1e-30), wBase = (float)wlo + 0.5f * wstep;
        struct Q1 { uint32_t du, v16, kw; double err, r; };
        std::vector<Q1> q1(keyed.size());
        double smax = 0.0, Rmax = 0.0;
        bool ok = true;
        for (size_t q = 0; q < keyed.size() && ok; ++q) {
            const uint32_t k = keyed[q].second, cell = keyed[q].first, iu = cell / nv, iv = cell % nv;
            const double fu = ((double)coord(k, axU) - (double)g0u) * (double)invH - (double)iu;  // position in the home cell, [0, 1) unless clamped
            const double fv = ((double)coord(k, axV) - (double)g0v) * (double)invH - (double)iv;
            const uint32_t du = (uint32_t)std::min(255.0, std::max(0.0, std::floor(fu * 256.0)));
            const uint32_t dv = (uint32_t)std::min(255.0, std::max(0.0, std::floor(fv * 256.0)));
            const uint32_t kw = (uint32_t)std::min(15.0, std::max(0.0, std::floor(((double)coord(k, w) - wlo) / std::max((double)wstep, 1e-30))));
            const uint32_t v16 = iv * 256u + dv;
            const float uBase = std::fmaf((float)iu, hF, uBase0);
            const float cu = std::fmaf((float)du, su, uBase), cv = std::fmaf((float)v16, su, vBase), cw = std::fmaf((float)kw, wstep, wBase);
            const double eu = (double)cu - coord(k, axU), ev = (double)cv - coord(k, axV), ew = (double)cw - coord(k, w);
            const double err = std::sqrt(eu * eu + ev * ev + ew * ew);
            q1[q] = {du, v16, kw, err, (double)sp[k].r};
            smax = std::max(smax, err);
            Rmax = std::max(Rmax, (double)sp[k].r + err);
        }
        // (a sphere clamped into an edge cell can sit far from its cell: then the classes would be too coarse to be of use)
        if (ok && smax > 0.02 * h + 0.5 * (double)wstep) ok = false;
        if (ok) {
            const float rstep = (float)(Rmax * (1.0 + 1e-5) / 16.0);
            L.gridQ.assign(L.scan.size(), 0u);
            for (size_t q = 0; q < keyed.size(); ++q) {
                const double need = (q1[q].r + q1[q].err) * (1.0 + 1e-6) + 1e-30;
                uint32_t kr = 0;
                while (kr < 15u && (double)std::fmaf((float)kr, rstep, rstep) < need) ++kr;
                if ((double)std::fmaf((float)kr, rstep, rstep) < need) { ok = false; break; }
                L.gridQ[base + q] = q1[q].du | q1[q].v16 << 8 | q1[q].kw << 24 | kr << 28;
            }
            const float s2 = (float)(smax * smax * (1.0 + 1e-5) + 1e-30);
            const float qc[8] = {su, uBase0, hF, vBase, wBase, wstep, rstep, s2};
            for (int c = 0; c < 8; ++c) L.gridQc[c] = qc[c];
        }
        if (!ok) L.gridQ.clear();
    }
    return true;
}

void BuildLayout(const rt_sphere* signedSp, uint32_t n, const PrepOptions& opt, SceneLayout& L) {
    const uint32_t topMax = opt.treeTop;
    const std::vector<rt_sphere> absSp = WithAbsRadii(signedSp, n);
    const rt_sphere* sp = absSp.data();  // bounds enclose |r|
    std::vector<float> radii(n);
    for (uint32_t k = 0; k < n; ++k) radii[k] = sp[k].r;
    std::vector<float> sorted = radii;
    std::nth_element(sorted.begin(), sorted.begin() + n / 2, sorted.end());
    const float median = sorted[n / 2];
    std::vector<uint32_t> big, small;
    for (uint32_t k = 0; k < n; ++k) (radii[k] > 4.f * median ? big : small).push_back(k);
    // scenes beyond the flat matrix-core filter (more than topMax groups of four): a cell grid over the layer of small spheres
    // when the scene suits it
    if (opt.grid && opt.bigApart && ((small.size() + 3) / 4 + big.size() > topMax || opt.gridForce) && BuildGridLayout(sp, big, small, opt.gridDensity, L)) return;
    L = SceneLayout{};
    // k-d median split down to leaves of four, emitted in tree order: compact, balanced groups whose
    // neighbours in the list are neighbours in space (Morton chunks of a jittered grid have 3x the summed R^2
    // and twice the filter candidates; tools/cluster_eval.py)
    std::vector<std::vector<uint32_t>> groups;
    for (uint32_t k : big) groups.push_back({k});
    while (!big.empty() && (groups.size() & 3u)) groups.push_back({});  // big spheres keep upper-level nodes of their own
    std::vector<std::pair<size_t, size_t>> stack;  // [begin, end) ranges of `small`
    if (!small.empty()) stack.push_back({0, small.size()});
    while (!stack.empty()) {
        const auto [b, e] = stack.back();
        stack.pop_back();
        if (e - b <= 4) {
            groups.push_back(std::vector<uint32_t>(small.begin() + b, small.begin() + e));
            continue;
        }
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (size_t k = b; k < e; ++k) {
            const float c[3] = {sp[small[k]].cx, sp[small[k]].cy, sp[small[k]].cz};
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(lo[a], c[a]);
                hi[a] = std::max(hi[a], c[a]);
            }
        }
        int ax = 0;
        if (hi[1] - lo[1] > hi[ax] - lo[ax]) ax = 1;
        if (hi[2] - lo[2] > hi[ax] - lo[ax]) ax = 2;
        std::stable_sort(small.begin() + b, small.begin() + e, [&](uint32_t x, uint32_t y) {
            const float cx[3] = {sp[x].cx, sp[x].cy, sp[x].cz}, cy[3] = {sp[y].cx, sp[y].cy, sp[y].cz};
            return cx[ax] < cy[ax];
        });
        // left part: the largest power-of-four multiple of 4 not above half, so whole subtrees stay aligned
        size_t half = ((e - b) / 2 + 3) / 4 * 4;
        size_t p4 = 4;
        while (p4 * 4 <= (e - b) / 2 + 3) p4 *= 4;
        if (p4 >= 16 && (e - b) > p4) half = std::max(p4, (size_t)(((e - b) / 2) / p4 * p4));
        if (half >= e - b) half = (e - b) / 2;
        stack.push_back({b + half, e});
        stack.push_back({b, b + half});
    }
    RefineGroups(sp, groups);
    while (groups.size() & 3u) groups.push_back({});  // whole nodes at the next level; also even for the VALU scan
    L.nGroups = (uint32_t)groups.size();
    const F4 never = MakeF4(0.f, 0.f, 0.f, -1e30f);  // r*r = -1e30: discriminant negative for any ray
    L.scan.assign((size_t)L.nGroups * 4 + 4, never);
    L.orig.assign((size_t)L.nGroups * 4 + 4, 0xffffffffu);
    for (uint32_t gi = 0; gi < L.nGroups; ++gi) {
        for (size_t m = 0; m < groups[gi].size(); ++m) {
            const uint32_t k = groups[gi][m];
            // radius * radius is the float product Sphere::Intersect forms per call (ray-tracing.cpp:48)
            L.scan[(size_t)gi * 4 + m] = MakeF4(sp[k].cx, sp[k].cy, sp[k].cz, sp[k].r * sp[k].r);
            L.orig[(size_t)gi * 4 + m] = k;
        }
    }
    // groups of one sphere (the big ones, mostly) as bitmap bits: bit 63 - N of half h is group 16 h + (N & 15) + 32 (N >> 4)
    // (rt_scan.h, next_candidate); only meaningful while the groups ARE the filter's top level (<= 128 of them)
    L.singleMask[0] = L.singleMask[1] = 0ull;
    if (L.nGroups <= 128u)
        for (uint32_t gi = 0; gi < L.nGroups; ++gi)
            if (groups[gi].size() == 1) {
                const uint32_t N = (gi & 15u) + 16u * (gi >> 5);
                L.singleMask[(gi >> 4) & 1u] |= 0x8000000000000000ull >> N;
            }
    L.leaf.assign(L.scan.size(), BoundOf(sp, {}, nullptr, rtd::kMarginKLeaf));  // padding entries are never candidates
    for (size_t e = 0; e < L.orig.size(); ++e)
        if (L.orig[e] != 0xffffffffu) L.leaf[e] = BoundOf(sp, {L.orig[e]}, nullptr, rtd::kMarginKLeaf);
    // levels: level 0 = the groups; level k+1 node j = level-k nodes 4j .. 4j+3; stop at <= topMax nodes.  The top
    // level is tested by the matrix-core filter (margin K = kMarginK), the levels below it on the VALU (kMarginKValu).
    std::vector<std::vector<std::vector<uint32_t>>> levels;
    levels.push_back(groups);
    // Hierarchy scan (more groups than the matrix-core level takes): the big spheres stay out of the bounds.  With the floor
    // inside, node 0 of every level is a candidate for every ray and drags its siblings into the descent; tested directly, a
    // big sphere costs one exact slot per live ray.  (At most eight; the flat scan keeps them as one-sphere groups.)
    L.nAlways = 0;
    if (groups.size() > topMax && opt.bigApart) {
        while (L.nAlways < 8u && L.nAlways < big.size() && groups[L.nAlways].size() == 1) {
            levels[0][L.nAlways].clear();
            ++L.nAlways;
        }
    }
    while (levels.back().size() > topMax && levels.size() < rtd::kMaxLevels) {
        std::vector<std::vector<uint32_t>>& cur = levels.back();
        while (cur.size() & 3u) cur.push_back({});  // pad this level to whole parents
        std::vector<std::vector<uint32_t>> up(cur.size() / 4);
        for (size_t j = 0; j < up.size(); ++j)
            for (int q = 0; q < 4; ++q) up[j].insert(up[j].end(), cur[4 * j + q].begin(), cur[4 * j + q].end());
        levels.push_back(std::move(up));
    }
    L.treeBoxOn = false;
    if (levels.size() > 1 && opt.treeBox) {
        std::vector<uint32_t> inTree;
        for (const auto& ids : levels[0]) inTree.insert(inTree.end(), ids.begin(), ids.end());
        L.treeBoxOn = BoxOf(sp, inTree, L.treeBox);
    }
    L.tree.clear();
    L.nLevels = (uint32_t)levels.size();
    for (uint32_t lvl = 0; lvl < L.nLevels; ++lvl) {
        L.levelOff[lvl] = (uint32_t)L.tree.size();
        L.levelCnt[lvl] = (uint32_t)levels[lvl].size();
        const float K = lvl + 1 == L.nLevels ? rtd::kMarginK : rtd::kMarginKValu;
        for (const auto& ids : levels[lvl]) L.tree.push_back(BoundOf(sp, ids, &L.boundNorm, K));
    }
}
// ---------------------------------------------------------------------------------- shadow index
// Footprints of the spheres in the plane perpendicular to the sun, binned into a uniform grid (rt_shade.h
// shadow_query).  Conservative by construction: footprint radius rho = sqrt(r^2 + 64 eps (2 P0^2 + 2|c|^2 + r^2))
// (1 + 1e-4) + 1e-5 (P0 + |c| + 1) covers the reference test's own rounding for hit points with |p| <= P0 (E/a <= 16
// eps (...), 4x safety) and the rounding of the float projection; a sphere is listed in every cell its footprint's
// bounding square touches.

// maxCells: cells per axis at most.  64 for the scenes whose index is staged into LDS next to the tables (the flat scan: 8-10 KB on
// the cover scene); 256 for the scenes whose index stays in global memory (cell-grid and hierarchy scans, 10,000-sphere class): at
// 64 x 64 a query of grid10k walked ~15 spheres -- 7 rounds of two dependent L2 reads -- at 256 x 256 (cells of about one
// footprint) ~5.
void BuildShadowGrid(const rt_sphere* signedSp, const SceneLayout& L, const float sunDir[3], uint32_t maxCells, ShadowGrid& G) {
    BuildShadowGridTier(signedSp, L, sunDir, maxCells, 1u, G);
}

// tier 1: the index above, valid within P0.  tier 2: THE SAME construction -- footprint formula, spill-to-global rule, halving rule --
// for the hit points beyond P0 (the ground towards the horizon), valid within
//     P2 = min(4 P0, P1),   P1 = 1.01 max_i(|c_i| + |r_i|) + 1e-30.
// Why not P1 alone: the footprints are inflated for the reference test's own rounding at the LARGEST point the index answers, by
// 128 eps P^2 under the root.  A floor of radius 1000 makes P1 about 2000 and every footprint of the cover scene 5.5 units wide where
// the spheres are 0.2: each covers more than an eighth of the cells, all 480 go to the global list, and the builder gives up (more
// than 64).  At 4 P0 the inflation is sixteen times the first index's (cover: footprints of 0.42, 20 x 32 cells, the floor alone in
// the global list), the grid is still a grid, and it reaches beyond every hit a camera near the field can see on such a floor (the
// horizon from height h on radius R is sqrt(2 R h) away: 63 units from h = 2; cover's P0 is 33, its P2 134).  P1 only caps P2 where the whole scene is smaller than 4 P0: a hit point lies on a sphere, so
// |p| <= |c| + |r| up to the rounding of t d + o and of the root, for which one per cent is ample; nothing RELIES on that bound --
// a point beyond P2 is answered by the any-hit over every entry (rt_kernels.h processHit), which is always right and merely slow.
// Not enabled where P2 <= P0 (no sphere reaches beyond the first index) or where the first index's own reasons apply.
namespace {
void BuildShadowGridAt(const rt_sphere* signedSp, const SceneLayout& L, const float sunDir[3], uint32_t maxCells, uint32_t tier, ShadowGrid& G,
                       ShadowBuildCounts& n) {
    G = ShadowGrid{};
    uint32_t nSp = 0;
    for (uint32_t o : L.orig)
        if (o != 0xffffffffu) nSp = std::max(nSp, o + 1u);
    const std::vector<rt_sphere> absSp = WithAbsRadii(signedSp, nSp);
    const rt_sphere* sp = absSp.data();  // footprints and the reach are those of |r|
    const double Lx = sunDir[0], Ly = sunDir[1], Lz = sunDir[2];
    const double ln = std::sqrt(Lx * Lx + Ly * Ly + Lz * Lz);
    if (!(ln > 0.5 && ln < 2.0)) {  // not a direction: keep the scan
        ++n.notADirection;
        return;
    }
    // orthonormal basis of the plane perpendicular to L
    double ax[3] = {1, 0, 0};
    if (std::fabs(Lx) > std::fabs(Ly) && std::fabs(Lx) > std::fabs(Lz)) {
        ax[0] = 0; ax[1] = 1;
        ++n.basisSwitch;
    }
    double e1[3] = {Ly * ax[2] - Lz * ax[1], Lz * ax[0] - Lx * ax[2], Lx * ax[1] - Ly * ax[0]};
    const double n1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    for (double& v : e1) v /= n1;
    double e2[3] = {(Ly * e1[2] - Lz * e1[1]) / ln, (Lz * e1[0] - Lx * e1[2]) / ln, (Lx * e1[1] - Ly * e1[0]) / ln};
    for (int k = 0; k < 3; ++k) {
        G.e1[k] = (float)e1[k];
        G.e2[k] = (float)e2[k];
    }
    const size_t nEnt = (size_t)L.nGroups * 4;
    // P0: twice the reach of the ordinary (non-huge) spheres, so that practically every hit point qualifies
    std::vector<double> rs;
    for (size_t e = 0; e < nEnt; ++e)
        if (L.orig[e] != 0xffffffffu) rs.push_back(sp[L.orig[e]].r);
    if (rs.empty()) return;
    std::nth_element(rs.begin(), rs.begin() + rs.size() / 2, rs.end());
    const double med = rs[rs.size() / 2];
    double reach = 0;
    for (size_t e = 0; e < nEnt; ++e) {
        if (L.orig[e] == 0xffffffffu) continue;
        const rt_sphere& q = sp[L.orig[e]];
        if (q.r > 4.0 * med) continue;
        reach = std::max(reach, std::sqrt((double)q.cx * q.cx + (double)q.cy * q.cy + (double)q.cz * q.cz) + q.r);
    }
    double P0 = 2.0 * reach + 8.0 * med + 1.0;
    if (tier >= 2u) {
        double far = 0;
        for (size_t e = 0; e < nEnt; ++e) {
            if (L.orig[e] == 0xffffffffu) continue;
            const rt_sphere& q = sp[L.orig[e]];
            far = std::max(far, std::sqrt((double)q.cx * q.cx + (double)q.cy * q.cy + (double)q.cz * q.cz) + q.r);
        }
        const double P2 = std::min(4.0 * P0, 1.01 * far + 1e-30);
        if (!(P2 > P0)) {
            ++n.noTier2;
            return;
        }
        P0 = P2;  // from here on the construction is the first index's, for this radius
    }
    const double eps = 5.9604644775390625e-08;
    struct Foot { double u, v, rho; uint16_t entry; };
    std::vector<Foot> feet;
    double lo[2] = {1e300, 1e300}, hi[2] = {-1e300, -1e300};
    std::vector<double> rhos;
    for (size_t e = 0; e < nEnt; ++e) {
        if (L.orig[e] == 0xffffffffu) continue;
        const rt_sphere& q = sp[L.orig[e]];
        // the device projects with the FLOAT basis; use the same vectors here
        const double u = q.cx * (double)G.e1[0] + q.cy * (double)G.e1[1] + q.cz * (double)G.e1[2];
        const double v = q.cx * (double)G.e2[0] + q.cy * (double)G.e2[1] + q.cz * (double)G.e2[2];
        const double cn = std::sqrt((double)q.cx * q.cx + (double)q.cy * q.cy + (double)q.cz * q.cz);
        const double rho = std::sqrt((double)q.r * q.r + 64.0 * eps * (2.0 * P0 * P0 + 2.0 * cn * cn + (double)q.r * q.r)) * (1.0 + 1e-4) +
                           1e-5 * (P0 + cn + 1.0);
        feet.push_back({u, v, rho, (uint16_t)e});
        if (q.r <= 4.0 * med) {
            lo[0] = std::min(lo[0], u - rho); hi[0] = std::max(hi[0], u + rho);
            lo[1] = std::min(lo[1], v - rho); hi[1] = std::max(hi[1], v + rho);
            rhos.push_back(rho);
        }
    }
    if (rhos.empty()) {  // only huge spheres: everything goes to the global list, a 1x1 grid
        lo[0] = lo[1] = -1.0;
        hi[0] = hi[1] = 1.0;
        rhos.push_back(1.0);
        ++n.onlyHuge;
    }
    std::nth_element(rhos.begin(), rhos.begin() + rhos.size() / 2, rhos.end());
    const double ext = std::max(hi[0] - lo[0], hi[1] - lo[1]);
    double cell = std::max(2.0 * rhos[rhos.size() / 2], ext / (double)maxCells);
    G.nx = (uint32_t)std::min((double)maxCells, std::max(1.0, std::ceil((hi[0] - lo[0]) / cell)));
    G.ny = (uint32_t)std::min((double)maxCells, std::max(1.0, std::ceil((hi[1] - lo[1]) / cell)));
    G.u0 = (float)lo[0];
    G.v0 = (float)lo[1];
    G.invCell = (float)(1.0 / cell);
    // cell of a coordinate exactly as the device computes it (float), widened by one ulp-ish slack through rho
    auto cellOf = [&](double x, float x0, uint32_t n) -> long {
        const double f = (x - (double)x0) * (double)G.invCell;
        return (long)std::floor(f);
    };
    std::vector<std::vector<uint16_t>> cells((size_t)G.nx * G.ny);
    const size_t ncell = cells.size();
    for (const Foot& f : feet) {
        // no extra cell of slack: rho already carries 1e-5 (P0 + |c| + 1), at least 20x the error of the device's float
        // projection and cell arithmetic (<= ~5e-7 P0 for |p| <= P0), and floor() is monotone
        long x0 = cellOf(f.u - f.rho, G.u0, G.nx), x1 = cellOf(f.u + f.rho, G.u0, G.nx);
        long y0 = cellOf(f.v - f.rho, G.v0, G.ny), y1 = cellOf(f.v + f.rho, G.v0, G.ny);
        const bool outside = x1 < 0 || y1 < 0 || x0 >= (long)G.nx || y0 >= (long)G.ny;
        x0 = std::max(0L, x0); y0 = std::max(0L, y0);
        x1 = std::min((long)G.nx - 1, x1); y1 = std::min((long)G.ny - 1, y1);
        const bool spills = (f.u - f.rho < lo[0]) || (f.u + f.rho > hi[0]) || (f.v - f.rho < lo[1]) || (f.v + f.rho > hi[1]);
        const size_t covered = outside ? 0 : (size_t)(x1 - x0 + 1) * (size_t)(y1 - y0 + 1);
        // a footprint reaching beyond the grid can shadow points outside it: it must be tested for every query
        if (spills || covered * 8 > ncell) {
            ++(spills ? n.spilled : n.wide);
            G.global.push_back(f.entry);
            continue;
        }
        for (long y = y0; y <= y1; ++y)
            for (long x = x0; x <= x1; ++x) cells[(size_t)y * G.nx + x].push_back(f.entry);
    }
    size_t total = 0;
    for (const auto& c : cells) total += c.size();
    if (total >= kShadowEntriesEnd && maxCells > 64u) {  // too many entries for 16-bit cell starts: the coarser grid
        ++n.halved;
        BuildShadowGridAt(sp, L, sunDir, maxCells / 2u, tier, G, n);
        return;
    }
    if (total >= kShadowEntriesEnd || G.global.size() > kShadowGlobalMax) {  // pathological: keep the scan
        ++n.gaveUp;
        return;
    }
    G.cellStart.resize(ncell + 1);
    G.entries.reserve(total);
    for (size_t c = 0; c < ncell; ++c) {
        G.cellStart[c] = (uint16_t)G.entries.size();
        G.entries.insert(G.entries.end(), cells[c].begin(), cells[c].end());
    }
    G.cellStart[ncell] = (uint16_t)G.entries.size();
    G.p0sq = (float)(P0 * P0 * (1.0 - 1e-6));
    G.enabled = true;
    ++n.enabled;
}
}  // namespace

void BuildShadowGridTier(const rt_sphere* signedSp, const SceneLayout& L, const float sunDir[3], uint32_t maxCells, uint32_t tier, ShadowGrid& G,
                         ShadowBuildCounts* counts) {
    ShadowBuildCounts own;
    ShadowBuildCounts& n = counts ? *counts : own;
    ++n.built;
    BuildShadowGridAt(signedSp, L, sunDir, maxCells, tier, G, n);
}

// The material table packed into 16 bytes per scan entry (rt_shade.h load_material16), or false when some material of the scene
// does not fit the form: a colour that is read (not a glass sphere's; rgb1 only under a checker texture) must be byte * (1 / 255)
// exactly -- what XMLoadColor of an XMCOLOR gives, i.e. every colour the reference can hold (texture.cpp:5,16-17).
static bool PackMaterials(const std::vector<rt_material>& matc, std::vector<U4>& out) {
    auto byteOf = [](float c, uint32_t& b) {
        const float r = std::nearbyint(c * 255.0f);
        if (!(r >= 0.f && r <= 255.f)) return false;
        b = (uint32_t)r;
        return (float)b * (1.0f / 255.0f) == c;
    };
    out.assign(matc.size(), U4{0u, 0u, 0u, 0u});
    for (size_t e = 0; e < matc.size(); ++e) {
        const rt_material& m = matc[e];
        if (m.type > 3u || m.tex_type > 1u) return false;
        uint32_t c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
        const bool glass = m.type == RT_MAT_DIELECTRIC_TRANSPARENT;
        for (int k = 0; k < 3; ++k) {
            if (!glass && !byteOf(m.rgb0[k], c0[k])) return false;
            if (!glass && m.tex_type == RT_TEX_CHECKER && !byteOf(m.rgb1[k], c1[k])) return false;
        }
        const float slotA = m.type == RT_MAT_EMISSIVE ? m.luminance : m.smoothness;
        const float slotB = glass ? m.ior : m.tiling;
        uint32_t a, b;
        std::memcpy(&a, &slotA, 4);
        std::memcpy(&b, &slotB, 4);
        out[e] = U4{m.type | m.tex_type << 2 | c0[0] << 8 | c0[1] << 16 | c0[2] << 24, c1[0] | c1[1] << 8 | c1[2] << 16, a, b};
    }
    return true;
}

PreparedMaterials PrepareMaterials(const rt_material* materials, uint32_t n, const uint32_t* orig, size_t nEntries) {
    PreparedMaterials M;
    M.mats.resize(nEntries);
    std::memset(M.mats.data(), 0, nEntries * sizeof(rt_material));
    for (size_t e = 0; e < nEntries; ++e)
        if (orig[e] != 0xffffffffu) M.mats[e] = materials[orig[e]];
    M.mats16Ok = PackMaterials(M.mats, M.mats16);
    M.matType.resize(n);
    for (uint32_t k = 0; k < n; ++k) M.matType[k] = materials[k].type;
    return M;
}

PreparedShadows PrepareShadows(const rt_sphere* spheres, const SceneLayout& L, const rt_light* lights, uint32_t n_lights, const PrepOptions& opt,
                               ShadowBuildCounts* counts) {
    PreparedShadows S;
    // the first light's index is staged into LDS where the scan's tables are; the others', one each, stay in global memory
    if (opt.shadowGrid && n_lights != 0)
        BuildShadowGridTier(spheres, L, lights[0].direction, L.InGlobalMemory() ? opt.shadowCellsGlobal : opt.shadowCellsLds, 1u, S.shadow, counts);
    S.extraShadow.resize(n_lights > 1 ? n_lights - 1 : 0);
    for (uint32_t k = 1; k < n_lights && opt.shadowGrid; ++k) 
        BuildShadowGridTier(spheres, L, lights[k].direction, opt.shadowCellsGlobal, 1u, S.extraShadow[k - 1], counts);
    // light 0's second index, for the hit points beyond the first one's radius: in global memory, like the extra lights'
    if (S.shadow.enabled) BuildShadowGridTier(spheres, L, lights[0].direction, opt.shadowCellsGlobal, 2u, S.shadowFar, counts);
    // RT_SG_SPH=1 (experiments): the index stays in global memory -- the sphere record of every entry side by side with the ids, so
    // that a walk round is one round trip instead of two.  Measured on grid10k: 7.79 -> 7.66 Gsamples/s (700 KB of duplicated
    // spheres hit the L1 less often than the 160 KB table they are shared from).  Default off.
    if (S.shadow.enabled && L.InGlobalMemory() && opt.sgSph) {
        S.sgSph.assign(S.shadow.entries.size() + 1, MakeF4(0.f, 0.f, 0.f, -1e30f));
        for (size_t k = 0; k < S.shadow.entries.size(); ++k) S.sgSph[k] = L.scan[S.shadow.entries[k]];
    }
    return S;
}

SceneLayout ShadowLayoutOf(const SceneLayout& L, const PrepOptions& opt) {
    SceneLayout K;
    K.orig = L.orig;
    K.nGroups = L.nGroups;
    K.nLevels = L.nLevels;
    K.gridOn = L.gridOn;
    if (opt.sgSph && L.InGlobalMemory()) K.scan = L.scan;
    return K;
}

PreparedScene PrepareScene(const rt_sphere* spheres, const rt_material* materials, uint32_t n, const rt_light* lights, uint32_t n_lights,
                           const PrepOptions& opt) {
    PreparedScene P;
    SceneLayout& L = P.layout;
    BuildLayout(spheres, n, opt, L);
    if (L.scan.size() >= 65536) return P;
    const size_t nPad = L.scan.size();
    P.radius.assign(nPad, 0.f);
    for (size_t e = 0; e < nPad; ++e)
        if (L.orig[e] != 0xffffffffu) P.radius[e] = spheres[L.orig[e]].r;
    PreparedMaterials M = PrepareMaterials(materials, n, L.orig.data(), nPad);
    P.mats = std::move(M.mats);
    P.mats16 = std::move(M.mats16);
    P.mats16Ok = M.mats16Ok;
    P.matType = std::move(M.matType);
    PreparedShadows S = PrepareShadows(spheres, L, lights, n_lights, opt);
    P.shadow = std::move(S.shadow);
    P.extraShadow = std::move(S.extraShadow);
    P.shadowFar = std::move(S.shadowFar);
    P.sgSph = std::move(S.sgSph);
    for (int h = 0; h < 2; ++h) P.singleMask[h] = opt.singleDirect ? L.singleMask[h] : 0ull;
    return P;
}

uint32_t RowsetRowsWithin(rt_rowset rs, uint32_t H) { return (uint64_t)rs.first_row + rs.num_rows > H ? 0u : RowsetLocalRows(rs); }

uint32_t UnitStripRows(rt_rowset rs, uint32_t W, uint32_t H) {
    const uint32_t rows = RowsetRowsWithin(rs, H);
    return (uint64_t)W * rows > (1ull << 31) ? 0u : rows;
}

void EntryOfSphere(const uint32_t* orig, size_t nEntries, uint32_t n, uint32_t shift, uint32_t* out) {
    for (uint32_t k = 0; k < n; ++k) out[k] = 0xffffffffu;
    for (size_t e = 0; e < nEntries; ++e)
        if (orig[e] < n) out[orig[e]] = (uint32_t)e >> shift;
}

namespace {

// The layout an upload would build under the environment of the moment, for the GPU-less queries below.
int LayoutFor(const char* who, const rt_sphere* spheres, uint32_t n, SceneLayout& L) {
    if (!AllFinite(spheres, n, nullptr)) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": a sphere's centre or radius is not finite");
    BuildLayout(spheres, n, PrepOptions::FromEnv(), L);
    return RT_OK;
}

// The flat scan's top level -- the groups themselves -- as the float[4] bounds rt_tile_mask.h takes; empty where the scene gets
// another scan (no tile tables).
std::vector<std::array<float, 4>> FlatTopBounds(const SceneLayout& L) {
    std::vector<std::array<float, 4>> out;
    const uint32_t nTop = L.levelCnt[L.nLevels - 1];
    if (L.nLevels != 1 || L.gridOn || nTop > 128u) return out;
    for (uint32_t g = 0; g < nTop; ++g) {
        const F4 B = L.tree[L.levelOff[L.nLevels - 1] + g];
        out.push_back({B.x, B.y, B.z, B.w});
    }
    return out;
}

rtd::TileMaskCam CamOf(const rt_camera* camera, uint32_t W, uint32_t H) {
    return rtd::tile_mask_cam(camera->origin, camera->x, camera->y, camera->origin_image_plane, camera->aperture, camera->focal_length, W, H);
}

}  // namespace
}  // namespace rtprep

using namespace rtprep;

extern "C" {

uint32_t rt_rowset_local_rows(rt_rowset rs) { return RowsetLocalRows(rs); }
uint32_t rt_rowset_global_row(rt_rowset rs, uint32_t lr) {
    const uint32_t lb = lr / rs.block_rows;
    const uint32_t k = lr % rs.block_rows;
    return rs.first_row + (lb * rs.nshards + rs.shard) * rs.block_rows + k;
}

// Host-only: the elementary functions of rt_device_math.h as this translation unit compiles them (the source the kernels compile)
int rt_unit_math_host(uint32_t op, const float* x, const float* y, uint32_t n, float* out) {
    if (!x || !out || op > 3 || (op == 2 && !y)) return Fail(RT_ERR_INVALID_ARG, "rt_unit_math_host: invalid argument");
    for (uint32_t k = 0; k < n; ++k)
        out[k] = op == 0 ? rtd::rt_sinf(x[k]) : (op == 1 ? rtd::rt_cosf(x[k]) : (op == 2 ? rtd::rt_powf(x[k], y[k]) : rtd::rt_tanf(x[k])));
    return RT_OK;
}

int rt_unit_noise_estimate_host(const float* hdr, const float* sq, uint32_t npix, uint32_t n, float floor, float* out) {
    if (!hdr || !sq || !out) return Fail(RT_ERR_INVALID_ARG, "rt_unit_noise_estimate_host: null argument");
    if (n < 2) return Fail(RT_ERR_SEQUENCE, "rt_unit_noise_estimate_host: the estimate needs at least 2 samples per pixel");
    for (uint32_t p = 0; p < npix; ++p) rtd::noise_estimate(hdr + 3 * (size_t)p, sq + 3 * (size_t)p, n, floor, out + 2 * (size_t)p);
    return RT_OK;
}

// Host-only: the per-sample step of the feature buffers (rt_features.h feature_sample, the source the kernel compiles) for n hit
// records of rt_unit_closest_hit's format; materials by ORIGINAL sphere index.
int rt_unit_features_host(const rt_material* materials, uint32_t n_materials, const rt_material* sky, const float* hits10, uint32_t n, float* out8,
                          uint32_t* out_ids) {
    if (!materials || !sky || !hits10 || !out8 || !out_ids) return Fail(RT_ERR_INVALID_ARG, "rt_unit_features_host: null argument");
    const rtd::V3 skyAlbedo = rtd::feature_sky_albedo(rtd::feature_material(*sky));
    for (uint32_t k = 0; k < n; ++k) {
        const float* h = hits10 + 10 * (size_t)k;
        int32_t oidx;
        std::memcpy(&oidx, &h[1], sizeof(oidx));
        const bool hit = oidx >= 0;
        if (hit && (uint32_t)oidx >= n_materials)
            return Fail(RT_ERR_INVALID_ARG, "rt_unit_features_host: record " + std::to_string(k) + " names a sphere beyond the material table");
        const rtd::Mat m = rtd::feature_material(hit ? materials[oidx] : *sky);
        rtd::feature_sample(hit, m, (uint32_t)oidx, h[0], rtd::v3(h[5], h[6], h[7]), h[8], h[9], skyAlbedo, out8 + rtd::kFeatureChannels * (size_t)k,
                            out_ids[k]);
    }
    return RT_OK;
}

// Host-only: the clustered layout rt_scene_upload builds (no device needed).  orig: 4 entries per group
// (0xffffffff = padding), bounds: Cx, Cy, Cz, |C|^2 - Rf^2 per group.  Pass cap_groups = 0 to query the count.
int rt_unit_layout(const rt_sphere* spheres, uint32_t n, uint32_t cap_groups, uint32_t* n_groups, uint32_t* orig, float* bounds) {
    if (!spheres || n == 0 || !n_groups) return Fail(RT_ERR_INVALID_ARG, "rt_unit_layout: invalid argument");
    SceneLayout L;
    if (const int rc = LayoutFor("rt_unit_layout", spheres, n, L)) return rc;
    *n_groups = L.nGroups;
    if (cap_groups == 0) return RT_OK;
    if (cap_groups < L.nGroups || !orig || !bounds) return Fail(RT_ERR_INVALID_ARG, "rt_unit_layout: capacity too small");
    std::memcpy(orig, L.orig.data(), (size_t)L.nGroups * 4 * sizeof(uint32_t));
    std::memcpy(bounds, L.tree.data(), (size_t)L.nGroups * sizeof(F4));  // level 0 comes first
    return RT_OK;
}

int rt_unit_layout_info(const rt_sphere* spheres, uint32_t n, uint32_t out[5]) {
    if (!spheres || n == 0 || !out) return Fail(RT_ERR_INVALID_ARG, "rt_unit_layout_info: invalid argument");
    SceneLayout L;
    if (const int rc = LayoutFor("rt_unit_layout_info", spheres, n, L)) return rc;
    out[0] = L.gridOn ? 1u : (L.nLevels > 1 ? 2u : 0u);
    out[1] = L.gridOn ? L.gridNu : 0u;
    out[2] = L.gridOn ? L.gridNv : 0u;
    out[3] = L.nAlways;
    out[4] = L.nLevels;
    return RT_OK;
}

int rt_unit_grid_info(const rt_sphere* spheres, uint32_t n, uint32_t out_u[5], float out_f[10], int32_t* home_cell) {
    if (!spheres || n == 0 || !out_u || !out_f) return Fail(RT_ERR_INVALID_ARG, "rt_unit_grid_info: invalid argument");
    SceneLayout L;
    if (const int rc = LayoutFor("rt_unit_grid_info", spheres, n, L)) return rc;
    out_u[0] = L.gridOn ? 1u : 0u;
    if (!L.gridOn) return RT_OK;
    out_u[1] = L.gridNu; out_u[2] = L.gridNv; out_u[3] = L.gridAxU; out_u[4] = L.gridAxV;
    out_f[0] = L.gridG0u; out_f[1] = L.gridG0v; out_f[2] = L.gridInvH; out_f[3] = L.gridRmaxOverH;
    for (int k = 0; k < 6; ++k) out_f[4 + k] = L.treeBox[k];
    if (home_cell) {  // read back from the table the scan reads: entries [cellStart[c], cellStart[c + 1]) are cell c's spheres
        for (uint32_t k = 0; k < n; ++k) home_cell[k] = -1;
        for (uint32_t c = 0; c < L.gridNu * L.gridNv; ++c)
            for (uint32_t e = L.gridCellStart[c]; e < L.gridCellStart[c + 1]; ++e)
                if (L.orig[e] < n) home_cell[L.orig[e]] = (int32_t)c;
    }
    return RT_OK;
}

// The two host twins below state the device's tile tables (rt_kernels.h rt_tile_mask_kernel) a second time, independently.
int rt_unit_tile_masks_host(const rt_sphere* spheres, uint32_t n, const rt_camera* camera, uint32_t W, uint32_t H, rt_rowset rs, uint32_t limit,
                            uint32_t cap_tiles, uint32_t* n_tiles, uint32_t* words, uint32_t* group_of_sphere) {
    if (!spheres || n == 0 || !camera || !n_tiles || W == 0 || H == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_masks_host: invalid argument");
    if (!AllFinite(spheres, n, nullptr)) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_masks_host: a sphere's centre or radius is not finite");
    const uint32_t rows = UnitStripRows(rs, W, H);
    if (rows == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_masks_host: bad row set");
    SceneLayout L;
    BuildLayout(spheres, n, PrepOptions::FromEnv(), L);
    const std::vector<std::array<float, 4>> top = FlatTopBounds(L);
    const uint32_t nFull = (W * rows) >> 6;
    *n_tiles = top.empty() ? 0u : nFull;
    if (*n_tiles == 0u || !words) return RT_OK;
    if (cap_tiles < nFull) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_masks_host: capacity too small");
    const rtd::TileMaskCam c = CamOf(camera, W, H);
    for (uint32_t t = 0; t < nFull; ++t) {
        uint32_t* w = words + (size_t)rtd::kTileMaskWords * t;
        for (uint32_t k = 0; k < rtd::kTileMaskWords; ++k) w[k] = 0u;
        bool bad = false;
        uint32_t cnt = 0;
        for (uint32_t g = 0; g < (uint32_t)top.size(); ++g) {
            const int r = rtd::tile_group_reached(c, rs, t, top[g].data());
            bad = bad || r < 0;
            if (r > 0) {
                uint32_t word, bit;
                rtd::tile_mask_slot(g, word, bit);
                w[word] |= bit;
                ++cnt;
            }
        }
        w[4] = rtd::tile_mask_flags(bad, cnt, limit);
        w[5] = cnt;
    }
    if (group_of_sphere) EntryOfSphere(L.orig.data(), L.orig.size(), n, 2, group_of_sphere);  // flat scan: scan entry = 4 * group + member
    return RT_OK;
}

int rt_unit_tile_spheres_host(const rt_sphere* spheres, uint32_t n, const rt_camera* camera, uint32_t W, uint32_t H, rt_rowset rs, uint32_t mask_limit,
                              uint32_t sphere_limit, uint32_t cap_tiles, uint32_t* n_tiles, uint16_t* lists, uint32_t* entry_of_sphere) {
    if (!spheres || n == 0 || !camera || !n_tiles || W == 0 || H == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_spheres_host: invalid argument");
    if (!AllFinite(spheres, n, nullptr)) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_spheres_host: a sphere's centre or radius is not finite");
    const uint32_t rows = UnitStripRows(rs, W, H);
    if (rows == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_spheres_host: bad row set");
    if (sphere_limit > rtd::kTileSphereMax) sphere_limit = rtd::kTileSphereMax;
    SceneLayout L;
    BuildLayout(spheres, n, PrepOptions::FromEnv(), L);
    const std::vector<std::array<float, 4>> top = FlatTopBounds(L);
    const uint32_t nTop = (uint32_t)top.size();
    const uint32_t nFull = (W * rows) >> 6;
    *n_tiles = (nTop != 0u && sphere_limit != 0u) ? nFull : 0u;
    if (entry_of_sphere) EntryOfSphere(L.orig.data(), L.orig.size(), n, 0, entry_of_sphere);
    if (*n_tiles == 0u || !lists) return RT_OK;
    if (cap_tiles < nFull) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_spheres_host: capacity too small");
    const rtd::TileMaskCam c = CamOf(camera, W, H);
    std::vector<int> reached(nTop);
    for (uint32_t t = 0; t < nFull; ++t) {
        uint16_t* rec = lists + (size_t)rtd::kTileSphereHalfs * t;
        for (uint32_t k = 0; k < rtd::kTileSphereHalfs; ++k) rec[k] = 0;
        bool bad = false;
        uint32_t cnt = 0;
        for (uint32_t g = 0; g < nTop; ++g) {
            reached[g] = rtd::tile_group_reached(c, rs, t, top[g].data());
            bad = bad || reached[g] < 0;
            cnt += reached[g] > 0 ? 1u : 0u;
        }
        uint32_t nS = 0;
        const bool masked = rtd::tile_mask_flags(bad, cnt, mask_limit) != 0u;
        for (uint32_t e = 0; masked && e < 4u * nTop && e < (uint32_t)L.leaf.size() && nS <= sphere_limit; ++e) {
            const F4 B = L.leaf[e];
            const float b[4] = {B.x, B.y, B.z, B.w};
            if (rtd::tile_entry_listed(c, rs, t, reached[e >> 2], L.orig[e], b)) {
                if (nS < sphere_limit) rec[1u + nS] = (uint16_t)e;
                ++nS;
            }
        }
        rec[0] = (uint16_t)((masked && nS <= sphere_limit) ? nS : rtd::kTileSphereNone);
    }
    return RT_OK;
}

int rt_unit_tile_cone(const rt_camera* camera, uint32_t W, uint32_t H, uint32_t i0, uint32_t i1, uint32_t j, double out[9]) {
    if (!camera || !out || W == 0 || H == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_cone: invalid argument");
    const rtd::TileCone t = rtd::tile_run_cone(CamOf(camera, W, H), i0, i1, j);
    for (int k = 0; k < 3; ++k) {
        out[k] = t.o[k];
        out[3 + k] = t.D[k];
    }
    out[6] = t.rhoL;
    out[7] = t.rhoF;
    out[8] = t.ok ? 1.0 : 0.0;
    return RT_OK;
}

}  // extern "C"
