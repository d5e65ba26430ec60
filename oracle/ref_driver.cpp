// ORACLE — TEST INFRASTRUCTURE ONLY.  C ABI over the reference's own classes (ref_api.h).  This file builds the reference's
// objects from the flat records of include/rt_api.h, calls their methods and copies results out.  It restates none of their
// methods: the only logic of its own is the loop of ref_list_closest (the reference has no list class) and the any-hit loop
// handed to DirectionalLight as its occlusion test.
//
// The reference keeps its members private and offers no getters for most of them; the headers are included with `private`
// spelled `public` so that counters and camera members can be read (and a light's members set to a record's).  Every standard
// header the reference's stdafx.h asks for is included first, so the respelling touches the reference's classes only.
#include <algorithm>
#include <array>
#include <atomic>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <execution>
#include <functional>
#include <iostream>
#include <iterator>
#include <limits>
#include <memory>
#include <optional>
#include <random>
#include <string>
#include <vector>

#define private public  // the six headers below are the reference's (-I $(REFERENCE)/src/common-lib)
#include <camera.h>
#include <light.h>
#include <material.h>
#include <quasi-random.h>
#include <ray-tracing.h>
#include <texture.h>
#undef private

#include "ref_api.h"

namespace {

// A material that only says which list entry a sphere is (Payload carries the material pointer, not an index).
struct Tag final : Material {
    int32_t index = -1;
    bool Scatter(const Ray&, const Payload&, XMVECTOR&, Ray&) const override { return false; }
    XMVECTOR Emit(const Payload&) const override { return XMVectorZero(); }
    XMVECTOR GetAlbedo(XMFLOAT2) const override { return XMVectorZero(); }
    XMVECTOR GetReflectance(XMFLOAT2) const override { return XMVectorZero(); }
    XMVECTOR GetSmoothness(XMFLOAT2) const override { return XMVectorZero(); }
};

Ray LoadRay(const float* r) { return Ray{XMVectorSet(r[0], r[1], r[2], 1.f), XMVectorSet(r[3], r[4], r[5], 0.f)}; }

void StoreHit(float* o, bool hit, const Payload& p) {
    int32_t idx = -1;
    if (!hit) {
        for (int q = 0; q < 10; ++q) o[q] = 0.f;
    } else {
        idx = p.material ? static_cast<const Tag*>(p.material)->index : 0;
        o[0] = p.t.x;
        o[2] = p.pos.x; o[3] = p.pos.y; o[4] = p.pos.z;
        o[5] = p.normal.x; o[6] = p.normal.y; o[7] = p.normal.z;
        o[8] = p.uv.x; o[9] = p.uv.y;
    }
    std::memcpy(&o[1], &idx, 4);
}

Payload LoadHit(const float* h) {
    Payload p{};
    p.t = XMVectorZero();
    p.pos = XMVectorSet(h[0], h[1], h[2], 0.f);
    p.normal = XMVectorSet(h[3], h[4], h[5], 0.f);
    p.uv = XMFLOAT2(h[6], h[7]);
    p.material = nullptr;
    return p;
}

// rt_material colours hold byte * (1/255); the XMCOLOR constructor quantises them back to that byte.
XMCOLOR ColorOf(const float* rgb) { return XMCOLOR(rgb[0], rgb[1], rgb[2], 1.f); }

std::unique_ptr<Texture> TextureOf(const rt_material& m) {
    if (m.tex_type == RT_TEX_CHECKER) return std::make_unique<CheckerTexture>(ColorOf(m.rgb0), ColorOf(m.rgb1), m.tiling);
    return std::make_unique<ConstTexture>(ColorOf(m.rgb0));
}

}  // namespace

struct ref_scene {
    std::vector<std::unique_ptr<Tag>> tags;
    std::vector<std::unique_ptr<Sphere>> list;
    BvhNode* bvh = nullptr;
    ~ref_scene() {
        // the tags are owned here, not by the spheres
        for (auto& s : list) (void)s->material.release();
        // The BvhNode and the spheres it took over are left allocated: Hitable has no virtual destructor, so the tree cannot be
        // destroyed through its own pointers.  Their material pointers are never followed again.
    }
    bool AnyHit(const Ray& ray) const {
        Payload p;
        for (const auto& s : list)
            if (s->Intersect(ray, p)) return true;
        return false;
    }
};

struct ref_material {
    std::unique_ptr<Texture> texture;
    Material* material = nullptr;
    uint32_t type = 0;
    ~ref_material() {  // Material has no virtual destructor: destroy as the class it was made as
        switch (type) {
            case RT_MAT_METAL: delete static_cast<Metal*>(material); break;
            case RT_MAT_DIELECTRIC_TRANSPARENT: delete static_cast<DielectricTransparent*>(material); break;
            case RT_MAT_EMISSIVE: delete static_cast<Emissive*>(material); break;
            default: delete static_cast<DielectricOpaque*>(material); break;
        }
    }
    void Counters(uint64_t c[2]) const {
        c[0] = c[1] = 0;
        switch (type) {
            case RT_MAT_METAL: c[1] = static_cast<const Metal*>(material)->m_reflectionProbabilitySampleIndex.load(); break;
            case RT_MAT_DIELECTRIC_TRANSPARENT: c[0] = static_cast<const DielectricTransparent*>(material)->m_sampleIndex.load(); break;
            case RT_MAT_EMISSIVE: break;
            default:
                c[0] = static_cast<const DielectricOpaque*>(material)->m_sampleIndex.load();
                c[1] = static_cast<const DielectricOpaque*>(material)->m_reflectionProbabilitySampleIndex.load();
                break;
        }
    }
};

namespace {

std::vector<std::unique_ptr<Light>> LightsOf(const rt_light* lights, uint32_t n, const ref_scene* occluders,
                                             std::vector<uint8_t>* occludedLog) {
    std::vector<std::unique_ptr<Light>> out;
    for (uint32_t k = 0; k < n; ++k) {
        const rt_light& l = lights[k];
        auto test = [occluders, occludedLog](const Ray& ray) -> bool {
            const bool occluded = occluders ? occluders->AnyHit(ray) : false;
            if (occludedLog) occludedLog->push_back(occluded ? 1 : 0);
            return occluded;
        };
        auto dl = std::make_unique<DirectionalLight>(XMVectorSet(l.direction[0], l.direction[1], l.direction[2], 0.f),
                                                     ColorOf(l.color), l.luminance, test);
        dl->m_direction = XMVectorSet(l.direction[0], l.direction[1], l.direction[2], 0.f);
        dl->m_color = XMVectorSet(l.color[0], l.color[1], l.color[2], 1.f);
        out.push_back(std::move(dl));
    }
    return out;
}

}  // namespace

extern "C" {

void ref_halton(const uint64_t* index, uint32_t n, uint32_t base, float* out) {
    for (uint32_t k = 0; k < n; ++k) out[k] = Random::HaltonSample(index[k], base);
}
void ref_halton_2d(const uint64_t* index, uint32_t n, uint32_t b1, uint32_t b2, float* out) {
    for (uint32_t k = 0; k < n; ++k) {
        const XMFLOAT2 v = Random::HaltonSample2D(index[k], b1, b2);
        out[2 * k] = v.x; out[2 * k + 1] = v.y;
    }
}
void ref_halton_ring(const uint64_t* index, uint32_t n, uint32_t base, float* out) {
    for (uint32_t k = 0; k < n; ++k) {
        const XMFLOAT2 v = Random::HaltonSampleRing(index[k], base);
        out[2 * k] = v.x; out[2 * k + 1] = v.y;
    }
}
void ref_halton_disk(const uint64_t* index, uint32_t n, uint32_t b1, uint32_t b2, float* out) {
    for (uint32_t k = 0; k < n; ++k) {
        const XMFLOAT2 v = Random::HaltonSampleDisk(index[k], b1, b2);
        out[2 * k] = v.x; out[2 * k + 1] = v.y;
    }
}
void ref_halton_hemisphere(const uint64_t* index, uint32_t n, uint32_t b1, uint32_t b2, float* out) {
    for (uint32_t k = 0; k < n; ++k) {
        const XMFLOAT3 v = Random::HaltonSampleHemisphere(index[k], b1, b2);
        out[3 * k] = v.x; out[3 * k + 1] = v.y; out[3 * k + 2] = v.z;
    }
}
int ref_libm(uint32_t op, const float* x, const float* y, uint32_t n, float* out) {
    for (uint32_t k = 0; k < n; ++k) {
        switch (op) {
            case 0: out[k] = std::sin(x[k]); break;
            case 1: out[k] = std::cos(x[k]); break;
            case 2: out[k] = std::pow(x[k], y[k]); break;
            case 3: out[k] = std::tan(x[k]); break;
            case 4: out[k] = std::sqrt(x[k]); break;
            default: return 1;
        }
    }
    return 0;
}

void ref_sphere_intersect(const rt_sphere* s, const float* rays, uint32_t n, float* out) {
    const Sphere sphere(XMVectorSet(s->cx, s->cy, s->cz, 0.f), s->r, nullptr);
    for (uint32_t k = 0; k < n; ++k) {
        Payload p;
        const bool hit = sphere.Intersect(LoadRay(rays + 6 * k), p);
        StoreHit(out + 10 * k, hit, p);
    }
}

ref_scene* ref_scene_new(const rt_sphere* spheres, uint32_t n, uint32_t bvh_srand) {
    auto* sc = new ref_scene();
    std::vector<std::unique_ptr<Hitable>> forBvh;
    for (uint32_t i = 0; i < n; ++i) {
        const rt_sphere& s = spheres[i];
        sc->tags.push_back(std::make_unique<Tag>());
        sc->tags.back()->index = (int32_t)i;
        Tag* tag = sc->tags.back().get();
        sc->list.push_back(std::make_unique<Sphere>(XMVectorSet(s.cx, s.cy, s.cz, 0.f), s.r, std::unique_ptr<Material>(tag)));
        forBvh.push_back(std::make_unique<Sphere>(XMVectorSet(s.cx, s.cy, s.cz, 0.f), s.r, std::unique_ptr<Material>(tag)));
    }
    if (n) {
        std::srand(bvh_srand);
        sc->bvh = new BvhNode(forBvh.begin(), forBvh.end());
    }
    return sc;
}
void ref_scene_free(ref_scene* s) { delete s; }

void ref_list_closest(const ref_scene* s, const float* rays, uint32_t n, float* out) {
    for (uint32_t k = 0; k < n; ++k) {
        const Ray ray = LoadRay(rays + 6 * k);
        Payload best, cand;
        bool any = false;
        for (const auto& sph : s->list) {
            if (sph->Intersect(ray, cand) && (!any || cand.t.x < best.t.x)) {
                best = cand;
                any = true;
            }
        }
        StoreHit(out + 10 * k, any, best);
    }
}
void ref_bvh_closest(const ref_scene* s, const float* rays, uint32_t n, float* out) {
    for (uint32_t k = 0; k < n; ++k) {
        Payload p;
        const bool hit = s->bvh && s->bvh->Intersect(LoadRay(rays + 6 * k), p);
        StoreHit(out + 10 * k, hit, p);
    }
}

static void StoreCamera(const Camera& c, rt_camera* out) {
    std::memset(out, 0, sizeof(*out));
    std::memcpy(out->origin, &c.m_origin, 16);
    std::memcpy(out->x, &c.m_x, 16);
    std::memcpy(out->y, &c.m_y, 16);
    std::memcpy(out->origin_image_plane, &c.m_originImagePlane, 16);
    out->aperture = c.m_aperture;
    out->focal_length = c.m_focalLength;
}
void ref_camera_make(const float o[3], const float l[3], float vfov, float aspect, float focal, float aperture, rt_camera* out) {
    const Camera cam(XMVectorSet(o[0], o[1], o[2], 1.f), XMVectorSet(l[0], l[1], l[2], 1.f), vfov, aspect, focal, aperture);
    StoreCamera(cam, out);
}
void ref_camera_ray(const rt_camera* c, const float* in, uint32_t n, float* out) {
    Camera cam(XMVectorSet(0.f, 0.f, 0.f, 1.f), XMVectorSet(0.f, 0.f, 1.f, 1.f), 90.f, 1.f, 1.f, 0.f);
    std::memcpy(&cam.m_origin, c->origin, 16);
    std::memcpy(&cam.m_x, c->x, 16);
    std::memcpy(&cam.m_y, c->y, 16);
    std::memcpy(&cam.m_originImagePlane, c->origin_image_plane, 16);
    cam.m_aperture = c->aperture;
    cam.m_focalLength = c->focal_length;
    for (uint32_t k = 0; k < n; ++k) {
        const float* q = in + 4 * k;
        const Ray r = cam.GetRay(XMFLOAT2(q[0], q[1]), XMFLOAT2(q[2], q[3]));
        float* w = out + 6 * k;
        w[0] = r.origin.x; w[1] = r.origin.y; w[2] = r.origin.z;
        w[3] = r.direction.x; w[4] = r.direction.y; w[5] = r.direction.z;
    }
}

void ref_texture_eval(const rt_material* m, const float* uv, uint32_t n, float* out) {
    const std::unique_ptr<Texture> tex = TextureOf(*m);
    for (uint32_t k = 0; k < n; ++k) {
        const XMVECTOR v = tex->Evaluate(XMFLOAT2(uv[2 * k], uv[2 * k + 1]));
        std::memcpy(out + 4 * k, &v, 16);
    }
}

ref_material* ref_material_new(const rt_material* m) {
    auto* r = new ref_material();
    r->type = m->type;
    if (m->type != RT_MAT_DIELECTRIC_TRANSPARENT) r->texture = TextureOf(*m);
    switch (m->type) {
        case RT_MAT_METAL: r->material = new Metal(r->texture.get(), XMVectorReplicate(m->smoothness)); break;
        case RT_MAT_DIELECTRIC_TRANSPARENT: r->material = new DielectricTransparent(XMVectorReplicate(m->smoothness), m->ior); break;
        case RT_MAT_EMISSIVE: r->material = new Emissive(m->luminance, r->texture.get()); break;
        default:
            r->type = RT_MAT_DIELECTRIC_OPAQUE;
            r->material = new DielectricOpaque(r->texture.get(), XMVectorReplicate(m->smoothness));
            break;
    }
    return r;
}
void ref_material_free(ref_material* m) { delete m; }
void ref_material_counters(const ref_material* m, uint64_t counters[2]) { m->Counters(counters); }

void ref_scatter(ref_material* m, const float* in, uint32_t n, float* out, uint64_t* counters) {
    for (uint32_t k = 0; k < n; ++k) {
        const float* q = in + 14 * k;
        const Ray ray = LoadRay(q);
        const Payload hit = LoadHit(q + 6);
        XMVECTOR atten = XMVectorZero();
        Ray scattered{XMVectorZero(), XMVectorZero()};
        m->Counters(counters + 4 * k);
        const bool flag = m->material->Scatter(ray, hit, atten, scattered);
        m->Counters(counters + 4 * k + 2);
        float* w = out + 10 * k;
        w[0] = flag ? 1.f : 0.f;
        w[1] = atten.x; w[2] = atten.y; w[3] = atten.z;
        w[4] = scattered.origin.x; w[5] = scattered.origin.y; w[6] = scattered.origin.z;
        w[7] = scattered.direction.x; w[8] = scattered.direction.y; w[9] = scattered.direction.z;
    }
}

void ref_emit(const ref_material* m, const float* hits, uint32_t n, float* out) {
    for (uint32_t k = 0; k < n; ++k) {
        const XMVECTOR v = m->material->Emit(LoadHit(hits + 8 * k));
        out[3 * k] = v.x; out[3 * k + 1] = v.y; out[3 * k + 2] = v.z;
    }
}

void ref_shade(const ref_material* m, const float* hits, uint32_t n, const rt_light* lights, uint32_t n_lights,
               const float vo[3], const ref_scene* occluders, float* out, uint8_t* out_occluded) {
    std::vector<uint8_t> log;
    const auto list = LightsOf(lights, n_lights, occluders, &log);
    const XMVECTOR viewOrigin = XMVectorSet(vo[0], vo[1], vo[2], 1.f);
    for (uint32_t k = 0; k < n; ++k) {
        log.clear();
        const XMVECTOR v = m->material->Shade(LoadHit(hits + 8 * k), list, viewOrigin);
        out[3 * k] = v.x; out[3 * k + 1] = v.y; out[3 * k + 2] = v.z;
        if (out_occluded)
            for (uint32_t q = 0; q < n_lights; ++q) out_occluded[(size_t)k * n_lights + q] = q < log.size() ? log[q] : 0xff;
    }
}

void ref_light_shade(const ref_material* m, const float* hits, uint32_t n, const rt_light* light, const float vo[3],
                     const ref_scene* occluders, float* out) {
    const auto list = LightsOf(light, 1, occluders, nullptr);
    const XMVECTOR viewOrigin = XMVectorSet(vo[0], vo[1], vo[2], 1.f);
    for (uint32_t k = 0; k < n; ++k) {
        const XMVECTOR v = list[0]->Shade(m->material, LoadHit(hits + 8 * k), viewOrigin);
        out[3 * k] = v.x; out[3 * k + 1] = v.y; out[3 * k + 2] = v.z;
    }
}

void ref_light_make(const float dir[3], float r, float g, float b, float luminance, rt_light* out) {
    const DirectionalLight l(XMVectorSet(dir[0], dir[1], dir[2], 0.f), XMCOLOR(r, g, b, 1.f), luminance, [](const Ray&) { return false; });
    out->direction[0] = l.m_direction.x; out->direction[1] = l.m_direction.y; out->direction[2] = l.m_direction.z;
    out->color[0] = l.m_color.x; out->color[1] = l.m_color.y; out->color[2] = l.m_color.z;
    out->luminance = l.m_luminance;
}

}  // extern "C"
