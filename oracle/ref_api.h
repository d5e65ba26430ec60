/* ORACLE — TEST INFRASTRUCTURE ONLY.  C ABI of oracle/_ref/libref.so: the reference's OWN translation units
 * (quasi-random.cpp, texture.cpp, light.cpp, camera.cpp, material.cpp, ray-tracing.cpp, compiled unmodified from $(REFERENCE)
 * over the stand-in headers of oracle/ref_shim/) behind the POD records of include/rt_api.h.  ref_driver.cpp builds the
 * reference's objects from those records, calls their methods and copies the results out; it restates no method of theirs.
 * tests/test_reference_code_cpu.py compares the oracle (oracle_api.h) with this library function by function, bit for bit.
 * Nothing here is thread safe (the reference's material counters are not): every call sequence is serial.
 * All batched calls take n items; hits are 10 floats as in orc_unit_closest_hit: t, index (int32 bits, -1 = miss), pos xyz,
 * normal xyz, uv; a miss is all zeros but the index. */
#ifndef REF_API_H
#define REF_API_H
#include "../include/rt_api.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Random::HaltonSample* (quasi-random.cpp) at 64-bit indices */
void ref_halton(const uint64_t* index, uint32_t n, uint32_t base, float* out);
void ref_halton_2d(const uint64_t* index, uint32_t n, uint32_t b1, uint32_t b2, float* out2);
void ref_halton_ring(const uint64_t* index, uint32_t n, uint32_t base, float* out2);
void ref_halton_disk(const uint64_t* index, uint32_t n, uint32_t b1, uint32_t b2, float* out2);
void ref_halton_hemisphere(const uint64_t* index, uint32_t n, uint32_t b1, uint32_t b2, float* out3);
/* the C library functions the reference's objects are linked against: op 0 sin, 1 cos, 2 pow(x,y), 3 tan, 4 sqrt */
int ref_libm(uint32_t op, const float* x, const float* y, uint32_t n, float* out);

/* Sphere::Intersect for one sphere.  The reference passes no tmin/tmax: its only bound is the bias inside Intersect. */
void ref_sphere_intersect(const rt_sphere* sphere, const float* rays6, uint32_t n, float* out_hits10);

/* A sphere list held twice: as a plain list (ref_list_closest: Sphere::Intersect for every sphere in list order, a strictly
 * smaller t replaces the candidate -- the reference has no list class, this loop is the driver's) and inside a BvhNode built by
 * the reference's constructor after std::srand(bvh_srand) (its split axes are std::rand() % 3 of THIS C library). */
typedef struct ref_scene ref_scene;
ref_scene* ref_scene_new(const rt_sphere* spheres, uint32_t n, uint32_t bvh_srand);
void ref_scene_free(ref_scene* s);
void ref_list_closest(const ref_scene* s, const float* rays6, uint32_t n, float* out_hits10);
void ref_bvh_closest(const ref_scene* s, const float* rays6, uint32_t n, float* out_hits10);

/* Camera::Camera (origin and look-at with w = 1, as the oracle's orc_camera_make passes them) -> every member */
void ref_camera_make(const float origin[3], const float look_at[3], float vfov, float aspect, float focal, float aperture,
                     rt_camera* out);
/* Camera::GetRay of a camera holding exactly the members of *camera; in: uv.x uv.y offset.x offset.y; out: origin, direction */
void ref_camera_ray(const rt_camera* camera, const float* uv_offset4, uint32_t n, float* out_rays6);

/* ConstTexture / CheckerTexture built from the material record's texture fields; out: the XMVECTOR (4 floats) per uv */
void ref_texture_eval(const rt_material* m, const float* uv2, uint32_t n, float* out4);

/* One material object (with its texture) of the record's kind; its Halton counters start at 0 and live as long as it does. */
typedef struct ref_material ref_material;
ref_material* ref_material_new(const rt_material* m);
void ref_material_free(ref_material* m);
/* counters[0] = m_sampleIndex, counters[1] = m_reflectionProbabilitySampleIndex (0 where the class has no such member) */
void ref_material_counters(const ref_material* m, uint64_t counters[2]);
/* Material::Scatter.  in (14 floats): ray origin xyz, ray direction xyz, hit pos xyz, hit normal xyz, uv.  out (10 floats):
 * scattered flag, attenuation xyz, scattered origin xyz, scattered direction xyz (outputs the reference leaves unwritten read
 * 0).  counters (4 per hit): m_sampleIndex and m_reflectionProbabilitySampleIndex before, then after the call. */
void ref_scatter(ref_material* m, const float* in14, uint32_t n, float* out10, uint64_t* counters4);
/* Material::Emit; in (8 floats): hit pos xyz, normal xyz, uv; out: xyz */
void ref_emit(const ref_material* m, const float* hits8, uint32_t n, float* out3);
/* Material::Shade with DirectionalLights in list order.  Each is built by the reference's constructor and then given the record's
 * direction and colour as they stand (an rt_light holds the members AFTER the constructor; normalising a normalised vector
 * again may move its last bit).  occluders: a light is occluded when any sphere of the scene is hit
 * by Sphere::Intersect (NULL: nothing occludes).  out_occluded (n * n_lights bytes, may be NULL): 1 occluded, 0 visible. */
void ref_shade(const ref_material* m, const float* hits8, uint32_t n, const rt_light* lights, uint32_t n_lights,
               const float view_origin[3], const ref_scene* occluders, float* out3, uint8_t* out_occluded);
/* DirectionalLight::Shade of one light alone */
void ref_light_shade(const ref_material* m, const float* hits8, uint32_t n, const rt_light* light, const float view_origin[3],
                     const ref_scene* occluders, float* out3);

/* DirectionalLight::DirectionalLight(dir, XMCOLOR(r, g, b, 1), luminance) -> its members as an rt_light */
void ref_light_make(const float dir[3], float r, float g, float b, float luminance, rt_light* out);

#ifdef __cplusplus
}
#endif
#endif
