// spheres-app.cpp — headless SpheresApp for MI355X (mirror of src/spheres/spheres-app.cpp).
#include "spheres-app.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>

namespace {
[[noreturn]] void ThrowRt(const char* where) { throw std::runtime_error(std::string(where) + ": " + rt_last_error()); }
#define RT_CALL(expr)                         \
    do {                                      \
        if ((expr) != RT_OK) ThrowRt(#expr);  \
    } while (0)
}  // namespace

// ------------------------------------------------------------------ RayTracingApp (app.cpp)
void RayTracingApp::Initialize(int deviceOrdinal) {  // app.cpp:16-54 minus RegisterClass/CreateWindow/InitDirect2D
    m_deviceOrdinal = deviceOrdinal;
    RT_CALL(rt_create(deviceOrdinal, &m_device));  // fails loudly without a GPU: there is no CPU render path
    InitBuffers();
    OnInitialize();
}
void RayTracingApp::InitBuffers() {  // app.cpp:112-119
    const size_t n = (size_t)GetBackBufferWidth() * GetBackBufferHeight();
    m_backbufferHdr.assign(n, XMVectorZero());
    m_backbufferLdr.assign(n, XMCOLOR(0.f, 0.f, 0.f, 0.f));
}
int RayTracingApp::Run(uint32_t frames) noexcept {  // app.cpp:56-76
    try {
        for (uint32_t f = 0; f < frames; ++f) {
            BeforeFrame(f, frames);
            OnRender();
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "spheres: %s\n", e.what());
        return 1;
    }
    return 0;
}

// ------------------------------------------------------------------------------ SpheresApp
SpheresApp::~SpheresApp() {
    if (m_device) rt_destroy(m_device);
}

void SpheresApp::OnInitialize() {  // spheres-app.cpp:4-8
    InitCamera();
    InitScene();
}

void SpheresApp::InitCamera() {  // spheres-app.cpp:35-49
    if (AppSettings.scene == "three") {  // SURVEY.md §8(d) C1 camera
        m_camera = std::make_unique<Camera>(XMVectorSet(0.f, 0.f, 0.f, 1.f), XMVectorSet(0.f, 0.f, 1.f, 1.f), AppSettings.k_verticalFov,
                                            AppSettings.AspectRatio(), 1.f, AppSettings.k_aperture);
        m_lookAt[0] = 0.f, m_lookAt[1] = 0.f, m_lookAt[2] = 1.f;
    } else {
        XMVECTOR camOrigin = XMVectorSet(12.f, 2.f, -2.5f, 1.f);
        XMVECTOR camLookAt = XMVectorSet(0, 1, 0, 1.f);
        m_camera = std::make_unique<Camera>(camOrigin, camLookAt, AppSettings.k_verticalFov, AppSettings.AspectRatio(),
                                            XMVectorGetX(XMVector3Length(camOrigin - camLookAt)), AppSettings.k_aperture);
        m_lookAt[0] = 0.f, m_lookAt[1] = 1.f, m_lookAt[2] = 0.f;
    }
    m_exposure = -15;
}

void SpheresApp::InitScene() {  // spheres-app.cpp:51-130
    // std::random_device seeding (:53-54) replaced by a fixed seed; uniform_real_distribution
    // (implementation defined) replaced by engine() * 2^-24.
    std::ranlux24_base generator((std::ranlux24_base::result_type)AppSettings.sceneSeed);
    auto uniformDist = [&generator]() -> float { return (float)generator() * 0x1p-24f; };

    m_scene.clear();
    m_textures.clear();
    m_lights.clear();
    m_scene.reserve(500);

    if (AppSettings.scene == "three") {
        const float cols[3][3] = {{0.5f, 0.5f, 0.5f}, {0.8f, 0.3f, 0.3f}, {0.8f, 0.8f, 0.0f}};
        const float geo[3][4] = {{0.f, 0.f, 1.f, 0.5f}, {1.f, 0.f, 1.f, 0.5f}, {0.f, -100.5f, 1.f, 100.f}};
        for (int k = 0; k < 3; ++k) {
            m_textures.push_back(std::make_unique<ConstTexture>(XMCOLOR{cols[k][0], cols[k][1], cols[k][2], 1.f}));
            m_scene.push_back(std::make_unique<Sphere>(XMVECTORF32{geo[k][0], geo[k][1], geo[k][2], 0.f}, geo[k][3],
                                                       std::make_unique<DielectricOpaque>(m_textures.back().get(), XMVectorReplicate(16.f))));
        }
    } else {
        const int lo = AppSettings.scene == "grid10k" ? -50 : -11;
        const int hi = AppSettings.scene == "grid10k" ? 50 : 11;
        // Floor
        m_textures.push_back(std::make_unique<CheckerTexture>(XMCOLOR{0.9f, 0.9f, 0.9f, 1.f}, XMCOLOR{0.2f, 0.3f, 0.1f, 1.f}, 2500.f));
        m_scene.push_back(std::make_unique<Sphere>(XMVECTORF32{0, -1000, 0, 0}, 1000.f,
                                                   std::make_unique<DielectricOpaque>(m_textures.back().get(), XMVectorReplicate(16.f))));
        // Random small spheres
        for (int a = lo; a < hi; ++a) {
            for (int b = lo; b < hi; ++b) {
                const float chooseMat = uniformDist();
                const float cx = a + 0.9f * uniformDist();
                const float cz = b + 0.9f * uniformDist();
                XMVECTORF32 center{cx, 0.2f, cz, 0.f};
                if (chooseMat < 0.8f) {
                    const float r0 = uniformDist(), r1 = uniformDist(), g0 = uniformDist(), g1 = uniformDist(), b0 = uniformDist(), b1 = uniformDist();
                    m_textures.push_back(std::make_unique<ConstTexture>(XMCOLOR{r0 * r1, g0 * g1, b0 * b1, 1.f}));
                    float smoothness = 8.f * (4.f + uniformDist());
                    m_scene.push_back(std::make_unique<Sphere>(center, 0.2f, std::make_unique<DielectricOpaque>(m_textures.back().get(), XMVectorReplicate(smoothness))));
                } else if (chooseMat < 0.95f) {
                    const float r = uniformDist(), g = uniformDist(), bl = uniformDist();
                    m_textures.push_back(std::make_unique<ConstTexture>(XMCOLOR{0.5f * (1.f + r), 0.5f * (1.f + g), 0.5f * (1.f + bl), 1.f}));
                    m_scene.push_back(std::make_unique<Sphere>(center, 0.2f, std::make_unique<Metal>(m_textures.back().get(), XM_Zero)));
                } else {
                    float smoothness = 8.f * (4.f + uniformDist());
                    m_scene.emplace_back(std::make_unique<Sphere>(center, 0.2f, std::make_unique<DielectricTransparent>(XMVectorReplicate(smoothness), 1.5f)));
                }
            }
        }
        // Large spheres
        m_scene.push_back(std::make_unique<Sphere>(XMVECTORF32{0, 1, 0, 0}, 1.f, std::make_unique<DielectricTransparent>(XMVectorReplicate(16.f), 1.5f)));
        m_textures.push_back(std::make_unique<ConstTexture>(XMCOLOR{0.4f, 0.2f, 0.1f, 1.f}));
        m_scene.push_back(std::make_unique<Sphere>(XMVECTORF32{-4, 1, 0, 0}, 1.f, std::make_unique<DielectricOpaque>(m_textures.back().get(), XMVectorReplicate(16.f))));
        m_textures.push_back(std::make_unique<ConstTexture>(XMCOLOR{0.7f, 0.6f, 0.5f, 1.f}));
        m_scene.push_back(std::make_unique<Sphere>(XMVECTORF32{4, 1, 0, 0}, 1.f, std::make_unique<Metal>(m_textures.back().get(), XM_Zero)));
    }

    // Construct BVH (moves the unique_ptrs out of m_scene, as the reference does)
    m_bvh = std::make_unique<BvhNode>(m_scene.begin(), m_scene.end());

    // Sky
    m_textures.push_back(std::make_unique<ConstTexture>(XMCOLOR{0.85f, 0.91f, 0.98f, 1.f}));
    m_skyMaterial = std::make_unique<Emissive>(8000.f, m_textures.back().get());

    // Sun
    auto lightOcclusionTest = [this](const Ray& ray) -> bool {
        Payload dummy{};
        return m_bvh->Intersect(ray, dummy);
    };
    m_lights.push_back(std::make_unique<DirectionalLight>(XMVECTORF32{1.f, 1.f, 1.f, 0.f}, XMCOLOR{1.f, 0.97f, 0.88f, 1.f}, 40000.f, lightOcclusionTest));
    m_uploaded = false;
}

void SpheresApp::DescribeScene(std::vector<rt_sphere>& spheres, std::vector<rt_material>& materials, rt_camera& camera,
                               std::vector<rt_light>& lights, rt_material& sky, float& exposureScale) const {
    spheres.clear();
    materials.clear();
    m_bvh->Flatten(spheres, materials);
    camera = m_camera->Describe();
    lights.clear();  // every light of the list, in list order (Material::Shade adds them in that order, material.cpp:4-13)
    for (const auto& l : m_lights) lights.push_back(l->Describe());
    sky = m_skyMaterial->Describe();
    exposureScale = static_cast<float>(std::pow(2, m_exposure));  // spheres-app.cpp:174
}

void SpheresApp::OnRender() {  // spheres-app.cpp:10-33 minus BeginPaint/BeginDraw
    const auto start = std::chrono::high_resolution_clock::now();
    const size_t rayCount = DrawBitmap();
    const auto stop = std::chrono::high_resolution_clock::now();
    const std::chrono::duration<double, std::micro> duration = stop - start;
    DisplayStats(rayCount, duration.count());
}

size_t SpheresApp::DrawBitmap() {  // spheres-app.cpp:163-222
    const uint32_t W = (uint32_t)GetBackBufferWidth(), H = (uint32_t)GetBackBufferHeight();
    if (!m_uploaded) {
        std::vector<rt_sphere> spheres;
        std::vector<rt_material> materials;
        rt_camera camera;
        std::vector<rt_light> lights;
        rt_material sky;
        float exposureAdjustment;
        DescribeScene(spheres, materials, camera, lights, sky, exposureAdjustment);
        RT_CALL(rt_scene_upload(m_device, spheres.data(), materials.data(), (uint32_t)spheres.size(), &camera, lights.data(), (uint32_t)lights.size(), &sky,
                                exposureAdjustment));
        RT_CALL(rt_set_sampler(m_device, AppSettings.samplerFlags));
        RT_CALL(rt_set_noise_estimate(m_device, AppSettings.noiseEstimate ? 1 : 0));
        RT_CALL(rt_set_frame_pipelining(m_device, AppSettings.framesInFlight));
        RT_CALL(rt_set_frame_batch(m_device, AppSettings.framesPerLaunch ? AppSettings.framesPerLaunch : 1u));
        m_uploaded = true;
    }
    const rt_rowset rs = m_hasRowset ? m_rowset : rt_rowset{0, H, H, 0, 1};
    const uint32_t s0 = (uint32_t)m_sampleCount + 1;  // ++m_sampleCount (:168): first frame uses index 1
    const uint32_t s1 = s0 + AppSettings.samplesPerFrame;
    // GenerateRays + trace (:171-184) and the tonemap (:196-214) on the device
    // per-frame statistics cost a host wait; a quiet progressive run stays asynchronous until the last frame
    rt_stats* wantStats = (m_quiet && !m_lastFrame) ? nullptr : &m_lastStats;
    RT_CALL(rt_render(m_device, W, H, rs, s0, s1, (uint32_t)AppSettings.k_recursionDepth, AppSettings.renderSeed, wantStats));
    if (!wantStats) m_lastStats.local_rows = rt_rowset_local_rows(rs);
    m_sampleCount += AppSettings.samplesPerFrame;
    if (wantStats) {  // the tonemap feeds the display in the reference; headless and quiet, only the last frame needs it
        RT_CALL(rt_resolve(m_device, (uint32_t)m_sampleCount));
        m_lastStats.ms_resolve = rt_last_resolve_ms(m_device);
    }
    return (size_t)W * m_lastStats.local_rows * AppSettings.samplesPerFrame;
}

bool SpheresApp::WritePPM(const std::string& path) const {
    const uint32_t W = (uint32_t)GetBackBufferWidth();
    const uint32_t rows = m_lastStats.local_rows;
    std::vector<uint8_t> rgb((size_t)W * rows * 3);
    if (rt_download(m_device, nullptr, rgb.data()) != RT_OK) return false;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "P6\n%u %u\n255\n", W, rows);
    const bool ok = std::fwrite(rgb.data(), 1, rgb.size(), f) == rgb.size();
    std::fclose(f);
    return ok;
}

bool SpheresApp::WriteNoisePFM(const std::string& path) const {
    const uint32_t W = (uint32_t)GetBackBufferWidth();
    const uint32_t rows = m_lastStats.local_rows;
    std::vector<float> map((size_t)W * rows * 2), abs((size_t)W * rows);
    if (rt_noise_map(m_device, AppSettings.noiseFloor, map.data()) != RT_OK) return false;
    for (size_t p = 0; p < abs.size(); ++p) abs[p] = map[2 * p];
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "Pf\n%u %u\n-1.0\n", W, rows);
    const bool ok = std::fwrite(abs.data(), sizeof(float), abs.size(), f) == abs.size();
    std::fclose(f);
    return ok;
}

bool SpheresApp::WriteFeaturePFMs(const std::string& prefix) const {
    const uint32_t W = (uint32_t)GetBackBufferWidth(), H = (uint32_t)GetBackBufferHeight();
    const uint32_t rows = m_lastStats.local_rows;
    if (m_sampleCount == 0) return false;
    const rt_rowset rs = m_hasRowset ? m_rowset : rt_rowset{0, H, H, 0, 1};
    if (rt_render_features(m_device, W, H, rs, 1u, (uint32_t)m_sampleCount + 1u, nullptr) != RT_OK) return false;
    const size_t npix = (size_t)W * rows;
    std::vector<float> feat(npix * 8);
    if (rt_download_features(m_device, feat.data(), nullptr) != RT_OK) return false;
    const float n = (float)m_sampleCount;
    struct Plane {
        const char* name;
        uint32_t first, channels;
    };
    const Plane planes[4] = {{"albedo", 0, 3}, {"normal", 3, 3}, {"depth", 6, 1}, {"coverage", 7, 1}};
    for (const Plane& pl : planes) {
        std::vector<float> out(npix * pl.channels);
        for (size_t p = 0; p < npix; ++p)
            for (uint32_t c = 0; c < pl.channels; ++c) out[p * pl.channels + c] = feat[p * 8 + pl.first + c] / n;
        FILE* f = std::fopen((prefix + "." + pl.name + ".pfm").c_str(), "wb");
        if (!f) return false;
        std::fprintf(f, "%s\n%u %u\n-1.0\n", pl.channels == 3 ? "PF" : "Pf", W, rows);
        const bool ok = std::fwrite(out.data(), sizeof(float), out.size(), f) == out.size();
        std::fclose(f);
        if (!ok) return false;
    }
    return true;
}

bool SpheresApp::WriteDenoisedPPM(const std::string& path, uint32_t levels, const rt_variance_params* variance) const {
    const uint32_t W = (uint32_t)GetBackBufferWidth(), H = (uint32_t)GetBackBufferHeight();
    const uint32_t rows = m_lastStats.local_rows;
    if (m_sampleCount == 0) return false;
    const rt_rowset rs = m_hasRowset ? m_rowset : rt_rowset{0, H, H, 0, 1};
    if (rt_render_features(m_device, W, H, rs, 1u, (uint32_t)m_sampleCount + 1u, nullptr) != RT_OK) return false;
    rt_denoise_params params;
    if (rt_denoise_default_params(&params) != RT_OK) return false;
    if (levels != 0) params.levels = levels;
    if ((variance ? rt_denoise_variance(m_device, &params, variance, nullptr) : rt_denoise(m_device, &params, nullptr)) != RT_OK) return false;
    std::vector<uint8_t> rgb((size_t)W * rows * 3);
    if (rt_download_denoised(m_device, nullptr, nullptr, rgb.data()) != RT_OK) return false;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "P6\n%u %u\n255\n", W, rows);
    const bool ok = std::fwrite(rgb.data(), 1, rgb.size(), f) == rgb.size();
    std::fclose(f);
    return ok;
}

rt_camera OrbitCamera(const rt_camera& camera, double degrees, const float pivot[3]) {
    const double a = degrees * (3.14159265358979323846 / 180.0);
    const double c = std::cos(a), s = std::sin(a);
    rt_camera out = camera;
    const float* src[4] = {camera.origin, camera.origin_image_plane, camera.x, camera.y};
    float* dst[4] = {out.origin, out.origin_image_plane, out.x, out.y};
    for (int k = 0; k < 4; ++k) {
        const bool point = k < 2;
        double v[3];
        for (int j = 0; j < 3; ++j) v[j] = point ? (double)src[k][j] - (double)pivot[j] : (double)src[k][j];
        const double r[3] = {c * v[0] + s * v[2], v[1], -s * v[0] + c * v[2]};
        for (int j = 0; j < 3; ++j) dst[k][j] = (float)(point ? r[j] + (double)pivot[j] : r[j]);
    }
    return out;
}

int SpheresApp::RunOrbit(uint32_t frames, double degPerFrame, uint32_t spp, uint32_t levels, uint32_t fetch, const rt_variance_params* variance) noexcept {
    try {
        const bool spatial = variance && variance->source == RT_VARIANCE_SPATIAL;
        const uint32_t W = (uint32_t)GetBackBufferWidth(), H = (uint32_t)GetBackBufferHeight();
        const rt_rowset rs = m_hasRowset ? m_rowset : rt_rowset{0, H, H, 0, 1};
        std::vector<rt_sphere> spheres;
        std::vector<rt_material> materials;
        rt_camera camera;
        std::vector<rt_light> lights;
        rt_material sky;
        float exposureAdjustment;
        DescribeScene(spheres, materials, camera, lights, sky, exposureAdjustment);
        rt_denoise_params params;
        RT_CALL(rt_denoise_default_params(&params));
        if (levels != 0) params.levels = levels;
        RT_CALL(rt_temporal_reset(m_device));
        for (uint32_t f = 0; f < frames; ++f) {
            const rt_camera turned = OrbitCamera(camera, (double)f * degPerFrame, m_lookAt);
            if (f == 0) {  // one upload; every later frame only moves the camera (rt_set_camera keeps the scene tables and the settings)
                RT_CALL(rt_scene_upload(m_device, spheres.data(), materials.data(), (uint32_t)spheres.size(), &turned, lights.data(), (uint32_t)lights.size(),
                                        &sky, exposureAdjustment));
                RT_CALL(rt_set_sampler(m_device, AppSettings.samplerFlags));
                RT_CALL(rt_set_noise_estimate(m_device, spatial ? (AppSettings.noiseEstimate ? 1 : 0) : 1));
                RT_CALL(rt_set_frame_pipelining(m_device, 0));
                RT_CALL(rt_set_frame_batch(m_device, 1u));
                m_uploaded = true;
            } else {
                RT_CALL(rt_set_camera(m_device, &turned));
            }
            RT_CALL(rt_render(m_device, W, H, rs, 1u, 1u + spp, (uint32_t)AppSettings.k_recursionDepth, AppSettings.renderSeed + f, &m_lastStats));
            m_sampleCount = spp;
            RT_CALL(rt_resolve(m_device, spp));
            m_lastStats.ms_resolve = rt_last_resolve_ms(m_device);
            RT_CALL(rt_render_features(m_device, W, H, rs, 1u, 1u + spp, nullptr));
            if (variance)
                RT_CALL(rt_denoise_temporal_variance(m_device, &params, nullptr, fetch, variance, nullptr));
            else if (fetch == RT_TEMPORAL_FETCH_NEAREST)
                RT_CALL(rt_denoise_temporal(m_device, &params, nullptr, nullptr));
            else
                RT_CALL(rt_denoise_temporal_fetch(m_device, &params, nullptr, fetch, nullptr));
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "spheres: %s\n", e.what());
        return 1;
    }
    return 0;
}

bool SpheresApp::WriteTemporalPPM(const std::string& path) const {
    const uint32_t W = (uint32_t)GetBackBufferWidth();
    const uint32_t rows = m_lastStats.local_rows;
    std::vector<uint8_t> rgb((size_t)W * rows * 3);
    if (rt_download_denoised(m_device, nullptr, nullptr, rgb.data()) != RT_OK) return false;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    std::fprintf(f, "P6\n%u %u\n255\n", W, rows);
    const bool ok = std::fwrite(rgb.data(), 1, rgb.size(), f) == rgb.size();
    std::fclose(f);
    return ok;
}

int SpheresApp::RunUntil(float relError, double fraction, uint32_t maxSpp) noexcept {
    try {
        const uint32_t step = AppSettings.samplesPerFrame;
        for (;;) {
            m_lastFrame = true;
            OnRender();
            if (m_sampleCount >= 2) {
                uint32_t above = 0;
                RT_CALL(rt_noise_summary(m_device, AppSettings.noiseFloor, &relError, 1, &above, nullptr));
                const double npix = (double)GetBackBufferWidth() * m_lastStats.local_rows;
                if ((double)above / npix <= fraction) break;
            }
            if (m_sampleCount + step > maxSpp) break;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "spheres: %s\n", e.what());
        return 1;
    }
    return 0;
}

void SpheresApp::DisplayStats(const size_t rayCount, const double timeElapsed) const {  // spheres-app.cpp:259-272 -> stdout JSON
    m_totalSeconds += timeElapsed * std::pow(10, -6);
    const double mraysPerSecond = static_cast<double>(rayCount) / timeElapsed;
    if (m_quiet) return;
    std::printf("{\"Mrays_per_s\": %.3f, \"spp\": %zu, \"time_s\": %.6f, \"kernel_ms\": %.3f, \"traversals_per_sample\": %.4f}\n", mraysPerSecond,
                m_sampleCount, m_totalSeconds, m_lastStats.ms_render + m_lastStats.ms_accumulate + m_lastStats.ms_resolve,
                m_lastStats.samples ? (double)m_lastStats.traversals / (double)m_lastStats.samples : 0.0);
}

int SpheresApp::GetBackBufferWidth() const { return AppSettings.k_backbufferWidth; }    // spheres-app.cpp:274-277
int SpheresApp::GetBackBufferHeight() const { return AppSettings.k_backbufferHeight; }  // spheres-app.cpp:279-282
