// main.cpp — headless replacement for src/spheres/main.cpp (WinMain, main.cpp:5-10): builds the
// app, renders `--spp` samples on MI355X through librt_hip.so and writes a PPM.  The reference has
// no command line; the flags below are new surface with AppSettings defaults.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "multi_gpu.h"
#include "spheres-app.h"

static void Usage() {
    std::puts("usage: spheres [--width N] [--height N] [--spp N] [--frame-spp N] [--depth N] [--fov F] [--aperture F]\n"
              "               [--scene cover|three|grid10k] [--scene-seed N] [--seed N] [--device N] [--gpus N] [--out file.ppm] [--quiet]\n"
              "               [--sampler reference|cosine|sqrtdisk|cosine+sqrtdisk]   (default: the reference's mappings)\n"
              "               [--pipeline N]   frames in flight for quiet progressive runs (--frame-spp 1 --quiet); 0 = off\n"
              "               [--batch N]      quiet progressive frames rendered per launch (rt_set_frame_batch); 1 = off\n"
              "               [--noise-out file.pfm]   per-pixel standard error of the image (HDR units) as a one-channel PFM, rows top to bottom\n"
              "               [--features-out PREFIX]  first-hit feature buffers of the rendered samples, as means: PREFIX.albedo.pfm and\n"
              "                                PREFIX.normal.pfm (three channels), PREFIX.depth.pfm and PREFIX.coverage.pfm (one channel)\n"
              "               [--denoise-out file.ppm [--denoise-levels N]]   the picture after the feature-guided a-trous filter (rt_denoise, N = 1..5\n"
              "                                levels, default 3), written beside --out, which is unchanged; needs --spp >= 2\n"
              "               [--denoise-variance moments|spatial [--denoise-radius R]]   with --denoise-out: where the filter's variance comes from\n"
              "                                (rt_denoise_variance).  moments (default): the second moments, --spp >= 2.  spatial: the picture's own\n"
              "                                (2R+1)^2 neighbourhoods (R = 1..3, default 1), so --spp 1 is enough -- with --orbit-frames too -- and the\n"
              "                                noise estimate is not switched on for the filter's sake\n"
              "               [--orbit-frames K [--orbit-deg D] [--orbit-fetch nearest|bilinear]]   with --denoise-out: K pictures of --spp samples each (seed --seed + f) from a camera\n"
              "                                that turns D degrees (default 0.5) per picture about the scene's look-at point, each followed by the\n"
              "                                feature pass and rt_denoise_temporal; the last picture is written.  --orbit-fetch bilinear\n"
              "                                interpolates the history (rt_denoise_temporal_fetch with that fetch's defaults); default nearest\n"
              "               [--target-error T [--target-fraction F] [--max-spp N]]   render --frame-spp samples at a time until at most the\n"
              "                                fraction F (default 0) of the pixels has a relative error above T, or N (default --spp) is reached\n"
              "               [--noise-floor F]        added to a pixel's r + g + b before the relative error divides by it (default 0.01)");
}

int main(int argc, char** argv) {
    AppSettingsT st;
    uint32_t spp = 16;
    int device = 0, gpus = 0;
    std::string out = "out.ppm", noiseOut, featuresOut, denoiseOut;
    uint32_t denoiseLevels = 0;  // 0: the default
    uint32_t orbitFrames = 0;
    double orbitDeg = 0.5;
    bool orbitSet = false;
    uint32_t orbitFetch = RT_TEMPORAL_FETCH_NEAREST;
    rt_variance_params variance;
    rt_variance_default_params(&variance);
    bool varianceSet = false;
    float targetError = 0.f;
    double targetFraction = 0.0;
    uint32_t maxSpp = 0;
    bool targetSet = false;
    bool quiet = false, fovSet = false, apSet = false;
    for (int a = 1; a < argc; ++a) {
        const std::string k = argv[a];
        auto val = [&]() -> const char* {
            if (a + 1 >= argc) { Usage(); std::exit(2); }
            return argv[++a];
        };
        if (k == "--width") st.k_backbufferWidth = std::atoi(val());
        else if (k == "--height") st.k_backbufferHeight = std::atoi(val());
        else if (k == "--spp") spp = (uint32_t)std::atoi(val());
        else if (k == "--frame-spp") st.samplesPerFrame = (uint32_t)std::atoi(val());
        else if (k == "--depth") st.k_recursionDepth = std::atoi(val());
        else if (k == "--fov") { st.k_verticalFov = (float)std::atof(val()); fovSet = true; }
        else if (k == "--aperture") { st.k_aperture = (float)std::atof(val()); apSet = true; }
        else if (k == "--scene") st.scene = val();
        else if (k == "--scene-seed") st.sceneSeed = std::strtoull(val(), nullptr, 10);
        else if (k == "--seed") st.renderSeed = std::strtoull(val(), nullptr, 10);
        else if (k == "--device") device = std::atoi(val());
        else if (k == "--gpus") gpus = std::atoi(val());
        else if (k == "--out") out = val();
        else if (k == "--quiet") quiet = true;
        else if (k == "--pipeline") st.framesInFlight = (uint32_t)std::atoi(val());
        else if (k == "--batch") st.framesPerLaunch = (uint32_t)std::atoi(val());
        else if (k == "--noise-out") noiseOut = val();
        else if (k == "--features-out") featuresOut = val();
        else if (k == "--denoise-out") denoiseOut = val();
        else if (k == "--denoise-levels") denoiseLevels = (uint32_t)std::atoi(val());
        else if (k == "--denoise-variance") {
            const std::string v = val();
            if (v != "moments" && v != "spatial") { Usage(); return 2; }
            variance.source = v == "spatial" ? RT_VARIANCE_SPATIAL : RT_VARIANCE_MOMENTS;
            varianceSet = true;
        }
        else if (k == "--denoise-radius") { variance.radius = (uint32_t)std::atoi(val()); varianceSet = true; }
        else if (k == "--orbit-frames") { orbitFrames = (uint32_t)std::atoi(val()); orbitSet = true; }
        else if (k == "--orbit-deg") { orbitDeg = std::atof(val()); orbitSet = true; }
        else if (k == "--orbit-fetch") {
            const std::string v = val();
            if (v != "nearest" && v != "bilinear") { Usage(); return 2; }
            orbitFetch = v == "bilinear" ? RT_TEMPORAL_FETCH_BILINEAR : RT_TEMPORAL_FETCH_NEAREST;
            orbitSet = true;
        }
        else if (k == "--target-error") { targetError = (float)std::atof(val()); targetSet = true; }
        else if (k == "--target-fraction") targetFraction = std::atof(val());
        else if (k == "--max-spp") maxSpp = (uint32_t)std::atoi(val());
        else if (k == "--noise-floor") st.noiseFloor = (float)std::atof(val());
        else if (k == "--sampler") {
            const std::string v = val();
            st.samplerFlags = (v.find("cosine") != std::string::npos ? RT_SAMPLER_COSINE_HEMISPHERE : 0u) |
                              (v.find("sqrtdisk") != std::string::npos ? RT_SAMPLER_SQRT_DISK : 0u);
            if (st.samplerFlags == 0u && v != "reference") { Usage(); return 2; }
        }
        else { Usage(); return k == "--help" ? 0 : 2; }
    }
    if (st.scene == "three") {  // C1 defaults
        if (!fovSet) st.k_verticalFov = 90.f;
        if (!apSet) st.k_aperture = 0.f;
    }
    if (st.samplesPerFrame == 0 || spp == 0 || st.k_backbufferWidth <= 0 || st.k_backbufferHeight <= 0) { Usage(); return 2; }
    if (spp % st.samplesPerFrame != 0) st.samplesPerFrame = 1;
    if (orbitSet && (denoiseOut.empty() || gpus > 0 || targetSet)) {
        std::fprintf(stderr, "spheres: --orbit-frames, --orbit-deg and --orbit-fetch need --denoise-out and are not available with --gpus or --target-error\n");
        return 2;
    }
    if (varianceSet && denoiseOut.empty()) {
        std::fprintf(stderr, "spheres: --denoise-variance and --denoise-radius need --denoise-out\n");
        return 2;
    }
    const bool spatial = variance.source == RT_VARIANCE_SPATIAL;
    if (spatial && (variance.radius < 1 || variance.radius > 3)) { Usage(); return 2; }
    if (orbitSet && (orbitFrames == 0 || spp < (spatial ? 1u : 2u) || !(orbitDeg == orbitDeg))) { Usage(); return 2; }
    if (!denoiseOut.empty() && gpus > 0) {
        std::fprintf(stderr, "spheres: --denoise-out is not available with --gpus: the multi-GPU gather carries neither second moments nor feature strips\n");
        return 2;
    }
    st.noiseEstimate = targetSet || !noiseOut.empty() || (!denoiseOut.empty() && !spatial);  // (the spatial source reads no second moments)
    if (st.noiseEstimate && gpus > 0) {
        std::fprintf(stderr, "spheres: --noise-out and --target-error are not available with --gpus: the multi-GPU gather carries no second moments\n");
        return 2;
    }
    if (!featuresOut.empty() && gpus > 0) {
        std::fprintf(stderr, "spheres: --features-out is not available with --gpus: the multi-GPU gather carries no feature strips\n");
        return 2;
    }
    if (targetSet) {
        if (maxSpp == 0) maxSpp = spp;
        if (!(targetError > 0.f) || !(targetFraction >= 0.0) || maxSpp < 2 || maxSpp < st.samplesPerFrame) { Usage(); return 2; }
    }
    if (gpus > 0) {  // rows sharded over `gpus` devices, RCCL gather to device 0
        MultiGpuResult res;
        std::string err;
        if (RenderMultiGpu(st, gpus, spp, res, &err) != 0) {
            std::fprintf(stderr, "spheres: %s\n", err.c_str());
            return 1;
        }
        FILE* f = std::fopen(out.c_str(), "wb");
        if (!f) {
            std::fprintf(stderr, "spheres: cannot write %s\n", out.c_str());
            return 1;
        }
        std::fprintf(f, "P6\n%d %d\n255\n", st.k_backbufferWidth, st.k_backbufferHeight);
        std::fwrite(res.ldr.data(), 1, res.ldr.size(), f);
        std::fclose(f);
        std::printf("{\"out\": \"%s\", \"gpus\": %d, \"spp\": %u, \"render_s\": %.4f, \"Msamples_per_s\": %.2f, \"traversals_per_sample\": %.4f}\n",
                    out.c_str(), gpus, spp, res.renderSeconds, (double)res.samples / res.renderSeconds / 1e6,
                    res.samples ? (double)res.traversals / (double)res.samples : 0.0);
        return 0;
    }
    SpheresApp app(st);
    app.SetQuiet(quiet);
    try {
        app.Initialize(device);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "spheres: %s\n", e.what());
        return 1;
    }
    const int rc = orbitSet ? app.RunOrbit(orbitFrames, orbitDeg, spp, denoiseLevels, orbitFetch, varianceSet ? &variance : nullptr)
                            : (targetSet ? app.RunUntil(targetError, targetFraction, maxSpp) : app.Run(spp / st.samplesPerFrame));
    if (rc != 0) return rc;
    if (!noiseOut.empty() && !app.WriteNoisePFM(noiseOut)) {
        std::fprintf(stderr, "spheres: cannot write %s: %s\n", noiseOut.c_str(), rt_last_error());
        return 1;
    }
    if (!featuresOut.empty() && !app.WriteFeaturePFMs(featuresOut)) {
        std::fprintf(stderr, "spheres: cannot write the feature buffers %s.*.pfm: %s\n", featuresOut.c_str(), rt_last_error());
        return 1;
    }
    if (orbitSet) {
        if (!app.WriteTemporalPPM(denoiseOut)) {
            std::fprintf(stderr, "spheres: cannot write the denoised picture %s: %s\n", denoiseOut.c_str(), rt_last_error());
            return 1;
        }
    } else if (!denoiseOut.empty() && !app.WriteDenoisedPPM(denoiseOut, denoiseLevels, varianceSet ? &variance : nullptr)) {
        std::fprintf(stderr, "spheres: cannot write the denoised picture %s: %s\n", denoiseOut.c_str(), rt_last_error());
        return 1;
    }
    if (targetSet) std::printf("{\"target_error\": %g, \"target_fraction\": %g, \"spp_reached\": %zu}\n", (double)targetError, targetFraction, app.SampleCount());
    if (!app.WritePPM(out)) {
        std::fprintf(stderr, "spheres: cannot write %s\n", out.c_str());
        return 1;
    }
    const rt_stats& ls = app.LastStats();
    std::printf("{\"out\": \"%s\", \"spp\": %zu, \"total_s\": %.4f, \"last_frame_kernel_ms\": %.3f}\n", out.c_str(), app.SampleCount(),
                app.TotalSeconds(), ls.ms_render + ls.ms_accumulate + ls.ms_resolve);
    return 0;
}
