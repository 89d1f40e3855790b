// `pathtracer` command line tool: the reference's headless renderer (src/main.cpp:22-295) on
// MI355X.  Same options, defaults, messages and output semantics; additions:
//   -gpus N        render on N GPUs of this process (8-row bands interleaved over the devices,
//                  RCCL gather to device 0; bit-identical to 1 GPU)
//   -chunk N       samples per render() call of the headless loop (default 8, main.cpp:272)
//   -call_loop     one kernel launch per render() call, as main.cpp:272-279 (the default runs all
//                  render() calls of the loop in one launch: bit-identical and 1.37x faster at
//                  1080p x 1024 spp; -single_launch is accepted for compatibility)
//   -adaptive T    adaptive sampling (Pathtracer::renderAdaptive): calls of -chunk samples per pixel
//                  until the standard error of the pixel's luminance is below T x (|mean| + 0.01);
//                  -spp is the budget (at most spp / chunk calls), -minspp N the samples every pixel
//                  gets (default two calls).  One GPU.
//   -denoise [N]   filter the image before -o / -ohdr write it: the edge-avoiding a-trous denoiser guided
//                  by the first-hit feature buffers (Pathtracer::renderFeatures + denoise), N = 1..8
//                  iterations (default 5), the other parameters at their defaults.  One GPU.
//   -denoise_guide adaptive
//                  with -adaptive and -denoise: the filter's colour weight follows a per-pixel variance made from
//                  the adaptive render's own moments (Pathtracer::denoiseAdaptive) instead of one colour sigma
//                  for the image.  Without both of them the option is invalid.
//   -despike       clamp fireflies before -o / -ohdr write the image: a pixel far brighter than its same-surface
//                  neighbours is scaled down to their level (Pathtracer::renderFeatures + despike, the parameters
//                  at their defaults).  With -denoise the filter runs on the despiked image.  One GPU; not with
//                  -denoise_guide adaptive, whose variance describes the unclamped colour.
//   -upsample K    K = 2..4: trace (and -despike / -denoise) at ceil(w / K) x ceil(h / K), take the first-hit features at
//                  both sizes and reconstruct the w x h image from them (Pathtracer::upsample, rule 8 of pt_hip.h).
//                  One GPU; not with -denoise_guide adaptive.
//   -upsample_aa S S = 2..4, with -upsample K only: take the full-size features at S w x S h, S x S first-hit samples
//                  per pixel, and give every pixel the mean of the reconstruction at its samples, which antialiases
//                  the silhouettes (Pathtracer::upsample(lo, planes), rule 9 of pt_hip.h).
// The windowed / interactive mode (-window, -enable_controls) is not supported.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pathtracer_amd.hpp"

static bool processArgs(int argc, char* argv[], Params& params, int& gpus)
{
    const char* helpOption = "-help";
    const char* widthOption = "-w";
    const char* heightOption = "-h";
    const char* sppOption = "-spp";
    const char* windowOption = "-window";
    const char* controlsOption = "-enable_controls";
    const char* outputOption = "-o";
    const char* outputHdrOption = "-ohdr";
    params = {};
    gpus = 1;
    bool displayHelp = false;
    auto uintArg = [&](int i, const char* opt, unsigned int& dst) {
        if (i + 1 < argc) {
            dst = (unsigned int)atoi(argv[i + 1]);
            if (dst == 0) { printf("Invalid input for %s!\n", opt); displayHelp = true; }
        } else {
            printf("Missing argument to %s!\n", opt);
            displayHelp = true;
        }
    };
    int i = 1;
    for (; i < (argc - 1);) {
        if (strcmp(argv[i], helpOption) == 0) { displayHelp = true; ++i; continue; }
        if (strcmp(argv[i], widthOption) == 0) { uintArg(i, widthOption, params.m_width); i += 2; continue; }
        if (strcmp(argv[i], heightOption) == 0) { uintArg(i, heightOption, params.m_height); i += 2; continue; }
        if (strcmp(argv[i], sppOption) == 0) { uintArg(i, sppOption, params.m_spp); i += 2; continue; }
        if (strcmp(argv[i], windowOption) == 0) { params.m_showWindow = true; ++i; continue; }
        if (strcmp(argv[i], controlsOption) == 0) { params.m_enableControls = true; ++i; continue; }
        if (strcmp(argv[i], outputHdrOption) == 0) { params.m_outputHdr = true; ++i; continue; }
        if (strcmp(argv[i], outputOption) == 0) {
            if (i + 1 < argc) params.m_outputFilepath = argv[i + 1];
            else { printf("Missing argument to %s!\n", outputOption); displayHelp = true; }
            i += 2;
            continue;
        }
        if (strcmp(argv[i], "-gpus") == 0) {
            unsigned int g = 1;
            uintArg(i, "-gpus", g);
            gpus = (int)g;
            i += 2;
            continue;
        }
        if (strcmp(argv[i], "-chunk") == 0) { uintArg(i, "-chunk", params.m_chunk); i += 2; continue; }
        if (strcmp(argv[i], "-single_launch") == 0) { params.m_singleLaunch = true; ++i; continue; }
        if (strcmp(argv[i], "-call_loop") == 0) { params.m_singleLaunch = false; ++i; continue; }
        if (strcmp(argv[i], "-adaptive") == 0) {
            char* end = nullptr;
            const float t = i + 1 < argc ? strtof(argv[i + 1], &end) : -1.0f;
            if (i + 1 >= argc || end == argv[i + 1] || !(t >= 0.0f)) { printf("Invalid input for -adaptive!\n"); displayHelp = true; }
            else params.m_adaptive = t;
            i += 2;
            continue;
        }
        if (strcmp(argv[i], "-denoise") == 0) {
            // the iteration count is optional: the next argument is taken as it unless it is another
            // option or the input file (the last argument)
            params.m_denoise = PT_DENOISE_DEFAULT_ITERATIONS;
            if (i + 2 < argc && argv[i + 1][0] != '-') {
                char* end = nullptr;
                const long n = strtol(argv[i + 1], &end, 10);
                if (end == argv[i + 1] || *end != '\0' || n < 1 || n > 8) {
                    printf("Invalid input for -denoise! (1..8 iterations)\n");
                    displayHelp = true;
                } else params.m_denoise = (unsigned int)n;
                i += 2;
            } else ++i;
            continue;
        }
        if (strcmp(argv[i], "-denoise_guide") == 0) {
            if (i + 1 < argc && strcmp(argv[i + 1], "adaptive") == 0) params.m_denoiseAdaptive = true;
            else { printf("Invalid input for -denoise_guide!\n"); displayHelp = true; }
            i += 2;
            continue;
        }
        if (strcmp(argv[i], "-despike") == 0) { params.m_despike = true; ++i; continue; }
        if (strcmp(argv[i], "-upsample") == 0) {
            char* end = nullptr;
            const long k = i + 1 < argc ? strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || k < 2 || k > 4) {
                printf("Invalid input for -upsample! (a factor of 2..4)\n");
                displayHelp = true;
            } else params.m_upsample = (unsigned int)k;
            i += 2;
            continue;
        }
        if (strcmp(argv[i], "-upsample_aa") == 0) {
            char* end = nullptr;
            const long s = i + 1 < argc ? strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 >= argc || end == argv[i + 1] || *end != '\0' || s < 2 || s > 4) {
                printf("Invalid input for -upsample_aa! (a factor of 2..4)\n");
                displayHelp = true;
            } else params.m_upsampleAa = (unsigned int)s;
            i += 2;
            continue;
        }
        if (strcmp(argv[i], "-minspp") == 0) { uintArg(i, "-minspp", params.m_minSpp); i += 2; continue; }
        printf("Can't parse argument: %s\n", argv[i]);
        displayHelp = true;
        break;
    }
    if (params.m_denoiseAdaptive && !(params.m_adaptive >= 0.0f && params.m_denoise)) {
        printf("Invalid input for -denoise_guide! (adaptive needs both -adaptive and -denoise)\n");
        displayHelp = true;
    }
    if (params.m_despike && params.m_denoiseAdaptive) {
        printf("Invalid input for -despike! (not with -denoise_guide adaptive)\n");
        displayHelp = true;
    }
    if (params.m_upsample && params.m_denoiseAdaptive) {
        printf("Invalid input for -upsample! (not with -denoise_guide adaptive)\n");
        displayHelp = true;
    }
    if (params.m_upsampleAa && !params.m_upsample) {
        printf("Invalid input for -upsample_aa! (needs -upsample K)\n");
        displayHelp = true;
    }
    // (`pathtracer -help` alone lists the options: the lone argument is not an input file)
    const bool helpOnly = argc == 2 && strcmp(argv[1], helpOption) == 0;
    if (helpOnly) displayHelp = true;
    else if (i < argc && argc > 1) params.m_inputFilepath = argv[argc - 1];
    else {
        printf("Missing input file argument!\n");
        displayHelp = true;
    }
    if (displayHelp) {
        printf("USAGE: pathtracer [options] <input file>\n\n");
        printf("Options:\n");
        printf("%-30s Display available options\n", helpOption);
        printf("%-30s Set width of output image\n", widthOption);
        printf("%-30s Set height of output image\n", heightOption);
        printf("%-30s Set number of samples per pixel\n", sppOption);
        printf("%-30s Shows a window and displays progressive rendering results (not supported)\n", windowOption);
        printf("%-30s Enables camera controls (not supported)\n", controlsOption);
        printf("%-30s Set filepath of output image\n", outputOption);
        printf("%-30s Save image as HDR instead of PNG\n", outputHdrOption);
        printf("%-30s Render on N GPUs (row bands interleaved, RCCL gather)\n", "-gpus");
        printf("%-30s Samples per render() call (default 8)\n", "-chunk");
        printf("%-30s One kernel launch per render() call (default: all calls in one launch)\n", "-call_loop");
        printf("%-30s Adaptive sampling to this relative noise tolerance; -spp is the budget\n", "-adaptive");
        printf("%-30s Samples every pixel gets with -adaptive (default two calls)\n", "-minspp");
        printf("%-30s Denoise before writing: a-trous filter guided by first-hit features, N = 1..8 iterations (default 5)\n",
               "-denoise [N]");
        printf("%-30s With -adaptive and -denoise: guide the filter by the adaptive render's own per-pixel variance\n",
               "-denoise_guide adaptive");
        printf("%-30s Clamp fireflies before writing (and before -denoise): same-surface neighbourhood limit\n", "-despike");
        printf("%-30s Trace at 1/K of the width and height, K = 2..4, and reconstruct the image from full-size features\n",
               "-upsample K");
        printf("%-30s With -upsample: antialias the reconstruction with S x S first-hit samples per pixel, S = 2..4\n",
               "-upsample_aa S");
        return false;
    }
    params.m_enableControls = params.m_enableControls && params.m_showWindow;
    return true;
}

int main(int argc, char* argv[])
{
    Params params;
    int gpus = 1;
    if (!processArgs(argc, argv, params, gpus)) return EXIT_SUCCESS;

    printf("Beginning rendering in configuration:\n");
    printf("Width: %d\n", (int)params.m_width);
    printf("Height: %d\n", (int)params.m_height);
    printf("Samples per Pixel: %d\n", (int)params.m_spp);
    printf("Window: %d\n", (int)params.m_showWindow);
    printf("Controls: %d\n", (int)params.m_enableControls);
    printf("Output HDR: %d\n", (int)params.m_outputHdr);
    printf("Output Filepath: %s\n", params.m_outputFilepath ? params.m_outputFilepath : "");
    printf("Input Filepath: %s\n", params.m_inputFilepath);
    if (params.m_showWindow) {
        printf("Windowed mode is not supported by this build; rendering headless.\n");
        params.m_showWindow = false;
    }

    int available = 0;
    pt_device_count(&available);
    if (available < 1) {
        printf("No GPU found.\n");
        return EXIT_FAILURE;
    }
    gpus = std::max(1, std::min(gpus, available));
    const bool adaptive = params.m_adaptive >= 0.0f;
    if (params.m_denoise && gpus > 1) {
        printf("-denoise renders on one GPU; ignoring -gpus.\n");
        gpus = 1;
    }
    if (params.m_despike && gpus > 1) {
        printf("-despike renders on one GPU; ignoring -gpus.\n");
        gpus = 1;
    }
    if (params.m_upsample && gpus > 1) {
        printf("-upsample renders on one GPU; ignoring -gpus.\n");
        gpus = 1;
    }
    if (adaptive && gpus > 1) {
        printf("-adaptive renders on one GPU; ignoring -gpus.\n");
        gpus = 1;
    }
    // main.cpp:263 constructs one Pathtracer on device 0; -gpus N spans N devices with the same
    // interface (row bands over the devices, RCCL gather to device 0 when the image is read)
    // -upsample K: `pathtracer` is the low-resolution one, which everything up to the filters runs on, and `full` the
    // one of the image's size, which only takes features and reconstructs (the camera is the image's: its aspect)
    std::unique_ptr<Pathtracer> pathtracer, full;
    const uint32_t K = params.m_upsample;
    if (K) {
        pathtracer.reset(new Pathtracer((params.m_width + K - 1) / K, (params.m_height + K - 1) / K));
        full.reset(new Pathtracer(params.m_width, params.m_height));
        loadScene(*full, params);
    } else if (gpus == 1) {
        pathtracer.reset(new Pathtracer(params.m_width, params.m_height));
    } else {
        std::vector<int> devices(gpus);
        for (int g = 0; g < gpus; ++g) devices[g] = g;
        pathtracer.reset(new Pathtracer(params.m_width, params.m_height, devices));
    }
    Camera camera = loadScene(*pathtracer, params);

    // headless loop (main.cpp:269-288)
    const uint32_t chunk = params.m_chunk;
    float totalGpuTime = 0.0f;
    if (adaptive) {
        const uint32_t maxCalls = std::max(2u, params.m_spp / chunk);
        const uint32_t minCalls = params.m_minSpp ? std::min(maxCalls, std::max(2u, (params.m_minSpp + chunk - 1) / chunk)) : 2u;
        const Pathtracer::AdaptiveResult res = pathtracer->renderAdaptive(camera, chunk, minCalls, maxCalls, params.m_adaptive);
        totalGpuTime = res.gpuMs;
        printf("Adaptive sampling: tolerance %g, %u..%u calls of %u samples, %u launches\n", params.m_adaptive, minCalls,
               maxCalls, chunk, res.rounds);
        printf("Finished accumulating %f samples per pixel on average (budget %d) in %f ms GPU time\n",
               (double)res.samples / ((double)params.m_width * params.m_height), (int)(maxCalls * chunk), totalGpuTime);
    } else if (params.m_singleLaunch && params.m_spp > 0) {
        const uint32_t full = params.m_spp / chunk, rest = params.m_spp % chunk;
        if (full) { pathtracer->renderChunks(camera, chunk, full, true); totalGpuTime += pathtracer->getTiming(); }
        if (rest) { pathtracer->renderChunks(camera, rest, 1, full == 0); totalGpuTime += pathtracer->getTiming(); }
        // the loop's progress lines (main.cpp:283-286), so the output reads as the reference's
        for (uint32_t i = 0; i < params.m_spp; i += chunk)
            if (i % (chunk * 4) == 0) printf("Accumulated %d samples\n", (int)i);
    } else {
        for (uint32_t i = 0; i < params.m_spp; i += chunk) {
            const uint32_t spp = std::min(i + chunk, params.m_spp) - i;
            pathtracer->render(camera, spp, i == 0);
            totalGpuTime += pathtracer->getTiming();
            if (i % (chunk * 4) == 0) printf("Accumulated %d samples\n", (int)i);
        }
    }
    if (!adaptive) printf("Finished accumulating %d samples in %f ms GPU time\n", (int)params.m_spp, totalGpuTime);

    if (params.m_despike) {
        pathtracer->renderFeatures(camera);
        pathtracer->despike();
        printf("Despiked: %u pixels clamped\n", pathtracer->despikeCount());
    }
    if (params.m_denoise && params.m_denoiseAdaptive) {
        Pathtracer::VarianceDenoiseOptions options;
        options.iterations = params.m_denoise;
        options.sigmaL = PT_ADENOISE_DEFAULT_SIGMA_L;
        pathtracer->renderFeatures(camera);
        pathtracer->denoiseAdaptive(Pathtracer::AdaptiveVarianceOptions(), options);
        printf("Denoised: %u a-trous iterations, guided by the adaptive render's variance\n", options.iterations);
    } else if (params.m_denoise) {
        Pathtracer::DenoiseOptions options;
        options.iterations = params.m_denoise;
        if (!params.m_despike) pathtracer->renderFeatures(camera);     // (a features call would end the despiked image)
        const float sigma = pathtracer->denoise(options);
        printf("Denoised: %u a-trous iterations, colour sigma %g\n", options.iterations, sigma);
    }

    if (K) {
        if (!params.m_despike && !params.m_denoise) pathtracer->renderFeatures(camera);
        const uint32_t S = params.m_upsampleAa;
        if (S) {          // the planes of an S-times frame of the same camera; `full` then takes no features of its own
            Pathtracer super(params.m_width * S, params.m_height * S);
            loadScene(super, params);
            super.renderFeatures(camera);
            full->upsample(*pathtracer, super);
        } else {
            full->renderFeatures(camera);
            full->upsample(*pathtracer);
        }
        uint32_t counts[2] = {0, 0};
        full->upsampleCounts(counts);
        if (S) printf("Antialiased: %u x %u first-hit samples per pixel\n", S, S);
        // (with -upsample_aa the counts are of first-hit samples, up to S * S per pixel)
        printf(S ? "Upsampled: %u x %u from %u x %u, %u samples from the wider ring, %u from the nearest pixel\n"
                 : "Upsampled: %u x %u from %u x %u, %u pixels from the wider ring, %u from the nearest pixel\n",
               params.m_width, params.m_height, (params.m_width + K - 1) / K, (params.m_height + K - 1) / K, counts[0], counts[1]);
        pathtracer = std::move(full);
    }

    if (params.m_outputFilepath) {
        printf("Writing result to %s\n", params.m_outputFilepath);
        const uint32_t W = params.m_width, H = params.m_height;
        const bool ok = params.m_outputHdr
                            ? ptamd::writeHDR(params.m_outputFilepath, W, H, pathtracer->getHDRImageData(), true)
                            : ptamd::writePNG(params.m_outputFilepath, W, H, (const uint8_t*)pathtracer->getImageData(), true);
        if (!ok) printf("Failed to write file!\n");
        if (gpus > 1) printf("Gathered %d GPU tiles over RCCL in %f ms\n", gpus, pathtracer->lastGatherMs());
    }
    return EXIT_SUCCESS;
}
