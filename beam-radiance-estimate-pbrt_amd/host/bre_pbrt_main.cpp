// bre_pbrt_main.cpp — `bre_pbrt scene.pbrt`: the pbrt command line for scenes whose Integrator
// is "photonbeam" (src/main/pbrt.cpp: parse, WorldEnd -> Render, film written by the integrator),
// with the render on an MI355X.  Options: --quick, --outfile FILE, --media (media bounded by surfaces:
// MediumInterface on shapes and lights, Material "none" boundaries), --lights (LightSource "distant" and
// "point", two-sided area lights), --device N, --devices A,B,... (the
// render split over several GPUs, one context per entry; a repeated ordinal is allowed); pbrt's
// --nthreads is accepted and ignored.  Without --devices, a BRE_DEVICES environment value naming more
// than one device selects them.  Exit status 0 on success.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bre_pbrt.h"

static const char *kUsage =
    "usage: bre_pbrt [--quick] [--media] [--lights] [--materials] [--outfile file.pfm] [--device n | --devices a,b,...] scene.pbrt\n";

// "0,1,2,3" -> ordinals; empty when the text is not a comma-separated list of non-negative integers
static std::vector<int32_t> ParseDevices(const char *text) {
    std::vector<int32_t> out;
    for (const char *q = text ? text : ""; *q;) {
        char *end = nullptr;
        const long v = std::strtol(q, &end, 10);
        if (end == q || v < 0 || (*end != ',' && *end != '\0')) return {};
        out.push_back((int32_t)v);
        q = *end == ',' ? end + 1 : end;
    }
    return out;
}

int main(int argc, char **argv) {
    const char *scene = nullptr, *outfile = nullptr;
    int quick = 0, device = 0, flags = 0;
    std::vector<int32_t> devices;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--quick")) quick = 1;
        else if (!strcmp(argv[i], "--media")) flags |= BRE_PBRT_MEDIA;
        else if (!strcmp(argv[i], "--lights")) flags |= BRE_PBRT_LIGHTS;
        else if (!strcmp(argv[i], "--materials")) flags |= BRE_PBRT_MATERIALS;
        else if (!strcmp(argv[i], "--outfile") && i + 1 < argc) outfile = argv[++i];
        else if (!strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--devices") && i + 1 < argc) {
            devices = ParseDevices(argv[++i]);
            if (devices.empty()) {
                fputs(kUsage, stderr);
                return 2;
            }
        } else if (!strcmp(argv[i], "--nthreads") && i + 1 < argc) ++i;
        else if (argv[i][0] == '-') {
            fputs(kUsage, stderr);
            return 2;
        } else scene = argv[i];
    }
    if (!scene) {
        fputs(kUsage, stderr);
        return 2;
    }
    if (devices.empty()) {
        // the mirror's one-process multi-GPU switch (DevicesFromEnv); one device or none: --device as before
        const std::vector<int32_t> env = ParseDevices(std::getenv("BRE_DEVICES"));
        if (env.size() > 1) devices = env;
    }
    bre_pbrt *p = nullptr;
    const bre_status st = bre_pbrt_parse_file_ex(scene, flags, &p);
    int ne = 0, nw = 0;
    fputs(bre_pbrt_messages(p, &ne, &nw), stderr);
    if (st != BRE_OK) {
        bre_pbrt_free(p);
        return 1;
    }
    int32_t w = 0, h = 0;
    char fn[1024];
    bre_pbrt_get_film(p, &w, &h, nullptr, fn, sizeof(fn));
    const auto t0 = std::chrono::steady_clock::now();
    const bre_status rs = devices.empty()
                              ? bre_pbrt_render(p, device, quick, outfile, 1, nullptr)
                              : bre_pbrt_render_devices(p, devices.data(), (int32_t)devices.size(), quick, outfile, 1,
                                                        nullptr);
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    bre_pbrt_free(p);
    if (rs != BRE_OK) {
        fprintf(stderr, "Error: render failed (status %d)\n", (int)rs);
        return 1;
    }
    printf("rendered %dx%d in %.3f s -> %s\n", w, h, s, outfile ? outfile : fn);
    return 0;
}
