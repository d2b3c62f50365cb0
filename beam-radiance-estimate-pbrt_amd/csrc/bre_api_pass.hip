// bre_api_pass.hip — the photon and camera passes behind the C ABI: bre_trace_photons, bre_camera_pass,
// bre_get_segments and the bre_render* loops over them.  The scene they trace is bre_api_scene.hip's.
#include <algorithm>
#include <cstring>
#include <vector>

#include "bre_ctx.h"

using namespace bre;

namespace bre {

bre_status check_params(bre_ctx *c, const bre_render_params *rp) {
    if (!rp) return fail(c, BRE_ERR_INVALID_ARG, "bre_render: null params");
    if (rp->width < 1 || rp->height < 1 || rp->start_iteration < 0 ||
        rp->end_iteration < rp->start_iteration || rp->max_depth < 1 || rp->max_depth > BRE_MAX_DEPTH)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_render: bad parameters");
    return BRE_OK;
}

// photonbeam.cpp:564: write at the last iteration and whenever (iter + 1) % writeFrequency == 0,
// negative frequencies included (-k fires every k iterations); the reference's default
// 1 << 31 wraps to INT32_MIN and never fires, and 0 (a division by zero there) means never
bool image_due(int32_t it, int32_t end_iteration, int32_t write_frequency) {
    const bool periodic = write_frequency != 0 && write_frequency != INT32_MIN && (it + 1) % write_frequency == 0;
    return it + 1 == end_iteration || periodic;
}

}  // namespace bre

extern "C" {

bre_status bre_trace_photons(bre_ctx *c, const bre_scene *scene, int64_t n_photons, int32_t iteration,
                             int32_t max_depth, float beam_radius, int64_t *n_beams) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (n_beams) *n_beams = 0;
    if (!scene) return fail(c, BRE_ERR_INVALID_ARG, "bre_trace_photons: null scene");
    if (n_photons < 0 || iteration < 0) return fail(c, BRE_ERR_INVALID_ARG, "bre_trace_photons: negative count");
    if (max_depth < 1 || max_depth > BRE_MAX_DEPTH)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_trace_photons: max_depth must be in [1, %d]", BRE_MAX_DEPTH);
    BRE_TRY(check_scene(c, scene, "bre_trace_photons"));
    BRE_TRY(check_medium(c, scene, "bre_trace_photons"));
    BRE_TRY(set_device(c));
    PassStream pass(c);
    // an earlier asynchronous gather's device errors are reported before this call changes anything
    BRE_TRY(check_flags(c));
    BRE_TRY(upload_scene(c, scene));
    const size_t N = (size_t)n_photons;
    int32_t *counts = nullptr;
    int64_t *offsets = nullptr;
    HIPCHK(c, c->ph_counts.get(N + 1, &counts));
    HIPCHK(c, c->ph_offsets.get(N + 1, &offsets));
    HIPCHK(c, c->ph_tmp.ensure(count_scan_temp_bytes(n_photons) + 16));
    const uint64_t seq0 = (uint64_t)iteration * (uint64_t)n_photons + 1;
    const DevScene *ds = c->dev.record.as<DevScene>();
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    const int sdepth = c->dev.head.stack_depth;
    const bool media = !c->held.media.empty();
    // single-trace form (bre_photon.hip): `cap` beam slots per photon, scratch at most 2.5 GB (62 slots at
    // 1M photons: the re-trace of the photons with more beams than slots is the form's tail, 1.65 ms
    // with 16 slots vs 1.41 with 64 at C2, profiles/r4/run36); below 4 slots, or with option 116 = 0,
    // the two-trace form
    int cap = c->photon_single ? (int)std::min<int64_t>(64, ((int64_t)5 << 29) / (40 * std::max<int64_t>(n_photons, 1))) : 0;
    if (cap < 4) cap = 0;
    if (c->photon_single >= 2) cap = c->photon_single;  // tests: a forced slot count (overflow paths)
    const int tier = c->held.mixed ? 3 : (c->held.lobed ? 2 : (c->held.glossy ? 1 : 0));
    if (c->held.glossy) {
        // the glossy photon kernels keep max_depth suspended frames a thread in LDS: refused here, by name
        if (c->lds_per_block == 0)
            HIPCHK(c, hipDeviceGetAttribute(&c->lds_per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
        const size_t need = photon_lds_bytes(sdepth, max_depth, true);
        if (need > (size_t)c->lds_per_block)
            return fail(c, BRE_ERR_INVALID_ARG, "bre_trace_photons: maxdepth %d with %s "
                        "materials needs %lld bytes of LDS per block for the photon kernels' suspended frames; the "
                        "device has %d", max_depth,
                        c->held.mixed ? "mix" : c->held.lobed ? "rough glass / uber / translucent / substrate"
                                                               : "plastic / metal / matte-sigma",
                        (long long)need, c->lds_per_block);
    }
    BeamArrays &slots = c->ph_s, &in = c->in;
    if (cap > 0) {
        HIPCHK(c, slots.ensure(N * (size_t)cap));
        HIPCHK(c, launch_photons(ds, sdepth, n_photons, seq0, max_depth, beam_radius, counts, nullptr, slots.out(), 2, cap,
                                 media, tier, c->stream));
    } else {
        HIPCHK(c, launch_photons(ds, sdepth, n_photons, seq0, max_depth, beam_radius, counts, nullptr, BeamOut{}, 0, 0,
                                 media, tier, c->stream));
    }
    HIPCHK(c, launch_count_scan(c->ph_tmp.ptr, c->ph_tmp.cap, counts, offsets, n_photons, c->stream,
                                c->slot_passes != 0));
    int64_t total = 0;
    BRE_TRY(read_small(c, {{&total, offsets + n_photons, sizeof(total)}}));
    if (total > 0) {
        HIPCHK(c, in.ensure((size_t)total));
        if (cap > 0)
            HIPCHK(c, launch_photon_slots(n_photons, cap, counts, offsets, slots.view(), in.out(), c->stream));
        // every photon (two-trace form), or only those with more beams than slots
        HIPCHK(c, launch_photons(ds, sdepth, n_photons, seq0, max_depth, beam_radius, counts, offsets, in.out(), 1, cap,
                                 media, tier, c->stream));
    }
    float photon_ms = 0.f;
    if (c->timing) {
        HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
        HIPCHK(c, hipEventSynchronize(c->ev[1]));
        HIPCHK(c, hipEventElapsedTime(&photon_ms, c->ev[0], c->ev[1]));
    }
    c->beams_kept = false;
    BRE_TRY(build(c, total, in.view()));
    c->beams_kept = true;
    c->stats.n_photons = n_photons;
    c->stats.photon_ms = photon_ms;
    if (n_beams) *n_beams = total;
    return check_flags(c);
}

bre_status bre_camera_pass(bre_ctx *c, const bre_scene *scene, int32_t width, int32_t height, int32_t iteration,
                           int32_t max_depth, int32_t render_surfaces, int32_t render_media, float *d_surface,
                           int64_t *n_segments) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (n_segments) *n_segments = 0;
    BRE_TRY(check_scene(c, scene, "bre_camera_pass"));
    if (width < 1 || height < 1 || (int64_t)width * height > (int64_t)INT32_MAX / BRE_MAX_DEPTH || iteration < 0)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_camera_pass: bad film size or iteration");
    if (max_depth < 1 || max_depth > BRE_MAX_DEPTH)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_camera_pass: max_depth must be in [1, %d]", BRE_MAX_DEPTH);
    BRE_TRY(check_medium(c, scene, "bre_camera_pass"));
    BRE_TRY(set_device(c));
    PassStream pass(c);
    BRE_TRY(check_flags(c));  // an earlier gather's device errors, before this pass changes anything
    // scene + camera/Halton tables (rebuilt when the scene or film changes)
    BRE_TRY(upload_scene(c, scene));
    if (c->cam_w != width || c->cam_h != height || memcmp(&c->cam_scene, scene, sizeof(bre_scene)) != 0) {
        DevCamera cam;
        std::vector<uint16_t> perms;
        prepare_camera(scene, width, height, &cam, &perms);
        HIPCHK(c, c->cam_dev.ensure(sizeof(DevCamera)));
        HIPCHK(c, c->cam_perms.ensure(perms.size() * sizeof(uint16_t)));
        HIPCHK(c, hipMemcpyAsync(c->cam_dev.ptr, &cam, sizeof(cam), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->cam_perms.ptr, perms.data(), perms.size() * sizeof(uint16_t),
                                 hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // host vectors go out of scope
        c->cam_w = width;
        c->cam_h = height;
        memcpy(&c->cam_scene, scene, sizeof(bre_scene));
    }
    const int64_t nslots = camera_slots(width, height);
    // the slot planes: a segment's plane is its ordinal along the path, which passes the depth only where the
    // path can cross an interface triangle; then BRE_OPT_SEGMENT_BUDGET more planes
    const bool media = !c->held.media.empty();
    const int planes = max_depth + (media && c->held.has_interface ? c->seg_budget : 0);
    if (nslots * planes > (int64_t)INT32_MAX)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_camera_pass: the film is too large for %d segment planes", planes);
    const size_t S = (size_t)(nslots * planes);
    int32_t *valid = nullptr, *depth = nullptr;
    int64_t *offs = nullptr;
    unsigned int *cam_flags = nullptr;
    HIPCHK(c, c->cs.ensure(S));
    HIPCHK(c, c->cs_valid.get(S, &valid));
    HIPCHK(c, c->cam_offs.get(S + 1, &offs));
    HIPCHK(c, c->cam_tmp.ensure(camera_scan_temp_bytes((int64_t)S) + 16));
    HIPCHK(c, c->cam_flags.get(1, &cam_flags));
    HIPCHK(c, fill_words(c, cam_flags, sizeof(unsigned int)));
    CamSlots cs{c->cs.out(), valid};
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    // the kernels with the general BSDF are also the ones that shade under a distant light: the others, whose waves
    // run inside another context's gather at 80 VGPRs, keep the code and the resources they had
    bool wide = c->held.glossy;
    for (const bre_light &l : c->held.lights) wide = wide || l.type == BRE_LIGHT_DISTANT;
    const int tier = c->held.mixed ? 3 : (c->held.lobed ? 2 : (wide ? 1 : 0));
    HIPCHK(c, launch_camera(c->dev.record.as<DevScene>(), c->dev.head.stack_depth, c->cam_dev.as<DevCamera>(),
                            c->cam_perms.as<uint16_t>(),
                            width, height, iteration, max_depth, render_surfaces, render_media, cs, d_surface,
                            cam_flags, c->shard_rank, c->shard_count,
                            c->shard_mode != 0 ? 0 : c->shard_block, c->film_classes, planes, media, tier, c->stream));
    // exclusive scan of the slots' valid flags into cam_offs: total = offs[S-1] + valid[S-1]
    HIPCHK(c, launch_camera_scan(c->cam_tmp.ptr, c->cam_tmp.cap, cs, nslots, planes, offs, c->stream,
                                 c->slot_passes != 0));
    int64_t last_off = 0;
    int32_t last_valid = 0;
    unsigned int flags = 0;
    BRE_TRY(read_small(c, {{&last_off, offs + (S - 1), sizeof(int64_t)},
                           {&last_valid, valid + (S - 1), sizeof(int32_t)},
                           {&flags, cam_flags, sizeof(flags)}}));
    if (flags & kCamFlagBudget) {
        c->cam_nseg = 0;
        return fail(c, BRE_ERR_STATE, "bre_camera_pass: a camera path crossed more medium interfaces than "
                    "BRE_OPT_SEGMENT_BUDGET (%d) allows beyond maxdepth: no segments are kept", c->seg_budget);
    }
    const int64_t n = last_off + last_valid;
    const size_t N = (size_t)(n > 0 ? n : 1);
    HIPCHK(c, c->seg.ensure(N));
    HIPCHK(c, c->seg_depth.get(N, &depth));
    HIPCHK(c, launch_camera_compact(cs, nslots, planes, offs, c->seg.out(), depth, c->stream));
    float ms = 0.f;
    if (c->timing) {
        HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
        HIPCHK(c, hipEventSynchronize(c->ev[1]));
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    }
    c->cam_nseg = n;
    c->cam_npix = (int64_t)width * height;
    c->stats.n_camera_segments = n;
    c->stats.camera_ms = ms;
    if (n_segments) *n_segments = n;
    return check_flags(c);
}

bre_status bre_get_segments(bre_ctx *c, int64_t capacity, float *o, float *p, float *d, float *tmax, int32_t *pixel,
                            int32_t *depth, int64_t *n_segments) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (capacity < 0) return fail(c, BRE_ERR_INVALID_ARG, "bre_get_segments: negative capacity");
    if (n_segments) *n_segments = c->cam_nseg;
    const int64_t k = capacity < c->cam_nseg ? capacity : c->cam_nseg;
    if (k <= 0) return BRE_OK;
    if (!o || !p || !d || !tmax || !pixel || !depth)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_get_segments: null array");
    BRE_TRY(set_device(c));
    const size_t K = (size_t)k;
    HIPCHK(c, c->seg.download(K, o, p, d, tmax, pixel, c->stream));
    HIPCHK(c, hipMemcpyAsync(depth, c->seg_depth.ptr, K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    return check_flags(c);
}

bre_status bre_render_iteration(bre_ctx *c, const bre_scene *scene, const bre_render_params *rp, int32_t iteration,
                                float *d_ld) {
    if (!c) return BRE_ERR_INVALID_ARG;
    BRE_TRY(check_params(c, rp));
    if (!d_ld) return fail(c, BRE_ERR_INVALID_ARG, "bre_render_iteration: null Ld buffer");
    const float R = bre_beam_radius_at(rp->initial_radius, rp->alpha, iteration);
    // photonsperiteration <= 0 means the film's pixel count (photonbeam.h:37-39, the -1 default)
    const int64_t photons =
        rp->photons_per_iteration > 0 ? rp->photons_per_iteration : (int64_t)rp->width * rp->height;
    BRE_TRY(bre_trace_photons(c, scene, photons, iteration, rp->max_depth, R, nullptr));
    BRE_TRY(bre_camera_pass(c, scene, rp->width, rp->height, iteration, rp->max_depth, rp->render_surfaces,
                            rp->render_media, d_ld, nullptr));
    if (rp->render_media) return bre_gather_camera(c, R, d_ld);
    return BRE_OK;
}

bre_status bre_render_progressive(bre_ctx *c, const bre_scene *scene, const bre_render_params *rp,
                                  int32_t write_frequency, bre_image_fn on_image, void *user) {
    if (!c) return BRE_ERR_INVALID_ARG;
    bre_status st = check_params(c, rp);
    if (st != BRE_OK) return st;
    if (c->film_classes > 1) return fail(c, BRE_ERR_STATE, "bre_render*: BRE_OPT_FILM_CLASSES is for caller device films");
    BRE_TRY(set_device(c));
    const int64_t npix = (int64_t)rp->width * rp->height;
    float *ld = nullptr;
    HIPCHK(c, hipMalloc(&ld, (size_t)npix * 3 * sizeof(float)));
    if (hipMemsetAsync(ld, 0, (size_t)npix * 3 * sizeof(float), c->stream) != hipSuccess)
        st = fail(c, BRE_ERR_HIP, "bre_render: memset failed");
    std::vector<float> h, img;
    for (int it = rp->start_iteration; st == BRE_OK && it < rp->end_iteration; ++it) {
        st = bre_render_iteration(c, scene, rp, it, ld);
        if (st != BRE_OK) break;
        if (!image_due(it, rp->end_iteration, write_frequency) || !on_image) continue;
        h.resize((size_t)npix * 3);
        img.resize(h.size());
        if (hipMemcpyAsync(h.data(), ld, h.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) {
            st = fail(c, BRE_ERR_HIP, "bre_render: copy-back failed");
            break;
        }
        st = bre_resolve_image(npix, h.data(), it, img.data());  // L = Ld / (iter + 1), :578
        if (st == BRE_OK && on_image(it, img.data(), user) != 0)
            st = fail(c, BRE_ERR_STATE, "bre_render: image callback stopped the render after iteration %d", it);
    }
    const bre_status fst = check_flags(c);  // the last iteration's gather
    if (st == BRE_OK) st = fst;
    (void)hipFree(ld);
    return st;
}

bre_status bre_render(bre_ctx *c, const bre_scene *scene, const bre_render_params *rp, float *image) {
    if (!c) return BRE_ERR_INVALID_ARG;
    BRE_TRY(check_params(c, rp));
    if (c->film_classes > 1) return fail(c, BRE_ERR_STATE, "bre_render: BRE_OPT_FILM_CLASSES is for caller device films");
    if (!image) return fail(c, BRE_ERR_INVALID_ARG, "bre_render: null image");
    FinalImage f{image, (size_t)rp->width * rp->height * 3};
    if (rp->end_iteration == rp->start_iteration) {
        memset(image, 0, f.n * sizeof(float));
        return BRE_OK;
    }
    // only the last iteration's image is kept (write_frequency 0 = at the end only)
    return bre_render_progressive(c, scene, rp, 0, keep_final_image, &f);
}

}  // extern "C"
