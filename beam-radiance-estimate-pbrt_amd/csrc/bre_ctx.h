// bre_ctx.h — the context behind the C ABI (include/bre.h), shared by the bre_api*.hip units: device
// buffers that own their memory, the context struct, the status macros and the few internal functions
// that cross units.  Internal: nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/bre.h"
#include "bre_device.h"
#include "bre_trace.h"

#ifndef BRE_KERNEL_READBACK
#define BRE_KERNEL_READBACK 1
#endif
// default of internal option 124: the specialised tile kernel's register budget, 7 waves per SIMD (DESIGN.md
// section 24; a build with 6 serves A/B runs through bench.py, which has no flag for the option)
#ifndef BRE_TILE_BUDGET
#define BRE_TILE_BUDGET 7
#endif
static_assert(BRE_TILE_BUDGET == 6 || BRE_TILE_BUDGET == 7, "BRE_TILE_BUDGET must be 6 or 7");

namespace bre {

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// A device buffer that grows on demand and frees itself.  Growth frees first, then allocates a quarter
// more than asked: the contents do not survive it.
struct DevMem : NoCopy {
    void *ptr = nullptr;
    size_t cap = 0;
    ~DevMem() { if (ptr) (void)hipFree(ptr); }
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&ptr, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    // room for `count` elements of T, and the typed pointer
    template <typename T>
    hipError_t get(size_t count, T **out) {
        const hipError_t e = ensure(count * sizeof(T));
        *out = as<T>();
        return e;
    }
    template <typename T>
    T *as() const { return static_cast<T *>(ptr); }
};

// A DevMem of T, for the array groups below
template <typename T>
struct DevArr : DevMem {
    hipError_t reserve(size_t n) { return ensure(n * sizeof(T)); }
    operator T *() const { return as<T>(); }
};

// Beams as the ABI passes them: start, end and power hold 3 floats per beam, radius 1
struct BeamArrays {
    DevArr<float> start, end, radius, power;
    hipError_t ensure(size_t n) {
        hipError_t e = start.reserve(3 * n);
        if (e == hipSuccess) e = end.reserve(3 * n);
        if (e == hipSuccess) e = radius.reserve(n);
        if (e == hipSuccess) e = power.reserve(3 * n);
        return e;
    }
    // the first n beams from / to host arrays, queued on `s`
    hipError_t upload(size_t n, const float *hs, const float *he, const float *hr, const float *hp, hipStream_t s) {
        hipError_t e = hipMemcpyAsync(start, hs, n * 3 * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(end, he, n * 3 * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(radius, hr, n * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(power, hp, n * 3 * sizeof(float), hipMemcpyHostToDevice, s);
        return e;
    }
    hipError_t download(size_t n, float *hs, float *he, float *hr, float *hp, hipStream_t s) const {
        hipError_t e = hipMemcpyAsync(hs, start, n * 3 * sizeof(float), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(he, end, n * 3 * sizeof(float), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(hr, radius, n * sizeof(float), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(hp, power, n * 3 * sizeof(float), hipMemcpyDeviceToHost, s);
        return e;
    }
    BeamView view() const { return {start, end, radius, power}; }
    BeamOut out() const { return {start, end, radius, power}; }
};

// Camera segments: o, p and d hold 3 floats per segment, t (tmax) 1, pix the pixel index
struct SegArrays {
    DevArr<float> o, p, d, t;
    DevArr<int32_t> pix;
    hipError_t ensure(size_t n, bool with_pix = true) {
        hipError_t e = o.reserve(3 * n);
        if (e == hipSuccess) e = p.reserve(3 * n);
        if (e == hipSuccess) e = d.reserve(3 * n);
        if (e == hipSuccess) e = t.reserve(n);
        if (e == hipSuccess && with_pix) e = pix.reserve(n);
        return e;
    }
    // the first n segments from / to host arrays, queued on `s`; a null hpix is skipped
    hipError_t upload(size_t n, const float *ho, const float *hp, const float *hd, const float *ht, const int32_t *hpix,
                      hipStream_t s) {
        hipError_t e = hipMemcpyAsync(o, ho, n * 3 * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(p, hp, n * 3 * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(d, hd, n * 3 * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(t, ht, n * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess && hpix) e = hipMemcpyAsync(pix, hpix, n * sizeof(int32_t), hipMemcpyHostToDevice, s);
        return e;
    }
    hipError_t download(size_t n, float *ho, float *hp, float *hd, float *ht, int32_t *hpix, hipStream_t s) const {
        hipError_t e = hipMemcpyAsync(ho, o, n * 3 * sizeof(float), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(hp, p, n * 3 * sizeof(float), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(hd, d, n * 3 * sizeof(float), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(ht, t, n * sizeof(float), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(hpix, pix, n * sizeof(int32_t), hipMemcpyDeviceToHost, s);
        return e;
    }
    SegView view() const { return {o, p, d, t, pix}; }
    SegOut out() const { return {o, p, d, t, pix}; }
};

// The double-buffered keys and values of a radix sort and its temporary storage
struct SortScratch {
    DevMem keys, keys_alt, tmp;
    DevArr<int32_t> vals, vals_alt;
    hipError_t reserve(size_t n, size_t key_bytes, size_t tmp_bytes) {
        hipError_t e = keys.ensure(n * key_bytes);
        if (e == hipSuccess) e = keys_alt.ensure(n * key_bytes);
        if (e == hipSuccess) e = vals.reserve(n);
        if (e == hipSuccess) e = vals_alt.reserve(n);
        if (e == hipSuccess) e = tmp.ensure(tmp_bytes);
        return e;
    }
};

// Owner of one HIP handle, released by Free.  Converts to the handle; `h` is assigned directly.
template <typename H, auto Free>
struct Owned : NoCopy {
    H h = nullptr;
    ~Owned() { if (h) (void)Free(h); }
    operator H() const { return h; }
};
using Event = Owned<hipEvent_t, hipEventDestroy>;
using PinnedWords = Owned<unsigned int *, hipHostFree>;
struct Stream : NoCopy {
    hipStream_t h = nullptr;
    bool owned = false;  // a caller's stream (bre_set_stream) is not destroyed
    ~Stream() { reset(); }
    void reset() {
        if (owned && h) {
            (void)hipStreamSynchronize(h);
            (void)hipStreamDestroy(h);
        }
        h = nullptr;
        owned = false;
    }
    operator hipStream_t() const { return h; }
};

// The scene state the sticky setters store on a context, beside the bre_scene every pass is given
struct SceneState {
    std::vector<bre_light> lights;   // bre_set_lights: the delta lights every pass adds to its scene
    // bre_set_materials / bre_set_materials_ex: the one table in its wide form (colours clamped) ...
    std::vector<bre_material_ex> mats;
    std::vector<int32_t> tri_mat;    // ... and each triangle's index into it (-1: its own matte kd)
    bool has_interface = false;      // ... one of which leads to a BRE_MATERIAL_INTERFACE entry
    bool glossy = false;             // the table holds a type >= BRE_MATERIAL_MATTE: the passes' glossy kernels
    bool lobed = false;              // ... a type >= BRE_MATERIAL_ROUGH_GLASS: the kernels with the N-lobe BSDF
    bool mixed = false;              // ... a BRE_MATERIAL_MIX: the tier-3 kernels over the wide lobe lists
    // bre_set_media: the table (grid_density pointing into media_grid), the triangles' (inside, outside) pairs
    // interleaved, the delta lights' media, the camera's; media_key: all of it as bytes, the grids for the pointers
    std::vector<bre_medium> media;
    std::vector<std::vector<float>> media_grid;
    std::vector<int32_t> tri_med, light_med;
    int cam_med = -1;
    std::vector<unsigned char> media_key;
};

// What upload_scene keeps on the device, and the host bytes it compares the next call's scene against
struct SceneDevice {
    // geometry: triangles, BVHAccel nodes + primitive order, scene.lights, the delta lights and the materials
    DevMem tris, nodes, prims, light_tri, light_func, light_cdf, dlights, mats, bsdfs, lobes, lobes_mx;
    DevScene head;                     // its fields of the record below
    uint64_t hash = 0;                 // hash of the uploaded triangles, lights and materials (0: none)
    // the uploaded triangles' bytes, the lights', the materials' and the map's: a hash match is confirmed by memcmp
    std::vector<unsigned char> bytes[4];
    DevMem md_table, md_pairs, md_light, md_dens;  // the media: table, pairs, lights' media, grids (upload_media)
    bool media_stale = false;                      // bre_set_media changed them since
    DevMem grid;                                   // the scene's own density grid,
    std::vector<unsigned char> grid_bytes;         // as last copied
    DevMem record;                                 // the DevScene the kernels read,
    std::vector<unsigned char> record_bytes;       // as last copied
};

}  // namespace bre

// Members are destroyed last to first: the buffers, then the pinned words, the events, and last the streams
// (bre_destroy has synchronised both by then).  The options are documented where they are set
// (bre_set_option, bre_api.hip).
struct bre_ctx {
    int device = 0;
    bre::Stream stream;   // the caller's work; the passes swap `h` for pstream's while they run (PassStream)
    bre::Stream pstream;  // the passes' own high-priority stream (option 117)
    bre::Event ev[4];     // timing: 0 / 1 around a build or pass, 2 / 3 around a gather
    bre::Event fork_ev, join_ev;  // PassStream
    bre::Event tile_ev;   // recorded after each tile-kernel launch (created on first use)
    bool tile_ev_valid = false;
    hipEvent_t user_ev[2] = {nullptr, nullptr};  // bre_set_gather_events: the caller's, not owned
    bre::PinnedWords flags_host;  // copy of DevCounters::flags (check_flags)
    bre::PinnedWords rb_host;     // words of read_small (kernel readback)
    std::string err;
    // options (bre.h), then the internal ones by number
    bool counters = false, timing = false, prefilter = true, sort_segments = true;
    int kernel = 0, leaf_size = 1, sqrt_mode = 0, split = 256, leaf2 = 64, chunk_len = 400, chunk_leaf = 1;
    int shard_rank = 0, shard_count = 1, shard_block = 1, shard_mode = 0, film_classes = 1;
    int stack_cap = 0, occupancy = 6, sort_key = 4, block_map = 3, tscan = -1;         // 101, 102, 105, 107, 108
    int64_t pktrec_nseg = 0;  // segments of the last tile launch: its packets' records are in `pktrec`
    int64_t partial_cap = (int64_t)4 << 30;                                            // 109, in bytes
    int beam_key = 2, margin = 1, tile_axis = 1, split_records = 0, film_compose = 1;  // 110 .. 114
    int photon_single = 1, pass_priority = 1, kernel_readback = BRE_KERNEL_READBACK;   // 116 .. 118
    int slot_passes = 1, coarse_keys = 0, stage_all = 0, tile_spec = 1;                // 119, 121, 122, 123
    int tile_budget = BRE_TILE_BUDGET;                                                 // 124
    // beam set
    int64_t nbeams = 0, nvalid = 0, nnodes = 0;
    bre::BeamSet bset;  // the built set's radius layout (BeamRec)
    int built_leaf_size = 1;
    int built_key_lo = 0;           // BuildBuffers::key_lo of the current build (bre_device_check kind 11)
    bool build_scratch_ok = false;  // sort.keys_alt / sort.vals_alt / leaf_parent still hold the current build's (kind 11)
    int roots_split = -1;           // split the roots buffer was computed for (-1: stale)
    bool nodes4_ok = false;         // nodes4 holds the 4-wide view of the current tree
    bool beams_kept = false;        // `in` holds the current beam set (bre_get_beams)
    bre::BeamArrays in;             // staging for host-pointer uploads, and the photon pass's beams
    bre::DevMem box, cent, cbounds, nvalid_buf, leaf_parent, visit, gbox;
    bre::SortScratch sort;  // the build's sort; reused by kernel 5's chunk index (gather_chunk)
    bre::DevMem recs, pow, nodes;
    // gather
    bre::SegArrays g;  // staging of the host-pointer API; g.pix only with a seg_pixel array
    bre::DevMem g_accum, g_seg_rgb, g_counts;  // each only when the caller passes that output
    bre::DevMem counters_buf, roots, roots_sh, roots_tmp, partial, pcnt, segrec, pktrec, tileax, segbox, nodes4;
    // kernel 5: capsule-chunk index, rebuilt per gather (bre_chunk.hip)
    bre::DevMem ch_bounds, ch_counts, ch_offsets, ch_range, ch_scan_tmp, ch_box, ch_cent, ch_slo, ch_shi, ch_par,
        ch_recs, ch_cpar, ch_nodes;
    int64_t n_chunks = 0;
    // coherence sort of the segments before the gather (bre_sort.hip)
    bre::DevMem ss_bounds;
    bre::SortScratch ss_sort;
    bre::SegArrays ss;
    bre::SegArrays sp;    // this packet shard's segments (contiguous)
    bre::DevMem sp_index;  // only with per-segment outputs
    // deterministic per-pixel compose; px_cls the film class per segment (BRE_OPT_FILM_CLASSES)
    bre::DevMem px_seg, px_cls;
    bre::SortScratch px_sort;
    // the scene model: what the setters stored, and what upload_scene keeps on the device (bre_api_scene.hip)
    bre::SceneState held;
    bre::SceneDevice dev;
    int seg_budget = 16;  // BRE_OPT_SEGMENT_BUDGET
    // photon pass
    bre::DevMem ph_counts, ph_offsets, ph_tmp;
    bre::BeamArrays ph_s;  // single-trace photon pass: per-photon beam slots
    // camera pass
    bre::DevMem cam_dev, cam_perms, cam_offs, cam_tmp, cam_flags;
    bre::SegArrays cs;  // one slot per pixel sample and depth
    bre::DevMem cs_valid;
    bre::SegArrays seg;  // the compacted segments
    bre::DevMem seg_depth;
    int64_t cam_nseg = 0;
    int64_t cam_npix = 0;
    int cam_w = -1, cam_h = -1;  // film the Halton / camera tables were prepared for
    bre_scene cam_scene;         // scene the camera tables were prepared for
    bre::DevMem chk_x, chk_aux, chk_y;  // bre_device_check staging
    int lds_per_block = 0;              // the device's LDS per workgroup, asked once (the glossy photon kernels' frames)
    bre_stats stats;
    // bre_set_gather_after: this context's tile kernels wait for `after`'s last one (after->tile_ev)
    bre_ctx *after = nullptr;
    std::vector<bre_ctx *> followers;  // contexts whose `after` is this one (unlinked in bre_destroy)
};

namespace bre {

// bre_api.hip
bre_status fail(bre_ctx *c, bre_status st, const char *fmt, ...);  // the message of bre_last_error; returns st
bre_status set_device(bre_ctx *c);
hipError_t fill_words(bre_ctx *c, void *p, size_t bytes);
struct HostSpan {
    void *host;
    const void *dev;
    size_t bytes;  // a multiple of 4, <= 64 words over all spans
};
bre_status read_small(bre_ctx *c, std::initializer_list<HostSpan> spans);
bre_status counters_block(bre_ctx *c, DevCounters **out);
bre_status check_flags(bre_ctx *c);
// bre_api_gather.hip: bre_gather; with film_stays the film starts at zero on the device (accum_rgb is only
// the "a film is wanted" flag), stays there as c->g_accum and is not copied back (bre_gather_sharded)
// (seg and out are host arrays here)
bre_status gather_host(bre_ctx *c, int64_t nseg, const SegView &seg, float R, int64_t npix, const GatherOut &out,
                       bool film_stays);
// bre_api_pass.hip
bre_status check_params(bre_ctx *c, const bre_render_params *rp);
// the write schedule of bre_render_progressive: is an image due after iteration `it`?
bool image_due(int32_t it, int32_t end_iteration, int32_t write_frequency);
// the bre_image_fn of bre_render and bre_render_sharded: keeps the last image it is given
struct FinalImage {
    float *dst;
    size_t n;
};
inline int keep_final_image(int32_t, const float *img, void *user) {
    const FinalImage *f = static_cast<const FinalImage *>(user);
    memcpy(f->dst, img, f->n * sizeof(float));
    return 0;
}
// bre_api_scene.hip: a bre_scene against the context's SceneState; the DevScene the kernels read
// (c->dev.record), rebuilt and copied only where it changed
bre_status check_scene(bre_ctx *c, const bre_scene *scene, const char *fn);
bre_status check_medium(bre_ctx *c, const bre_scene *scene, const char *fn);
bre_status upload_scene(bre_ctx *c, const bre_scene *scene);
// the part that differs, "lights (bre_set_lights)", "materials ..." or "media ...", or null: the same state
const char *scene_state_differs(const SceneState &a, const SceneState &b);
// a plastic, metal or matte record as bre_set_materials_ex checks and keeps it (colours clamped): "", or what
// is wrong with it
std::string check_glossy_material(bre_material_ex &m);
// ... the same for every type from BRE_MATERIAL_MATTE up (bre_device_check kind 14)
std::string check_lobed_or_glossy_material(bre_material_ex &m);
// a whole table as bre_set_materials_ex checks it on a context without media, the rules a mix brings included
// (records clamped in place); "" or what material *bad has
std::string check_material_table(std::vector<bre_material_ex> &mats, int *bad);
// bre_api_build.hip
bre_status build(bre_ctx *c, int64_t n, const BeamView &in);

#define HIPCHK(ctx, call)                                                                                    \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fail((ctx), e_ == hipErrorOutOfMemory ? BRE_ERR_OOM : BRE_ERR_HIP, "%s: %s (%s:%d)", #call, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                          \
    } while (0)

// return a failing status to the caller
#define BRE_TRY(call)                    \
    do {                                 \
        const bre_status st_ = (call);   \
        if (st_ != BRE_OK) return st_;   \
    } while (0)

// The photon pass (with its BVH build) and the camera pass run on a stream of the device's highest
// priority, forked from the caller's stream and joined back to it (option 117, default on): stream
// order towards the caller is unchanged, but when two contexts pipeline the render (iteration k+1's
// passes beside iteration k's gather, bench.py --pipeline 1) the dispatcher hands the passes' few
// workgroups the CUs as the gather's one-wave blocks retire, instead of queueing them behind millions
// of gather blocks (round 4: k_photons averaged 80 ms in the pipelined trace against 1.4 ms alone).
struct PassStream {
    bre_ctx *c;
    hipStream_t user = nullptr;
    PassStream(bre_ctx *c_) : c(c_) {
        if (!c->pass_priority) return;
        if (!c->pstream) {
            int least = 0, greatest = 0;
            if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return;
            if (hipStreamCreateWithPriority(&c->pstream.h, hipStreamNonBlocking, greatest) != hipSuccess) {
                c->pstream.h = nullptr;
                return;
            }
            c->pstream.owned = true;
            if (hipEventCreateWithFlags(&c->fork_ev.h, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&c->join_ev.h, hipEventDisableTiming) != hipSuccess)
                return;
        }
        if (!c->fork_ev || !c->join_ev) return;
        if (hipEventRecord(c->fork_ev, c->stream) != hipSuccess ||
            hipStreamWaitEvent(c->pstream, c->fork_ev, 0) != hipSuccess)
            return;
        user = c->stream;
        c->stream.h = c->pstream;
    }
    ~PassStream() {
        if (!user) return;
        // the caller's stream waits for everything the pass queued (also on an early error return)
        (void)hipEventRecord(c->join_ev, c->pstream);
        (void)hipStreamWaitEvent(user, c->join_ev, 0);
        c->stream.h = user;
    }
};

}  // namespace bre
