// bre_api.hip — C ABI of libbre.so (include/bre.h): context lifetime, options, stream, stats, the
// gather-after links and events, and the small device reads and fills every other unit uses
// (bre_ctx.h).  The build is in bre_api_build.hip, the gathers in bre_api_gather.hip, the scene setters and
// upload in bre_api_scene.hip, the passes in bre_api_pass.hip, the multi-context calls in bre_api_shard.hip,
// the test hooks in bre_api_check.hip and the host-only helpers in bre_api_host.hip.  No exceptions cross
// the ABI; every failure is a status code plus a message for bre_last_error().
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "bre_ctx.h"

namespace bre {

bre_status fail(bre_ctx *c, bre_status st, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return st;
}

bre_status set_device(bre_ctx *c) {
    HIPCHK(c, hipSetDevice(c->device));
    return BRE_OK;
}

// Zero `bytes` (a multiple of 4) of device memory on the context's stream: a one-wave fill kernel
// (bre_slot.hip) instead of hipMemsetAsync's runtime kernel, which waits for CUs behind a concurrent
// gather (the pipelined pass chain); option 119 = 0 keeps hipMemsetAsync.
hipError_t fill_words(bre_ctx *c, void *p, size_t bytes) {
    if (!c->slot_passes || bytes % 4) return hipMemsetAsync(p, 0, bytes, c->stream);
    return slot_fill(p, (int64_t)(bytes / 4), 0u, c->stream);
}

// Small device-to-host reads of the pass chain (the photon total, the build's valid count, the camera
// pass's segment total, the sticky error flags), synchronising the context's stream.  With option 118
// a one-wave kernel stores the words into pinned host memory; otherwise hipMemcpyAsync, whose copy
// kernel (the runtime's own, with multi-wave workgroups) waited up to 32 ms for CUs behind a
// concurrent gather's one-wave blocks in the round-5 pipelined trace.
namespace {
struct ReadSpans {
    const unsigned int *src[4];
    int words[4];
    int n;
};
__global__ __launch_bounds__(64) void k_readback(ReadSpans r, unsigned int *__restrict__ dst) {
    int o = 0;
    for (int i = 0; i < r.n; ++i) {
        if ((int)threadIdx.x < r.words[i]) dst[o + threadIdx.x] = r.src[i][threadIdx.x];
        o += r.words[i];
    }
}
}  // namespace
bre_status read_small(bre_ctx *c, std::initializer_list<HostSpan> spans) {
    if (!c->kernel_readback) {
        for (const HostSpan &h : spans)
            HIPCHK(c, hipMemcpyAsync(h.host, h.dev, h.bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BRE_OK;
    }
    if (!c->rb_host) HIPCHK(c, hipHostMalloc((void **)&c->rb_host.h, 64 * sizeof(unsigned int), hipHostMallocDefault));
    ReadSpans r{};
    int tot = 0;
    for (const HostSpan &h : spans) {
        if (r.n == 4 || h.bytes % 4 || tot + (int)(h.bytes / 4) > 64) return fail(c, BRE_ERR_STATE, "read_small: bad span");
        r.src[r.n] = static_cast<const unsigned int *>(h.dev);
        r.words[r.n] = (int)(h.bytes / 4);
        tot += r.words[r.n++];
    }
    hipLaunchKernelGGL(k_readback, dim3(1), dim3(64), 0, c->stream, r, c->rb_host.h);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int o = 0;
    for (const HostSpan &h : spans) {
        memcpy(h.host, c->rb_host.h + o, h.bytes);
        o += (int)(h.bytes / 4);
    }
    return BRE_OK;
}

// The counter block of the context: zeroed once at allocation; per gather only the counters are
// zeroed, the sticky `flags` word stays until check_flags has read it.
bre_status counters_block(bre_ctx *c, DevCounters **out) {
    if (!c->counters_buf.ptr) {
        HIPCHK(c, c->counters_buf.ensure(sizeof(DevCounters)));
        HIPCHK(c, fill_words(c, c->counters_buf.ptr, sizeof(DevCounters)));
    }
    *out = c->counters_buf.as<DevCounters>();
    static_assert(offsetof(DevCounters, flags) % 4 == 0, "DevCounters: word-aligned flags");
    HIPCHK(c, fill_words(c, *out, offsetof(DevCounters, flags)));
    return BRE_OK;
}

// Synchronise the stream and turn the device's sticky error flags into a status (then clear them).
// Every synchronising entry point ends here, so a traversal-stack overflow or a bad pixel index of
// an earlier asynchronous gather is reported whatever the counters option (never silent).
bre_status check_flags(bre_ctx *c) {
    if (!c->counters_buf.ptr) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BRE_OK;
    }
    if (!c->flags_host) HIPCHK(c, hipHostMalloc((void **)&c->flags_host.h, sizeof(unsigned int), hipHostMallocDefault));
    unsigned int *dflags = &c->counters_buf.as<DevCounters>()->flags;
    BRE_TRY(read_small(c, {{c->flags_host.h, dflags, sizeof(unsigned int)}}));
    const unsigned int f = *c->flags_host.h;
    if (f == 0) return BRE_OK;
    HIPCHK(c, fill_words(c, dflags, sizeof(unsigned int)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (f & kFlagStack)
        return fail(c, BRE_ERR_STATE, "bre_gather: traversal stack overflow (BVH deeper than the stack): contributions "
                    "were dropped");
    return fail(c, BRE_ERR_INVALID_ARG, "bre_gather: seg_pixel out of [0, npix): segments were skipped");
}

}  // namespace bre

using namespace bre;

// bre_set_gather_after links: guarded, since the two contexts may be driven from two host threads
static std::mutex &link_mu() {
    static std::mutex m;
    return m;
}
static void unlink_follower(bre_ctx *lead, bre_ctx *f) {
    auto &v = lead->followers;
    v.erase(std::remove(v.begin(), v.end(), f), v.end());
}

// The options that are an int in lo..hi: bre_set_option checks the range, reports `msg` (which may
// print hi as %d) and stores the value.
namespace {
struct IntOption {
    int id;
    int bre_ctx::*field;
    int lo, hi;
    const char *msg;
};
const IntOption kIntOptions[] = {
    {BRE_OPT_LEAF_SIZE, &bre_ctx::leaf_size, 1, 64, "BRE_OPT_LEAF_SIZE must be in 1..64"},
    {BRE_OPT_SQRT_MODE, &bre_ctx::sqrt_mode, 0, 1, "BRE_OPT_SQRT_MODE must be 0 or 1"},
    // kernel 5: chunk length in units of E / 100 (default 400)
    {BRE_OPT_CHUNK_LEN, &bre_ctx::chunk_len, 25, 100000, "BRE_OPT_CHUNK_LEN must be in 25..100000 (units of E/100)"},
    // kernel 5: chunks per LBVH leaf
    {BRE_OPT_CHUNK_LEAF, &bre_ctx::chunk_leaf, 1, 64, "BRE_OPT_CHUNK_LEAF must be in 1..64"},
    // kernel 0: beams per leaf tile of the tile tree (default 64, best at C2)
    {BRE_OPT_TILE_LEAF, &bre_ctx::leaf2, 1, 64, "BRE_OPT_TILE_LEAF must be in 1..64"},
    // tiles per side (image-tile shards) or packets (packet shards) of the blocks dealt to the shards
    {BRE_OPT_SHARD_BLOCK, &bre_ctx::shard_block, 1, 4096, "BRE_OPT_SHARD_BLOCK must be in 1..4096"},
    // 0 image tiles, 1 packet ranges, 2 work roots
    {BRE_OPT_SHARD_MODE, &bre_ctx::shard_mode, 0, 2, "BRE_OPT_SHARD_MODE must be 0, 1 or 2"},
    // internal: traversal stack entries to use, 0 = all (tests force an overflow)
    {101, &bre_ctx::stack_cap, 0, kStackDepth, "stack cap must be in 0..%d"},
    // internal: segment coherence sort key (SegSort::key_mode, sweeps); default 4, measured best at C2
    {105, &bre_ctx::sort_key, 0, 4, "segment sort key must be 0..4"},
    // internal: tile kernel block mapping (GatherArgs::block_map), 0 XCD-aware subtrees / 1 rotated /
    // 3 LPT, roots by size (default; sweeps)
    {107, &bre_ctx::block_map, 0, 3, "block map must be 0..3"},
    // internal: tile kernel transposed-scan threshold in eighths (GatherArgs::tscan), 0 = off, -1 = by the
    // gather's MaxDistance (tscan_for, bre_api_gather.hip; the default since round 6, 4 fixed until then:
    // round 5, 4 over 6, C2 +0.5%, C3 +4.8%, profiles/r5/run20, run22)
    {108, &bre_ctx::tscan, -1, 64, "transposed-scan threshold must be in -1..64"},
    // internal: tree order of the build (BuildBuffers::beam_key): 2 / 1 (start, end) in Hilbert (default) /
    // Morton order, 0 centroid
    {110, &bre_ctx::beam_key, 0, 2, "tree order must be 0..2"},
    // internal: tile kernel prefilter margins (GatherArgs::margin), 1 tight (default) / 0 round 2's (A/B)
    {111, &bre_ctx::margin, 0, 1, "margin mode must be 0 or 1"},
    // internal: per-lane tile line reject (GatherArgs::tileax), 1 on (default since round 4) / 0 off (A/B);
    // 2 = 1 (round-4 scripts)
    {112, &bre_ctx::tile_axis, 0, 2, "tile axis mode must be 0, 1 or 2"},
    // internal: beam record layout, 0 power in the record for uniform-radius sets (default) / 1 always radius
    // in the record, power apart (never carry the power in BeamRec; A/B; applies from the next build)
    {113, &bre_ctx::split_records, 0, 1, "record layout must be 0 or 1"},
    // internal: film accumulation, 1 deterministic per-pixel compose (default) / 0 float atomics (A/B)
    {114, &bre_ctx::film_compose, 0, 1, "film mode must be 0 or 1"},
    // internal: photon pass, 1 single trace with per-photon slots (default) / 0 two traces (A/B) /
    // 2..64 single trace with that many slots per photon (tests: forces the overflow re-trace)
    {116, &bre_ctx::photon_single, 0, 64, "photon pass mode must be in 0..64"},
    // internal: photon / camera passes on a high-priority stream (PassStream), 1 (default) / 0 on the caller's (A/B)
    {117, &bre_ctx::pass_priority, 0, 1, "pass priority must be 0 or 1"},
    // internal: small device-to-host reads (read_small) by a one-wave kernel into pinned memory (1) / hipMemcpyAsync (0)
    {118, &bre_ctx::kernel_readback, 0, 1, "readback mode must be 0 or 1"},
    // internal: pass-chain scans / sorts / fills, 1 the one-wave primitives (bre_slot.hip, default) / 0 rocPRIM
    // and hipMemsetAsync (A/B)
    {119, &bre_ctx::slot_passes, 0, 1, "pass primitives mode must be 0 or 1"},
    // internal: coarse sort keys (1: the tree-order sort on bits [16, 64), the segment sort on [12, 60): 6 radix
    // passes each instead of 8; round 6, profiles/r6/e13) / all bits (0, default).  Off: its first form hung the
    // full C5 render (the hierarchy saw unsorted low bits) and the fixed form is not yet measured on the GPU.
    {121, &bre_ctx::coarse_keys, 0, 1, "coarse keys mode must be 0 or 1"},
    // internal: the film collective of the sharded calls, read from context 0: 0 (default) reads a source on context
    // 0's device in place and stages only the other devices' through hipMemcpyPeerAsync / 1 stages every non-root
    // source (tests: the cross-device path on one GPU)
    {122, &bre_ctx::stage_all, 0, 1, "collective staging must be 0 or 1"},
    // internal: the tile kernel's specialised production instantiation (TileProd, bre_gather.hip), 1 allowed
    // (default) whenever a launch's bound options and beam set match it / 0 always the generic one (A/B).
    // bre_stats::tile_variant reports which one the last gather ran.
    {123, &bre_ctx::tile_spec, 0, 1, "tile specialisation must be 0 or 1"},
};
}  // namespace

extern "C" {

int bre_abi_version(void) { return BRE_ABI_VERSION; }

bre_status bre_create(int device, bre_ctx **out) {
    if (!out) return BRE_ERR_INVALID_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return BRE_ERR_NO_DEVICE;
    if (device < 0 || device >= count) return BRE_ERR_NO_DEVICE;
    bre_ctx *c = new bre_ctx();
    c->device = device;
    // a half-built context releases what it holds (delete c)
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return BRE_ERR_HIP;
    }
    c->stream.owned = true;
    for (auto &e : c->ev) {
        if (hipEventCreate(&e.h) != hipSuccess) {
            delete c;
            return BRE_ERR_HIP;
        }
    }
    *out = c;
    return BRE_OK;
}

void bre_destroy(bre_ctx *c) {
    if (!c) return;
    {
        // a pipelined partner must not keep waiting on this context's event once it is gone
        std::lock_guard<std::mutex> lk(link_mu());
        for (bre_ctx *f : c->followers) f->after = nullptr;
        if (c->after) unlink_follower(c->after, c);
    }
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->pstream) (void)hipStreamSynchronize(c->pstream);
    delete c;  // every member releases what it owns (bre_ctx.h); the caller's stream and events are not owned
}

const char *bre_last_error(const bre_ctx *c) { return c ? c->err.c_str() : "null context"; }

bre_status bre_set_option(bre_ctx *c, int option, int64_t value) {
    if (!c) return BRE_ERR_INVALID_ARG;
    for (const IntOption &o : kIntOptions) {
        if (o.id != option) continue;
        if (value < o.lo || value > o.hi) return fail(c, BRE_ERR_INVALID_ARG, o.msg, o.hi);
        c->*o.field = (int)value;
        return BRE_OK;
    }
    switch (option) {
    case BRE_OPT_COUNTERS: c->counters = value != 0; return BRE_OK;
    case BRE_OPT_TIMING: c->timing = value != 0; return BRE_OK;
    case BRE_OPT_PREFILTER: c->prefilter = value != 0; return BRE_OK;
    case BRE_OPT_SORT_SEGMENTS: c->sort_segments = value != 0; return BRE_OK;
    case BRE_OPT_KERNEL:
        if (value != 0 && value != 2 && value != 4 && value != 5)
            return fail(c, BRE_ERR_INVALID_ARG, "BRE_OPT_KERNEL must be 0, 2, 4 or 5 (kernels 1, 3 and 6 were removed)");
        c->kernel = (int)value;
        return BRE_OK;
    case BRE_OPT_SPLIT:
        // work roots per packet: default 256 (r2: 64 with the rotated block map, C2 +42% over 8; 256 +2% on the
        // final kernel, partials 3 KB per segment)
        if (value < 1 || value > kMaxSplit || (value & (value - 1)))
            return fail(c, BRE_ERR_INVALID_ARG, "BRE_OPT_SPLIT must be a power of two in 1..%d", kMaxSplit);
        c->split = (int)value;
        return BRE_OK;
    case BRE_OPT_SHARD_RANK:  // this context's shard: image tiles of the camera pass, packets or work roots
        if (value < 0 || value >= c->shard_count)
            return fail(c, BRE_ERR_INVALID_ARG, "BRE_OPT_SHARD_RANK must be in [0, shard count)");
        c->shard_rank = (int)value;
        return BRE_OK;
    case BRE_OPT_SHARD_COUNT:
        if (value < 1 || value > 65536) return fail(c, BRE_ERR_INVALID_ARG, "BRE_OPT_SHARD_COUNT must be in 1..65536");
        c->shard_count = (int)value;
        if (c->shard_rank >= c->shard_count) c->shard_rank = 0;
        return BRE_OK;
    case BRE_OPT_FILM_CLASSES:  // 1, or BRE_FILM_CLASSES planes per film
        if (value != 1 && value != BRE_FILM_CLASSES)
            return fail(c, BRE_ERR_INVALID_ARG, "BRE_OPT_FILM_CLASSES must be 1 or %d", BRE_FILM_CLASSES);
        c->film_classes = (int)value;
        return BRE_OK;
    case BRE_OPT_SEGMENT_BUDGET:  // camera pass with media: segment planes beyond maxdepth
        if (value < 0 || value > 240) return fail(c, BRE_ERR_INVALID_ARG, "segment budget must be in 0..240");
        c->seg_budget = (int)value;
        return BRE_OK;
    case 102:  // internal: tile kernel register budget, min waves per SIMD (sweeps); default 6 with the lane ray
               // in registers (r2 final, 77 VGPRs; explore38)
        if (value != 1 && (value < 4 || value > 8))
            return fail(c, BRE_ERR_INVALID_ARG, "occupancy must be 1 or 4..8");
        c->occupancy = (int)value;
        return BRE_OK;
    case 124:  // internal: register budget of the tile kernel's specialised instantiation (TileProd), 7 (default:
               // 72 VGPRs and 5,120 B of LDS, seven waves on every SIMD, C2 +2.2%) or 6 waves
               // per SIMD (A/B): k_gather_tile<false, 7 or 6, TileProd>.  Option 102 keeps its meaning (the generic
               // instantiations' budget; the specialised one still needs it at its default 6), and
               // bre_stats::tile_variant is 2 at either budget.  Bound per launch, like option 123.
        if (value != 6 && value != 7) return fail(c, BRE_ERR_INVALID_ARG, "specialised tile budget must be 6 or 7");
        c->tile_budget = (int)value;
        return BRE_OK;
    case 109:  // internal: tile kernel bytes of per-subtree partial sums per launch, in MiB (default 4 GiB; tests
               // force several launches)
        if (value < 1 || value > ((int64_t)1 << 20)) return fail(c, BRE_ERR_INVALID_ARG, "partial cap must be in 1..2^20 MiB");
        c->partial_cap = value << 20;
        return BRE_OK;
    default: return fail(c, BRE_ERR_INVALID_ARG, "unknown option %d", option);
    }
}

bre_status bre_set_stream(bre_ctx *c, void *stream) {
    if (!c) return BRE_ERR_INVALID_ARG;
    c->stream.reset();
    if (stream) {
        c->stream.h = (hipStream_t)stream;
    } else {
        if (hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking) != hipSuccess)
            return fail(c, BRE_ERR_HIP, "hipStreamCreate failed");
        c->stream.owned = true;
    }
    return BRE_OK;
}

bre_status bre_synchronize(bre_ctx *c) {
    if (!c) return BRE_ERR_INVALID_ARG;
    return check_flags(c);
}

bre_status bre_get_stats(const bre_ctx *c, bre_stats *out) {
    if (!c || !out) return BRE_ERR_INVALID_ARG;
    *out = c->stats;
    return BRE_OK;
}

bre_status bre_set_gather_events(bre_ctx *c, void *start_event, void *end_event) {
    if (!c) return BRE_ERR_INVALID_ARG;
    c->user_ev[0] = static_cast<hipEvent_t>(start_event);
    c->user_ev[1] = static_cast<hipEvent_t>(end_event);
    return BRE_OK;
}

bre_status bre_set_gather_after(bre_ctx *c, bre_ctx *prev) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (prev == c || (prev && prev->device != c->device))
        return fail(c, BRE_ERR_INVALID_ARG, "bre_set_gather_after: another context of the same device");
    std::lock_guard<std::mutex> lk(link_mu());
    if (c->after) unlink_follower(c->after, c);
    c->after = prev;
    if (prev) prev->followers.push_back(c);
    return BRE_OK;
}

}  // extern "C"
