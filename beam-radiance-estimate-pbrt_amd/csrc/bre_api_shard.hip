// bre_api_shard.hip — the multi-GPU calls of the C ABI: one host thread per context, each driving the
// single-context entry points (bre_set_beams, bre_gather) on its own device.
#include <string>
#include <thread>
#include <vector>

#include "bre_ctx.h"

using namespace bre;

namespace {
struct ShardSave {
    int mode, count, rank, block;
};
// Run fn(i) for every context on its own thread (fn(0) on the caller's); the first failing
// context's status and message (prefixed with its index) end up in ctxs[0].
template <typename Fn>
bre_status for_each_ctx(bre_ctx *const *ctxs, int n, Fn fn) {
    std::vector<bre_status> st((size_t)n, BRE_OK);
    std::vector<std::thread> th;
    th.reserve((size_t)n);
    for (int i = 1; i < n; ++i) th.emplace_back([&, i] { st[(size_t)i] = fn(i); });
    st[0] = fn(0);
    for (auto &t : th) t.join();
    for (int i = 0; i < n; ++i) {
        if (st[(size_t)i] == BRE_OK) continue;
        const std::string msg = "context " + std::to_string(i) + ": " + ctxs[i]->err;
        ctxs[0]->err = msg;
        return st[(size_t)i];
    }
    return BRE_OK;
}
bre_status check_ctxs(bre_ctx *const *ctxs, int n) {
    if (!ctxs || n < 1) return BRE_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i]) return BRE_ERR_INVALID_ARG;
        for (int j = 0; j < i; ++j)
            if (ctxs[j] == ctxs[i]) return fail(ctxs[0], BRE_ERR_INVALID_ARG, "bre_*_sharded: context %d repeated", i);
    }
    return BRE_OK;
}
}  // namespace

extern "C" {

bre_status bre_set_beams_sharded(bre_ctx *const *ctxs, int n_ctx, int64_t n, const float *start, const float *end,
                                 const float *radius, const float *power) {
    BRE_TRY(check_ctxs(ctxs, n_ctx));
    return for_each_ctx(ctxs, n_ctx, [&](int i) { return bre_set_beams(ctxs[i], n, start, end, radius, power); });
}

bre_status bre_gather_sharded(bre_ctx *const *ctxs, int n_ctx, int64_t nseg, const float *o, const float *p,
                              const float *d, const float *tmax, const int32_t *pixel, float R, int64_t npix,
                              float *accum, float *seg_rgb, int32_t *seg_counts) {
    BRE_TRY(check_ctxs(ctxs, n_ctx));
    if (nseg < 0 || npix < 0) return fail(ctxs[0], BRE_ERR_INVALID_ARG, "bre_gather_sharded: negative size");
    for (int i = 0; i < n_ctx; ++i)
        if (ctxs[i]->film_classes > 1)
            return fail(ctxs[0], BRE_ERR_STATE, "bre_gather_sharded: BRE_OPT_FILM_CLASSES is for caller device films");
    const size_t F = accum && npix > 0 ? (size_t)npix * 3 : 0, S = (size_t)nseg;
    // per context: its partial film and per-segment outputs (only its own packets' entries are
    // nonzero); the contexts' shard options are set for the call and restored afterwards
    std::vector<std::vector<float>> film((size_t)n_ctx), rgb((size_t)n_ctx);
    std::vector<std::vector<int32_t>> cnt((size_t)n_ctx);
    std::vector<ShardSave> saved((size_t)n_ctx);
    for (int i = 0; i < n_ctx; ++i) {
        bre_ctx *c = ctxs[i];
        saved[(size_t)i] = ShardSave{c->shard_mode, c->shard_count, c->shard_rank, c->shard_block};
        c->shard_mode = 1;
        c->shard_count = n_ctx;
        c->shard_rank = i;
        c->shard_block = 1;
    }
    const bre_status st = for_each_ctx(ctxs, n_ctx, [&](int i) {
        const size_t k = (size_t)i;
        film[k].assign(F, 0.f);
        if (seg_rgb) rgb[k].assign(S * 3, 0.f);
        if (seg_counts) cnt[k].assign(S * 2, 0);
        return bre_gather(ctxs[i], nseg, o, p, d, tmax, pixel, R, npix, F ? film[k].data() : nullptr,
                          seg_rgb ? rgb[k].data() : nullptr, seg_counts ? cnt[k].data() : nullptr);
    });
    for (int i = 0; i < n_ctx; ++i) {
        bre_ctx *c = ctxs[i];
        const ShardSave &v = saved[(size_t)i];
        c->shard_mode = v.mode;
        c->shard_count = v.count;
        c->shard_rank = v.rank;
        c->shard_block = v.block;
    }
    if (st != BRE_OK) return st;
    // each output is the contexts' parts added in context order (deterministic)
    const auto sum = [&](const auto &parts, size_t len, auto *out, bool add) {
        for (size_t j = 0; j < len; ++j) {
            auto v = parts[0][j];
            for (int i = 1; i < n_ctx; ++i) v += parts[(size_t)i][j];
            out[j] = add ? out[j] + v : v;
        }
    };
    sum(film, F, accum, true);                           // the films, then into the caller's Ld
    if (seg_rgb) sum(rgb, S * 3, seg_rgb, false);        // one nonzero term per entry
    if (seg_counts) sum(cnt, S * 2, seg_counts, false);
    return BRE_OK;
}

}  // extern "C"
