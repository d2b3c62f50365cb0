// bre_api_shard.hip — the multi-GPU calls of the C ABI: one host thread per context, each driving the
// single-context entry points (bre_set_beams, bre_gather, the passes of a render iteration) on its own
// device, and the film collective that brings the contexts' films together on context 0's device.
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bre_ctx.h"

using namespace bre;

namespace {
constexpr int kMaxCtx = 8;  // contexts of one sharded render

// The options a sharded call sets on every context for its duration
struct ShardSave {
    int mode, count, rank, block, classes;
};
struct ShardScope : NoCopy {
    bre_ctx *const *ctxs;
    int n;
    std::vector<ShardSave> saved;
    // packet shards (mode 1, count n, rank i, block 1) with `classes` film planes
    ShardScope(bre_ctx *const *ctxs_, int n_, int classes) : ctxs(ctxs_), n(n_), saved((size_t)n_) {
        for (int i = 0; i < n; ++i) {
            bre_ctx *c = ctxs[i];
            saved[(size_t)i] = ShardSave{c->shard_mode, c->shard_count, c->shard_rank, c->shard_block, c->film_classes};
            c->shard_mode = 1;
            c->shard_count = n;
            c->shard_rank = i;
            c->shard_block = 1;
            c->film_classes = classes;
        }
    }
    ~ShardScope() {
        for (int i = 0; i < n; ++i) {
            bre_ctx *c = ctxs[i];
            const ShardSave &v = saved[(size_t)i];
            c->shard_mode = v.mode;
            c->shard_count = v.count;
            c->shard_rank = v.rank;
            c->shard_block = v.block;
            c->film_classes = v.classes;
        }
    }
};

// The first failing context's status, its message (prefixed with its index) in ctxs[0]
bre_status first_failure(bre_ctx *const *ctxs, int n, const bre_status *st) {
    for (int i = 0; i < n; ++i) {
        if (st[i] == BRE_OK) continue;
        const std::string msg = "context " + std::to_string(i) + ": " + ctxs[i]->err;
        ctxs[0]->err = msg;
        return st[i];
    }
    return BRE_OK;
}
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
    return first_failure(ctxs, n, st.data());
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

// The film collective on context 0's device.  Every context records `done[i]` on its stream behind the last
// write of its film; context 0's stream waits for the events, reads a source on its own device in place,
// copies a source of another device (every non-root source with internal option 122) into `stage` with
// hipMemcpyPeerAsync on its own stream, and adds the sources in table order with one kernel
// (launch_film_sum) into `out`.  Only context 0's thread calls add / sum.
struct Collective : NoCopy {
    bre_ctx *const *ctxs;
    int n;
    std::vector<Event> done;
    DevMem stage, out;  // on context 0's device
    FilmSources table{};
    size_t staged = 0;  // floats of `stage` in use
    Collective(bre_ctx *const *ctxs_, int n_) : ctxs(ctxs_), n(n_), done((size_t)n_) {}
    // the events, each on its context's device, and room for `stage_floats` staged and `out_floats` summed floats
    bre_status prepare(size_t stage_floats, size_t out_floats) {
        for (int i = 1; i < n; ++i) {
            BRE_TRY(set_device(ctxs[i]));
            HIPCHK(ctxs[i], hipEventCreateWithFlags(&done[(size_t)i].h, hipEventDisableTiming));
        }
        bre_ctx *r = ctxs[0];
        BRE_TRY(set_device(r));
        if (n > 1) HIPCHK(r, stage.ensure((stage_floats > 0 ? stage_floats : 1) * sizeof(float)));
        HIPCHK(r, out.ensure((out_floats > 0 ? out_floats : 1) * sizeof(float)));
        return BRE_OK;
    }
    // context i (its own thread): its film is complete behind everything queued on its stream so far
    bre_status mark(int i) {
        if (i == 0) return BRE_OK;
        HIPCHK(ctxs[i], hipEventRecord(done[(size_t)i], ctxs[i]->stream));
        return BRE_OK;
    }
    void begin() {
        table.n = 0;
        staged = 0;
    }
    // the next source: `floats` floats at `src`, owned by context i.  A full table is first added up into `out`,
    // which then heads the table: the order of the adds stays the order of the sources.
    bre_status add(int i, const float *src, size_t floats) {
        bre_ctx *r = ctxs[0];
        if (table.n == kFilmSources) {
            if (floats * sizeof(float) > out.cap) return fail(r, BRE_ERR_STATE, "film collective: output overflow");
            HIPCHK(r, launch_film_sum(table, (int64_t)floats, out.as<float>(), 0, r->stream));
            table.src[0] = out.as<float>();
            table.n = 1;
        }
        if (i != 0 && (ctxs[i]->device != r->device || r->stage_all)) {
            if ((staged + floats) * sizeof(float) > stage.cap) return fail(r, BRE_ERR_STATE, "film collective: staging overflow");
            float *dst = stage.as<float>() + staged;
            HIPCHK(r, hipMemcpyPeerAsync(dst, r->device, src, ctxs[i]->device, floats * sizeof(float), r->stream));
            staged += floats;
            src = dst;
        }
        table.src[table.n++] = src;
        return BRE_OK;
    }
    // context 0's stream waits for the other contexts' films (before the first add of a round)
    bre_status wait_films() {
        bre_ctx *r = ctxs[0];
        for (int i = 1; i < n; ++i) HIPCHK(r, hipStreamWaitEvent(r->stream, done[(size_t)i], 0));
        return BRE_OK;
    }
    // out = the sources in table order; then the `floats` floats to the host, synchronising context 0's stream
    bre_status sum_to_host(size_t floats, float *host) {
        bre_ctx *r = ctxs[0];
        if (floats * sizeof(float) > out.cap) return fail(r, BRE_ERR_STATE, "film collective: output overflow");
        HIPCHK(r, launch_film_sum(table, (int64_t)floats, out.as<float>(), 0, r->stream));
        HIPCHK(r, hipMemcpyAsync(host, out.ptr, floats * sizeof(float), hipMemcpyDeviceToHost, r->stream));
        HIPCHK(r, hipStreamSynchronize(r->stream));
        return BRE_OK;
    }
};

// All n threads arrive, then all leave
class Rendezvous {
  public:
    explicit Rendezvous(int n) : n_(n) {}
    void arrive_and_wait() {
        std::unique_lock<std::mutex> lk(mu_);
        const unsigned gen = gen_;
        if (++count_ == n_) {
            count_ = 0;
            ++gen_;
            cv_.notify_all();
            return;
        }
        cv_.wait(lk, [&] { return gen_ != gen; });
    }

  private:
    std::mutex mu_;
    std::condition_variable cv_;
    const int n_;
    int count_ = 0;
    unsigned gen_ = 0;
};

// The class-plane films (n_ctx divides 8: the same bits for every such count) need the deterministic
// per-pixel compose of kernels 0 / 4 wherever a gather runs
bool class_films(int n_ctx) { return BRE_FILM_CLASSES % n_ctx == 0; }

// What the call cannot do is refused before any launch, no context changed
bre_status check_render_sharded(bre_ctx *const *ctxs, int n_ctx, const bre_scene *scene, const bre_render_params *rp,
                                const char *fn) {
    // the count first: no more than kMaxCtx entries of the caller's array are read
    if (n_ctx > kMaxCtx)
        return fail(ctxs ? ctxs[0] : nullptr, BRE_ERR_INVALID_ARG, "%s: at most %d contexts", fn, kMaxCtx);
    BRE_TRY(check_ctxs(ctxs, n_ctx));
    if (!scene) return fail(ctxs[0], BRE_ERR_INVALID_ARG, "%s: null scene", fn);
    BRE_TRY(check_params(ctxs[0], rp));
    // the contexts' films are summed: every context must light the scene alike, shade it alike, in the same media
    for (int i = 1; i < n_ctx; ++i)
        if (const char *part = scene_state_differs(ctxs[0]->held, ctxs[i]->held))
            return fail(ctxs[0], BRE_ERR_INVALID_ARG, "context %d: %s: its %s differ from context 0's", i, fn, part);
    if (!class_films(n_ctx) || !rp->render_media) return BRE_OK;
    for (int i = 0; i < n_ctx; ++i) {
        const bre_ctx *c = ctxs[i];
        if ((c->kernel == 0 || c->kernel == 4) && c->film_compose) continue;
        return fail(ctxs[0], BRE_ERR_STATE, "context %d: %s: %d contexts render class-plane films, which need the deterministic "
                    "compose of kernels 0 / 4", i, fn, n_ctx);
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
    Collective coll(ctxs, F ? n_ctx : 1);
    if (F) BRE_TRY(coll.prepare((size_t)(n_ctx - 1) * F, F));
    // per context: its partial film (on its device, c->g_accum) and per-segment outputs (only its own
    // packets' entries are nonzero); the contexts' shard options are set for the call and restored afterwards
    std::vector<std::vector<float>> rgb((size_t)n_ctx);
    std::vector<std::vector<int32_t>> cnt((size_t)n_ctx);
    bre_status st;
    {
        ShardScope scope(ctxs, n_ctx, 1);
        st = for_each_ctx(ctxs, n_ctx, [&](int i) {
            const size_t k = (size_t)i;
            if (seg_rgb) rgb[k].assign(S * 3, 0.f);
            if (seg_counts) cnt[k].assign(S * 2, 0);
            const GatherOut out{F ? accum : nullptr, seg_rgb ? rgb[k].data() : nullptr,
                                seg_counts ? cnt[k].data() : nullptr};
            BRE_TRY(gather_host(ctxs[i], nseg, SegView{o, p, d, tmax, pixel}, R, npix, out, true));
            return F ? coll.mark(i) : BRE_OK;
        });
    }
    if (st != BRE_OK) return st;
    // each output is the contexts' parts added in context order (deterministic): the films on context
    // 0's device, then into the caller's Ld on the host
    if (F) {
        std::vector<float> film(F);
        BRE_TRY(set_device(ctxs[0]));
        coll.begin();
        BRE_TRY(coll.wait_films());
        for (int i = 0; i < n_ctx; ++i) BRE_TRY(coll.add(i, ctxs[i]->g_accum.as<float>(), F));
        BRE_TRY(coll.sum_to_host(F, film.data()));
        for (size_t j = 0; j < F; ++j) accum[j] = accum[j] + film[j];
    }
    const auto sum = [&](const auto &parts, size_t len, auto *out) {
        for (size_t j = 0; j < len; ++j) {
            auto v = parts[0][j];
            for (int i = 1; i < n_ctx; ++i) v += parts[(size_t)i][j];
            out[j] = v;
        }
    };
    if (seg_rgb) sum(rgb, S * 3, seg_rgb);  // one nonzero term per entry
    if (seg_counts) sum(cnt, S * 2, seg_counts);
    return BRE_OK;
}

bre_status bre_render_progressive_sharded(bre_ctx *const *ctxs, int n_ctx, const bre_scene *scene,
                                          const bre_render_params *rp, int32_t write_frequency, bre_image_fn on_image,
                                          void *user) {
    BRE_TRY(check_render_sharded(ctxs, n_ctx, scene, rp, "bre_render_progressive_sharded"));
    const bool classes = class_films(n_ctx);
    const int planes = classes ? BRE_FILM_CLASSES : 1;
    const size_t F = (size_t)rp->width * rp->height * 3;  // floats of one plane
    // what context 0 stages at a written image: the other contexts' own planes, or their films
    Collective coll(ctxs, n_ctx);
    BRE_TRY(coll.prepare(classes ? (size_t)(planes - planes / n_ctx) * F : (size_t)(n_ctx - 1) * F, F));
    ShardScope scope(ctxs, n_ctx, planes);
    Rendezvous meet(n_ctx);
    std::atomic<bool> failed{false};
    bool stop = false;  // written by context 0's thread between the two rendezvous of an image, read after the second
    bre_status status[kMaxCtx];
    DevMem films[kMaxCtx];  // per context: the render's film, then the iteration's
    std::vector<float> h, img;

    // context 0, between the rendezvous: the image after iteration `it`
    const auto write_image = [&](int32_t it) -> bre_status {
        bre_ctx *r = ctxs[0];
        coll.begin();
        BRE_TRY(coll.wait_films());
        if (classes) {
            // plane c from the context that computed it, the planes in class order (bre_resolve_classes')
            for (int c = 0; c < planes; ++c) BRE_TRY(coll.add(c % n_ctx, films[c % n_ctx].as<float>() + (size_t)c * F, F));
        } else {
            for (int i = 0; i < n_ctx; ++i) BRE_TRY(coll.add(i, films[i].as<float>(), F));
        }
        h.resize(F);
        img.resize(F);
        BRE_TRY(coll.sum_to_host(F, h.data()));
        BRE_TRY(bre_resolve_image((int64_t)(F / 3), h.data(), it, img.data()));  // L = Ld / (iter + 1), :578
        if (on_image(it, img.data(), user) != 0)
            return fail(r, BRE_ERR_STATE, "bre_render: image callback stopped the render after iteration %d", it);
        return BRE_OK;
    };
    const auto drive = [&](int i) {
        bre_ctx *c = ctxs[i];
        bre_status &st = status[i];
        const auto check = [&](bre_status s) {
            if (st == BRE_OK && s != BRE_OK) {
                st = s;
                failed.store(true);
            }
            return s == BRE_OK;
        };
        float *film = nullptr, *ld = nullptr;
        const auto setup = [&]() -> bre_status {
            BRE_TRY(set_device(c));
            HIPCHK(c, films[i].get(2 * (size_t)planes * F, &film));
            ld = film + (size_t)planes * F;
            HIPCHK(c, fill_words(c, film, 2 * (size_t)planes * F * sizeof(float)));
            return BRE_OK;
        };
        const auto iterate = [&](int32_t it) -> bre_status {
            BRE_TRY(bre_render_iteration(c, scene, rp, it, ld));
            // film += ld; ld = 0 (bre_film_add's operation)
            HIPCHK(c, launch_film_add((int64_t)((size_t)planes * F), ld, film, 1, c->stream));
            return BRE_OK;
        };
        check(setup());
        for (int32_t it = rp->start_iteration; it < rp->end_iteration; ++it) {
            // a failure anywhere stops the work at the next iteration boundary; the thread still arrives at every
            // rendezvous, where context 0 decides for all of them that the render ends
            if (!failed.load()) check(iterate(it));
            if (!on_image || !image_due(it, rp->end_iteration, write_frequency)) continue;
            if (!failed.load()) check(coll.mark(i));
            meet.arrive_and_wait();
            if (i == 0) {
                if (!failed.load()) check(write_image(it));
                stop = failed.load();
            }
            // the others leave their films alone until context 0's stream has read them (sum_to_host synchronises)
            meet.arrive_and_wait();
            if (stop) break;
        }
        // the last iteration's gather; also leaves the context's stream idle whatever happened
        const bre_status fst = check_flags(c);
        check(fst);
    };
    for (int i = 0; i < n_ctx; ++i) status[i] = BRE_OK;
    {
        std::vector<std::thread> th;
        th.reserve((size_t)n_ctx);
        for (int i = 1; i < n_ctx; ++i) th.emplace_back([&, i] { drive(i); });
        drive(0);
        for (auto &t : th) t.join();
    }
    (void)set_device(ctxs[0]);
    return first_failure(ctxs, n_ctx, status);
}

bre_status bre_render_sharded(bre_ctx *const *ctxs, int n_ctx, const bre_scene *scene, const bre_render_params *rp,
                              float *image) {
    BRE_TRY(check_render_sharded(ctxs, n_ctx, scene, rp, "bre_render_sharded"));
    if (!image) return fail(ctxs[0], BRE_ERR_INVALID_ARG, "bre_render_sharded: null image");
    FinalImage f{image, (size_t)rp->width * rp->height * 3};
    if (rp->end_iteration == rp->start_iteration) {
        memset(image, 0, f.n * sizeof(float));
        return BRE_OK;
    }
    // only the last iteration's image is kept (write_frequency 0 = at the end only)
    return bre_render_progressive_sharded(ctxs, n_ctx, scene, rp, 0, keep_final_image, &f);
}

}  // extern "C"
