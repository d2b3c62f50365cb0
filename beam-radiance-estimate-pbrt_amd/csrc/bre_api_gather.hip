// bre_api_gather.hip — the gathers behind the C ABI, in three layers: gather_device launches one
// kernel family on device segments (gather_chunk for kernel 5), gather_segments_core puts the segments
// in the coherence order and picks a packet shard's, gather_segments composes the film per pixel.
// The entry points gather the caller's host or device segments or the last camera pass's.
#include <algorithm>

#include "bre_ctx.h"

using namespace bre;

namespace {

// With counters or timing on, copy the counter block back (synchronising) into the stats.
bre_status read_counters(bre_ctx *c, DevCounters *ctr) {
    if (!(c->timing || c->counters)) return BRE_OK;
    DevCounters h;
    HIPCHK(c, hipMemcpyAsync(&h, ctr, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->timing) {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
        c->stats.gather_ms = ms;
    }
    c->stats.candidates = (int64_t)h.candidates;
    c->stats.contributions = (int64_t)h.contributions;
    c->stats.node_visits = (int64_t)h.node_visits;
    c->stats.leaf_visits = (int64_t)h.leaf_visits;
    c->stats.beam_evals = (int64_t)h.beam_evals;
    c->stats.ccp_wave_evals = (int64_t)h.ccp_wave_evals;
    c->stats.prefilter_rejects = (int64_t)h.prefilter_rejects;
    c->stats.useful_beam_evals = (int64_t)h.useful_beam_evals;
    c->stats.max_stack_depth = (int64_t)h.max_stack;
    c->stats.redo_items = 0;
    c->stats.queued_pairs = (int64_t)h.queued_pairs;
    c->stats.n_chunks = c->n_chunks;
    return check_flags(c);
}

// Kernel 5: build the capsule-chunk index for this gather's segments and R, then gather through it
// (bre_chunk.hip).  Every array is a context buffer reused across calls; the beam build's sort
// scratch (keys / vals / sort_tmp / leaf_parent / visit) is reused, it is dead after the build.
bre_status gather_chunk(bre_ctx *c, const GatherArgs &a) {
    const int64_t np = c->nvalid;
    c->build_scratch_ok = false;  // the chunk index reuses the beam build's keys / vals / leaf_parent
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    ChunkBuild cb;
    HIPCHK(c, c->ch_bounds.get(12, &cb.seg_bounds));
    HIPCHK(c, c->ch_counts.get((size_t)(np + 1), &cb.counts));
    HIPCHK(c, c->ch_offsets.get((size_t)(np + 1), &cb.offsets));
    HIPCHK(c, c->ch_range.get((size_t)(2 * np + 2), &cb.range));
    const size_t st = chunk_scan_temp_bytes(np);
    HIPCHK(c, c->ch_scan_tmp.ensure(st + 16));
    cb.parents = c->recs.as<BeamRec>();
    cb.bset = c->bset;
    cb.nparents = np;
    cb.seg_o = a.seg.o;
    cb.seg_p = a.seg.p;
    cb.nseg = a.nseg;
    cb.R = a.R;
    cb.len_factor = (float)c->chunk_len / 100.f;
    cb.cbounds = cb.seg_bounds + 6;
    cb.scan_tmp = c->ch_scan_tmp.ptr;
    cb.scan_tmp_bytes = st;
    HIPCHK(c, launch_chunk_count(cb, c->stream));
    int64_t total = 0;
    HIPCHK(c, hipMemcpyAsync(&total, cb.offsets + np, sizeof(total), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (total > ((int64_t)1 << 30))
        return fail(c, BRE_ERR_INVALID_ARG, "bre_gather: kernel 5 needs %lld chunks (> 2^30); raise BRE_OPT_CHUNK_LEN "
                    "or use kernel 0", (long long)total);
    c->n_chunks = total;
    if (total == 0) {
        HIPCHK(c, launch_zero_outputs(a, c->stream));
        return BRE_OK;
    }
    const size_t C = (size_t)total;
    const int K = c->chunk_leaf;
    const int64_t nleaf = (total + K - 1) / K;
    const int64_t nnodes = nleaf > 1 ? nleaf - 1 : 1;
    float *slo = nullptr, *shi = nullptr;
    int32_t *par = nullptr, *cpar = nullptr;
    ChunkRec *recs = nullptr;
    BuildBuffers bb{};
    bb.n = total;
    bb.leaf_size = K;
    bb.cbounds = cb.cbounds;
    HIPCHK(c, c->ch_box.get(C * 6, &bb.box));
    HIPCHK(c, c->ch_cent.get(C * 3, &bb.cent));
    HIPCHK(c, c->ch_slo.get(C, &slo));
    HIPCHK(c, c->ch_shi.get(C, &shi));
    HIPCHK(c, c->ch_par.get(C, &par));
    const size_t sb = sort_temp_bytes(total);
    HIPCHK(c, c->sort.reserve(C, 8, sb + 16));
    bb.keys = c->sort.keys.as<unsigned long long>();
    bb.keys_alt = c->sort.keys_alt.as<unsigned long long>();
    bb.vals = c->sort.vals;
    bb.vals_alt = c->sort.vals_alt;
    HIPCHK(c, c->ch_recs.get(C, &recs));
    HIPCHK(c, c->ch_cpar.get(C, &cpar));
    HIPCHK(c, c->ch_nodes.get((size_t)nnodes, &bb.nodes));
    HIPCHK(c, c->leaf_parent.get((size_t)nleaf, &bb.leaf_parent));
    HIPCHK(c, c->visit.get((size_t)nnodes, &bb.visit));
    HIPCHK(c, launch_chunk_emit(cb, bb.box, bb.cent, slo, shi, par, c->stream));
    bb.sort_tmp = c->sort.tmp.ptr;
    bb.sort_tmp_bytes = sb;
    bb.recs = reinterpret_cast<BeamRec *>(recs);  // same leading lo / hi layout
    bb.nodes_cap = c->ch_nodes.cap / sizeof(Node);
    bb.leaf_parent_cap = c->leaf_parent.cap / sizeof(int32_t);
    bb.visit_cap = c->visit.cap / sizeof(unsigned int);
    HIPCHK(c, launch_morton(bb, c->stream));
    HIPCHK(c, launch_sort(bb, c->stream));
    HIPCHK(c, launch_chunk_pack(cb, total, bb.vals_alt, bb.box, slo, shi, par, recs, cpar, c->stream));
    HIPCHK(c, launch_hierarchy(bb, total, c->stream));
    ChunkGatherArgs g;
    g.nseg = a.nseg;
    g.seg = a.seg;
    g.R = a.R;
    g.npix = a.npix;
    g.out = a.out;
    g.chunks = recs;
    g.chunk_parent = cpar;
    g.parents = c->recs.as<BeamRec>();
    g.pow = c->pow.as<float4>();
    g.nodes = bb.nodes;
    g.nchunks = total;
    g.leaf_size = K;
    g.prefilter = c->prefilter;
    g.ctr = a.ctr;
    HIPCHK(c, launch_gather_chunk(g, c->counters, c->stream));
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
    return read_counters(c, a.ctr);
}

// The transposed-scan threshold by the gather's MaxDistance (option 108 = -1, the default since round 6).
// A tile is scanned transposed when its on-lanes * 8 < kept beams * t; the best t falls as the pass rate of
// the lane tests rises, and that rate grows with MaxDistance against the packets' bundle spread (~0.06-0.12
// in the unit-box scenes).  Measured on one box (profiles/r6/e6, sums bit-identical for every t): C2
// iteration 0 (MaxDistance 0.02) 252.8 / 254.2 / 257.3 ms for t = 3 / 4 / 5, iteration 15 (0.005) 110.4 /
// 108.9 / 108.3 ms; C3 iteration 0 (0.02) 2965 / 3001 / 3064 ms.
int tscan_for(float maxd) { return maxd >= 0.015f ? 3 : (maxd >= 0.008f ? 4 : 5); }

// One kernel family on nseg device segments; the caller (gather_segments_core) has checked the arguments.
bre_status gather_device(bre_ctx *c, int64_t nseg, const SegView &seg, float R, int64_t npix, const GatherOut &out,
                         const int32_t *seg_index = nullptr) {
    DevCounters *ctr = nullptr;
    BRE_TRY(counters_block(c, &ctr));
    GatherArgs a{};
    a.nseg = nseg;
    a.seg = seg;
    a.R = R;
    a.npix = npix;
    a.out = out;
    a.seg_index = seg_index;
    a.recs = c->recs.as<BeamRec>();
    a.pow = c->pow.as<float4>();
    a.bset = c->bset;
    a.nodes = c->nodes.as<Node>();
    a.nvalid = c->nvalid;
    a.leaf_size = c->built_leaf_size;
    a.ctr = ctr;
    a.split = c->split;
    a.prefilter = c->prefilter;
    a.occupancy = c->occupancy;
    a.block_map = c->block_map;
    a.tscan = c->tscan >= 0 ? c->tscan : tscan_for(R + c->bset.radius);
    a.margin = c->margin;
    a.stack_cap = c->stack_cap;
    a.tile_spec = c->tile_spec;
    a.tile_budget = c->tile_budget;
    c->stats.tile_variant = 0;
    a.tile_variant = &c->stats.tile_variant;
    c->stats.n_segments = nseg;
    if (c->nvalid == 0) {
        // empty PhotonBeamBVH: Intersect returns nothing (photonbeambvh.cpp:687)
        HIPCHK(c, launch_zero_outputs(a, c->stream));
        return BRE_OK;
    }
    const int kernel = c->kernel;
    // work-root shards split the tile kernel's work roots: kernels 2 and 5 have none, and would gather
    // every segment against every beam on every shard (films summing to count x the image)
    if (c->shard_mode == 2 && c->shard_count > 1 && (kernel == 2 || kernel == 5))
        return fail(c, BRE_ERR_STATE, "work-root shards (BRE_OPT_SHARD_MODE 2) need the tile kernel (BRE_OPT_KERNEL 0 or 4)");
    if (kernel == 5) {
        if (seg_index) return fail(c, BRE_ERR_STATE, "kernel 5 gathers in the caller's order only");
        return gather_chunk(c, a);
    }
    if (kernel == 2 && seg_index) return fail(c, BRE_ERR_STATE, "kernel 2 gathers in the caller's order only");
    if (kernel == 2) {
        if (c->timing) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
        HIPCHK(c, launch_gather_thread(a, c->counters, c->stream));
        if (c->timing) HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
        return read_counters(c, a.ctr);
    }
    // Kernels 0 and 4: the tile kernel, each on the tile tree built for it.
    // The tile kernel keeps S partial sums per segment (12 B each, + 8 B of counts when asked for).
    // A gather of many segments runs as consecutive launches over whole-packet ranges, so that the
    // partials stay within partial_cap (4 GiB: C2's ~0.6M segments in one launch, C4's ~9.6M in 7)
    // and the grid within HIP's 2^32 work items.  Every segment's sum is still its subtrees'
    // partials added in root order by k_reduce: the per-segment results do not depend on the split.
    const bool want_cnt = c->counters || out.seg_counts;
    // work-root shards (BRE_OPT_SHARD_MODE 2): this shard takes every count-th work root of the
    // size-ordered list (rank, rank + count, ...) for ALL segments, so its waves sweep whole subtrees
    // with every packet, as one GPU does; the per-segment sums are this shard's subtrees' share
    const bool rshard = c->shard_mode == 2 && c->shard_count > 1;
    const int S_eff = rshard ? (c->split + c->shard_count - 1) / c->shard_count : c->split;
    const size_t per_seg = (size_t)S_eff * (12 + (want_cnt ? 8 : 0));
    // the exact stage addresses a launch's SegRec records with 32-bit byte offsets (BRE_BUF_LOADS):
    // at most 2^26 segments (64 B each) per launch (launch_chunk, bre_packet.h)
    const int64_t chunk = launch_chunk(nseg, c->partial_cap, per_seg);
    int32_t *roots = nullptr;
    HIPCHK(c, c->roots.get(kMaxSplit + 1, &roots));
    HIPCHK(c, c->partial.get(3 * (size_t)chunk * (size_t)S_eff, &a.partial));
    if (c->roots_split != c->split) {
        HIPCHK(c, c->roots_tmp.ensure(roots_scratch_bytes()));
        HIPCHK(c, launch_roots(a.nodes, c->split, roots, c->roots_tmp.ptr, c->stream));
        c->roots_split = c->split;
    }
    if (!c->nodes4_ok) {
        // the tile kernel's 4-wide view of the tree (Node4), once per build
        Node4 *nodes4 = nullptr;
        HIPCHK(c, c->nodes4.get((size_t)c->nnodes, &nodes4));
        HIPCHK(c, launch_collapse4(a.nodes, c->nnodes, nodes4, c->stream));
        c->nodes4_ok = true;
    }
    a.nodes4 = c->nodes4.as<Node4>();
    a.roots = roots;
    if (rshard) {
        int32_t *roots_sh = nullptr;
        HIPCHK(c, c->roots_sh.get(kMaxSplit + 1, &roots_sh));
        HIPCHK(c, launch_roots_shard(roots, c->split, c->shard_rank, c->shard_count, S_eff, roots_sh, c->stream));
        a.roots = roots_sh;
        a.split = S_eff;
    }
    HIPCHK(c, c->segrec.get((size_t)((chunk + 63) / 64 * 64), &a.segrec));  // whole packets
    HIPCHK(c, c->pktrec.get((size_t)packet_count(chunk), &a.pktrec));        // one record per packet of a launch
    if (want_cnt) HIPCHK(c, c->pcnt.get(2 * (size_t)chunk * (size_t)S_eff, &a.pcnt));
    if (c->tile_axis && a.leaf_size > 0) {
        const int64_t ntiles = (c->nvalid + a.leaf_size - 1) / a.leaf_size;
        HIPCHK(c, c->tileax.get((size_t)ntiles, &a.tileax));
        HIPCHK(c, c->segbox.get(8, &a.segbox));
    }
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
    if (!c->tile_ev) HIPCHK(c, hipEventCreateWithFlags(&c->tile_ev.h, hipEventDisableTiming));
    for (int64_t off = 0; off < nseg; off += chunk) {
        GatherArgs ac = a;
        // pipelined contexts (bre_set_gather_after): the first launch waits for the other context's last
        // tile kernel, the last one marks this context's
        ac.wait_ev = (off == 0 && c->after && c->after->tile_ev_valid) ? c->after->tile_ev.h : nullptr;
        ac.done_ev = off + chunk >= nseg ? c->tile_ev.h : nullptr;
        ac.user_start = off == 0 ? c->user_ev[0] : nullptr;
        ac.user_end = off + chunk >= nseg ? c->user_ev[1] : nullptr;
        ac.nseg = std::min(chunk, nseg - off);
        ac.seg = seg.slice(off);
        if (seg_index)
            ac.seg_index = seg_index + off;  // outputs are addressed through the index
        else
            ac.out = out.slice(off);
        HIPCHK(c, launch_gather_tile(ac, c->counters, c->stream));
        c->pktrec_nseg = ac.nseg;  // what the packet records hold now (bre_device_check kind 15)
    }
    c->tile_ev_valid = true;
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
    return read_counters(c, a.ctr);
}

// n device segments against the beam set in the production order: the segments only add into
// their pixels, so the packet kernel takes them in a coherence order (bre_sort.hip; kernels 0 / 4);
// per-segment outputs (optional) are scattered back to the caller's order.  Under
// BRE_OPT_SHARD_MODE 1 with a shard count > 1 only this shard's packets of that order are gathered
// (bre_shard_segments): the other entries of the per-segment outputs are zeroed, and the shards'
// films and outputs sum to the one-shard results.  Used by bre_gather_camera (the camera pass's
// segments), bre_gather_device and bre_gather (the caller's segments).
bre_status gather_segments_core(bre_ctx *c, int64_t n, const SegView &seg, float R, int64_t npix,
                                const GatherOut &out) {
    const bool pshard = c->shard_mode == 1 && c->shard_count > 1;
    const bool sortable = c->kernel == 0 || c->kernel == 4;  // kernels 2 / 5 write in the caller's order
    const bool seg_out = out.seg_rgb || out.seg_counts;
    if (n < 0 || npix < 0) return fail(c, BRE_ERR_INVALID_ARG, "bre_gather: negative size");
    if (n > 0 && (!seg.o || !seg.p || !seg.d || !seg.t))
        return fail(c, BRE_ERR_INVALID_ARG, "bre_gather: null segment array");
    if (out.accum && !seg.pix) return fail(c, BRE_ERR_INVALID_ARG, "bre_gather: accum_rgb given without seg_pixel");
    if (pshard && seg_out) {
        if (!sortable) return fail(c, BRE_ERR_STATE, "packet shards with per-segment outputs need kernel 0 or 4");
        // every entry is defined: the other shards' segments read 0 here
        GatherArgs z{};
        z.nseg = n;
        z.out = out;
        HIPCHK(c, launch_zero_outputs(z, c->stream));
    }
    // packet sharding: this shard gathers the chunks c = rank (mod count) of BRE_OPT_SHARD_BLOCK
    // consecutive 64-segment packets of the (sorted) order, copied into contiguous arrays first
    const auto pick = [&](const SegView &from, const int32_t *index) -> bre_status {
        const int64_t m = bre_shard_segments(n, c->shard_rank, c->shard_count, c->shard_block);
        c->stats.n_segments = m;
        if (m == 0) return BRE_OK;
        SegArrays &sp = c->sp;
        int32_t *sp_index = nullptr;
        HIPCHK(c, sp.ensure((size_t)m));
        if (seg_out) HIPCHK(c, c->sp_index.get((size_t)m, &sp_index));
        const PacketPick pk{n, m, c->shard_rank, c->shard_count, c->shard_block, from, index, sp.out(), sp_index};
        HIPCHK(c, launch_packet_pick(pk, c->stream));
        SegView picked = sp.view();
        if (!from.pix) picked.pix = nullptr;
        return gather_device(c, m, picked, R, npix, out, sp_index);
    };
    if (!c->sort_segments || n < 2 || (!sortable && seg_out)) {
        if (pshard) return pick(seg, nullptr);
        return gather_device(c, n, seg, R, npix, out);
    }
    const size_t N = (size_t)n;
    SegSort ss{n, seg};
    HIPCHK(c, c->ss_bounds.get(8, &ss.bounds));
    ss.tmp_bytes = seg_sort_temp_bytes(n);
    HIPCHK(c, c->ss_sort.reserve(N, 8, ss.tmp_bytes + 16));
    ss.keys = c->ss_sort.keys.as<unsigned long long>();
    ss.keys_alt = c->ss_sort.keys_alt.as<unsigned long long>();
    ss.vals = c->ss_sort.vals;
    ss.vals_alt = c->ss_sort.vals_alt;
    ss.tmp = c->ss_sort.tmp.ptr;
    HIPCHK(c, c->ss.ensure(N));
    ss.out = c->ss.out();
    ss.key_mode = c->sort_key;
    ss.slot = c->slot_passes;
    ss.key_lo = c->coarse_keys ? 12 : 0;
    HIPCHK(c, launch_sort_segments(ss, c->stream));
    // ss.vals_alt[i] = the caller's index of sorted segment i (the sort's permutation)
    SegView sorted = ss.out;
    if (pshard) return pick(sorted, ss.vals_alt);
    if (!seg.pix) sorted.pix = nullptr;
    return gather_device(c, n, sorted, R, npix, out, seg_out ? ss.vals_alt : nullptr);
}

// A gather of n caller-order segments.  With a film (d_accum) the production kernels (0 / 4) add to it
// deterministically: the per-segment sums go to a buffer in the caller's order (the caller's d_seg_rgb
// or an internal one; under packet shards the other shards' entries are 0), then launch_pixel_compose
// adds each pixel's segments in the caller's order -- for the camera pass, the path depths in order,
// as the reference's pixel.Ld += does (photonbeam.cpp:477-504) -- with one thread per pixel and no
// float atomics, so the film is the same bits on every run.  Kernels 2 and 5 (cross-checks) add by
// float atomics.
bre_status gather_segments(bre_ctx *c, int64_t n, const SegView &seg, float R, int64_t npix, const GatherOut &out) {
    const bool sortable = c->kernel == 0 || c->kernel == 4;
    float *const d_accum = out.accum;
    if (c->film_classes > 1 && d_accum && (!sortable || !c->film_compose))
        return fail(c, BRE_ERR_STATE, "BRE_OPT_FILM_CLASSES needs the deterministic compose of kernels 0 / 4");
    // work-root shards gather every segment against a subset of the subtrees: each rank's sums are partial in
    // every class plane, so per-rank planes cannot be gathered plane by plane (dist.ShardedFrame refuses it too)
    if (c->film_classes > 1 && d_accum && c->shard_mode == 2 && c->shard_count > 1)
        return fail(c, BRE_ERR_STATE, "BRE_OPT_FILM_CLASSES needs packet shards (BRE_OPT_SHARD_MODE 1), not work-root shards");
    if (c->film_classes > 1 && d_accum && (uint64_t)BRE_FILM_CLASSES * (uint64_t)(npix + 1) > 0xffffffffull)
        return fail(c, BRE_ERR_INVALID_ARG, "BRE_OPT_FILM_CLASSES: the film is too large for the class keys");
    if (!d_accum || !sortable || n <= 0 || !seg.pix || c->nvalid == 0 || !c->film_compose)
        return gather_segments_core(c, n, seg, R, npix, out);
    const size_t N = (size_t)n;
    float *segbuf = out.seg_rgb;
    if (!segbuf) HIPCHK(c, c->px_seg.get(N * 3, &segbuf));
    BRE_TRY(gather_segments_core(c, n, seg, R, npix, GatherOut{nullptr, segbuf, out.seg_counts}));
    PixelCompose pc{n, seg.pix, segbuf, npix, d_accum, nullptr, c->film_classes};
    pc.tmp_bytes = pixel_sort_temp_bytes(n);
    HIPCHK(c, c->px_sort.reserve(N, 4, pc.tmp_bytes + 16));
    pc.keys = c->px_sort.keys.as<unsigned int>();
    pc.keys_alt = c->px_sort.keys_alt.as<unsigned int>();
    pc.vals = c->px_sort.vals;
    pc.vals_alt = c->px_sort.vals_alt;
    pc.tmp = c->px_sort.tmp.ptr;
    // the flags word of the counter block (a packet shard with no segments never reached the gather's
    // counters_block, so make sure it exists)
    if (!c->counters_buf.ptr) {
        DevCounters *fresh = nullptr;
        BRE_TRY(counters_block(c, &fresh));
    }
    pc.flags = &c->counters_buf.as<DevCounters>()->flags;
    pc.bad_pixel_flag = kFlagPixel;
    pc.slot = c->slot_passes;
    if (c->film_classes > 1) {
        // each segment's class: its packet chunk in the order the gather used (sorted when sorting is on)
        uint8_t *cls = nullptr;
        HIPCHK(c, c->px_cls.get(N, &cls));
        const bool sorted = c->sort_segments && n >= 2;
        HIPCHK(c, launch_seg_classes(n, c->shard_block, c->film_classes,
                                     sorted ? c->ss_sort.vals_alt.as<int32_t>() : nullptr, cls, c->stream));
        pc.cls = cls;
    }
    HIPCHK(c, launch_pixel_compose(pc, c->stream));
    return BRE_OK;
}

// The camera segments of the last camera pass against the beam set (gather_segments).
bre_status gather_camera(bre_ctx *c, float R, const GatherOut &out) {
    if (c->cam_npix == 0) return fail(c, BRE_ERR_STATE, "bre_gather_camera: no camera pass yet");
    BRE_TRY(set_device(c));
    return gather_segments(c, c->cam_nseg, c->seg.view(), R, c->cam_npix, out);
}

}  // namespace

namespace bre {

bre_status gather_host(bre_ctx *c, int64_t nseg, const SegView &seg, float R, int64_t npix, const GatherOut &out,
                       bool film_stays) {
    if (!c) return BRE_ERR_INVALID_ARG;
    const int32_t *const pixel = seg.pix;
    float *const accum = out.accum, *const seg_rgb = out.seg_rgb;
    int32_t *const seg_counts = out.seg_counts;
    if (nseg < 0 || npix < 0) return fail(c, BRE_ERR_INVALID_ARG, "bre_gather: negative size");
    if (c->film_classes > 1 && accum)
        return fail(c, BRE_ERR_STATE, "bre_gather: BRE_OPT_FILM_CLASSES is for caller device films (bre_gather_device)");
    if (nseg > 0 && (!seg.o || !seg.p || !seg.d || !seg.t))
        return fail(c, BRE_ERR_INVALID_ARG, "bre_gather: null segment array");
    if (accum && !pixel) return fail(c, BRE_ERR_INVALID_ARG, "bre_gather: accum_rgb given without seg_pixel");
    if (accum && pixel) {
        for (int64_t s = 0; s < nseg; ++s)
            if (pixel[s] < 0 || pixel[s] >= npix)
                return fail(c, BRE_ERR_INVALID_ARG, "bre_gather: seg_pixel[%lld]=%d out of [0,%lld)", (long long)s,
                            pixel[s], (long long)npix);
    }
    BRE_TRY(set_device(c));
    const size_t S = (size_t)nseg, P = (size_t)npix;
    if (film_stays && accum && npix > 0) {
        float *film = nullptr;
        HIPCHK(c, c->g_accum.get(P * 3, &film));
        HIPCHK(c, fill_words(c, film, P * 3 * sizeof(float)));
    }
    if (nseg == 0) {
        // nothing to copy or launch, but the stats describe this gather, not the one before it
        // (bre_gather_device with no segments reports the same through gather_device)
        c->stats.n_segments = 0;
        if (c->counters) {
            c->stats.candidates = c->stats.contributions = 0;
            c->stats.node_visits = c->stats.leaf_visits = c->stats.beam_evals = 0;
            c->stats.ccp_wave_evals = c->stats.prefilter_rejects = c->stats.useful_beam_evals = 0;
            c->stats.max_stack_depth = c->stats.queued_pairs = 0;
        }
        return BRE_OK;
    }
    SegArrays &g = c->g;
    HIPCHK(c, g.ensure(S, pixel != nullptr));
    HIPCHK(c, g.upload(S, seg.o, seg.p, seg.d, seg.t, pixel, c->stream));
    float *daccum = nullptr, *dseg = nullptr;
    int32_t *dcnt = nullptr;
    if (accum && npix > 0) {
        HIPCHK(c, c->g_accum.get(P * 3, &daccum));
        if (!film_stays)
            HIPCHK(c, hipMemcpyAsync(daccum, accum, P * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    if (seg_rgb) HIPCHK(c, c->g_seg_rgb.get(S * 3, &dseg));
    if (seg_counts) HIPCHK(c, c->g_counts.get(S * 2, &dcnt));
    SegView staged = g.view();
    if (!pixel) staged.pix = nullptr;
    BRE_TRY(gather_segments(c, nseg, staged, R, npix, GatherOut{daccum, dseg, dcnt}));
    if (daccum && !film_stays) HIPCHK(c, hipMemcpyAsync(accum, daccum, P * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (dseg) HIPCHK(c, hipMemcpyAsync(seg_rgb, dseg, S * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (dcnt) HIPCHK(c, hipMemcpyAsync(seg_counts, dcnt, S * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    return check_flags(c);
}

}  // namespace bre

extern "C" {

bre_status bre_gather_camera(bre_ctx *c, float R, float *d_accum) {
    if (!c) return BRE_ERR_INVALID_ARG;
    return gather_camera(c, R, GatherOut{d_accum, nullptr, nullptr});
}

bre_status bre_gather_camera_segments(bre_ctx *c, float R, float *d_accum, float *d_seg_rgb, int32_t *d_seg_counts) {
    if (!c) return BRE_ERR_INVALID_ARG;
    return gather_camera(c, R, GatherOut{d_accum, d_seg_rgb, d_seg_counts});
}

bre_status bre_gather_device(bre_ctx *c, int64_t nseg, const float *o, const float *p, const float *d,
                             const float *tmax, const int32_t *pixel, float R, int64_t npix, float *accum,
                             float *seg_rgb, int32_t *seg_counts) {
    if (!c) return BRE_ERR_INVALID_ARG;
    BRE_TRY(set_device(c));
    return gather_segments(c, nseg, SegView{o, p, d, tmax, pixel}, R, npix, GatherOut{accum, seg_rgb, seg_counts});
}

bre_status bre_gather(bre_ctx *c, int64_t nseg, const float *o, const float *p, const float *d, const float *tmax,
                      const int32_t *pixel, float R, int64_t npix, float *accum, float *seg_rgb,
                      int32_t *seg_counts) {
    return gather_host(c, nseg, SegView{o, p, d, tmax, pixel}, R, npix, GatherOut{accum, seg_rgb, seg_counts},
                       false);
}

bre_status bre_film_add(bre_ctx *c, int64_t n_floats, float *d_src, float *d_dst, int32_t clear_src) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (n_floats < 0 || (n_floats > 0 && (!d_src || !d_dst)) || d_src == d_dst)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_film_add: bad films");
    BRE_TRY(set_device(c));
    HIPCHK(c, launch_film_add(n_floats, d_src, d_dst, clear_src != 0, c->stream));
    return BRE_OK;
}

bre_status bre_resolve_classes(bre_ctx *c, int64_t npix, const float *d_classes, float *d_out) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (npix < 0 || (npix > 0 && (!d_classes || !d_out))) return fail(c, BRE_ERR_INVALID_ARG, "bre_resolve_classes: bad film");
    BRE_TRY(set_device(c));
    HIPCHK(c, launch_resolve_classes(3 * npix, BRE_FILM_CLASSES, d_classes, d_out, c->stream));
    return BRE_OK;
}

}  // extern "C"
