// bre_api_build.hip — the beam build behind the C ABI: the BVH of a beam set from device arrays, and
// the entry points that set the beams from host or device arrays or read them back.
#include <cstring>

#include "bre_ctx.h"

namespace bre {

// Build the BVH from device arrays (start/end/radius/power) of n beams.
bre_status build(bre_ctx *c, int64_t n, const BeamView &in) {
    c->nbeams = n;
    c->nvalid = 0;
    c->bset = BeamSet{};
    c->nnodes = 0;
    c->roots_split = -1;
    c->nodes4_ok = false;
    c->build_scratch_ok = false;
    c->built_key_lo = 0;
    c->stats = bre_stats{};
    c->stats.n_beams = n;
    if (n == 0) return BRE_OK;
    if (n > (int64_t)INT32_MAX / 2)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_set_beams: %lld beams exceeds the 2^30 limit of this build",
                    (long long)n);
    const size_t N = (size_t)n;
    BuildBuffers b;
    b.in = in;
    b.n = n;
    b.sqrt_mode = c->sqrt_mode;
    b.slot = c->slot_passes;
    b.leaf_size = c->leaf_size;
    b.beam_key = c->beam_key;
    HIPCHK(c, c->box.get(N * 6, &b.box));
    HIPCHK(c, c->cent.get(N * 3, &b.cent));
    HIPCHK(c, c->cbounds.get(12, &b.cbounds));
    HIPCHK(c, c->nvalid_buf.get(3, &b.nvalid));
    HIPCHK(c, c->sort.reserve(N, 8, sort_temp_bytes(n)));
    b.keys = c->sort.keys.as<unsigned long long>();
    b.keys_alt = c->sort.keys_alt.as<unsigned long long>();
    b.vals = c->sort.vals;
    b.vals_alt = c->sort.vals_alt;
    b.sort_tmp = c->sort.tmp.ptr;
    b.sort_tmp_bytes = c->sort.tmp.cap;
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    HIPCHK(c, launch_prep(b, c->stream));
    // tree keys 1 / 2 (the tile kernel's tree): the first sort only groups equal centroids (a hash key,
    // bre_build.hip k_cent_hash); otherwise the centroid Morton order is the tree order
    const bool se_tree = c->kernel == 0 && c->beam_key >= 1;
    if (se_tree) {
        HIPCHK(c, launch_cent_hash(b, c->stream));
        HIPCHK(c, launch_sort(b, c->stream, 32));
    } else {
        HIPCHK(c, launch_morton(b, c->stream));
        HIPCHK(c, launch_sort(b, c->stream));
    }
    unsigned int nv[3] = {0u, 0u, 0u};  // valid beams, min / max of their radius bits (k_prep)
    BRE_TRY(read_small(c, {{nv, b.nvalid, sizeof(nv)}}));
    const int64_t nvalid = nv[0];
    c->nvalid = nvalid;
    // one radius for every valid beam: the records carry the power instead (BeamRec, BeamSet)
    c->bset.uniform = (nvalid > 0 && nv[1] == nv[2] && !c->split_records) ? 1 : 0;
    std::memcpy(&c->bset.radius, &nv[1], sizeof(float));
    if (!c->bset.uniform) c->bset.radius = 0.f;
    b.uniform_radius = c->bset.uniform;
    c->stats.n_beams_valid = nvalid;
    if (nvalid == 0) return BRE_OK;
    if (se_tree) {
        // tree order by (start, end): group boxes from the centroid order, then the second sort
        HIPCHK(c, c->gbox.get(N * 6, &b.gbox));
        HIPCHK(c, launch_tree_key(b, nvalid, c->stream));
        b.key_lo = c->coarse_keys ? 16 : 0;  // the hierarchy compares the bits the sort ordered
        HIPCHK(c, launch_sort(b, c->stream, 64, b.key_lo));
    } else {
        b.beam_key = 0;
    }
    // kernel 0 runs the tile kernel on one tree of leaf2-beam tiles; kernels 2 / 4 / 5 on a tree of
    // BRE_OPT_LEAF_SIZE-beam leaves
    const int K = c->kernel == 0 ? c->leaf2 : c->leaf_size;
    b.leaf_size = K;  // the hierarchy kernels size their work by it: must match the buffers below
    const int64_t nleaf = (nvalid + K - 1) / K;
    const int64_t nnodes = nleaf > 1 ? nleaf - 1 : 1;
    HIPCHK(c, c->recs.get((size_t)nvalid, &b.recs));
    HIPCHK(c, c->pow.get((size_t)nvalid, &b.pow));
    HIPCHK(c, c->nodes.get((size_t)nnodes, &b.nodes));
    HIPCHK(c, c->leaf_parent.get((size_t)nleaf, &b.leaf_parent));
    HIPCHK(c, c->visit.get((size_t)nnodes, &b.visit));
    b.nodes_cap = c->nodes.cap / sizeof(Node);
    b.leaf_parent_cap = c->leaf_parent.cap / sizeof(int32_t);
    b.visit_cap = c->visit.cap / sizeof(unsigned int);
    HIPCHK(c, launch_pack(b, nvalid, c->stream));
    HIPCHK(c, launch_hierarchy(b, nvalid, c->stream));
    if (c->timing) {
        HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
        HIPCHK(c, hipEventSynchronize(c->ev[1]));
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        c->stats.build_ms = ms;
    }
    c->nnodes = nnodes;
    c->built_leaf_size = K;
    c->built_key_lo = b.key_lo;
    c->build_scratch_ok = true;
    c->stats.n_nodes = nnodes;
    if (c->kernel == 0 || c->kernel == 4) {
        // the tile kernel's work roots and 4-wide view, here on the build's stream: with two contexts
        // pipelined they overlap the other context's gather instead of preceding this one's
        int32_t *roots = nullptr;
        Node4 *nodes4 = nullptr;
        HIPCHK(c, c->roots.get(kMaxSplit + 1, &roots));
        HIPCHK(c, c->roots_tmp.ensure(roots_scratch_bytes()));
        HIPCHK(c, launch_roots(b.nodes, c->split, roots, c->roots_tmp.ptr, c->stream));
        c->roots_split = c->split;
        HIPCHK(c, c->nodes4.get((size_t)nnodes, &nodes4));
        HIPCHK(c, launch_collapse4(b.nodes, nnodes, nodes4, c->stream));
        c->nodes4_ok = true;
    }
    return BRE_OK;
}

}  // namespace bre

using namespace bre;

extern "C" {

bre_status bre_set_beams(bre_ctx *c, int64_t n, const float *start, const float *end, const float *radius,
                         const float *power) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (n < 0) return fail(c, BRE_ERR_INVALID_ARG, "bre_set_beams: negative count");
    if (n > 0 && (!start || !end || !radius || !power))
        return fail(c, BRE_ERR_INVALID_ARG, "bre_set_beams: null array");
    BRE_TRY(set_device(c));
    if (n > 0) {
        HIPCHK(c, c->in.ensure((size_t)n));
        HIPCHK(c, c->in.upload((size_t)n, start, end, radius, power, c->stream));
    }
    c->beams_kept = false;
    BRE_TRY(build(c, n, c->in.view()));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->beams_kept = true;
    return BRE_OK;
}

bre_status bre_set_beams_device(bre_ctx *c, int64_t n, const float *start, const float *end, const float *radius,
                                const float *power) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (n < 0) return fail(c, BRE_ERR_INVALID_ARG, "bre_set_beams_device: negative count");
    if (n > 0 && (!start || !end || !radius || !power))
        return fail(c, BRE_ERR_INVALID_ARG, "bre_set_beams_device: null array");
    BRE_TRY(set_device(c));
    c->beams_kept = false;
    return build(c, n, BeamView{start, end, radius, power});
}

bre_status bre_get_beams(bre_ctx *c, int64_t capacity, float *start, float *end, float *radius, float *power,
                         int64_t *n_beams) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (capacity < 0) return fail(c, BRE_ERR_INVALID_ARG, "bre_get_beams: negative capacity");
    if (!c->beams_kept && c->nbeams > 0)
        return fail(c, BRE_ERR_STATE, "bre_get_beams: the beam set came from caller device arrays");
    if (n_beams) *n_beams = c->nbeams;
    const int64_t k = capacity < c->nbeams ? capacity : c->nbeams;
    if (k <= 0) return BRE_OK;
    if (!start || !end || !radius || !power) return fail(c, BRE_ERR_INVALID_ARG, "bre_get_beams: null array");
    BRE_TRY(set_device(c));
    HIPCHK(c, c->in.download((size_t)k, start, end, radius, power, c->stream));
    return check_flags(c);
}

}  // extern "C"
