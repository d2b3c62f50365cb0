// bre_api_check.hip — bre_device_check, the test hooks of the C ABI: device functions, the pass
// chain's one-wave primitives and the hierarchy kernels on caller data, and the read-back of the
// context's current build.
#include <cmath>
#include <cstring>
#include <vector>

#include "bre_ctx.h"

using namespace bre;

namespace {

// bre_device_check kind 10: the hierarchy kernels (k_karras and k_refit, or k_single; then k_collapse4) on
// the caller's sorted keys and member boxes, through the production launchers and their capacity checks,
// in the check's own buffers (the context's current build is not touched).  x: m keys (2 words each), then
// m boxes (lo xyz, hi xyz); y: the Node records, the leaf_parent words, the Node4 records.
bre_status check_hierarchy(bre_ctx *c, int64_t n, const float *x, int32_t n_aux, const float *aux, float *y) {
    if (n_aux < 2 || !aux) return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 10 needs aux = (key_lo, leaf_size)");
    const int key_lo = (int)aux[0], K = (int)aux[1];
    if (n < 8 || n % 8 || !x || !y || key_lo < 0 || key_lo > 63 || K < 1 || K > 64 || n / 8 > ((int64_t)1 << 24))
        return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 10 needs m <= 2^24 keys and boxes (8 words each), "
                    "key_lo in 0..63 and leaf_size in 1..64");
    const int64_t m = n / 8;
    std::vector<unsigned long long> keys((size_t)m);
    std::memcpy(keys.data(), x, (size_t)m * 8);
    // the hierarchy is only ever launched on the order its sort left: a non-monotone sequence is refused here
    for (int64_t i = 1; i < m; ++i)
        if ((keys[(size_t)i] >> key_lo) < (keys[(size_t)i - 1] >> key_lo))
            return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 10 keys >> %d decrease at %lld: the hierarchy "
                        "kernels need a non-decreasing sequence", key_lo, (long long)i);
    std::vector<BeamRec> recs((size_t)m);  // zeroed; only lo / hi are read
    const float *bx = x + 2 * m;
    for (int64_t i = 0; i < m; ++i)
        for (int k = 0; k < 3; ++k) {
            recs[(size_t)i].lo[k] = bx[6 * i + k];
            recs[(size_t)i].hi[k] = bx[6 * i + 3 + k];
        }
    const int64_t nleaf = (m + K - 1) / K;
    const int64_t nnodes = nleaf > 1 ? nleaf - 1 : 1;
    BRE_TRY(set_device(c));
    const size_t recs_off = ((size_t)m * 8 + 63) / 64 * 64;
    const size_t n4_off = (size_t)nnodes * sizeof(Node), lp_off = n4_off + (size_t)nnodes * sizeof(Node4);
    HIPCHK(c, c->chk_x.ensure(recs_off + (size_t)m * sizeof(BeamRec)));
    HIPCHK(c, c->chk_y.ensure(lp_off + (size_t)nleaf * sizeof(int32_t)));
    HIPCHK(c, c->chk_aux.ensure((size_t)nnodes * sizeof(unsigned int)));
    char *dx = static_cast<char *>(c->chk_x.ptr), *dy = static_cast<char *>(c->chk_y.ptr);
    BuildBuffers b{};
    b.n = m;
    b.leaf_size = K;
    b.key_lo = key_lo;
    b.slot = c->slot_passes;
    b.keys_alt = reinterpret_cast<unsigned long long *>(dx);
    b.recs = reinterpret_cast<BeamRec *>(dx + recs_off);
    b.nodes = reinterpret_cast<Node *>(dy);
    b.leaf_parent = reinterpret_cast<int32_t *>(dy + lp_off);
    b.visit = c->chk_aux.as<unsigned int>();
    b.nodes_cap = (uint64_t)nnodes;  // exactly what is read back below
    b.leaf_parent_cap = (uint64_t)nleaf;
    b.visit_cap = (uint64_t)nnodes;
    Node4 *d4 = reinterpret_cast<Node4 *>(dy + n4_off);
    HIPCHK(c, hipMemcpyAsync(b.keys_alt, keys.data(), (size_t)m * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.recs, recs.data(), (size_t)m * sizeof(BeamRec), hipMemcpyHostToDevice, c->stream));
    // a single leaf has no leaf_parent word (k_single writes none): 0, the root
    HIPCHK(c, hipMemsetAsync(b.leaf_parent, 0, (size_t)nleaf * sizeof(int32_t), c->stream));
    HIPCHK(c, launch_hierarchy(b, m, c->stream));
    HIPCHK(c, launch_collapse4(b.nodes, nnodes, d4, c->stream));
    char *hy = reinterpret_cast<char *>(y);
    HIPCHK(c, hipMemcpyAsync(hy, b.nodes, (size_t)nnodes * sizeof(Node), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hy + n4_off, b.leaf_parent, (size_t)nleaf * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hy + n4_off + (size_t)nleaf * 4, d4, (size_t)nnodes * sizeof(Node4), hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BRE_OK;
}

// bre_device_check kind 11: the context's current build read back (layout: include/bre.h); n = the words y holds
bre_status check_read_tree(bre_ctx *c, int64_t n, float *y) {
    if (!y || n < 8) return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 11 needs y of at least 8 words");
    if (c->nvalid > 0 && !c->build_scratch_ok)
        return fail(c, BRE_ERR_STATE, "bre_device_check: kind 11 reads a build after bre_set_beams* and before a "
                    "kernel-5 gather has reused its sort buffers");
    const int64_t nv = c->nvalid, nn = nv > 0 ? c->nnodes : 0;
    const int K = c->built_leaf_size;
    const int64_t nleaf = nv > 0 ? (nv + K - 1) / K : 0;
    const bool has4 = nv > 0 && c->nodes4_ok;
    const int64_t need = 8 + 9 * nv + 16 * nn + nleaf + (has4 ? 32 * nn : 0);
    if (n < need)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 11: y holds %lld words, the build needs %lld",
                    (long long)n, (long long)need);
    int32_t head[8] = {0, 0, K, c->built_key_lo, (int32_t)nn, has4 ? 1 : 0, (int32_t)nleaf, 0};
    std::memcpy(head, &nv, sizeof(int64_t));
    std::memcpy(y, head, sizeof(head));
    if (nv == 0) return BRE_OK;
    BRE_TRY(set_device(c));
    float *keys = y + 8, *idx = keys + 2 * nv, *box = idx + nv, *nodes = box + 6 * nv, *lp = nodes + 16 * nn,
          *nodes4 = lp + nleaf;
    std::vector<BeamRec> recs((size_t)nv);
    HIPCHK(c, hipMemcpyAsync(keys, c->sort.keys_alt.ptr, (size_t)nv * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(idx, c->sort.vals_alt.ptr, (size_t)nv * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(recs.data(), c->recs.ptr, (size_t)nv * sizeof(BeamRec), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(nodes, c->nodes.ptr, (size_t)nn * sizeof(Node), hipMemcpyDeviceToHost, c->stream));
    if (nleaf > 1)
        HIPCHK(c, hipMemcpyAsync(lp, c->leaf_parent.ptr, (size_t)nleaf * 4, hipMemcpyDeviceToHost, c->stream));
    if (has4)
        HIPCHK(c, hipMemcpyAsync(nodes4, c->nodes4.ptr, (size_t)nn * sizeof(Node4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nleaf == 1) std::memset(lp, 0, 4);  // k_single writes no leaf_parent word: 0, the root
    for (int64_t i = 0; i < nv; ++i)
        for (int k = 0; k < 3; ++k) {
            box[6 * i + k] = recs[(size_t)i].lo[k];
            box[6 * i + 3 + k] = recs[(size_t)i].hi[k];
        }
    return BRE_OK;
}

}  // namespace

extern "C" {

bre_status bre_device_check(bre_ctx *c, int32_t kind, int64_t n, const float *x, int32_t n_aux, const float *aux,
                            float *y) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (kind < 0 || kind > 15) return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind %d not in [0, 15]", kind);
    if (kind == 10) return check_hierarchy(c, n, x, n_aux, aux, y);
    if (kind == 11) return check_read_tree(c, n, y);
    if (n < 0 || (n > 0 && (!x || !y))) return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: bad arrays");
    if (kind == 15) {
        // the packet records of the context's last tile launch (PacketRec, bre_packet.h) against the bundle and
        // margin formed again from that launch's segments: x = n / 10 segments in the GATHERED order, 10 floats
        // each (o, p, d, tmax); y[0] = the record words that differ, y[1] = the packets compared
        if (n % 10 || n == 0) return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 15 needs whole segments of 10 floats");
        const int64_t ns = n / 10;
        if (c->pktrec_nseg != ns || !c->pktrec.ptr)
            return fail(c, BRE_ERR_STATE, "bre_device_check: kind 15: the context's last tile launch gathered %lld "
                        "segments, not %lld", (long long)c->pktrec_nseg, (long long)ns);
        BRE_TRY(set_device(c));
        std::vector<float> soa((size_t)n);
        float *ho = soa.data(), *hp = ho + 3 * ns, *hd = hp + 3 * ns, *ht = hd + 3 * ns;
        for (int64_t i = 0; i < ns; ++i) {
            for (int k = 0; k < 3; ++k) {
                ho[3 * i + k] = x[10 * i + k];
                hp[3 * i + k] = x[10 * i + 3 + k];
                hd[3 * i + k] = x[10 * i + 6 + k];
            }
            ht[i] = x[10 * i + 9];
        }
        float *dx = nullptr;
        unsigned int *dy = nullptr;
        HIPCHK(c, c->chk_x.get((size_t)n, &dx));
        HIPCHK(c, c->chk_y.get((size_t)1, &dy));
        HIPCHK(c, hipMemcpyAsync(dx, soa.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(dy, 0, 4, c->stream));
        const SegView sv{dx, dx + 3 * ns, dx + 6 * ns, dx + 9 * ns, nullptr};
        HIPCHK(c, launch_packet_check(ns, sv, c->pktrec.as<PacketRec>(), dy, c->stream));
        unsigned int bad = 0;
        HIPCHK(c, hipMemcpyAsync(&bad, dy, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        y[0] = (float)bad;
        y[1] = (float)packet_count(ns);
        return BRE_OK;
    }
    if (kind == 12) {
        // the specular lobe of the photon and camera passes on records of 6 floats (layout: include/bre.h)
        if (n % 6) return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 12 needs whole records of 6 floats");
        if (n == 0) return BRE_OK;
        BRE_TRY(set_device(c));
        float *dx = nullptr, *dy = nullptr;
        HIPCHK(c, c->chk_x.get((size_t)n, &dx));
        HIPCHK(c, c->chk_y.get((size_t)n, &dy));
        HIPCHK(c, hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_check_specular(n / 6, dx, dy, c->stream));
        HIPCHK(c, hipMemcpyAsync(y, dy, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BRE_OK;
    }
    if (kind == 13) {
        // the general BSDF of the photon and camera passes: records of 9 floats against a table of
        // bre_material_ex records in aux (layout: include/bre.h)
        constexpr int kWords = (int)(sizeof(bre_material_ex) / 4);
        if (n % 9 || n_aux < kWords || n_aux % kWords || !aux)
            return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 13 needs whole records of 9 floats and, in aux, "
                        "whole bre_material_ex records of %d words", kWords);
        const int n_mats = n_aux / kWords;
        std::vector<bre_material_ex> mats((size_t)n_mats);
        std::memcpy(mats.data(), aux, (size_t)n_aux * 4);
        std::vector<DevBsdf> table((size_t)n_mats);
        for (int k = 0; k < n_mats; ++k) {
            const std::string what = check_glossy_material(mats[(size_t)k]);
            if (!what.empty())
                return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 13: material %d has %s", k, what.c_str());
            table[(size_t)k] = make_bsdf(mats[(size_t)k]);
        }
        for (int64_t i = 0; i < n / 9; ++i)
            if (!(x[9 * i + 8] >= 0 && x[9 * i + 8] < (float)n_mats) || x[9 * i + 8] != std::floor(x[9 * i + 8]))
                return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 13: record %lld names material %g of %d",
                            (long long)i, (double)x[9 * i + 8], n_mats);
        if (n == 0) return BRE_OK;
        BRE_TRY(set_device(c));
        float *dx = nullptr, *dy = nullptr;
        DevBsdf *dt = nullptr;
        const size_t outs = (size_t)(n / 9) * 12;
        HIPCHK(c, c->chk_x.get((size_t)n, &dx));
        HIPCHK(c, c->chk_y.get(outs, &dy));
        HIPCHK(c, c->chk_aux.get((size_t)n_mats, &dt));
        HIPCHK(c, hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(dt, table.data(), table.size() * sizeof(DevBsdf), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_check_bsdf(n / 9, dx, dt, n_mats, dy, c->stream));
        HIPCHK(c, hipMemcpyAsync(y, dy, outs * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BRE_OK;
    }
    if (kind == 14) {
        // the BSDF of any number of lobes: kind 13's records with a transport mode and a flag set, against a table
        // of bre_material_ex records of types 4 .. 6 and 8 .. 11 (layout: include/bre.h)
        constexpr int kWords = (int)(sizeof(bre_material_ex) / 4), kRec = 11;
        if (n % kRec || n_aux < kWords || n_aux % kWords || !aux)
            return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 14 needs whole records of %d floats and, in aux, "
                        "whole bre_material_ex records of %d words", kRec, kWords);
        const int n_mats = n_aux / kWords;
        std::vector<bre_material_ex> mats((size_t)n_mats);
        std::memcpy(mats.data(), aux, (size_t)n_aux * 4);
        bool mixed = false;
        for (int k = 0; k < n_mats; ++k) mixed = mixed || mats[(size_t)k].type == BRE_MATERIAL_MIX;
        if (mixed) {
            // a table that holds a mix: checked as bre_set_materials_ex checks it (mirror and glass children and the
            // rules between records included) and evaluated through the wide lists of a mixed context
            int bad = 0;
            const std::string what = check_material_table(mats, &bad);
            if (!what.empty())
                return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 14: material %d has %s", bad, what.c_str());
            std::vector<DevLobesMx> wide;
            make_lobes_mx(mats.data(), n_mats, &wide);
            for (int64_t i = 0; i < n / kRec; ++i) {
                const float *r = x + kRec * i;
                if (!(r[8] >= 0 && r[8] < (float)n_mats) || r[8] != std::floor(r[8]))
                    return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 14: record %lld names material %g of %d",
                                (long long)i, (double)r[8], n_mats);
                if (mats[(size_t)r[8]].type < BRE_MATERIAL_MATTE)
                    return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 14: record %lld names material %d, a "
                                "mirror or glass: it is evaluated only as a mix's child", (long long)i, (int)r[8]);
                if ((r[9] != 0.f && r[9] != 1.f) || (r[10] != 0.f && r[10] != 1.f))
                    return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 14: record %lld has a mode or a flag "
                                "set that is not 0 or 1", (long long)i);
            }
            if (n == 0) return BRE_OK;
            BRE_TRY(set_device(c));
            float *dx = nullptr, *dy = nullptr;
            DevLobesMx *dt = nullptr;
            const size_t outs = (size_t)(n / kRec) * 12;
            HIPCHK(c, c->chk_x.get((size_t)n, &dx));
            HIPCHK(c, c->chk_y.get(outs, &dy));
            HIPCHK(c, c->chk_aux.get((size_t)n_mats, &dt));
            HIPCHK(c, hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(dt, wide.data(), wide.size() * sizeof(DevLobesMx), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, launch_check_lobes_mx(n / kRec, dx, dt, n_mats, dy, c->stream));
            HIPCHK(c, hipMemcpyAsync(y, dy, outs * 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            return BRE_OK;
        }
        std::vector<DevLobes> table((size_t)n_mats);
        for (int k = 0; k < n_mats; ++k) {
            const std::string what = check_lobed_or_glossy_material(mats[(size_t)k]);
            if (!what.empty())
                return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 14: material %d has %s", k, what.c_str());
            table[(size_t)k] = make_lobes(mats[(size_t)k]);
        }
        for (int64_t i = 0; i < n / kRec; ++i) {
            const float *r = x + kRec * i;
            if (!(r[8] >= 0 && r[8] < (float)n_mats) || r[8] != std::floor(r[8]))
                return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 14: record %lld names material %g of %d",
                            (long long)i, (double)r[8], n_mats);
            if ((r[9] != 0.f && r[9] != 1.f) || (r[10] != 0.f && r[10] != 1.f))
                return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 14: record %lld has a mode or a flag set "
                            "that is not 0 or 1", (long long)i);
        }
        if (n == 0) return BRE_OK;
        BRE_TRY(set_device(c));
        float *dx = nullptr, *dy = nullptr;
        DevLobes *dt = nullptr;
        const size_t outs = (size_t)(n / kRec) * 12;
        HIPCHK(c, c->chk_x.get((size_t)n, &dx));
        HIPCHK(c, c->chk_y.get(outs, &dy));
        HIPCHK(c, c->chk_aux.get((size_t)n_mats, &dt));
        HIPCHK(c, hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(dt, table.data(), table.size() * sizeof(DevLobes), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_check_lobes(n / kRec, dx, dt, n_mats, dy, c->stream));
        HIPCHK(c, hipMemcpyAsync(y, dy, outs * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BRE_OK;
    }
    if (kind >= 6 && kind <= 8) {
        // the pass chain's one-wave primitives (bre_slot.hip) on caller data
        BRE_TRY(set_device(c));
        if (n == 0) return BRE_OK;
        if (kind == 7) {  // exclusive scan of n int32 words; y: n + 1 int64 (the total last)
            int32_t *dx = nullptr;
            int64_t *dy = nullptr;
            HIPCHK(c, c->chk_x.get((size_t)n, &dx));
            HIPCHK(c, c->chk_y.get((size_t)(n + 1), &dy));
            HIPCHK(c, c->chk_aux.ensure(slot_scan_temp_bytes(n)));
            HIPCHK(c, hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, slot_exclusive_scan(dx, dy, n, dy + n, c->chk_aux.ptr, c->stream));
            HIPCHK(c, hipMemcpyAsync(y, dy, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            return BRE_OK;
        }
        // kind 6 / 8: stable sort of m = n / 2 64-bit (n 32-bit) keys by bits [aux[0], aux[1]), values = the
        // input positions; y: the sorted keys, then the values
        if (n_aux < 2 || !aux) return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kinds 6 / 8 need aux[0..1] bits");
        const int kb = kind == 6 ? 8 : 4;
        if ((n * 4) % kb) return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 6 needs an even word count");
        const int64_t m = n * 4 / kb;
        const size_t tb = slot_sort_temp_bytes(m, kb);
        HIPCHK(c, c->chk_x.ensure((size_t)m * (kb + 4) * 2 + tb + 512));
        char *base = static_cast<char *>(c->chk_x.ptr);
        char *k0 = base, *k1 = k0 + (size_t)m * kb, *v0 = k1 + (size_t)m * kb, *v1 = v0 + (size_t)m * 4;
        void *tmp = v1 + ((size_t)m * 4 + 256) / 256 * 256;
        std::vector<int32_t> idx((size_t)m);
        for (int64_t i = 0; i < m; ++i) idx[(size_t)i] = (int32_t)i;
        HIPCHK(c, hipMemcpyAsync(k0, x, (size_t)m * kb, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(v0, idx.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
        const int b0 = (int)aux[0], b1 = (int)aux[1];
        if (kb == 8)
            HIPCHK(c, slot_sort_pairs(tmp, reinterpret_cast<unsigned long long *>(k0), reinterpret_cast<unsigned long long *>(k1),
                                      reinterpret_cast<int32_t *>(v0), reinterpret_cast<int32_t *>(v1), m, b0, b1, c->stream));
        else
            HIPCHK(c, slot_sort_pairs(tmp, reinterpret_cast<unsigned int *>(k0), reinterpret_cast<unsigned int *>(k1),
                                      reinterpret_cast<int32_t *>(v0), reinterpret_cast<int32_t *>(v1), m, b0, b1, c->stream));
        HIPCHK(c, hipMemcpyAsync(y, k1, (size_t)m * kb, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(reinterpret_cast<char *>(y) + (size_t)m * kb, v1, (size_t)m * 4, hipMemcpyDeviceToHost,
                                 c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BRE_OK;
    }
    if (kind == 5) {
        // the tile kernel's work roots (k_roots) of a caller tree: x = n / 16 Node records as words
        if (n_aux < 1 || !aux) return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 5 needs aux[0] = S");
        const int S = (int)aux[0];
        if (n < 16 || n % 16 || S < 1 || S > kMaxSplit || (S & (S - 1)))
            return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind 5 needs whole Node records and S a power of two <= %d",
                        kMaxSplit);
        BRE_TRY(set_device(c));
        Node *dx = nullptr;
        int32_t *dy = nullptr;
        HIPCHK(c, c->chk_x.get((size_t)n / 16, &dx));
        HIPCHK(c, c->chk_y.get((size_t)(S + 1), &dy));
        HIPCHK(c, hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, c->roots_tmp.ensure(roots_scratch_bytes()));
        HIPCHK(c, launch_roots(dx, S, dy, c->roots_tmp.ptr, c->stream));
        HIPCHK(c, hipMemcpyAsync(y, dy, (size_t)(S + 1) * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return BRE_OK;
    }
    const bool need_aux = kind == 3 || kind == 4;
    if (need_aux && (n_aux < 1 || !aux)) return fail(c, BRE_ERR_INVALID_ARG, "bre_device_check: kind %d needs aux", kind);
    if (n == 0) return BRE_OK;
    BRE_TRY(set_device(c));
    const int64_t outs = kind == 9 ? 4 * n : (kind == 2 || kind == 4) ? 2 * n : n;
    float *dx = nullptr, *dy = nullptr, *daux = nullptr;
    HIPCHK(c, c->chk_x.get((size_t)n, &dx));
    HIPCHK(c, c->chk_y.get((size_t)outs, &dy));
    HIPCHK(c, c->chk_aux.get(need_aux ? (size_t)n_aux : 1, &daux));
    HIPCHK(c, hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    if (need_aux) HIPCHK(c, hipMemcpyAsync(daux, aux, (size_t)n_aux * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_device_check(kind, n, dx, need_aux ? n_aux : 0, daux, dy, c->stream));
    HIPCHK(c, hipMemcpyAsync(y, dy, (size_t)outs * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BRE_OK;
}

}  // extern "C"
