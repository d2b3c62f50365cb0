// bre_thread.hip — kernel 2 (k_gather_thread): the classic thread-per-segment traversal with a
// per-thread LDS stack, a structurally independent implementation of the gather kept as a cross-check
// of the tile kernel (bre_gather.hip).
#include <hip/hip_runtime.h>

#include "bre_device.h"
#include "bre_lane.h"
#include "bre_math.h"

namespace bre {

namespace {

constexpr int kThreadBlock = 128;  // 2 waves, 32 KiB LDS stack

// ---------------------------------------------------------------------------------------------
// Kernel 2 helpers: evaluate one beam record for one lane — reference box test, closest points,
// kernel (photonbeam.cpp:495-507) — and write the lane's results.
template <bool COUNT>
__device__ __forceinline__ void eval_beam(const Lane &L, bool lane_on, const BeamV &r, const float4 *__restrict__ pw,
                                          int64_t bi, float R, float &cr, float &cg, float &cb, int &cand,
                                          int &contrib) {
    // candidate: the reference's own slab test on the beam's (group) box.  For a lane whose 1/d has
    // no infinite component, node_test(box, inv) is the same decision (bre_math.h); lanes with an
    // axis-parallel direction (inf, possible NaN paths) take the literal statement.
    float te;
    bool hit = lane_on & node_test(r.box, L.o, L.invs, L.tmax, te);
    if (L.has_inf) hit = lane_on & slab_test(r.box, L.o, L.inv, L.n0, L.n1, L.n2, L.tmax, nullptr);
    if (COUNT) cand += hit;
    if (!hit) return;
    const float maxd = R + r.radius;  // MaxDistance = currentBeamRadius + beam->radius
    float dist;
    const bool ok = closest_distance(L.o, L.p, L.au, L.mag_a, r.b0, r.bu, r.mag_b, dist);
    if (ok & (dist < maxd)) {
        const float rr = dist / maxd;
        const float w = sqrtf(1.0f - rr * rr);
        const float4 pv = pw[bi];
        cr += pv.x * w;
        cg += pv.y * w;
        cb += pv.z * w;
        ++contrib;
    }
}

template <bool COUNT>
__device__ __forceinline__ void finish_lane(int64_t s, bool valid, float cr, float cg, float cb, int cand, int contrib,
                                            unsigned long long visits, const int32_t *__restrict__ pixel, int64_t npix,
                                            float *__restrict__ accum, float *__restrict__ seg_rgb,
                                            int32_t *__restrict__ seg_counts, DevCounters *ctr) {
    if (valid) {
        if (seg_rgb) {
            seg_rgb[3 * s] = cr;
            seg_rgb[3 * s + 1] = cg;
            seg_rgb[3 * s + 2] = cb;
        }
        if (accum) {
            const int32_t px = pixel[s];
            if (px < 0 || px >= npix) {
                atomicOr(&ctr->flags, kFlagPixel);
            } else if (cr != 0.f || cg != 0.f || cb != 0.f) {
                atomicAdd(&accum[3 * (int64_t)px], cr);
                atomicAdd(&accum[3 * (int64_t)px + 1], cg);
                atomicAdd(&accum[3 * (int64_t)px + 2], cb);
            }
        }
        if (seg_counts) {
            seg_counts[2 * s] = COUNT ? cand : -1;
            seg_counts[2 * s + 1] = contrib;
        }
    }
    if (COUNT) {
        unsigned long long c = valid ? (unsigned long long)cand : 0ull;
        unsigned long long k = valid ? (unsigned long long)contrib : 0ull;
        unsigned long long v = visits;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            c += __shfl_xor(c, off);
            k += __shfl_xor(k, off);
            v += __shfl_xor(v, off);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&ctr->candidates, c);
            atomicAdd(&ctr->contributions, k);
            atomicAdd(&ctr->node_visits, v);
        }
    }
}

template <bool COUNT>
__global__ __launch_bounds__(kThreadBlock) void k_gather_thread(
    int64_t nseg, const float *__restrict__ so, const float *__restrict__ sp_, const float *__restrict__ sd,
    const float *__restrict__ stmax, const int32_t *__restrict__ pixel, float R, int64_t npix,
    float *__restrict__ accum, float *__restrict__ seg_rgb, int32_t *__restrict__ seg_counts,
    const BeamRec *__restrict__ recs, const float4 *__restrict__ pw, BeamSet bset, const Node *__restrict__ nodes,
    int64_t nvalid, int leaf_size, DevCounters *ctr, int stack_cap) {
    __shared__ int32_t stk[kThreadStackDepth][kThreadBlock];
    const int tid = threadIdx.x;
    const int64_t s = (int64_t)blockIdx.x * kThreadBlock + tid;
    Lane L;
    const bool valid = load_lane(s, nseg, so, sp_, sd, stmax, L);
    float cr = 0.f, cg = 0.f, cb = 0.f;
    int cand = 0, contrib = 0;
    unsigned long long visits = 0;
    if (valid && nvalid > 0) {
        int node = 0;
        int sp = 0;
        const int cap = stack_cap < kThreadStackDepth ? stack_cap : kThreadStackDepth;
        while (true) {
            const NodeV n = load_node(nodes, node);
            if (COUNT) ++visits;
            const int32_t c0 = n.c0, c1 = n.c1;
            float te0 = 0.f, te1 = 0.f;
            bool h0 = (c0 != kEmptyChild) & node_test(n.b0, L.o, L.invs, L.tmax, te0);
            bool h1 = (c1 != kEmptyChild) & node_test(n.b1, L.o, L.invs, L.tmax, te1);
            if (h0 && c0 < 0) {
                const int64_t first = (int64_t)(~c0) * leaf_size;
                const int cnt = (int)min((int64_t)leaf_size, nvalid - first);
                for (int j = 0; j < cnt; ++j)
                    eval_beam<COUNT>(L, true, load_beam(recs, first + j, bset), pw, first + j, R, cr, cg, cb, cand, contrib);
                h0 = false;
            }
            if (h1 && c1 < 0) {
                const int64_t first = (int64_t)(~c1) * leaf_size;
                const int cnt = (int)min((int64_t)leaf_size, nvalid - first);
                for (int j = 0; j < cnt; ++j)
                    eval_beam<COUNT>(L, true, load_beam(recs, first + j, bset), pw, first + j, R, cr, cg, cb, cand, contrib);
                h1 = false;
            }
            if (h0 && h1) {
                const bool first0 = !(te1 < te0);
                if (sp >= cap) {
                    atomicOr(&ctr->flags, kFlagStack);
                    break;
                }
                stk[sp][tid] = first0 ? c1 : c0;
                ++sp;
                node = first0 ? c0 : c1;
            } else if (h0) {
                node = c0;
            } else if (h1) {
                node = c1;
            } else {
                if (sp == 0) break;
                --sp;
                node = stk[sp][tid];
            }
        }
    }
    finish_lane<COUNT>(s, valid, cr, cg, cb, cand, contrib, visits, pixel, npix, accum, seg_rgb, seg_counts, ctr);
}

}  // namespace

hipError_t launch_gather_thread(const GatherArgs &a, bool counters, hipStream_t s) {
    if (a.nseg == 0) return hipSuccess;
    const int stack_cap = a.stack_cap > 0 ? a.stack_cap : kStackDepth;
    if (stack_cap > kStackDepth) return hipErrorInvalidValue;
    if (a.seg_index && (a.out.seg_rgb || a.out.seg_counts)) return hipErrorInvalidValue;  // kernel 2 writes in place
    const dim3 grid((unsigned int)((a.nseg + kThreadBlock - 1) / kThreadBlock));
    if (counters)
        hipLaunchKernelGGL(k_gather_thread<true>, grid, dim3(kThreadBlock), 0, s, a.nseg, a.seg.o, a.seg.p, a.seg.d,
                           a.seg.t, a.seg.pix, a.R, a.npix, a.out.accum, a.out.seg_rgb, a.out.seg_counts, a.recs, a.pow,
                           a.bset, a.nodes, a.nvalid, a.leaf_size, a.ctr, stack_cap);
    else
        hipLaunchKernelGGL(k_gather_thread<false>, grid, dim3(kThreadBlock), 0, s, a.nseg, a.seg.o, a.seg.p, a.seg.d,
                           a.seg.t, a.seg.pix, a.R, a.npix, a.out.accum, a.out.seg_rgb, a.out.seg_counts, a.recs, a.pow,
                           a.bset, a.nodes, a.nvalid, a.leaf_size, a.ctr, stack_cap);
    return hipGetLastError();
}

}  // namespace bre
