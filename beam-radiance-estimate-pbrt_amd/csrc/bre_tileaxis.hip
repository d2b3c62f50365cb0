// bre_tileaxis.hip — the per-gather tile-axis pass ahead of the tile kernel (bre_gather.hip): the box of
// the launch's segments (k_segbox_init, k_segbox) and one axis line per leaf tile (k_tile_axis), which
// the tile kernel's per-lane tile line reject tests.
#include <hip/hip_runtime.h>

#include <float.h>

#include <algorithm>

#include "bre_device.h"
#include "bre_lane.h"
#include "bre_math.h"

namespace bre {

namespace {

// ---------------------------------------------------------------------------------------------
// Per-lane tile line reject (option 112 = 1).  A contributing pair (lane i, beam j) has the reference's
// pA on segment i (to rounding) and pB on beam j's line with |pA - pB| < maxd_j, so pB lies in the box
// of the launch's segments grown by maxd_j.  k_tile_axis gives every tile an axis line such that every
// beam LINE of the tile, clipped to that box (plus a margin), lies within rho of it (distance to a line
// is convex along a line, so the clipped piece's two end points bound it).  Then
//   D(line_i, axis) <= d(pA, axis) <= |pA - pB| + d(pB, axis) < maxd_j + rho,
// so a lane whose segment LINE is farther than rho + maxd_max from the axis line has no pair in the
// tile that can contribute.  The test is the scan's own separable line-distance test
// (scan_keep_mask) with the axis as a pseudo-beam whose threshold is rho + Ab' (Ab' with the tile's
// largest |b0|_1 and |B|, so the scan's rounding analysis covers every beam of the tile): per leaf
// visit one 14-VALU test per lane, before the tile is staged.  Lanes it rejects are taken off the tile
// (fewer lanes on: more tiles take the transposed scan), and a tile no lane keeps is not staged at all.
// Only the production instantiation tests (the counting one box-tests every beam of a visited tile for
// C); the rejected pairs never contribute, so the queues differ only by non-contributing pairs and
// every per-segment sum is bit-identical (tests/test_prefilter_options_gpu.py).
__global__ void k_segbox_init(unsigned int *__restrict__ b) {
    if (threadIdx.x < 6) b[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
}

// box of the launch's finite segment end points (6 ordered uints: min xyz, max xyz).  Grid-stride
// over a bounded grid, reduced per wave and then per block in LDS: one set of six atomics per block
// (per-wave atomics on the same six words serialised at the L2: 0.64 ms at C2's 0.6M segments)
constexpr int kSegboxBlocks = 512;
__global__ __launch_bounds__(kPassBlock) void k_segbox(int64_t nseg, const float *__restrict__ o, const float *__restrict__ p,
                                                unsigned int *__restrict__ b) {
    __shared__ unsigned int red[kPassBlock / 64][6];
    unsigned int mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    for (int64_t i = (int64_t)blockIdx.x * kPassBlock + threadIdx.x; i < nseg; i += (int64_t)gridDim.x * kPassBlock) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float *q = (e ? p : o) + 3 * i;
            const float v[3] = {q[0], q[1], q[2]};
            if (isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2])) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    mn[k] = min(mn[k], f2ord(v[k]));
                    mx[k] = max(mx[k], f2ord(v[k]));
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mn[k] = min(mn[k], (unsigned int)__shfl_xor((int)mn[k], off));
            mx[k] = max(mx[k], (unsigned int)__shfl_xor((int)mx[k], off));
        }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            red[w][k] = mn[k];
            red[w][3 + k] = mx[k];
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        unsigned int v = red[0][k];
        for (int j = 1; j < kPassBlock / 64; ++j) v = k < 3 ? min(v, red[j][k]) : max(v, red[j][k]);
        if (k < 3)
            atomicMin(&b[k], v);
        else
            atomicMax(&b[k], v);
    }
}

// One wave per leaf tile: axis = mean start -> mean end of its usable beams, rho = the largest
// distance of a clipped beam line's end points from the axis (with rounding margins), stored as the
// pseudo-beam record the per-lane tile line reject tests (TileAxis).
__global__ __launch_bounds__(64) void k_tile_axis(const BeamRec *__restrict__ recs, BeamSet bset, int64_t nvalid,
                                                  int leaf_size,
                                                  const unsigned int *__restrict__ segb, float R,
                                                  TileAxis *__restrict__ out) {
    const int64_t tile = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t j = tile * leaf_size + lane;
    bool ok = lane < leaf_size && j < nvalid;
    f3 b0 = mk(0.f, 0.f, 0.f), bu = mk(0.f, 0.f, 0.f);
    float mb = 0.f, rad = 0.f;
    if (ok) {
        const BeamV r = load_beam(recs, j, bset);
        b0 = r.b0;
        bu = r.bu;
        mb = r.mag_b;
        rad = r.radius;
        // a zero-length or non-finite beam has a NaN / infinite reference box: never a candidate
        ok = mb > 0.f && isfinite(mb) && isfinite(b0.x) && isfinite(b0.y) && isfinite(b0.z) && isfinite(bu.x) &&
             isfinite(bu.y) && isfinite(bu.z) && isfinite(rad);
    }
    const float rmax = wave_max(ok ? rad : 0.f);
    const float n = wave_sum(ok ? 1.f : 0.f);
    TileAxis A;
    if (n == 0.f || !(segb[0] <= segb[3] && segb[1] <= segb[4] && segb[2] <= segb[5])) {
        // no usable beam (or no finite segment): nothing of this tile can contribute
        A.d[0] = 1.f;
        A.d[1] = A.d[2] = 0.f;
        A.thr = 0.f;
        A.m[0] = A.m[1] = A.m[2] = 0.f;
        A.grow = -1.f;
        if (lane == 0) out[tile] = A;
        return;
    }
    const f3 e = add3(b0, scale3(bu, mb));
    // the axis through the centres of the starts' and the ends' boxes (round 5: C2 +1.2% over the
    // mean start -> mean end, profiles/r5/run3)
    const auto ctr = [&](float v) {
        const float hi = wave_max(ok ? v : -FLT_MAX), lo = -wave_max(ok ? -v : -FLT_MAX);
        return 0.5f * lo + 0.5f * hi;
    };
    const f3 ps = mk(ctr(b0.x), ctr(b0.y), ctr(b0.z));
    const f3 pe = mk(ctr(e.x), ctr(e.y), ctr(e.z));
    f3 d = sub3(pe, ps);
    const float dl = sqrtf(lensq3(d));
    d = (dl > 1e-6f * (1.f + fabsf(ps.x) + fabsf(ps.y) + fabsf(ps.z)) && isfinite(dl)) ? scale3(d, 1.f / dl)
                                                                                      : mk(1.f, 0.f, 0.f);
    // the region: segment box grown by maxd_max = R + rmax, plus margins
    const float lo[3] = {ord2f(segb[0]), ord2f(segb[1]), ord2f(segb[2])};
    const float hi[3] = {ord2f(segb[3]), ord2f(segb[4]), ord2f(segb[5])};
    const float cm = fmaxf(fmaxf(fmaxf(fabsf(lo[0]), fabsf(lo[1])), fmaxf(fabsf(lo[2]), fabsf(hi[0]))),
                           fmaxf(fabsf(hi[1]), fabsf(hi[2])));
    const float grow = (R + rmax) * 1.001f + 1e-5f * cm + 1e-6f;
    float dist = 0.f;
    if (ok) {
        const float o3[3] = {b0.x, b0.y, b0.z}, u3[3] = {bu.x, bu.y, bu.z};
        float t0 = -FLT_MAX, t1 = FLT_MAX;
        bool in = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float l = lo[k] - grow, h = hi[k] + grow;
            if (u3[k] == 0.f) {
                in = in && o3[k] >= l && o3[k] <= h;
            } else {
                float a = (l - o3[k]) / u3[k], c = (h - o3[k]) / u3[k];
                if (a > c) {
                    const float x = a;
                    a = c;
                    c = x;
                }
                t0 = fmaxf(t0, a);
                t1 = fminf(t1, c);
            }
        }
        if (in && t0 <= t1) {
            // widen the piece by a little (the slab parameters carry rounding)
            const float tw = 1e-5f * (fabsf(t0) + fabsf(t1)) + 1e-6f;
            t0 -= tw;
            t1 += tw;
            const auto dax = [&](float t) {
                const f3 q = sub3(add3(b0, scale3(bu, t)), ps);
                const f3 c = mk(q.y * d.z - q.z * d.y, q.z * d.x - q.x * d.z, q.x * d.y - q.y * d.x);
                return sqrtf(lensq3(c));
            };
            dist = fmaxf(dax(t0), dax(t1));
            // a NaN distance must not shrink rho: treat it as unbounded
            if (!(dist == dist)) dist = FLT_MAX;
        }
    }
    const float rho_raw = wave_max(dist);
    const float pm = fmaxf(fmaxf(fabsf(ps.x), fabsf(ps.y)), fabsf(ps.z));
    const float rho = rho_raw * 1.0001f + 1e-5f * (cm + pm + grow) + 1e-6f;
    // the scan's beam-side margin Ab' (make_scan_beam) with maxd_max and the tile's largest |b0|_1 and
    // |B| (the separable form evaluates t.n at the axis point: its |p|_1 joins the max)
    const float b1 = wave_max(ok ? fabsf(b0.x) + fabsf(b0.y) + fabsf(b0.z) : 0.f);
    const float p1 = fabsf(ps.x) + fabsf(ps.y) + fabsf(ps.z);
    const float bmag = wave_max(ok ? mb : 0.f);
    const float ab = (R + rmax) * 1.000001f + 1.93e-5f * fmaxf(b1, p1) + 2.4e-7f * bmag + 1e-6f;
    const float thr = (rho + ab) * 1.0001f + 1e-6f;
    A.d[0] = d.x;
    A.d[1] = d.y;
    A.d[2] = d.z;
    A.thr = (rho_raw < FLT_MAX && isfinite(thr)) ? thr : FLT_MAX;  // FLT_MAX: never a reject
    A.m[0] = d.y * ps.z - d.z * ps.y;  // m = d x p (the scan's m0 = bu x b0)
    A.m[1] = d.z * ps.x - d.x * ps.z;
    A.m[2] = d.x * ps.y - d.y * ps.x;
    A.grow = grow;
    if (lane == 0) out[tile] = A;
}

}  // namespace

hipError_t launch_tile_axis(const GatherArgs &a, hipStream_t s) {
    const int64_t ntiles = (a.nvalid + a.leaf_size - 1) / a.leaf_size;
    hipLaunchKernelGGL(k_segbox_init, dim3(1), dim3(64), 0, s, a.segbox);
    hipLaunchKernelGGL(k_segbox, dim3((unsigned int)std::min<int64_t>(kSegboxBlocks, (a.nseg + kPassBlock - 1) / kPassBlock)), dim3(kPassBlock), 0, s, a.nseg, a.seg.o, a.seg.p,
                       a.segbox);
    hipLaunchKernelGGL(k_tile_axis, dim3((unsigned int)ntiles), dim3(64), 0, s, a.recs, a.bset, a.nvalid,
                       a.leaf_size, a.segbox, a.R, a.tileax);
    return hipGetLastError();
}

}  // namespace bre
