// bre_photon.hip — the photon pass on the GPU: emission + TracePhotonBeamRecursive
// (src/integrators/photonbeam.cpp:258-325, 383-421) for every photon of an iteration, one thread
// per photon, producing the beam set the gather consumes.
//
// The reference recurses on every medium scattering event (the scattered photon is traced to
// completion, then the parent path continues, :274-288).  Here the recursion is an explicit
// per-thread stack of suspended parent frames (at most maxdepth of them, since each level adds
// one to depth), and the random numbers are drawn in exactly the reference's order from the
// photon's own PCG32 sequence iter*N + i + 1 (:386-389), so each photon's beams, their order and
// their bits are those of the reference's single-threaded loop.
//
// Output is deterministic and photon-major: beam k of photon i lands at offsets[i] + k, offsets the
// inclusive scan of the per-photon counts.  The default single-trace form (round 4) traces each photon
// once, writing its first `cap` beams to the photon's own slots of a scratch array and its count;
// after the scan a copy puts the slots at their offsets, and only the photons with more than `cap`
// beams are traced again, straight to their offsets (the same code and random sequence: the same
// bits).  cap is sized so the scratch stays within 2.5 GB (62 slots at 1M photons; C2's photons
// average 2.7 beams, but the few long paths re-traced past 16 slots cost 0.25 ms); the two-trace form
// (count, scan, re-trace every photon) is the fallback.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <type_traits>

#include "bre_device.h"
#include "bre_trace.h"

namespace bre {

namespace {

#ifndef BRE_PHOTON_BLOCK
#define BRE_PHOTON_BLOCK 64  // one wave: fits a concurrent gather's slots (bre_slot.hip; 128 until round 5)
#endif
constexpr int kPhotonBlock = BRE_PHOTON_BLOCK;

// A path suspended at a medium scattering event while its scattered child is traced.
struct Frame {
    f3 o, d;     // photonRay
    float tmax;  // its surface hit distance
    f3 p, perr;  // isect.p and its error bound
    int tri;
    int depth;
    float beta[3];
};
// ... with media (bre_set_media): the parent resumes in its own medium
struct FrameMed : Frame {
    int med;
};

// MODE 0: count each photon's beams; 1: write them at offsets[i] + k (with over > 0: only the photons
// whose count exceeds `over`, the single-trace form's overflow); 2: write the first `over` beams to
// the photon's slots i * over + k and count them all.
// MED: the context holds media: the ray carries its medium (an index into S.media, -1 vacuum), taken by
// GetMedium at every spawn, and an interface triangle is passed through (photonbeam.cpp:300-304).  MED false
// is the one-medium walk, the code it was before media.
// GL: the context's table holds a plastic, metal or matte entry (bre_set_materials_ex): such a triangle scatters
// through the general BSDF (bsdf_sample, bre_trace.h).  GL false is the code it was before them, held to 80 VGPRs
// because its waves run inside another context's gather; the glossy kernels carry the
// microfacet lobe's registers and take kGlossyWaves waves per SIMD instead.
// GL keeps the suspended frames in the block's dynamic LDS, behind the scene traversal stack, instead of a
// per-thread array: word w of thread t's frame k at [(k * kFrameWords + w) * kPhotonBlock + t].  A path holds at
// most max_depth frames (each push adds one to depth), so the launch sizes the region to max_depth frames.
// TIER: 0 = GL false, 1 = GL true, 2 = the table holds a rough glass, uber, translucent or substrate entry
// (bre_set_materials_ex, types 8 .. 11): every entry from BRE_MATERIAL_MATTE up scatters through the BSDF of any
// number of lobes (bsdfn_sample with BSDF_ALL in TransportMode::Importance); frames in LDS as for GL.  The walk is one
// body: k_photons<MODE, MED, GL> runs tiers 0 and 1 under the names and bounds it had, k_photons_tr<MODE, MED> tier 2.
// TIER 3 (the table holds a BRE_MATERIAL_MIX): tier 2 over the wide lists (S.lobes_mx: up to BRE_MAX_BXDFS lobes, each
// under its chain of ScaledBxDF scales), in k_photons_mx<MODE, MED>.  A triangle whose own material is a mirror or a
// smooth glass keeps the one-lobe specular path in every tier.
constexpr int kFrameWords = 19;  // o, d, tmax, p, perr, tri, depth, beta, med
template <int MODE, bool MED, int TIER>
__device__ __forceinline__ void photon_walk(const DevScene *__restrict__ Sp, int64_t n, uint64_t seq0, int max_depth,
                                            float radius, int32_t *__restrict__ counts,
                                            const int64_t *__restrict__ offsets, float *__restrict__ bs,
                                            float *__restrict__ be, float *__restrict__ br, float *__restrict__ bp,
                                            int over) {
    constexpr bool GL = TIER >= 1;
    const int64_t i = (int64_t)blockIdx.x * kPhotonBlock + threadIdx.x;
    if (i >= n) return;
    if (MODE == 1 && over > 0 && counts[i] <= over) return;
    const DevScene &S = *Sp;
    Pcg rng;
    pcg_seed(rng, seq0 + (uint64_t)i);
    const int64_t w = MODE == 1 ? offsets[i] : (MODE == 2 ? i * (int64_t)over : 0);
    int cnt = 0;

    // ---- emission, photonbeam.cpp:393-418: a light by power, then its Sample_Le (DiffuseAreaLight on a
    // triangle, PointLight, SpotLight or DistantLight); the five draws are the same whatever the light ----
    float light_pdf;
    const int ln = sample_light(S, pcg_float(rng), light_pdf);  // lightSample
    float u0x, u0y, u1x, u1y;
    pcg_2d(rng, u0x, u0y);
    pcg_2d(rng, u1x, u1y);
    (void)pcg_float(rng);  // uLightTime
    const int lt = S.light_tri[ln];
    f3 o, d;
    float beta[3];
    bool alive;
    int med = -1;  // MED: photonRay.medium
    if (lt >= 0) {
        const PTri &L = S.t[lt];
        const ShapeSample ps = sample_tri(L, u0x, u0y);
        const float pdf_pos = ps.pdf;
        f3 wl;
        float pdf_dir;
        if (L.emit == BRE_EMIT_TWO_SIDED) {
            // diffuse.cpp:100-112: u[0] < .5 picks the side and is remapped to [0, 1); the far side's w.z is negated
            const bool near = u1x < .5f;
            wl = cosine_hemisphere(smin(near ? u1x * 2 : (u1x - .5f) * 2, kOneMinusEps), u1y);
            if (!near) wl.z *= -1;
            pdf_dir = 0.5f * (fabsf(wl.z) * kInvPi);
        } else {
            wl = cosine_hemisphere(u1x, u1y);
            pdf_dir = wl.z * kInvPi;
        }
        f3 v1, v2;
        coord_system(ps.n, v1, v2);
        d = add3(add3(scale3(v1, wl.x), scale3(v2, wl.y)), scale3(ps.n, wl.z));
        o = offset_origin(ps.p, ps.perr, ps.n, d);
        // DiffuseAreaLight::Sample_Le: pShape.mediumInterface = mediumInterface, the ray is pShape.SpawnRay(w)
        if constexpr (MED) med = dot3(d, ps.n) > 0 ? S.tri_med[2 * lt + 1] : S.tri_med[2 * lt];
        const bool front = L.emit == BRE_EMIT_TWO_SIDED || dot3(ps.n, d) > 0;  // DiffuseAreaLight::L (diffuse.h:56-58)
        alive = !(pdf_pos == 0 || pdf_dir == 0 || !front || black3(L.Le));
        if (alive) {
            const float ad = fabsf(dot3(ps.n, d));
            const float den = light_pdf * pdf_pos * pdf_dir;
            for (int c = 0; c < 3; ++c) beta[c] = (ad * L.Le[c]) / den;
            alive = !black3(beta);
        }
    } else {
        // PointLight / SpotLight::Sample_Le: the ray leaves pLight itself, nLight = d, pdfPos = 1; a
        // direction the two matrices push outside the cone has Falloff 0 and the photon ends (:412).
        // DistantLight::Sample_Le: from the disk outside the world, pdfPos = 1 / (Pi r^2); its medium is -1
        // (an empty MediumInterface, checked by the host), so the leg down to the first surface is in vacuum
        // and still leaves a beam
        const DLight &D = S.dlights[~lt];
        float pdf_pos, pdf_dir, fo;
        light_sample_le(D, u0x, u0y, o, d, pdf_pos, pdf_dir, fo);
        if constexpr (MED) med = S.light_med[~lt];  // Ray(pLight, w, Infinity, time, mediumInterface.inside)
        float Le[3];
        for (int c = 0; c < 3; ++c) Le[c] = D.I[c] * fo;
        alive = !(pdf_pos == 0 || pdf_dir == 0 || black3(Le));
        if (alive) {
            const float ad = fabsf(dot3(d, d));
            const float den = light_pdf * pdf_pos * pdf_dir;
            for (int c = 0; c < 3; ++c) beta[c] = (ad * Le[c]) / den;
            alive = !black3(beta);
        }
    }

    // ---- TracePhotonBeamRecursive as a state machine ----
    typename std::conditional<GL, char, typename std::conditional<MED, FrameMed, Frame>::type>::type
        stk[GL ? 1 : BRE_MAX_DEPTH];
    extern __shared__ int bre_scene_stack[];  // GL: the frames follow intersect_scene's stack_depth * blockDim words
    float *const frames = reinterpret_cast<float *>(bre_scene_stack) +
                          (GL ? (S.stack_depth > 0 ? S.stack_depth : 1) * kPhotonBlock + (int)threadIdx.x : 0);
    (void)stk;
    int sp = 0;
    int depth = 0;
    float tmax = 0;
    Hit hit;
    bool resume = false;
    while (alive) {
        bool stop = false;
        if (!resume) {
            tmax = __builtin_huge_valf();
            if (depth >= max_depth || !intersect_scene(S, o, d, tmax, hit)) {
                stop = true;
            } else {
                bool scattered = false;
                float ts = 0;
                scattered = ray_medium_sample<MED>(S, med, rng, o, d, tmax, ts);
                if (black3(beta)) {
                    stop = true;
                } else if (scattered) {
                    // HG direction from the scattering point; the child path starts there with
                    // beta * Tr(whole segment) (photonbeam.cpp:276-285)
                    float hx, hy;
                    pcg_2d(rng, hx, hy);
                    float g = S.own.g;
                    if constexpr (MED) g = S.media[med].g;
                    const f3 wi = hg_sample(g, neg3(d), hx, hy);
                    float tr[3];
                    ray_medium_tr<MED>(S, med, rng, o, d, tmax, tr);
                    if constexpr (GL) {
                        float *f = frames + sp++ * (kFrameWords * kPhotonBlock);
                        const float w[kFrameWords] = {o.x, o.y, o.z, d.x, d.y, d.z, tmax, hit.p.x, hit.p.y, hit.p.z,
                                                      hit.perr.x, hit.perr.y, hit.perr.z, __int_as_float(hit.tri),
                                                      __int_as_float(depth), beta[0], beta[1], beta[2],
                                                      __int_as_float(med)};
#pragma unroll
                        for (int k = 0; k < kFrameWords; ++k) f[k * kPhotonBlock] = w[k];
                        for (int c = 0; c < 3; ++c) beta[c] = beta[c] * tr[c];
                    } else {
                        auto &f = stk[sp++];
                        f.o = o;
                        f.d = d;
                        f.tmax = tmax;
                        f.p = hit.p;
                        f.perr = hit.perr;
                        f.tri = hit.tri;
                        f.depth = depth;
                        if constexpr (MED) f.med = med;  // the child stays in it too (MediumInterface(this))
                        for (int c = 0; c < 3; ++c) {
                            f.beta[c] = beta[c];
                            beta[c] = beta[c] * tr[c];
                        }
                    }
                    o = ray_at(o, d, ts);  // MediumInteraction::SpawnRay: no offset
                    d = wi;
                    depth += 1;
                    continue;
                }
            }
        }
        if (!stop) {
            resume = false;
            // beam for the whole surface-hit segment, powerEnd = Tr * beta (:289-294)
            float bm[3];
            ray_medium_tr<MED>(S, med, rng, o, d, tmax, bm);
            if (MODE == 1 || (MODE == 2 && cnt < over)) {
                const int64_t k = w + cnt;
                bs[3 * k + 0] = o.x;
                bs[3 * k + 1] = o.y;
                bs[3 * k + 2] = o.z;
                be[3 * k + 0] = hit.p.x;
                be[3 * k + 1] = hit.p.y;
                be[3 * k + 2] = hit.p.z;
                br[k] = radius;
                for (int c = 0; c < 3; ++c) bp[3 * k + c] = bm[c] * beta[c];
            }
            ++cnt;
            if constexpr (MED) {
                // no BSDF (:300-304): --depth; photonRay = isect.SpawnRay(photonRay.d); continue -- before the
                // Get2D, with beta as it was (not multiplied by the segment's Tr) and without roulette
                const PTri &qi = S.t[hit.tri];
                if (qi.mat == kMatInterface) {
                    o = offset_origin(hit.p, hit.perr, qi.n, d);
                    med = medium_towards(S, hit.tri, qi.n, d, med);
                    continue;
                }
            }
            // surface scattering (:296-323): BSDF::Sample_f of the Lambertian lobe, or of a mirror's or
            // glass's specular lobe in TransportMode::Importance; the Get2D comes first either way
            float ux, uy;
            pcg_2d(rng, ux, uy);
            const PTri &q = S.t[hit.tri];
            if (q.mat == kMatNone) {
                stop = true;
            } else {
                const f3 wo = neg3(d);
                const float woz = dot3(wo, q.n);
                if (woz == 0) {
                    stop = true;
                } else {
                    f3 wil, wiw;
                    float pdf, fr[3];
                    bool world = false;  // GL: wiw is BSDF::Sample_f's own LocalToWorld(wi)
                    if constexpr (TIER == 3) world = q.mat >= kMatTable && S.lobes_mx[q.mat - kMatTable].type != 0;
                    else if constexpr (TIER == 2) world = q.mat >= kMatTable && S.lobes[q.mat - kMatTable].type != 0;
                    else if constexpr (GL) world = q.mat >= kMatTable && S.bsdfs[q.mat - kMatTable].type != 0;
                    if (world) {
                        int type;
                        pdf = 0.f;
                        if constexpr (TIER == 3)
                            bsdfn_sample(q, S.lobes_mx[q.mat - kMatTable], wo, ux, uy, kBsdfAll, kModeImportance, wiw,
                                         pdf, fr, type);
                        else if constexpr (TIER == 2)
                            bsdfn_sample(q, S.lobes[q.mat - kMatTable], wo, ux, uy, kBsdfAll, kModeImportance, wiw, pdf,
                                         fr, type);
                        else
                            bsdf_sample(q, S.bsdfs[q.mat - kMatTable], wo, ux, uy, wiw, pdf, fr, type);
                    } else if (q.mat >= kMatTable) {
                        int type;
                        specular_sample(S.mats[q.mat - kMatTable], mk(dot3(wo, q.ss), dot3(wo, q.ts), woz), ux,
                                        kModeImportance, wil, pdf, fr, type);
                    } else {
                        wil = cosine_hemisphere(ux, uy);
                        if (woz < 0) wil.z *= -1;
                        pdf = (woz * wil.z > 0) ? fabsf(wil.z) * kInvPi : 0.f;
                        for (int c = 0; c < 3; ++c) fr[c] = q.kd[c] * kInvPi;
                    }
                    if (pdf == 0 || black3(fr)) {
                        stop = true;
                    } else {
                        const f3 wi = world ? wiw : to_world(q, wil);
                        const float ad = fabsf(dot3(wi, q.n));
                        float bn[3];
                        for (int c = 0; c < 3; ++c) bn[c] = bm[c] * beta[c] * fr[c] * ad / pdf;
                        o = offset_origin(hit.p, hit.perr, q.n, wi);
                        d = wi;
                        if constexpr (MED) med = medium_towards(S, hit.tri, q.n, wi, med);  // isect.SpawnRay(wi)
                        const float qrr = smax(0.f, 1 - lum3(bn) / lum3(beta));
                        if (pcg_float(rng) < qrr) {
                            stop = true;
                        } else {
                            for (int c = 0; c < 3; ++c) beta[c] = bn[c] / (1 - qrr);
                            depth += 1;
                        }
                    }
                }
            }
            if (!stop) continue;
        }
        // this path ends: resume the innermost suspended parent after its recursive call
        if (sp == 0) break;
        if constexpr (GL) {
            const float *f = frames + --sp * (kFrameWords * kPhotonBlock);
            float w[kFrameWords];
#pragma unroll
            for (int k = 0; k < kFrameWords; ++k) w[k] = f[k * kPhotonBlock];
            o = mk(w[0], w[1], w[2]);
            d = mk(w[3], w[4], w[5]);
            tmax = w[6];
            hit.p = mk(w[7], w[8], w[9]);
            hit.perr = mk(w[10], w[11], w[12]);
            hit.tri = __float_as_int(w[13]);
            depth = __float_as_int(w[14]);
            for (int c = 0; c < 3; ++c) beta[c] = w[15 + c];
            if constexpr (MED) med = __float_as_int(w[18]);
        } else {
            const auto &f = stk[--sp];
            o = f.o;
            d = f.d;
            tmax = f.tmax;
            hit.p = f.p;
            hit.perr = f.perr;
            hit.tri = f.tri;
            depth = f.depth;
            for (int c = 0; c < 3; ++c) beta[c] = f.beta[c];
            if constexpr (MED) med = f.med;
        }
        resume = true;
    }
    if (MODE != 1) counts[i] = cnt;
}

template <int MODE, bool MED, bool GL>
__global__ __launch_bounds__(kPhotonBlock, GL ? kGlossyWaves : 6) void k_photons(const DevScene *__restrict__ Sp, int64_t n, uint64_t seq0,
                                                          int max_depth, float radius, int32_t *__restrict__ counts,
                                                          const int64_t *__restrict__ offsets, float *__restrict__ bs,
                                                          float *__restrict__ be, float *__restrict__ br,
                                                          float *__restrict__ bp, int over) {
    photon_walk<MODE, MED, GL ? 1 : 0>(Sp, n, seq0, max_depth, radius, counts, offsets, bs, be, br, bp, over);
}

template <int MODE, bool MED>
__global__ __launch_bounds__(kPhotonBlock, kGlossyWaves) void k_photons_tr(const DevScene *__restrict__ Sp, int64_t n, uint64_t seq0,
                                                          int max_depth, float radius, int32_t *__restrict__ counts,
                                                          const int64_t *__restrict__ offsets, float *__restrict__ bs,
                                                          float *__restrict__ be, float *__restrict__ br,
                                                          float *__restrict__ bp, int over) {
    photon_walk<MODE, MED, 2>(Sp, n, seq0, max_depth, radius, counts, offsets, bs, be, br, bp, over);
}

template <int MODE, bool MED>
__global__ __launch_bounds__(kPhotonBlock, kMixWaves) void k_photons_mx(const DevScene *__restrict__ Sp, int64_t n, uint64_t seq0,
                                                          int max_depth, float radius, int32_t *__restrict__ counts,
                                                          const int64_t *__restrict__ offsets, float *__restrict__ bs,
                                                          float *__restrict__ be, float *__restrict__ br,
                                                          float *__restrict__ bp, int over) {
    photon_walk<MODE, MED, 3>(Sp, n, seq0, max_depth, radius, counts, offsets, bs, be, br, bp, over);
}

// The single-trace form's copy: photon i's first min(count, cap) beams from its slots to its offsets.
// Each wave copies the beams of its 64 photons as one run: lane j takes the wave's j-th beam (owner by
// a search of the wave's prefix sums in LDS), so the writes of consecutive lanes are consecutive and a
// photon's slots are read together (a thread per photon strided its reads by cap slots: 0.27 ms at C2).
constexpr int kSlotsBlock = 64;
__global__ __launch_bounds__(kSlotsBlock) void k_photon_slots(int64_t n, int cap, const int32_t *__restrict__ counts,
                                                      const int64_t *__restrict__ offsets, const float *__restrict__ ss,
                                                      const float *__restrict__ se, const float *__restrict__ sr,
                                                      const float *__restrict__ sp, float *__restrict__ bs,
                                                      float *__restrict__ be, float *__restrict__ br,
                                                      float *__restrict__ bp) {
    __shared__ int pre[kSlotsBlock / 64][65];      // per wave: exclusive prefix sums of the photons' copied beams
    __shared__ int64_t off[kSlotsBlock / 64][64];  // per wave: the photons' output offsets
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kSlotsBlock + threadIdx.x;
    const int64_t i0 = i - lane;
    const int m = i < n ? min(counts[i], cap) : 0;
    int incl = m;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    pre[w][lane + 1] = incl;
    if (lane == 0) pre[w][0] = 0;
    off[w][lane] = i < n ? offsets[i] : 0;
    __builtin_amdgcn_wave_barrier();
    const int total = __shfl(incl, 63);
    for (int j = lane; j < total; j += 64) {
        int lo = 0, hi = 64;  // the photon p with pre[p] <= j < pre[p + 1]
#pragma unroll
        for (int it = 0; it < 6; ++it) {
            const int mid = (lo + hi) >> 1;
            if (pre[w][mid] <= j) lo = mid;
            else hi = mid;
        }
        const int k = j - pre[w][lo];
        const int64_t a = (i0 + lo) * (int64_t)cap + k, b = off[w][lo] + k;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            bs[3 * b + c] = ss[3 * a + c];
            be[3 * b + c] = se[3 * a + c];
            bp[3 * b + c] = sp[3 * a + c];
        }
        br[b] = sr[a];
    }
}

inline unsigned grid_of(int64_t n) { return (unsigned)((n + kPhotonBlock - 1) / kPhotonBlock); }

}  // namespace

size_t photon_lds_bytes(int stack_depth, int max_depth, bool glossy) {
    const size_t frames = (size_t)(max_depth > 0 ? max_depth : 1) * kFrameWords * kPhotonBlock * sizeof(float);
    return scene_stack_bytes(stack_depth, kPhotonBlock) + (glossy ? frames : 0);
}

hipError_t launch_photons(const DevScene *scene, int stack_depth, int64_t n, uint64_t seq0, int max_depth,
                          float radius, int32_t *counts, const int64_t *offsets, const BeamOut &out, int mode,
                          int over, bool media, int tier, hipStream_t s) {
    if (n == 0) return hipSuccess;
    // tiers 1 and 2 keep their frames in LDS too (the caller has checked the device's room: photon_lds_bytes)
    const size_t lds = photon_lds_bytes(stack_depth, max_depth, tier >= 1);
    const auto go = [&](auto kernel, int ov) {
        hipLaunchKernelGGL(kernel, dim3(grid_of(n)), dim3(kPhotonBlock), lds, s, scene, n, seq0, max_depth, radius,
                           counts, offsets, out.start, out.end, out.radius, out.power, ov);
    };
    if (tier == 3) {
        if (mode == 1) media ? go(k_photons_mx<1, true>, over) : go(k_photons_mx<1, false>, over);
        else if (mode == 2) media ? go(k_photons_mx<2, true>, over) : go(k_photons_mx<2, false>, over);
        else media ? go(k_photons_mx<0, true>, 0) : go(k_photons_mx<0, false>, 0);
        return hipGetLastError();
    }
    if (tier == 2) {
        if (mode == 1) media ? go(k_photons_tr<1, true>, over) : go(k_photons_tr<1, false>, over);
        else if (mode == 2) media ? go(k_photons_tr<2, true>, over) : go(k_photons_tr<2, false>, over);
        else media ? go(k_photons_tr<0, true>, 0) : go(k_photons_tr<0, false>, 0);
        return hipGetLastError();
    }
    if (tier == 1) {
        if (mode == 1) media ? go(k_photons<1, true, true>, over) : go(k_photons<1, false, true>, over);
        else if (mode == 2) media ? go(k_photons<2, true, true>, over) : go(k_photons<2, false, true>, over);
        else media ? go(k_photons<0, true, true>, 0) : go(k_photons<0, false, true>, 0);
        return hipGetLastError();
    }
    if (mode == 1) media ? go(k_photons<1, true, false>, over) : go(k_photons<1, false, false>, over);
    else if (mode == 2) media ? go(k_photons<2, true, false>, over) : go(k_photons<2, false, false>, over);
    else media ? go(k_photons<0, true, false>, 0) : go(k_photons<0, false, false>, 0);
    return hipGetLastError();
}

hipError_t launch_photon_slots(int64_t n, int cap, const int32_t *counts, const int64_t *offsets,
                               const BeamView &slots, const BeamOut &out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_photon_slots, dim3((unsigned int)((n + kSlotsBlock - 1) / kSlotsBlock)), dim3(kSlotsBlock), 0, s, n, cap, counts, offsets,
                       slots.start, slots.end, slots.radius, slots.power, out.start, out.end, out.radius, out.power);
    return hipGetLastError();
}

size_t count_scan_temp_bytes(int64_t n) {
    size_t bytes = 0;
    (void)rocprim::inclusive_scan(nullptr, bytes, (const int32_t *)nullptr, (int64_t *)nullptr, (size_t)n,
                                  rocprim::plus<int64_t>());
    return std::max(bytes, slot_scan_temp_bytes(n));
}

// offsets[0] = 0, offsets[k + 1] = counts[0] + ... + counts[k].  slot: the one-wave scan (bre_slot.hip)
hipError_t launch_count_scan(void *tmp, size_t bytes, const int32_t *counts, int64_t *offsets, int64_t n,
                             hipStream_t s, bool slot) {
    if (slot) return slot_exclusive_scan(counts, offsets, n, offsets + n, tmp, s);
    hipError_t e = hipMemsetAsync(offsets, 0, sizeof(int64_t), s);
    if (e != hipSuccess || n == 0) return e;
    return rocprim::inclusive_scan(tmp, bytes, counts, offsets + 1, (size_t)n, rocprim::plus<int64_t>(), s);
}

}  // namespace bre
