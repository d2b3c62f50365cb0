// bre_check.hip — device self-check of the scalar primitives the passes and the gather share.
//
// The photon and camera passes step every spawned ray origin with NextFloatUp / NextFloatDown
// (OffsetRayOrigin, geometry.h:1438-1458; pbrt.h:215-239) and choose the emitting light with
// FindInterval (Distribution1D::SampleDiscrete, sampling.h:90-100; pbrt.h:377-389); the gather's
// exact stage takes its square roots and its shared-divisor quotient without the compiler's general
// expansions (bre_math.h sqrt_cr_noscale, div_by_shared).  bre_device_check runs those very device
// functions on caller-supplied inputs so the tests can hold them bit for bit against the reference's
// own primitive tests (src/tests/fp_tests.cpp, find_interval.cpp) and against the compiler's sqrtf
// and division -- a toolchain change to the f32 sqrt lowering then fails a test instead of silently
// moving the exact stage off the reference's rounding.
#include <hip/hip_runtime.h>

#include "bre_device.h"
#include "bre_math.h"
#include "bre_trace.h"

namespace bre {

namespace {

// kind 0: next_up; 1: next_down; 2: sqrt_cr_noscale and sqrtf (two outputs per input);
// 3: find_interval over aux[0, n_aux) with pred aux[i] <= x (the index as a float);
// 4: div_by_shared(x, aux[0], 1 / aux[0]) and x / aux[0] (two outputs per input);
// 9: the passes' expf, logf, sinf and cosf (include/bre_fmath.h; four outputs per input)
__global__ __launch_bounds__(256) void k_check(int kind, int64_t n, const float *__restrict__ x, int n_aux,
                                               const float *__restrict__ aux, float *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    switch (kind) {
    case 0: y[i] = next_up(v); break;
    case 1: y[i] = next_down(v); break;
    case 2:
        y[2 * i] = sqrt_cr_noscale(v);
        y[2 * i + 1] = sqrtf(v);
        break;
    case 3: y[i] = (float)find_interval(n_aux, [&](int k) { return aux[k] <= v; }); break;
    case 9:
        y[4 * i] = bre_expf(v);
        y[4 * i + 1] = bre_logf(v);
        bre_sincosf(v, &y[4 * i + 2], &y[4 * i + 3]);
        break;
    default: {
        const float b = aux[0];
        const float inv = 1.0f / b;
        y[2 * i] = div_by_shared(v, b, inv);
        y[2 * i + 1] = v / b;
    }
    }
}

// kind 12: specular_sample (bre_trace.h) on n records of 6 floats (wo xyz, u0, eta with 0 = mirror, mode),
// Kr = Kt = 1; 6 words out per record: wi xyz, pdf, f, the sampled type (int32)
__global__ __launch_bounds__(256) void k_check_specular(int64_t n, const float *__restrict__ x, float *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *r = x + 6 * i;
    bre_material m;
    m.type = r[4] == 0.f ? BRE_MATERIAL_MIRROR : BRE_MATERIAL_GLASS;
    m.kr[0] = m.kr[1] = m.kr[2] = m.kt[0] = m.kt[1] = m.kt[2] = 1.f;
    m.eta = r[4];
    f3 wi = mk(0.f, 0.f, 0.f);
    float pdf, f[3];
    int type;
    if (!specular_sample(m, mk(r[0], r[1], r[2]), r[3], r[5] != 0.f ? kModeRadiance : kModeImportance, wi, pdf, f, type))
        wi = mk(0.f, 0.f, 0.f);
    float *o = y + 6 * i;
    o[0] = wi.x;
    o[1] = wi.y;
    o[2] = wi.z;
    o[3] = pdf;
    o[4] = f[0];
    o[5] = __int_as_float(type);
}

// kind 13: the general BSDF (bre_trace.h) on n records of 9 floats (wo xyz, u0, u1, wi2 xyz, the index into
// `table`) in the frame ss = x, ts = y, n = z; 12 words out per record: wi xyz, pdf, f rgb, the sampled type
// (int32), f(wo, wi2) rgb, Pdf(wo, wi2)
__global__ __launch_bounds__(256) void k_check_bsdf(int64_t n, const float *__restrict__ x,
                                                    const DevBsdf *__restrict__ table, int n_table,
                                                    float *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *r = x + 9 * i;
    const int k = (int)r[8];
    float *o = y + 12 * i;
    for (int j = 0; j < 12; ++j) o[j] = 0.f;
    if (k < 0 || k >= n_table) return;
    const DevBsdf m = table[k];
    PTri q{};
    q.ss = mk(1.f, 0.f, 0.f);
    q.ts = mk(0.f, 1.f, 0.f);
    q.n = mk(0.f, 0.f, 1.f);
    const f3 wo = mk(r[0], r[1], r[2]), wi2 = mk(r[5], r[6], r[7]);
    f3 wi = mk(0.f, 0.f, 0.f);
    float pdf = 0.f, f[3];
    int type;
    if (bsdf_sample(q, m, wo, r[3], r[4], wi, pdf, f, type)) {
        o[0] = wi.x;
        o[1] = wi.y;
        o[2] = wi.z;
        o[3] = pdf;
        o[4] = f[0];
        o[5] = f[1];
        o[6] = f[2];
        o[7] = __int_as_float(type);
    }
    bsdf_f(q, m, wo, wi2, f);
    o[8] = f[0];
    o[9] = f[1];
    o[10] = f[2];
    o[11] = bsdf_pdf(q, m, wo, wi2);
}

// kind 14: the BSDF of any number of lobes (bre_trace.h) on n records of 11 floats: those of kind 13, then the
// transport mode (0: Importance) and the flag set (0: BSDF_ALL, 1: BSDF_ALL & ~BSDF_SPECULAR); the same 12 words out
template <class REC>
__device__ __forceinline__ void check_lobes(int64_t n, const float *__restrict__ x, const REC *__restrict__ table,
                                            int n_table, float *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *r = x + 11 * i;
    const int k = (int)r[8];
    float *o = y + 12 * i;
    for (int j = 0; j < 12; ++j) o[j] = 0.f;
    if (k < 0 || k >= n_table) return;
    const REC &m = table[k];  // read in place: its lobes are indexed at run time
    const int mode = r[9] != 0.f ? kModeRadiance : kModeImportance;
    const int flags = r[10] != 0.f ? kBsdfNonSpecular : kBsdfAll;
    PTri q{};
    q.ss = mk(1.f, 0.f, 0.f);
    q.ts = mk(0.f, 1.f, 0.f);
    q.n = mk(0.f, 0.f, 1.f);
    const f3 wo = mk(r[0], r[1], r[2]), wi2 = mk(r[5], r[6], r[7]);
    f3 wi = mk(0.f, 0.f, 0.f);
    float pdf = 0.f, f[3];
    int type;
    if (bsdfn_sample(q, m, wo, r[3], r[4], flags, mode, wi, pdf, f, type)) {
        o[0] = wi.x;
        o[1] = wi.y;
        o[2] = wi.z;
        o[3] = pdf;
        o[4] = f[0];
        o[5] = f[1];
        o[6] = f[2];
        o[7] = __int_as_float(type);
    }
    bsdfn_f(q, m, wo, wi2, flags, mode, f);
    o[8] = f[0];
    o[9] = f[1];
    o[10] = f[2];
    o[11] = bsdfn_pdf(q, m, wo, wi2, flags);
}

__global__ __launch_bounds__(256) void k_check_lobes(int64_t n, const float *__restrict__ x,
                                                     const DevLobes *__restrict__ table, int n_table,
                                                     float *__restrict__ y) {
    check_lobes(n, x, table, n_table, y);
}
// ... over the wide lists of a table that holds a mix
__global__ __launch_bounds__(256) void k_check_lobes_mx(int64_t n, const float *__restrict__ x,
                                                        const DevLobesMx *__restrict__ table, int n_table,
                                                        float *__restrict__ y) {
    check_lobes(n, x, table, n_table, y);
}

}  // namespace

hipError_t launch_check_lobes_mx(int64_t n, const float *x, const DevLobesMx *table, int n_table, float *y,
                                 hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_check_lobes_mx, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, s, n, x, table, n_table, y);
    return hipGetLastError();
}

hipError_t launch_check_lobes(int64_t n, const float *x, const DevLobes *table, int n_table, float *y, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_check_lobes, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, s, n, x, table, n_table, y);
    return hipGetLastError();
}

hipError_t launch_check_bsdf(int64_t n, const float *x, const DevBsdf *table, int n_table, float *y, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_check_bsdf, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, s, n, x, table, n_table, y);
    return hipGetLastError();
}

hipError_t launch_check_specular(int64_t n, const float *x, float *y, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_check_specular, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, s, n, x, y);
    return hipGetLastError();
}

// outputs per input: 1 for kinds 0, 1, 3; 2 for kinds 2 and 4; 4 for kind 9
hipError_t launch_device_check(int kind, int64_t n, const float *x, int n_aux, const float *aux, float *y,
                               hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_check, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, s, kind, n, x, n_aux, aux, y);
    return hipGetLastError();
}

}  // namespace bre
