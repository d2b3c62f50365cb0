// bre_trace.h — scene evaluation for the on-device photon and camera passes (host + device).
//
// Float arithmetic follows the reference's operation order (see the file:line next to each
// function) and is compiled without FMA contraction, with correctly rounded division and sqrt,
// and with the transcendentals of include/bre_fmath.h, so a photon path on the GPU takes the
// same random decisions and produces the same beam bits as the CPU restatement in oracle/.
#pragma once

#include "../../include/bre_fmath.h"
#include "../../include/bre_scene.h"
#include "bre_math.h"
#include "bre_views.h"

#include <type_traits>
#include <vector>

namespace bre {

#define BRE_TD __host__ __device__ __forceinline__

constexpr float kPi = 3.14159265358979323846f;
constexpr float kInvPi = 0.31830988618379067154f;
constexpr float kInv4Pi = 0.07957747154594766788f;
constexpr float kPiOver2 = 1.57079632679489661923f;
constexpr float kPiOver4 = 0.78539816339744830961f;
constexpr float kOneMinusEps = 0x1.fffffep-1f;
constexpr float kMaxFloat = 3.402823466e+38f;

// gamma(n) of pbrt.h:263-265 in float
BRE_TD float gamma_n(int n) {
    const float eps = 0x1p-24f;
    return (n * eps) / (1 - n * eps);
}

// ---- PCG32 as pbrt seeds and uses it (rng.h:78-85, 129-144) ----
struct Pcg {
    uint64_t state, inc;
};
BRE_TD uint32_t pcg_next(Pcg &r) {
    const uint64_t old = r.state;
    r.state = old * 0x5851f42d4c957f2dULL + r.inc;
    const uint32_t xs = (uint32_t)(((old >> 18u) ^ old) >> 27u);
    const uint32_t rot = (uint32_t)(old >> 59u);
    return (xs >> rot) | (xs << ((~rot + 1u) & 31));
}
BRE_TD void pcg_seed(Pcg &r, uint64_t seq) {
    r.state = 0u;
    r.inc = (seq << 1u) | 1u;
    (void)pcg_next(r);
    r.state += 0x853c49e6748fea9bULL;
    (void)pcg_next(r);
}
BRE_TD float pcg_float(Pcg &r) {
    return smin(kOneMinusEps, (float)pcg_next(r) * 0x1p-32f);  // std::min(OneMinusEpsilon, .)
}
// Get2D of the reference's samplers: Point2f(Get1D(), Get1D()) built by g++ right to left
// (photonbeam.cpp:207-212, 239-241), so x is the second draw.
BRE_TD void pcg_2d(Pcg &r, float &x, float &y) {
    const float first = pcg_float(r);
    const float second = pcg_float(r);
    x = second;
    y = first;
}

// ---- vector helpers (geometry.h) ----
BRE_TD f3 neg3(f3 a) { return mk(-a.x, -a.y, -a.z); }
BRE_TD f3 abs3(f3 a) { return mk(fabsf(a.x), fabsf(a.y), fabsf(a.z)); }
BRE_TD f3 normalize3(f3 v) { return div3(v, len3(v)); }
BRE_TD f3 ray_at(f3 o, f3 d, float t) { return add3(o, scale3(d, t)); }
// CoordinateSystem, geometry.h:1020-1027
BRE_TD void coord_system(f3 v1, f3 &v2, f3 &v3) {
    if (fabsf(v1.x) > fabsf(v1.y))
        v2 = div3(mk(-v1.z, 0, v1.x), sqrtf(v1.x * v1.x + v1.z * v1.z));
    else
        v2 = div3(mk(0, v1.z, -v1.y), sqrtf(v1.y * v1.y + v1.z * v1.z));
    v3 = cross3d(v1, v2);
}
BRE_TD float next_up(float v) {
    if (v == __builtin_huge_valf()) return v;
    if (v == -0.f) v = 0.f;
    uint32_t ui = bre_f2u(v);
    if (v >= 0) ++ui;
    else --ui;
    return bre_u2f(ui);
}
BRE_TD float next_down(float v) {
    if (v == -__builtin_huge_valf()) return v;
    if (v == 0.f) v = -0.f;
    uint32_t ui = bre_f2u(v);
    if (v > 0) --ui;
    else ++ui;
    return bre_u2f(ui);
}
// OffsetRayOrigin, geometry.h:1438-1458
BRE_TD f3 offset_origin(f3 p, f3 perr, f3 n, f3 w) {
    const float d = dot3(abs3(n), perr);
    f3 off = scale3(n, d);
    if (dot3(w, n) < 0) off = neg3(off);
    f3 po = add3(p, off);
    po.x = off.x > 0 ? next_up(po.x) : (off.x < 0 ? next_down(po.x) : po.x);
    po.y = off.y > 0 ? next_up(po.y) : (off.y < 0 ? next_down(po.y) : po.y);
    po.z = off.z > 0 ? next_up(po.z) : (off.z < 0 ? next_down(po.z) : po.z);
    return po;
}

// ---- sampling (sampling.cpp:113-133, sampling.h:159-165) ----
// ConcentricSampleDisk, sampling.cpp:113-133
BRE_TD void concentric_disk(float ux, float uy, float &dx, float &dy) {
    const float ox = 2.f * ux - 1, oy = 2.f * uy - 1;
    dx = 0;
    dy = 0;
    if (!(ox == 0 && oy == 0)) {
        float theta, r;
        if (fabsf(ox) > fabsf(oy)) {
            r = ox;
            theta = kPiOver4 * (oy / ox);
        } else {
            r = oy;
            theta = kPiOver2 - kPiOver4 * (ox / oy);
        }
        float s, c;
        bre_sincosf(theta, &s, &c);
        dx = c * r;
        dy = s * r;
    }
}
// CosineSampleHemisphere, sampling.h:159-165
BRE_TD f3 cosine_hemisphere(float ux, float uy) {
    float dx, dy;
    concentric_disk(ux, uy, dx, dy);
    return mk(dx, dy, sqrtf(smax(0.f, 1 - dx * dx - dy * dy)));
}

// ---- Henyey-Greenstein Sample_p (medium.cpp:194-213); the returned pdf is unused here ----
BRE_TD f3 hg_sample(float g, f3 wo, float u0, float u1) {
    float cos_t;
    if ((double)fabsf(g) < 1e-3) {  // std::abs(g) < 1e-3 compares in double
        cos_t = 1 - 2 * u0;
    } else {
        const float sq = (1 - g * g) / (1 - g + 2 * g * u0);
        cos_t = (1 + g * g - sq * sq) / (2 * g);
    }
    const float sin_t = sqrtf(smax(0.f, 1 - cos_t * cos_t));
    const float phi = 2 * kPi * u1;
    f3 v1, v2;
    coord_system(wo, v1, v2);
    float sp, cp;
    bre_sincosf(phi, &sp, &cp);
    // SphericalDirection(sinT, cosT, phi, v1, v2, -wo), geometry.h:1465-1470
    return add3(add3(scale3(v1, sin_t * cp), scale3(v2, sin_t * sp)), scale3(neg3(wo), cos_t));
}

// ---- scene on the device: pbrt Triangles (include/bre_scene.h) ----
struct PTri {
    f3 p0, p1, p2;
    f3 n;        // Triangle::Intersect's normal: normalize(cross(p0 - p2, p1 - p2)), negated if flip
    f3 ss, ts;   // BSDF frame: ss = normalize(dpdu), ts = cross(ns, ss)
    f3 ns;       // Triangle::Sample's normal: normalize(cross(p1 - p0, p2 - p0)), negated if flip
    float kd[3], Le[3];
    float area;  // 0.5 * |cross(p1 - p0, p2 - p0)|
    int mat;     // kMatMatte: Lambertian kd; kMatNone: no BxDF (black kd, or a black mirror / glass);
                 // kMatTable + k: entry k of DevScene::mats; kMatInterface: no BSDF
    int emit;    // a DiffuseAreaLight
};
constexpr int kMatMatte = 0, kMatNone = 1, kMatTable = 2;
constexpr int kMatInterface = -1;  // BRE_MATERIAL_INTERFACE: no BSDF at all, the walks pass through

// BxDFType bits (reflection.h:126-134) of the lobes sampled here
constexpr int kBsdfReflection = 1, kBsdfTransmission = 2, kBsdfDiffuse = 4, kBsdfGlossy = 8, kBsdfSpecular = 16;
constexpr int kModeImportance = 0, kModeRadiance = 1;  // TransportMode of a specular_sample call

// The specular materials on the device are the context's bre_material records (Kr, Kt clamped)
static_assert(sizeof(bre_material) == 32, "bre_material has no padding: the geometry cache compares its bytes");
static_assert(sizeof(bre_material_ex) == 112, "bre_material_ex has no padding: the geometry cache compares its bytes");

// A plastic, metal or matte table entry (bre_material_ex, type >= BRE_MATERIAL_MATTE) as its material's
// ComputeScatteringFunctions leaves the BSDF (make_bsdf): the BxDFs added, in the order added, and what they hold.
// An entry of the narrow kinds has type 0 here (its record is DevScene::mats[k]).
constexpr int kLobeDiffuse = 1, kLobeMicro = 2;
struct DevBsdf {
    int type;             // BRE_MATERIAL_MATTE / _PLASTIC / _METAL, or 0
    int lobes;            // kLobeDiffuse (first), kLobeMicro (second)
    float kd[3];          // LambertianReflection / OrenNayar R
    float ks[3];          // MicrofacetReflection R (metal: 1)
    float ceta[3], ck[3]; // metal: FresnelConductor(1, eta, k); plastic: FresnelDielectric(1.5, 1)
    float ax, ay;         // TrowbridgeReitzDistribution alphax, alphay (RoughnessToAlpha applied on the host)
    float A, B;           // OrenNayar's constants
    int oren;             // the diffuse lobe is an OrenNayar
    int conductor;        // the microfacet lobe's Fresnel term is the conductor's
};

// The BSDF of any number of lobes (a table that holds a rough glass, uber, translucent or substrate entry): every
// entry from BRE_MATERIAL_MATTE up as its ComputeScatteringFunctions leaves the BSDF (make_lobes), the BxDFs in the
// order added.  BSDF::eta is read nowhere in photonbeam.cpp and has no place here.  The kernels read a record
// where it lies in device memory (a lobe is indexed at run time: a copy in registers would go to scratch).
constexpr int kBsdfAll = 31;                             // BSDF_ALL, reflection.h:128-129
constexpr int kBsdfNonSpecular = 31 & ~kBsdfSpecular;    // EstimateDirect's BSDF_ALL & ~BSDF_SPECULAR
constexpr int kMaxLobes = 5;                             // uber.cpp adds at most five
enum LobeKind : int {
    kLobeLambertR = 1,  // LambertianReflection(c)
    kLobeLambertT,      // LambertianTransmission(c)
    kLobeOren,          // OrenNayar(c), A = ax, B = ay
    kLobeMicroR,        // MicrofacetReflection(c, TR(ax, ay), FresnelDielectric(etaA, etaB))
    kLobeMicroRC,       // MicrofacetReflection(c, TR(ax, ay), FresnelConductor(1, s, t))
    kLobeMicroT,        // MicrofacetTransmission(c, TR(ax, ay), etaA, etaB, mode)
    kLobeSpecR,         // SpecularReflection(c, FresnelDielectric(etaA, etaB))
    kLobeSpecT,         // SpecularTransmission(c, etaA, etaB, mode)
    kLobeBlend          // FresnelBlend(Rd = c, Rs = s, TR(ax, ay))
};
struct DevLobe {
    int kind;         // LobeKind
    int type;         // its BxDFType bits
    float c[3];       // R or T: the product (op * Kd, r * ks, ...) formed on the host in the reference's operations
    float s[3], t[3]; // kLobeBlend: Rs; kLobeMicroRC: the conductor's eta and k
    float ax, ay;     // the distribution's alphas (RoughnessToAlpha applied on the host); kLobeOren: A, B
    float etaA, etaB;
};
struct DevLobes {
    int type;         // BRE_MATERIAL_MATTE .. _METAL, _ROUGH_GLASS .. _SUBSTRATE; 0: a mirror, glass or interface
    int n;            // BxDFs added
    int n_nonspec;    // NumComponents(BSDF_ALL & ~BSDF_SPECULAR)
    int pad;
    DevLobe lobe[kMaxLobes];
};

// The wide lobe list (a table that holds a BRE_MATERIAL_MIX): every entry from BRE_MATERIAL_MATTE up as above, and a
// mix as MixMaterial::ComputeScatteringFunctions leaves the BSDF (mixmat.cpp:51-63): the first child's BxDFs in order,
// then the second's, each a ScaledBxDF once per enclosing mix.  A lobe carries that chain of scales innermost first:
// ScaledBxDF::f is scale * bxdf->f in float, so a nest is s_outer * (s_inner * f), which is not (s_outer * s_inner) * f
// in bits: the scales are not multiplied on the host.  A scaled lobe's type and Pdf are its inner lobe's
// (reflection.h:230-232, reflection.cpp:108-110).  Under a mix a mirror and a smooth glass are lobes among others:
constexpr int kLobeSpecNoOp = kLobeBlend + 1;     // SpecularReflection(c, FresnelNoOp): mirror.cpp:50-56
constexpr int kLobeFresnelSpec = kLobeBlend + 2;  // FresnelSpecular(c, s, etaA, etaB, mode): glass.cpp:71-73
constexpr int kMaxLobesMx = BRE_MAX_BXDFS;
struct DevLobeMx : DevLobe {
    int nscale;                             // enclosing mixes: 0 for the own lobe of an entry that is no mix
    float scale[BRE_MAX_MIX_DEPTH][3];      // innermost first
};
struct DevLobesMx {
    int type;         // BRE_MATERIAL_MATTE .. _METAL, _ROUGH_GLASS .. _MIX; 0: a mirror, glass or interface
    int n;
    int n_nonspec;
    int pad;
    DevLobeMx lobe[kMaxLobesMx];
};

// One node of the scene's bounding volume hierarchy: the reference's BVHAccel LinearBVHNode
// (src/accelerators/bvh.cpp, 32 B, depth-first order: an interior node's first child follows it).
struct SceneNode {
    float lo[3], hi[3];  // Bounds3f
    int32_t offset;      // leaf: primitivesOffset; interior: secondChildOffset
    uint16_t nprims;     // 0 for an interior node
    uint8_t axis;        // interior: split axis
    uint8_t pad;
};
static_assert(sizeof(SceneNode) == 32, "SceneNode is BVHAccel's 32-B LinearBVHNode");
constexpr int kSceneStack = 64;  // BVHAccel::Intersect's nodesToVisit[64]: the deepest tree accepted

// A delta light (bre_light: PointLight, src/lights/point.cpp; SpotLight, src/lights/spot.cpp) as its
// constructor leaves it: pLight = LightToWorld(Point3f(0, 0, 0)), the 3x3 blocks of LightToWorld and
// WorldToLight (vectors only ever go through them), I, and the two cosines (host, bre_fmath.h).
// A DistantLight (src/lights/distant.cpp) is the same record read differently, after its constructor and its
// Preprocess: p = worldCenter, l2w[0..2] = wLight, l2w[3] = worldRadius (Scene::WorldBound().BoundingSphere),
// I = L; it has no matrices and no cone.
static_assert(sizeof(bre_light) == 156, "bre_light has no padding: the geometry cache compares its bytes");
constexpr int kLightPoint = 0, kLightSpot = 1, kLightDistant = 2;
struct DLight {
    f3 p;
    float l2w[9], w2l[9];  // row-major
    float I[3];
    float cos_total, cos_start;  // cosTotalWidth, cosFalloffStart
    int kind;                    // kLightPoint / kLightSpot / kLightDistant
};

// A medium as the HomogeneousMedium / GridDensityMedium constructors leave it (make_medium): the scene's own
// (DevScene::own, from the bre_scene fields) or an entry of the context's media table (from a bre_medium).
static_assert(sizeof(bre_medium) == 120, "bre_medium has no padding: the pointer is part of the layout");
struct DevMedium {
    int medium;  // BRE_MEDIUM_HOMOGENEOUS / _GRID; BRE_MEDIUM_NONE only in DevScene::own
    float sigma_t[3];
    float g;
    // GridDensityMedium (grid.h:50-80): sigma_t = (sigma_a + sigma_s)[0], invMaxDensity
    int gn[3];
    float grid_sigma_t, grid_inv_max;
    float w2m[16];         // WorldToMedium, row-major
    const float *density;  // device copy of the grid (nx*ny*nz)
};

struct DevScene {
    int n_tris, n_lights, n_nodes, stack_depth;  // stack_depth: traversal stack entries per thread (the tree depth)
    DevMedium own;                               // the scene's one medium (bre_scene.has_medium; own.medium == 0: none)
    // the triangles in scene order, the BVHAccel over them (nodes + primitive order) and
    // scene.lights (the emitting triangles and the context's delta lights, merged by bre_light.order)
    // with the Distribution1D of their Power().y()
    // (ComputeLightPowerDistribution, integrator.cpp:217-225; sampling.h:55-69): device arrays
    const PTri *t;
    const SceneNode *nodes;
    const int32_t *prims;       // BVH primitive slot -> triangle index
    const int32_t *light_tri;   // per light: >= 0 the emitting triangle, < 0 the delta light ~value of dlights
    const DLight *dlights;
    const float *light_func;
    const float *light_cdf;     // n_lights + 1
    float light_func_int;
    const bre_material *mats; // the mirror / glass table a PTri::mat >= kMatTable refers to (device array)
    // bre_set_media (null / 0 without): the table, per triangle its (inside, outside) pair of table indices
    // (-1: vacuum), per delta light its medium, and the camera's
    const DevMedium *media;
    const int32_t *tri_med;    // 2 * n_tris
    const int32_t *light_med;  // one per entry of dlights
    int n_media, cam_med;
    const DevBsdf *bsdfs;  // beside mats, one per table entry (bre_set_materials_ex); last: the layout before it stays
    const DevLobes *lobes; // beside bsdfs, one per table entry; read only by the kernels of a table with a type >= 8
    const DevLobesMx *lobes_mx; // one per table entry, only where the table holds a BRE_MATERIAL_MIX (else null): read
                                // by the tier-3 kernels instead of lobes
};

// Host side of the scene: everything prepare_geometry derives, in host memory; the context uploads
// the arrays and points the DevScene at them.
struct HostScene {
    DevScene head;  // scalars; the array pointers are filled after the upload
    std::vector<PTri> tris;
    std::vector<SceneNode> nodes;
    std::vector<int32_t> prims;
    std::vector<int32_t> light_tri;
    std::vector<DLight> dlights;
    std::vector<float> light_func, light_cdf;
    std::vector<bre_material> mats;
    std::vector<DevBsdf> bsdfs;
    std::vector<DevLobes> lobes;
    std::vector<DevLobesMx> lobes_mx;
    int depth = 0;  // deepest node of the BVH (root = 1)
};

// The context's materials (bre_set_materials, bre_set_materials_ex): the table and the per-triangle index (-1: matte)
struct MaterialMap {
    const bre_material_ex *mats = nullptr;
    int n_mats = 0;
    const int32_t *tri_mat = nullptr;  // one per scene triangle when n_mats > 0
};

// host (bre_scene.hip): derive the per-triangle constants, the light distribution and the scene BVH exactly
// as oracle/ora_pbrt.h make_scene does: out->head's geometry fields and the arrays
// (`lights`: the context's delta lights, each with order <= s->n_triangles; `mm`: its materials, the map
// holding s->n_triangles entries)
void prepare_geometry(const bre_scene *s, HostScene *out, const bre_light *lights = nullptr, int n_lights = 0,
                      const MaterialMap &mm = MaterialMap());
// a bre_light as the PointLight / SpotLight constructor leaves it
DLight prepare_light(const bre_light &l);
// a table entry as its material leaves the BSDF (plastic.cpp:45-70, metal.cpp:59-80, matte.cpp:45-62); type 0 for
// a mirror, glass or interface
DevBsdf make_bsdf(const bre_material_ex &m);
// a table entry as its material leaves the BSDF, any number of lobes: the above for types 4 .. 6, and glass.cpp:45-92,
// uber.cpp:45-101, translucent.cpp:45-80, substrate.cpp:45-65 for types 8 .. 11; type 0 below BRE_MATERIAL_MATTE
DevLobes make_lobes(const bre_material_ex &m);
// the wide lists of a checked table that holds a mix (children before their mix, the expansions within kMaxLobesMx):
// entry k as make_lobes leaves it with no scale, a mix as mixmat.cpp:51-63 leaves it, type 0 for the others
void make_lobes_mx(const bre_material_ex *table, int n, std::vector<DevLobesMx> *out);
// a medium as its constructor leaves it: sigma_t = sigma_a + sigma_s per channel; for a grid, channel 0 of it,
// 1 / max_density and `d_density`, the device copy of the grid (the grid arguments are not read otherwise)
DevMedium make_medium(int type, const float sigma_a[3], const float sigma_s[3], float g, const int32_t grid_n[3],
                      const float world_to_medium[16], const float *d_density, float max_density);
void prepare_medium(const bre_scene *s, DevScene *d, const float *d_density);  // d->own, from s's medium fields
// host: the scene's BVHAccel (bvh.cpp: SAH, 12 buckets, maxPrimsInNode 4, depth-first layout) over
// the triangles' world bounds; returns the tree depth
int build_scene_bvh(const std::vector<PTri> &tris, std::vector<SceneNode> *nodes, std::vector<int32_t> *prims);
// the scene's triangle array: the inline one or triangles_ext (bre_scene.h)
inline const bre_triangle *scene_triangles(const bre_scene *s) { return s->triangles_ext ? s->triangles_ext : s->triangles; }
// host: GridDensityMedium ctor's maxDensity loop (grid.h:73-76), std::max order; of the scene's grid
float max_density(const float *density, int64_t n);
float grid_max_density(const bre_scene *s);

struct Hit {
    f3 p, perr;
    int tri;
};

BRE_TD int max_dim(f3 v) { return (v.x > v.y) ? ((v.x > v.z) ? 0 : 2) : ((v.y > v.z) ? 1 : 2); }
BRE_TD float comp(f3 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : v.z); }
BRE_TD f3 permute3(f3 v, int x, int y, int z) { return mk(comp(v, x), comp(v, y), comp(v, z)); }
BRE_TD float max_comp(f3 v) { return smax(v.x, smax(v.y, v.z)); }

// Triangle::Intersect, triangle.cpp:177-300: the watertight test (translate to the ray origin,
// permute so |d| is largest in z, shear, edge functions with a double-precision fallback on zero,
// scaled t against tMax, conservative t > deltaT), then the barycentric hit point and its error bound
__device__ __forceinline__ bool intersect_tri(const PTri &T, f3 o, f3 dir, float tmax, float &t, Hit &h) {
    f3 p0t = sub3(T.p0, o), p1t = sub3(T.p1, o), p2t = sub3(T.p2, o);
    const int kz = max_dim(abs3(dir));
    int kx = kz + 1;
    if (kx == 3) kx = 0;
    int ky = kx + 1;
    if (ky == 3) ky = 0;
    const f3 d = permute3(dir, kx, ky, kz);
    p0t = permute3(p0t, kx, ky, kz);
    p1t = permute3(p1t, kx, ky, kz);
    p2t = permute3(p2t, kx, ky, kz);
    const float Sx = -d.x / d.z, Sy = -d.y / d.z, Sz = 1.f / d.z;
    p0t.x += Sx * p0t.z;
    p0t.y += Sy * p0t.z;
    p1t.x += Sx * p1t.z;
    p1t.y += Sy * p1t.z;
    p2t.x += Sx * p2t.z;
    p2t.y += Sy * p2t.z;
    float e0 = p1t.x * p2t.y - p1t.y * p2t.x;
    float e1 = p2t.x * p0t.y - p2t.y * p0t.x;
    float e2 = p0t.x * p1t.y - p0t.y * p1t.x;
    if (e0 == 0.0f || e1 == 0.0f || e2 == 0.0f) {
        e0 = (float)((double)p2t.y * (double)p1t.x - (double)p2t.x * (double)p1t.y);
        e1 = (float)((double)p0t.y * (double)p2t.x - (double)p0t.x * (double)p2t.y);
        e2 = (float)((double)p1t.y * (double)p0t.x - (double)p1t.x * (double)p0t.y);
    }
    if ((e0 < 0 || e1 < 0 || e2 < 0) && (e0 > 0 || e1 > 0 || e2 > 0)) return false;
    const float det = e0 + e1 + e2;
    if (det == 0) return false;
    p0t.z *= Sz;
    p1t.z *= Sz;
    p2t.z *= Sz;
    const float tScaled = e0 * p0t.z + e1 * p1t.z + e2 * p2t.z;
    if (det < 0 && (tScaled >= 0 || tScaled < tmax * det)) return false;
    if (det > 0 && (tScaled <= 0 || tScaled > tmax * det)) return false;
    const float invDet = 1 / det;
    const float b0 = e0 * invDet, b1 = e1 * invDet, b2 = e2 * invDet;
    t = tScaled * invDet;
    const float maxZt = max_comp(abs3(mk(p0t.z, p1t.z, p2t.z)));
    const float deltaZ = gamma_n(3) * maxZt;
    const float maxXt = max_comp(abs3(mk(p0t.x, p1t.x, p2t.x)));
    const float maxYt = max_comp(abs3(mk(p0t.y, p1t.y, p2t.y)));
    const float deltaX = gamma_n(5) * (maxXt + maxZt);
    const float deltaY = gamma_n(5) * (maxYt + maxZt);
    const float deltaE = 2 * (gamma_n(2) * maxXt * maxYt + deltaY * maxXt + deltaX * maxYt);
    const float maxE = max_comp(abs3(mk(e0, e1, e2)));
    const float deltaT = 3 * (gamma_n(3) * maxE * maxZt + deltaE * maxZt + deltaZ * maxE) * fabsf(invDet);
    if (t <= deltaT) return false;
    const float xs = fabsf(b0 * T.p0.x) + fabsf(b1 * T.p1.x) + fabsf(b2 * T.p2.x);
    const float ys = fabsf(b0 * T.p0.y) + fabsf(b1 * T.p1.y) + fabsf(b2 * T.p2.y);
    const float zs = fabsf(b0 * T.p0.z) + fabsf(b1 * T.p1.z) + fabsf(b2 * T.p2.z);
    h.perr = scale3(mk(xs, ys, zs), gamma_n(7));
    h.p = add3(add3(scale3(T.p0, b0), scale3(T.p1, b1)), scale3(T.p2, b2));
    return true;
}

// Scene::Intersect = BVHAccel::Intersect (bvh.cpp): depth-first through the scene BVH, near child
// first by dirIsNeg[axis], every node tested with the reference's slab test against the CURRENT
// tMax, every leaf triangle with Triangle::Intersect, each hit shrinking tMax (primitive.cpp:97-101).
// The triangles are tested in the reference's order, so among equal-t hits the same one wins.  The
// stack lives in the kernel's dynamic LDS (entry k of thread t at [k * blockDim.x + t]), sized by
// the launch to the tree's depth (scene_stack_bytes): it holds at most one entry per level of the
// current path.  The host rejects trees deeper than kSceneStack (upload_scene).
__device__ __forceinline__ bool intersect_scene(const DevScene &S, f3 o, f3 d, float &tmax, Hit &h) {
    extern __shared__ int bre_scene_stack[];
    int *stack = bre_scene_stack + threadIdx.x;
    const int stride = blockDim.x;
    const f3 inv = mk(1 / d.x, 1 / d.y, 1 / d.z);
    const int n0 = inv.x < 0, n1 = inv.y < 0, n2 = inv.z < 0;
    int sp = 0, cur = 0;
    bool hit = false;
    while (true) {
        const SceneNode &nd = S.nodes[cur];
        const Box6 b{nd.lo[0], nd.lo[1], nd.lo[2], nd.hi[0], nd.hi[1], nd.hi[2]};
        if (slab_test(b, o, inv, n0, n1, n2, tmax, nullptr)) {
            if (nd.nprims > 0) {
                for (int i = 0; i < nd.nprims; ++i) {
                    const int ti = S.prims[nd.offset + i];
                    float t;
                    Hit tmp;
                    if (!intersect_tri(S.t[ti], o, d, tmax, t, tmp)) continue;
                    tmax = t;
                    h.p = tmp.p;
                    h.perr = tmp.perr;
                    h.tri = ti;
                    hit = true;
                }
                if (sp == 0) break;
                cur = stack[--sp * stride];
            } else {
                const int neg = nd.axis == 0 ? n0 : (nd.axis == 1 ? n1 : n2);
                stack[sp++ * stride] = neg ? cur + 1 : nd.offset;
                cur = neg ? nd.offset : cur + 1;
            }
        } else {
            if (sp == 0) break;
            cur = stack[--sp * stride];
        }
    }
    return hit;
}

// Triangle::Sample(u, pdf), triangle.cpp:543-568, with UniformSampleTriangle
struct ShapeSample {
    f3 p, perr, n;
    float pdf;
};
BRE_TD ShapeSample sample_tri(const PTri &T, float u0, float u1) {
    ShapeSample r;
    const float su0 = sqrtf(u0);
    const float b0 = 1 - su0, b1 = u1 * su0;
    const float b2 = 1 - b0 - b1;
    const f3 a = scale3(T.p0, b0), b = scale3(T.p1, b1), c = scale3(T.p2, b2);
    r.p = add3(add3(a, b), c);
    r.n = T.ns;
    r.perr = scale3(add3(add3(abs3(a), abs3(b)), abs3(c)), gamma_n(6));
    r.pdf = 1 / T.area;
    return r;
}

// FindInterval, pbrt.h:377-389: bisection for the last index with pred true, then
// Clamp(first - 1, 0, size - 2) (pbrt.h:278-284: the low bound is tested first)
template <typename Pred>
BRE_TD int find_interval(int size, const Pred &pred) {
    int first = 0, len = size;
    while (len > 0) {
        const int half = len >> 1, middle = first + half;
        if (pred(middle)) {
            first = middle + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    const int v = first - 1;
    return v < 0 ? 0 : (v > size - 2 ? size - 2 : v);
}

// Distribution1D::SampleDiscrete with FindInterval (sampling.h:90-100, pbrt.h:377-389) over the
// light powers; returns the light index (into light_tri)
BRE_TD int sample_light(const DevScene &S, float u, float &pdf) {
    const float *cdf = S.light_cdf;
    const int off = find_interval(S.n_lights + 1, [&](int i) { return cdf[i] <= u; });
    pdf = (S.light_func_int > 0) ? S.light_func[off] / (S.light_func_int * (float)S.n_lights) : 0.f;
    return off;
}

// ---- delta lights (src/lights/point.cpp, src/lights/spot.cpp) ----
// Transform::operator()(Vector3f) through a 3x3 block, transform.h:236-242
BRE_TD f3 xform_vec3(const float *m, f3 v) {
    return mk(m[0] * v.x + m[1] * v.y + m[2] * v.z, m[3] * v.x + m[4] * v.y + m[5] * v.z,
              m[6] * v.x + m[7] * v.y + m[8] * v.z);
}
// SpotLight::Falloff, spot.cpp:64-73 (a PointLight has none: 1)
BRE_TD float light_falloff(const DLight &D, f3 w) {
    if (D.kind != kLightSpot) return 1.f;
    const float cos_t = normalize3(xform_vec3(D.w2l, w)).z;
    if (cos_t < D.cos_total) return 0.f;
    if (cos_t > D.cos_start) return 1.f;
    const float delta = (cos_t - D.cos_total) / (D.cos_start - D.cos_total);
    return (delta * delta) * (delta * delta);
}
// Sample_Le of a delta light from uLight0 (point.cpp:61-71: UniformSampleSphere, sampling.cpp:98-103;
// spot.cpp:83-93: UniformSampleCone and UniformConePdf, sampling.cpp:132-142).  The ray starts at
// D.p; d is not normalised (a spot's goes through LightToWorld); nLight = d, pdfPos = 1.
// A DistantLight's (distant.cpp:69-85) starts on the disk of the world's bounding sphere that faces wLight, pushed
// out by worldRadius along wLight, without an offset (no SpawnRay): d = -wLight, pdfPos = 1 / (Pi r^2), pdfDir = 1.
BRE_TD f3 distant_w(const DLight &D) { return mk(D.l2w[0], D.l2w[1], D.l2w[2]); }
BRE_TD float distant_radius(const DLight &D) { return D.l2w[3]; }
BRE_TD void light_sample_le(const DLight &D, float u0, float u1, f3 &o, f3 &d, float &pdf_pos, float &pdf_dir,
                            float &fo) {
    float s, c;
    o = D.p;
    pdf_pos = 1.f;
    if (D.kind == kLightDistant) {
        const f3 wl = distant_w(D);
        const float r = distant_radius(D);
        f3 v1, v2;
        coord_system(wl, v1, v2);
        float cx, cy;
        concentric_disk(u0, u1, cx, cy);
        const f3 p_disk = add3(D.p, scale3(add3(scale3(v1, cx), scale3(v2, cy)), r));
        o = add3(p_disk, scale3(wl, r));
        d = neg3(wl);
        pdf_pos = 1 / (kPi * r * r);
        pdf_dir = 1.f;
        fo = 1.f;
        return;
    }
    if (D.kind == kLightSpot) {
        const float cos_t = (1.f - u0) + u0 * D.cos_total;
        const float sin_t = sqrtf(1.f - cos_t * cos_t);
        const float phi = u1 * 2 * kPi;
        bre_sincosf(phi, &s, &c);
        d = xform_vec3(D.l2w, mk(c * sin_t, s * sin_t, cos_t));
        pdf_dir = 1 / (2 * kPi * (1 - D.cos_total));
    } else {
        const float z = 1 - 2 * u0;
        const float r = sqrtf(smax(0.f, 1.f - z * z));
        const float phi = 2 * kPi * u1;
        bre_sincosf(phi, &s, &c);
        d = mk(r * c, r * s, z);
        pdf_dir = kInv4Pi;
    }
    fo = light_falloff(D, d);
}

// Sampler draws: the photon pass draws from PCG32 (AwesomeHaltonSampler past its 1000 Halton
// dimensions); the camera pass overloads smp_1d for its AwesomeSampler (bre_camera.hip).
__device__ __forceinline__ float smp_1d(Pcg &r) { return pcg_float(r); }

// HomogeneousMedium::Tr, homogeneous.cpp:44-48
__device__ __forceinline__ void medium_tr(const DevMedium &S, f3 d, float tmax, float tr[3]) {
    const float x = smin(tmax * len3(d), kMaxFloat);
    // one expf per distinct argument (a grey medium's three channels share theirs: the same values)
    const float a0 = -S.sigma_t[0] * x, a1 = -S.sigma_t[1] * x, a2 = -S.sigma_t[2] * x;
    tr[0] = bre_expf(a0);
    tr[1] = a1 == a0 ? tr[0] : bre_expf(a1);
    tr[2] = a2 == a1 ? tr[1] : bre_expf(a2);
}

// HomogeneousMedium::Sample distance part, homogeneous.cpp:50-60 (two draws)
template <class Smp>
__device__ __forceinline__ bool medium_sample(const DevMedium &S, Smp &rng, f3 d, float tmax, float &t) {
    int ch = (int)(smp_1d(rng) * 3);
    ch = (2 < ch) ? 2 : ch;  // std::min(ch, 2)
    const float st = ch == 0 ? S.sigma_t[0] : (ch == 1 ? S.sigma_t[1] : S.sigma_t[2]);
    const float dist = -bre_logf(1 - smp_1d(rng)) / st;
    t = smin(dist * len3(d), tmax);
    return t < tmax;
}

// ---- GridDensityMedium (src/media/grid.{h,cpp}) ----
BRE_TD float lerp_ref(float t, float v1, float v2) { return (1 - t) * v1 + t * v2; }  // pbrt.h:391

// GridDensityMedium::D, grid.h:84-88 (0 outside [0, n) per axis)
__device__ __forceinline__ float grid_D(const DevMedium &S, int x, int y, int z) {
    if (!(x >= 0 && x < S.gn[0] && y >= 0 && y < S.gn[1] && z >= 0 && z < S.gn[2])) return 0.f;
    return S.density[((int64_t)z * S.gn[1] + y) * S.gn[0] + x];
}

// GridDensityMedium::Density, grid.cpp:46-60: trilinear over the sample lattice at cell centres
__device__ __forceinline__ float grid_density(const DevMedium &S, f3 p) {
    const float sx = p.x * (float)S.gn[0] - .5f, sy = p.y * (float)S.gn[1] - .5f, sz = p.z * (float)S.gn[2] - .5f;
    const int ix = (int)floorf(sx), iy = (int)floorf(sy), iz = (int)floorf(sz);
    const float dx = sx - (float)ix, dy = sy - (float)iy, dz = sz - (float)iz;
    const float d00 = lerp_ref(dx, grid_D(S, ix, iy, iz), grid_D(S, ix + 1, iy, iz));
    const float d10 = lerp_ref(dx, grid_D(S, ix, iy + 1, iz), grid_D(S, ix + 1, iy + 1, iz));
    const float d01 = lerp_ref(dx, grid_D(S, ix, iy, iz + 1), grid_D(S, ix + 1, iy, iz + 1));
    const float d11 = lerp_ref(dx, grid_D(S, ix, iy + 1, iz + 1), grid_D(S, ix + 1, iy + 1, iz + 1));
    const float d0 = lerp_ref(dy, d00, d10);
    const float d1 = lerp_ref(dy, d01, d11);
    return lerp_ref(dz, d0, d1);
}

// WorldToMedium(Ray(o, Normalize(d), tMax * |d|)) (grid.cpp:66-67) through
// Transform::operator()(Ray) (transform.h:251-264, point with error bound :278-299, vector :236-242),
// then Bounds3f(0, 1)::IntersectP(ray, &t0, &t1) (geometry.h:1386-1408).  Returns false on a miss.
__device__ __forceinline__ bool grid_ray(const DevMedium &S, f3 o, f3 d, float tmax, f3 &mo, f3 &md, float &t0,
                                         float &t1) {
    const f3 dn = normalize3(d);
    const float tm = tmax * len3(d);
    const float *m = S.w2m;
    const float xp = m[0] * o.x + m[1] * o.y + m[2] * o.z + m[3];
    const float yp = m[4] * o.x + m[5] * o.y + m[6] * o.z + m[7];
    const float zp = m[8] * o.x + m[9] * o.y + m[10] * o.z + m[11];
    const float wp = m[12] * o.x + m[13] * o.y + m[14] * o.z + m[15];
    const float xs = fabsf(m[0] * o.x) + fabsf(m[1] * o.y) + fabsf(m[2] * o.z) + fabsf(m[3]);
    const float ys = fabsf(m[4] * o.x) + fabsf(m[5] * o.y) + fabsf(m[6] * o.z) + fabsf(m[7]);
    const float zs = fabsf(m[8] * o.x) + fabsf(m[9] * o.y) + fabsf(m[10] * o.z) + fabsf(m[11]);
    const float g3 = gamma_n(3);
    const f3 oerr = mk(g3 * xs, g3 * ys, g3 * zs);
    f3 po = mk(xp, yp, zp);
    if (!(wp == 1)) {
        const float inv = (float)1 / wp;
        po = mk(inv * xp, inv * yp, inv * zp);
    }
    const f3 dv = mk(m[0] * dn.x + m[1] * dn.y + m[2] * dn.z, m[4] * dn.x + m[5] * dn.y + m[6] * dn.z,
                     m[8] * dn.x + m[9] * dn.y + m[10] * dn.z);
    float rt = tm;
    const float l2 = lensq3(dv);
    if (l2 > 0) {
        const float dt = dot3(abs3(dv), oerr) / l2;
        po = add3(po, scale3(dv, dt));
        rt -= dt;
    }
    mo = po;
    md = dv;
    float a = 0, b = rt;
    const float pad = 1 + 2 * gamma_n(3);
    const float oo[3] = {po.x, po.y, po.z}, dd[3] = {dv.x, dv.y, dv.z};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float inv = 1 / dd[i];
        float tn = (0.f - oo[i]) * inv;
        float tf = (1.f - oo[i]) * inv;
        if (tn > tf) {
            const float x = tn;
            tn = tf;
            tf = x;
        }
        tf *= pad;
        a = tn > a ? tn : a;
        b = tf < b ? tf : b;
        if (a > b) return false;
    }
    t0 = a;
    t1 = b;
    return true;
}

// GridDensityMedium::Sample, grid.cpp:62-89: delta tracking.  On an interaction, t is the
// medium-space distance and the interaction point is rWorld(t) = o + d*t (as the reference).
template <class Smp>
__device__ __forceinline__ bool grid_sample(const DevMedium &S, Smp &smp, f3 o, f3 d, float tmax, float &t_out) {
    f3 mo, md;
    float tmin, tm;
    if (!grid_ray(S, o, d, tmax, mo, md, tmin, tm)) return false;
    float t = tmin;
    while (true) {
        t -= bre_logf(1 - smp_1d(smp)) * S.grid_inv_max / S.grid_sigma_t;
        if (t >= tm) break;
        if (grid_density(S, ray_at(mo, md, t)) * S.grid_inv_max > smp_1d(smp)) {
            t_out = t;
            return true;
        }
    }
    return false;
}

// GridDensityMedium::Tr, grid.cpp:91-118: ratio tracking with Russian roulette below 0.1
template <class Smp>
__device__ __forceinline__ float grid_tr(const DevMedium &S, Smp &smp, f3 o, f3 d, float tmax) {
    f3 mo, md;
    float tmin, tm;
    if (!grid_ray(S, o, d, tmax, mo, md, tmin, tm)) return 1.f;
    float tr = 1, t = tmin;
    while (true) {
        t -= bre_logf(1 - smp_1d(smp)) * S.grid_inv_max / S.grid_sigma_t;
        if (t >= tm) break;
        const float density = grid_density(S, ray_at(mo, md, t));
        tr *= 1 - smax(0.f, density * S.grid_inv_max);
        const float rr = 0.1f;
        if (tr < rr) {
            const float q = smax(0.05f, 1 - tr);
            if (smp_1d(smp) < q) return 0.f;
            tr /= 1 - q;
        }
    }
    return tr;
}

// Medium::Tr of the world ray (o, d, tmax) for either medium type
template <class Smp>
__device__ __forceinline__ void medium_tr_any(const DevMedium &S, Smp &smp, f3 o, f3 d, float tmax, float tr[3]) {
    if (S.medium == BRE_MEDIUM_GRID) {
        const float t = grid_tr(S, smp, o, d, tmax);
        tr[0] = tr[1] = tr[2] = t;
    } else {
        medium_tr(S, d, tmax, tr);
    }
}

// Medium::Sample distance decision; on true the interaction point is o + d*t
template <class Smp>
__device__ __forceinline__ bool medium_sample_any(const DevMedium &S, Smp &smp, f3 o, f3 d, float tmax, float &t) {
    if (S.medium == BRE_MEDIUM_GRID) return grid_sample(S, smp, o, d, tmax, t);
    return medium_sample(S, smp, d, tmax, t);
}

// ---- the medium a ray travels in.  MED false: the scene's one medium (S.own), `med` unused.  MED true
// (bre_set_media): entry `med` of S.media, or vacuum for -1: nothing is drawn and Tr = 1. ----
template <bool MED, class Smp>
__device__ __forceinline__ bool ray_medium_sample(const DevScene &S, int med, Smp &smp, f3 o, f3 d, float tmax,
                                                  float &t) {
    if constexpr (MED) return med >= 0 && medium_sample_any(S.media[med], smp, o, d, tmax, t);
    else return S.own.medium && medium_sample_any(S.own, smp, o, d, tmax, t);
}
// tr = Tr of the segment (1 in vacuum)
template <bool MED, class Smp>
__device__ __forceinline__ void ray_medium_tr(const DevScene &S, int med, Smp &smp, f3 o, f3 d, float tmax,
                                              float tr[3]) {
    tr[0] = tr[1] = tr[2] = 1.f;
    if constexpr (MED) {
        if (med >= 0) medium_tr_any(S.media[med], smp, o, d, tmax, tr);
    } else {
        if (S.own.medium) medium_tr_any(S.own, smp, o, d, tmax, tr);
    }
}
// Interaction::GetMedium(w) (interaction.h:86-88) at a point of triangle `tri` reached by a ray in medium
// `med`: the triangle's pair when it is a transition, else the ray's medium on both sides
// (GeometricPrimitive::Intersect, primitive.cpp:97-101)
__device__ __forceinline__ int medium_towards(const DevScene &S, int tri, f3 n, f3 w, int med) {
    const int in = S.tri_med[2 * tri], out = S.tri_med[2 * tri + 1];
    if (in == out) return med;
    return dot3(w, n) > 0 ? out : in;
}

BRE_TD bool black3(const float v[3]) { return v[0] == 0 && v[1] == 0 && v[2] == 0; }
BRE_TD float lum3(const float v[3]) { return 0.212671f * v[0] + 0.715160f * v[1] + 0.072169f * v[2]; }

// ---- the shading frame of a triangle's BSDF: WorldToLocal / LocalToWorld, reflection.h:437-446 ----
BRE_TD f3 to_local(const PTri &q, f3 v) { return mk(dot3(v, q.ss), dot3(v, q.ts), dot3(v, q.n)); }
BRE_TD f3 to_world(const PTri &q, f3 v) {
    return mk(q.ss.x * v.x + q.ts.x * v.y + q.n.x * v.z, q.ss.y * v.x + q.ts.y * v.y + q.n.y * v.z,
              q.ss.z * v.x + q.ts.z * v.y + q.n.z * v.z);
}

// ---- mirror and glass (src/materials/mirror.cpp, glass.cpp; one specular lobe each) ----
// FrDielectric, reflection.cpp:47-68
BRE_TD float fr_dielectric(float cos_i, float eta_i, float eta_t) {
    cos_i = cos_i < -1.f ? -1.f : (cos_i > 1.f ? 1.f : cos_i);  // Clamp, pbrt.h:278-284
    if (!(cos_i > 0.f)) {
        const float x = eta_i;
        eta_i = eta_t;
        eta_t = x;
        cos_i = fabsf(cos_i);
    }
    const float sin_i = sqrtf(smax(0.f, 1 - cos_i * cos_i));
    const float sin_t = eta_i / eta_t * sin_i;
    if (sin_t >= 1) return 1.f;
    const float cos_t = sqrtf(smax(0.f, 1 - sin_t * sin_t));
    const float r_parl = ((eta_t * cos_i) - (eta_i * cos_t)) / ((eta_t * cos_i) + (eta_i * cos_t));
    const float r_perp = ((eta_i * cos_i) - (eta_t * cos_t)) / ((eta_i * cos_i) + (eta_t * cos_t));
    return (r_parl * r_parl + r_perp * r_perp) / 2;
}

// BSDF::Sample_f (reflection.cpp:703-768) of a BSDF whose one BxDF is SpecularReflection(Kr, FresnelNoOp)
// (mirror; Sample_f :136-143) or FresnelSpecular(Kr, Kt, 1, eta, mode) (glass; :477-511, with Refract of
// reflection.h:96-108), called with BSDF_ALL.  wo and wi are in the shading frame, wi is not normalised;
// u0 is u[0] (one matching component leaves it as it is: min(u[0] * 1 - 0, OneMinusEpsilon)).  Returns
// false where Sample_f returns 0 (wo.z == 0, a failed Refract): pdf, f and type are then 0.
BRE_TD bool specular_sample(const bre_material &m, f3 wo, float u0, int mode, f3 &wi, float &pdf, float f[3],
                            int &type) {
    f[0] = f[1] = f[2] = 0.f;
    pdf = 0.f;
    type = 0;
    if (wo.z == 0) return false;
    if (m.type == BRE_MATERIAL_MIRROR) {
        wi = mk(-wo.x, -wo.y, wo.z);
        pdf = 1.f;
        type = kBsdfSpecular | kBsdfReflection;
        const float ac = fabsf(wi.z);
        for (int c = 0; c < 3; ++c) f[c] = (1.f * m.kr[c]) / ac;  // fresnel->Evaluate() * R / AbsCosTheta(wi)
        return true;
    }
    const float F = fr_dielectric(wo.z, 1.f, m.eta);
    if (u0 < F) {
        wi = mk(-wo.x, -wo.y, wo.z);
        pdf = F;
        type = kBsdfSpecular | kBsdfReflection;
        const float ac = fabsf(wi.z);
        for (int c = 0; c < 3; ++c) f[c] = (m.kr[c] * F) / ac;
        return true;
    }
    const bool entering = wo.z > 0;
    const float eta_i = entering ? 1.f : m.eta, eta_t = entering ? m.eta : 1.f;
    // Refract(wo, Faceforward(Normal3f(0, 0, 1), wo), etaI / etaT, wi)
    const float eta = eta_i / eta_t;
    const f3 n = (wo.z < 0.f) ? mk(-0.f, -0.f, -1.f) : mk(0.f, 0.f, 1.f);
    const float cos_i = dot3(n, wo);
    const float sin2_i = smax(0.f, 1 - cos_i * cos_i);
    const float sin2_t = eta * eta * sin2_i;
    if (sin2_t >= 1) return false;
    const float cos_t = sqrtf(1 - sin2_t);
    const float k = eta * cos_i - cos_t;
    wi = mk(eta * -wo.x + k * n.x, eta * -wo.y + k * n.y, eta * -wo.z + k * n.z);
    pdf = 1 - F;
    if (pdf == 0) return false;  // BSDF::Sample_f's own test (F < 1 here: unreachable, kept as the text has it)
    type = kBsdfSpecular | kBsdfTransmission;
    const float ac = fabsf(wi.z);
    for (int c = 0; c < 3; ++c) {
        float ft = m.kt[c] * (1 - F);
        if (mode == kModeRadiance) ft *= (eta_i * eta_i) / (eta_t * eta_t);
        f[c] = ft / ac;
    }
    return true;
}

// ---- plastic, metal and rough matte: the lobes (reflection.{h,cpp}, microfacet.{h,cpp}) and the general BSDF ----
BRE_TD bool is_inf(float v) { return fabsf(v) == __builtin_huge_valf(); }
// the shading-frame trigonometry of reflection.h:56-83
BRE_TD float cos2_theta(f3 w) { return w.z * w.z; }
BRE_TD float sin2_theta(f3 w) { return smax(0.f, 1.f - cos2_theta(w)); }
BRE_TD float sin_theta(f3 w) { return sqrtf(sin2_theta(w)); }
BRE_TD float tan_theta(f3 w) { return sin_theta(w) / w.z; }
BRE_TD float tan2_theta(f3 w) { return sin2_theta(w) / cos2_theta(w); }
BRE_TD float cos_phi(f3 w) {
    const float s = sin_theta(w);
    return (s == 0) ? 1.f : clampf_ref(w.x / s, -1.f, 1.f);
}
BRE_TD float sin_phi(f3 w) {
    const float s = sin_theta(w);
    return (s == 0) ? 0.f : clampf_ref(w.y / s, -1.f, 1.f);
}

// TrowbridgeReitzDistribution::RoughnessToAlpha, microfacet.h:123-128 (host: a constant of the material)
BRE_TD float roughness_to_alpha(float roughness) {
    roughness = smax(roughness, 1e-3f);
    const float x = bre_logf(roughness);
    return 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x;
}
// TrowbridgeReitzDistribution::D, microfacet.cpp:155-163
BRE_TD float tr_D(float ax, float ay, f3 wh) {
    const float tan2 = tan2_theta(wh);
    if (is_inf(tan2)) return 0.f;
    const float cos4 = cos2_theta(wh) * cos2_theta(wh);
    const float cp = cos_phi(wh), sp = sin_phi(wh);
    const float e = ((cp * cp) / (ax * ax) + (sp * sp) / (ay * ay)) * tan2;
    return 1 / (kPi * ax * ay * cos4 * (1 + e) * (1 + e));
}
// TrowbridgeReitzDistribution::Lambda, microfacet.cpp:176-184
BRE_TD float tr_lambda(float ax, float ay, f3 w) {
    const float abs_tan = fabsf(tan_theta(w));
    if (is_inf(abs_tan)) return 0.f;
    const float cp = cos_phi(w), sp = sin_phi(w);
    const float alpha = sqrtf((cp * cp) * ax * ax + (sp * sp) * ay * ay);
    const float a2t2 = (alpha * abs_tan) * (alpha * abs_tan);
    return (-1 + sqrtf(1.f + a2t2)) / 2;
}
// MicrofacetDistribution::G1 and G, microfacet.h:54-60
BRE_TD float tr_G1(float ax, float ay, f3 w) { return 1 / (1 + tr_lambda(ax, ay, w)); }
BRE_TD float tr_G(float ax, float ay, f3 wo, f3 wi) { return 1 / (1 + tr_lambda(ax, ay, wo) + tr_lambda(ax, ay, wi)); }
// TrowbridgeReitzSample11, microfacet.cpp:238-282.  Its normal-incidence branch compares against a double and
// calls the double sqrt, cos and sin (unqualified names on Floats): (float)sqrt((double)x) is sqrtf(x) (a
// correctly rounded root of a 24-bit value survives the second rounding), the double product is an IEEE
// operation, and cos / sin are bre_sincos_2pi, the one place where "bit-exact" carries a stated exception
// (DESIGN.md section 23).  The CHECKs of :280-281 are not reproduced.
BRE_TD void tr_sample11(float cos_t, float U1, float U2, float &slope_x, float &slope_y) {
    if ((double)cos_t > .9999) {
        const float r = sqrtf(U1 / (1 - U1));
        const float phi = (float)(6.28318530718 * (double)U2);
        double s, c;
        bre_sincos_2pi((double)phi, &s, &c);
        slope_x = (float)((double)r * c);
        slope_y = (float)((double)r * s);
        return;
    }
    const float sin_t = sqrtf(smax(0.f, 1.f - cos_t * cos_t));
    const float tan_t = sin_t / cos_t;
    const float a = 1 / tan_t;
    const float G1 = 2 / (1 + sqrtf(1.f + 1.f / (a * a)));
    const float A = 2 * U1 / G1 - 1;
    float tmp = 1.f / (A * A - 1.f);
    if ((double)tmp > 1e10) tmp = (float)1e10;
    const float B = tan_t;
    const float D = sqrtf(smax(B * B * tmp * tmp - (A * A - B * B) * tmp, 0.f));
    const float sx1 = B * tmp - D;
    const float sx2 = B * tmp + D;
    slope_x = (A < 0 || sx2 > 1.f / tan_t) ? sx1 : sx2;
    float S;
    if (U2 > 0.5f) {
        S = 1.f;
        U2 = 2.f * (U2 - .5f);
    } else {
        S = -1.f;
        U2 = 2.f * (.5f - U2);
    }
    const float z = (U2 * (U2 * (U2 * 0.27385f - 0.73369f) + 0.46341f)) /
                    (U2 * (U2 * (U2 * 0.093073f + 0.309420f) - 1.000000f) + 0.597999f);
    slope_y = S * z * sqrtf(1.f + slope_x * slope_x);
}
// TrowbridgeReitzDistribution::Sample_wh on its sampleVisibleArea branch (microfacet.cpp:330-334) over
// TrowbridgeReitzSample (:284-305)
BRE_TD f3 tr_sample_wh(float ax, float ay, f3 wo, float u0, float u1) {
    const bool flip = wo.z < 0;
    const f3 wi = flip ? neg3(wo) : wo;
    const f3 ws = normalize3(mk(ax * wi.x, ay * wi.y, wi.z));
    float sx, sy;
    tr_sample11(ws.z, u0, u1, sx, sy);
    const float cp = cos_phi(ws), sp = sin_phi(ws);
    const float tmp = cp * sx - sp * sy;
    sy = sp * sx + cp * sy;
    sx = tmp;
    sx = ax * sx;
    sy = ay * sy;
    const f3 wh = normalize3(mk(-sx, -sy, 1.f));
    return flip ? neg3(wh) : wh;
}
// MicrofacetDistribution::Pdf with sampleVisibleArea, microfacet.cpp:338-341
BRE_TD float tr_pdf(float ax, float ay, f3 wo, f3 wh) {
    return tr_D(ax, ay, wh) * tr_G1(ax, ay, wo) * fabsf(dot3(wo, wh)) / fabsf(wo.z);
}
// FrConductor, reflection.cpp:71-95, one channel of it with etai = 1 (FresnelConductor(1., eta, k))
BRE_TD float fr_conductor(float cos_i, float etat, float k) {
    cos_i = clampf_ref(cos_i, -1.f, 1.f);
    const float eta = etat / 1.f, etak = k / 1.f;
    const float cos2 = cos_i * cos_i;
    const float sin2 = (float)(1. - (double)cos2);
    const float eta2 = eta * eta, etak2 = etak * etak;
    const float t0 = eta2 - etak2 - sin2;
    const float a2b2 = sqrtf(t0 * t0 + eta2 * 4.f * etak2);
    const float t1 = a2b2 + cos2;
    const float a = sqrtf((a2b2 + t0) * 0.5f);
    const float t2 = a * ((float)2 * cos_i);
    const float Rs = (t1 - t2) / (t1 + t2);
    const float t3 = a2b2 * cos2 + sin2 * sin2;
    const float t4 = t2 * sin2;
    const float Rp = Rs * (t3 - t4) / (t3 + t4);
    return (Rp + Rs) * 0.5f;
}

// BxDF::f of lobe `lobe` (kLobeDiffuse: LambertianReflection::f, reflection.cpp:178-180, or OrenNayar::f,
// :197-219; kLobeMicro: MicrofacetReflection::f, :226-236); wo, wi in the shading frame
BRE_TD void lobe_f(const DevBsdf &m, int lobe, f3 wo, f3 wi, float f[3]) {
    if (lobe == kLobeDiffuse) {
        if (!m.oren) {
            for (int c = 0; c < 3; ++c) f[c] = m.kd[c] * kInvPi;
            return;
        }
        const float sin_i = sin_theta(wi), sin_o = sin_theta(wo);
        float max_cos = 0;
        if ((double)sin_i > 1e-4 && (double)sin_o > 1e-4) {
            const float spi = sin_phi(wi), cpi = cos_phi(wi);
            const float spo = sin_phi(wo), cpo = cos_phi(wo);
            const float d_cos = cpi * cpo + spi * spo;
            max_cos = smax(0.f, d_cos);
        }
        float sin_alpha, tan_beta;
        if (fabsf(wi.z) > fabsf(wo.z)) {
            sin_alpha = sin_o;
            tan_beta = sin_i / fabsf(wi.z);
        } else {
            sin_alpha = sin_i;
            tan_beta = sin_o / fabsf(wo.z);
        }
        const float s = m.A + m.B * max_cos * sin_alpha * tan_beta;
        for (int c = 0; c < 3; ++c) f[c] = m.kd[c] * kInvPi * s;
        return;
    }
    f[0] = f[1] = f[2] = 0.f;
    const float cos_o = fabsf(wo.z), cos_i = fabsf(wi.z);
    f3 wh = add3(wi, wo);
    if (cos_i == 0 || cos_o == 0) return;
    if (wh.x == 0 && wh.y == 0 && wh.z == 0) return;
    wh = normalize3(wh);
    const float ci = dot3(wi, wh);
    const float D = tr_D(m.ax, m.ay, wh), G = tr_G(m.ax, m.ay, wo, wi);
    const float den = 4 * cos_i * cos_o;
    if (m.conductor) {
        for (int c = 0; c < 3; ++c) f[c] = m.ks[c] * D * G * fr_conductor(fabsf(ci), m.ceta[c], m.ck[c]) / den;
    } else {
        const float F = fr_dielectric(ci, 1.5f, 1.f);
        for (int c = 0; c < 3; ++c) f[c] = m.ks[c] * D * G * F / den;
    }
}
// BxDF::Pdf (reflection.cpp:387-389) or MicrofacetReflection::Pdf (:419-423)
BRE_TD float lobe_pdf(const DevBsdf &m, int lobe, f3 wo, f3 wi) {
    if (lobe == kLobeDiffuse) return (wo.z * wi.z > 0) ? fabsf(wi.z) * kInvPi : 0.f;
    if (!(wo.z * wi.z > 0)) return 0.f;
    const f3 wh = normalize3(add3(wo, wi));
    return tr_pdf(m.ax, m.ay, wo, wh) / (4 * dot3(wo, wh));
}
// BxDF::Sample_f (reflection.cpp:378-385) or MicrofacetReflection::Sample_f (:405-417); pdf arrives as 0 and
// stays 0 where the lobe returns early; wo.z != 0
BRE_TD void lobe_sample(const DevBsdf &m, int lobe, f3 wo, float u0, float u1, f3 &wi, float &pdf, float f[3]) {
    f[0] = f[1] = f[2] = 0.f;
    if (lobe == kLobeDiffuse) {
        wi = cosine_hemisphere(u0, u1);
        if (wo.z < 0) wi.z *= -1;
        pdf = lobe_pdf(m, lobe, wo, wi);
        lobe_f(m, lobe, wo, wi, f);
        return;
    }
    const f3 wh = tr_sample_wh(m.ax, m.ay, wo, u0, u1);
    const float d = dot3(wo, wh);
    wi = add3(neg3(wo), scale3(wh, 2 * d));  // Reflect, reflection.h:92-94
    if (!(wo.z * wi.z > 0)) return;
    pdf = tr_pdf(m.ax, m.ay, wo, wh) / (4 * dot3(wo, wh));
    lobe_f(m, lobe, wo, wi, f);
}

// BSDF::f (reflection.cpp:670-683) for flags that match every lobe here (BSDF_ALL, or BSDF_ALL & ~BSDF_SPECULAR):
// all of them reflect, so f is their sum on the geometric normal's reflecting side and 0 on the other
BRE_TD void bsdf_f(const PTri &q, const DevBsdf &m, f3 wo_w, f3 wi_w, float f[3]) {
    f[0] = f[1] = f[2] = 0.f;
    const f3 wi = to_local(q, wi_w), wo = to_local(q, wo_w);
    if (wo.z == 0) return;
    if (!(dot3(wi_w, q.n) * dot3(wo_w, q.n) > 0)) return;
    for (int lobe = kLobeDiffuse; lobe <= kLobeMicro; lobe <<= 1) {
        if (!(m.lobes & lobe)) continue;
        float fl[3];
        lobe_f(m, lobe, wo, wi, fl);
        for (int c = 0; c < 3; ++c) f[c] = f[c] + fl[c];
    }
}
// BSDF::Pdf, reflection.cpp:770-785
BRE_TD float bsdf_pdf(const PTri &q, const DevBsdf &m, f3 wo_w, f3 wi_w) {
    if (m.lobes == 0) return 0.f;
    const f3 wo = to_local(q, wo_w), wi = to_local(q, wi_w);
    if (wo.z == 0) return 0.f;
    float pdf = 0.f;
    int n = 0;
    for (int lobe = kLobeDiffuse; lobe <= kLobeMicro; lobe <<= 1) {
        if (!(m.lobes & lobe)) continue;
        ++n;
        pdf += lobe_pdf(m, lobe, wo, wi);
    }
    return pdf / (float)n;
}
// BSDF::Sample_f, reflection.cpp:703-768: the component by floor(u[0] * matchingComps), u[0] remapped, the
// lobe's Sample_f, then with two lobes the other's Pdf added and halved and f taken again over both.  Returns
// false where Sample_f returns 0 before f is known (no lobe, wo.z == 0 with pdf untouched, pdf == 0); type is
// then 0.
BRE_TD bool bsdf_sample(const PTri &q, const DevBsdf &m, f3 wo_w, float u0, float u1, f3 &wi_w, float &pdf, float f[3],
                        int &type) {
    f[0] = f[1] = f[2] = 0.f;
    type = 0;
    const int n = (m.lobes & kLobeDiffuse ? 1 : 0) + (m.lobes & kLobeMicro ? 1 : 0);
    if (n == 0) {
        pdf = 0.f;
        return false;
    }
    const int fl = (int)floorf(u0 * (float)n);
    const int comp = fl < n - 1 ? fl : n - 1;
    const int lobe = (n == 2) ? (comp == 0 ? kLobeDiffuse : kLobeMicro) : m.lobes;
    const float ur = smin(u0 * (float)n - (float)comp, kOneMinusEps);
    const f3 wo = to_local(q, wo_w);
    if (wo.z == 0) return false;
    pdf = 0.f;
    f3 wi = mk(0.f, 0.f, 0.f);
    lobe_sample(m, lobe, wo, ur, u1, wi, pdf, f);
    if (pdf == 0) {
        f[0] = f[1] = f[2] = 0.f;
        return false;
    }
    type = kBsdfReflection | (lobe == kLobeDiffuse ? kBsdfDiffuse : kBsdfGlossy);
    wi_w = to_world(q, wi);
    if (n > 1) {
        const int other = lobe == kLobeDiffuse ? kLobeMicro : kLobeDiffuse;
        pdf += lobe_pdf(m, other, wo, wi);
        pdf /= (float)n;
        const bool reflect = dot3(wi_w, q.n) * dot3(wo_w, q.n) > 0;
        f[0] = f[1] = f[2] = 0.f;
        if (reflect)
            for (int l = kLobeDiffuse; l <= kLobeMicro; l <<= 1) {
                float fl2[3];
                lobe_f(m, l, wo, wi, fl2);
                for (int c = 0; c < 3; ++c) f[c] = f[c] + fl2[c];
            }
    }
    return true;
}

// ---- the BSDF of any number of lobes, with BxDFType flags and a TransportMode (DevLobes) ----
// Refract, reflection.h:96-108 (n a Normal3f); false on total internal reflection
BRE_TD bool refract(f3 wi, f3 n, float eta, f3 &wt) {
    const float cos_i = dot3(n, wi);
    const float sin2_i = smax(0.f, 1 - cos_i * cos_i);
    const float sin2_t = eta * eta * sin2_i;
    if (sin2_t >= 1) return false;
    const float cos_t = sqrtf(1 - sin2_t);
    const float k = eta * cos_i - cos_t;
    wt = mk(eta * -wi.x + k * n.x, eta * -wi.y + k * n.y, eta * -wi.z + k * n.z);
    return true;
}
BRE_TD float pow5(float v) { return (v * v) * (v * v) * v; }

// BxDF::f of one lobe, wo and wi in the shading frame: LambertianReflection / Transmission (reflection.cpp:178-190),
// OrenNayar (:197-219), MicrofacetReflection (:226-236), MicrofacetTransmission (:244-266), FresnelBlend (:285-298
// with SchlickFresnel, reflection.h:488-491); 0 for the specular lobes (reflection.h:313-315, 338-340)
BRE_TD void loben_f(const DevLobe &L, f3 wo, f3 wi, int mode, float f[3]) {
    f[0] = f[1] = f[2] = 0.f;
    const int kind = L.kind;
    if (kind == kLobeLambertR || kind == kLobeLambertT) {
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = L.c[c] * kInvPi;
        return;
    }
    if (kind == kLobeOren) {
        const float sin_i = sin_theta(wi), sin_o = sin_theta(wo);
        float max_cos = 0;
        if ((double)sin_i > 1e-4 && (double)sin_o > 1e-4) {
            const float spi = sin_phi(wi), cpi = cos_phi(wi);
            const float spo = sin_phi(wo), cpo = cos_phi(wo);
            const float d_cos = cpi * cpo + spi * spo;
            max_cos = smax(0.f, d_cos);
        }
        float sin_alpha, tan_beta;
        if (fabsf(wi.z) > fabsf(wo.z)) {
            sin_alpha = sin_o;
            tan_beta = sin_i / fabsf(wi.z);
        } else {
            sin_alpha = sin_i;
            tan_beta = sin_o / fabsf(wo.z);
        }
        const float s = L.ax + L.ay * max_cos * sin_alpha * tan_beta;
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = L.c[c] * kInvPi * s;
        return;
    }
    if (kind == kLobeMicroR || kind == kLobeMicroRC) {
        const float cos_o = fabsf(wo.z), cos_i = fabsf(wi.z);
        f3 wh = add3(wi, wo);
        if (cos_i == 0 || cos_o == 0) return;
        if (wh.x == 0 && wh.y == 0 && wh.z == 0) return;
        wh = normalize3(wh);
        const float ci = dot3(wi, wh);
        const float D = tr_D(L.ax, L.ay, wh), G = tr_G(L.ax, L.ay, wo, wi);
        const float den = 4 * cos_i * cos_o;
        if (kind == kLobeMicroRC) {
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c] = L.c[c] * D * G * fr_conductor(fabsf(ci), L.s[c], L.t[c]) / den;
        } else {
            const float F = fr_dielectric(ci, L.etaA, L.etaB);
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c] = L.c[c] * D * G * F / den;
        }
        return;
    }
    if (kind == kLobeMicroT) {
        if (wo.z * wi.z > 0) return;  // transmission only
        const float cos_o = wo.z, cos_i = wi.z;
        if (cos_i == 0 || cos_o == 0) return;
        const float eta = wo.z > 0 ? (L.etaB / L.etaA) : (L.etaA / L.etaB);
        f3 wh = normalize3(add3(wo, scale3(wi, eta)));
        if (wh.z < 0) wh = neg3(wh);
        const float F = fr_dielectric(dot3(wo, wh), L.etaA, L.etaB);
        const float sd = dot3(wo, wh) + eta * dot3(wi, wh);
        const float factor = (mode == kModeRadiance) ? (1 / eta) : 1.f;
        const float v = fabsf(tr_D(L.ax, L.ay, wh) * tr_G(L.ax, L.ay, wo, wi) * eta * eta * fabsf(dot3(wi, wh)) *
                              fabsf(dot3(wo, wh)) * factor * factor / (cos_i * cos_o * sd * sd));
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = (1.f - F) * L.c[c] * v;
        return;
    }
    if (kind == kLobeBlend) {
        const float a = 1 - pow5(1 - .5f * fabsf(wi.z)), b = 1 - pow5(1 - .5f * fabsf(wo.z));
        f3 wh = add3(wi, wo);
        if (wh.x == 0 && wh.y == 0 && wh.z == 0) return;
        wh = normalize3(wh);
        const float sc = tr_D(L.ax, L.ay, wh) / (4 * fabsf(dot3(wi, wh)) * smax(fabsf(wi.z), fabsf(wo.z)));
        const float p5 = pow5(1 - dot3(wi, wh));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float diffuse = (28.f / (23.f * kPi)) * L.c[c] * (1.f - L.s[c]) * a * b;
            const float specular = sc * (L.s[c] + p5 * (1.f - L.s[c]));
            f[c] = diffuse + specular;
        }
    }
}
// BxDF::Pdf (reflection.cpp:387-389), LambertianTransmission's (:400-403), MicrofacetReflection's (:419-423),
// MicrofacetTransmission's (:436-448), FresnelBlend's (:470-475); 0 for the specular lobes
BRE_TD float loben_pdf(const DevLobe &L, f3 wo, f3 wi) {
    const int kind = L.kind;
    const bool same = wo.z * wi.z > 0;
    if (kind == kLobeLambertR || kind == kLobeOren) return same ? fabsf(wi.z) * kInvPi : 0.f;
    if (kind == kLobeLambertT) return !same ? fabsf(wi.z) * kInvPi : 0.f;
    if (kind == kLobeMicroR || kind == kLobeMicroRC) {
        if (!same) return 0.f;
        const f3 wh = normalize3(add3(wo, wi));
        return tr_pdf(L.ax, L.ay, wo, wh) / (4 * dot3(wo, wh));
    }
    if (kind == kLobeMicroT) {
        if (same) return 0.f;
        const float eta = wo.z > 0 ? (L.etaB / L.etaA) : (L.etaA / L.etaB);
        const f3 wh = normalize3(add3(wo, scale3(wi, eta)));
        const float sd = dot3(wo, wh) + eta * dot3(wi, wh);
        const float dwh_dwi = fabsf((eta * eta * dot3(wi, wh)) / (sd * sd));
        return tr_pdf(L.ax, L.ay, wo, wh) * dwh_dwi;
    }
    if (kind == kLobeBlend) {
        if (!same) return 0.f;
        const f3 wh = normalize3(add3(wo, wi));
        const float pdf_wh = tr_pdf(L.ax, L.ay, wo, wh);
        return .5f * (fabsf(wi.z) * kInvPi + pdf_wh / (4 * dot3(wo, wh)));
    }
    return 0.f;
}
// The lobe's Sample_f (reflection.cpp:136-166, 378-385, 391-398, 405-417, 425-434, 450-468); pdf arrives as 0 and
// stays 0 where the lobe returns early, f then being what the caller put there; wo.z != 0
BRE_TD void loben_sample(const DevLobe &L, f3 wo, float u0, float u1, int mode, f3 &wi, float &pdf, float f[3]) {
    const int kind = L.kind;
    if (kind == kLobeSpecR) {
        wi = mk(-wo.x, -wo.y, wo.z);
        pdf = 1.f;
        const float F = fr_dielectric(wi.z, L.etaA, L.etaB);
        const float ac = fabsf(wi.z);
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = F * L.c[c] / ac;
        return;
    }
    if (kind == kLobeSpecT) {
        const bool entering = wo.z > 0;
        const float eta_i = entering ? L.etaA : L.etaB, eta_t = entering ? L.etaB : L.etaA;
        // Faceforward(Normal3f(0, 0, 1), wo)
        const f3 n = (wo.z < 0.f) ? mk(-0.f, -0.f, -1.f) : mk(0.f, 0.f, 1.f);
        if (!refract(wo, n, eta_i / eta_t, wi)) return;
        pdf = 1.f;
        const float F = fr_dielectric(wi.z, L.etaA, L.etaB);
        const float ac = fabsf(wi.z);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float ft = L.c[c] * (1.f - F);
            if (mode == kModeRadiance) ft *= (eta_i * eta_i) / (eta_t * eta_t);
            f[c] = ft / ac;
        }
        return;
    }
    if (kind == kLobeLambertR || kind == kLobeOren || kind == kLobeLambertT) {
        wi = cosine_hemisphere(u0, u1);
        if (kind == kLobeLambertT ? wo.z > 0 : wo.z < 0) wi.z *= -1;
    } else if (kind == kLobeMicroT) {
        const f3 wh = tr_sample_wh(L.ax, L.ay, wo, u0, u1);
        const float eta = wo.z > 0 ? (L.etaA / L.etaB) : (L.etaB / L.etaA);
        if (!refract(wo, wh, eta, wi)) return;
    } else {
        if (kind == kLobeBlend) {
            if (u0 < .5f) {
                wi = cosine_hemisphere(smin(2 * u0, kOneMinusEps), u1);
                if (wo.z < 0) wi.z *= -1;
                pdf = loben_pdf(L, wo, wi);
                loben_f(L, wo, wi, mode, f);
                return;
            }
            u0 = smin(2 * (u0 - .5f), kOneMinusEps);
        }
        const f3 wh = tr_sample_wh(L.ax, L.ay, wo, u0, u1);
        wi = add3(neg3(wo), scale3(wh, 2 * dot3(wo, wh)));  // Reflect, reflection.h:92-94
        if (!(wo.z * wi.z > 0)) return;
        if (kind != kLobeBlend) {  // MicrofacetReflection: the pdf of the sampled wh, not of Normalize(wo + wi)
            pdf = tr_pdf(L.ax, L.ay, wo, wh) / (4 * dot3(wo, wh));
            loben_f(L, wo, wi, mode, f);
            return;
        }
    }
    pdf = loben_pdf(L, wo, wi);
    loben_f(L, wo, wi, mode, f);
}

BRE_TD bool lobe_matches(const DevLobe &L, int flags) { return (L.type & flags) == L.type; }  // BxDF::MatchesFlags

// ---- the lobes of a wide list (DevLobeMx): the two specular lobes a mix brings, and ScaledBxDF around any lobe ----
// ScaledBxDF's scale * f (reflection.cpp:97-106) once per enclosing mix, innermost first; nothing for a DevLobe
BRE_TD void lobe_scale(const DevLobe &, float[3]) {}
BRE_TD void lobe_scale(const DevLobeMx &L, float f[3]) {
    for (int k = 0; k < L.nscale; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = L.scale[k][c] * f[c];
}
// BxDF::f and Pdf through the scales: loben_f leaves 0 for the two new kinds as for every specular lobe, and
// ScaledBxDF::Pdf is the inner Pdf
BRE_TD void lobex_f(const DevLobe &L, f3 wo, f3 wi, int mode, float f[3]) { loben_f(L, wo, wi, mode, f); }
BRE_TD void lobex_f(const DevLobeMx &L, f3 wo, f3 wi, int mode, float f[3]) {
    loben_f(L, wo, wi, mode, f);
    lobe_scale(L, f);
}
// Sample_f; `type` arrives as the lobe's own and is changed only by FresnelSpecular (reflection.cpp:486-487, 506-507)
BRE_TD void lobex_sample(const DevLobeMx &L, f3 wo, float u0, float u1, int mode, f3 &wi, float &pdf, float f[3],
                         int &type) {
    if (L.kind == kLobeSpecNoOp) {  // SpecularReflection::Sample_f under FresnelNoOp, reflection.cpp:136-143
        wi = mk(-wo.x, -wo.y, wo.z);
        pdf = 1.f;
        const float ac = fabsf(wi.z);
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = (1.f * L.c[c]) / ac;
    } else if (L.kind == kLobeFresnelSpec) {  // FresnelSpecular::Sample_f, reflection.cpp:477-511 (R = c, T = s)
        const float F = fr_dielectric(wo.z, L.etaA, L.etaB);
        if (u0 < F) {
            wi = mk(-wo.x, -wo.y, wo.z);
            type = kBsdfSpecular | kBsdfReflection;
            pdf = F;
            const float ac = fabsf(wi.z);
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c] = (F * L.c[c]) / ac;
        } else {
            const bool entering = wo.z > 0;
            const float eta_i = entering ? L.etaA : L.etaB, eta_t = entering ? L.etaB : L.etaA;
            const f3 n = (wo.z < 0.f) ? mk(-0.f, -0.f, -1.f) : mk(0.f, 0.f, 1.f);
            if (!refract(wo, n, eta_i / eta_t, wi)) return;  // pdf stays 0
            type = kBsdfSpecular | kBsdfTransmission;
            pdf = 1 - F;
            const float ac = fabsf(wi.z);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float ft = L.s[c] * (1 - F);
                if (mode == kModeRadiance) ft *= (eta_i * eta_i) / (eta_t * eta_t);
                f[c] = ft / ac;
            }
        }
    } else {
        loben_sample(L, wo, u0, u1, mode, wi, pdf, f);
    }
    lobe_scale(L, f);
}
// BSDF::f, reflection.cpp:670-683: the matching lobes on the side of the geometric normal that wi lies on
// (REC: DevLobes, or DevLobesMx with its scales and its two more kinds; the walk is the same)
template <class REC>
BRE_TD void bsdfn_f(const PTri &q, const REC &m, f3 wo_w, f3 wi_w, int flags, int mode, float f[3]) {
    f[0] = f[1] = f[2] = 0.f;
    const f3 wi = to_local(q, wi_w), wo = to_local(q, wo_w);
    if (wo.z == 0) return;
    const bool reflect = dot3(wi_w, q.n) * dot3(wo_w, q.n) > 0;
    for (int i = 0; i < m.n; ++i) {
        const auto &L = m.lobe[i];
        if (!lobe_matches(L, flags) || !(L.type & (reflect ? kBsdfReflection : kBsdfTransmission))) continue;
        float fl[3];
        lobex_f(L, wo, wi, mode, fl);
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c] = f[c] + fl[c];
    }
}
// BSDF::Pdf, reflection.cpp:770-785
template <class REC>
BRE_TD float bsdfn_pdf(const PTri &q, const REC &m, f3 wo_w, f3 wi_w, int flags) {
    if (m.n == 0) return 0.f;
    const f3 wo = to_local(q, wo_w), wi = to_local(q, wi_w);
    if (wo.z == 0) return 0.f;
    float pdf = 0.f;
    int n = 0;
    for (int i = 0; i < m.n; ++i) {
        if (!lobe_matches(m.lobe[i], flags)) continue;
        ++n;
        pdf += loben_pdf(m.lobe[i], wo, wi);
    }
    return n > 0 ? pdf / (float)n : 0.f;
}
// BSDF::Sample_f, reflection.cpp:703-768: NumComponents(flags), the component by floor(u[0] * n) over the matching
// lobes, u[0] remapped, the lobe's Sample_f; unless that lobe is specular, the other matching lobes' Pdf added and f
// taken again over all of them (:749-764).  Returns false where Sample_f returns 0 before f is known (no matching
// lobe, wo.z == 0 with pdf untouched, pdf == 0); type is then 0.
template <class REC>
BRE_TD bool bsdfn_sample(const PTri &q, const REC &m, f3 wo_w, float u0, float u1, int flags, int mode, f3 &wi_w,
                         float &pdf, float f[3], int &type) {
    f[0] = f[1] = f[2] = 0.f;
    type = 0;
    int n = 0;
    for (int i = 0; i < m.n; ++i) n += lobe_matches(m.lobe[i], flags) ? 1 : 0;
    if (n == 0) {
        pdf = 0.f;
        return false;
    }
    const int fl = (int)floorf(u0 * (float)n);
    const int comp = fl < n - 1 ? fl : n - 1;
    int at = 0;
    for (int i = 0, count = comp; i < m.n; ++i)
        if (lobe_matches(m.lobe[i], flags) && count-- == 0) {
            at = i;
            break;
        }
    const auto &L = m.lobe[at];
    const float ur = smin(u0 * (float)n - (float)comp, kOneMinusEps);
    const f3 wo = to_local(q, wo_w);
    if (wo.z == 0) return false;
    pdf = 0.f;
    f3 wi = mk(0.f, 0.f, 0.f);
    if constexpr (std::is_same<REC, DevLobes>::value) {  // the statements tier 2 had, in their order
        loben_sample(L, wo, ur, u1, mode, wi, pdf, f);
        if (pdf == 0) return false;  // f is whatever the lobe left: the callers read it only behind pdf != 0
        type = L.type;
    } else {
        int sampled = L.type;  // *sampledType = bxdf->type before the lobe's Sample_f (:737), which may change it
        lobex_sample(L, wo, ur, u1, mode, wi, pdf, f, sampled);
        if (pdf == 0) return false;
        type = sampled;
    }
    wi_w = to_world(q, wi);
    const bool mix = !(L.type & kBsdfSpecular) && n > 1;
    if (mix)
        for (int i = 0; i < m.n; ++i)
            if (i != at && lobe_matches(m.lobe[i], flags)) pdf += loben_pdf(m.lobe[i], wo, wi);
    if (n > 1) pdf /= (float)n;
    if (mix) {
        const bool reflect = dot3(wi_w, q.n) * dot3(wo_w, q.n) > 0;
        f[0] = f[1] = f[2] = 0.f;
        for (int i = 0; i < m.n; ++i) {
            const auto &K = m.lobe[i];
            if (!lobe_matches(K, flags) || !(K.type & (reflect ? kBsdfReflection : kBsdfTransmission))) continue;
            float fl2[3];
            lobex_f(K, wo, wi, mode, fl2);
#pragma unroll
            for (int c = 0; c < 3; ++c) f[c] = f[c] + fl2[c];
        }
    }
    return true;
}

// ---- camera pass (bre_camera.hip) ----
constexpr int kHaltonDims = 1000;  // HaltonSampler's PrimeTableSize = AwesomeSampler's limit (photonbeam.cpp:460)

struct DevCamera {
    f3 pos, dir, right, nup;           // LookAt frame
    float sx0, sx1, sy0, sy1;          // screen window
    float tan_ang, fw, fh;             // tan(fov/2), film size as float
    int width, height;
    int base_scale[2], base_exp[2];    // HaltonSampler baseScales / baseExponents
    int stride;                        // sampleStride
    int mult_inv[2];                   // multInverse
    int primes[kHaltonDims];
    int prime_sums[kHaltonDims];
};

// per-(depth, pixel-slot) camera segments before compaction
struct CamSlots {
    SegOut seg;
    int32_t *valid;
};

void prepare_camera(const bre_scene *s, int width, int height, DevCamera *c, std::vector<uint16_t> *perms);
int64_t camera_slots(int width, int height);
// `planes`: the slot planes of `s` (max_depth, plus the segment budget with media and an interface triangle);
// `media`: the context holds media (the kernel that carries a medium per ray); `tier`: as for launch_photons (1 also
// where the context holds a distant light)
hipError_t launch_camera(const DevScene *scene, int stack_depth, const DevCamera *cam, const uint16_t *perms, int width,
                         int height, int iteration, int max_depth, int render_surfaces, int render_media,
                         const CamSlots &s, float *surface, unsigned int *flags, int shard_rank, int shard_count,
                         int shard_block, int classes, int planes, bool media, int tier, hipStream_t stream);
constexpr unsigned int kCamFlagBudget = 1u;  // k_camera's flag word: a path overran its segment budget
size_t camera_scan_temp_bytes(int64_t n);
hipError_t launch_camera_scan(void *tmp, size_t tmp_bytes, const CamSlots &s, int64_t nslots, int max_depth,
                              int64_t *offs, hipStream_t stream, bool slot);
hipError_t launch_camera_compact(const CamSlots &s, int64_t nslots, int max_depth, const int64_t *offs,
                                 const SegOut &out, int32_t *depth, hipStream_t stream);

// bre_device_check kind 12 (bre_check.hip): specular_sample on n records of 6 floats, 6 words out each
hipError_t launch_check_specular(int64_t n, const float *x, float *y, hipStream_t s);
// kind 13 (bre_check.hip): bsdf_sample, bsdf_f and bsdf_pdf on n records of 9 floats against `table`, 12 words out each
hipError_t launch_check_bsdf(int64_t n, const float *x, const DevBsdf *table, int n_table, float *y, hipStream_t s);
// kind 14 (bre_check.hip): bsdfn_sample, bsdfn_f and bsdfn_pdf on n records of 11 floats against `table`, 12 words out
hipError_t launch_check_lobes(int64_t n, const float *x, const DevLobes *table, int n_table, float *y, hipStream_t s);
// kind 14 over a table that holds a mix: the same records against the wide lists
hipError_t launch_check_lobes_mx(int64_t n, const float *x, const DevLobesMx *table, int n_table, float *y,
                                 hipStream_t s);

// dynamic LDS of a photon / camera launch: the scene traversal stack of every thread of a block
inline size_t scene_stack_bytes(int stack_depth, int block) {
    return (size_t)(stack_depth > 0 ? stack_depth : 1) * (size_t)block * sizeof(int);
}

// waves per SIMD the glossy (GL) instantiations of k_photons and k_camera are bounded to; the others keep 6
constexpr int kGlossyWaves = 2;
// ... and the tier-3 kernels (k_photons_mx, k_camera_mx): the walk of tier 2 with a scale chain per lobe
constexpr int kMixWaves = 2;

// photon pass launchers (bre_photon.hip)
// dynamic LDS of a photon launch: the traversal stack and, for the glossy kernels, max_depth suspended frames a thread
size_t photon_lds_bytes(int stack_depth, int max_depth, bool glossy);
// mode 0: count beams per photon; 1: write them at offsets (over > 0: only photons with more than `over`
// beams); 2: write the first `over` beams to per-photon slots and count them all (single-trace form)
// `media`: the context holds media (the kernels that carry a medium per ray); `tier`: 1 where its table holds a
// plastic, metal or matte entry (the kernels with the two-lobe BSDF), 2 where it holds a rough glass, uber,
// translucent or substrate entry (the kernels with the BSDF of any number of lobes), 3 where it holds a mix (the same
// over the wide lists, DevScene::lobes_mx), else 0
hipError_t launch_photons(const DevScene *scene, int stack_depth, int64_t n, uint64_t seq0, int max_depth,
                          float radius, int32_t *counts, const int64_t *offsets, const BeamOut &out, int mode,
                          int over, bool media, int tier, hipStream_t s);
// the single-trace form's copy of each photon's slots to its offsets
hipError_t launch_photon_slots(int64_t n, int cap, const int32_t *counts, const int64_t *offsets,
                               const BeamView &slots, const BeamOut &out, hipStream_t s);
size_t count_scan_temp_bytes(int64_t n);
hipError_t launch_count_scan(void *tmp, size_t bytes, const int32_t *counts, int64_t *offsets, int64_t n, hipStream_t s,
                             bool slot);

}  // namespace bre
