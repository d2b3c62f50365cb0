// bre_scene.hip — the host side of the scene model the photon and camera passes share: a bre_scene, the
// context's delta lights and materials as the reference's constructors leave them (per-triangle constants,
// scene.lights with their power distribution, the BVHAccel of bre_accel.hip), and a medium record.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "bre_trace.h"

namespace bre {

float max_density(const float *density, int64_t n) {
    float mx = 0;
    for (int64_t i = 0; i < n; ++i) mx = std::max(mx, density[i]);
    return mx;
}
float grid_max_density(const bre_scene *s) {
    return max_density(s->grid_density, (int64_t)s->grid_n[0] * s->grid_n[1] * s->grid_n[2]);
}

DevMedium make_medium(int type, const float sigma_a[3], const float sigma_s[3], float g, const int32_t grid_n[3],
                      const float world_to_medium[16], const float *d_density, float max_dens) {
    DevMedium d{};
    d.medium = type;
    for (int c = 0; c < 3; ++c) d.sigma_t[c] = sigma_a[c] + sigma_s[c];  // HomogeneousMedium ctor: sigma_a + sigma_s
    d.g = g;
    if (type != BRE_MEDIUM_GRID) return d;
    // GridDensityMedium ctor (grid.h:58-77): sigma_t = (sigma_a + sigma_s)[0]; invMaxDensity
    for (int k = 0; k < 3; ++k) d.gn[k] = grid_n[k];
    d.grid_sigma_t = sigma_a[0] + sigma_s[0];
    d.grid_inv_max = 1 / max_dens;
    for (int k = 0; k < 16; ++k) d.w2m[k] = world_to_medium[k];
    d.density = d_density;
    return d;
}

void prepare_medium(const bre_scene *s, DevScene *d, const float *d_density) {
    const int type = s->has_medium == BRE_MEDIUM_GRID ? BRE_MEDIUM_GRID : (s->has_medium ? BRE_MEDIUM_HOMOGENEOUS : 0);
    d->own = make_medium(type, s->sigma_a, s->sigma_s, s->g, s->grid_n, s->world_to_medium, d_density,
                         type == BRE_MEDIUM_GRID ? grid_max_density(s) : 0.f);
}

// PointLight / SpotLight constructors (point.h, spot.cpp:44-51) and Light's (light.cpp:46-55); a DistantLight's
// record already holds what its constructor leaves (distant.cpp:43-47), its centre and radius come with the BVH
DLight prepare_light(const bre_light &l) {
    DLight D{};
    const float *m = l.light_to_world;
    if (l.type == BRE_LIGHT_DISTANT) {
        D.kind = kLightDistant;
        for (int k = 0; k < 3; ++k) {
            D.l2w[k] = m[k];
            D.I[k] = l.I[k];
        }
        return D;
    }
    // pLight = LightToWorld(Point3f(0, 0, 0)), Transform::operator()(Point3f) (transform.h:223-233)
    const float x = 0.f, y = 0.f, z = 0.f;
    const float xp = m[0] * x + m[1] * y + m[2] * z + m[3];
    const float yp = m[4] * x + m[5] * y + m[6] * z + m[7];
    const float zp = m[8] * x + m[9] * y + m[10] * z + m[11];
    const float wp = m[12] * x + m[13] * y + m[14] * z + m[15];
    D.p = wp == 1 ? mk(xp, yp, zp) : div3(mk(xp, yp, zp), wp);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            D.l2w[3 * r + c] = l.light_to_world[4 * r + c];
            D.w2l[3 * r + c] = l.world_to_light[4 * r + c];
        }
    for (int k = 0; k < 3; ++k) D.I[k] = l.I[k];
    D.kind = l.type == BRE_LIGHT_SPOT ? kLightSpot : kLightPoint;
    if (D.kind == kLightSpot) {  // std::cos(Radians(.)), pbrt.h:295
        D.cos_total = bre_cosf((kPi / 180) * l.cone_total_deg);
        D.cos_start = bre_cosf((kPi / 180) * l.cone_falloff_start_deg);
    }
    return D;
}

// Power().y(): 4 * Pi * I (point.cpp:55); I * 2 * Pi * (1 - .5f * (cosFalloffStart + cosTotalWidth))
// (spot.cpp:75-77); L * Pi * worldRadius * worldRadius (distant.cpp:61-63)
static float light_power_y(const DLight &D) {
    float pw[3];
    for (int k = 0; k < 3; ++k) {
        if (D.kind == kLightDistant) pw[k] = D.I[k] * kPi * distant_radius(D) * distant_radius(D);
        else pw[k] = D.kind == kLightSpot ? D.I[k] * 2 * kPi * (1 - .5f * (D.cos_start + D.cos_total)) : D.I[k] * (4 * kPi);
    }
    return lum3(pw);
}

// Bounds3::BoundingSphere (geometry.h) of Scene::WorldBound(), the root box of the scene's BVHAccel (the union of
// the Triangle::WorldBound()s, whatever their order), as DistantLight::Preprocess takes it (distant.h)
static void world_bounding_sphere(const SceneNode &root, f3 *center, float *radius) {
    const f3 lo = mk(root.lo[0], root.lo[1], root.lo[2]), hi = mk(root.hi[0], root.hi[1], root.hi[2]);
    *center = div3(add3(lo, hi), 2.f);  // (pMin + pMax) / 2
    const f3 c = *center;
    const bool inside = c.x >= lo.x && c.x <= hi.x && c.y >= lo.y && c.y <= hi.y && c.z >= lo.z && c.z <= hi.z;
    *radius = inside ? len3(sub3(c, hi)) : 0.f;  // Inside(*center, *this) ? Distance(*center, pMax) : 0
}

// PlasticMaterial / MetalMaterial / MatteMaterial::ComputeScatteringFunctions (plastic.cpp:45-70, metal.cpp:59-80,
// matte.cpp:45-62) on the record's constants (the setter has clamped Kd and Ks and checked the roughnesses)
DevBsdf make_bsdf(const bre_material_ex &m) {
    DevBsdf b{};
    if (m.type < BRE_MATERIAL_MATTE || m.type > BRE_MATERIAL_METAL) return b;
    b.type = m.type;
    b.ax = b.ay = 1.f;
    if (m.type == BRE_MATERIAL_MATTE) {
        const float sig = clampf_ref(m.sigma, 0.f, 90.f);
        if (!black3(m.kd)) b.lobes = kLobeDiffuse;
        for (int c = 0; c < 3; ++c) b.kd[c] = m.kd[c];
        if (sig != 0) {  // OrenNayar's constructor, reflection.h:417-423
            const float sigma = (kPi / 180) * sig;
            const float sigma2 = sigma * sigma;
            b.A = 1.f - (sigma2 / (2.f * (sigma2 + 0.33f)));
            b.B = 0.45f * sigma2 / (sigma2 + 0.09f);
            b.oren = 1;
        }
    } else if (m.type == BRE_MATERIAL_PLASTIC) {
        if (!black3(m.kd)) b.lobes |= kLobeDiffuse;
        if (!black3(m.ks)) b.lobes |= kLobeMicro;
        for (int c = 0; c < 3; ++c) {
            b.kd[c] = m.kd[c];
            b.ks[c] = m.ks[c];
        }
        float rough = m.roughness;
        if (m.remap) rough = roughness_to_alpha(rough);
        b.ax = b.ay = rough;
    } else {
        float u = m.uroughness != 0 ? m.uroughness : m.roughness;
        float v = m.vroughness != 0 ? m.vroughness : m.roughness;
        if (m.remap) {
            u = roughness_to_alpha(u);
            v = roughness_to_alpha(v);
        }
        b.ax = u;
        b.ay = v;
        b.lobes = kLobeMicro;
        b.conductor = 1;
        for (int c = 0; c < 3; ++c) {
            b.ks[c] = 1.f;
            b.ceta[c] = m.ceta[c];
            b.ck[c] = m.ck[c];
        }
    }
    return b;
}

// The same three materials as a list of lobes, and GlassMaterial with roughness (glass.cpp:45-92), UberMaterial
// (uber.cpp:45-101), TranslucentMaterial (translucent.cpp:45-80) and SubstrateMaterial (substrate.cpp:45-65): the
// BxDFs in the order added, each colour the product the reference forms (op * Kd, r * ks, ...), in its operations.
// The setter has clamped the colours and checked the roughnesses.
DevLobes make_lobes(const bre_material_ex &m) {
    DevLobes b{};
    if (m.type < BRE_MATERIAL_MATTE || m.type == 7 || m.type > BRE_MATERIAL_SUBSTRATE) return b;
    b.type = m.type;
    const auto add = [&](int kind, int type, const float c[3], float ax, float ay, float etaA, float etaB) -> DevLobe & {
        DevLobe &L = b.lobe[b.n++];
        L.kind = kind;
        L.type = type;
        for (int k = 0; k < 3; ++k) L.c[k] = c[k];
        L.ax = ax;
        L.ay = ay;
        L.etaA = etaA;
        L.etaB = etaB;
        if (!(type & kBsdfSpecular)) ++b.n_nonspec;
        return L;
    };
    const auto mul3 = [](const float a[3], const float x[3], float out[3]) {
        for (int k = 0; k < 3; ++k) out[k] = a[k] * x[k];
    };
    constexpr int R = kBsdfReflection, T = kBsdfTransmission;
    if (m.type <= BRE_MATERIAL_METAL) {
        const DevBsdf o = make_bsdf(m);
        if (o.lobes & kLobeDiffuse)
            add(o.oren ? kLobeOren : kLobeLambertR, R | kBsdfDiffuse, o.kd, o.oren ? o.A : 1.f, o.oren ? o.B : 1.f, 1.f, 1.f);
        if (o.lobes & kLobeMicro) {
            DevLobe &L = add(o.conductor ? kLobeMicroRC : kLobeMicroR, R | kBsdfGlossy, o.ks, o.ax, o.ay, 1.5f, 1.f);
            for (int k = 0; k < 3; ++k) {
                L.s[k] = o.ceta[k];
                L.t[k] = o.ck[k];
            }
        }
        return b;
    }
    if (m.type == BRE_MATERIAL_ROUGH_GLASS) {
        if (black3(m.kr) && black3(m.kt)) return b;
        float u = m.uroughness, v = m.vroughness;
        if (m.remap) {
            u = roughness_to_alpha(u);
            v = roughness_to_alpha(v);
        }
        if (!black3(m.kr)) add(kLobeMicroR, R | kBsdfGlossy, m.kr, u, v, 1.f, m.eta);
        if (!black3(m.kt)) add(kLobeMicroT, T | kBsdfGlossy, m.kt, u, v, 1.f, m.eta);
        return b;
    }
    if (m.type == BRE_MATERIAL_UBER) {
        const float e = m.eta;
        float t[3], c[3];
        for (int k = 0; k < 3; ++k) t[k] = clampf_ref(-m.opacity[k] + 1.f, 0.f, kMaxFloat);  // (-op + Spectrum(1.f)).Clamp()
        if (!black3(t)) add(kLobeSpecT, T | kBsdfSpecular, t, 1.f, 1.f, 1.f, 1.f);
        mul3(m.opacity, m.kd, c);
        if (!black3(c)) add(kLobeLambertR, R | kBsdfDiffuse, c, 1.f, 1.f, 1.f, 1.f);
        mul3(m.opacity, m.ks, c);
        if (!black3(c)) {
            float u = m.uroughness != 0 ? m.uroughness : m.roughness;
            float v = m.vroughness != 0 ? m.vroughness : u;
            if (m.remap) {
                u = roughness_to_alpha(u);
                v = roughness_to_alpha(v);
            }
            add(kLobeMicroR, R | kBsdfGlossy, c, u, v, 1.f, e);
        }
        mul3(m.opacity, m.kr, c);
        if (!black3(c)) add(kLobeSpecR, R | kBsdfSpecular, c, 1.f, 1.f, 1.f, e);
        mul3(m.opacity, m.kt, c);
        if (!black3(c)) add(kLobeSpecT, T | kBsdfSpecular, c, 1.f, 1.f, 1.f, e);
        return b;
    }
    if (m.type == BRE_MATERIAL_TRANSLUCENT) {
        const float *r = m.kr, *t = m.kt;  // "reflect", "transmit"
        if (black3(r) && black3(t)) return b;
        float c[3];
        if (!black3(m.kd)) {
            mul3(r, m.kd, c);
            if (!black3(r)) add(kLobeLambertR, R | kBsdfDiffuse, c, 1.f, 1.f, 1.f, 1.f);
            mul3(t, m.kd, c);
            if (!black3(t)) add(kLobeLambertT, T | kBsdfDiffuse, c, 1.f, 1.f, 1.f, 1.f);
        }
        if (!black3(m.ks)) {
            float rough = m.roughness;
            if (m.remap) rough = roughness_to_alpha(rough);
            mul3(r, m.ks, c);
            if (!black3(r)) add(kLobeMicroR, R | kBsdfGlossy, c, rough, rough, 1.f, 1.5f);
            mul3(t, m.ks, c);
            if (!black3(t)) add(kLobeMicroT, T | kBsdfGlossy, c, rough, rough, 1.f, 1.5f);
        }
        return b;
    }
    // substrate
    if (!black3(m.kd) || !black3(m.ks)) {
        float u = m.uroughness, v = m.vroughness;
        if (m.remap) {
            u = roughness_to_alpha(u);
            v = roughness_to_alpha(v);
        }
        DevLobe &L = add(kLobeBlend, R | kBsdfGlossy, m.kd, u, v, 1.f, 1.f);
        for (int k = 0; k < 3; ++k) L.s[k] = m.ks[k];
    }
    return b;
}

// The BxDFs a table entry brings to a mix that names it (mixmat.cpp:54-55: the child's own
// ComputeScatteringFunctions, allowMultipleLobes true as both walks pass it): a mirror's SpecularReflection under
// FresnelNoOp (mirror.cpp:50-56), a smooth glass's FresnelSpecular (glass.cpp:71-73), else the entry's wide list, which
// for a mix already carries its scales
static DevLobesMx child_lobes(const bre_material_ex &m, const DevLobesMx &own) {
    if (m.type != BRE_MATERIAL_MIRROR && m.type != BRE_MATERIAL_GLASS) return own;
    DevLobesMx b{};
    DevLobeMx L{};
    L.ax = L.ay = L.etaA = L.etaB = 1.f;
    for (int k = 0; k < 3; ++k) L.c[k] = m.kr[k];
    if (m.type == BRE_MATERIAL_MIRROR) {
        if (black3(m.kr)) return b;
        L.kind = kLobeSpecNoOp;
        L.type = kBsdfReflection | kBsdfSpecular;
    } else {
        if (black3(m.kr) && black3(m.kt)) return b;
        L.kind = kLobeFresnelSpec;
        L.type = kBsdfReflection | kBsdfTransmission | kBsdfSpecular;
        for (int k = 0; k < 3; ++k) L.s[k] = m.kt[k];
        L.etaB = m.eta;
    }
    b.lobe[b.n++] = L;
    return b;
}

void make_lobes_mx(const bre_material_ex *table, int n, std::vector<DevLobesMx> *out) {
    out->assign((size_t)n, DevLobesMx{});
    for (int k = 0; k < n; ++k) {
        const bre_material_ex &m = table[k];
        DevLobesMx &w = (*out)[(size_t)k];
        if (m.type != BRE_MATERIAL_MIX) {
            const DevLobes b = make_lobes(m);  // type 0 below BRE_MATERIAL_MATTE
            w.type = b.type;
            w.n = b.n;
            w.n_nonspec = b.n_nonspec;
            for (int i = 0; i < b.n; ++i) static_cast<DevLobe &>(w.lobe[i]) = b.lobe[i];
            continue;
        }
        w.type = BRE_MATERIAL_MIX;
        // s1 = scale->Evaluate(*si).Clamp() (the setter has clamped it), s2 = (Spectrum(1.f) - s1).Clamp()
        float s[2][3];
        for (int c = 0; c < 3; ++c) {
            s[0][c] = m.amount[c];
            s[1][c] = clampf_ref(1.f - s[0][c], 0.f, kMaxFloat);
        }
        for (int side = 0; side < 2; ++side) {
            const int ch = m.mix_child[side];
            if (ch < 0 || ch >= k) continue;  // refused by the setter
            const DevLobesMx from = child_lobes(table[ch], (*out)[(size_t)ch]);
            for (int i = 0; i < from.n && w.n < kMaxLobesMx; ++i) {
                DevLobeMx &L = w.lobe[w.n++];
                L = from.lobe[i];
                if (L.nscale < BRE_MAX_MIX_DEPTH) {
                    for (int c = 0; c < 3; ++c) L.scale[L.nscale][c] = s[side][c];
                    ++L.nscale;
                }
                if (!(L.type & kBsdfSpecular)) ++w.n_nonspec;
            }
        }
    }
}

void prepare_geometry(const bre_scene *s, HostScene *out, const bre_light *lights, int n_lights,
                      const MaterialMap &mm) {
    DevScene &d = out->head;
    d.n_tris = s->n_triangles;
    // the table twice: the narrow records of the mirror / glass / interface entries, and beside them the BSDFs of
    // the plastic / metal / matte ones
    out->mats.resize((size_t)mm.n_mats);
    out->bsdfs.resize((size_t)mm.n_mats);
    // the lobe lists only where a kernel reads them: a table with a rough glass, uber, translucent or substrate entry
    bool lobed = false, mixed = false;
    for (int k = 0; k < mm.n_mats; ++k) {
        lobed = lobed || mm.mats[k].type >= BRE_MATERIAL_ROUGH_GLASS;
        mixed = mixed || mm.mats[k].type == BRE_MATERIAL_MIX;
    }
    // a table that holds a mix: the wide lists instead, which the tier-3 kernels read
    out->lobes_mx.clear();
    if (mixed) {
        make_lobes_mx(mm.mats, mm.n_mats, &out->lobes_mx);
        lobed = false;
    }
    out->lobes.assign(lobed ? (size_t)mm.n_mats : 0, DevLobes{});
    for (int k = 0; k < mm.n_mats; ++k) {
        const bre_material_ex &m = mm.mats[k];
        bre_material &n = out->mats[(size_t)k];
        n.type = m.type;
        for (int c = 0; c < 3; ++c) {
            n.kr[c] = m.kr[c];
            n.kt[c] = m.kt[c];
        }
        n.eta = m.eta;
        out->bsdfs[(size_t)k] = make_bsdf(m);
        if (lobed) out->lobes[(size_t)k] = make_lobes(m);
    }
    const bre_triangle *tri = scene_triangles(s);
    out->tris.resize((size_t)s->n_triangles);
    out->light_tri.clear();
    out->light_func.clear();
    // scene.lights in declaration order: a delta light comes before the area lights of the triangles
    // with index >= its order; equal orders keep their array order (a stable sort by order)
    out->dlights.resize((size_t)n_lights);
    std::vector<int> by_order((size_t)n_lights);
    for (int k = 0; k < n_lights; ++k) {
        out->dlights[(size_t)k] = prepare_light(lights[k]);
        by_order[(size_t)k] = k;
    }
    std::stable_sort(by_order.begin(), by_order.end(), [&](int a, int b) { return lights[a].order < lights[b].order; });
    size_t next = 0;
    const auto delta_up_to = [&](int i) {
        for (; next < by_order.size() && lights[by_order[next]].order <= i; ++next) {
            out->light_tri.push_back(~by_order[next]);
            out->light_func.push_back(light_power_y(out->dlights[(size_t)by_order[next]]));
        }
    };
    for (int i = 0; i < s->n_triangles; ++i) {
        const bre_triangle &t = tri[i];
        PTri &T = out->tris[(size_t)i];
        T.p0 = mk(t.p[0][0], t.p[0][1], t.p[0][2]);
        T.p1 = mk(t.p[1][0], t.p[1][1], t.p[1][2]);
        T.p2 = mk(t.p[2][0], t.p[2][1], t.p[2][2]);
        const f3 dp02 = sub3(T.p0, T.p2), dp12 = sub3(T.p1, T.p2);
        // dpdu for pbrt's default uvs (0,0), (1,0), (1,1): (duv12[1] dp02 - duv02[1] dp12) invdet
        // with duv12[1] = duv02[1] = -1, invdet = 1 (triangle.cpp:276-285)
        const f3 dpdu = scale3(sub3(scale3(dp02, -1.f), scale3(dp12, -1.f)), 1.f);
        T.n = normalize3(cross3d(dp02, dp12));
        T.ns = normalize3(cross3d(sub3(T.p1, T.p0), sub3(T.p2, T.p0)));
        if (t.flip) {
            T.n = neg3(T.n);
            T.ns = neg3(T.ns);
        }
        T.ss = normalize3(dpdu);
        T.ts = cross3d(T.n, T.ss);
        T.area = (float)(0.5 * (double)len3(cross3d(sub3(T.p1, T.p0), sub3(T.p2, T.p0))));
        for (int k = 0; k < 3; ++k) {
            T.kd[k] = t.kd[k];
            T.Le[k] = t.Le[k];
        }
        T.mat = black3(t.kd) ? kMatNone : kMatMatte;
        if (mm.n_mats > 0 && mm.tri_mat[i] >= 0) {
            // mirror.cpp:50-56, glass.cpp:53-64: black Kr (and Kt) adds no BxDF
            const bre_material_ex &m = mm.mats[mm.tri_mat[i]];
            const bool none = black3(m.kr) && (m.type == BRE_MATERIAL_MIRROR || black3(m.kt));
            T.mat = none ? kMatNone : kMatTable + mm.tri_mat[i];
            if (m.type == BRE_MATERIAL_INTERFACE) T.mat = kMatInterface;  // GetMaterial() == nullptr: no BSDF
            if (m.type >= BRE_MATERIAL_ROUGH_GLASS) {
                const int nl = mixed ? out->lobes_mx[(size_t)mm.tri_mat[i]].n : out->lobes[(size_t)mm.tri_mat[i]].n;
                T.mat = nl == 0 ? kMatNone : kMatTable + mm.tri_mat[i];
            } else if (m.type >= BRE_MATERIAL_MATTE) {
                const DevBsdf &b = out->bsdfs[(size_t)mm.tri_mat[i]];
                T.mat = b.lobes == 0 ? kMatNone : kMatTable + mm.tri_mat[i];
                if (b.type == BRE_MATERIAL_MATTE && !b.oren) {
                    // matte.cpp:57-58: the Lambertian lobe of a triangle's own kd, with the entry's Kd
                    for (int k = 0; k < 3; ++k) T.kd[k] = b.kd[k];
                    if (b.lobes) T.mat = kMatMatte;
                }
            }
        }
        T.emit = t.emit == BRE_EMIT_TWO_SIDED ? BRE_EMIT_TWO_SIDED : t.emit != 0;
        if (T.emit) {
            delta_up_to(i);
            out->light_tri.push_back(i);
            // DiffuseAreaLight::Power() = (twoSided ? 2 : 1) * Lemit * area * Pi (diffuse.cpp:64-66), .y()
            const float sides = T.emit == BRE_EMIT_TWO_SIDED ? 2.f : 1.f;
            float pw[3];
            for (int k = 0; k < 3; ++k) pw[k] = ((T.Le[k] * sides) * T.area) * kPi;
            out->light_func.push_back(lum3(pw));
        }
    }
    delta_up_to(s->n_triangles);
    out->depth = build_scene_bvh(out->tris, &out->nodes, &out->prims);
    d.n_nodes = (int)out->nodes.size();
    d.stack_depth = out->depth;
    const int nl = (int)out->light_tri.size();
    d.n_lights = nl;
    // DistantLight::Preprocess(scene): the world's bounding sphere, and with it the light's Power()
    for (int i = 0; i < nl; ++i) {
        if (out->light_tri[(size_t)i] >= 0) continue;
        DLight &D = out->dlights[(size_t)~out->light_tri[(size_t)i]];
        if (D.kind != kLightDistant) continue;
        world_bounding_sphere(out->nodes[0], &D.p, &D.l2w[3]);
        out->light_func[(size_t)i] = light_power_y(D);
    }
    // Distribution1D(func, n) (sampling.h:57-69)
    std::vector<float> &cdf = out->light_cdf;
    const std::vector<float> &func = out->light_func;
    cdf.assign((size_t)nl + 1, 0.f);
    for (int i = 1; i < nl + 1; ++i) cdf[(size_t)i] = cdf[(size_t)i - 1] + func[(size_t)i - 1] / (float)nl;
    d.light_func_int = cdf[(size_t)nl];
    if (d.light_func_int == 0) {
        for (int i = 1; i < nl + 1; ++i) cdf[(size_t)i] = (float)i / (float)nl;
    } else {
        for (int i = 1; i < nl + 1; ++i) cdf[(size_t)i] /= d.light_func_int;
    }
}

}  // namespace bre
