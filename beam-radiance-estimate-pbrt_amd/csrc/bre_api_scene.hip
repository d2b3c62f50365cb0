// bre_api_scene.hip — the scene model behind the C ABI: the sticky setters (bre_set_lights,
// bre_set_materials, bre_set_media) that fill a context's SceneState, the checks of a bre_scene against it,
// the comparison of two states, and upload_scene with its geometry cache, which keeps the SceneDevice.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "bre_ctx.h"

using namespace bre;

namespace {

// v into m on the context's stream, *at the device copy; m holds at least 4 bytes, so an empty array has a pointer
template <typename T>
hipError_t upload(bre_ctx *c, DevMem &m, const std::vector<T> &v, const T **at = nullptr) {
    const hipError_t e = m.ensure(v.empty() ? 4 : v.size() * sizeof(T));
    if (at) *at = m.as<T>();
    if (e != hipSuccess || v.empty()) return e;
    return hipMemcpyAsync(m.ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream);
}

// `bytes` of src into m unless m holds them already (`last`: the bytes it was given last).  A copy is waited
// for: the DMA reads the caller's memory.
bre_status upload_changed(bre_ctx *c, DevMem &m, std::vector<unsigned char> &last, const void *src, size_t bytes) {
    const unsigned char *b = static_cast<const unsigned char *>(src);
    if (m.ptr && last.size() == bytes && memcmp(last.data(), b, bytes) == 0) return BRE_OK;
    HIPCHK(c, m.ensure(bytes));
    HIPCHK(c, hipMemcpyAsync(m.ptr, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    last.assign(b, b + bytes);
    return BRE_OK;
}

// The context's media on the device: the table with its grids behind one another, the pairs and the lights'
// media.  Uploaded when bre_set_media changed them.
bre_status upload_media(bre_ctx *c) {
    const SceneState &h = c->held;
    SceneDevice &dv = c->dev;
    if (!dv.media_stale) return BRE_OK;
    std::vector<DevMedium> table(h.media.size());
    std::vector<float> dens;
    std::vector<size_t> first(h.media.size(), 0);
    for (size_t k = 0; k < h.media.size(); ++k) {
        const bre_medium &m = h.media[k];
        const std::vector<float> &g = h.media_grid[k];  // empty unless a grid
        table[k] = make_medium(m.type, m.sigma_a, m.sigma_s, m.g, m.grid_n, m.world_to_medium, nullptr,
                               max_density(g.data(), (int64_t)g.size()));
        first[k] = dens.size();
        dens.insert(dens.end(), g.begin(), g.end());
    }
    HIPCHK(c, upload(c, dv.md_dens, dens));
    for (size_t k = 0; k < table.size(); ++k)
        if (table[k].medium == BRE_MEDIUM_GRID) table[k].density = dv.md_dens.as<float>() + first[k];
    HIPCHK(c, upload(c, dv.md_table, table));
    HIPCHK(c, upload(c, dv.md_pairs, h.tri_med));
    HIPCHK(c, upload(c, dv.md_light, h.light_med));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
    dv.media_stale = false;
    return BRE_OK;
}

// A byte range of a key.  The lights, materials and material map of a SceneState are compared as such ranges:
// between two contexts (scene_state_differs), and behind the scene's triangles by the geometry cache.
struct KeyPart {
    const void *p;
    size_t bytes;
};
bool same_bytes(const KeyPart &a, const KeyPart &b) {
    return a.bytes == b.bytes && (a.bytes == 0 || memcmp(a.p, b.p, a.bytes) == 0);
}
void state_key(const SceneState &h, KeyPart part[3]) {
    part[0] = {h.lights.data(), h.lights.size() * sizeof(bre_light)};
    part[1] = {h.mats.data(), h.mats.size() * sizeof(bre_material_ex)};
    part[2] = {h.tri_mat.data(), h.tri_mat.size() * sizeof(int32_t)};
}
// the ranges of SceneDevice::bytes: the scene's triangles, then the state's three
void geometry_key(const SceneState &h, const bre_scene *s, KeyPart part[4]) {
    part[0] = {scene_triangles(s), (size_t)s->n_triangles * sizeof(bre_triangle)};
    state_key(h, part + 1);
}

uint64_t hash_bytes(uint64_t h, const void *data, size_t bytes) {
    const unsigned char *p = static_cast<const unsigned char *>(data);
    size_t i = 0;
    for (; i + 8 <= bytes; i += 8) {
        uint64_t w;
        memcpy(&w, p + i, 8);
        h = (h ^ w) * 0x100000001b3ull;
        h ^= h >> 29;
    }
    for (; i < bytes; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

// 64-bit hash of the scene's triangles and the context's lights, materials and material map (the
// geometry cache key of upload_scene); without lights and materials it is the hash of the triangles alone
uint64_t hash_geometry(const bre_scene *s, const KeyPart part[4]) {
    uint64_t h = hash_bytes(0x9e3779b97f4a7c15ull ^ (uint64_t)s->n_triangles, part[0].p, part[0].bytes);
    for (int k = 1; k < 4; ++k)
        if (part[k].bytes) h = hash_bytes(h ^ (uint64_t)(part[k].bytes * (size_t)k), part[k].p, part[k].bytes);
    return h | 1ull;  // never 0 (= no scene)
}

// A rough glass, uber, translucent or substrate record (types 8 .. 11): the fields its type reads are finite, its
// alphas are > 0 after the material's own fallbacks and mapping (glass.cpp:66-69, uber.cpp:72-83,
// translucent.cpp:66-68, substrate.cpp:57-60), and every field it does not read is 0; its colours are clamped.
std::string check_lobed_material(bre_material_ex &m) {
    static const char *const kName[4] = {"rough glass", "uber", "translucent", "substrate"};
    const std::string name = kName[m.type - BRE_MATERIAL_ROUGH_GLASS];
    const bool glass = m.type == BRE_MATERIAL_ROUGH_GLASS, uber = m.type == BRE_MATERIAL_UBER;
    const bool trans = m.type == BRE_MATERIAL_TRANSLUCENT;
    struct Field {
        const char *name;
        float *v;
        int n;
        bool read, colour;
    };
    const Field fields[] = {
        {trans ? "reflect" : "Kr", m.kr, 3, glass || uber || trans, true},
        {trans ? "transmit" : "Kt", m.kt, 3, glass || uber || trans, true},
        {"eta", &m.eta, 1, glass || uber, false},          {"Kd", m.kd, 3, !glass, true},
        {"Ks", m.ks, 3, !glass, true},                     {"opacity", m.opacity, 3, uber, true},
        {"k", m.ck, 3, false, false},                      {"roughness", &m.roughness, 1, uber || trans, false},
        {"uroughness", &m.uroughness, 1, !trans, false},   {"vroughness", &m.vroughness, 1, !trans, false},
        {"sigma", &m.sigma, 1, false, false},
    };
    for (const Field &f : fields)
        for (int j = 0; j < f.n; ++j) {
            if (f.read && !std::isfinite(f.v[j])) return "a non-finite " + std::string(f.name) + " (" + name + ")";
            if (!f.read && !(f.v[j] == 0))  // a NaN too
                return std::string(std::isfinite(f.v[j]) ? "a non-zero " : "a non-finite ") + f.name + ", which a " + name +
                       " does not read" +
                       (f.v == m.opacity ? " (opacity shares the storage of the metal's eta)" : "");
        }
    if (m.remap != 0 && m.remap != 1) return "a remap that is not 0 or 1 (" + name + ")";
    if ((glass || uber) && !(m.eta > 0)) {
        char buf[96];
        snprintf(buf, sizeof(buf), "eta %g (must be finite and > 0; %s)", m.eta, name.c_str());
        return buf;
    }
    if (glass && m.uroughness == 0 && m.vroughness == 0)
        return "uroughness and vroughness both 0 (rough glass): that is BRE_MATERIAL_GLASS";
    float u, v;
    if (uber) {
        u = m.uroughness != 0 ? m.uroughness : m.roughness;
        v = m.vroughness != 0 ? m.vroughness : u;
    } else if (trans) {
        u = v = m.roughness;
    } else {
        u = m.uroughness;
        v = m.vroughness;
    }
    if (m.remap) {
        u = roughness_to_alpha(u);
        v = roughness_to_alpha(v);
    }
    if (!(u > 0) || !(v > 0))
        return "an alpha that is not > 0 (" + name + ": the roughnesses after " +
               (m.remap ? "RoughnessToAlpha" : "the fallbacks, remaproughness false") + ")";
    for (const Field &f : fields)
        if (f.read && f.colour)
            for (int j = 0; j < 3; ++j) f.v[j] = f.v[j] < 0.f ? 0.f : (f.v[j] > 1.f ? 1.f : f.v[j]);
    return "";
}

// A mix record (type 12): it reads `amount` (the words of kd) and its two children (the words of reserved[0..1]) and
// nothing else; amount is clamped.
std::string check_mix_material(bre_material_ex &m) {
    struct Field {
        const char *name;
        const float *v;
        int n;
    };
    const Field unread[] = {{"Kr", m.kr, 3},           {"Kt", m.kt, 3},
                            {"eta", &m.eta, 1},        {"Ks", m.ks, 3},
                            {"metal eta", m.ceta, 3},  {"k", m.ck, 3},
                            {"roughness", &m.roughness, 1},   {"uroughness", &m.uroughness, 1},
                            {"vroughness", &m.vroughness, 1}, {"sigma", &m.sigma, 1}};
    for (int j = 0; j < 3; ++j)
        if (!std::isfinite(m.amount[j])) return "a non-finite amount (mix)";
    for (int j = 0; j < 2; ++j)
        if (m.mix_child[j] < 0) {
            char buf[96];
            snprintf(buf, sizeof(buf), "a negative child index %d (mix: mix_child[%d])", m.mix_child[j], j);
            return buf;
        }
    if (m.reserved[2] != 0) return "a non-zero reserved[2] (mix: only reserved[0..1] hold its children)";
    for (const Field &f : unread)
        for (int j = 0; j < f.n; ++j)
            if (!(f.v[j] == 0))  // a NaN too
                return std::string(std::isfinite(f.v[j]) ? "a non-zero " : "a non-finite ") + f.name +
                       ", which a mix does not read";
    if (m.remap != 0) return "a non-zero remap, which a mix does not read";
    for (int j = 0; j < 3; ++j) m.amount[j] = m.amount[j] < 0.f ? 0.f : (m.amount[j] > 1.f ? 1.f : m.amount[j]);
    return "";
}

// One record of the table as the context keeps it: checked, colours clamped, unused fields left as given (equal
// tables compare equal).  `wide`: types past BRE_MATERIAL_INTERFACE are known.  Returns "", or what the material
// has that is wrong (the narrow cases in bre_set_materials's words).
std::string check_material(bre_material_ex &m, bool wide, bool media, bool *is_interface) {
    *is_interface = false;
    const auto finite3 = [](const float v[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); };
    const auto clamp3 = [](float v[3]) {
        for (int j = 0; j < 3; ++j) v[j] = v[j] < 0.f ? 0.f : (v[j] > 1.f ? 1.f : v[j]);
    };
    char buf[160];
    if (wide && m.type == BRE_MATERIAL_MIX) return check_mix_material(m);
    if (m.reserved[0] || m.reserved[1] || m.reserved[2]) return "non-zero reserved words";
    if (m.type == BRE_MATERIAL_INTERFACE && media) {
        // no BSDF: every parameter is ignored (kept as zeros, so that equal tables compare equal)
        m = bre_material_ex{};
        m.type = BRE_MATERIAL_INTERFACE;
        *is_interface = true;
        return "";
    }
    if (m.type == BRE_MATERIAL_MIRROR || m.type == BRE_MATERIAL_GLASS) {
        if (!std::isfinite(m.eta) || !(m.eta > 0)) {
            snprintf(buf, sizeof(buf), "eta %g (must be finite and > 0)", m.eta);
            return buf;
        }
        if (!finite3(m.kr) || !finite3(m.kt)) return "a non-finite Kr or Kt";
        // Kr->Evaluate(*si).Clamp() (mirror.cpp:52, glass.cpp:54-55) bounds the value below by 0; the ABI
        // also bounds it above by 1 (a reflectance), which a physical scene file never exceeds
        clamp3(m.kr);
        clamp3(m.kt);
        return "";
    }
    if (wide && m.type >= BRE_MATERIAL_ROUGH_GLASS && m.type <= BRE_MATERIAL_SUBSTRATE) return check_lobed_material(m);
    if (!wide || m.type < BRE_MATERIAL_MATTE || m.type > BRE_MATERIAL_METAL) {
        snprintf(buf, sizeof(buf), "unknown type %d%s", m.type,
                 m.type == BRE_MATERIAL_INTERFACE ? " (BRE_MATERIAL_INTERFACE needs bre_set_media first)" : "");
        return buf;
    }
    if (m.type == BRE_MATERIAL_MATTE) {
        if (!finite3(m.kd) || !std::isfinite(m.sigma)) return "a non-finite Kd or sigma";
        clamp3(m.kd);
        return "";
    }
    if (m.remap != 0 && m.remap != 1) return "a remap that is not 0 or 1";
    if (m.type == BRE_MATERIAL_PLASTIC) {
        if (!finite3(m.kd) || !finite3(m.ks) || !std::isfinite(m.roughness)) return "a non-finite Kd, Ks or roughness";
        if (!(m.roughness > 0)) return "a roughness that is not > 0";
        clamp3(m.kd);
        clamp3(m.ks);
        return "";
    }
    if (!finite3(m.ceta) || !finite3(m.ck) || !std::isfinite(m.roughness) || !std::isfinite(m.uroughness) ||
        !std::isfinite(m.vroughness))
        return "a non-finite eta, k or roughness";
    if (m.ceta[0] == 0 || m.ceta[1] == 0 || m.ceta[2] == 0) return "an eta channel of 0";
    const float u = m.uroughness != 0 ? m.uroughness : m.roughness, v = m.vroughness != 0 ? m.vroughness : m.roughness;
    if (!(u > 0) || !(v > 0)) return "a roughness that is not > 0 (uroughness / vroughness after the fallback to roughness)";
    return "";
}

// The rules between the records of a checked table, which a mix brings: its children come earlier (the parser's
// declaration order; no cycles) and have a BSDF, it nests at most BRE_MAX_MIX_DEPTH deep and expands to at most
// BRE_MAX_BXDFS BxDFs (BSDF::Add CHECK_LTs against MaxBxDFs, reflection.h:166).  Returns "" or what material *bad has.
std::string check_mix_table(const std::vector<bre_material_ex> &mats, int *bad) {
    const size_t n = mats.size();
    std::vector<int> depth(n, 0), count(n, 0);
    char buf[200];
    for (size_t k = 0; k < n; ++k) {
        const bre_material_ex &m = mats[k];
        *bad = (int)k;
        if (m.type != BRE_MATERIAL_MIX) {
            if (m.type == BRE_MATERIAL_MIRROR) count[k] = black3(m.kr) ? 0 : 1;
            else if (m.type == BRE_MATERIAL_GLASS) count[k] = black3(m.kr) && black3(m.kt) ? 0 : 1;
            else count[k] = make_lobes(m).n;  // 0 for an interface
            continue;
        }
        for (int j = 0; j < 2; ++j) {
            const int ch = m.mix_child[j];
            if (ch >= (int)k) {
                snprintf(buf, sizeof(buf), "child %d (mix_child[%d]) that does not come before it: a mix's children are "
                         "earlier entries of the table", ch, j);
                return buf;
            }
            if (mats[(size_t)ch].type == BRE_MATERIAL_INTERFACE) {
                snprintf(buf, sizeof(buf), "child %d (mix_child[%d]) that is a BRE_MATERIAL_INTERFACE, which has no BSDF "
                         "to scale", ch, j);
                return buf;
            }
            depth[k] = std::max(depth[k], depth[(size_t)ch] + 1);
            count[k] += count[(size_t)ch];
        }
        if (depth[k] > BRE_MAX_MIX_DEPTH) {
            snprintf(buf, sizeof(buf), "a nest %d mixes deep (at most BRE_MAX_MIX_DEPTH = %d)", depth[k], BRE_MAX_MIX_DEPTH);
            return buf;
        }
        if (count[k] > BRE_MAX_BXDFS) {
            snprintf(buf, sizeof(buf), "%d BxDFs after expansion (at most BRE_MAX_BXDFS = %d, the reference's "
                     "BSDF::MaxBxDFs)", count[k], BRE_MAX_BXDFS);
            return buf;
        }
    }
    return "";
}

bre_status set_material_table(bre_ctx *c, const char *fn, const bre_material_ex *materials, int32_t n_materials,
                              const int32_t *triangle_material, int64_t n_triangles, bool wide) {
    if (n_materials < 0 || n_materials > BRE_MAX_MATERIALS)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: material count must be in 0..%d", fn, BRE_MAX_MATERIALS);
    if (n_materials == 0) {
        c->held.mats.clear();
        c->held.tri_mat.clear();
        c->held.has_interface = false;
        c->held.glossy = false;
        c->held.lobed = false;
        c->held.mixed = false;
        return BRE_OK;
    }
    if (n_triangles < 0 || n_triangles > BRE_MAX_SCENE_TRIANGLES)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: the material map's triangle count must be in 0..%d", fn,
                    BRE_MAX_SCENE_TRIANGLES);
    if (!materials || (n_triangles > 0 && !triangle_material))
        return fail(c, BRE_ERR_INVALID_ARG, "%s: null material table or triangle_material map", fn);
    std::vector<bre_material_ex> mats(materials, materials + n_materials);
    std::vector<char> is_interface((size_t)n_materials, 0);
    bool glossy = false, lobed = false, mixed = false;
    for (int k = 0; k < n_materials; ++k) {
        bool iface = false;
        const std::string what = check_material(mats[(size_t)k], wide, !c->held.media.empty(), &iface);
        if (!what.empty()) return fail(c, BRE_ERR_INVALID_ARG, "%s: material %d has %s", fn, k, what.c_str());
        is_interface[(size_t)k] = iface;
        glossy = glossy || mats[(size_t)k].type >= BRE_MATERIAL_MATTE;
        lobed = lobed || mats[(size_t)k].type >= BRE_MATERIAL_ROUGH_GLASS;
        mixed = mixed || mats[(size_t)k].type == BRE_MATERIAL_MIX;
    }
    if (mixed) {
        int bad = 0;
        const std::string what = check_mix_table(mats, &bad);
        if (!what.empty()) return fail(c, BRE_ERR_INVALID_ARG, "%s: material %d has %s", fn, bad, what.c_str());
    }
    for (int64_t i = 0; i < n_triangles; ++i)
        if (triangle_material[i] < -1 || triangle_material[i] >= n_materials)
            return fail(c, BRE_ERR_INVALID_ARG, "%s: triangle %lld has material index %d outside [-1, %d)", fn,
                        (long long)i, triangle_material[i], n_materials);
    c->held.mats.swap(mats);
    c->held.tri_mat.assign(triangle_material, triangle_material + n_triangles);
    c->held.has_interface = false;
    c->held.glossy = glossy;
    c->held.lobed = lobed;
    c->held.mixed = mixed;
    for (int64_t i = 0; i < n_triangles; ++i)
        if (triangle_material[i] >= 0 && is_interface[(size_t)triangle_material[i]]) c->held.has_interface = true;
    return BRE_OK;
}

}  // namespace

namespace bre {

std::string check_glossy_material(bre_material_ex &m) {
    bool iface;
    if (m.type < BRE_MATERIAL_MATTE || m.type > BRE_MATERIAL_METAL)
        return "a type outside BRE_MATERIAL_MATTE .. BRE_MATERIAL_METAL";
    return check_material(m, true, false, &iface);
}

std::string check_material_table(std::vector<bre_material_ex> &mats, int *bad) {
    bool mixed = false;
    for (size_t k = 0; k < mats.size(); ++k) {
        bool iface;
        *bad = (int)k;
        const std::string what = check_material(mats[k], true, false, &iface);
        if (!what.empty()) return what;
        mixed = mixed || mats[k].type == BRE_MATERIAL_MIX;
    }
    return mixed ? check_mix_table(mats, bad) : std::string();
}

std::string check_lobed_or_glossy_material(bre_material_ex &m) {
    bool iface;
    if (m.type < BRE_MATERIAL_MATTE) return "a type below BRE_MATERIAL_MATTE";
    return check_material(m, true, false, &iface);
}

const char *scene_state_differs(const SceneState &a, const SceneState &b) {
    KeyPart ka[3], kb[3];
    state_key(a, ka);
    state_key(b, kb);
    if (!same_bytes(ka[0], kb[0])) return "lights (bre_set_lights)";
    // the stored table is the clamped one on both sides
    if (!same_bytes(ka[1], kb[1]) || !same_bytes(ka[2], kb[2])) return "materials (bre_set_materials)";
    if (a.media_key != b.media_key) return "media (bre_set_media)";
    return nullptr;
}

// Medium parameters: GridDensityMedium needs a density grid with a positive maximum (the ctor's
// invMaxDensity = 1/maxDensity, grid.h:73-76); a non-uniform sigma_t is accepted as pbrt does
// (its Error() only reports it, grid.h:66-70) and channel 0 is used.
bre_status check_medium(bre_ctx *c, const bre_scene *scene, const char *fn) {
    if (!scene) return fail(c, BRE_ERR_INVALID_ARG, "%s: null scene", fn);
    if (scene->has_medium < BRE_MEDIUM_NONE || scene->has_medium > BRE_MEDIUM_GRID)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: unknown medium type %d", fn, scene->has_medium);
    if (scene->has_medium != BRE_MEDIUM_GRID) return BRE_OK;
    const int64_t nx = scene->grid_n[0], ny = scene->grid_n[1], nz = scene->grid_n[2];
    if (nx < 1 || ny < 1 || nz < 1 || nx * ny * nz > BRE_MAX_GRID_CELLS)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: grid dimensions must be >= 1 with at most %d cells", fn,
                    BRE_MAX_GRID_CELLS);
    if (!scene->grid_density) return fail(c, BRE_ERR_INVALID_ARG, "%s: null grid_density", fn);
    if (!(grid_max_density(scene) > 0))
        return fail(c, BRE_ERR_INVALID_ARG, "%s: grid density maximum must be > 0", fn);
    return BRE_OK;
}

// Triangle count in range and at least one light: an emitting triangle, or a delta light of the context
// (the passes need scene.lights non-empty); every delta light's order within the triangle count
bre_status check_scene(bre_ctx *c, const bre_scene *scene, const char *fn) {
    if (!scene) return fail(c, BRE_ERR_INVALID_ARG, "%s: null scene", fn);
    const SceneState &h = c->held;
    const int cap = scene->triangles_ext ? BRE_MAX_SCENE_TRIANGLES : BRE_MAX_TRIANGLES;
    if (scene->n_triangles < 1 || scene->n_triangles > cap)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: triangle count must be in 1..%d (%s)", fn, cap,
                    scene->triangles_ext ? "triangles_ext" : "inline triangles; use triangles_ext for more");
    const bre_triangle *tri = scene_triangles(scene);
    int64_t lights = 0;
    for (int i = 0; i < scene->n_triangles; ++i) lights += tri[i].emit != 0;
    if (lights == 0 && h.lights.empty()) return fail(c, BRE_ERR_INVALID_ARG, "%s: the scene has no area light", fn);
    for (size_t k = 0; k < h.lights.size(); ++k)
        if (h.lights[k].order > scene->n_triangles)
            return fail(c, BRE_ERR_INVALID_ARG, "%s: light %d has order %d, the scene has %d triangles", fn, (int)k,
                        h.lights[k].order, scene->n_triangles);
    if (!h.mats.empty() && h.tri_mat.size() != (size_t)scene->n_triangles)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: the material map (bre_set_materials) covers %lld triangles, the scene "
                    "has %d", fn, (long long)h.tri_mat.size(), scene->n_triangles);
    // A DistantLight has an empty MediumInterface (distant.cpp:45): its photons start in vacuum.  The one-medium
    // model ("every ray travels in it") cannot say that; the media table can, with -1 for the light.
    bool distant = false;
    for (size_t k = 0; k < h.lights.size(); ++k) distant = distant || h.lights[k].type == BRE_LIGHT_DISTANT;
    if (distant && h.media.empty() && scene->has_medium != BRE_MEDIUM_NONE)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: the context holds a distant light, whose photons start in vacuum: a "
                    "scene with a medium of its own (has_medium) cannot hold it; bound the medium with surfaces "
                    "(bre_set_media)", fn);
    if (h.media.empty()) {
        if (h.has_interface)
            return fail(c, BRE_ERR_INVALID_ARG, "%s: a BRE_MATERIAL_INTERFACE triangle needs the context's media "
                        "(bre_set_media)", fn);
        return BRE_OK;
    }
    // two sources of media would be ambiguous
    if (scene->has_medium != BRE_MEDIUM_NONE)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: the context holds media (bre_set_media): the scene's has_medium must "
                    "be BRE_MEDIUM_NONE", fn);
    if (h.tri_med.size() != 2 * (size_t)scene->n_triangles)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: the media pairs (bre_set_media) cover %lld triangles, the scene has %d",
                    fn, (long long)(h.tri_med.size() / 2), scene->n_triangles);
    if (h.light_med.size() != h.lights.size())
        return fail(c, BRE_ERR_INVALID_ARG, "%s: the media (bre_set_media) name %lld delta lights, the context holds "
                    "%lld", fn, (long long)h.light_med.size(), (long long)h.lights.size());
    for (size_t k = 0; k < h.lights.size(); ++k)
        if (h.lights[k].type == BRE_LIGHT_DISTANT && h.light_med[k] != -1)
            return fail(c, BRE_ERR_INVALID_ARG, "%s: distant light %d has medium %d (bre_set_media): a distant light "
                        "is in vacuum, its medium must be -1", fn, (int)k, h.light_med[k]);
    return BRE_OK;
}

// DevScene (+ the density grid of a GridDensityMedium) into dev.record on the context's stream.  The
// geometry (triangles, BVHAccel, lights, materials) is rebuilt and uploaded only when the triangles, the
// context's lights or its materials change.
bre_status upload_scene(bre_ctx *c, const bre_scene *scene) {
    const SceneState &h = c->held;
    SceneDevice &dv = c->dev;
    float *dd = nullptr;
    if (scene->has_medium == BRE_MEDIUM_GRID) {
        // copied only when the density values change (every pass of a render shares one grid)
        const size_t n = (size_t)scene->grid_n[0] * scene->grid_n[1] * scene->grid_n[2];
        BRE_TRY(upload_changed(c, dv.grid, dv.grid_bytes, scene->grid_density, n * sizeof(float)));
        dd = dv.grid.as<float>();
    }
    KeyPart part[4];
    geometry_key(h, scene, part);
    const uint64_t hash = hash_geometry(scene, part);
    // the geometry is reused only when the hash AND the bytes match (a hash collision between two
    // scenes must not trace against the stale BVH, lights and materials)
    bool same = hash == dv.hash;
    for (int k = 0; k < 4; ++k) same = same && same_bytes({dv.bytes[k].data(), dv.bytes[k].size()}, part[k]);
    if (!same) {
        HostScene hs;
        const MaterialMap mm{h.mats.data(), (int)h.mats.size(), h.tri_mat.data()};
        prepare_geometry(scene, &hs, h.lights.data(), (int)h.lights.size(), mm);
        if (hs.depth > kSceneStack)
            return fail(c, BRE_ERR_INVALID_ARG, "scene BVH depth %d exceeds the %d-entry traversal stack (as in "
                        "BVHAccel::Intersect)", hs.depth, kSceneStack);
        dv.hash = 0;  // the cached geometry is overwritten from here on
        dv.head = hs.head;
        HIPCHK(c, upload(c, dv.tris, hs.tris, &dv.head.t));
        HIPCHK(c, upload(c, dv.nodes, hs.nodes, &dv.head.nodes));
        HIPCHK(c, upload(c, dv.prims, hs.prims, &dv.head.prims));
        HIPCHK(c, upload(c, dv.light_tri, hs.light_tri, &dv.head.light_tri));
        HIPCHK(c, upload(c, dv.light_func, hs.light_func, &dv.head.light_func));
        HIPCHK(c, upload(c, dv.light_cdf, hs.light_cdf, &dv.head.light_cdf));
        HIPCHK(c, upload(c, dv.dlights, hs.dlights, &dv.head.dlights));
        HIPCHK(c, upload(c, dv.mats, hs.mats, &dv.head.mats));
        HIPCHK(c, upload(c, dv.bsdfs, hs.bsdfs, &dv.head.bsdfs));
        HIPCHK(c, upload(c, dv.lobes, hs.lobes, &dv.head.lobes));
        dv.head.lobes_mx = nullptr;  // only a table that holds a mix has the wide lists
        if (!hs.lobes_mx.empty()) HIPCHK(c, upload(c, dv.lobes_mx, hs.lobes_mx, &dv.head.lobes_mx));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
        dv.hash = hash;
        for (int k = 0; k < 4; ++k) {
            const unsigned char *b = static_cast<const unsigned char *>(part[k].p);
            dv.bytes[k].assign(b, b + part[k].bytes);
        }
    }
    DevScene ds;
    memcpy(&ds, &dv.head, sizeof(DevScene));  // padding bytes included: the record compares bytewise
    prepare_medium(scene, &ds, dd);
    const bool media = !h.media.empty();  // (cleared media leave cam_med at -1)
    if (media) BRE_TRY(upload_media(c));
    ds.media = media ? dv.md_table.as<DevMedium>() : nullptr;
    ds.tri_med = media ? dv.md_pairs.as<int32_t>() : nullptr;
    ds.light_med = media ? dv.md_light.as<int32_t>() : nullptr;
    ds.n_media = (int)h.media.size();
    ds.cam_med = h.cam_med;
    // the scene record is copied only when it changes: in a render every pass uploads the same record,
    // and a copy queued behind another context's gather waits for that gather's blocks (round 5 trace:
    // a 1.6 KB upload took 110 ms in the two-context pipeline)
    return upload_changed(c, dv.record, dv.record_bytes, &ds, sizeof(DevScene));
}

}  // namespace bre

extern "C" {

bre_status bre_check_material_ex(const bre_material_ex *material, char *message, int32_t capacity) {
    if (message && capacity > 0) message[0] = 0;
    if (!material) return BRE_ERR_INVALID_ARG;
    bre_material_ex m = *material;
    bool iface = false;
    const std::string what = check_material(m, true, false, &iface);
    if (what.empty()) return BRE_OK;
    if (message && capacity > 0) snprintf(message, (size_t)capacity, "%s", what.c_str());
    return BRE_ERR_INVALID_ARG;
}

bre_status bre_check_material_table_ex(const bre_material_ex *materials, int32_t n_materials, char *message,
                                       int32_t capacity) {
    if (message && capacity > 0) message[0] = 0;
    if (!materials || n_materials < 0 || n_materials > BRE_MAX_MATERIALS) return BRE_ERR_INVALID_ARG;
    std::vector<bre_material_ex> mats(materials, materials + n_materials);
    int bad = 0;
    const std::string what = check_material_table(mats, &bad);
    if (what.empty()) return BRE_OK;
    if (message && capacity > 0) snprintf(message, (size_t)capacity, "material %d has %s", bad, what.c_str());
    return BRE_ERR_INVALID_ARG;
}

bre_status bre_set_lights(bre_ctx *c, const bre_light *lights, int32_t n) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (n < 0 || n > BRE_MAX_LIGHTS)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_set_lights: light count must be in 0..%d", BRE_MAX_LIGHTS);
    if (n > 0 && !lights) return fail(c, BRE_ERR_INVALID_ARG, "bre_set_lights: null lights");
    for (int k = 0; k < n; ++k) {
        const bre_light &l = lights[k];
        if (l.type != BRE_LIGHT_POINT && l.type != BRE_LIGHT_SPOT && l.type != BRE_LIGHT_DISTANT)
            return fail(c, BRE_ERR_INVALID_ARG, "bre_set_lights: light %d has unknown type %d", k, l.type);
        if (l.order < 0) return fail(c, BRE_ERR_INVALID_ARG, "bre_set_lights: light %d has a negative order", k);
        bool finite = std::isfinite(l.cone_total_deg) && std::isfinite(l.cone_falloff_start_deg);
        for (int j = 0; j < 3; ++j) finite = finite && std::isfinite(l.I[j]);
        for (int j = 0; j < 16; ++j)
            finite = finite && std::isfinite(l.light_to_world[j]) && std::isfinite(l.world_to_light[j]);
        if (!finite) return fail(c, BRE_ERR_INVALID_ARG, "bre_set_lights: light %d has a non-finite field", k);
        if (l.type != BRE_LIGHT_DISTANT) continue;
        // a DistantLight: wLight (light_to_world[0..2]) is a direction, L a radiance, the fields it does not read 0
        if (l.light_to_world[0] == 0 && l.light_to_world[1] == 0 && l.light_to_world[2] == 0)
            return fail(c, BRE_ERR_INVALID_ARG, "bre_set_lights: light %d (distant) has a zero wLight", k);
        if (l.I[0] < 0 || l.I[1] < 0 || l.I[2] < 0)
            return fail(c, BRE_ERR_INVALID_ARG, "bre_set_lights: light %d (distant) has a negative L", k);
        bool zero = l.cone_total_deg == 0 && l.cone_falloff_start_deg == 0;
        for (int j = 3; j < 16; ++j) zero = zero && l.light_to_world[j] == 0;
        for (int j = 0; j < 16; ++j) zero = zero && l.world_to_light[j] == 0;
        if (!zero)
            return fail(c, BRE_ERR_INVALID_ARG, "bre_set_lights: light %d (distant) has a non-zero reserved field "
                        "(light_to_world[3..15], world_to_light, the cone angles)", k);
    }
    c->held.lights.assign(lights, lights + n);
    return BRE_OK;
}

bre_status bre_set_materials_ex(bre_ctx *c, const bre_material_ex *materials, int32_t n_materials,
                                const int32_t *triangle_material, int64_t n_triangles) {
    if (!c) return BRE_ERR_INVALID_ARG;
    return set_material_table(c, "bre_set_materials_ex", materials, n_materials, triangle_material, n_triangles, true);
}

// the widening of its records: the same table
bre_status bre_set_materials(bre_ctx *c, const bre_material *materials, int32_t n_materials,
                             const int32_t *triangle_material, int64_t n_triangles) {
    if (!c) return BRE_ERR_INVALID_ARG;
    std::vector<bre_material_ex> wide;
    if (materials && n_materials > 0 && n_materials <= BRE_MAX_MATERIALS) {
        wide.assign((size_t)n_materials, bre_material_ex{});
        for (int k = 0; k < n_materials; ++k) std::memcpy(&wide[(size_t)k], &materials[k], sizeof(bre_material));
    }
    return set_material_table(c, "bre_set_materials", materials ? wide.data() : nullptr, n_materials, triangle_material,
                              n_triangles, false);
}

bre_status bre_set_media(bre_ctx *c, const bre_medium *media, int32_t n_media, const int32_t *tri_inside,
                         const int32_t *tri_outside, int64_t n_triangles, int32_t camera_medium,
                         const int32_t *light_medium, int32_t n_lights) {
    if (!c) return BRE_ERR_INVALID_ARG;
    const char *fn = "bre_set_media";
    if (n_media < 0 || n_media > BRE_MAX_MEDIA)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: medium count must be in 0..%d", fn, BRE_MAX_MEDIA);
    if (n_media == 0) {
        c->held.media.clear();
        c->held.media_grid.clear();
        c->held.tri_med.clear();
        c->held.light_med.clear();
        c->held.media_key.clear();
        c->held.cam_med = -1;
        c->dev.media_stale = true;
        return BRE_OK;
    }
    if (n_triangles < 0 || n_triangles > BRE_MAX_SCENE_TRIANGLES)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: the media pairs' triangle count must be in 0..%d", fn,
                    BRE_MAX_SCENE_TRIANGLES);
    if (n_lights < 0 || n_lights > BRE_MAX_LIGHTS)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: the light media count must be in 0..%d", fn, BRE_MAX_LIGHTS);
    if (!media || (n_triangles > 0 && (!tri_inside || !tri_outside)) || (n_lights > 0 && !light_medium))
        return fail(c, BRE_ERR_INVALID_ARG, "%s: null media table, triangle pair array or light media array", fn);
    const auto index_ok = [&](int32_t v) { return v >= -1 && v < n_media; };
    int64_t cells = 0;
    for (int k = 0; k < n_media; ++k) {
        const bre_medium &m = media[k];
        if (m.type != BRE_MEDIUM_HOMOGENEOUS && m.type != BRE_MEDIUM_GRID)
            return fail(c, BRE_ERR_INVALID_ARG, "%s: medium %d has unknown type %d", fn, k, m.type);
        for (int j = 0; j < 3; ++j)
            if (!std::isfinite(m.sigma_a[j]) || !std::isfinite(m.sigma_s[j]) || m.sigma_a[j] < 0 || m.sigma_s[j] < 0)
                return fail(c, BRE_ERR_INVALID_ARG, "%s: medium %d has a non-finite or negative sigma", fn, k);
        if (!std::isfinite(m.g) || std::fabs(m.g) > 1)
            return fail(c, BRE_ERR_INVALID_ARG, "%s: medium %d has g %g (|g| must be <= 1)", fn, k, m.g);
        if (m.type != BRE_MEDIUM_GRID) continue;
        const float st0 = m.sigma_a[0] + m.sigma_s[0];
        if (m.sigma_a[1] + m.sigma_s[1] != st0 || m.sigma_a[2] + m.sigma_s[2] != st0)
            return fail(c, BRE_ERR_INVALID_ARG, "%s: grid medium %d: sigma_a + sigma_s must be spectrally uniform", fn, k);
        const int64_t nx = m.grid_n[0], ny = m.grid_n[1], nz = m.grid_n[2];
        if (nx < 1 || ny < 1 || nz < 1 || nx * ny * nz > BRE_MAX_GRID_CELLS || (cells += nx * ny * nz) > BRE_MAX_GRID_CELLS)
            return fail(c, BRE_ERR_INVALID_ARG, "%s: grid medium %d: dimensions must be >= 1, with at most %d cells "
                        "over the table", fn, k, BRE_MAX_GRID_CELLS);
        if (!m.grid_density) return fail(c, BRE_ERR_INVALID_ARG, "%s: grid medium %d has a null density", fn, k);
        const float mx = max_density(m.grid_density, nx * ny * nz);
        if (!(mx > 0) || !std::isfinite(mx))
            return fail(c, BRE_ERR_INVALID_ARG, "%s: grid medium %d: the density maximum must be finite and > 0", fn, k);
    }
    for (int64_t i = 0; i < n_triangles; ++i)
        if (!index_ok(tri_inside[i]) || !index_ok(tri_outside[i]))
            return fail(c, BRE_ERR_INVALID_ARG, "%s: triangle %lld has a medium index outside [-1, %d)", fn, (long long)i,
                        n_media);
    if (!index_ok(camera_medium))
        return fail(c, BRE_ERR_INVALID_ARG, "%s: the camera medium index %d is outside [-1, %d)", fn, camera_medium, n_media);
    for (int j = 0; j < n_lights; ++j)
        if (!index_ok(light_medium[j]))
            return fail(c, BRE_ERR_INVALID_ARG, "%s: light %d has a medium index outside [-1, %d)", fn, j, n_media);
    // accepted: copy everything, the grids included
    std::vector<unsigned char> key;
    const auto put = [&](const void *p, size_t bytes) {
        const unsigned char *b = static_cast<const unsigned char *>(p);
        key.insert(key.end(), b, b + bytes);
    };
    c->held.media.assign(media, media + n_media);
    c->held.media_grid.assign((size_t)n_media, std::vector<float>());
    for (int k = 0; k < n_media; ++k) {
        bre_medium &m = c->held.media[(size_t)k];
        m.reserved = 0;
        if (m.type == BRE_MEDIUM_GRID) {
            const size_t n = (size_t)m.grid_n[0] * m.grid_n[1] * m.grid_n[2];
            c->held.media_grid[(size_t)k].assign(m.grid_density, m.grid_density + n);
            m.grid_density = c->held.media_grid[(size_t)k].data();
        } else {
            m.grid_density = nullptr;
        }
        put(&m, offsetof(bre_medium, grid_density));
        put(c->held.media_grid[(size_t)k].data(), c->held.media_grid[(size_t)k].size() * sizeof(float));
    }
    c->held.tri_med.resize(2 * (size_t)n_triangles);
    for (int64_t i = 0; i < n_triangles; ++i) {
        c->held.tri_med[2 * (size_t)i] = tri_inside[i];
        c->held.tri_med[2 * (size_t)i + 1] = tri_outside[i];
    }
    c->held.light_med.assign(light_medium, light_medium + n_lights);
    c->held.cam_med = camera_medium;
    put(c->held.tri_med.data(), c->held.tri_med.size() * sizeof(int32_t));
    put(c->held.light_med.data(), c->held.light_med.size() * sizeof(int32_t));
    put(&camera_medium, sizeof(camera_medium));
    c->held.media_key.swap(key);
    c->dev.media_stale = true;
    return BRE_OK;
}

}  // extern "C"
