// bre_api_pass.hip — the photon and camera passes behind the C ABI: scene and medium checks, the
// scene upload with its geometry cache, bre_trace_photons, bre_camera_pass, bre_get_segments and the
// bre_render* loops over them.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "bre_ctx.h"

using namespace bre;

namespace {

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
    const int cap = scene->triangles_ext ? BRE_MAX_SCENE_TRIANGLES : BRE_MAX_TRIANGLES;
    if (scene->n_triangles < 1 || scene->n_triangles > cap)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: triangle count must be in 1..%d (%s)", fn, cap,
                    scene->triangles_ext ? "triangles_ext" : "inline triangles; use triangles_ext for more");
    const bre_triangle *tri = scene_triangles(scene);
    int64_t lights = 0;
    for (int i = 0; i < scene->n_triangles; ++i) lights += tri[i].emit != 0;
    if (lights == 0 && c->lights.empty()) return fail(c, BRE_ERR_INVALID_ARG, "%s: the scene has no area light", fn);
    for (size_t k = 0; k < c->lights.size(); ++k)
        if (c->lights[k].order > scene->n_triangles)
            return fail(c, BRE_ERR_INVALID_ARG, "%s: light %d has order %d, the scene has %d triangles", fn, (int)k,
                        c->lights[k].order, scene->n_triangles);
    if (!c->mats.empty() && c->tri_mat.size() != (size_t)scene->n_triangles)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: the material map (bre_set_materials) covers %lld triangles, the scene "
                    "has %d", fn, (long long)c->tri_mat.size(), scene->n_triangles);
    if (c->media.empty()) {
        if (c->has_interface)
            return fail(c, BRE_ERR_INVALID_ARG, "%s: a BRE_MATERIAL_INTERFACE triangle needs the context's media "
                        "(bre_set_media)", fn);
        return BRE_OK;
    }
    // two sources of media would be ambiguous
    if (scene->has_medium != BRE_MEDIUM_NONE)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: the context holds media (bre_set_media): the scene's has_medium must "
                    "be BRE_MEDIUM_NONE", fn);
    if (c->tri_med.size() != 2 * (size_t)scene->n_triangles)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: the media pairs (bre_set_media) cover %lld triangles, the scene has %d",
                    fn, (long long)(c->tri_med.size() / 2), scene->n_triangles);
    if (c->light_med.size() != c->lights.size())
        return fail(c, BRE_ERR_INVALID_ARG, "%s: the media (bre_set_media) name %lld delta lights, the context holds "
                    "%lld", fn, (long long)c->light_med.size(), (long long)c->lights.size());
    return BRE_OK;
}

// The context's media on the device: the table with its grids behind one another, the pairs and the lights'
// media.  Uploaded when bre_set_media changed them.
bre_status upload_media(bre_ctx *c) {
    if (!c->media_dirty) return BRE_OK;
    std::vector<DevMedium> table(c->media.size());
    std::vector<float> dens;
    std::vector<size_t> first(c->media.size(), 0);
    for (size_t k = 0; k < c->media.size(); ++k) {
        const bre_medium &m = c->media[k];
        DevMedium &d = table[k];
        d = DevMedium{};
        d.medium = m.type;
        for (int j = 0; j < 3; ++j) d.sigma_t[j] = m.sigma_a[j] + m.sigma_s[j];  // HomogeneousMedium ctor
        d.g = m.g;
        if (m.type != BRE_MEDIUM_GRID) continue;
        // GridDensityMedium ctor (grid.h:58-77): sigma_t = (sigma_a + sigma_s)[0]; invMaxDensity, std::max order
        const std::vector<float> &g = c->media_grid[k];
        float mx = 0;
        for (float v : g) mx = std::max(mx, v);
        for (int j = 0; j < 3; ++j) d.gn[j] = m.grid_n[j];
        d.grid_sigma_t = m.sigma_a[0] + m.sigma_s[0];
        d.grid_inv_max = 1 / mx;
        for (int j = 0; j < 16; ++j) d.w2m[j] = m.world_to_medium[j];
        first[k] = dens.size();
        dens.insert(dens.end(), g.begin(), g.end());
    }
    float *dd = nullptr;
    HIPCHK(c, c->md_dens.get(dens.size() + 1, &dd));
    for (size_t k = 0; k < table.size(); ++k)
        if (table[k].medium == BRE_MEDIUM_GRID) table[k].density = dd + first[k];
    const auto up = [&](DevMem &m, const void *src, size_t bytes) -> hipError_t {
        hipError_t e = m.ensure(bytes > 0 ? bytes : 4);
        if (e != hipSuccess || bytes == 0) return e;
        return hipMemcpyAsync(m.ptr, src, bytes, hipMemcpyHostToDevice, c->stream);
    };
    HIPCHK(c, up(c->md_dens, dens.data(), dens.size() * sizeof(float)));
    HIPCHK(c, up(c->md_table, table.data(), table.size() * sizeof(DevMedium)));
    HIPCHK(c, up(c->md_pairs, c->tri_med.data(), c->tri_med.size() * sizeof(int32_t)));
    HIPCHK(c, up(c->md_light, c->light_med.data(), c->light_med.size() * sizeof(int32_t)));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
    c->media_dirty = false;
    return BRE_OK;
}

// The byte ranges the geometry cache is keyed by, in the order sc_bytes keeps them: the scene's triangles,
// then the context's lights, materials and material map
struct KeyPart {
    const void *p;
    size_t bytes;
};
void geometry_key(const bre_ctx *c, const bre_scene *s, KeyPart part[4]) {
    part[0] = {scene_triangles(s), (size_t)s->n_triangles * sizeof(bre_triangle)};
    part[1] = {c->lights.data(), c->lights.size() * sizeof(bre_light)};
    part[2] = {c->mats.data(), c->mats.size() * sizeof(bre_material)};
    part[3] = {c->tri_mat.data(), c->tri_mat.size() * sizeof(int32_t)};
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

// DevScene (+ the density grid of a GridDensityMedium) into ph_scene on the context's stream.  The
// geometry (triangles, BVHAccel, lights, materials) is rebuilt and uploaded only when the triangles, the
// context's lights or its materials change.
bre_status upload_scene(bre_ctx *c, const bre_scene *scene) {
    float *dd = nullptr;
    if (scene->has_medium == BRE_MEDIUM_GRID) {
        const size_t n = (size_t)scene->grid_n[0] * scene->grid_n[1] * scene->grid_n[2];
        // uploaded only when the density values change (every pass of a render shares one grid)
        const unsigned char *src = reinterpret_cast<const unsigned char *>(scene->grid_density);
        const bool same = c->grid_dens.ptr && c->grid_bytes.size() == n * sizeof(float) &&
                          memcmp(c->grid_bytes.data(), src, n * sizeof(float)) == 0;
        if (!same) {
            HIPCHK(c, c->grid_dens.get(n, &dd));
            HIPCHK(c, hipMemcpyAsync(dd, scene->grid_density, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->grid_bytes.assign(src, src + n * sizeof(float));
        }
        dd = c->grid_dens.as<float>();
    }
    KeyPart part[4];
    geometry_key(c, scene, part);
    const uint64_t h = hash_geometry(scene, part);
    // the geometry is reused only when the hash AND the bytes match (a hash collision between two
    // scenes must not trace against the stale BVH, lights and materials)
    bool same = h == c->sc_hash;
    for (int k = 0; k < 4; ++k) same = same && c->sc_part[k] == part[k].bytes;
    size_t off = 0;
    for (int k = 0; same && k < 4; ++k) {
        same = part[k].bytes == 0 || memcmp(c->sc_bytes.data() + off, part[k].p, part[k].bytes) == 0;
        off += part[k].bytes;
    }
    if (!same) {
        HostScene hs;
        MaterialMap mm;
        mm.mats = c->mats.data();
        mm.n_mats = (int)c->mats.size();
        mm.tri_mat = c->tri_mat.data();
        prepare_geometry(scene, &hs, c->lights.data(), (int)c->lights.size(), mm);
        if (hs.depth > kSceneStack)
            return fail(c, BRE_ERR_INVALID_ARG, "scene BVH depth %d exceeds the %d-entry traversal stack (as in "
                        "BVHAccel::Intersect)", hs.depth, kSceneStack);
        const auto up = [&](DevMem &m, const void *src, size_t bytes) -> hipError_t {
            hipError_t e = m.ensure(bytes > 0 ? bytes : 4);
            if (e != hipSuccess || bytes == 0) return e;
            return hipMemcpyAsync(m.ptr, src, bytes, hipMemcpyHostToDevice, c->stream);
        };
        HIPCHK(c, up(c->sc_tris, hs.tris.data(), hs.tris.size() * sizeof(PTri)));
        HIPCHK(c, up(c->sc_nodes, hs.nodes.data(), hs.nodes.size() * sizeof(SceneNode)));
        HIPCHK(c, up(c->sc_prims, hs.prims.data(), hs.prims.size() * sizeof(int32_t)));
        HIPCHK(c, up(c->sc_light_tri, hs.light_tri.data(), hs.light_tri.size() * sizeof(int32_t)));
        HIPCHK(c, up(c->sc_light_func, hs.light_func.data(), hs.light_func.size() * sizeof(float)));
        HIPCHK(c, up(c->sc_light_cdf, hs.light_cdf.data(), hs.light_cdf.size() * sizeof(float)));
        HIPCHK(c, up(c->sc_dlights, hs.dlights.data(), hs.dlights.size() * sizeof(DLight)));
        HIPCHK(c, up(c->sc_mats, hs.mats.data(), hs.mats.size() * sizeof(bre_material)));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
        c->sc_head = hs.head;
        c->sc_head.t = c->sc_tris.as<PTri>();
        c->sc_head.nodes = c->sc_nodes.as<SceneNode>();
        c->sc_head.prims = c->sc_prims.as<int32_t>();
        c->sc_head.light_tri = c->sc_light_tri.as<int32_t>();
        c->sc_head.light_func = c->sc_light_func.as<float>();
        c->sc_head.light_cdf = c->sc_light_cdf.as<float>();
        c->sc_head.dlights = c->sc_dlights.as<DLight>();
        c->sc_head.mats = c->sc_mats.as<bre_material>();
        c->sc_hash = h;
        c->sc_bytes.clear();
        for (int k = 0; k < 4; ++k) {
            const unsigned char *b = static_cast<const unsigned char *>(part[k].p);
            if (part[k].bytes) c->sc_bytes.insert(c->sc_bytes.end(), b, b + part[k].bytes);
            c->sc_part[k] = part[k].bytes;
        }
    }
    DevScene ds;
    memcpy(&ds, &c->sc_head, sizeof(DevScene));  // padding bytes included: the record compares bytewise
    prepare_medium(scene, &ds, dd);
    if (!c->media.empty()) {
        BRE_TRY(upload_media(c));
        ds.media = c->md_table.as<DevMedium>();
        ds.tri_med = c->md_pairs.as<int32_t>();
        ds.light_med = c->md_light.as<int32_t>();
        ds.n_media = (int)c->media.size();
        ds.cam_med = c->cam_med;
    } else {
        ds.media = nullptr;
        ds.tri_med = ds.light_med = nullptr;
        ds.n_media = 0;
        ds.cam_med = -1;
    }
    // the scene record is copied only when it changes: in a render every pass uploads the same record,
    // and a copy queued behind another context's gather waits for that gather's blocks (round 5 trace:
    // a 1.6 KB upload took 110 ms in the two-context pipeline)
    if (!c->ph_scene.ptr || memcmp(&ds, &c->ph_scene_host, sizeof(DevScene)) != 0) {
        HIPCHK(c, c->ph_scene.ensure(sizeof(DevScene)));
        HIPCHK(c, hipMemcpyAsync(c->ph_scene.ptr, &ds, sizeof(DevScene), hipMemcpyHostToDevice, c->stream));
        // the host copies are read by the DMA before the call returns
        HIPCHK(c, hipStreamSynchronize(c->stream));
        memcpy(&c->ph_scene_host, &ds, sizeof(DevScene));
    }
    return BRE_OK;
}

struct FinalImage {
    float *dst;
    size_t n;
};
int keep_final_image(int32_t, const float *img, void *user) {
    FinalImage *f = static_cast<FinalImage *>(user);
    memcpy(f->dst, img, f->n * sizeof(float));
    return 0;
}

}  // namespace

namespace bre {

bre_status check_params(bre_ctx *c, const bre_render_params *rp) {
    if (!rp) return fail(c, BRE_ERR_INVALID_ARG, "bre_render: null params");
    if (rp->width < 1 || rp->height < 1 || rp->start_iteration < 0 ||
        rp->end_iteration < rp->start_iteration || rp->max_depth < 1 || rp->max_depth > BRE_MAX_DEPTH)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_render: bad parameters");
    return BRE_OK;
}

// photonbeam.cpp:564: write at the last iteration and whenever (iter + 1) % writeFrequency == 0,
// negative frequencies included (-k fires every k iterations); the reference's default
// 1 << 31 wraps to INT32_MIN and never fires, and 0 (a division by zero there) means never
bool image_due(int32_t it, int32_t end_iteration, int32_t write_frequency) {
    const bool periodic = write_frequency != 0 && write_frequency != INT32_MIN && (it + 1) % write_frequency == 0;
    return it + 1 == end_iteration || periodic;
}

}  // namespace bre

extern "C" {

bre_status bre_set_lights(bre_ctx *c, const bre_light *lights, int32_t n) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (n < 0 || n > BRE_MAX_LIGHTS)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_set_lights: light count must be in 0..%d", BRE_MAX_LIGHTS);
    if (n > 0 && !lights) return fail(c, BRE_ERR_INVALID_ARG, "bre_set_lights: null lights");
    for (int k = 0; k < n; ++k) {
        const bre_light &l = lights[k];
        if (l.type != BRE_LIGHT_POINT && l.type != BRE_LIGHT_SPOT)
            return fail(c, BRE_ERR_INVALID_ARG, "bre_set_lights: light %d has unknown type %d", k, l.type);
        if (l.order < 0) return fail(c, BRE_ERR_INVALID_ARG, "bre_set_lights: light %d has a negative order", k);
        bool finite = std::isfinite(l.cone_total_deg) && std::isfinite(l.cone_falloff_start_deg);
        for (int j = 0; j < 3; ++j) finite = finite && std::isfinite(l.I[j]);
        for (int j = 0; j < 16; ++j)
            finite = finite && std::isfinite(l.light_to_world[j]) && std::isfinite(l.world_to_light[j]);
        if (!finite) return fail(c, BRE_ERR_INVALID_ARG, "bre_set_lights: light %d has a non-finite field", k);
    }
    c->lights.assign(lights, lights + n);
    return BRE_OK;
}

bre_status bre_set_materials(bre_ctx *c, const bre_material *materials, int32_t n_materials,
                             const int32_t *triangle_material, int64_t n_triangles) {
    if (!c) return BRE_ERR_INVALID_ARG;
    const char *fn = "bre_set_materials";
    if (n_materials < 0 || n_materials > BRE_MAX_MATERIALS)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: material count must be in 0..%d", fn, BRE_MAX_MATERIALS);
    if (n_materials == 0) {
        c->mats.clear();
        c->tri_mat.clear();
        c->has_interface = false;
        return BRE_OK;
    }
    if (n_triangles < 0 || n_triangles > BRE_MAX_SCENE_TRIANGLES)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: the material map's triangle count must be in 0..%d", fn,
                    BRE_MAX_SCENE_TRIANGLES);
    if (!materials || (n_triangles > 0 && !triangle_material))
        return fail(c, BRE_ERR_INVALID_ARG, "%s: null material table or triangle_material map", fn);
    std::vector<bre_material> mats(materials, materials + n_materials);
    std::vector<char> is_interface((size_t)n_materials, 0);
    for (int k = 0; k < n_materials; ++k) {
        bre_material &m = mats[(size_t)k];
        if (m.type == BRE_MATERIAL_INTERFACE && !c->media.empty()) {
            // no BSDF: Kr, Kt and eta are ignored (kept as zeros, so that equal tables compare equal)
            m = bre_material{};
            m.type = BRE_MATERIAL_INTERFACE;
            is_interface[(size_t)k] = 1;
            continue;
        }
        // (an interface on a context without media is refused like an unknown type: bre_set_media comes first)
        if (m.type != BRE_MATERIAL_MIRROR && m.type != BRE_MATERIAL_GLASS)
            return fail(c, BRE_ERR_INVALID_ARG, "%s: material %d has unknown type %d%s", fn, k, m.type,
                        m.type == BRE_MATERIAL_INTERFACE ? " (BRE_MATERIAL_INTERFACE needs bre_set_media first)" : "");
        if (!std::isfinite(m.eta) || !(m.eta > 0))
            return fail(c, BRE_ERR_INVALID_ARG, "%s: material %d has eta %g (must be finite and > 0)", fn, k, m.eta);
        for (int j = 0; j < 3; ++j) {
            if (!std::isfinite(m.kr[j]) || !std::isfinite(m.kt[j]))
                return fail(c, BRE_ERR_INVALID_ARG, "%s: material %d has a non-finite Kr or Kt", fn, k);
            // Kr->Evaluate(*si).Clamp() (mirror.cpp:52, glass.cpp:54-55) bounds the value below by 0; the ABI
            // also bounds it above by 1 (a reflectance), which a physical scene file never exceeds
            m.kr[j] = m.kr[j] < 0.f ? 0.f : (m.kr[j] > 1.f ? 1.f : m.kr[j]);
            m.kt[j] = m.kt[j] < 0.f ? 0.f : (m.kt[j] > 1.f ? 1.f : m.kt[j]);
        }
    }
    for (int64_t i = 0; i < n_triangles; ++i)
        if (triangle_material[i] < -1 || triangle_material[i] >= n_materials)
            return fail(c, BRE_ERR_INVALID_ARG, "%s: triangle %lld has material index %d outside [-1, %d)", fn,
                        (long long)i, triangle_material[i], n_materials);
    c->mats.swap(mats);
    c->tri_mat.assign(triangle_material, triangle_material + n_triangles);
    c->has_interface = false;
    for (int64_t i = 0; i < n_triangles; ++i)
        if (triangle_material[i] >= 0 && is_interface[(size_t)triangle_material[i]]) c->has_interface = true;
    return BRE_OK;
}

bre_status bre_set_media(bre_ctx *c, const bre_medium *media, int32_t n_media, const int32_t *tri_inside,
                         const int32_t *tri_outside, int64_t n_triangles, int32_t camera_medium,
                         const int32_t *light_medium, int32_t n_lights) {
    if (!c) return BRE_ERR_INVALID_ARG;
    const char *fn = "bre_set_media";
    if (n_media < 0 || n_media > BRE_MAX_MEDIA)
        return fail(c, BRE_ERR_INVALID_ARG, "%s: medium count must be in 0..%d", fn, BRE_MAX_MEDIA);
    if (n_media == 0) {
        c->media.clear();
        c->media_grid.clear();
        c->tri_med.clear();
        c->light_med.clear();
        c->media_key.clear();
        c->cam_med = -1;
        c->media_dirty = true;
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
        float mx = 0;
        for (int64_t i = 0; i < nx * ny * nz; ++i) mx = std::max(mx, m.grid_density[i]);
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
    c->media.assign(media, media + n_media);
    c->media_grid.assign((size_t)n_media, std::vector<float>());
    for (int k = 0; k < n_media; ++k) {
        bre_medium &m = c->media[(size_t)k];
        m.reserved = 0;
        if (m.type == BRE_MEDIUM_GRID) {
            const size_t n = (size_t)m.grid_n[0] * m.grid_n[1] * m.grid_n[2];
            c->media_grid[(size_t)k].assign(m.grid_density, m.grid_density + n);
            m.grid_density = c->media_grid[(size_t)k].data();
        } else {
            m.grid_density = nullptr;
        }
        put(&m, offsetof(bre_medium, grid_density));
        put(c->media_grid[(size_t)k].data(), c->media_grid[(size_t)k].size() * sizeof(float));
    }
    c->tri_med.resize(2 * (size_t)n_triangles);
    for (int64_t i = 0; i < n_triangles; ++i) {
        c->tri_med[2 * (size_t)i] = tri_inside[i];
        c->tri_med[2 * (size_t)i + 1] = tri_outside[i];
    }
    c->light_med.assign(light_medium, light_medium + n_lights);
    c->cam_med = camera_medium;
    put(c->tri_med.data(), c->tri_med.size() * sizeof(int32_t));
    put(c->light_med.data(), c->light_med.size() * sizeof(int32_t));
    put(&camera_medium, sizeof(camera_medium));
    c->media_key.swap(key);
    c->media_dirty = true;
    return BRE_OK;
}

bre_status bre_trace_photons(bre_ctx *c, const bre_scene *scene, int64_t n_photons, int32_t iteration,
                             int32_t max_depth, float beam_radius, int64_t *n_beams) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (n_beams) *n_beams = 0;
    if (!scene) return fail(c, BRE_ERR_INVALID_ARG, "bre_trace_photons: null scene");
    if (n_photons < 0 || iteration < 0) return fail(c, BRE_ERR_INVALID_ARG, "bre_trace_photons: negative count");
    if (max_depth < 1 || max_depth > BRE_MAX_DEPTH)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_trace_photons: max_depth must be in [1, %d]", BRE_MAX_DEPTH);
    BRE_TRY(check_scene(c, scene, "bre_trace_photons"));
    BRE_TRY(check_medium(c, scene, "bre_trace_photons"));
    BRE_TRY(set_device(c));
    PassStream pass(c);
    // an earlier asynchronous gather's device errors are reported before this call changes anything
    BRE_TRY(check_flags(c));
    BRE_TRY(upload_scene(c, scene));
    const size_t N = (size_t)n_photons;
    int32_t *counts = nullptr;
    int64_t *offsets = nullptr;
    HIPCHK(c, c->ph_counts.get(N + 1, &counts));
    HIPCHK(c, c->ph_offsets.get(N + 1, &offsets));
    HIPCHK(c, c->ph_tmp.ensure(count_scan_temp_bytes(n_photons) + 16));
    const uint64_t seq0 = (uint64_t)iteration * (uint64_t)n_photons + 1;
    const DevScene *ds = c->ph_scene.as<DevScene>();
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    const int sdepth = c->sc_head.stack_depth;
    const bool media = !c->media.empty();
    // single-trace form (bre_photon.hip): `cap` beam slots per photon, scratch at most 2.5 GB (62 slots at
    // 1M photons: the re-trace of the photons with more beams than slots is the form's tail, 1.65 ms
    // with 16 slots vs 1.41 with 64 at C2, profiles/r4/run36); below 4 slots, or with option 116 = 0,
    // the two-trace form
    int cap = c->photon_single ? (int)std::min<int64_t>(64, ((int64_t)5 << 29) / (40 * std::max<int64_t>(n_photons, 1))) : 0;
    if (cap < 4) cap = 0;
    if (c->photon_single >= 2) cap = c->photon_single;  // tests: a forced slot count (overflow paths)
    BeamArrays &slots = c->ph_s, &in = c->in;
    if (cap > 0) {
        HIPCHK(c, slots.ensure(N * (size_t)cap));
        HIPCHK(c, launch_photons(ds, sdepth, n_photons, seq0, max_depth, beam_radius, counts, nullptr, slots.out(), 2, cap,
                                 media, c->stream));
    } else {
        HIPCHK(c, launch_photons(ds, sdepth, n_photons, seq0, max_depth, beam_radius, counts, nullptr, BeamOut{}, 0, 0,
                                 media, c->stream));
    }
    HIPCHK(c, launch_count_scan(c->ph_tmp.ptr, c->ph_tmp.cap, counts, offsets, n_photons, c->stream,
                                c->slot_passes != 0));
    int64_t total = 0;
    BRE_TRY(read_small(c, {{&total, offsets + n_photons, sizeof(total)}}));
    if (total > 0) {
        HIPCHK(c, in.ensure((size_t)total));
        if (cap > 0)
            HIPCHK(c, launch_photon_slots(n_photons, cap, counts, offsets, slots.view(), in.out(), c->stream));
        // every photon (two-trace form), or only those with more beams than slots
        HIPCHK(c, launch_photons(ds, sdepth, n_photons, seq0, max_depth, beam_radius, counts, offsets, in.out(), 1, cap,
                                 media, c->stream));
    }
    float photon_ms = 0.f;
    if (c->timing) {
        HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
        HIPCHK(c, hipEventSynchronize(c->ev[1]));
        HIPCHK(c, hipEventElapsedTime(&photon_ms, c->ev[0], c->ev[1]));
    }
    c->beams_kept = false;
    BRE_TRY(build(c, total, in.view()));
    c->beams_kept = true;
    c->stats.n_photons = n_photons;
    c->stats.photon_ms = photon_ms;
    if (n_beams) *n_beams = total;
    return check_flags(c);
}

bre_status bre_camera_pass(bre_ctx *c, const bre_scene *scene, int32_t width, int32_t height, int32_t iteration,
                           int32_t max_depth, int32_t render_surfaces, int32_t render_media, float *d_surface,
                           int64_t *n_segments) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (n_segments) *n_segments = 0;
    BRE_TRY(check_scene(c, scene, "bre_camera_pass"));
    if (width < 1 || height < 1 || (int64_t)width * height > (int64_t)INT32_MAX / BRE_MAX_DEPTH || iteration < 0)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_camera_pass: bad film size or iteration");
    if (max_depth < 1 || max_depth > BRE_MAX_DEPTH)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_camera_pass: max_depth must be in [1, %d]", BRE_MAX_DEPTH);
    BRE_TRY(check_medium(c, scene, "bre_camera_pass"));
    BRE_TRY(set_device(c));
    PassStream pass(c);
    BRE_TRY(check_flags(c));  // an earlier gather's device errors, before this pass changes anything
    // scene + camera/Halton tables (rebuilt when the scene or film changes)
    BRE_TRY(upload_scene(c, scene));
    if (c->cam_w != width || c->cam_h != height || memcmp(&c->cam_scene, scene, sizeof(bre_scene)) != 0) {
        DevCamera cam;
        std::vector<uint16_t> perms;
        prepare_camera(scene, width, height, &cam, &perms);
        HIPCHK(c, c->cam_dev.ensure(sizeof(DevCamera)));
        HIPCHK(c, c->cam_perms.ensure(perms.size() * sizeof(uint16_t)));
        HIPCHK(c, hipMemcpyAsync(c->cam_dev.ptr, &cam, sizeof(cam), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->cam_perms.ptr, perms.data(), perms.size() * sizeof(uint16_t),
                                 hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));  // host vectors go out of scope
        c->cam_w = width;
        c->cam_h = height;
        memcpy(&c->cam_scene, scene, sizeof(bre_scene));
    }
    const int64_t nslots = camera_slots(width, height);
    // the slot planes: a segment's plane is its ordinal along the path, which passes the depth only where the
    // path can cross an interface triangle; then BRE_OPT_SEGMENT_BUDGET more planes
    const bool media = !c->media.empty();
    const int planes = max_depth + (media && c->has_interface ? c->seg_budget : 0);
    if (nslots * planes > (int64_t)INT32_MAX)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_camera_pass: the film is too large for %d segment planes", planes);
    const size_t S = (size_t)(nslots * planes);
    int32_t *valid = nullptr, *depth = nullptr;
    int64_t *offs = nullptr;
    unsigned int *cam_flags = nullptr;
    HIPCHK(c, c->cs.ensure(S));
    HIPCHK(c, c->cs_valid.get(S, &valid));
    HIPCHK(c, c->cam_offs.get(S + 1, &offs));
    HIPCHK(c, c->cam_tmp.ensure(camera_scan_temp_bytes((int64_t)S) + 16));
    HIPCHK(c, c->cam_flags.get(1, &cam_flags));
    HIPCHK(c, fill_words(c, cam_flags, sizeof(unsigned int)));
    CamSlots cs{c->cs.out(), valid};
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
    HIPCHK(c, launch_camera(c->ph_scene.as<DevScene>(), c->sc_head.stack_depth, c->cam_dev.as<DevCamera>(),
                            c->cam_perms.as<uint16_t>(),
                            width, height, iteration, max_depth, render_surfaces, render_media, cs, d_surface,
                            cam_flags, c->shard_rank, c->shard_count,
                            c->shard_mode != 0 ? 0 : c->shard_block, c->film_classes, planes, media, c->stream));
    // exclusive scan of the slots' valid flags into cam_offs: total = offs[S-1] + valid[S-1]
    HIPCHK(c, launch_camera_scan(c->cam_tmp.ptr, c->cam_tmp.cap, cs, nslots, planes, offs, c->stream,
                                 c->slot_passes != 0));
    int64_t last_off = 0;
    int32_t last_valid = 0;
    unsigned int flags = 0;
    BRE_TRY(read_small(c, {{&last_off, offs + (S - 1), sizeof(int64_t)},
                           {&last_valid, valid + (S - 1), sizeof(int32_t)},
                           {&flags, cam_flags, sizeof(flags)}}));
    if (flags & kCamFlagBudget) {
        c->cam_nseg = 0;
        return fail(c, BRE_ERR_STATE, "bre_camera_pass: a camera path crossed more medium interfaces than "
                    "BRE_OPT_SEGMENT_BUDGET (%d) allows beyond maxdepth: no segments are kept", c->seg_budget);
    }
    const int64_t n = last_off + last_valid;
    const size_t N = (size_t)(n > 0 ? n : 1);
    HIPCHK(c, c->seg.ensure(N));
    HIPCHK(c, c->seg_depth.get(N, &depth));
    HIPCHK(c, launch_camera_compact(cs, nslots, planes, offs, c->seg.out(), depth, c->stream));
    float ms = 0.f;
    if (c->timing) {
        HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
        HIPCHK(c, hipEventSynchronize(c->ev[1]));
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    }
    c->cam_nseg = n;
    c->cam_npix = (int64_t)width * height;
    c->stats.n_camera_segments = n;
    c->stats.camera_ms = ms;
    if (n_segments) *n_segments = n;
    return check_flags(c);
}

bre_status bre_get_segments(bre_ctx *c, int64_t capacity, float *o, float *p, float *d, float *tmax, int32_t *pixel,
                            int32_t *depth, int64_t *n_segments) {
    if (!c) return BRE_ERR_INVALID_ARG;
    if (capacity < 0) return fail(c, BRE_ERR_INVALID_ARG, "bre_get_segments: negative capacity");
    if (n_segments) *n_segments = c->cam_nseg;
    const int64_t k = capacity < c->cam_nseg ? capacity : c->cam_nseg;
    if (k <= 0) return BRE_OK;
    if (!o || !p || !d || !tmax || !pixel || !depth)
        return fail(c, BRE_ERR_INVALID_ARG, "bre_get_segments: null array");
    BRE_TRY(set_device(c));
    const size_t K = (size_t)k;
    HIPCHK(c, c->seg.download(K, o, p, d, tmax, pixel, c->stream));
    HIPCHK(c, hipMemcpyAsync(depth, c->seg_depth.ptr, K * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    return check_flags(c);
}

bre_status bre_render_iteration(bre_ctx *c, const bre_scene *scene, const bre_render_params *rp, int32_t iteration,
                                float *d_ld) {
    if (!c) return BRE_ERR_INVALID_ARG;
    BRE_TRY(check_params(c, rp));
    if (!d_ld) return fail(c, BRE_ERR_INVALID_ARG, "bre_render_iteration: null Ld buffer");
    const float R = bre_beam_radius_at(rp->initial_radius, rp->alpha, iteration);
    // photonsperiteration <= 0 means the film's pixel count (photonbeam.h:37-39, the -1 default)
    const int64_t photons =
        rp->photons_per_iteration > 0 ? rp->photons_per_iteration : (int64_t)rp->width * rp->height;
    BRE_TRY(bre_trace_photons(c, scene, photons, iteration, rp->max_depth, R, nullptr));
    BRE_TRY(bre_camera_pass(c, scene, rp->width, rp->height, iteration, rp->max_depth, rp->render_surfaces,
                            rp->render_media, d_ld, nullptr));
    if (rp->render_media) return bre_gather_camera(c, R, d_ld);
    return BRE_OK;
}

bre_status bre_render_progressive(bre_ctx *c, const bre_scene *scene, const bre_render_params *rp,
                                  int32_t write_frequency, bre_image_fn on_image, void *user) {
    if (!c) return BRE_ERR_INVALID_ARG;
    bre_status st = check_params(c, rp);
    if (st != BRE_OK) return st;
    if (c->film_classes > 1) return fail(c, BRE_ERR_STATE, "bre_render*: BRE_OPT_FILM_CLASSES is for caller device films");
    BRE_TRY(set_device(c));
    const int64_t npix = (int64_t)rp->width * rp->height;
    float *ld = nullptr;
    HIPCHK(c, hipMalloc(&ld, (size_t)npix * 3 * sizeof(float)));
    if (hipMemsetAsync(ld, 0, (size_t)npix * 3 * sizeof(float), c->stream) != hipSuccess)
        st = fail(c, BRE_ERR_HIP, "bre_render: memset failed");
    std::vector<float> h, img;
    for (int it = rp->start_iteration; st == BRE_OK && it < rp->end_iteration; ++it) {
        st = bre_render_iteration(c, scene, rp, it, ld);
        if (st != BRE_OK) break;
        if (!image_due(it, rp->end_iteration, write_frequency) || !on_image) continue;
        h.resize((size_t)npix * 3);
        img.resize(h.size());
        if (hipMemcpyAsync(h.data(), ld, h.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) {
            st = fail(c, BRE_ERR_HIP, "bre_render: copy-back failed");
            break;
        }
        st = bre_resolve_image(npix, h.data(), it, img.data());  // L = Ld / (iter + 1), :578
        if (st == BRE_OK && on_image(it, img.data(), user) != 0)
            st = fail(c, BRE_ERR_STATE, "bre_render: image callback stopped the render after iteration %d", it);
    }
    const bre_status fst = check_flags(c);  // the last iteration's gather
    if (st == BRE_OK) st = fst;
    (void)hipFree(ld);
    return st;
}

bre_status bre_render(bre_ctx *c, const bre_scene *scene, const bre_render_params *rp, float *image) {
    if (!c) return BRE_ERR_INVALID_ARG;
    BRE_TRY(check_params(c, rp));
    if (c->film_classes > 1) return fail(c, BRE_ERR_STATE, "bre_render: BRE_OPT_FILM_CLASSES is for caller device films");
    if (!image) return fail(c, BRE_ERR_INVALID_ARG, "bre_render: null image");
    FinalImage f{image, (size_t)rp->width * rp->height * 3};
    if (rp->end_iteration == rp->start_iteration) {
        memset(image, 0, f.n * sizeof(float));
        return BRE_OK;
    }
    // only the last iteration's image is kept (write_frequency 0 = at the end only)
    return bre_render_progressive(c, scene, rp, 0, keep_final_image, &f);
}

}  // extern "C"
