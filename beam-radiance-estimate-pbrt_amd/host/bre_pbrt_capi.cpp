// bre_pbrt_capi.cpp — the C ABI of include/bre_pbrt.h over pbrt_scene.h / photonbeam_gpu.h.
#include <cstring>
#include <string>

#include "../../include/bre_pbrt.h"
#include "photonbeam_gpu.h"

using namespace bre_host;

struct bre_pbrt {
    PbrtScene scene;
    bool ok = false;
};

static bre_status finish_parse(bre_pbrt *p, bool ok) {
    p->ok = ok;
    if (ok) p->scene.Bind();
    return ok ? BRE_OK : BRE_ERR_INVALID_ARG;
}

extern "C" {

static_assert(BRE_PBRT_MEDIA == kParseMedia && BRE_PBRT_LIGHTS == kParseLights && BRE_PBRT_MATERIALS == kParseMaterials,
              "the ABI's flags are the parser's");

bre_status bre_pbrt_parse_file_ex(const char *path, int32_t flags, bre_pbrt **out) {
    if (!out) return BRE_ERR_INVALID_ARG;
    *out = new bre_pbrt();
    if (!path || (flags & ~(BRE_PBRT_MEDIA | BRE_PBRT_LIGHTS | BRE_PBRT_MATERIALS))) return BRE_ERR_INVALID_ARG;
    return finish_parse(*out, ParsePbrtFile(path, &(*out)->scene, flags));
}

bre_status bre_pbrt_parse_string_ex(const char *text, int32_t flags, bre_pbrt **out) {
    if (!out) return BRE_ERR_INVALID_ARG;
    *out = new bre_pbrt();
    if (!text || (flags & ~(BRE_PBRT_MEDIA | BRE_PBRT_LIGHTS | BRE_PBRT_MATERIALS))) return BRE_ERR_INVALID_ARG;
    return finish_parse(*out, ParsePbrtString(text, &(*out)->scene, flags));
}

bre_status bre_pbrt_parse_file(const char *path, bre_pbrt **out) { return bre_pbrt_parse_file_ex(path, 0, out); }

bre_status bre_pbrt_parse_string(const char *text, bre_pbrt **out) { return bre_pbrt_parse_string_ex(text, 0, out); }

void bre_pbrt_free(bre_pbrt *p) { delete p; }

const char *bre_pbrt_messages(const bre_pbrt *p, int32_t *n_errors, int32_t *n_warnings) {
    if (!p) return "";
    if (n_errors) *n_errors = p->scene.errors;
    if (n_warnings) *n_warnings = p->scene.warnings;
    return p->scene.messages.c_str();
}

bre_status bre_pbrt_get_scene(const bre_pbrt *p, bre_scene *out) {
    if (!p || !out || !p->ok) return BRE_ERR_INVALID_ARG;
    *out = p->scene.scene;
    return BRE_OK;
}

bre_status bre_pbrt_get_lights(const bre_pbrt *p, int32_t capacity, bre_light *out, int32_t *n) {
    if (!p || !p->ok || capacity < 0) return BRE_ERR_INVALID_ARG;
    const int32_t have = (int32_t)p->scene.lights.size();
    if (n) *n = have;
    const int32_t k = capacity < have ? capacity : have;
    if (k > 0 && !out) return BRE_ERR_INVALID_ARG;
    for (int32_t i = 0; i < k; ++i) out[i] = p->scene.lights[(size_t)i];
    return BRE_OK;
}

bre_status bre_pbrt_get_materials(const bre_pbrt *p, int32_t mat_capacity, bre_material *materials,
                                  int32_t *n_materials, int64_t tri_capacity, int32_t *triangle_material,
                                  int64_t *n_triangles) {
    if (!p || !p->ok || mat_capacity < 0 || tri_capacity < 0) return BRE_ERR_INVALID_ARG;
    const int32_t nm = (int32_t)p->scene.materials.size();
    const int64_t nt = (int64_t)p->scene.triangleMaterial.size();
    if (n_materials) *n_materials = nm;
    if (n_triangles) *n_triangles = nt;
    const int32_t km = mat_capacity < nm ? mat_capacity : nm;
    const int64_t kt = tri_capacity < nt ? tri_capacity : nt;
    if ((km > 0 && !materials) || (kt > 0 && !triangle_material)) return BRE_ERR_INVALID_ARG;
    // a plastic, a metal or a matte with sigma does not fit the narrow record: bre_pbrt_get_materials_ex
    for (int32_t i = 0; i < nm; ++i)
        if (p->scene.materials[(size_t)i].type >= BRE_MATERIAL_MATTE) return BRE_ERR_STATE;
    for (int32_t i = 0; i < km; ++i) memcpy(&materials[i], &p->scene.materials[(size_t)i], sizeof(bre_material));
    for (int64_t i = 0; i < kt; ++i) triangle_material[i] = p->scene.triangleMaterial[(size_t)i];
    return BRE_OK;
}

bre_status bre_pbrt_get_materials_ex(const bre_pbrt *p, int32_t mat_capacity, bre_material_ex *materials,
                                     int32_t *n_materials, int64_t tri_capacity, int32_t *triangle_material,
                                     int64_t *n_triangles) {
    if (!p || !p->ok || mat_capacity < 0 || tri_capacity < 0) return BRE_ERR_INVALID_ARG;
    const int32_t nm = (int32_t)p->scene.materials.size();
    const int64_t nt = (int64_t)p->scene.triangleMaterial.size();
    if (n_materials) *n_materials = nm;
    if (n_triangles) *n_triangles = nt;
    const int32_t km = mat_capacity < nm ? mat_capacity : nm;
    const int64_t kt = tri_capacity < nt ? tri_capacity : nt;
    if ((km > 0 && !materials) || (kt > 0 && !triangle_material)) return BRE_ERR_INVALID_ARG;
    for (int32_t i = 0; i < km; ++i) materials[i] = p->scene.materials[(size_t)i];
    for (int64_t i = 0; i < kt; ++i) triangle_material[i] = p->scene.triangleMaterial[(size_t)i];
    return BRE_OK;
}

bre_status bre_pbrt_get_media(const bre_pbrt *p, int32_t med_capacity, bre_medium *media, int32_t *n_media,
                              int64_t tri_capacity, int32_t *tri_inside, int32_t *tri_outside, int64_t *n_triangles,
                              int32_t *camera_medium, int32_t light_capacity, int32_t *light_medium, int32_t *n_lights) {
    if (!p || !p->ok || med_capacity < 0 || tri_capacity < 0 || light_capacity < 0) return BRE_ERR_INVALID_ARG;
    const SceneMedia &sm = p->scene.media;
    const int32_t nm = (int32_t)sm.media.size(), nl = (int32_t)sm.lightMedium.size();
    const int64_t nt = (int64_t)sm.triInside.size();
    if (n_media) *n_media = nm;
    if (n_triangles) *n_triangles = nt;
    if (n_lights) *n_lights = nl;
    if (camera_medium) *camera_medium = sm.cameraMedium;
    const int32_t km = med_capacity < nm ? med_capacity : nm, kl = light_capacity < nl ? light_capacity : nl;
    const int64_t kt = tri_capacity < nt ? tri_capacity : nt;
    if ((km > 0 && !media) || (kt > 0 && (!tri_inside || !tri_outside)) || (kl > 0 && !light_medium))
        return BRE_ERR_INVALID_ARG;
    for (int32_t i = 0; i < km; ++i) media[i] = sm.media[(size_t)i];
    for (int64_t i = 0; i < kt; ++i) {
        tri_inside[i] = sm.triInside[(size_t)i];
        tri_outside[i] = sm.triOutside[(size_t)i];
    }
    for (int32_t i = 0; i < kl; ++i) light_medium[i] = sm.lightMedium[(size_t)i];
    return BRE_OK;
}

bre_status bre_pbrt_make_spot_light(const float from[3], const float to[3], const float I[3], float coneangle,
                                    float conedeltaangle, const float *ctm, const float *ctm_inv, int32_t order,
                                    bre_light *out) {
    if (!from || !to || !I || !out) return BRE_ERR_INVALID_ARG;
    Xform l2w = Xform::Identity();
    if (ctm) {
        float m[4][4];
        memcpy(m, ctm, sizeof(m));
        l2w = Xform::FromMatrix(m);
        if (ctm_inv) memcpy(l2w.mInv, ctm_inv, sizeof(l2w.mInv));  // the inverse the caller tracked
    }
    MakeSpotLight(l2w, from, to, I, coneangle, conedeltaangle, order, out);
    return BRE_OK;
}

static PhotonBeamParams params_of(const bre_pbrt *p, int32_t quick) {
    PhotonBeamParams::Lookup lk;
    const ParamSet &ps = p->scene.integratorParams;
    lk.findInt = [&](const char *n, int d) { return ps.FindOneInt(n, d); };
    lk.findFloat = [&](const char *n, float d) { return ps.FindOneFloat(n, d); };
    lk.findBool = [&](const char *n, bool d) { return ps.FindOneBool(n, d); };
    return PhotonBeamParams::FromLookup(lk, quick != 0, p->scene.film.xres * p->scene.film.yres);
}

bre_status bre_pbrt_get_render_params(const bre_pbrt *p, int32_t quick, bre_render_params *out,
                                      int32_t *write_frequency) {
    if (!p || !out || !p->ok) return BRE_ERR_INVALID_ARG;
    const PhotonBeamParams pp = params_of(p, quick);
    memset(out, 0, sizeof(*out));
    out->width = p->scene.film.xres;
    out->height = p->scene.film.yres;
    out->iterations = pp.nIterations;
    out->start_iteration = pp.startIteration;
    out->end_iteration = pp.endIteration;
    out->photons_per_iteration = pp.photonsPerIteration;
    out->max_depth = pp.maxDepth;
    out->render_surfaces = pp.renderSurfaces;
    out->render_media = pp.renderMedia;
    out->initial_radius = pp.initialBeamRadius;
    out->alpha = pp.alpha;
    if (write_frequency) *write_frequency = pp.writeFrequency;  // bre_render_progressive applies the reference's modulo
    return BRE_OK;
}

bre_status bre_pbrt_get_film(const bre_pbrt *p, int32_t *xres, int32_t *yres, float *scale, char *filename,
                             int32_t cap) {
    if (!p || !p->ok) return BRE_ERR_INVALID_ARG;
    if (xres) *xres = p->scene.film.xres;
    if (yres) *yres = p->scene.film.yres;
    if (scale) *scale = p->scene.film.scale;
    if (filename && cap > 0) {
        strncpy(filename, p->scene.film.filename.c_str(), (size_t)cap - 1);
        filename[cap - 1] = '\0';
    }
    return BRE_OK;
}

bre_status bre_pbrt_render(const bre_pbrt *p, int32_t device, int32_t quick, const char *outfile,
                           int32_t write_files, float *image_rgb) {
    return bre_pbrt_render_devices(p, &device, 1, quick, outfile, write_files, image_rgb);
}

bre_status bre_pbrt_render_devices(const bre_pbrt *p, const int32_t *devices, int32_t n_devices, int32_t quick,
                                   const char *outfile, int32_t write_files, float *image_rgb) {
    if (!p || !p->ok) return BRE_ERR_INVALID_ARG;
    if (!devices || n_devices < 1 || n_devices > 8) return BRE_ERR_INVALID_ARG;
    if (p->scene.integratorName != "photonbeam") return BRE_ERR_INVALID_ARG;
    FilmDesc film = p->scene.film;
    if (outfile) film.filename = outfile;
    PhotonBeamIntegrator integ(params_of(p, quick), film, std::vector<int>(devices, devices + n_devices));
    if (!integ.Context()) return BRE_ERR_NO_DEVICE;
    integ.writeFiles = write_files != 0;
    if (!integ.Render(p->scene.scene, p->scene.lights, p->scene.materials, p->scene.triangleMaterial, &p->scene.media))
        return BRE_ERR_STATE;
    if (image_rgb && !integ.Image().empty())
        memcpy(image_rgb, integ.Image().data(), integ.Image().size() * sizeof(float));
    return BRE_OK;
}

bre_status bre_film_finalize(int64_t npix, const float *L, float scale, float *out) {
    if (npix < 0 || (npix > 0 && (!L || !out))) return BRE_ERR_INVALID_ARG;
    FilmFinalize(L, npix, scale, out);
    return BRE_OK;
}

bre_status bre_write_pfm(const char *path, const float *rgb, int32_t w, int32_t h) {
    if (!path || !rgb || w <= 0 || h <= 0) return BRE_ERR_INVALID_ARG;
    return WritePFM(path, rgb, w, h, nullptr) ? BRE_OK : BRE_ERR_STATE;
}

bre_status bre_read_pfm(const char *path, float *rgb, int64_t capacity, int32_t *w, int32_t *h) {
    if (!path) return BRE_ERR_INVALID_ARG;
    std::vector<float> img;
    int W = 0, H = 0;
    if (!ReadPFM(path, &img, &W, &H, nullptr)) return BRE_ERR_STATE;
    if (w) *w = W;
    if (h) *h = H;
    if (rgb && capacity > 0)
        memcpy(rgb, img.data(), (size_t)std::min<int64_t>(capacity, (int64_t)img.size()) * sizeof(float));
    return BRE_OK;
}

}  // extern "C"
