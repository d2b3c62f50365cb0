// pbrt_scene.h — the .pbrt scene-file subset that feeds the photon-beam integrator on the GPU.
//
// Reference surface mirrored (bwiberg/beam-radiance-estimate-pbrt, pbrt-v3 fork):
//   tokenizer / grammar              src/core/pbrtlex.ll, src/core/pbrtparse.y (numbers via atof,
//                                    then (Float); "integer" values converted from the double)
//   ParamSet FindOne* / ReportUnused src/core/paramset.{h,cpp}
//   graphics state, CTM, media       src/core/api.cpp:765-1005 (Identity .. AttributeEnd),
//                                    :955-982 (MakeNamedMedium, MediumInterface), :1086-1157
//                                    (Material, MakeNamedMaterial, AreaLightSource, Shape)
//   Transform / Inverse / LookAt     src/core/transform.{h,cpp} (m and mInv tracked together)
//   MakeMedium                       src/core/api.cpp:547-593 (defaults, "scale", grid data2Medium)
//   camera medium                    api.cpp:651-655 (CreateMediumInterface at WorldEnd, outside)
//   film / camera / integrator       api.cpp:898-953 (parameters kept for the render)
//
// What the subset accepts is what the GPU scene model (include/bre_scene.h) can render; anything
// else is reported with pbrt-style Error()/Warning() text and the offending statement skipped:
//   * Shape "trianglemesh" -> one bre_triangle per index triple (vertices through the CTM exactly
//     as TriangleMesh does, mesh->p[i] = ObjectToWorld(P[i]), shapes/triangle.cpp; flip =
//     ReverseOrientation ^ TransformSwapsHandedness); any number up to BRE_MAX_SCENE_TRIANGLES (more
//     than BRE_MAX_TRIANGLES go through bre_scene.triangles_ext).
//   * Material "matte" with "Kd" (rgb, default 0.5) and "sigma" (0: the triangle's own kd; otherwise Oren-Nayar, a
//     table entry); MakeNamedMaterial/NamedMaterial.
//   * Material "plastic" ("Kd", "Ks" default 0.25, "roughness" 0.1, "remaproughness") and "metal" (explicit
//     "rgb eta" and "rgb k"; "roughness" 0.01, "uroughness" / "vroughness", "remaproughness"), direct or named:
//     wide table entries (bre_material_ex).
//   * Material "mirror" ("Kr", default 0.9), and MakeNamedMaterial with "string type" "mirror" or "glass"
//     ("Kr", "Kt" default 1; "eta", else "index", default 1.5; "uroughness" / "vroughness" must be 0): a
//     bre_material_ex in PbrtScene::materials, referred to by the triangles declared under it
//     (PbrtScene::triangleMaterial).  "bumpmap" and texture-valued parameters are reported and the statement
//     falls back to matte.  The direct statement Material "glass" is reported as unsupported.
//   * With kParseMaterials: "glass" with "uroughness" / "vroughness" (rough glass) and as a direct statement,
//     "uber", "translucent" and "substrate", direct or named (see kParseMaterials below).
//   * AreaLightSource "diffuse" ("L" x "scale"; one-sided, with kParseLights also "bool twosided"): every
//     triangle of an emitting mesh is its own light, as pbrtShape makes one DiffuseAreaLight per shape (api.cpp).
//   * media: "homogeneous" or "heterogeneous" (GridDensityMedium).  By default the scene has ONE medium
//     filling all space, so every shape's inside/outside medium and the camera medium must be
//     that medium (or all empty = vacuum); with kParseMedia every named medium in use becomes a table
//     entry and every shape and light keeps its MediumInterface (PbrtScene::media).
//   * LightSource "spot" ("I" x "scale", "from", "to", "coneangle", "conedeltaangle"): a bre_light with
//     CreateSpotLight's transform, in PbrtScene::lights; its outside medium must be the scene's medium.
//     Every other LightSource is reported as unsupported, unless kParseLights is given: then "point" ("I" x
//     "scale", "from") and "distant" ("L" x "scale", "from", "to"; always in vacuum) are bre_lights too.
//   * Camera "perspective" ("fov", lensradius 0) whose CTM is Identity followed by one LookAt.
//   * Film "image" (xresolution, yresolution, filename, scale); Integrator "photonbeam".
//   * Sampler / PixelFilter / Accelerator are accepted and ignored: the photon-beam integrator
//     draws from its own AwesomeSampler over HaltonSampler (photonbeam.cpp:456-462) and sets the
//     film image directly (Film::SetImage), so neither the scene's sampler nor filter is used.
//   * Include "file" (relative to the including file), comments, AttributeBegin/End,
//     TransformBegin/End, Translate, Scale, Rotate, LookAt, Transform, ConcatTransform,
//     CoordinateSystem, CoordSysTransform, ReverseOrientation.
#pragma once

#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/bre_scene.h"

namespace bre_host {

// One "type name" [values] parameter (pbrtparse.y ParamListItem after InitParamSet).
struct ParamItem {
    std::string type;  // integer float point3 vector3 normal rgb xyz spectrum bool string texture point2 ...
    std::string name;
    std::vector<float> floats;  // numeric values, converted from the double atof gave (Float)
    std::vector<int> ints;      // "integer" values
    std::vector<std::string> strings;
    std::vector<bool> bools;
    mutable bool lookedUp = false;
};

// pbrt::ParamSet subset (paramset.h): typed lookups with defaults, plus ReportUnused.
class ParamSet {
  public:
    void Add(ParamItem it);
    int FindOneInt(const std::string &name, int d) const;
    float FindOneFloat(const std::string &name, float d) const;
    bool FindOneBool(const std::string &name, bool d) const;
    std::string FindOneString(const std::string &name, const std::string &d) const;
    bool FindOnePoint3f(const std::string &name, float out[3]) const;
    // rgb / color only (RGBSpectrum::FromRGB copies); xyz is converted with XYZToRGB
    bool FindOneSpectrum(const std::string &name, float out[3]) const;
    const std::vector<float> *FindFloats(const std::string &name) const;
    const std::vector<int> *FindInts(const std::string &name) const;
    const std::vector<float> *FindPoint3fs(const std::string &name) const;
    bool Has(const std::string &name) const { return Find(name) != nullptr; }
    // names never looked up, "type name" each (paramset.cpp ReportUnused warns on them)
    std::vector<std::string> Unused() const;
    const std::vector<ParamItem> &Items() const { return items_; }

  private:
    const ParamItem *Find(const std::string &name) const;
    const ParamItem *FindTyped(const std::string &name, std::initializer_list<const char *> types) const;
    std::vector<ParamItem> items_;
};

// 4x4 matrix + tracked inverse, float arithmetic as pbrt's Transform (transform.{h,cpp}).
struct Xform {
    float m[4][4];
    float mInv[4][4];
    static Xform Identity();
    static Xform FromMatrix(const float rowMajor[4][4]);  // Transform(Matrix4x4): mInv = Inverse(m)
    static Xform Translate(float x, float y, float z);
    static Xform Scale(float x, float y, float z);
    static Xform Rotate(float thetaDeg, float ax, float ay, float az);
    static Xform LookAt(const float pos[3], const float look[3], const float up[3], bool *ok);
    Xform operator*(const Xform &t) const;
    Xform Inverse() const;  // pbrt Inverse(Transform): swaps m and mInv
    void ApplyPoint(const float p[3], float out[3]) const;
    bool IsIdentity() const;
};
// pbrt Matrix4x4 Inverse (Gauss-Jordan, full pivoting, transform.cpp:82-136); false if singular.
bool MatrixInverse(const float m[4][4], float out[4][4]);

struct FilmDesc {
    int xres = 1280, yres = 720;         // Film "image" defaults (film.cpp CreateFilm)
    std::string filename = "pbrt.pfm";   // "pbrt.exr" in the reference; this build writes PFM only
    float scale = 1.f;
};

// The media of a scene parsed with kParseMedia (bre_set_media's arguments): the table of the named media in
// use (equal media share an entry), per scene triangle its MediumInterface as indices into it (-1: vacuum),
// the camera's medium and each spot light's.  All empty / -1 otherwise.
constexpr int kParseMedia = 1;  // BRE_PBRT_MEDIA (include/bre_pbrt.h)
// LightSource "distant" (CreateDistantLight, distant.cpp:94-102) and "point" (CreatePointLight, point.cpp:80-88)
// become bre_lights and "bool twosided" "true" on an AreaLightSource "diffuse" gives BRE_EMIT_TWO_SIDED triangles,
// instead of the three refusals of the default parse
constexpr int kParseLights = 2;  // BRE_PBRT_LIGHTS
// kParseMaterials: Material "glass" with a roughness (rough glass), "glass" as a direct statement, "uber",
// "translucent" and "substrate" become bre_material_ex records of types 8 .. 11 (2 for a smooth glass), direct or
// named, with the defaults of the reference's Create...Material functions; without it the parse reports them as
// before.  Texture-valued parameters and "bumpmap" are reported and the statement falls back to matte, as for the
// other materials.  Material "mix" (api.cpp:430-446) becomes a record of type 12 after the entries of its two named
// materials (an undeclared one is a matte of the statement's own parameters; a table the library refuses is reported in
// its words and the statement falls back to matte); "subsurface" and "kdsubsurface" become the glass or rough glass of
// their dielectric boundary (Kr = Kt = 1, eta 1.33) with a warning: photonbeam.cpp never reads the BSSRDF.
constexpr int kParseMaterials = 4;  // BRE_PBRT_MATERIALS
struct SceneMedia {
    std::vector<bre_medium> media;             // grid_density points into `density`
    std::vector<std::vector<float>> density;   // per table entry: a heterogeneous medium's data
    std::vector<int32_t> triInside, triOutside, lightMedium;
    int32_t cameraMedium = -1;
    void Bind() {
        for (size_t k = 0; k < media.size(); ++k) media[k].grid_density = density[k].empty() ? nullptr : density[k].data();
    }
};

// Everything the render needs from one .pbrt file.
struct PbrtScene {
    bre_scene scene;                  // grid_density / triangles_ext point into the vectors below
    std::vector<float> density;       // heterogeneous medium data (nx*ny*nz)
    std::vector<bre_triangle> triangles;  // the triangles when there are more than BRE_MAX_TRIANGLES
    // Re-point scene.grid_density / scene.triangles_ext at this object's vectors (after a copy).
    void Bind();
    std::vector<bre_light> lights;    // LightSource "spot" statements, in declaration order (bre_set_lights)
    // Material "mirror" and named "mirror" / "glass" materials in use (bre_set_materials): the table, and per
    // scene triangle its index into it (-1: matte); both empty for a matte-only scene
    // (wide records: plastic, metal and matte with "sigma" are entries too, bre_set_materials_ex)
    std::vector<bre_material_ex> materials;
    std::vector<int32_t> triangleMaterial;
    SceneMedia media;                 // kParseMedia: the scene's media; scene.has_medium is then BRE_MEDIUM_NONE
    FilmDesc film;
    std::string integratorName;       // "photonbeam" expected
    ParamSet integratorParams;        // CreatePhotonBeamIntegrator's ParamSet
    std::string cameraName;
    bool haveCamera = false;
    int errors = 0, warnings = 0;
    std::string messages;             // Error()/Warning() text, one message per line
};

// CreateSpotLight (src/lights/spot.cpp:104-124): light2world = l2w * Translate(from) * Inverse(dirToZ) with
// dirToZ from CoordinateSystem(Normalize(to - from)), world_to_light the tracked inverse of the product;
// falloffStart = coneangle - conedelta.  I is "I" * "scale"; order = triangles declared before the light.
void MakeSpotLight(const Xform &l2w, const float from[3], const float to[3], const float I[3], float coneangle,
                   float conedelta, int order, bre_light *out);

// Parse a .pbrt file / string (pbrtParseFile / pbrtParseString).  Returns false only on a fatal
// problem (unreadable file, syntax error, no renderable scene); per-statement problems are
// recorded as errors and the statement skipped, as pbrt does.
// `flags`: 0, or kParseMedia: media bounded by surfaces are accepted (MediumInterface on any shape or light,
// Material "" / "none" shapes as interface triangles) and arrive as PbrtScene::media instead of the one
// medium of bre_scene.
bool ParsePbrtFile(const std::string &path, PbrtScene *out, int flags = 0);
bool ParsePbrtString(const std::string &text, PbrtScene *out, int flags = 0);

// Film::SetImage(L) + Film::WriteImage (film.cpp:132-140, 168-210) for the photon-beam
// integrator's image: per pixel RGB -> XYZ (RGBSpectrum::ToXYZ), filterWeightSum = 1, no splats,
// XYZ -> RGB, max(0, .) after the 1/weight multiply, + splatScale * 0, * scale.
void FilmFinalize(const float *L_rgb, int64_t npix, float scale, float *out_rgb);
// WriteImagePFM / ReadImagePFM (imageio.cpp:437-482): "PF", width height, -1 (little endian),
// rows bottom to top.  rgb is row-major from the top row.
bool WritePFM(const std::string &filename, const float *rgb, int width, int height, std::string *err);
bool ReadPFM(const std::string &filename, std::vector<float> *rgb, int *width, int *height, std::string *err);

}  // namespace bre_host
