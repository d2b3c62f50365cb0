/*
 * bre_pbrt.h — C ABI of libbre_host.so: the .pbrt scene-format front end and the film output of
 * the photon-beam integrator, over the GPU integrator of bre.h.
 *
 *   reference (pbrt-v3 fork)                                  this ABI
 *   --------------------------------------------------------  --------------------------------
 *   pbrtParseFile / pbrtParseString (src/core/parser.h,       bre_pbrt_parse_file /
 *     pbrtparse.y, api.cpp:765-1361)                            bre_pbrt_parse_string
 *   RenderOptions::MakeIntegrator "photonbeam"                bre_pbrt_get_render_params
 *     (api.cpp:1463-1471) -> CreatePhotonBeamIntegrator
 *     (photonbeam.cpp:589-611)
 *   pbrtWorldEnd -> integrator->Render(*scene)                bre_pbrt_render / bre_pbrt_render_devices
 *     (api.cpp:1361-1380, photonbeam.cpp:329-586)
 *   Film::SetImage + Film::WriteImage (film.cpp:132-210)      bre_film_finalize
 *   WriteImagePFM / ReadImagePFM (imageio.cpp:437-482)        bre_write_pfm / bre_read_pfm
 *
 * The accepted subset of the scene format is documented in host/pbrt_scene.h.  Problems in a
 * statement are reported pbrt-style (text in bre_pbrt_messages) and the statement is skipped;
 * a scene the GPU model cannot render fails the parse with BRE_ERR_INVALID_ARG.
 */
#ifndef BRE_PBRT_H
#define BRE_PBRT_H

#include <stdint.h>

#include "bre.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bre_pbrt bre_pbrt;

/* Parse a scene.  *out is always set (free it with bre_pbrt_free) so that the messages of a
   failed parse can be read; BRE_OK iff the scene is renderable. */
bre_status bre_pbrt_parse_file(const char *path, bre_pbrt **out);
bre_status bre_pbrt_parse_string(const char *text, bre_pbrt **out);
/* The same with flags.  BRE_PBRT_MEDIA: media bounded by surfaces are accepted instead of refused --
   MediumInterface on any shape or light, Material "" / "none" shapes as BRE_MATERIAL_INTERFACE triangles --
   and every named medium in use becomes an entry of the table bre_pbrt_get_media returns (equal media share
   one); the bre_scene then has no medium of its own.  An undefined medium name fails the parse, as in pbrt.
   BRE_PBRT_LIGHTS: LightSource "distant" and LightSource "point" become bre_lights (bre_pbrt_get_lights) and
   "bool twosided" "true" on an AreaLightSource "diffuse" makes BRE_EMIT_TWO_SIDED triangles.  A distant light is
   in vacuum whatever MediumInterface is current (its entry of light_medium is -1); a scene whose one medium fills
   all space cannot hold one: bound the medium with surfaces and add BRE_PBRT_MEDIA.
   BRE_PBRT_MATERIALS: Material "glass" with "uroughness" / "vroughness" (rough glass), "glass" as a direct
   statement, "uber", "translucent" and "substrate", direct or named, become bre_material_ex records of types 8 .. 11
   (bre_pbrt_get_materials_ex) with the defaults of pbrt's Create...Material functions.  Material "mix" ("string
   namedmaterial1", "string namedmaterial2", "rgb|float amount") becomes a record of type 12 behind its two children's
   entries, and "subsurface" / "kdsubsurface" the glass or rough glass of their dielectric boundary, with one warning
   (the integrator never reads the BSSRDF).  The flags combine.
   flags 0 is bre_pbrt_parse_file / _string, which keep refusing such scenes. */
#define BRE_PBRT_MEDIA 1
#define BRE_PBRT_LIGHTS 2
#define BRE_PBRT_MATERIALS 4
bre_status bre_pbrt_parse_file_ex(const char *path, int32_t flags, bre_pbrt **out);
bre_status bre_pbrt_parse_string_ex(const char *text, int32_t flags, bre_pbrt **out);
void bre_pbrt_free(bre_pbrt *p);
/* Error()/Warning() text, one message per line; counts may be NULL. */
const char *bre_pbrt_messages(const bre_pbrt *p, int32_t *n_errors, int32_t *n_warnings);
/* The scene for bre_trace_photons / bre_camera_pass / bre_render; grid_density and (for more than
   BRE_MAX_TRIANGLES triangles) triangles_ext point into the parsed scene and stay valid until
   bre_pbrt_free. */
bre_status bre_pbrt_get_scene(const bre_pbrt *p, bre_scene *out);
/* The scene's LightSource "spot" (with BRE_PBRT_LIGHTS also "point" and "distant") statements as bre_light (bre_scene.h), in declaration order, for
   bre_set_lights: at most `capacity` are written to `out`, *n (may be NULL) receives their number.
   bre_pbrt_render sets them on every context it makes. */
bre_status bre_pbrt_get_lights(const bre_pbrt *p, int32_t capacity, bre_light *out, int32_t *n);
/* The scene's mirror and glass materials (Material "mirror"; MakeNamedMaterial with "string type" "mirror"
   or "glass") as a bre_material table, and per scene triangle its index into it (-1: matte), for
   bre_set_materials.  At most mat_capacity table entries and tri_capacity map entries are written;
   *n_materials and *n_triangles (may be NULL) receive the counts (n_materials 0: a matte-only scene).
   bre_pbrt_render sets them on every context it makes. */
bre_status bre_pbrt_get_materials(const bre_pbrt *p, int32_t mat_capacity, bre_material *materials,
                                  int32_t *n_materials, int64_t tri_capacity, int32_t *triangle_material,
                                  int64_t *n_triangles);
/* The same table in its wide form (bre_material_ex, for bre_set_materials_ex): Material "plastic" and "metal"
   (direct or named; metal with explicit "rgb eta" and "rgb k") and Material "matte" with a "sigma" other than 0 are
   entries of it too.  bre_pbrt_get_materials is unchanged for the scenes it can express and returns BRE_ERR_STATE
   (with the counts written) for a scene that holds one of these. */
bre_status bre_pbrt_get_materials_ex(const bre_pbrt *p, int32_t mat_capacity, bre_material_ex *materials,
                                     int32_t *n_materials, int64_t tri_capacity, int32_t *triangle_material,
                                     int64_t *n_triangles);
/* The media of a scene parsed with BRE_PBRT_MEDIA, for bre_set_media: the table (grid_density points into the
   parsed scene and stays valid until bre_pbrt_free), per scene triangle its MediumInterface as indices into it
   (-1: vacuum), the camera's medium (the outside medium at WorldEnd) and each spot light's (the outside medium
   where it was declared).  At most the given capacities are written; the counts and *camera_medium may be NULL.
   n_media 0: a scene without media, or parsed without the flag.  bre_pbrt_render sets them on every context it
   makes, before the materials. */
bre_status bre_pbrt_get_media(const bre_pbrt *p, int32_t med_capacity, bre_medium *media, int32_t *n_media,
                              int64_t tri_capacity, int32_t *tri_inside, int32_t *tri_outside, int64_t *n_triangles,
                              int32_t *camera_medium, int32_t light_capacity, int32_t *light_medium, int32_t *n_lights);
/* A spot light as CreateSpotLight (src/lights/spot.cpp:104-124) builds it, by the code the parser uses:
   light_to_world = CTM * Translate(from) * Inverse(dirToZ), world_to_light the tracked inverse,
   cone_falloff_start_deg = coneangle - conedeltaangle.  I is "I" times "scale"; ctm is a row-major 4x4
   current transform or NULL for the identity, ctm_inv the inverse tracked with it or NULL for
   Inverse(ctm) as Transform(Matrix4x4) computes it; order as bre_light.order.  (A point light needs only
   Translate(from): fill its bre_light by hand.) */
bre_status bre_pbrt_make_spot_light(const float from[3], const float to[3], const float I[3], float coneangle,
                                    float conedeltaangle, const float *ctm, const float *ctm_inv, int32_t order,
                                    bre_light *out);
/* CreatePhotonBeamIntegrator's parameters for the film of the scene (quick != 0 is pbrt's
   --quick); *write_frequency (may be NULL) receives "imagewritefrequency" as given (default 1 << 31 =
   INT32_MIN, never periodic; bre_render_progressive applies the reference's (iter + 1) % k test). */
bre_status bre_pbrt_get_render_params(const bre_pbrt *p, int32_t quick, bre_render_params *out,
                                      int32_t *write_frequency);
/* Film "image" resolution, scale and output file name (NUL-terminated, truncated to cap). */
bre_status bre_pbrt_get_film(const bre_pbrt *p, int32_t *xres, int32_t *yres, float *scale, char *filename,
                             int32_t cap);
/* The whole render on GPU `device`: BRE_ERR_INVALID_ARG unless the scene's Integrator is
   "photonbeam".  Writes the film (PFM, to outfile when non-NULL, else the film's filename with a
   .pfm extension) at every write of the reference's schedule unless write_files is 0; the last
   film image (after Film::WriteImage's conversion, top row first) goes to image_rgb
   (float[3*xres*yres], may be NULL). */
bre_status bre_pbrt_render(const bre_pbrt *p, int32_t device, int32_t quick, const char *outfile,
                           int32_t write_files, float *image_rgb);
/* The same on the n_devices (1..8) GPUs of `devices`, one libbre context each (a repeated ordinal puts
   several contexts on one device): with more than one the render is split over them by
   bre_render_progressive_sharded (bre.h), with exactly one it is bre_pbrt_render on that device. */
bre_status bre_pbrt_render_devices(const bre_pbrt *p, const int32_t *devices, int32_t n_devices, int32_t quick,
                                   const char *outfile, int32_t write_files, float *image_rgb);
/* Film::SetImage(L) + Film::WriteImage's per-pixel conversion with the film's scale. */
bre_status bre_film_finalize(int64_t npix, const float *L_rgb, float scale, float *out_rgb);
/* PFM file IO (rows top-first in memory, bottom-first on disk, little endian). bre_read_pfm
   writes at most capacity floats; width/height are always returned when the header parses. */
bre_status bre_write_pfm(const char *path, const float *rgb, int32_t width, int32_t height);
bre_status bre_read_pfm(const char *path, float *rgb, int64_t capacity, int32_t *width, int32_t *height);

#ifdef __cplusplus
}
#endif
#endif /* BRE_PBRT_H */
