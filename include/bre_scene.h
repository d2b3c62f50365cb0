/*
 * bre_scene.h — scene description for the on-device photon pass and camera pass.
 *
 * The gather (bre.h) consumes beams and camera segments; this header describes the scene that
 * produces them, so the photon pass (TracePhotonBeamRecursive + emission,
 * src/integrators/photonbeam.cpp:258-325, 383-421) and the camera pass
 * (photonbeam.cpp:456-555) can run on the GPU next to the gather.
 *
 * The scene model is the subset of pbrt-v3 the benchmark scenes of SURVEY.md §8d need, kept at
 * pbrt's own granularity so every random decision and every float matches the reference:
 *   - bre_triangle      one pbrt Triangle of a "trianglemesh" (src/shapes/triangle.cpp): its three
 *                       world-space vertices in the mesh's index order, hit by the watertight
 *                       Triangle::Intersect (:177-300), with the triangle's own geometric normal
 *                       normalize(cross(p0 - p2, p1 - p2)) and shading frame ss = normalize(p1 - p0)
 *                       (dpdu for pbrt's default (0,0), (1,0), (1,1) uvs, :276-294), and a
 *                       Lambertian reflectance (MatteMaterial with sigma 0, src/materials/matte.cpp;
 *                       black kd = no BxDF, so a photon hitting it is absorbed,
 *                       reflection.cpp:708-713).  `flip` = ReverseOrientation ^
 *                       TransformSwapsHandedness (the normal is negated, :296-297).
 *   - diffuse area lights: every triangle with `emit` set is its own DiffuseAreaLight, one-sided
 *                       (BRE_EMIT_ONE_SIDED) or "twosided" (BRE_EMIT_TWO_SIDED: both hemispheres emit, the
 *                       power doubles, L() is Lemit seen from either side) (src/lights/diffuse.cpp:64-66,
 *                       89-123; pbrtShape makes one light per shape of an
 *                       emitting mesh, api.cpp), in triangle order = scene.lights order.  The photon
 *                       pass picks one by power (ComputeLightPowerDistribution,
 *                       integrator.cpp:217-225); the camera pass uniformly (UniformSampleOneLight).
 *   - point and spot lights (bre_light below; PointLight, src/lights/point.cpp, and SpotLight,
 *                       src/lights/spot.cpp), set on the context with bre_set_lights and merged with
 *                       the area lights into scene.lights by their `order`.  The photon pass emits from
 *                       them with their Sample_Le, the camera pass lights surfaces with their Sample_Li
 *                       (no MIS, a shadow ray to the light's position); a scene lit only by them needs
 *                       no emitting triangle.
 *   - distant lights    (bre_light with BRE_LIGHT_DISTANT; DistantLight, src/lights/distant.cpp), in the same
 *                       list.  Its disk of emission and the far end of its shadow rays come from the bounding
 *                       sphere of the scene BVH's root box (Scene::WorldBound().BoundingSphere, as
 *                       DistantLight::Preprocess takes it).  The reference constructs it with an empty
 *                       MediumInterface: its photons start in vacuum and reach a medium only through an
 *                       interface triangle.  So with bre_set_media its light medium must be -1, and a scene
 *                       with a medium of its own (has_medium != BRE_MEDIUM_NONE, "every ray travels in it")
 *                       is refused while the context holds a distant light: use bre_set_media.  A photon's
 *                       leg through vacuum still leaves a beam, as in the reference (photonbeam.cpp:290-294).
 *   - mirror and glass (bre_material below; MirrorMaterial, src/materials/mirror.cpp, and GlassMaterial
 *                       with zero roughness, src/materials/glass.cpp), set on the context with
 *                       bre_set_materials as a table and a per-triangle index.  Both passes sample the one
 *                       specular lobe (SpecularReflection::Sample_f, FresnelSpecular::Sample_f;
 *                       reflection.cpp:136-143, 477-511): the photon pass in TransportMode::Importance,
 *                       the camera pass in Radiance (the eta^2 factor), with isect.Le added after a
 *                       specular bounce and no direct light on a specular vertex.  Without bre_set_media
 *                       the scene's one medium fills the glass too.
 *   - plastic, metal and rough matte (bre_material_ex below; PlasticMaterial, MetalMaterial and MatteMaterial
 *                       with "sigma"), set with bre_set_materials_ex as the same table in its wide form.  Both
 *                       passes go through the general BSDF (BSDF::f, Pdf and Sample_f, reflection.cpp:670-785)
 *                       over a Lambertian or Oren-Nayar lobe and a Trowbridge-Reitz microfacet lobe.
 *   - rough glass, uber, translucent and substrate (bre_material_ex types 8 .. 11; GlassMaterial with roughness,
 *                       UberMaterial, TranslucentMaterial, SubstrateMaterial), in the same table.  Their BSDFs hold
 *                       up to five lobes, reflecting and transmitting, specular and not: both passes sample them
 *                       with BSDF_ALL, the photon pass in TransportMode::Importance and the camera pass in Radiance,
 *                       and EstimateDirect evaluates them with BSDF_ALL & ~BSDF_SPECULAR on both sides of the
 *                       surface (src/core/integrator.cpp:112-113).
 *   - mix             (bre_material_ex type 12; MixMaterial, src/materials/mixmat.cpp), in the same table: two earlier
 *                       entries of it on one surface.  Its BSDF holds the first child's BxDFs, then the second's, each
 *                       a ScaledBxDF (reflection.cpp:97-110) under `amount` and max(1 - amount, 0), up to
 *                       BRE_MAX_BXDFS of them; a child may itself be a mix, BRE_MAX_MIX_DEPTH deep.  A mirror or a
 *                       smooth glass under a mix is one specular lobe among the others (SpecularReflection under
 *                       FresnelNoOp, FresnelSpecular).
 *   - media bounded by surfaces (bre_medium below; pbrt's MediumInterface): a context holds a table of
 *                       media, a per-triangle (inside, outside) pair, the camera's medium and each delta
 *                       light's (bre_set_media, bre.h).  Every ray carries its medium; a triangle whose
 *                       material is BRE_MATERIAL_INTERFACE has no BSDF and both walks pass through it.
 *   - otherwise an optional medium filling all of space (every ray -- camera, photon, spawned -- travels
 *                       in it) with a Henyey-Greenstein phase function (src/core/medium.cpp:194-213):
 *                       BRE_MEDIUM_HOMOGENEOUS = HomogeneousMedium (src/media/homogeneous.cpp:44-77),
 *                       BRE_MEDIUM_GRID = GridDensityMedium (src/media/grid.{h:50-100,cpp:46-120}):
 *                       trilinear density over an nx*ny*nz grid on the medium-space unit cube, delta
 *                       tracking (Sample) and ratio tracking with Russian roulette (Tr); both draw
 *                       from the path's sampler.  sigma_a + sigma_s must be spectrally uniform.
 *   - a perspective pinhole camera (src/cameras/perspective.cpp, lensradius 0).
 * The GPU passes and the oracle evaluate it with IEEE float, no FMA contraction (DESIGN.md
 * "Photon pass").
 */
#ifndef BRE_SCENE_H
#define BRE_SCENE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BRE_MAX_TRIANGLES 128               /* triangles held inline in bre_scene.triangles */
#define BRE_MAX_SCENE_TRIANGLES (1 << 24)  /* triangles through bre_scene.triangles_ext */
#define BRE_MAX_DEPTH 16 /* maxdepth accepted by the photon / camera passes */

#define BRE_MEDIUM_NONE 0
#define BRE_MEDIUM_HOMOGENEOUS 1
#define BRE_MEDIUM_GRID 2
#define BRE_MAX_GRID_CELLS (1 << 26) /* nx*ny*nz accepted for a GridDensityMedium */

#define BRE_EMIT_ONE_SIDED 1 /* DiffuseAreaLight, twoSided = false: emits on the normal's side */
#define BRE_EMIT_TWO_SIDED 2 /* "bool twosided" "true": emits on both sides (diffuse.cpp:64-66, 100-112) */

typedef struct bre_triangle {
    float p[3][3]; /* world-space vertices mesh->p[v[0..2]] (ObjectToWorld applied) */
    float kd[3];   /* Lambertian reflectance; all-zero = absorbing (no BxDF) */
    float Le[3];   /* DiffuseAreaLight "L" (Lemit) when emit != 0 */
    int32_t emit;  /* BRE_EMIT_ONE_SIDED / BRE_EMIT_TWO_SIDED: a diffuse area light; 0: none */
    int32_t flip;  /* 1: ReverseOrientation ^ TransformSwapsHandedness (normal negated) */
} bre_triangle;

typedef struct bre_scene {
    int32_t n_triangles;   /* 1 .. BRE_MAX_TRIANGLES inline, or 1 .. BRE_MAX_SCENE_TRIANGLES through
                              triangles_ext; at least one with emit != 0 unless the context holds
                              lights (bre_set_lights) */
    int32_t has_medium;    /* BRE_MEDIUM_NONE (vacuum) / _HOMOGENEOUS / _GRID, filling all space; must be
                              BRE_MEDIUM_NONE while the context holds media (bre_set_media) */
    float sigma_a[3];      /* medium sigma_a (already multiplied by "scale") */
    float sigma_s[3];      /* medium sigma_s */
    float g;               /* Henyey-Greenstein asymmetry */
    float cam_pos[3];      /* LookAt eye */
    float cam_look[3];     /* LookAt target */
    float cam_up[3];       /* LookAt up */
    float cam_fov_deg;     /* perspective "fov" (degrees, spans the shorter image axis) */
    bre_triangle triangles[BRE_MAX_TRIANGLES];
    /* GridDensityMedium only (has_medium == BRE_MEDIUM_GRID; MakeMedium "heterogeneous",
       api.cpp:547-593): */
    int32_t grid_n[3];          /* nx, ny, nz (each >= 1, product <= BRE_MAX_GRID_CELLS) */
    float world_to_medium[16];  /* WorldToMedium = Inverse(mediumToWorld * Translate(p0) *
                                   Scale(p1 - p0)), row-major 4x4 (grid.h:58) */
    const float *grid_density;  /* nx*ny*nz densities, index (z*ny + y)*nx + x (grid.h:84-88);
                                   caller-owned host memory, read during the call */
    /* Any number of triangles (BRE_MAX_SCENE_TRIANGLES): when non-NULL, the scene's triangles are
       triangles_ext[0 .. n_triangles) (caller-owned host memory, read during the call) and the
       inline array is unused.  Either way the passes intersect the scene through pbrt's BVHAccel
       (src/accelerators/bvh.cpp: SAH, 12 buckets, maxnodeprims 4 -- the "bvh" accelerator's
       defaults, CreateBVHAccelerator), built on the host over the triangles in scene order, so
       equal-distance hits resolve in the reference's order. */
    const bre_triangle *triangles_ext;
} bre_scene;

/* Delta lights: pbrt's PointLight (src/lights/point.cpp), SpotLight (src/lights/spot.cpp) and DistantLight
   (src/lights/distant.cpp).  They are not part of bre_scene (its layout is fixed): a context holds them
   (bre_set_lights, bre.h) and every pass or render that takes a bre_scene uses the scene's triangles plus the
   context's lights.
   A distant light's record holds what its constructor leaves: I = "L" * "scale", and in light_to_world[0..2] the
   world-space wLight = Normalize(LightToWorld(from - to)), the direction TOWARDS the light (finite, not zero).
   It reads nothing else: the rest of light_to_world, world_to_light and the two cone angles are reserved and must
   be 0, so a point or spot record relabelled as distant is refused.  Point and spot records are unchanged. */
#define BRE_LIGHT_POINT 1
#define BRE_LIGHT_SPOT 2
#define BRE_LIGHT_DISTANT 3
#define BRE_MAX_LIGHTS 1024 /* delta lights accepted by bre_set_lights */

typedef struct bre_light {
    int32_t type;               /* BRE_LIGHT_POINT / BRE_LIGHT_SPOT / BRE_LIGHT_DISTANT */
    float I[3];                 /* "I" (distant: "L"), already multiplied by "scale"; distant: >= 0 */
    float light_to_world[16];   /* LightToWorld, row-major 4x4 (a point light: Translate(from) * CTM);
                                   distant: [0..2] = wLight, see above */
    float world_to_light[16];   /* its inverse as the reference tracks it (Transform::mInv), row-major;
                                   SpotLight::Falloff goes through it */
    float cone_total_deg;       /* spot: "coneangle" (totalWidth, degrees) */
    float cone_falloff_start_deg; /* spot: "coneangle" - "conedeltaangle" (falloffStart, degrees) */
    int32_t order;              /* the number of scene triangles declared before this light: in
                                   scene.lights the light comes before the area lights of the triangles
                                   with index >= order; lights of equal order keep their array order */
} bre_light;

/* Perfectly specular materials: pbrt's MirrorMaterial (src/materials/mirror.cpp: one SpecularReflection
   with FresnelNoOp) and GlassMaterial with zero roughness (src/materials/glass.cpp: one FresnelSpecular
   between index 1 outside and `eta` inside).  Like the lights they are not part of bre_scene: a context
   holds a table of them and a per-triangle index into it (bre_set_materials, bre.h); a triangle mapped to
   -1 keeps its own matte kd.  `emit` is independent of the material, as in pbrt. */
#define BRE_MATERIAL_MIRROR 1
#define BRE_MATERIAL_GLASS 2
/* pbrt's Material "" / "none": GetMaterial() == nullptr, no BSDF at all.  Both walks pass through such a
   triangle (photonbeam.cpp:300-304, 515-517) and shadow rays step over it (VisibilityTester::Tr,
   Scene::IntersectTr); kr, kt and eta are ignored.  It is not a BSDF without a BxDF (a black mirror), which
   ends the path.  bre_set_materials accepts it only on a context that holds media (bre_set_media first). */
#define BRE_MATERIAL_INTERFACE 3
#define BRE_MAX_MATERIALS 1024 /* table entries accepted by bre_set_materials */

typedef struct bre_material {
    int32_t type; /* BRE_MATERIAL_MIRROR / BRE_MATERIAL_GLASS / BRE_MATERIAL_INTERFACE */
    float kr[3];  /* "Kr", clamped to [0, 1] (Spectrum::Clamp); black = no reflection lobe */
    float kt[3];  /* glass: "Kt", clamped to [0, 1]; ignored for a mirror */
    float eta;    /* glass: "eta" / "index", finite and > 0 (also checked for a mirror, which ignores it) */
} bre_material;   /* 32 bytes, no padding */

/* Glossy and rough materials: pbrt's PlasticMaterial (src/materials/plastic.cpp: a LambertianReflection plus a
   Trowbridge-Reitz MicrofacetReflection under FresnelDielectric(1.5, 1)), MetalMaterial (src/materials/metal.cpp:
   one anisotropic Trowbridge-Reitz MicrofacetReflection under FresnelConductor(1, eta, k)) and MatteMaterial with
   "sigma" (src/materials/matte.cpp: OrenNayar, or the Lambertian lobe at sigma 0).  They do not fit a bre_material:
   bre_material_ex is the wide record, a superset of it that holds pbrt's parameters (not derived values), set with
   bre_set_materials_ex (bre.h).  Its first 32 bytes are a bre_material. */
#define BRE_MATERIAL_MATTE 4   /* kd, sigma */
#define BRE_MATERIAL_PLASTIC 5 /* kd, ks, roughness, remap */
#define BRE_MATERIAL_METAL 6   /* ceta, ck, roughness / uroughness / vroughness, remap */
/* Type 7 is unassigned and refused as unknown.
   Transmissive and layered materials, through the BSDF of any number of lobes with BxDFType flags and a transport
   mode (BSDF::f, Pdf, Sample_f with their reflect / transmit split, reflection.cpp:670-785):
   - rough glass (GlassMaterial with "uroughness" or "vroughness" != 0, src/materials/glass.cpp:45-92): a
     MicrofacetReflection under FresnelDielectric(1, eta) and a MicrofacetTransmission between 1 and eta.  Both
     roughnesses 0 is BRE_MATERIAL_GLASS and refused here; with remap, one of them may be 0 (RoughnessToAlpha
     clamps at 1e-3).
   - uber (UberMaterial, src/materials/uber.cpp:45-101): SpecularTransmission(1 - opacity, 1, 1),
     LambertianReflection(op Kd), MicrofacetReflection(op Ks), SpecularReflection(op Kr), SpecularTransmission(op Kt,
     1, eta), each only where its colour is not black.  uroughness 0 = not given: `roughness`; vroughness 0 = not
     given: the u value (uber.cpp:72-79).  `opacity` shares the storage of `ceta`, which uber never reads.
   - translucent (TranslucentMaterial, src/materials/translucent.cpp:45-80): "reflect" in kr, "transmit" in kt;
     Lambertian reflection and transmission of Kd, microfacet reflection and transmission of Ks between 1 and 1.5.
   - substrate (SubstrateMaterial, src/materials/substrate.cpp:45-65): one FresnelBlend(Kd, Ks).
   Every field a type does not read must be 0 in a record of these four types. */
#define BRE_MATERIAL_ROUGH_GLASS 8  /* kr, kt, eta, uroughness, vroughness, remap */
#define BRE_MATERIAL_UBER 9         /* kd, ks, kr, kt, eta, roughness, uroughness, vroughness, remap, opacity */
#define BRE_MATERIAL_TRANSLUCENT 10 /* kd, ks, kr ("reflect"), kt ("transmit"), roughness, remap */
#define BRE_MATERIAL_SUBSTRATE 11   /* kd, ks, uroughness, vroughness, remap */
/* - mix (MixMaterial, src/materials/mixmat.cpp:46-64): the BxDFs of table entry mix_child[0] ("namedmaterial1"), each
     a ScaledBxDF under s1 = `amount`, then those of entry mix_child[1] ("namedmaterial2") under
     s2 = max(1 - s1, 0) per channel.  A ScaledBxDF is added even where its scale is black: it counts in
     NumComponents and takes its share of the samples.  Both children come earlier in the table (no cycles) and are
     not BRE_MATERIAL_INTERFACE (no BSDF to scale); a child may be a mix, at most BRE_MAX_MIX_DEPTH mixes deep, and the
     expanded BSDF holds at most BRE_MAX_BXDFS BxDFs (BSDF::MaxBxDFs, reflection.h:202; the reference aborts past it).
     `amount` shares the storage of `kd` and `mix_child` that of reserved[0..1], neither of which a mix reads; every
     other field is 0 in a mix record.  bre_set_materials (the narrow form) does not know it. */
#define BRE_MATERIAL_MIX 12         /* amount, mix_child */
#define BRE_MAX_MIX_DEPTH 4 /* a mix sits at most this many mixes deep (itself included) */
#define BRE_MAX_BXDFS 8     /* BxDFs of an expanded mix */

typedef struct bre_material_ex {
    int32_t type;     /* BRE_MATERIAL_MIRROR .. BRE_MATERIAL_METAL, BRE_MATERIAL_ROUGH_GLASS .. BRE_MATERIAL_MIX */
    float kr[3];      /* as in bre_material; translucent: "reflect" */
    float kt[3];      /* translucent: "transmit" */
    float eta;        /* mirror / glass / rough glass / uber: finite and > 0; ignored by types 4 .. 6 */
#if defined(__cplusplus) || (defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L)
    union {
        float kd[3];      /* matte, plastic, uber, translucent, substrate: "Kd", clamped to [0, 1] */
        float amount[3];  /* mix: "amount", clamped to [0, 1] (pbrt's default is 0.5) */
    };
#else
    float kd[3];      /* "Kd"; mix: "amount" */
#endif
    float ks[3];      /* plastic, uber, translucent, substrate: "Ks", clamped to [0, 1] */
#if defined(__cplusplus) || (defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L)
    union {
        float ceta[3];    /* metal: "eta" (the conductor's index per channel), finite and != 0 */
        float opacity[3]; /* uber: "opacity", clamped to [0, 1] (pbrt's default is 1, the record's is what it holds) */
    };
#else
    float ceta[3];    /* metal: "eta"; uber: "opacity" */
#endif
    float ck[3];      /* metal: "k" (its absorption per channel) */
    float roughness;  /* plastic, translucent: "roughness" (> 0); metal, uber: used where u / vroughness is 0 */
    float uroughness; /* metal, uber: "uroughness" (>= 0; 0 = not given); rough glass, substrate: "uroughness" */
    float vroughness; /* metal, uber: "vroughness" (likewise); rough glass, substrate: "vroughness" */
    float sigma;      /* matte: "sigma" in degrees (clamped to [0, 90]; 0 = Lambertian) */
    int32_t remap;    /* every type with a roughness: "remaproughness" (0 / 1): roughness -> alpha by RoughnessToAlpha */
#if defined(__cplusplus) || (defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L)
    union {
        int32_t reserved[3];  /* 0 (a mix: reserved[2] is 0) */
        int32_t mix_child[2]; /* mix: the table indices of "namedmaterial1" and "namedmaterial2", both below its own */
    };
#else
    int32_t reserved[3]; /* 0; mix: [0] and [1] are the table indices of its two children */
#endif
} bre_material_ex;    /* 112 bytes, no padding */
#ifdef __cplusplus
static_assert(sizeof(bre_material_ex) == 112, "bre_material_ex stays 112 bytes");
static_assert(offsetof(bre_material_ex, ceta) == 56 && offsetof(bre_material_ex, opacity) == 56 &&
              offsetof(bre_material_ex, ck) == 68 && offsetof(bre_material_ex, roughness) == 80 &&
              offsetof(bre_material_ex, remap) == 96 && offsetof(bre_material_ex, reserved) == 100,
              "bre_material_ex keeps every offset; opacity shares ceta's storage");
static_assert(offsetof(bre_material_ex, kd) == 32 && offsetof(bre_material_ex, amount) == 32,
              "amount shares kd's storage");
static_assert(offsetof(bre_material_ex, mix_child) == 100 && sizeof(((bre_material_ex *)0)->mix_child) == 8,
              "mix_child shares reserved[0..1]");
#endif

/* Media bounded by surfaces: pbrt's MediumInterface.  Like the lights and materials they are not part of
   bre_scene: a context holds a table of media, each triangle's (inside, outside) pair, the camera's medium
   and each delta light's (bre_set_media, bre.h).  The fields mean what the same-named bre_scene fields mean. */
#define BRE_MAX_MEDIA 64 /* table entries accepted by bre_set_media; their grids together hold at most
                            BRE_MAX_GRID_CELLS cells */

typedef struct bre_medium {
    int32_t type;               /* BRE_MEDIUM_HOMOGENEOUS / BRE_MEDIUM_GRID */
    float sigma_a[3];           /* finite, >= 0 */
    float sigma_s[3];           /* finite, >= 0; a grid medium's sigma_a + sigma_s is spectrally uniform */
    float g;                    /* Henyey-Greenstein asymmetry, |g| <= 1 */
    int32_t grid_n[3];          /* grid: nx, ny, nz (each >= 1) */
    float world_to_medium[16];  /* grid: WorldToMedium, row-major 4x4 */
    int32_t reserved;           /* 0: keeps the pointer aligned without compiler padding */
    const float *grid_density;  /* grid: nx*ny*nz densities with a positive maximum, copied at the call */
} bre_medium;                   /* 120 bytes, no padding */

/* PhotonBeamIntegrator parameters (CreatePhotonBeamIntegrator, photonbeam.cpp:589-611). */
typedef struct bre_render_params {
    int32_t width, height;          /* film resolution (pixelBounds = [0,W) x [0,H)) */
    int32_t iterations;             /* "iterations" (default 64) */
    int32_t start_iteration;        /* "startiteration" (default 0) */
    int32_t end_iteration;          /* "enditeration" (default = iterations) */
    int64_t photons_per_iteration;  /* "photonsperiteration"; <= 0: width * height (photonbeam.h:37-39) */
    int32_t max_depth;              /* "maxdepth" (default 5) */
    int32_t render_surfaces;        /* "rendersurfaces" (default 1) */
    int32_t render_media;           /* "rendermedia" (default 1) */
    float initial_radius;           /* "initialbeamradius" (default 1) */
    float alpha;                    /* "alpha" (default 0.5) */
} bre_render_params;

/* The benchmark scene of SURVEY.md §8d (C1/C2), scenes/cornell_world.pbrt: unit-cube Cornell box
   (white floor, ceiling and back wall, red left wall, green right wall, white front wall behind
   the camera), a 0.3 x 0.3 area light just below the ceiling facing down, each wall one
   "trianglemesh" of two triangles (v0 v1 v2)(v0 v2 v3), homogeneous fog sigma_a, sigma_s (grey),
   HG g, camera at (0.5, 0.5, 0.02) looking at (0.5, 0.5, 1) with a 60 degree field of view. */
void bre_scene_cornell(bre_scene *scene, float sigma_a, float sigma_s, float g);

/* SURVEY.md §8d C3/C5 smoke: the same Cornell box with a GridDensityMedium of sigma_a, sigma_s
   (grey) and HG g over the box's unit cube (world_to_medium = identity); `density` (n^3 floats,
   caller-owned, must outlive the scene's use) is filled with bre_smoke_density's seeded value
   noise. */
void bre_scene_cornell_smoke(bre_scene *scene, float sigma_a, float sigma_s, float g, int32_t n,
                             const float *density);
/* Seeded value-noise smoke density (n^3 floats, x fastest): 3 octaves of trilinear lattice noise
   from PCG32(seed), shaped by a soft sphere of radius 0.45 around the box centre, >= 0. */
void bre_smoke_density(int32_t n, uint64_t seed, float *density);

#ifdef __cplusplus
}
#endif

#endif /* BRE_SCENE_H */
