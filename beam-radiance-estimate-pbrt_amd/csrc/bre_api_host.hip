// bre_api_host.hip — the entry points of the C ABI that take no context and make no HIP call: the
// built-in scenes, the smoke density, the radius schedule, the image resolve and the packet-shard
// count.  Built with the library's flags: the float helpers are bit-pinned against the oracle.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/bre.h"
#include "bre_trace.h"

extern "C" {

void bre_scene_cornell(bre_scene *s, float sigma_a, float sigma_s, float g) {
    if (!s) return;
    memset(s, 0, sizeof(*s));
    // scenes/cornell_world.pbrt: one "trianglemesh" per wall, indices [0 1 2 0 2 3]
    struct M {
        float v[4][3], kd[3];
        int emit;
    };
    const float W = 0.73f, R0 = 0.63f, R1 = 0.065f, R2 = 0.05f, G0 = 0.14f, G1 = 0.45f, G2 = 0.091f;
    const M ms[7] = {
        {{{0, 0, 0}, {0, 0, 1}, {1, 0, 1}, {1, 0, 0}}, {W, W, W}, 0},          // floor, normal +y
        {{{0, 1, 0}, {1, 1, 0}, {1, 1, 1}, {0, 1, 1}}, {W, W, W}, 0},          // ceiling, normal -y
        {{{0, 0, 1}, {0, 1, 1}, {1, 1, 1}, {1, 0, 1}}, {W, W, W}, 0},          // back wall, normal -z
        {{{0, 0, 0}, {1, 0, 0}, {1, 1, 0}, {0, 1, 0}}, {W, W, W}, 0},          // front wall (behind camera), +z
        {{{0, 0, 0}, {0, 1, 0}, {0, 1, 1}, {0, 0, 1}}, {R0, R1, R2}, 0},       // left wall (red), +x
        {{{1, 0, 0}, {1, 0, 1}, {1, 1, 1}, {1, 1, 0}}, {G0, G1, G2}, 0},       // right wall (green), -x
        {{{0.35f, 0.999f, 0.35f}, {0.65f, 0.999f, 0.35f}, {0.65f, 0.999f, 0.65f}, {0.35f, 0.999f, 0.65f}},
         {0, 0, 0}, 1},                                                         // light, normal -y
    };
    const float Le[3] = {17.f, 12.f, 4.f};
    const int idx[6] = {0, 1, 2, 0, 2, 3};
    s->n_triangles = 14;
    for (int m = 0; m < 7; ++m)
        for (int t = 0; t < 2; ++t) {
            bre_triangle &T = s->triangles[2 * m + t];
            for (int v = 0; v < 3; ++v) memcpy(T.p[v], ms[m].v[idx[3 * t + v]], 12);
            memcpy(T.kd, ms[m].kd, 12);
            T.emit = ms[m].emit;
            if (T.emit) memcpy(T.Le, Le, 12);
        }
    s->has_medium = 1;
    for (int k = 0; k < 3; ++k) {
        s->sigma_a[k] = sigma_a;
        s->sigma_s[k] = sigma_s;
    }
    s->g = g;
    const float pos[3] = {0.5f, 0.5f, 0.02f}, look[3] = {0.5f, 0.5f, 1.f}, up[3] = {0, 1, 0};
    memcpy(s->cam_pos, pos, 12);
    memcpy(s->cam_look, look, 12);
    memcpy(s->cam_up, up, 12);
    s->cam_fov_deg = 60.f;
}

void bre_scene_cornell_smoke(bre_scene *s, float sigma_a, float sigma_s, float g, int32_t n, const float *density) {
    if (!s) return;
    bre_scene_cornell(s, sigma_a, sigma_s, g);
    s->has_medium = BRE_MEDIUM_GRID;
    s->grid_n[0] = s->grid_n[1] = s->grid_n[2] = n;
    memset(s->world_to_medium, 0, sizeof(s->world_to_medium));
    for (int k = 0; k < 4; ++k) s->world_to_medium[5 * k] = 1.f;  // the grid spans the box's unit cube
    s->grid_density = density;
}

void bre_smoke_density(int32_t n, uint64_t seed, float *density) {
    if (!density || n < 1) return;
    // 3 octaves of trilinear value noise on lattices of 5, 9, 17 points per axis, values from
    // PCG32 sequence `seed` (rng.h:78-85) in lattice order
    bre::Pcg r;
    bre::pcg_seed(r, seed);
    std::vector<float> lat[3];
    int m[3];
    for (int k = 0; k < 3; ++k) {
        m[k] = (4 << k) + 1;
        lat[k].resize((size_t)m[k] * m[k] * m[k]);
        for (float &v : lat[k]) v = bre::pcg_float(r);
    }
    for (int z = 0; z < n; ++z)
        for (int y = 0; y < n; ++y)
            for (int x = 0; x < n; ++x) {
                const float p[3] = {(x + 0.5f) / n, (y + 0.5f) / n, (z + 0.5f) / n};
                float v = 0.f, amp = 0.5f;
                for (int k = 0; k < 3; ++k, amp *= 0.5f) {
                    const int L = m[k] - 1;
                    int i[3];
                    float f[3];
                    for (int a = 0; a < 3; ++a) {
                        const float q = p[a] * L;
                        i[a] = std::min((int)q, L - 1);
                        f[a] = q - (float)i[a];
                    }
                    float acc = 0.f;
                    for (int c = 0; c < 8; ++c) {
                        const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
                        const float w = (dx ? f[0] : 1 - f[0]) * (dy ? f[1] : 1 - f[1]) * (dz ? f[2] : 1 - f[2]);
                        acc += w * lat[k][((size_t)(i[2] + dz) * m[k] + (i[1] + dy)) * m[k] + (i[0] + dx)];
                    }
                    v += amp * acc;
                }
                const float dx = p[0] - 0.5f, dy = p[1] - 0.45f, dz = p[2] - 0.55f;
                const float rr = std::sqrt(dx * dx + dy * dy + dz * dz);
                const float shape = std::min(1.f, std::max(0.f, (0.45f - rr) / 0.2f));
                density[((size_t)z * n + y) * n + x] = std::max(0.f, 2.f * v - 0.4f) * shape;
            }
}

int64_t bre_shard_segments(int64_t n_segments, int32_t rank, int32_t count, int32_t chunk) {
    if (n_segments <= 0) return 0;
    if (count <= 1) return n_segments;
    if (rank < 0 || rank >= count || chunk < 1) return 0;
    const int64_t npk = (n_segments + 63) / 64, K = chunk;
    const int64_t nch = (npk + K - 1) / K;                              // chunks of K packets
    const int64_t q = rank < nch ? (nch - 1 - rank) / count + 1 : 0;    // chunks c = rank (mod count)
    const bool last = (nch - 1) % count == rank;                        // owns the only partial chunk
    const int64_t packets = q * K - (last ? nch * K - npk : 0);
    return packets * 64 - (last ? npk * 64 - n_segments : 0);
}

float bre_beam_radius_at(float initial_radius, float alpha, int iteration) {
    float r = initial_radius;
    for (int i = 0; i < iteration; ++i) r = r * (float(i + alpha) / float(i + 1));
    return r;
}

bre_status bre_resolve_image(int64_t npix, const float *ld, int iteration, float *out) {
    if (npix < 0 || (npix > 0 && (!ld || !out)) || iteration < 0) return BRE_ERR_INVALID_ARG;
    // Spectrum L = pixel.Ld / (iter + 1): operator/(Float) divides each channel (spectrum.h:180-186)
    const float div = (float)(iteration + 1);
    for (int64_t i = 0; i < 3 * npix; ++i) out[i] = ld[i] / div;
    return BRE_OK;
}

}  // extern "C"
