// bre_views.h — the pointer groups the host side passes between the C ABI and the kernel launchers:
// camera segments, beams and a gather's outputs.  Plain pointers only (no HIP include): a view owns
// nothing, and the launchers unpack it at the kernel launch (no kernel takes a view).
#pragma once

#include <stdint.h>

namespace bre {

// Camera segments: o, p and d hold 3 floats per segment, t (tmax) 1, pix the pixel index (may be null)
struct SegView {
    const float *o, *p, *d, *t;
    const int32_t *pix;
    // the segments from `off` on; a null pix stays null
    SegView slice(int64_t off) const { return {o + 3 * off, p + 3 * off, d + 3 * off, t + off, pix ? pix + off : nullptr}; }
};
struct SegOut {
    float *o, *p, *d, *t;
    int32_t *pix;
    operator SegView() const { return {o, p, d, t, pix}; }
};

// Beams as the ABI passes them: start, end and power hold 3 floats per beam, radius 1
struct BeamView {
    const float *start, *end, *radius, *power;
};
struct BeamOut {
    float *start, *end, *radius, *power;
    operator BeamView() const { return {start, end, radius, power}; }
};

// A gather's outputs, each may be null: the film (3 floats per pixel), the per-segment sums (3 per
// segment) and the per-segment candidate / contribution counts (2 per segment)
struct GatherOut {
    float *accum, *seg_rgb;
    int32_t *seg_counts;
    // the per-segment outputs from segment `off` on (nulls stay null); the film is the same
    GatherOut slice(int64_t off) const {
        return {accum, seg_rgb ? seg_rgb + 3 * off : nullptr, seg_counts ? seg_counts + 2 * off : nullptr};
    }
};

}  // namespace bre
