// views_check.cpp — csrc/bre_views.h alone, on the host (tests/test_views.py builds this with
// -fsanitize=address,undefined and runs it): the slices a gather's launch loop takes and the
// mutable -> const conversions.  Every array has exactly the gather's size, so a slice that points or
// strides wrong reads the wrong value or outside the array.
#include <cstdio>
#include <vector>

#include "bre_views.h"

using namespace bre;

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED %s (line %d)\n", #cond, __LINE__);     \
            ++failures;                                                \
        }                                                              \
    } while (0)

int main() {
    const int64_t n = 130;  // two packets of 64 and a partial one
    std::vector<float> o(3 * n), p(3 * n), d(3 * n), t(n), rgb(3 * n), film(3);
    std::vector<int32_t> pix(n), counts(2 * n);
    for (int64_t i = 0; i < 3 * n; ++i) {
        o[i] = 1000.f + i;
        p[i] = 2000.f + i;
        d[i] = 3000.f + i;
        rgb[i] = 4000.f + i;
    }
    for (int64_t i = 0; i < n; ++i) {
        t[i] = 5000.f + i;
        pix[i] = 6000 + (int32_t)i;
        counts[2 * i] = 7000 + (int32_t)(2 * i);
        counts[2 * i + 1] = 7000 + (int32_t)(2 * i + 1);
    }
    const SegOut so{o.data(), p.data(), d.data(), t.data(), pix.data()};
    const SegView seg = so;  // SegOut -> SegView
    CHECK(seg.o == o.data() && seg.p == p.data() && seg.d == d.data() && seg.t == t.data() && seg.pix == pix.data());
    const GatherOut out{film.data(), rgb.data(), counts.data()};
    const int64_t offs[3] = {0, 64, 128};
    for (const int64_t off : offs) {
        const SegView s = seg.slice(off);
        const GatherOut g = out.slice(off);
        CHECK(g.accum == film.data());  // the film is not per segment
        for (int64_t i = 0; i < n - off; ++i) {  // every segment of the launches from `off` on
            for (int k = 0; k < 3; ++k) {
                CHECK(s.o[3 * i + k] == 1000.f + 3 * (off + i) + k);
                CHECK(s.p[3 * i + k] == 2000.f + 3 * (off + i) + k);
                CHECK(s.d[3 * i + k] == 3000.f + 3 * (off + i) + k);
                CHECK(g.seg_rgb[3 * i + k] == 4000.f + 3 * (off + i) + k);
            }
            CHECK(s.t[i] == 5000.f + (off + i));
            CHECK(s.pix[i] == 6000 + (int32_t)(off + i));
            CHECK(g.seg_counts[2 * i] == 7000 + (int32_t)(2 * (off + i)));
            CHECK(g.seg_counts[2 * i + 1] == 7000 + (int32_t)(2 * (off + i) + 1));
        }
        // a gather without a film has no pixel array, one without per-segment outputs no such arrays:
        // nulls stay null at every offset
        SegView np = seg;
        np.pix = nullptr;
        const SegView ns = np.slice(off);
        CHECK(ns.pix == nullptr && ns.o == s.o && ns.p == s.p && ns.d == s.d && ns.t == s.t);
        const GatherOut film_only = GatherOut{film.data(), nullptr, nullptr}.slice(off);
        CHECK(film_only.accum == film.data() && film_only.seg_rgb == nullptr && film_only.seg_counts == nullptr);
        const GatherOut rgb_only = GatherOut{nullptr, rgb.data(), nullptr}.slice(off);
        CHECK(rgb_only.accum == nullptr && rgb_only.seg_rgb == rgb.data() + 3 * off && rgb_only.seg_counts == nullptr);
        const GatherOut cnt_only = GatherOut{nullptr, nullptr, counts.data()}.slice(off);
        CHECK(cnt_only.seg_rgb == nullptr && cnt_only.seg_counts == counts.data() + 2 * off);
    }
    // slices compose: 64 then 64 is 128
    const SegView s2 = seg.slice(64).slice(64), s128 = seg.slice(128);
    CHECK(s2.o == s128.o && s2.p == s128.p && s2.d == s128.d && s2.t == s128.t && s2.pix == s128.pix);

    std::vector<float> bs(3 * 2), be(3 * 2), br(2), bp(3 * 2);
    const BeamOut bo{bs.data(), be.data(), br.data(), bp.data()};
    const BeamView bv = bo;  // BeamOut -> BeamView
    CHECK(bv.start == bs.data() && bv.end == be.data() && bv.radius == br.data() && bv.power == bp.data());

    std::printf("%d failures\n", failures);
    return failures == 0 ? 0 : 1;
}
