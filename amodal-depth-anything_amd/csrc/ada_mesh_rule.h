// The candidate rule that the regular mesh (ada_geometry.hip) and the adaptive mesh (ada_adaptive.hip) share: depth -> z, which z makes a vertex, and
// the host's checks of the arguments that state it.  Both files are built with -ffp-contract=off; the products and sums are spelled rounded anyway.
#pragma once
#include "ada_common.h"

namespace {

struct ZRule {
    int inverse;     // 0: z = depth; 1: z = 1 / (a * depth + b)
    double a, b;
};

ADA_DEV double z_of(const ZRule& r, float d) {
    const double v = (double)d;
    if (!r.inverse) return v;
    return 1.0 / __dadd_rn(__dmul_rn(r.a, v), r.b);     // the correctly rounded quotient: no fast-math flag in this build
}
ADA_DEV bool z_valid(double z) { return z > 0.0 && z < __builtin_inf(); }     // finite and positive; false for NaN

// the arguments that ada_mesh_triangles_fwd and ada_mesh_adaptive_fwd take alike; `who` names the entry point in the message
int mesh_rule_check(const char* who, const uint8_t* mask, int64_t row_pitch_bytes, int64_t image_stride_bytes, int32_t inverse, double max_ratio,
                    int32_t batch, int32_t h, int32_t w, int32_t capacity) {
    ADA_REQUIRE(capacity >= 0 && (int64_t)batch * capacity * 3 < ((int64_t)1 << 40), ADA_EINVAL, "%s: capacity=%d", who, capacity);
    ADA_REQUIRE(inverse == 0 || inverse == 1, ADA_EINVAL, "%s: inverse=%d (0 or 1)", who, inverse);
    ADA_REQUIRE(!mask || (row_pitch_bytes >= w && (batch == 1 || image_stride_bytes >= (int64_t)(h - 1) * row_pitch_bytes + w)), ADA_EINVAL,
                "%s: mask pitch %ld / stride %ld too small for %d x %d", who, (long)row_pitch_bytes, (long)image_stride_bytes, h, w);
    ADA_REQUIRE(max_ratio == max_ratio, ADA_EINVAL, "%s: max_ratio is NaN", who);
    return ADA_OK;
}

}  // namespace
