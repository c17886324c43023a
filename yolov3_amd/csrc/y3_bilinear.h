// The bilinear arithmetic of torch's F.interpolate(mode="bilinear", align_corners=False), ONE definition for every kernel that restates it
// (val_edge.hip::scale_img_kernel, batch_edge.hip).  Both translation units are built with -ffp-contract=off; the pragmas below pin the same rounding
// whatever the flags.
#pragma once
#include "y3_common.h"

// Source taps of output index o along one axis: s = max(0, ratio * (o + 0.5) - 0.5) as ONE fused multiply-add, like torch's kernels (two roundings move
// the weights by an ulp of the index: 1.7e-6 on the goldens instead of 1.2e-7); i0 = floor(s), i1 its right / lower neighbour inside the source, l = s - i0 the
// neighbour's fp32 weight.  ratio = (float)in / (float)out (torch's area_pixel_compute_scale without a scale factor), or 1 / scale_factor when one is given.
// The min() only guards the address: s < in_size for every size below 2^23.
Y3_DEV void y3_bilinear_tap(float ratio, int o, int in_size, int& i0, int& i1, float& l) {
    const float s = fmaxf(fmaf(ratio, (float)o + 0.5f, -0.5f), 0.0f);
    i0 = (int)s;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l = s - (float)i0;
}

// The four products summed in torch's order (row pairs first); hy = 1 - ly, hx = 1 - lx.
Y3_DEV float y3_bilinear_mix(float hy, float hx, float ly, float lx, float v00, float v01, float v10, float v11) {
#pragma clang fp contract(off)
    return hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
}
