// The coefficient arithmetic of cv2.resize(INTER_LINEAR) on 8-bit images, ONE definition for every kernel that restates it (val_edge.hip::letterbox_u8_kernel,
// crops.hip::crop_resize_kernel).  Restated from OpenCV's resize.cpp (HResizeLinear / VResizeLinear<uchar, int, short>); the Python statement of the same
// arithmetic is oracle.yolo_oracle.resize_linear_u8.
#pragma once
#include "y3_common.h"

// Output index d along one axis of `size` source pixels, scale = 1 / (out / in) in double: the source coordinate f = (d + 0.5) * scale - 0.5 in double, cast to
// float; s = floor(f) and the two taps' weights saturate_cast<short>(w * 2048) (round half to even).  clamp_frac (the x axis): a column left of 0 or right of
// size - 1 reads the border pixel with weight 2048; on the y axis the caller clamps the rows and the fractional weights are kept.
Y3_DEV void y3_resize_coef(int d, double scale, int size, bool clamp_frac, int& s, int& c0, int& c1) {
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
    if (clamp_frac) {   // x axis: outside columns read one pixel with full weight
        if (s < 0) { f = 0.0f; s = 0; }
        if (s >= size - 1) { f = 0.0f; s = size - 1; }
    }
    c0 = (int)(short)__float2int_rn((1.0f - f) * 2048.0f);
    c1 = (int)(short)__float2int_rn(f * 2048.0f);
}
