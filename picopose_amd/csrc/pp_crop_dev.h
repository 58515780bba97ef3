// Device functions of the crop kernels: cv2.resize's INTER_LINEAR taps and INTER_NEAREST index on a crop window, the
// normalised colour blend and the back-projection of a depth sample.  One statement of the arithmetic for
// pp_crop_resize_normalize / pp_depth_points_nearest (pp_sample.hip) and pp_templates_crop (pp_render.hip), so the
// batched template crop is bit-equal to the per-view calls by construction.  Include it BEFORE any
// `#pragma clang fp contract`: these expressions are compiled in the build's default mode in every translation unit.
#ifndef PP_CROP_DEV_H
#define PP_CROP_DEV_H
#include <hip/hip_runtime.h>

// INTER_LINEAR taps of output index o over a source extent n resized to S (pixel centres, edge clamp)
__device__ __forceinline__ void pp_crop_taps(int o, int n, int S_, int& i0, int& i1, double& fr) {
    const double f = ((double)o + 0.5) * ((double)n / (double)S_) - 0.5;
    i0 = (int)floor(f);
    fr = f - (double)i0;
    if (i0 < 0) {
        i0 = 0;
        fr = 0.0;
    }
    if (i0 >= n - 1) {
        i0 = n - 1;
        fr = 0.0;
    }
    i1 = i0 + 1 < n ? i0 + 1 : n - 1;
}

// INTER_NEAREST source index of output index o
__device__ __forceinline__ int pp_crop_nearest(int o, int n, int S_) {
    const int i = (int)floor((double)o * ((double)n / (double)S_));
    return i < n - 1 ? i : n - 1;
}

// (bilinear blend of px(y, x, c) - mean) / std in double, rounded to float once; px returns the channel value / 255 (masked or not)
template <class Px>
__device__ __forceinline__ float pp_crop_blend(Px px, int c, int ya, int yb, int xa, int xb, double fx, double fy, double mean,
                                               double stdv) {
    const double top = px(ya, xa, c) * (1.0 - fx) + px(ya, xb, c) * fx;
    const double bot = px(yb, xa, c) * (1.0 - fx) + px(yb, xb, c) * fx;
    return (float)(((top * (1.0 - fy) + bot * fy) - mean) / stdv);
}

// utils/data_utils.py:97-115 at image pixel (x, y) with depth z
__device__ __forceinline__ void pp_depth_point(float z, int x, int y, float fx, float fy, float cx, float cy, float* out) {
    out[0] = ((float)x - cx) * z / fx;
    out[1] = ((float)y - cy) * z / fy;
    out[2] = z;
}

#endif
