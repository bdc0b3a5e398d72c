/*
 * ss_undistort_steps.h -- the steps of Frame's keypoint post-processing (the rules: include/sendslam_orb.h):
 * Frame::UndistortKeyPoints, Frame::ComputeImageBounds and Frame::ComputeStereoFromRGBD.  k_undistort and k_depth
 * (ss_undistort.hip), the host twins ss_undistort_host, ss_undistort_bounds_host and ss_depth_host (ss_api_search.cpp) and
 * tests/native/undistort_steps_asan.cpp compile this text.
 *
 * The undistortion runs in double, one IEEE operation per step, left to right as written, and rounds each coordinate to float32
 * once at the end; the depth rule runs in float32 in the same manner.  Compile with -ffp-contract=off.  The divisions are correctly
 * rounded on both sides (hipcc's default).
 */
#ifndef SS_UNDISTORT_STEPS_H
#define SS_UNDISTORT_STEPS_H

#include "../../include/sendslam_orb.h"
#include "ss_float_steps.h" /* SS_HD, math.h */

/* what the rule reads of a camera; none: all four coefficients are zero and positions are copied bit for bit (72 bytes) */
struct ss_undist_cam {
    double fx, fy, cx, cy, k1, k2, p1, p2;
    int32_t none, reserved;
};

SS_HD ss_undist_cam ss_undist_cam_of(const ss_camera &c)
{
    ss_undist_cam u;
    u.fx = c.fx, u.fy = c.fy, u.cx = c.cx, u.cy = c.cy;
    u.k1 = c.k1, u.k2 = c.k2, u.p1 = c.p1, u.p2 = c.p2;
    u.none = c.k1 == 0.0 && c.k2 == 0.0 && c.p1 == 0.0 && c.p2 == 0.0;
    u.reserved = 0;
    return u;
}

/* fx and fy finite and not 0: the one refusal of the undistortion calls.  Written so that a NaN fails it */
SS_HD bool ss_undist_focal_ok(double fx, double fy)
{
    return fx - fx == 0.0 && fy - fy == 0.0 && fx != 0.0 && fy != 0.0;
}

/* every number the bounds read is finite, and the focal lengths divide */
SS_HD bool ss_undist_cam_finite(const ss_undist_cam &c)
{
    const double v[8] = {c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2};
    for (int k = 0; k < 8; k++)
        if (!(v[k] - v[k] == 0.0)) return false;
    return c.fx != 0.0 && c.fy != 0.0;
}

/* mvKeysUn of one position: cv::undistortPoints' five fixed-point iterations as oracle/vo_oracle.py::undistort states them, then
 * one rounding to float32.  Non-finite input goes through the same operations */
SS_HD void ss_undist_point(const ss_undist_cam &c, float xin, float yin, float *xout, float *yout)
{
    if (c.none) {
        *xout = xin;
        *yout = yin;
        return;
    }
    const double x0 = ((double)xin - c.cx) / c.fx, y0 = ((double)yin - c.cy) / c.fy;
    double x = x0, y = y0;
    for (int it = 0; it < 5; it++) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1.0 + (c.k2 * r2 + c.k1) * r2);
        const double dx = 2 * c.p1 * x * y + c.p2 * (r2 + 2 * x * x);
        const double dy = c.p1 * (r2 + 2 * y * y) + 2 * c.p2 * x * y;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
    *xout = (float)(x * c.fx + c.cx);
    *yout = (float)(y * c.fy + c.cy);
}

/* Frame::ComputeImageBounds: out = min_x, max_x, min_y, max_y */
SS_HD void ss_undist_bounds(const ss_undist_cam &c, int width, int height, float out[4])
{
    const float w = (float)width, h = (float)height;
    if (c.none) {
        out[0] = 0.0f, out[1] = w, out[2] = 0.0f, out[3] = h;
        return;
    }
    float x[4], y[4]; /* (0,0) (w,0) (0,h) (w,h) */
    ss_undist_point(c, 0.0f, 0.0f, &x[0], &y[0]);
    ss_undist_point(c, w, 0.0f, &x[1], &y[1]);
    ss_undist_point(c, 0.0f, h, &x[2], &y[2]);
    ss_undist_point(c, w, h, &x[3], &y[3]);
    out[0] = x[0] < x[2] ? x[0] : x[2];
    out[1] = x[1] > x[3] ? x[1] : x[3];
    out[2] = y[0] < y[1] ? y[0] : y[1];
    out[3] = y[2] > y[3] ? y[2] : y[3];
}

/* a count as told -> 0 .. rows */
SS_HD int ss_undist_clamp(int n, int rows) { return n < 0 ? 0 : n > rows ? rows : n; }

/* ---- RGB-D depth ---- */
/* step 1: what a sample is multiplied by */
SS_HD float ss_depth_inv(float factor) { return fabsf(factor) < 1e-5f ? 1.0f : 1.0f / factor; }
/* step 2: whether a float32 sample is multiplied at all (a uint16 sample always is) */
SS_HD bool ss_depth_scales_float(float inv) { return fabsf(inv - 1.0f) > 1e-5f; }

/* step 3: the pixel (int)x, (int)y of a raw position, or false outside the frame.  The range is tested on the floats, so that no
 * conversion leaves int: x in (-1, 0) truncates to column 0 as the cast does, a NaN is outside */
SS_HD bool ss_depth_pixel(float x, float y, int width, int height, int *col, int *row)
{
    if (!(x > -1.0f && x < (float)width && y > -1.0f && y < (float)height)) return false;
    *col = (int)x, *row = (int)y;
    return true;
}

/* steps 2 - 3: the sample of frame `base` (rows of row_stride bytes) at a raw position -> metres; false: none */
SS_HD bool ss_depth_sample(const uint8_t *base, int width, int height, int64_t row_stride, int depth_type, float inv, bool scale_float, float x_raw,
                           float y_raw, float *d)
{
    int col, row;
    if (!ss_depth_pixel(x_raw, y_raw, width, height, &col, &row)) return false;
    const uint8_t *line = base + (int64_t)row * row_stride;
    if (depth_type == 1) {
        *d = (float)((const uint16_t *)line)[col] * inv;
    } else {
        const float v = ((const float *)line)[col];
        *d = scale_float ? v * inv : v;
    }
    return true;
}

/* step 4: depth and right coordinate of a row from its sample (have false: none) */
SS_HD void ss_depth_row(bool have, float d, float x_un, float bf, float *right, float *depth)
{
    if (have && d > 0.0f) {
        *depth = d;
        *right = x_un - bf / d;
    } else {
        *depth = -1.0f;
        *right = -1.0f;
    }
}

#endif
