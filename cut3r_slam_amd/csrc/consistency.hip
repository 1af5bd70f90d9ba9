// Multi-view depth consistency (cut3r_slam_amd/depth_consistency.py): every pixel of a reference depth map is cross-checked against up
// to 16 source views before the maps are fused (the geometric check of MVSNet / Gipuma / COLMAP fusion, plus a free-space test).  Compiled
// with -ffp-contract=off: tests/consistency_oracle.py restates every operation in this order and the results are compared bit for bit.
//
// One thread per reference pixel, grid (ceil(HW / 256), R); the thread walks its reference's sources in order and keeps its counters in
// registers.  No atomics, no shared state: every run gives the same bits.  The rigid rows of a (reference, source) pair are the same for
// the whole block.  All arithmetic is fp64, one rounding per operation; depth_avg is rounded once to fp32.
#include "common.h"

namespace {

constexpr int CONS_MAX_SRC = 16;

DEVINL bool cons_valid(float d, double depth_max) { return isfinite(d) && (double)d > 0.0 && (double)d <= depth_max; }

__global__ __launch_bounds__(256) void depth_consistency_kernel(const float* __restrict__ depth, const float* __restrict__ K, int N, int H,
                                                                int W, const int* __restrict__ ref, const int* __restrict__ src, int S,
                                                                const double* __restrict__ fwd, const double* __restrict__ bwd,
                                                                double depth_max, double pix, double rel, double z_min,
                                                                unsigned char* __restrict__ support, unsigned char* __restrict__ violation,
                                                                float* __restrict__ depth_avg) {
    const int r = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int HW = H * W;
    if (p >= HW) return;
    const size_t out = (size_t)r * HW + p;
    const int vr = ref[r];
    float df = 0.f;
    if (vr >= 0 && vr < N) df = depth[(size_t)vr * HW + p];  // an index outside the stack reads nothing (the caller refuses it first)
    if (!cons_valid(df, depth_max)) {
        support[out] = 0;
        violation[out] = 0;
        if (depth_avg) depth_avg[out] = 0.f;
        return;
    }
    const double d = (double)df;
    const double u = (double)(p % W), v = (double)(p / W);
    const double fx = (double)K[4 * vr], fy = (double)K[4 * vr + 1], cx = (double)K[4 * vr + 2], cy = (double)K[4 * vr + 3];
    const double x = (u - cx) * d / fx;
    const double y = (v - cy) * d / fy;
    const double wmax = (double)(W - 1), hmax = (double)(H - 1);
    const double keep = 1.0 - rel;
    int n_sup = 0, n_vio = 0;
    double acc = d;
    for (int k = 0; k < S; k++) {
        const int vs_ = src[(size_t)r * S + k];
        if (vs_ < 0 || vs_ >= N) continue;
        const double* F = fwd + ((size_t)r * S + k) * 12;
        const double X = ((F[0] * x + F[1] * y) + F[2] * d) + F[3];
        const double Y = ((F[4] * x + F[5] * y) + F[6] * d) + F[7];
        const double Z = ((F[8] * x + F[9] * y) + F[10] * d) + F[11];
        if (!(Z > z_min)) continue;
        const double fxs = (double)K[4 * vs_], fys = (double)K[4 * vs_ + 1], cxs = (double)K[4 * vs_ + 2], cys = (double)K[4 * vs_ + 3];
        const double us = fxs * X / Z + cxs;
        const double vs = fys * Y / Z + cys;
        if (!(us >= 0.0 && us <= wmax && vs >= 0.0 && vs <= hmax)) continue;
        const double fx0 = floor(us), fy0 = floor(vs);
        const int x0 = (int)fx0, y0 = (int)fy0;
        const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
        const float* ds_ = depth + (size_t)vs_ * HW;
        const float f00 = ds_[y0 * W + x0], f01 = ds_[y0 * W + x1], f10 = ds_[y1 * W + x0], f11 = ds_[y1 * W + x1];
        if (!(cons_valid(f00, depth_max) && cons_valid(f01, depth_max) && cons_valid(f10, depth_max) && cons_valid(f11, depth_max))) continue;
        const double t00 = (double)f00, t01 = (double)f01, t10 = (double)f10, t11 = (double)f11;
        // free space: the source sees through the reference's surface at all four taps (an interpolated depth across a discontinuity
        // of the source would mean nothing, so one nearer tap is enough to withhold the verdict)
        if (Z < t00 * keep && Z < t01 * keep && Z < t10 * keep && Z < t11 * keep) {
            n_vio++;
            continue;
        }
        const double ax = us - fx0, ay = vs - fy0;
        const double ds = (t00 * (1.0 - ax) + t01 * ax) * (1.0 - ay) + (t10 * (1.0 - ax) + t11 * ax) * ay;
        const double xs = (us - cxs) * ds / fxs;
        const double ys = (vs - cys) * ds / fys;
        const double* Bk = bwd + ((size_t)r * S + k) * 12;
        const double X2 = ((Bk[0] * xs + Bk[1] * ys) + Bk[2] * ds) + Bk[3];
        const double Y2 = ((Bk[4] * xs + Bk[5] * ys) + Bk[6] * ds) + Bk[7];
        const double Z2 = ((Bk[8] * xs + Bk[9] * ys) + Bk[10] * ds) + Bk[11];
        if (!(Z2 > z_min)) continue;
        const double du = (fx * X2 / Z2 + cx) - u;
        const double dv = (fy * Y2 / Z2 + cy) - v;
        if (du * du + dv * dv < pix * pix && fabs(Z2 - d) < rel * d) {
            n_sup++;
            acc = acc + Z2;
        }
    }
    support[out] = (unsigned char)n_sup;
    violation[out] = (unsigned char)n_vio;
    if (depth_avg) depth_avg[out] = (float)(acc / (double)(1 + n_sup));
}

}  // namespace

extern "C" int cut3r_depth_consistency(const float* depth, const float* K, int N, int H, int W, const int* ref, const int* src, int R, int S,
                                       const double* fwd, const double* bwd, double depth_max, double pix, double rel, double z_min,
                                       unsigned char* support, unsigned char* violation, float* depth_avg, void* stream) {
    if (!depth || !K || !ref || !src || !fwd || !bwd || !support || !violation) return CUT3R_ERR_ARG;
    if (N <= 0 || H <= 0 || W <= 0 || R <= 0 || S <= 0 || S > CONS_MAX_SRC || R > 65535) return CUT3R_ERR_ARG;
    if ((long long)H * W >= (1ll << 31) / 16) return CUT3R_ERR_ARG;
    if (!(depth_max > 0.0) || !(pix > 0.0) || !(rel > 0.0) || !(rel < 1.0) || !(z_min >= 0.0)) return CUT3R_ERR_ARG;
    const int nblk = (H * W + 255) / 256;
    hipLaunchKernelGGL(depth_consistency_kernel, dim3(nblk, R), dim3(256), 0, (hipStream_t)stream, depth, K, N, H, W, ref, src, S, fwd, bwd,
                       depth_max, pix, rel, z_min, support, violation, depth_avg);
    return cut3r_check_launch();
}
