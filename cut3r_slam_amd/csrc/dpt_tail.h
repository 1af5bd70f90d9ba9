// Per-pixel tail of the DPT head: the final 1x1 convolution (Cin -> 4) on the fp16 output of head.2 and the point / confidence
// activations (heads/postprocess.py:11-28,113-151).  ONE piece of code for the stand-alone kernels (elementwise.hip, compiled
// with FMA contraction on) and for the epilogue of the 192 x 128 convolution tile (gemm.hip, compiled with -ffp-contract=off):
// every multiply-add below is either an explicit fmaf or, under `#pragma clang fp contract(off)`, a separate multiply and add, so
// the rounding of a pixel does not depend on the translation unit that inlines it.
//
// Lane layout: LPP = Cin / 8 lanes per pixel (LPP divides 64), lane `chunk` of a pixel owns the 8 consecutive channels
// chunk * 8 .. chunk * 8 + 7.  All 64 lanes of the wave must be active through dpt_lane_sum.
#pragma once
#include "common.h"

// partial dot product of this lane's 8 channels with its 8 weights of one output row of the final convolution: an fmaf chain from 0,
// channel order
DEVINL float dpt_dot8(const half8_t& v, const float (&w)[8]) {
    float a = 0.f;
#pragma unroll
    for (int e = 0; e < 8; e++) a = fmaf((float)v[e], w[e], a);
    return a;
}

// the LPP partial sums of a pixel combined by xor-shuffles, distances LPP/2 .. 1: every lane of the pixel ends with the same four totals
// (a + b and b + a are the same bits)
DEVINL void dpt_lane_sum(float (&a)[4], int lpp) {
    for (int o = lpp >> 1; o > 0; o >>= 1) {
        a[0] += __shfl_xor(a[0], o, 64);
        a[1] += __shfl_xor(a[1], o, 64);
        a[2] += __shfl_xor(a[2], o, 64);
        a[3] += __shfl_xor(a[3], o, 64);
    }
}

// the same sums for LPP = 16 without the LDS crossbar: the partner at xor distance 8, 4, 2, 1 inside a DPP row of 16 lanes is a row rotation
// by 8, a rotation by 4 (lanes with bit 2 set read lane - 4) merged with one by 12 (the others read lane + 4), and two quad permutations.
// Same partners, same adds, same order: the bits of dpt_lane_sum(a, 16).
template <int CTRL, int BANKS>
DEVINL float dpt_dpp(float keep, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, keep), __builtin_bit_cast(int, v), CTRL, 0xF, BANKS, false));
}
DEVINL void dpt_lane_sum16(float (&a)[4]) {
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] += dpt_dpp<0x128, 0xF>(a[k], a[k]);                                        // row_ror:8
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] += dpt_dpp<0x12C, 0x5>(dpt_dpp<0x124, 0xA>(a[k], a[k]), a[k]);             // row_ror:4 | row_ror:12
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] += dpt_dpp<0x4E, 0xF>(a[k], a[k]);                                         // quad_perm [2,3,0,1]
#pragma unroll
    for (int k = 0; k < 4; k++) a[k] += dpt_dpp<0xB1, 0xF>(a[k], a[k]);                                         // quad_perm [1,0,3,2]
}

// pts = xyz / max(|xyz|, 1e-8) * expm1(|xyz|) and conf = 1 + exp(c), stored to pts[0..2] and conf[0].
// The squared norm is written as the contraction-on build of each stand-alone kernel has always computed it (one of the two adds of
// x*x + y*y + z*z was contracted, and not the same one in both): YX = true  fma(y, y, x*x) + z*z  (coalesced kernel, convolution
// epilogue), YX = false  fma(x, x, y*y) + z*z  (per-lane kernel).
template <bool YX>
DEVINL void dpt_pts_conf(float x, float y, float z, float c, float* pts, float* conf) {
#pragma clang fp contract(off)
    const float xx = x * x, yy = y * y, zz = z * z;
    const float d = sqrtf((YX ? fmaf(y, y, xx) : fmaf(x, x, yy)) + zz);
    const float dc = fmaxf(d, 1e-8f);
    const float e = expm1f(d);
    pts[0] = x / dc * e;
    pts[1] = y / dc * e;
    pts[2] = z / dc * e;
    conf[0] = 1.0f + expf(c);
}
// the same on a pixel's four totals: the bias of the final convolution is added last, to the combined sum
DEVINL void dpt_bias_pts_conf(const float (&a)[4], float b0, float b1, float b2, float b3, float* pts, float* conf) {
    dpt_pts_conf<true>(a[0] + b0, a[1] + b1, a[2] + b2, a[3] + b3, pts, conf);
}
