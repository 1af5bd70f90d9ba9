// LPIPS (AlexNet) of the rendering evaluation (cut3r_slam_amd/lpips.py; the reference's gaussian/utils/eval_utils.py:29,83,92 and
// :115,141,150, torchmetrics LearnedPerceptualImagePatchSimilarity(net_type="alex", normalize=True)).  Compiled with -ffp-contract=off:
// tests/lpips_oracle.py restates every operation in this order and the feature maps and the per-tap maps are compared bit for bit.
//
// Activations are channels-last fp32 [n, H, W, C]; the n images of a call are the B first images followed by the B second images.  A
// convolution weight is [kh, kw, ci, co] (k = (ky kw + kx) ci_n + ci, co fastest), so that one output is the chain
//     acc = bias[co];  acc = fmaf(w[k, co], x[k], acc) for k ascending;  relu
// with x[k] = 0 on a padded tap.  The convolution is an implicit GEMM (M = output pixels of all images, N = co, K = kh kw ci) on
// v_mfma_f32_32x32x2_f32, which IS that chain: D = fma(a_k1, b_k1, fma(a_k0, b_k0, C)), one rounding per product.  Every accumulator walks
// the whole K in ascending order (no split-K, no second accumulator per output), so the bits do not depend on the tile an output falls in,
// nor on how many images a call carries.  impl = 1 runs the same chain as explicit fmaf on the VALU, one thread per output (the check of
// the MFMA path, and its replacement should a layer ever differ); impl = 2 / 3 force the 128- / 64-row tile that impl = 0 chooses by M.
//
// No floating-point atomics anywhere: the fp64 sum of a tap is a fixed strided partial per thread and a fixed tree per block.
#include "common.h"

namespace {

constexpr int BN = 64, BK = 16;               // block tile of the MFMA convolution: (64 or 128) x 64 x 16
constexpr int LPIPS_CUS = 256;                // workgroups below which the 64-row tile is chosen (one per compute unit of the MI355X)

struct ConvShape {
    int H, W, Ci, Co, KH, KW, stride, pad, Ho, Wo, M, K;        // M = images x Ho x Wo, K = KH x KW x Ci
};

// ---------------------------------------------------------------------------------------------------------------- input transform
// [n,3,H,W] in [0,1] -> channels-last [n,H,W,3]: x = ((2 v - 1) - shift_c) / scale_c, every step rounded, the division correctly rounded
__global__ __launch_bounds__(256) void lpips_input_kernel(const float* __restrict__ a, const float* __restrict__ b, int B, int HW,
                                                          float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;               // over n * HW * 3, c fastest
    const size_t total = (size_t)2 * B * HW * 3;
    if (i >= total) return;
    const int c = (int)(i % 3);
    const size_t p = i / 3;
    const int img = (int)(p / HW);
    const size_t px = p % HW;
    const float* src = img < B ? a + (size_t)img * 3 * HW : b + (size_t)(img - B) * 3 * HW;
    const float v = src[(size_t)c * HW + px];
    const float shift = c == 0 ? -.030f : (c == 1 ? -.088f : -.188f);
    const float scale = c == 0 ? .458f : (c == 1 ? .448f : .450f);
    out[i] = ((2.0f * v - 1.0f) - shift) / scale;
}

// ---------------------------------------------------------------------------------------------------------------- convolution (MFMA)
// Block tile (32 WM x 2) x 64 x 16, 4 waves, each WM independent 32x32 accumulators along M (WM = 2: 128 rows, the B operand shared by
// both; WM = 1: 64 rows, twice the workgroups when M is small).  The next k-tile is fetched into registers while the MFMAs of this one run.
// VEC: Ci % 8 == 0, so a run of 8 aligned k shares one tap and is 32 contiguous bytes of the input.
template <bool VEC, int WM>
__global__ __launch_bounds__(256) void lpips_conv_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ y, const ConvShape s) {
    constexpr int TM = 64 * WM;             // rows of the block tile
    constexpr int NA = BK * TM / 256;       // 256 threads gather TM rows x BK: NA consecutive k each, 8 (WM 2) or 4 (WM 1)
    __shared__ float As[BK][TM + 32];       // row strides of 32 mod 64 banks: the two k rows a wave reads fall on different banks
    __shared__ float Bs[BK][BN + 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * TM, n0 = blockIdx.y * BN;
    // gather role: row gm of the tile, NA consecutive k from gk
    const int gm = tid & (TM - 1), gk = (tid / TM) * NA;
    const int mg = m0 + gm;
    const bool mvalid = mg < s.M;
    int iy0 = 0, ix0 = 0;
    const float* ximg = x;
    if (mvalid) {
        const int per = s.Ho * s.Wo;
        const int img = mg / per, r = mg - img * per;
        const int oy = r / s.Wo, ox = r - oy * s.Wo;
        iy0 = oy * s.stride - s.pad;
        ix0 = ox * s.stride - s.pad;
        ximg = x + (size_t)img * s.H * s.W * s.Ci;
    }
    // weight role: row bk of the tile, 4 consecutive co
    const int bk = tid >> 4, bn = (tid & 15) * 4;
    // MFMA role
    const int wm = (wave & 1) * 32 * WM, wn = (wave >> 1) * 32;
    const int li = lane & 31, lk = lane >> 5;
    const float bv = bias[n0 + wn + li];                                  // Co % BN == 0 (checked by the entry point)
    f32x16 acc[WM];
#pragma unroll
    for (int t = 0; t < WM; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = bv;

    float av[NA];
    float4 wv;
    // the operands of k-tile k0 into registers; a padded tap, a row past M and a k past K give 0, and no address is formed for them
    auto fetch = [&](int k0) {
#pragma unroll
        for (int j = 0; j < NA; ++j) av[j] = 0.f;
        const int kb = k0 + gk;
        if (mvalid && kb < s.K) {
            int tap = kb / s.Ci, ci = kb - tap * s.Ci;
            int ky = tap / s.KW, kx = tap - ky * s.KW;
            if (VEC) {                                                     // K % 8 == 0 and NA | 8: the whole run is inside K and one tap
                const int iy = iy0 + ky, ix = ix0 + kx;
                if (iy >= 0 && iy < s.H && ix >= 0 && ix < s.W) {
                    const float4* p = reinterpret_cast<const float4*>(ximg + ((size_t)iy * s.W + ix) * s.Ci + ci);
#pragma unroll
                    for (int q = 0; q < NA / 4; ++q) {
                        const float4 u = p[q];
                        av[4 * q] = u.x; av[4 * q + 1] = u.y; av[4 * q + 2] = u.z; av[4 * q + 3] = u.w;
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < NA; ++j) {
                    const int iy = iy0 + ky, ix = ix0 + kx;
                    if (kb + j < s.K && iy >= 0 && iy < s.H && ix >= 0 && ix < s.W) av[j] = ximg[((size_t)iy * s.W + ix) * s.Ci + ci];
                    if (++ci == s.Ci) {                                    // the next k: ci fastest, then kx, then ky
                        ci = 0;
                        if (++kx == s.KW) { kx = 0; ++ky; }
                    }
                }
            }
        }
        wv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k0 + bk < s.K) wv = *reinterpret_cast<const float4*>(w + (size_t)(k0 + bk) * s.Co + n0 + bn);
    };

    fetch(0);
    for (int k0 = 0; k0 < s.K; k0 += BK) {
        __syncthreads();                                                   // the previous tile's MFMAs have read the LDS
#pragma unroll
        for (int j = 0; j < NA; ++j) As[gk + j][gm] = av[j];
        *reinterpret_cast<float4*>(&Bs[bk][bn]) = wv;
        __syncthreads();
        if (k0 + BK < s.K) fetch(k0 + BK);                                 // in flight during the MFMAs below
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const float b = Bs[kk + lk][wn + li];
#pragma unroll
            for (int t = 0; t < WM; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + lk][wm + 32 * t + li], b, acc[t], 0, 0, 0);
        }
    }
    // C/D map of the 32x32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int co = n0 + wn + li;
#pragma unroll
    for (int t = 0; t < WM; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + wm + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lk;
            if (m < s.M) y[(size_t)m * s.Co + co] = fmaxf(acc[t][r], 0.f);
        }
}

// the same chain on the VALU: one thread per output, co fastest
__global__ __launch_bounds__(256) void lpips_conv_valu_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ y, const ConvShape s) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)s.M * s.Co) return;
    const int co = (int)(i % s.Co), mg = (int)(i / s.Co);
    const int per = s.Ho * s.Wo;
    const int img = mg / per, r = mg - img * per;
    const int oy = r / s.Wo, ox = r - oy * s.Wo;
    const float* ximg = x + (size_t)img * s.H * s.W * s.Ci;
    float acc = bias[co];
    for (int ky = 0; ky < s.KH; ++ky)
        for (int kx = 0; kx < s.KW; ++kx) {
            const int iy = oy * s.stride - s.pad + ky, ix = ox * s.stride - s.pad + kx;
            const bool in = iy >= 0 && iy < s.H && ix >= 0 && ix < s.W;
            const float* px = in ? ximg + ((size_t)iy * s.W + ix) * s.Ci : nullptr;
            const float* wk = w + (size_t)(ky * s.KW + kx) * s.Ci * s.Co + co;
            for (int ci = 0; ci < s.Ci; ++ci) acc = fmaf(wk[(size_t)ci * s.Co], in ? px[ci] : 0.f, acc);
        }
    y[i] = fmaxf(acc, 0.f);
}

// ---------------------------------------------------------------------------------------------------------------- 3x3 stride-2 max-pool
// no padding, floor: every window lies inside the input
__global__ __launch_bounds__(256) void lpips_pool_kernel(const float* __restrict__ x, int n, int H, int W, int C, int Ho, int Wo,
                                                         float* __restrict__ y) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)n * Ho * Wo * C) return;
    const int c = (int)(i % C);
    size_t p = i / C;
    const int ox = (int)(p % Wo);
    p /= Wo;
    const int oy = (int)(p % Ho), img = (int)(p / Ho);
    const float* base = x + (((size_t)img * H + 2 * oy) * W + 2 * ox) * C + c;
    float m = base[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) m = fmaxf(m, base[((size_t)dy * W + dx) * C]);
    y[i] = m;
}

// ---------------------------------------------------------------------------------------------------------------- tail of one tap
// one thread per (pair, pixel): both feature vectors once for the two sums of squares, once more for the weighted squared difference
template <bool LPIPS_NORM>
__global__ __launch_bounds__(256) void lpips_tail_kernel(const float* __restrict__ feat, const float* __restrict__ lin, int B, int P, int C,
                                                         float* __restrict__ v) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * P) return;
    const float4* f0 = reinterpret_cast<const float4*>(feat + i * C);                       // C % 4 == 0
    const float4* f1 = reinterpret_cast<const float4*>(feat + ((size_t)B * P + i) * C);
    const float4* l4 = reinterpret_cast<const float4*>(lin);
    float s0 = 0.f, s1 = 0.f;
#pragma unroll 8
    for (int c = 0; c < C / 4; ++c) {
        const float4 p = f0[c], q = f1[c];
        s0 = fmaf(p.x, p.x, s0); s0 = fmaf(p.y, p.y, s0); s0 = fmaf(p.z, p.z, s0); s0 = fmaf(p.w, p.w, s0);
        s1 = fmaf(q.x, q.x, s1); s1 = fmaf(q.y, q.y, s1); s1 = fmaf(q.z, q.z, s1); s1 = fmaf(q.w, q.w, s1);
    }
    const float d0 = LPIPS_NORM ? sqrtf(s0) + 1e-10f : sqrtf(1e-8f + s0);
    const float d1 = LPIPS_NORM ? sqrtf(s1) + 1e-10f : sqrtf(1e-8f + s1);
    float acc = 0.f;
#pragma unroll 8
    for (int c = 0; c < C / 4; ++c) {
        const float4 p = f0[c], q = f1[c], l = l4[c];
        float d;
        d = p.x / d0 - q.x / d1; acc = fmaf(l.x, d * d, acc);
        d = p.y / d0 - q.y / d1; acc = fmaf(l.y, d * d, acc);
        d = p.z / d0 - q.z / d1; acc = fmaf(l.z, d * d, acc);
        d = p.w / d0 - q.w / d1; acc = fmaf(l.w, d * d, acc);
    }
    v[i] = acc;
}

// one block per pair: thread t adds v[t], v[t + 256], ... in fp64, then a fixed tree; score[b] (+)= sum / P
__global__ __launch_bounds__(256) void lpips_mean_kernel(const float* __restrict__ v, int P, int accumulate, double* __restrict__ score) {
    __shared__ double part[256];
    const float* vb = v + (size_t)blockIdx.x * P;
    double s = 0.0;
    for (int i = threadIdx.x; i < P; i += 256) s += (double)vb[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mean = part[0] / (double)P;
        score[blockIdx.x] = accumulate ? score[blockIdx.x] + mean : mean;
    }
}

bool blocks_for(size_t items, unsigned* grid) {
    const size_t g = (items + 255) / 256;
    if (g == 0 || g > 0x7fffffffull) return false;
    *grid = (unsigned)g;
    return true;
}

}  // namespace

extern "C" {

int cut3r_lpips_input(const float* a, const float* b, int B, int H, int W, float* out, void* stream) {
    if (!a || !b || !out || B <= 0 || H <= 0 || W <= 0) return CUT3R_ERR_ARG;
    if ((long long)H * W > 0x7fffffffll) return CUT3R_ERR_ARG;
    unsigned grid;
    if (!blocks_for((size_t)2 * B * H * W * 3, &grid)) return CUT3R_ERR_ARG;
    hipLaunchKernelGGL(lpips_input_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a, b, B, H * W, out);
    return cut3r_check_launch();
}

int cut3r_lpips_conv_out(int in, int k, int stride, int pad) {
    if (in <= 0 || k <= 0 || stride <= 0 || pad < 0 || in + 2 * pad < k) return 0;
    return (in + 2 * pad - k) / stride + 1;
}

int cut3r_lpips_conv(const float* x, const float* w, const float* bias, float* y, int n, int H, int W, int Ci, int Co, int KH, int KW,
                     int stride, int pad, int impl, void* stream) {
    if (!x || !w || !bias || !y || n <= 0 || H <= 0 || W <= 0 || Ci <= 0 || Co <= 0 || KH <= 0 || KW <= 0 || stride <= 0 || pad < 0)
        return CUT3R_ERR_ARG;
    if (impl < 0 || impl > 3) return CUT3R_ERR_ARG;
    if (pad >= KH || pad >= KW) return CUT3R_ERR_ARG;
    ConvShape s;
    s.H = H; s.W = W; s.Ci = Ci; s.Co = Co; s.KH = KH; s.KW = KW; s.stride = stride; s.pad = pad;
    s.Ho = cut3r_lpips_conv_out(H, KH, stride, pad);
    s.Wo = cut3r_lpips_conv_out(W, KW, stride, pad);
    if (s.Ho <= 0 || s.Wo <= 0) return CUT3R_ERR_ARG;                                        // the output would be empty
    const long long M = (long long)n * s.Ho * s.Wo, K = (long long)KH * KW * Ci;
    if (M > 0x7fffffffll - 128 || K > 0x7fffffffll - BK || (long long)n * H * W > 0x7fffffffll) return CUT3R_ERR_ARG;
    s.M = (int)M;
    s.K = (int)K;
    if (impl == 1) {
        unsigned grid;
        if (!blocks_for((size_t)M * Co, &grid)) return CUT3R_ERR_ARG;
        hipLaunchKernelGGL(lpips_conv_valu_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, w, bias, y, s);
        return cut3r_check_launch();
    }
    if (Co % BN != 0 || Co / BN > 65535) return CUT3R_ERR_ARG;
    // 128-row tiles when they give every compute unit a workgroup, else 64-row tiles (impl 2 / 3 force one: the bits are the same)
    const bool wide = impl == 2 || (impl == 0 && ((M + 127) / 128) * (Co / BN) >= LPIPS_CUS);
    const int TM = wide ? 128 : 64;
    const dim3 grid((unsigned)((M + TM - 1) / TM), (unsigned)(Co / BN));
    auto kernel = Ci % 8 == 0 ? (wide ? lpips_conv_mfma_kernel<true, 2> : lpips_conv_mfma_kernel<true, 1>)
                              : (wide ? lpips_conv_mfma_kernel<false, 2> : lpips_conv_mfma_kernel<false, 1>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, (hipStream_t)stream, x, w, bias, y, s);
    return cut3r_check_launch();
}

int cut3r_lpips_pool(const float* x, float* y, int n, int H, int W, int C, void* stream) {
    if (!x || !y || n <= 0 || C <= 0 || H < 3 || W < 3) return CUT3R_ERR_ARG;                // below 3 the output would be empty
    const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
    if ((long long)n * H * W > 0x7fffffffll) return CUT3R_ERR_ARG;
    unsigned grid;
    if (!blocks_for((size_t)n * Ho * Wo * C, &grid)) return CUT3R_ERR_ARG;
    hipLaunchKernelGGL(lpips_pool_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, n, H, W, C, Ho, Wo, y);
    return cut3r_check_launch();
}

int cut3r_lpips_tail(const float* feat, const float* lin, int B, int P, int C, int norm, int accumulate, float* v, double* score,
                     void* stream) {
    if (!feat || !lin || !v || !score || B <= 0 || P <= 0 || C <= 0 || C % 4 != 0) return CUT3R_ERR_ARG;
    if (norm != 0 && norm != 1) return CUT3R_ERR_ARG;
    if ((long long)B * P > 0x7fffffffll) return CUT3R_ERR_ARG;
    unsigned grid;
    if (!blocks_for((size_t)B * P, &grid)) return CUT3R_ERR_ARG;
    if (norm == 1)
        hipLaunchKernelGGL(lpips_tail_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, feat, lin, B, P, C, v);
    else
        hipLaunchKernelGGL(lpips_tail_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, feat, lin, B, P, C, v);
    if (int rc = cut3r_check_launch()) return rc;
    hipLaunchKernelGGL(lpips_mean_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, v, P, accumulate ? 1 : 0, score);
    return cut3r_check_launch();
}

}  // extern "C"
