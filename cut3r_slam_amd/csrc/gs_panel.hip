// Diagnostic panels and single-layer frames of the Gaussian mapper (GSMapper.panel / viz, cut3r_slam_amd/gs_view.py): the image
// composition of hislam2/gs_backend_per_frame.py:596-637 (`viz`) as two launches with no host round trip between them.  Compiled with
// -ffp-contract=off: tests/gs_panel_oracle.py restates every operation in this order and every byte is compared.
//
//   panel_ranges   min and max of the four maps the turbo cells normalise by (a, b, |a - b|, alpha > 0.5).  Min and max are exact, so
//                  the reduction order cannot change a bit: threads, waves and workgroups reduce the ORDER-PRESERVING uint32 image of
//                  the floats (key), and one integer atomicMax per value and workgroup lands in ranges[8].  The minimum is kept as the
//                  maximum of ~key, so an all-zero buffer is the identity of all eight slots: a memset node, not a launch, clears it.
//   panel          one thread = PANEL_PIX consecutive pixels of one image row -> the same pixels of all nine cells.  Reads run along
//                  rows; the four central-difference neighbours of the depth normal come through the cache.  The 9W-byte rows carry no
//                  alignment: when W % 4 == 0 a thread's 12 bytes of a cell are three aligned dword stores, otherwise byte stores.
//   frame          one layer of one image through the same cell code.
// Inputs are finite (documented, not checked).
#include "common.h"

namespace {

constexpr int PANEL_PIX = 4;
constexpr int RANGE_SLOTS = 4;  // a, b, |a - b|, alpha > 0.5

__constant__ unsigned char TURBO_U8[768] = {
#include "turbo_u8.h"
};

DEVINL unsigned f2key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
DEVINL float key2f(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

DEVINL unsigned wave_umax(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}

__global__ __launch_bounds__(256) void panel_ranges_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           const float* __restrict__ alpha, int n, unsigned* __restrict__ ranges) {
    unsigned k[2 * RANGE_SLOTS];
#pragma unroll
    for (int s = 0; s < 2 * RANGE_SLOTS; s++) k[s] = 0u;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        float v[RANGE_SLOTS];
        bool have[RANGE_SLOTS] = {a != nullptr, b != nullptr, a != nullptr && b != nullptr, alpha != nullptr};
        v[0] = a ? a[i] : 0.f;
        v[1] = b ? b[i] : 0.f;
        v[2] = fabsf(v[0] - v[1]);
        v[3] = (alpha && alpha[i] > 0.5f) ? 1.f : 0.f;
#pragma unroll
        for (int s = 0; s < RANGE_SLOTS; s++)
            if (have[s]) {
                const unsigned key = f2key(v[s]);
                k[2 * s] = max(k[2 * s], ~key);
                k[2 * s + 1] = max(k[2 * s + 1], key);
            }
    }
    __shared__ unsigned part[4][2 * RANGE_SLOTS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int s = 0; s < 2 * RANGE_SLOTS; s++) {
        const unsigned m = wave_umax(k[s]);
        if (lane == 0) part[wave][s] = m;
    }
    __syncthreads();
    if (threadIdx.x < 2 * RANGE_SLOTS) {
        const int s = threadIdx.x;
        const unsigned m = max(max(part[0][s], part[1][s]), max(part[2][s], part[3][s]));
        if (m) atomicMax(&ranges[s], m);
    }
}

// ---- the cell arithmetic (include/cut3r_hip.h states it; tests/gs_panel_oracle.py restates it)
struct Range {
    float lo, den;
};
DEVINL Range load_range(const unsigned* __restrict__ ranges, int slot) {
    const float lo = key2f(~ranges[2 * slot]), hi = key2f(ranges[2 * slot + 1]);
    return {lo, (float)((double)hi - (double)lo + 1e-10)};
}
DEVINL Range fixed_range(float lo, float hi) { return {lo, (float)((double)hi - (double)lo + 1e-10)}; }

DEVINL unsigned pack3(unsigned r, unsigned g, unsigned b) { return r | (g << 8) | (b << 16); }

DEVINL unsigned turbo_px(float x, Range r) {
    float q = __fdiv_rn(x - r.lo, r.den);
    q = fminf(fmaxf(q, 0.f), 1.f);
    const int idx = (int)(q * 255.f);
    return pack3(TURBO_U8[3 * idx], TURBO_U8[3 * idx + 1], TURBO_U8[3 * idx + 2]);
}
DEVINL unsigned color_u8(float v) {
    const double c = fmin(fmax((double)v, 0.0), 1.0);
    return (unsigned)floor(c * 255.0 + 0.5);
}
DEVINL unsigned color_px(float r, float g, float b) { return pack3(color_u8(r), color_u8(g), color_u8(b)); }
DEVINL unsigned normal_px(float nx, float ny, float nz) {
    return color_px((nx + 1.f) * 0.5f, (ny + 1.f) * 0.5f, (nz + 1.f) * 0.5f);
}

// gs_mapper.depth_to_normal at (x, y): zero on the one-pixel border
DEVINL void depth_normal(const float* __restrict__ d, int x, int y, int H, int W, float fx, float fy, float cx, float cy, float n[3]) {
    n[0] = n[1] = n[2] = 0.f;
    if (x < 1 || y < 1 || x > W - 2 || y > H - 2) return;
    const float rxm = __fdiv_rn((float)(x - 1) - cx, fx), rxp = __fdiv_rn((float)(x + 1) - cx, fx), rx = __fdiv_rn((float)x - cx, fx);
    const float rym = __fdiv_rn((float)(y - 1) - cy, fy), ryp = __fdiv_rn((float)(y + 1) - cy, fy), ry = __fdiv_rn((float)y - cy, fy);
    const float dl = d[y * W + x - 1], dr = d[y * W + x + 1], du = d[(y - 1) * W + x], dd = d[(y + 1) * W + x];
    const float ax = rxp * dr - rxm * dl, ay = ry * dr - ry * dl, az = dr - dl;   // p(x+1, y) - p(x-1, y)
    const float bx = rx * dd - rx * du, by = ryp * dd - rym * du, bz = dd - du;   // p(x, y+1) - p(x, y-1)
    const float c0 = ay * bz - az * by, c1 = az * bx - ax * bz, c2 = ax * by - ay * bx;
    const float len = fmaxf(__fsqrt_rn((c0 * c0 + c1 * c1) + c2 * c2), 1e-12f);
    n[0] = __fdiv_rn(c0, len);
    n[1] = __fdiv_rn(c1, len);
    n[2] = __fdiv_rn(c2, len);
}

// PANEL_PIX packed pixels (0x00bbggrr each) -> 3 PANEL_PIX bytes at dst: three dword stores when `wide`, byte stores otherwise
DEVINL void store_px(unsigned char* __restrict__ dst, const unsigned px[PANEL_PIX], int count, bool wide) {
    if (wide) {
        unsigned* w = reinterpret_cast<unsigned*>(dst);
        w[0] = px[0] | (px[1] << 24);
        w[1] = (px[1] >> 8) | (px[2] << 16);
        w[2] = (px[2] >> 16) | (px[3] << 8);
        return;
    }
    for (int j = 0; j < count; j++) {
        dst[3 * j] = (unsigned char)(px[j] & 255u);
        dst[3 * j + 1] = (unsigned char)((px[j] >> 8) & 255u);
        dst[3 * j + 2] = (unsigned char)((px[j] >> 16) & 255u);
    }
}

__global__ __launch_bounds__(256) void panel_kernel(const float* __restrict__ gt, const float* __restrict__ render,
                                                    const float* __restrict__ exp_a, const float* __restrict__ exp_b,
                                                    const float* __restrict__ gt_depth, const float* __restrict__ depth,
                                                    const float* __restrict__ normal, const float* __restrict__ alpha, float fx, float fy,
                                                    float cx, float cy, int H, int W, const unsigned* __restrict__ ranges,
                                                    unsigned char* __restrict__ out, bool wide) {
    const int groups = (W + PANEL_PIX - 1) / PANEL_PIX;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= groups * H) return;
    const int y = t / groups, x0 = (t - y * groups) * PANEL_PIX;
    const int count = min(PANEL_PIX, W - x0);
    const size_t HW = (size_t)H * W;
    const Range r_gtd = load_range(ranges, 0), r_d = load_range(ranges, 1), r_diff = load_range(ranges, 2), r_mask = load_range(ranges, 3);
    float A[9], B[3];
#pragma unroll
    for (int i = 0; i < 9; i++) A[i] = exp_a[i];
#pragma unroll
    for (int i = 0; i < 3; i++) B[i] = exp_b[i];
    unsigned px[9][PANEL_PIX];
#pragma unroll
    for (int j = 0; j < PANEL_PIX; j++) {
        const int x = min(x0 + j, W - 1);                            // (a tail lane recomputes the last pixel and stores nothing)
        const size_t p = (size_t)y * W + x;
        const float g0 = gt[p], g1 = gt[HW + p], g2 = gt[2 * HW + p];
        const float r0 = render[p], r1 = render[HW + p], r2 = render[2 * HW + p];
        float e[3];
#pragma unroll
        for (int c = 0; c < 3; c++) e[c] = ((r0 * A[c] + r1 * A[3 + c]) + r2 * A[6 + c]) + B[c];
        px[0][j] = color_px(g0, g1, g2);
        px[1][j] = color_px(r0, r1, r2);
        px[2][j] = color_px(fabsf(g0 - e[0]) * 10.f, fabsf(g1 - e[1]) * 10.f, fabsf(g2 - e[2]) * 10.f);
        const float gd = gt_depth[p], d = depth[p];
        px[3][j] = turbo_px(gd, r_gtd);
        px[4][j] = turbo_px(d, r_d);
        px[5][j] = turbo_px(fabsf(gd - d), r_diff);
        px[6][j] = normal_px(normal[p], normal[HW + p], normal[2 * HW + p]);
        float n[3];
        depth_normal(depth, x, y, H, W, fx, fy, cx, cy, n);
        px[7][j] = normal_px(n[0], n[1], n[2]);
        px[8][j] = turbo_px(alpha[p] > 0.5f ? 1.f : 0.f, r_mask);
    }
#pragma unroll
    for (int cell = 0; cell < 9; cell++) {
        const int row = cell / 3, col = cell - 3 * row;
        unsigned char* dst = out + (((size_t)(row * H + y)) * (3 * W) + (size_t)col * W + x0) * 3;
        store_px(dst, px[cell], count, wide);
    }
}

// layer 0: rgb of src [3,H,W]; 1: turbo of src [H,W]; 2: (src [3,H,W] + 1) / 2
__global__ __launch_bounds__(256) void frame_kernel(const float* __restrict__ src, int layer, int H, int W, const unsigned* __restrict__ ranges,
                                                    float lo, float hi, unsigned char* __restrict__ out, bool wide) {
    const int groups = (W + PANEL_PIX - 1) / PANEL_PIX;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= groups * H) return;
    const int y = t / groups, x0 = (t - y * groups) * PANEL_PIX;
    const int count = min(PANEL_PIX, W - x0);
    const size_t HW = (size_t)H * W;
    Range r = {0.f, 1.f};
    if (layer == 1) r = ranges ? load_range(ranges, 0) : fixed_range(lo, hi);
    unsigned px[PANEL_PIX];
#pragma unroll
    for (int j = 0; j < PANEL_PIX; j++) {
        const size_t p = (size_t)y * W + min(x0 + j, W - 1);
        if (layer == 1)
            px[j] = turbo_px(src[p], r);
        else if (layer == 0)
            px[j] = color_px(src[p], src[HW + p], src[2 * HW + p]);
        else
            px[j] = normal_px(src[p], src[HW + p], src[2 * HW + p]);
    }
    store_px(out + ((size_t)y * W + x0) * 3, px, count, wide);
}

constexpr long long PANEL_MAX_PIXELS = (1ll << 31) / 32;  // 27 H W bytes of a panel and 4 H W pixel indices stay below 2^31

}  // namespace

extern "C" int cut3r_gs_panel_ranges(const float* a, const float* b, const float* alpha, long long n, unsigned int* ranges, void* stream) {
    if (!ranges || (!a && !b && !alpha) || n < 1 || n >= PANEL_MAX_PIXELS) return CUT3R_ERR_ARG;
    if (hipMemsetAsync(ranges, 0, 2 * RANGE_SLOTS * sizeof(unsigned), (hipStream_t)stream) != hipSuccess) return CUT3R_ERR_LAUNCH;
    const int nblk = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(panel_ranges_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, a, b, alpha, (int)n, ranges);
    return cut3r_check_launch();
}

extern "C" int cut3r_gs_panel(const float* gt, const float* render, const float* exposure_a, const float* exposure_b, const float* gt_depth,
                              const float* depth, const float* normal, const float* alpha, float fx, float fy, float cx, float cy, int H, int W,
                              const unsigned int* ranges, unsigned char* out, void* stream) {
    if (!gt || !render || !exposure_a || !exposure_b || !gt_depth || !depth || !normal || !alpha || !ranges || !out) return CUT3R_ERR_ARG;
    if (H < 1 || W < 1 || (long long)H * W >= PANEL_MAX_PIXELS) return CUT3R_ERR_ARG;
    if (!(fx != 0.f) || !(fy != 0.f)) return CUT3R_ERR_ARG;
    const bool wide = W % 4 == 0 && ((uintptr_t)out & 3) == 0;
    const long long threads = (long long)((W + PANEL_PIX - 1) / PANEL_PIX) * H;
    hipLaunchKernelGGL(panel_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gt, render, exposure_a,
                       exposure_b, gt_depth, depth, normal, alpha, fx, fy, cx, cy, H, W, ranges, out, wide);
    return cut3r_check_launch();
}

extern "C" int cut3r_gs_frame(const float* src, int layer, int H, int W, const unsigned int* ranges, float lo, float hi, unsigned char* out,
                              void* stream) {
    if (!src || !out || layer < 0 || layer > 2) return CUT3R_ERR_ARG;
    if (H < 1 || W < 1 || (long long)H * W >= PANEL_MAX_PIXELS) return CUT3R_ERR_ARG;
    const bool wide = W % 4 == 0 && ((uintptr_t)out & 3) == 0;
    const long long threads = (long long)((W + PANEL_PIX - 1) / PANEL_PIX) * H;
    hipLaunchKernelGGL(frame_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, layer, H, W, ranges, lo, hi,
                       out, wide);
    return cut3r_check_launch();
}
