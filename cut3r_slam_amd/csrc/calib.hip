// Focal length from the network's own self-view pointmaps (cut3r_slam_amd/self_calib.py): the two estimators of the reference's
// src/dust3r/post_process.py:estimate_focal_knowing_depth, "weiszfeld" (:38-55) and "median" (:27-36).  Compiled with -ffp-contract=off;
// tests/focal_oracle.py restates both, the Weiszfeld result bit for bit.
//
// Inputs of both: pts fp32 [B,H,W,3], pp fp32 [B,2] (one principal point per view), an optional confidence conf fp32 [B,H,W] (a pixel with
// conf < conf_min takes no part; NULL = no gate).  Pixel p = row W + col of view b has u = float(col) - ppx, v = float(row) - ppy.
//
// Weiszfeld, per pixel in fp32 with every operation rounded on its own:
//     xz = x / z, yz = y / z, each replaced by 0 when it is not finite;  a = xz u + yz v;  b = xz xz + yz yz
//     start:      f = float(double(sum a) / double(sum b))
//     iteration:  du = u - f xz, dv = v - f yz, dis = sqrtf(du du + dv dv), w = 1 / fmaxf(dis, 1e-8f)
//                 f = float(double(sum fl32(w a)) / double(sum fl32(w b)))
// (the reference divides the two means; the pixel count cancels).  The sums are fp64 in ONE fixed order: G = 16 workgroups per view, workgroup g
// owns the row-major pixels [g C, min(HW, (g + 1) C)) with C = ceil(HW / G); its thread t (of 256) adds the pixels g C + t, g C + t + 256, ...
// in increasing order, starting from +0; the 256 thread sums are folded by the halving tree s[t] += s[t + o], o = 128, 64, ..., 1; the G
// workgroup sums are then added in increasing g, starting from +0.  A gated pixel adds nothing.
// Launch scheme: one launch of B x G workgroups for the start and one per iteration; every workgroup of a launch first re-adds the G
// partial pairs the previous launch left in the workspace (redundant, deterministic) to get f, so nothing waits for another workgroup and
// nothing is read back; a last launch of B threads writes focal.  iters + 2 dependent launches, no atomics.  A view without a
// participating pixel, or with sum b == 0, yields NaN.
//
// Median: the votes fx = (u z) / x and fy = (v z) / y (product rounded, IEEE division) of every participating pixel, 2 HW per view; NaN
// votes are void, +-inf votes take part.  The result is the vote of rank (n - 1) / 2 in ascending order of the n non-void votes (what
// torch.nanmedian returns), NaN when n == 0.  It is found by a radix select over the order-preserving uint32 image of the float (sign bit
// set for positives, all bits flipped for negatives), most significant 8-bit digit first: a pass counts, in LDS and then with integer
// atomicAdd into the view's 256-bin table of that pass, the digit of every vote whose higher digits are the chosen ones; the next pass
// (every workgroup, redundantly) finds the chosen bin of the previous tables by a scan.  Integer counts are exact in any arrival order.
// One memset, four passes of B x G workgroups, one launch of B workgroups that writes focal.  Nothing is sorted.
#include "common.h"
#include "cut3r_hip.h"

namespace {

constexpr int G = 16;            // workgroups per view
constexpr int T = 256;           // threads per workgroup

struct Layout {                  // of the workspace
    long long partial_bytes, table_bytes;
};

Layout layout_of(int B) {
    Layout l;
    l.partial_bytes = (long long)B * G * 2 * 2 * (long long)sizeof(double);      // two buffers [B,G,2]: a launch reads one and writes the other
    l.table_bytes = (long long)B * 4 * 256 * (long long)sizeof(unsigned);         // four 256-bin tables per view
    return l;
}

bool sizes_ok(int B, int H, int W) {
    if (B < 1 || B > (1 << 24) || H < 1 || W < 1) return false;
    return 2ll * H * W < (1ll << 31);
}

DEVINL float finite_or_zero(float v) { return __builtin_isfinite(v) ? v : 0.0f; }

// ---------------------------------------------------------------------------------------------------------------------- Weiszfeld
// prev == NULL: the unweighted start.  prev, out: [B,G,2] (sum a, sum b)
__global__ __launch_bounds__(T) void weiszfeld_kernel(const float* __restrict__ pts, const float* __restrict__ conf, float conf_min,
                                                      const float* __restrict__ pp, int HW, int W, int chunk,
                                                      const double* __restrict__ prev, double* __restrict__ out) {
    __shared__ double sa[T], sb[T];
    const int b = blockIdx.x / G, g = blockIdx.x % G, t = threadIdx.x;
    const bool weighted = prev != nullptr;
    float f = 0.0f;
    if (weighted) {
        double A = 0.0, Bs = 0.0;
        for (int k = 0; k < G; k++) {
            A += prev[((long long)b * G + k) * 2];
            Bs += prev[((long long)b * G + k) * 2 + 1];
        }
        f = (float)(A / Bs);
    }
    const float ppx = pp[2 * b], ppy = pp[2 * b + 1];
    const int lo = g * chunk, hi = min(HW, lo + chunk);
    double A = 0.0, Bs = 0.0;
    for (int p = lo + t; p < hi; p += T) {
        const long long i = (long long)b * HW + p;
        if (conf != nullptr && conf[i] < conf_min) continue;
        const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const float xz = finite_or_zero(x / z), yz = finite_or_zero(y / z);
        const int row = p / W, col = p - row * W;
        const float u = (float)col - ppx, v = (float)row - ppy;
        float a = xz * u + yz * v;
        float bb = xz * xz + yz * yz;
        if (weighted) {
            const float du = u - f * xz, dv = v - f * yz;
            const float dis = sqrtf(du * du + dv * dv);
            const float w = 1.0f / fmaxf(dis, 1e-8f);
            a = w * a;
            bb = w * bb;
        }
        A += (double)a;
        Bs += (double)bb;
    }
    sa[t] = A;
    sb[t] = Bs;
    __syncthreads();
    for (int o = T / 2; o > 0; o >>= 1) {
        if (t < o) {
            sa[t] += sa[t + o];
            sb[t] += sb[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[((long long)b * G + g) * 2] = sa[0];
        out[((long long)b * G + g) * 2 + 1] = sb[0];
    }
}

__global__ __launch_bounds__(T) void weiszfeld_final_kernel(const double* __restrict__ prev, int B, float* __restrict__ focal) {
    const int b = blockIdx.x * T + threadIdx.x;
    if (b >= B) return;
    double A = 0.0, Bs = 0.0;
    for (int k = 0; k < G; k++) {
        A += prev[((long long)b * G + k) * 2];
        Bs += prev[((long long)b * G + k) * 2 + 1];
    }
    focal[b] = Bs == 0.0 ? __builtin_nanf("") : (float)(A / Bs);
}

// ------------------------------------------------------------------------------------------------------------------------- median
DEVINL unsigned key_of(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

DEVINL float value_of(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// The state in front of pass `pass` from the tables of the passes before it (tab: the view's [4][256]): prefix = the chosen digits in the top
// 8 pass bits, rank = the rank of the wanted vote among those that carry the prefix, n = the non-void votes of the view.  All T threads call
// it and all get the same values; s [T + 2] is scratch.
DEVINL void select_state(const unsigned* __restrict__ tab, int pass, unsigned* s, unsigned& prefix, unsigned& rank, unsigned& n) {
    const int t = threadIdx.x;
    prefix = 0, rank = 0, n = 0;
    for (int j = 0; j < pass; j++) {
        const unsigned c = tab[j * 256 + t];
        __syncthreads();
        s[t] = c;
        if (t == 0) s[T] = 0, s[T + 1] = 0;
        __syncthreads();
        for (int o = 1; o < T; o <<= 1) {                  // inclusive scan
            const unsigned add = t >= o ? s[t - o] : 0u;
            __syncthreads();
            s[t] += add;
            __syncthreads();
        }
        const unsigned inc = s[t], total = s[T - 1];
        if (j == 0) {
            n = total;
            rank = n > 0 ? (n - 1) / 2 : 0;
        }
        if (total > 0 && inc - c <= rank && rank < inc) s[T] = (unsigned)t, s[T + 1] = rank - (inc - c);
        __syncthreads();
        prefix |= s[T] << (24 - 8 * j);
        rank = s[T + 1];
    }
    __syncthreads();
}

__global__ __launch_bounds__(T) void median_pass_kernel(const float* __restrict__ pts, const float* __restrict__ conf, float conf_min,
                                                        const float* __restrict__ pp, int HW, int W, int chunk, int pass,
                                                        unsigned* __restrict__ tables) {
    __shared__ unsigned hist[256];
    __shared__ unsigned scratch[T + 2];
    const int b = blockIdx.x / G, g = blockIdx.x % G, t = threadIdx.x;
    unsigned* tab = tables + (long long)b * 4 * 256;
    unsigned prefix, rank, n;
    select_state(tab, pass, scratch, prefix, rank, n);
    if (pass > 0 && n == 0) return;
    hist[t] = 0;
    __syncthreads();
    const float ppx = pp[2 * b], ppy = pp[2 * b + 1];
    const int lo = g * chunk, hi = min(HW, lo + chunk);
    const int high = 32 - 8 * pass, shift = 24 - 8 * pass;       // bits above the digit of this pass are [high, 32)
    for (int p = lo + t; p < hi; p += T) {
        const long long i = (long long)b * HW + p;
        if (conf != nullptr && conf[i] < conf_min) continue;
        const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const int row = p / W, col = p - row * W;
        const float u = (float)col - ppx, v = (float)row - ppy;
        const float vote[2] = {(u * z) / x, (v * z) / y};
#pragma unroll
        for (int k = 0; k < 2; k++) {
            if (vote[k] != vote[k]) continue;
            const unsigned key = key_of(vote[k]);
            if (pass == 0 || (key >> high) == (prefix >> high)) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    if (hist[t] != 0) atomicAdd(&tab[pass * 256 + t], hist[t]);
}

__global__ __launch_bounds__(T) void median_final_kernel(const unsigned* __restrict__ tables, float* __restrict__ focal) {
    __shared__ unsigned scratch[T + 2];
    const int b = blockIdx.x;
    unsigned prefix, rank, n;
    select_state(tables + (long long)b * 4 * 256, 4, scratch, prefix, rank, n);
    if (threadIdx.x == 0) focal[b] = n == 0 ? __builtin_nanf("") : value_of(prefix);
}

int check_args(const float* pts, const float* pp, int B, int H, int W, const float* focal, const void* ws, long long ws_bytes) {
    if (!pts || !pp || !focal || !ws || !sizes_ok(B, H, W)) return CUT3R_ERR_ARG;
    if (((uintptr_t)ws & 7u) != 0 || ws_bytes < cut3r_focal_workspace_bytes(B, H, W)) return CUT3R_ERR_ARG;
    return CUT3R_OK;
}

}  // namespace

extern "C" long long cut3r_focal_workspace_bytes(int B, int H, int W) {
    if (!sizes_ok(B, H, W)) return -1;
    const Layout l = layout_of(B);
    return l.partial_bytes + l.table_bytes;
}

extern "C" int cut3r_focal_weiszfeld(const float* pts, const float* conf, float conf_min, const float* pp, int B, int H, int W, int iters,
                                     float* focal, void* ws, long long ws_bytes, void* stream) {
    if (check_args(pts, pp, B, H, W, focal, ws, ws_bytes) != CUT3R_OK || iters < 0) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int HW = H * W, chunk = (HW + G - 1) / G;
    double* buf[2] = {(double*)ws, (double*)ws + (long long)B * G * 2};
    for (int k = 0; k <= iters; k++) {
        hipLaunchKernelGGL(weiszfeld_kernel, dim3(B * G), dim3(T), 0, s, pts, conf, conf_min, pp, HW, W, chunk,
                           k == 0 ? (const double*)nullptr : (const double*)buf[(k - 1) & 1], buf[k & 1]);
        if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(weiszfeld_final_kernel, dim3((B + T - 1) / T), dim3(T), 0, s, (const double*)buf[iters & 1], B, focal);
    return cut3r_check_launch();
}

extern "C" int cut3r_focal_median(const float* pts, const float* conf, float conf_min, const float* pp, int B, int H, int W, float* focal,
                                  void* ws, long long ws_bytes, void* stream) {
    if (check_args(pts, pp, B, H, W, focal, ws, ws_bytes) != CUT3R_OK) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const Layout l = layout_of(B);
    const int HW = H * W, chunk = (HW + G - 1) / G;
    unsigned* tables = (unsigned*)((char*)ws + l.partial_bytes);
    if (hipMemsetAsync(tables, 0, (size_t)l.table_bytes, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    for (int pass = 0; pass < 4; pass++) {
        hipLaunchKernelGGL(median_pass_kernel, dim3(B * G), dim3(T), 0, s, pts, conf, conf_min, pp, HW, W, chunk, pass, tables);
        if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(median_final_kernel, dim3(B), dim3(T), 0, s, (const unsigned*)tables, focal);
    return cut3r_check_launch();
}
