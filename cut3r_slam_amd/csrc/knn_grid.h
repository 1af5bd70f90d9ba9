// Uniform-grid binning of a point set for exact nearest-neighbour searches (gs.hip: the 3-NN of simple_knn.distCUDA2; recon.hip: the
// 1-NN of the reconstruction metrics and ICP).  Builds the ROBUST bounding box of the points, a cubic-cell grid over it and a counting
// sort of the points by cell; the searches themselves live with their callers.  Everything here is in an anonymous namespace: each
// translation unit that includes it gets its own copy of the kernels.
#pragma once
#include <hipcub/hipcub.hpp>
#include "common.h"

namespace {

// The grid: cell edge = longest extent of the robust box / G, G ~ sqrt(P) / 2 capped at 160 (pointmaps and mesh samples are surfaces,
// so an occupied cell then holds a few tens of points).
struct KnnHdr { float minx, miny, minz, cs, inv_cs; int gx, gy, gz; };

DEVINL unsigned knn_enc(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }     // order-preserving
DEVINL float knn_dec(unsigned e) { return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

// bb[0..5]: order-preserving encodings of the per-axis minima / maxima; mom[0..5] (floats behind them): per-axis sum and sum of squares
// RELATIVE TO POINT 0 (so that the squares stay small for a map far from the origin)
__global__ __launch_bounds__(256) void knn_bbox_kernel(const float* __restrict__ pts, int P, unsigned* __restrict__ bb) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    float lo[3] = {3.4e38f, 3.4e38f, 3.4e38f}, hi[3] = {-3.4e38f, -3.4e38f, -3.4e38f}, d[3] = {0.f, 0.f, 0.f};
    if (i < P) {
#pragma unroll
        for (int a = 0; a < 3; a++) { lo[a] = hi[a] = pts[3 * (size_t)i + a]; d[a] = lo[a] - pts[a]; }
    }
    float* mom = reinterpret_cast<float*>(bb + 6);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        float l = lo[a], h = hi[a], s1 = d[a], s2 = d[a] * d[a];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            l = fminf(l, __shfl_xor(l, o, 64)); h = fmaxf(h, __shfl_xor(h, o, 64));
            s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64);
        }
        if ((threadIdx.x & 63) == 0) { atomicMin(bb + a, knn_enc(l)); atomicMax(bb + 3 + a, knn_enc(h)); atomicAdd(mom + a, s1); atomicAdd(mom + 3 + a, s2); }
    }
}

// second moment pass: only the points inside the first pass's box count (bb[12..17]: its lo / hi as floats; mom2 = bb[18..23], count bb[24]).
// Ten outliers at 100 x the extent among 2e5 surface points triple sigma by themselves; trimmed to the first box, sigma is the surface's.
__global__ __launch_bounds__(256) void knn_trim_kernel(const float* __restrict__ pts, int P, unsigned* __restrict__ bb) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float* box = reinterpret_cast<const float*>(bb + 12);
    float d[3] = {0.f, 0.f, 0.f};
    bool in = i < P;
    if (i < P) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float x = pts[3 * (size_t)i + a];
            in = in && x >= box[a] && x <= box[3 + a];
            d[a] = x - pts[a];
        }
    }
    float* mom = reinterpret_cast<float*>(bb + 18);
    const float c = in ? 1.f : 0.f;
    float cnt = c;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
#pragma unroll
    for (int a = 0; a < 3; a++) {
        float s1 = c * d[a], s2 = c * d[a] * d[a];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
        if ((threadIdx.x & 63) == 0) { atomicAdd(mom + a, s1); atomicAdd(mom + 3 + a, s2); }
    }
    if ((threadIdx.x & 63) == 0) atomicAdd(mom + 6, cnt);
}

// The grid covers the ROBUST box: per axis [mean - 3 sigma, mean + 3 sigma] intersected with the true bounding box.  A few far outliers
// (sky / far-depth pixels with conf > 0) would otherwise stretch the box, the surface would fall into a handful of cells and every thread
// of the query kernel would scan them serially (O(P^2) from global memory).  Points outside the grid are clamped into its border cells
// (knn_cell) or, when the caller asks for it, binned into one extra cell of their own (knn_count_kernel); either way the searches stay
// EXACT -- the statistics only steer the speed, which is why their atomic summation order does not matter.
// pass 0: box from the moments of ALL points -> bb[12..17] (read by knn_trim_kernel); pass 1: box from the trimmed moments -> the header
__global__ void knn_header_kernel(unsigned* __restrict__ bb, const float* __restrict__ pts, int P, int G, KnnHdr* __restrict__ hdr, int pass) {
    if (threadIdx.x != 0) return;
    const float* mom = reinterpret_cast<const float*>(bb + (pass == 0 ? 6 : 18));
    const float n = pass == 0 ? (float)P : fmaxf(mom[6], 1.f);
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float mean_d = mom[a] / n;
        const float var = fmaxf(mom[3 + a] / n - mean_d * mean_d, 0.f);
        const float mu = pts[a] + mean_d, sg = sqrtf(var);
        lo[a] = fmaxf(knn_dec(bb[a]), mu - 3.f * sg);
        hi[a] = fminf(knn_dec(bb[3 + a]), mu + 3.f * sg);
        if (!(hi[a] >= lo[a])) { lo[a] = knn_dec(bb[a]); hi[a] = knn_dec(bb[3 + a]); }
    }
    if (pass == 0) {
        float* box = reinterpret_cast<float*>(bb + 12);
#pragma unroll
        for (int a = 0; a < 3; a++) { box[a] = lo[a]; box[3 + a] = hi[a]; }
        return;
    }
    const float lx = lo[0], ly = lo[1], lz = lo[2];
    const float ex = hi[0] - lx, ey = hi[1] - ly, ez = hi[2] - lz;
    float cs = fmaxf(ex, fmaxf(ey, ez)) / (float)G;
    if (!(cs > 0.f)) cs = 1.f;                                   // all points identical
    KnnHdr h;
    h.minx = lx; h.miny = ly; h.minz = lz; h.cs = cs; h.inv_cs = 1.0f / cs;
    h.gx = min(G + 1, (int)(ex * h.inv_cs) + 1); h.gy = min(G + 1, (int)(ey * h.inv_cs) + 1); h.gz = min(G + 1, (int)(ez * h.inv_cs) + 1);
    *hdr = h;
}

DEVINL void knn_cell(const KnnHdr& h, float x, float y, float z, int& cx, int& cy, int& cz) {
    cx = min(h.gx - 1, max(0, (int)((x - h.minx) * h.inv_cs)));
    cy = min(h.gy - 1, max(0, (int)((y - h.miny) * h.inv_cs)));
    cz = min(h.gz - 1, max(0, (int)((z - h.minz) * h.inv_cs)));
}

// the closed box the cells tile, [min, min + g * cs] per axis; every caller in one translation unit evaluates it with this one expression
DEVINL void knn_box_hi(const KnnHdr& h, float& hx, float& hy, float& hz) {
    hx = h.minx + (float)h.gx * h.cs;
    hy = h.miny + (float)h.gy * h.cs;
    hz = h.minz + (float)h.gz * h.cs;
}

// split_outside = 0: every point is clamped into a cell.  1: a point outside the closed box of knn_box_hi goes to the extra cell
// gx*gy*gz (its count follows the grid's in `counts`, its run follows the grid's in the sorted order).
__global__ __launch_bounds__(256) void knn_count_kernel(const float* __restrict__ pts, int P, const KnnHdr* __restrict__ hdr, int* __restrict__ cell_of,
                                                        unsigned* __restrict__ counts, int split_outside) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const KnnHdr h = *hdr;
    const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
    int c;
    float hx, hy, hz;
    knn_box_hi(h, hx, hy, hz);
    if (split_outside && !(x >= h.minx && x <= hx && y >= h.miny && y <= hy && z >= h.minz && z <= hz)) {
        c = h.gx * h.gy * h.gz;
    } else {
        int cx, cy, cz;
        knn_cell(h, x, y, z, cx, cy, cz);
        c = (cz * h.gy + cy) * h.gx + cx;
    }
    cell_of[i] = c;
    atomicAdd(counts + c, 1u);
}

__global__ __launch_bounds__(256) void knn_scatter_kernel(const float* __restrict__ pts, int P, const int* __restrict__ cell_of,
                                                          const unsigned* __restrict__ starts, unsigned* __restrict__ cursor,
                                                          float* __restrict__ spts, int* __restrict__ sidx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int c = cell_of[i];
    const unsigned pos = starts[c] + atomicAdd(cursor + c, 1u);
    spts[3 * (size_t)pos] = pts[3 * (size_t)i]; spts[3 * (size_t)pos + 1] = pts[3 * (size_t)i + 1]; spts[3 * (size_t)pos + 2] = pts[3 * (size_t)i + 2];
    sidx[pos] = i;
}

int knn3_grid_G(int P) {
    int G = (int)ceil(sqrt((double)P) / 2.0);
    return G < 8 ? 8 : (G > 160 ? 160 : G);
}

// The whole construction.  hdr: 64 B; bb: 25 words; cell_of [P]; counts / starts [nscan] (nscan = cells + 1, + 1 more with split_outside);
// cursor [nscan - 1]; spts [P,3]; sidx [P].  starts[c] .. starts[c + 1] is cell c's run of (spts, sidx).
int knn_grid_build(const float* pts, int P, int G, KnnHdr* hdr, unsigned* bb, int* cell_of, unsigned* counts, unsigned* starts, unsigned* cursor,
                   float* spts, int* sidx, long long nscan, int split_outside, void* scan_ws, size_t scan_bytes, hipStream_t s) {
    if (hipMemsetAsync(bb, 0xFF, 3 * sizeof(unsigned), s) != hipSuccess) return CUT3R_ERR_LAUNCH;          // encoded minima start at the top
    if (hipMemsetAsync(bb + 3, 0, 22 * sizeof(unsigned), s) != hipSuccess) return CUT3R_ERR_LAUNCH;         // maxima, moments, first box, trimmed moments + count
    if (hipMemsetAsync(counts, 0, sizeof(unsigned) * (size_t)nscan, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    if (hipMemsetAsync(cursor, 0, sizeof(unsigned) * (size_t)(nscan - 1), s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    const unsigned nb = (unsigned)((P + 255) / 256);
    hipLaunchKernelGGL(knn_bbox_kernel, dim3(nb), dim3(256), 0, s, pts, P, bb);
    hipLaunchKernelGGL(knn_header_kernel, dim3(1), dim3(64), 0, s, bb, pts, P, G, hdr, 0);
    hipLaunchKernelGGL(knn_trim_kernel, dim3(nb), dim3(256), 0, s, pts, P, bb);
    hipLaunchKernelGGL(knn_header_kernel, dim3(1), dim3(64), 0, s, bb, pts, P, G, hdr, 1);
    hipLaunchKernelGGL(knn_count_kernel, dim3(nb), dim3(256), 0, s, pts, P, hdr, cell_of, counts, split_outside);
    if (hipcub::DeviceScan::ExclusiveSum(scan_ws, scan_bytes, counts, starts, (int)nscan, s) != hipSuccess) return CUT3R_ERR_ARG;
    hipLaunchKernelGGL(knn_scatter_kernel, dim3(nb), dim3(256), 0, s, pts, P, cell_of, starts, cursor, spts, sidx);
    return cut3r_check_launch();
}

}  // namespace
