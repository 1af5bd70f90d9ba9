// What the voxel downsample of a point cloud (cloud.hip) and the vertex clustering of a mesh (mesh_clean.hip) share, so that a cluster of
// the mesh IS the voxel of the downsample, bit for bit, by construction: Open3D's voxel frame, the 63-bit key, the stable radix sort of
// (key, point index), the run heads and starts and the fp64 means in ascending point index, with their workspace layout and host driver.
// Both files are compiled with -ffp-contract=off; tests/cloud_oracle.py restates every operation in this order.
#pragma once
#include <cmath>
#include <hipcub/hipcub.hpp>
#include "common.h"
#include "../../include/cut3r_hip.h"

namespace {

constexpr int VOXEL_BITS = 21;                               // three indices in one 63-bit key
constexpr long long VOXEL_MAX_INDEX = (1ll << VOXEL_BITS) - 1;

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// for every thread of a 256-thread block: the number of flagged threads before it (threads in order), which is the rank of a flagged
// thread among the flagged ones; and the block's total
DEVINL unsigned block_rank(bool flag, unsigned* total) {
    __shared__ unsigned wtot[4];
    const unsigned long long m = __ballot(flag);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned r = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[w] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned base = 0, t = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < w) base += wtot[k];
        t += wtot[k];
    }
    __syncthreads();
    *total = t;
    return base + r;
}

struct VoxelFrame {
    double lo[3];                                            // (double)min - voxel / 2
    double voxel;
};

DEVINL unsigned long long voxel_index(float c, double lo, double voxel) {
    const double f = floor(((double)c - lo) / voxel);
    if (!(f >= 0.0)) return 0ull;                            // the host has refused such clouds; a key is never an address anyway
    if (f > (double)VOXEL_MAX_INDEX) return (unsigned long long)VOXEL_MAX_INDEX;
    return (unsigned long long)f;
}

__global__ __launch_bounds__(256) void voxel_key_kernel(const float* __restrict__ p, int N, const VoxelFrame fr, unsigned long long* __restrict__ keys,
                                                        unsigned* __restrict__ vals) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const unsigned long long ix = voxel_index(p[3 * i + 0], fr.lo[0], fr.voxel);
    const unsigned long long iy = voxel_index(p[3 * i + 1], fr.lo[1], fr.voxel);
    const unsigned long long iz = voxel_index(p[3 * i + 2], fr.lo[2], fr.voxel);
    keys[i] = (ix << (2 * VOXEL_BITS)) | (iy << VOXEL_BITS) | iz;
    vals[i] = (unsigned)i;
}

DEVINL bool voxel_head(const unsigned long long* __restrict__ keys, long long i, int N) {
    return i < N && (i == 0 || keys[i] != keys[i - 1]);
}

// bcount[blk] = run heads among the block's sorted keys; the entry after the last block is 0
__global__ __launch_bounds__(256) void voxel_heads_kernel(const unsigned long long* __restrict__ keys, int N, unsigned* __restrict__ bcount) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned total;
    (void)block_rank(voxel_head(keys, i, N), &total);
    if (threadIdx.x == 0) {
        bcount[blockIdx.x] = total;
        if (blockIdx.x == 0) bcount[gridDim.x] = 0;
    }
}

// starts[m] = sorted position of the first point of voxel m, starts[M] = N, *total = M
__global__ __launch_bounds__(256) void voxel_starts_kernel(const unsigned long long* __restrict__ keys, int N, const unsigned* __restrict__ offs,
                                                           unsigned* __restrict__ starts, long long* __restrict__ total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool head = voxel_head(keys, i, N);
    unsigned t;
    const unsigned r = block_rank(head, &t);
    if (head) starts[offs[blockIdx.x] + r] = (unsigned)i;
    if (i == (long long)N - 1) {
        starts[offs[gridDim.x]] = (unsigned)N;
        *total = (long long)offs[gridDim.x];
    }
}

// one thread per voxel: the fp64 sums of its points in ascending point index (the order the stable sort leaves), one add at a time
__global__ __launch_bounds__(256) void voxel_mean_kernel(const float* __restrict__ p, const unsigned char* __restrict__ col, int N,
                                                         const unsigned* __restrict__ starts, const unsigned* __restrict__ vals,
                                                         const unsigned* __restrict__ offs, int nblk, long long M, const int* __restrict__ dst,
                                                         long long cap, float* __restrict__ out, unsigned char* __restrict__ out_col,
                                                         int* __restrict__ out_cnt) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long Mtrue = (long long)offs[nblk];
    if (v >= M || v >= Mtrue) return;
    const long long m = dst ? (long long)dst[v] : v;          // the output row of voxel v (dst: a renumbering, < 0 = not written)
    if (m < 0 || m >= cap) return;
    const unsigned s = starts[v], e = min(starts[v + 1], (unsigned)N);
    double sx = 0.0, sy = 0.0, sz = 0.0, cr = 0.0, cg = 0.0, cb = 0.0;
    for (unsigned k = s; k < e; k++) {
        const unsigned i = vals[k];
        if (i >= (unsigned)N) continue;
        sx += (double)p[3 * (size_t)i + 0];
        sy += (double)p[3 * (size_t)i + 1];
        sz += (double)p[3 * (size_t)i + 2];
        if (col) {
            cr += (double)col[3 * (size_t)i + 0];
            cg += (double)col[3 * (size_t)i + 1];
            cb += (double)col[3 * (size_t)i + 2];
        }
    }
    const double n = (double)(e - s);
    out[3 * m + 0] = (float)(sx / n);
    out[3 * m + 1] = (float)(sy / n);
    out[3 * m + 2] = (float)(sz / n);
    if (col) {
        out_col[3 * m + 0] = (unsigned char)floor(cr / n + 0.5);
        out_col[3 * m + 1] = (unsigned char)floor(cg / n + 0.5);
        out_col[3 * m + 2] = (unsigned char)floor(cb / n + 0.5);
    }
    if (out_cnt) out_cnt[m] = (int)(e - s);
}

// keys_in (later: starts [N + 1] u32) | keys_out | vals_in | vals_out | bcount, offs [nblk + 1] | sort / scan scratch
struct VoxelLayout {
    int nblk;
    size_t keys_in, keys_out, vals_in, vals_out, bcount, offs, temp, sort_bytes, scan_bytes, total;
};

VoxelLayout voxel_layout(int N) {
    VoxelLayout L;
    L.nblk = (int)(((long long)N + 255) / 256);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align256(o + bytes); return r; };
    L.keys_in = take(8 * (size_t)N);
    L.keys_out = take(8 * (size_t)N);
    L.vals_in = take(4 * (size_t)N);
    L.vals_out = take(4 * (size_t)N);
    L.bcount = take(4 * ((size_t)L.nblk + 1));
    L.offs = take(4 * ((size_t)L.nblk + 1));
    L.sort_bytes = L.scan_bytes = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, L.sort_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned*)nullptr,
                                             (unsigned*)nullptr, N, 0, 3 * VOXEL_BITS, (hipStream_t)0);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, L.scan_bytes, (unsigned*)nullptr, (unsigned*)nullptr, L.nblk + 1, (hipStream_t)0);
    L.temp = take(L.sort_bytes > L.scan_bytes ? L.sort_bytes : L.scan_bytes);
    L.total = o;
    return L;
}

// the frame of HOST bounds lo, hi (fp32 [3]); false when the voxel or the bounds are refused (an index >= 2^21 included)
bool voxel_frame(double voxel, const float* lo, const float* hi, VoxelFrame* fr) {
    if (!(voxel > 0.0) || !std::isfinite(voxel)) return false;
    fr->voxel = voxel;
    for (int a = 0; a < 3; a++) {
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || hi[a] < lo[a]) return false;
        fr->lo[a] = (double)lo[a] - voxel * 0.5;
        const double top = std::floor(((double)hi[a] - fr->lo[a]) / voxel);
        if (!(top <= (double)VOXEL_MAX_INDEX)) return false;
    }
    return true;
}

// keys, stable sort, heads, scan, starts into the workspace w laid out by L = voxel_layout(N); *total = M (device)
int voxel_sort_runs(const float* points, int N, const VoxelFrame& fr, const VoxelLayout& L, char* w, long long* total, hipStream_t s) {
    unsigned long long* keys_in = (unsigned long long*)(w + L.keys_in);
    unsigned long long* keys_out = (unsigned long long*)(w + L.keys_out);
    unsigned* vals_in = (unsigned*)(w + L.vals_in);
    unsigned* vals_out = (unsigned*)(w + L.vals_out);
    unsigned* bcount = (unsigned*)(w + L.bcount);
    unsigned* offs = (unsigned*)(w + L.offs);
    hipLaunchKernelGGL(voxel_key_kernel, dim3(L.nblk), dim3(256), 0, s, points, N, fr, keys_in, vals_in);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    size_t tb = L.sort_bytes;
    if (hipcub::DeviceRadixSort::SortPairs(w + L.temp, tb, keys_in, keys_out, vals_in, vals_out, N, 0, 3 * VOXEL_BITS, s) != hipSuccess)
        return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(voxel_heads_kernel, dim3(L.nblk), dim3(256), 0, s, keys_out, N, bcount);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    tb = L.scan_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(w + L.temp, tb, bcount, offs, L.nblk + 1, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(voxel_starts_kernel, dim3(L.nblk), dim3(256), 0, s, keys_out, N, offs, (unsigned*)keys_in, total);
    return cut3r_check_launch();
}

// the means of the M voxels from the workspace voxel_sort_runs left; voxel v goes to row dst[v] (dst NULL: row v) when 0 <= row < cap
int voxel_means(const float* points, const unsigned char* colors, int N, const VoxelLayout& L, const char* w, float* out_points,
                unsigned char* out_colors, int* out_counts, long long M, const int* dst, long long cap, hipStream_t s) {
    hipLaunchKernelGGL(voxel_mean_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, s, points, colors, N, (const unsigned*)(w + L.keys_in),
                       (const unsigned*)(w + L.vals_out), (const unsigned*)(w + L.offs), L.nblk, M, dst, cap, out_points, out_colors, out_counts);
    return cut3r_check_launch();
}

}  // namespace
