// Dense point clouds for the depth-map evaluation (cut3r_slam_amd/eval_dense.py, the reference's scripts/eval7_scenes_dense.py): depth maps
// -> one world point cloud (Open3D create_from_rgbd_image + transform), and Open3D's PointCloud.voxel_down_sample.  Compiled with
// -ffp-contract=off: tests/cloud_oracle.py restates every operation in this order and the results are compared bit for bit.
//
// Both are count -> scan -> emit compactions: a block counts its valid items, hipcub scans the block counts, the block recomputes the
// flags and writes each item at (block offset + rank inside the block).  No atomic decides a position, so the output order is the input
// order and every run gives the same bits.
#include <hipcub/hipcub.hpp>
#include "common.h"
#include "../../include/cut3r_hip.h"

namespace {

constexpr int CLOUD_MAX_VIEWS = 16;
constexpr int VOXEL_BITS = 21;                               // three indices in one 63-bit key
constexpr long long VOXEL_MAX_INDEX = (1ll << VOXEL_BITS) - 1;
constexpr int BOUNDS_MAX_BLOCKS = 1024;

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// rank of a flagged thread among the flagged threads of its 256-thread block (threads in order), and the block's total
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

// ------------------------------------------------------------------------------------------------------------- depth maps -> cloud
struct CloudViews {
    double c2w[CLOUD_MAX_VIEWS][12];
    double K[CLOUD_MAX_VIEWS][4];
};

// grid pixel (i, j) of the H1 x W1 sampling grid reads source pixel (min(i H / H1, H - 1), min(j W / W1, W - 1)): the exact floor
DEVINL size_t cloud_src(int i, int j, int H, int W, int H1, int W1) {
    const int si = min((int)((long long)i * H / H1), H - 1);
    const int sj = min((int)((long long)j * W / W1), W - 1);
    return (size_t)si * W + sj;
}

DEVINL bool cloud_valid(float d, float trunc) { return isfinite(d) && d > 0.f && d < trunc; }

// grid (ceil(H1 W1 / 256), B): bcount[b * gridDim.x + blockIdx.x] = valid pixels of the block; the entry after the last block is 0
__global__ __launch_bounds__(256) void cloud_count_kernel(const float* __restrict__ depth, int H, int W, int H1, int W1, float trunc,
                                                          unsigned* __restrict__ bcount) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    bool valid = false;
    if (p < H1 * W1) valid = cloud_valid(depth[(size_t)b * H * W + cloud_src(p / W1, p % W1, H, W, H1, W1)], trunc);
    unsigned total;
    (void)block_rank(valid, &total);
    if (threadIdx.x == 0) {
        bcount[(size_t)b * gridDim.x + blockIdx.x] = total;
        if (b == 0 && blockIdx.x == 0) bcount[(size_t)gridDim.x * gridDim.y] = 0;
    }
}

__global__ void cloud_view_counts_kernel(const unsigned* __restrict__ offs, int B, int nblk, long long* __restrict__ counts) {
    const int b = threadIdx.x;
    if (b < B) counts[b] = (long long)offs[(size_t)(b + 1) * nblk] - (long long)offs[(size_t)b * nblk];
}

__global__ __launch_bounds__(256) void cloud_emit_kernel(const float* __restrict__ depth, const unsigned char* __restrict__ rgb, int H, int W,
                                                         int H1, int W1, float trunc, const CloudViews v, const unsigned* __restrict__ offs,
                                                         long long n, float* __restrict__ points, unsigned char* __restrict__ colors) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    bool valid = false;
    float d = 0.f;
    size_t src = 0;
    int i = 0, j = 0;
    if (p < H1 * W1) {
        i = p / W1;
        j = p % W1;
        src = cloud_src(i, j, H, W, H1, W1);
        d = depth[(size_t)b * H * W + src];
        valid = cloud_valid(d, trunc);
    }
    unsigned total;
    const unsigned r = block_rank(valid, &total);
    if (!valid) return;
    const long long pos = (long long)offs[(size_t)b * gridDim.x + blockIdx.x] + r;
    if (pos >= n) return;                                    // cannot happen with the workspace of the count; never write past the output
    const double* T = v.c2w[b];
    const double fx = v.K[b][0], fy = v.K[b][1], cx = v.K[b][2], cy = v.K[b][3];
    const double z = (double)d;
    const double x = ((double)j - cx) * z / fx;
    const double y = ((double)i - cy) * z / fy;
    points[3 * pos + 0] = (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);
    points[3 * pos + 1] = (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
    points[3 * pos + 2] = (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
    if (colors) {
        const size_t plane = (size_t)H * W;
        const unsigned char* c = rgb + (size_t)b * 3 * plane + src;
        colors[3 * pos + 0] = c[0];
        colors[3 * pos + 1] = c[plane];
        colors[3 * pos + 2] = c[2 * plane];
    }
}

struct CloudLayout {
    int nblk;
    size_t nscan, bcount, offs, scan, scan_bytes, total;
};

bool cloud_sizes_ok(int B, int H, int W, int H1, int W1) {
    if (B < 1 || B > CLOUD_MAX_VIEWS || H <= 0 || W <= 0 || H1 <= 0 || W1 <= 0) return false;
    return (long long)H * W < (1ll << 31) / CLOUD_MAX_VIEWS && (long long)H1 * W1 < (1ll << 31) / CLOUD_MAX_VIEWS;
}

CloudLayout cloud_layout(int B, int H1, int W1) {
    CloudLayout L;
    L.nblk = (int)(((long long)H1 * W1 + 255) / 256);
    L.nscan = (size_t)B * L.nblk + 1;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align256(o + bytes); return r; };
    L.bcount = take(4 * L.nscan);
    L.offs = take(4 * L.nscan);
    L.scan_bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, L.scan_bytes, (unsigned*)nullptr, (unsigned*)nullptr, (int)L.nscan, (hipStream_t)0);
    L.scan = take(L.scan_bytes);
    L.total = o;
    return L;
}

// ---------------------------------------------------------------------------------------------------------------- voxel downsample
DEVINL float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// part[blk][7] = min xyz, max xyz over the finite coordinates of the block's points, and 1 when one coordinate is not finite
__global__ __launch_bounds__(256) void cloud_bounds_kernel(const float* __restrict__ p, int N, float* __restrict__ part) {
    float v[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.f};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < N; i += (long long)gridDim.x * 256) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float c = p[3 * i + a];
            if (isfinite(c)) {
                v[a] = fminf(v[a], c);
                v[3 + a] = fmaxf(v[3 + a], c);
            } else {
                v[6] = 1.f;
            }
        }
    }
    __shared__ float sh[4][7];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 7; a++) {
        const float r = a < 3 ? wave_min(v[a]) : wave_max(v[a]);
        if (lane == 0) sh[w][a] = r;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int a = threadIdx.x;
        float r = sh[0][a];
        for (int k = 1; k < 4; k++) r = a < 3 ? fminf(r, sh[k][a]) : fmaxf(r, sh[k][a]);
        part[(size_t)blockIdx.x * 7 + a] = r;
    }
}

__global__ void cloud_bounds_fold_kernel(const float* __restrict__ part, int nblk, float* __restrict__ out) {
    const int a = threadIdx.x;
    if (a >= 7) return;
    float r = part[a];
    for (int k = 1; k < nblk; k++) r = a < 3 ? fminf(r, part[(size_t)k * 7 + a]) : fmaxf(r, part[(size_t)k * 7 + a]);
    out[a] = r;
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
                                                         const unsigned* __restrict__ offs, int nblk, long long M, float* __restrict__ out,
                                                         unsigned char* __restrict__ out_col, int* __restrict__ out_cnt) {
    const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long Mtrue = (long long)offs[nblk];
    if (m >= M || m >= Mtrue) return;
    const unsigned s = starts[m], e = min(starts[m + 1], (unsigned)N);
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
    out_cnt[m] = (int)(e - s);
}

int bounds_blocks(int N) {
    const long long g = ((long long)N + 255) / 256;
    return (int)(g < BOUNDS_MAX_BLOCKS ? g : BOUNDS_MAX_BLOCKS);
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

bool finite_all(const double* v, int n) {
    for (int k = 0; k < n; k++)
        if (!std::isfinite(v[k])) return false;
    return true;
}

}  // namespace

extern "C" long long cut3r_depth_cloud_workspace_bytes(int B, int H1, int W1) {
    if (!cloud_sizes_ok(B, 1, 1, H1, W1)) return -1;
    return (long long)cloud_layout(B, H1, W1).total;
}

extern "C" int cut3r_depth_cloud_count(const float* depth, int B, int H, int W, int H1, int W1, float depth_trunc, void* workspace,
                                       long long workspace_bytes, long long* counts, void* stream) {
    if (!depth || !workspace || !counts || !cloud_sizes_ok(B, H, W, H1, W1) || !(depth_trunc > 0.f)) return CUT3R_ERR_ARG;
    const CloudLayout L = cloud_layout(B, H1, W1);
    if (workspace_bytes < (long long)L.total) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)workspace;
    unsigned* bcount = (unsigned*)(w + L.bcount);
    unsigned* offs = (unsigned*)(w + L.offs);
    hipLaunchKernelGGL(cloud_count_kernel, dim3(L.nblk, B), dim3(256), 0, s, depth, H, W, H1, W1, depth_trunc, bcount);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    size_t sb = L.scan_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(w + L.scan, sb, bcount, offs, (int)L.nscan, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(cloud_view_counts_kernel, dim3(1), dim3(64), 0, s, offs, B, L.nblk, counts);
    return cut3r_check_launch();
}

extern "C" int cut3r_depth_cloud_emit(const float* depth, const unsigned char* rgb, int B, int H, int W, int H1, int W1, const double* c2w,
                                      const double* K, float depth_trunc, const void* workspace, long long workspace_bytes, float* points,
                                      unsigned char* colors, long long n, long long capacity, void* stream) {
    if (!depth || !c2w || !K || !workspace || !cloud_sizes_ok(B, H, W, H1, W1) || !(depth_trunc > 0.f)) return CUT3R_ERR_ARG;
    if ((colors != nullptr) != (rgb != nullptr)) return CUT3R_ERR_ARG;
    if (n < 0 || capacity < n || (n > 0 && !points)) return CUT3R_ERR_ARG;
    if (!finite_all(c2w, 12 * B) || !finite_all(K, 4 * B)) return CUT3R_ERR_ARG;
    for (int b = 0; b < B; b++)
        if (!(K[4 * b] > 0.0) || !(K[4 * b + 1] > 0.0)) return CUT3R_ERR_ARG;
    const CloudLayout L = cloud_layout(B, H1, W1);
    if (workspace_bytes < (long long)L.total) return CUT3R_ERR_ARG;
    if (n == 0) return CUT3R_OK;
    CloudViews v;
    for (int b = 0; b < B; b++) {
        for (int k = 0; k < 12; k++) v.c2w[b][k] = c2w[12 * b + k];
        for (int k = 0; k < 4; k++) v.K[b][k] = K[4 * b + k];
    }
    for (int b = B; b < CLOUD_MAX_VIEWS; b++) {
        for (int k = 0; k < 12; k++) v.c2w[b][k] = 0.0;
        for (int k = 0; k < 4; k++) v.K[b][k] = 1.0;
    }
    const unsigned* offs = (const unsigned*)((const char*)workspace + L.offs);
    hipLaunchKernelGGL(cloud_emit_kernel, dim3(L.nblk, B), dim3(256), 0, (hipStream_t)stream, depth, rgb, H, W, H1, W1, depth_trunc, v, offs, n,
                       points, colors);
    return cut3r_check_launch();
}

extern "C" long long cut3r_cloud_bounds_workspace_bytes(int N) {
    if (N <= 0) return -1;
    return (long long)align256(sizeof(float) * 7 * (size_t)bounds_blocks(N));
}

extern "C" int cut3r_cloud_bounds(const float* points, int N, float* out, void* workspace, long long workspace_bytes, void* stream) {
    if (!points || !out || !workspace || N <= 0 || workspace_bytes < cut3r_cloud_bounds_workspace_bytes(N)) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int nblk = bounds_blocks(N);
    hipLaunchKernelGGL(cloud_bounds_kernel, dim3(nblk), dim3(256), 0, s, points, N, (float*)workspace);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(cloud_bounds_fold_kernel, dim3(1), dim3(64), 0, s, (const float*)workspace, nblk, out);
    return cut3r_check_launch();
}

extern "C" long long cut3r_voxel_downsample_workspace_bytes(int N) {
    if (N <= 0) return -1;
    return (long long)voxel_layout(N).total;
}

extern "C" int cut3r_voxel_downsample_count(const float* points, int N, double voxel, const float* lo, const float* hi, void* workspace,
                                            long long workspace_bytes, long long* total, void* stream) {
    if (!points || !lo || !hi || !workspace || !total || N <= 0) return CUT3R_ERR_ARG;
    if (!(voxel > 0.0) || !std::isfinite(voxel)) return CUT3R_ERR_ARG;
    VoxelFrame fr;
    fr.voxel = voxel;
    for (int a = 0; a < 3; a++) {
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || hi[a] < lo[a]) return CUT3R_ERR_ARG;
        fr.lo[a] = (double)lo[a] - voxel * 0.5;
        const double top = std::floor(((double)hi[a] - fr.lo[a]) / voxel);
        if (!(top <= (double)VOXEL_MAX_INDEX)) return CUT3R_ERR_ARG;
    }
    const VoxelLayout L = voxel_layout(N);
    if (workspace_bytes < (long long)L.total) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)workspace;
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

extern "C" int cut3r_voxel_downsample_emit(const float* points, const unsigned char* colors, int N, const void* workspace,
                                           long long workspace_bytes, float* out_points, unsigned char* out_colors, int* out_counts, long long M,
                                           long long capacity, void* stream) {
    if (!points || !workspace || !out_points || !out_counts || N <= 0) return CUT3R_ERR_ARG;
    if ((colors != nullptr) != (out_colors != nullptr)) return CUT3R_ERR_ARG;
    if (M <= 0 || M > N || capacity < M) return CUT3R_ERR_ARG;
    const VoxelLayout L = voxel_layout(N);
    if (workspace_bytes < (long long)L.total) return CUT3R_ERR_ARG;
    const char* w = (const char*)workspace;
    hipLaunchKernelGGL(voxel_mean_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, colors, N,
                       (const unsigned*)(w + L.keys_in), (const unsigned*)(w + L.vals_out), (const unsigned*)(w + L.offs), L.nblk, M, out_points,
                       out_colors, out_counts);
    return cut3r_check_launch();
}
