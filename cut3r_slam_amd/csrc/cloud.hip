// Dense point clouds for the depth-map evaluation (cut3r_slam_amd/eval_dense.py, the reference's scripts/eval7_scenes_dense.py): depth maps
// -> one world point cloud (Open3D create_from_rgbd_image + transform), and Open3D's PointCloud.voxel_down_sample.  Compiled with
// -ffp-contract=off: tests/cloud_oracle.py restates every operation in this order and the results are compared bit for bit.
//
// Both are count -> scan -> emit compactions: a block counts its valid items, hipcub scans the block counts, the block recomputes the
// flags and writes each item at (block offset + rank inside the block).  No atomic decides a position, so the output order is the input
// order and every run gives the same bits.
#include "voxel_cluster.h"

namespace {

constexpr int CLOUD_MAX_VIEWS = 16;
constexpr int BOUNDS_MAX_BLOCKS = 1024;

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

int bounds_blocks(int N) {
    const long long g = ((long long)N + 255) / 256;
    return (int)(g < BOUNDS_MAX_BLOCKS ? g : BOUNDS_MAX_BLOCKS);
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
    VoxelFrame fr;
    if (!voxel_frame(voxel, lo, hi, &fr)) return CUT3R_ERR_ARG;
    const VoxelLayout L = voxel_layout(N);
    if (workspace_bytes < (long long)L.total) return CUT3R_ERR_ARG;
    return voxel_sort_runs(points, N, fr, L, (char*)workspace, total, (hipStream_t)stream);
}

extern "C" int cut3r_voxel_downsample_emit(const float* points, const unsigned char* colors, int N, const void* workspace,
                                           long long workspace_bytes, float* out_points, unsigned char* out_colors, int* out_counts, long long M,
                                           long long capacity, void* stream) {
    if (!points || !workspace || !out_points || !out_counts || N <= 0) return CUT3R_ERR_ARG;
    if ((colors != nullptr) != (out_colors != nullptr)) return CUT3R_ERR_ARG;
    if (M <= 0 || M > N || capacity < M) return CUT3R_ERR_ARG;
    const VoxelLayout L = voxel_layout(N);
    if (workspace_bytes < (long long)L.total) return CUT3R_ERR_ARG;
    return voxel_means(points, colors, N, L, (const char*)workspace, out_points, out_colors, out_counts, M, nullptr, capacity,
                       (hipStream_t)stream);
}
