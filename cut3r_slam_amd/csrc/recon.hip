// Reconstruction metrics on gfx950: area-weighted surface sampling of a triangle mesh, exact 1-NN between two point sets on a uniform grid,
// and the fp64 moments of point-to-point ICP.  They replace the CPU libraries behind the reference's scripts/eval_recon.py (trimesh
// sample_surface :104-107, scipy cKDTree :22-41, Open3D registration_icp :44-58) and geometry_eval_utils.py:79-110 (pykdtree).
//
// Every formula is written in one fixed order and the file is compiled with -ffp-contract=off: tests/recon_oracle.py restates the
// samples and the NN results bit for bit.
#include <hipcub/hipcub.hpp>
#include "common.h"
#include "knn_grid.h"
#include "../../include/cut3r_hip.h"

namespace {

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---------------------------------------------------------------------------------------------------------------------- sampling
// counter-based random numbers: h(seed, stream, c) = sm(key ^ c), key = sm(sm(seed) ^ stream), sm = splitmix64.  No state: sample i uses
// the counters 3i, 3i + 1, 3i + 2, whatever the launch shape.
__host__ __device__ inline unsigned long long splitmix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

DEVINL bool face_ok(const int* __restrict__ faces, int f, int V, int& a, int& b, int& c) {
    a = faces[3 * (size_t)f];
    b = faces[3 * (size_t)f + 1];
    c = faces[3 * (size_t)f + 2];
    return a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V;
}

// area = 0.5 |(b - a) x (c - a)|; a face with an index out of range has area 0 (never sampled, never read)
__global__ __launch_bounds__(256) void recon_area_kernel(const float* __restrict__ v, int V, const int* __restrict__ faces, int F,
                                                         float* __restrict__ area) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int a, b, c;
    if (!face_ok(faces, f, V, a, b, c)) {
        area[f] = 0.f;
        return;
    }
    const float* pa = v + 3 * (size_t)a;
    const float* pb = v + 3 * (size_t)b;
    const float* pc = v + 3 * (size_t)c;
    const float e1x = pb[0] - pa[0], e1y = pb[1] - pa[1], e1z = pb[2] - pa[2];
    const float e2x = pc[0] - pa[0], e2y = pc[1] - pa[1], e2z = pc[2] - pa[2];
    const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
    area[f] = 0.5f * sqrtf((cx * cx + cy * cy) + cz * cz);
}

struct AreaToDouble {
    __host__ __device__ double operator()(float a) const { return (double)a; }
};

// sample i: face = the first f with cdf[f] > u0 * cdf[F-1] (u0: 53 bits), then p = (a + u1 (b - a)) + u2 (c - a) with u1, u2 (24 bits each)
// reflected to 1 - u when u1 + u2 > 1
__global__ __launch_bounds__(256) void recon_sample_kernel(const float* __restrict__ v, int V, const int* __restrict__ faces, int F,
                                                           const double* __restrict__ cdf, long long n, unsigned long long key,
                                                           float* __restrict__ out) {
    const double total = cdf[F - 1];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long c = 3ull * (unsigned long long)i;
        const unsigned long long h0 = splitmix64(key ^ c), h1 = splitmix64(key ^ (c + 1)), h2 = splitmix64(key ^ (c + 2));
        const double target = (double)(h0 >> 11) * 0x1p-53 * total;
        int lo = 0, hi = F - 1;                        // upper bound: the first cdf > target (F - 1 when none is, i.e. total == 0)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cdf[mid] > target) hi = mid;
            else lo = mid + 1;
        }
        float u1 = (float)(h1 >> 40) * 0x1p-24f, u2 = (float)(h2 >> 40) * 0x1p-24f;
        if (u1 + u2 > 1.f) {
            u1 = 1.f - u1;
            u2 = 1.f - u2;
        }
        float* o = out + 3 * (size_t)i;
        int a, b, cc;
        if (!face_ok(faces, lo, V, a, b, cc)) {
            o[0] = o[1] = o[2] = __builtin_nanf("");
            continue;
        }
        const float* pa = v + 3 * (size_t)a;
        const float* pb = v + 3 * (size_t)b;
        const float* pc = v + 3 * (size_t)cc;
        for (int k = 0; k < 3; ++k) o[k] = (pa[k] + u1 * (pb[k] - pa[k])) + u2 * (pc[k] - pa[k]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------- 1-NN
// The grid of knn_grid.h over the reference set R, built with split_outside = 1: the points of R outside the closed box B that the cells
// tile (the outliers the robust box leaves out) form their own run, scanned in full by every query.  Every other point p of R lies in B
// and in the cell knn_cell gives it.
//
// Stopping rule.  Let q be a query, c_q = knn_cell(q) (clamped), proj(q) the projection of q onto B and gap = |q - proj(q)|.  Before the
// shell of Chebyshev radius R around c_q is scanned, every unscanned p in B lies in a cell c_p with |c_p - c_q|_inf >= R, i.e. on some
// axis a, c_p[a] >= c_q[a] + R (or the mirror case).  Since c_p[a] >= 1 is not clamped from below, the cell rule gives p[a] - min[a] >=
// c_p[a] cs; proj(q)[a] - min[a] < (c_q[a] + 1) cs (q below the box on axis a: proj(q)[a] = min[a]).  So p[a] - proj(q)[a] > (R - 1) cs,
// up to the rounding of the cell rule: one fp32 subtraction, one product with fl(1/cs), at most 3 ulp of (c + 1) cs <= 162 cs, under
// 1e-4 cs -- taken as 1e-3 cs.  B is convex and proj(q) the nearest point of B to q, so (q - proj(q)) . (p - proj(q)) <= 0 and
//     |q - p|^2 >= gap^2 + |proj(q) - p|^2 >= gap^2 + max(0, R - 1.001)^2 cs^2 = L(R).
// The fp32 d2 of such a p is >= |q - p|^2 (1 - 5 u), and L is evaluated in fp32 to within a few u; lb = L(R) (1 - 1e-6) is therefore at
// most every unscanned d2.  The search stops once lb > min(best, lim): every unscanned point then has d2 > best (it can neither win nor
// tie) or d2 > lim (it is rejected) -- the result is the exhaustive search's, smallest reference index first among equal d2.  A query
// outside B starts with lb = gap^2: with max_dist, a query farther than max_dist from B stops before its first shell.
DEVINL void xform_point(const float* __restrict__ T, float x, float y, float z, float& ox, float& oy, float& oz) {
    if (!T) {
        ox = x; oy = y; oz = z;
        return;
    }
    ox = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    oy = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    oz = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

__global__ __launch_bounds__(256) void recon_xform_kernel(const float* __restrict__ q, int Q, const float* __restrict__ T, float* __restrict__ qt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Q) return;
    xform_point(T, q[3 * (size_t)i], q[3 * (size_t)i + 1], q[3 * (size_t)i + 2], qt[3 * (size_t)i], qt[3 * (size_t)i + 1], qt[3 * (size_t)i + 2]);
}

DEVINL void nn_consider(const float* __restrict__ spts, const int* __restrict__ sidx, unsigned j, float x, float y, float z, float lim,
                        float& best, int& bi) {
    const float dx = spts[3 * (size_t)j] - x, dy = spts[3 * (size_t)j + 1] - y, dz = spts[3 * (size_t)j + 2] - z;
    const float d = dx * dx + dy * dy + dz * dz;
    if (d <= lim) {
        const int r = sidx[j];
        if (d < best || (d == best && r < bi)) {
            best = d;
            bi = r;
        }
    }
}

// one thread per query in cell-sorted order (neighbouring threads walk the same cells)
__global__ __launch_bounds__(256) void recon_nn_kernel(int Q, const KnnHdr* __restrict__ hdr, const unsigned* __restrict__ starts,
                                                       const float* __restrict__ spts, const int* __restrict__ sidx, const float* __restrict__ sq,
                                                       const int* __restrict__ qidx, float lim, float* __restrict__ dist2, int* __restrict__ idx) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Q) return;
    const KnnHdr h = *hdr;
    const float x = sq[3 * (size_t)t], y = sq[3 * (size_t)t + 1], z = sq[3 * (size_t)t + 2];
    float hx, hy, hz;
    knn_box_hi(h, hx, hy, hz);
    const float gx = x < h.minx ? h.minx - x : (x > hx ? x - hx : 0.f);
    const float gy = y < h.miny ? h.miny - y : (y > hy ? y - hy : 0.f);
    const float gz = z < h.minz ? h.minz - z : (z > hz ? z - hz : 0.f);
    const float gap2 = (gx * gx + gy * gy) + gz * gz;
    float best = __builtin_inff();
    int bi = -1;
    const int ncell = h.gx * h.gy * h.gz;
    for (unsigned j = starts[ncell], e = starts[ncell + 1]; j < e; ++j) nn_consider(spts, sidx, j, x, y, z, lim, best, bi);
    int cx, cy, cz;
    knn_cell(h, x, y, z, cx, cy, cz);
    const int rmax = max(h.gx, max(h.gy, h.gz));
    for (int R = 0; R <= rmax; R++) {
        const float reach = fmaxf(0.f, (float)R - 1.001f) * h.cs;
        const float lb = (gap2 + reach * reach) * (1.f - 1e-6f);
        if (lb > fminf(best, lim)) break;
        const int z0 = max(0, cz - R), z1 = min(h.gz - 1, cz + R), y0 = max(0, cy - R), y1 = min(h.gy - 1, cy + R);
        const int x0 = max(0, cx - R), x1 = min(h.gx - 1, cx + R);
        for (int zz = z0; zz <= z1; zz++)
            for (int yy = y0; yy <= y1; yy++) {
                const bool face = (zz == cz - R) || (zz == cz + R) || (yy == cy - R) || (yy == cy + R);      // whole row on the shell
                for (int xx = x0; xx <= x1; xx += (face || R == 0) ? 1 : max(1, x1 - x0)) {
                    if (!face && R > 0 && xx != cx - R && xx != cx + R) continue;                            // interior rows: the two end cells only
                    const int c = (zz * h.gy + yy) * h.gx + xx;
                    for (unsigned j = starts[c], e = starts[c + 1]; j < e; j++) nn_consider(spts, sidx, j, x, y, z, lim, best, bi);
                }
            }
    }
    const int o = qidx[t];
    dist2[o] = bi >= 0 ? best : __builtin_inff();
    idx[o] = bi;
}

// ----------------------------------------------------------------------------------------------------------------------- ICP moments
// over the correspondences (idx >= 0) in fp64: [0] count, [1] sum d2, [2..4] sum src, [5..7] sum dst, [8 + 3a + b] sum src_a dst_b, src =
// the query under T exactly as recon_xform_kernel loads it.  A fixed grid (it depends on Q only) of grid-stride blocks; per block a wave
// butterfly and the four waves in order; the blocks folded in order by one thread per moment: the same bits on every run.
constexpr int ICP_NM = 17, ICP_MAX_BLOCKS = 1024;

int icp_blocks(int Q) {
    const int b = (Q + 255) / 256;
    return b < ICP_MAX_BLOCKS ? b : ICP_MAX_BLOCKS;
}

__global__ __launch_bounds__(256) void recon_moments_kernel(const float* __restrict__ src, int Q, const float* __restrict__ ref,
                                                            const float* __restrict__ T, const float* __restrict__ dist2,
                                                            const int* __restrict__ idx, double* __restrict__ part) {
    __shared__ double sm[4][ICP_NM];
    double acc[ICP_NM];
#pragma unroll
    for (int k = 0; k < ICP_NM; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < Q; i += gridDim.x * 256) {
        const int j = idx[i];
        if (j < 0) continue;
        float s[3];
        xform_point(T, src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2], s[0], s[1], s[2]);
        const float* d = ref + 3 * (size_t)j;
        acc[0] += 1.0;
        acc[1] += (double)dist2[i];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            acc[2 + a] += (double)s[a];
            acc[5 + a] += (double)d[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) acc[8 + 3 * a + b] += (double)s[a] * (double)d[b];
        }
    }
#pragma unroll
    for (int k = 0; k < ICP_NM; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        acc[k] = v;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < ICP_NM; ++k) sm[w][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < ICP_NM) {
        const int k = threadIdx.x;
        part[(size_t)blockIdx.x * ICP_NM + k] = ((sm[0][k] + sm[1][k]) + sm[2][k]) + sm[3][k];
    }
}

__global__ void recon_moments_fold_kernel(const double* __restrict__ part, int nblk, double* __restrict__ out) {
    const int k = threadIdx.x;
    if (k >= ICP_NM) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)b * ICP_NM + k];
    out[k] = s;
}

// ------------------------------------------------------------------------------------------------------------------------ layouts
size_t cdf_scan_bytes(int F) {
    size_t b = 0;
    rocprim::transform_iterator<const float*, AreaToDouble, double> it(nullptr, AreaToDouble());
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, b, it, (double*)nullptr, F > 0 ? F : 1, (hipStream_t)0);
    return b;
}

// hdr + bb | R: cell_of [P] | counts, starts, cursor [nscan] | spts [P,3] | sidx [P] | scan scratch || Q: qt [Q,3] | qcell [Q] | qcounts,
// qstarts, qcursor [nscan] | sq [Q,3] | qidx [Q].  nscan = (G + 1)^3 + 2: the cells, the outside run, the end.
struct NnLayout {
    int G;
    long long nscan;
    size_t cell_of, counts, starts, cursor, spts, sidx, scan, scan_bytes, grid_end;
    size_t qt, qcell, qcounts, qstarts, qcursor, sq, qidx, total;
};

NnLayout nn_layout(int P, int Q) {
    NnLayout L;
    L.G = knn3_grid_G(P);
    L.nscan = (long long)(L.G + 1) * (L.G + 1) * (L.G + 1) + 2;
    size_t o = 256;
    auto take = [&](size_t bytes) { const size_t r = o; o = align256(o + bytes); return r; };
    const size_t ns = 4 * (size_t)L.nscan;
    L.cell_of = take(4 * (size_t)P);
    L.counts = take(ns);
    L.starts = take(ns);
    L.cursor = take(ns);
    L.spts = take(12 * (size_t)P);
    L.sidx = take(4 * (size_t)P);
    L.scan_bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, L.scan_bytes, (unsigned*)nullptr, (unsigned*)nullptr, (int)L.nscan, (hipStream_t)0);
    L.scan = take(L.scan_bytes);
    L.grid_end = o;
    L.qt = take(12 * (size_t)Q);
    L.qcell = take(4 * (size_t)Q);
    L.qcounts = take(ns);
    L.qstarts = take(ns);
    L.qcursor = take(ns);
    L.sq = take(12 * (size_t)Q);
    L.qidx = take(4 * (size_t)Q);
    L.total = o;
    return L;
}

}  // namespace

extern "C" long long cut3r_mesh_cdf_workspace_bytes(int F) {
    if (F <= 0) return -1;
    return (long long)align256(cdf_scan_bytes(F));
}

extern "C" int cut3r_mesh_area_cdf(const float* verts, int V, const int* faces, int F, float* area, double* cdf, void* workspace,
                                   long long workspace_bytes, void* stream) {
    if (!verts || !faces || !area || !cdf || !workspace || V <= 0 || F <= 0) return CUT3R_ERR_ARG;
    if (workspace_bytes < cut3r_mesh_cdf_workspace_bytes(F)) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(recon_area_kernel, dim3((F + 255) / 256), dim3(256), 0, s, verts, V, faces, F, area);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    size_t tb = cdf_scan_bytes(F);
    rocprim::transform_iterator<const float*, AreaToDouble, double> it(area, AreaToDouble());
    if (hipcub::DeviceScan::InclusiveSum(workspace, tb, it, cdf, F, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    return cut3r_check_launch();
}

extern "C" int cut3r_mesh_sample(const float* verts, int V, const int* faces, int F, const double* cdf, long long n, unsigned long long seed,
                                 unsigned long long stream_id, float* out, void* stream) {
    if (!verts || !faces || !cdf || !out || V <= 0 || F <= 0 || n <= 0) return CUT3R_ERR_ARG;
    const unsigned long long key = splitmix64(splitmix64(seed) ^ stream_id);
    const long long g = (n + 255) / 256;
    hipLaunchKernelGGL(recon_sample_kernel, dim3((unsigned)(g < 256 * 64 ? g : 256 * 64)), dim3(256), 0, (hipStream_t)stream, verts, V, faces, F,
                       cdf, n, key, out);
    return cut3r_check_launch();
}

extern "C" long long cut3r_nn_workspace_bytes(int P, int Q) {
    if (P <= 0 || Q < 0) return -1;
    return (long long)nn_layout(P, Q).total;
}

extern "C" int cut3r_nn_build(const float* ref, int P, void* workspace, long long workspace_bytes, void* stream) {
    if (!ref || !workspace || P <= 0 || workspace_bytes < cut3r_nn_workspace_bytes(P, 0)) return CUT3R_ERR_ARG;
    const NnLayout L = nn_layout(P, 0);
    char* w = (char*)workspace;
    return knn_grid_build(ref, P, L.G, (KnnHdr*)w, (unsigned*)(w + 64), (int*)(w + L.cell_of), (unsigned*)(w + L.counts),
                          (unsigned*)(w + L.starts), (unsigned*)(w + L.cursor), (float*)(w + L.spts), (int*)(w + L.sidx), L.nscan, 1,
                          w + L.scan, L.scan_bytes, (hipStream_t)stream);
}

extern "C" int cut3r_nn_query(int P, const float* query, int Q, const float* T, float max_dist, float* dist2, int* idx, void* workspace,
                              long long workspace_bytes, void* stream) {
    if (!query || !dist2 || !idx || !workspace || P <= 0 || Q <= 0 || !(max_dist >= 0.f)) return CUT3R_ERR_ARG;
    if (workspace_bytes < cut3r_nn_workspace_bytes(P, Q)) return CUT3R_ERR_ARG;
    const NnLayout L = nn_layout(P, Q);
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)workspace;
    const KnnHdr* hdr = (const KnnHdr*)w;
    float* qt = (float*)(w + L.qt);
    int* qcell = (int*)(w + L.qcell);
    unsigned* qcounts = (unsigned*)(w + L.qcounts);
    unsigned* qstarts = (unsigned*)(w + L.qstarts);
    unsigned* qcursor = (unsigned*)(w + L.qcursor);
    float* sq = (float*)(w + L.sq);
    int* qidx = (int*)(w + L.qidx);
    const unsigned nb = (unsigned)((Q + 255) / 256);
    if (hipMemsetAsync(qcounts, 0, 4 * (size_t)L.nscan, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    if (hipMemsetAsync(qcursor, 0, 4 * (size_t)L.nscan, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(recon_xform_kernel, dim3(nb), dim3(256), 0, s, query, Q, T, qt);
    hipLaunchKernelGGL(knn_count_kernel, dim3(nb), dim3(256), 0, s, qt, Q, hdr, qcell, qcounts, 0);
    size_t sb = L.scan_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(w + L.scan, sb, qcounts, qstarts, (int)L.nscan, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(knn_scatter_kernel, dim3(nb), dim3(256), 0, s, qt, Q, qcell, qstarts, qcursor, sq, qidx);
    const float lim = max_dist * max_dist;
    hipLaunchKernelGGL(recon_nn_kernel, dim3(nb), dim3(256), 0, s, Q, hdr, (const unsigned*)(w + L.starts), (const float*)(w + L.spts),
                       (const int*)(w + L.sidx), sq, qidx, lim, dist2, idx);
    return cut3r_check_launch();
}

extern "C" long long cut3r_icp_moments_workspace_bytes(int Q) {
    if (Q <= 0) return -1;
    return (long long)(sizeof(double) * ICP_NM * (size_t)icp_blocks(Q));
}

extern "C" int cut3r_icp_moments(const float* src, int Q, const float* ref, int P, const float* T, const float* dist2, const int* idx, double* out,
                                 void* workspace, long long workspace_bytes, void* stream) {
    if (!src || !ref || !dist2 || !idx || !out || !workspace || Q <= 0 || P <= 0) return CUT3R_ERR_ARG;
    if (workspace_bytes < cut3r_icp_moments_workspace_bytes(Q)) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int nblk = icp_blocks(Q);
    double* part = (double*)workspace;
    hipLaunchKernelGGL(recon_moments_kernel, dim3(nblk), dim3(256), 0, s, src, Q, ref, T, dist2, idx, part);
    hipLaunchKernelGGL(recon_moments_fold_kernel, dim3(1), dim3(64), 0, s, part, nblk, out);
    return cut3r_check_launch();
}
