// TSDF fusion of depth maps into a dense voxel grid and triangle-mesh extraction by marching tetrahedra (gfx950).
//
// Replaces the Open3D VoxelBlockGrid of the reference's tsdf_integrate.py (:31-62 integrate, :83-88 extract_triangle_mesh) with a
// DENSE grid: structure-of-arrays fp32 planes tsdf [N], weight [N], color [3][N] (0..255 as float), N = X*Y*Z, voxel n =
// (k*Y + j)*X + i (x fastest).  Every formula is written in one fixed order and the file is compiled with -ffp-contract=off: the numpy
// restatement in tests/tsdf_oracle.py reproduces the bits.
//
// The per-voxel fusion, the tetrahedron tables and the count packing live in tsdf_voxel.h, shared with the sparse brick volume
// (tsdf_sparse.hip).
//
// Mesh: the Kuhn (Freudenthal) split of every cell into six tetrahedra along its corner-0 -> corner-7 diagonal, one per axis permutation.
// Corners are numbered by bits (bit 0 = +x, bit 1 = +y, bit 2 = +z); the tetrahedron of permutation p is the chain 0 -> 1<<p0 ->
// (1<<p0)|(1<<p1) -> 7, so every tetrahedron edge joins a corner to a superset corner: a global edge is (lower voxel, direction mask m in
// 1..7) and that voxel owns its vertex.  Three passes: count (per voxel: a 7-bit mask of the vertices it owns + the triangles of the cell
// whose corner 0 it is), two exclusive scans of those counts (hipcub), emit.
#include "tsdf_voxel.h"
#include "../../include/cut3r_hip.h"

namespace {

DEVINL long long corner_offset(int c, long long X, long long XY) { return (c & 1) + ((c >> 1) & 1) * X + ((c >> 2) & 1) * XY; }

// ------------------------------------------------------------------------------------------------------------------------- integrate
// One thread per voxel (grid-stride); the B <= 16 views of the batch are applied in order with the voxel's state in registers, so the
// planes are read and written at most once per batch -- and not at all for a voxel that no view updates.
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color,
                                                             int X, int Y, long long N, float ox, float oy, float oz, float voxel,
                                                             const float* __restrict__ depth, const unsigned char* __restrict__ rgb,
                                                             const float* __restrict__ conf, int B, int H, int W, int ch, int cw, int ds,
                                                             float conf_min, const float* __restrict__ w2c, const float* __restrict__ K,
                                                             float trunc, float depth_max) {
    __shared__ float sv[TSDF_MAX_VIEWS * 16];          // per view: w2c rows [12], fx fy cx cy
    for (int t = threadIdx.x; t < B * 16; t += blockDim.x) {
        const int b = t >> 4, c = t & 15;
        sv[t] = c < 12 ? w2c[b * 12 + c] : K[b * 4 + (c - 12)];
    }
    __syncthreads();
    for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long long)gridDim.x * blockDim.x) {
        const unsigned n32 = (unsigned)n, r = n32 / (unsigned)X;      // N < 2^31: 32-bit division (a 64-bit one costs ~3x)
        const unsigned i = n32 - r * (unsigned)X, k = r / (unsigned)Y, j = r - k * (unsigned)Y;
        const float px = ox + voxel * (float)i, py = oy + voxel * (float)j, pz = oz + voxel * (float)k;
        tsdf_fuse_voxel<false>(tsdf, weight, color, n, N, px, py, pz, sv, 0u, depth, rgb, conf, B, H, W, ch, cw, ds, conf_min, trunc,
                               depth_max);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------- count
// code[n] = (vertex mask of voxel n: bit m-1 = the edge (n, m) carries a vertex) | (triangles of the cell with corner 0 at n) << 8.
// An edge carries a vertex when its ends differ in sign and some valid cell (all 8 corners weight >= threshold) contains it: the
// cells n - d, d in {0,1}^3 with d & m == 0.  Every sign-changing edge of a tetrahedron of a valid cell is used by that tetrahedron's
// triangles, so these are exactly the vertices some face references.
__global__ __launch_bounds__(256) void tsdf_mesh_count_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, int X, int Y,
                                                              int Z, long long N, float wth, unsigned short* __restrict__ code) {
    const long long XL = X, XY = (long long)X * Y;
    for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long long)gridDim.x * blockDim.x) {
        const unsigned n32 = (unsigned)n, r = n32 / (unsigned)X, kk = r / (unsigned)Y;
        const int i = (int)(n32 - r * (unsigned)X), j = (int)(r - kk * (unsigned)Y), k = (int)kk;
        // signs of the 8 voxels n + e, e in {0,1}^3 (outside the grid: same sign as n, i.e. no crossing)
        const bool in0 = tsdf[n] < 0.f;
        unsigned inside = in0 ? 1u : 0u;
        bool mixed = false;
        for (int e = 1; e < 8; ++e) {
            const int ei = i + (e & 1), ej = j + ((e >> 1) & 1), ek = k + ((e >> 2) & 1);
            bool s = in0;
            if (ei < X && ej < Y && ek < Z) s = tsdf[n + corner_offset(e, XL, XY)] < 0.f;
            inside |= (s ? 1u : 0u) << e;
            mixed |= s != in0;
        }
        if (!mixed) {
            code[n] = 0;
            continue;
        }
        // weight >= threshold over the 3x3x3 neighbourhood (bit (dz+1)*9 + (dy+1)*3 + (dx+1)); outside the grid = not ok
        unsigned ok = 0;
        for (int q = 0; q < 27; ++q) {
            const int dx = q % 3 - 1, dy = (q / 3) % 3 - 1, dz = q / 9 - 1;
            const int a = i + dx, b = j + dy, c = k + dz;
            if (a < 0 || b < 0 || c < 0 || a >= X || b >= Y || c >= Z) continue;
            if (weight[n + dx + dy * XL + dz * XY] >= wth) ok |= 1u << q;
        }
        code[n] = mesh_code(inside, valid_cells(ok));
    }
}

__global__ void tsdf_mesh_totals_kernel(const unsigned short* __restrict__ code, const long long* __restrict__ vofs,
                                        const long long* __restrict__ fofs, long long N, long long* __restrict__ totals) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const unsigned c = code[N - 1];
        totals[0] = vofs[N - 1] + __builtin_popcount(c & 0x7fu);
        totals[1] = fofs[N - 1] + (c >> 8);
    }
}

// ----------------------------------------------------------------------------------------------------------------------------- emit
// vertex (n, m): s = t0 / (t0 - t1), p = p0 + s (p1 - p0) per axis, colour c0 + s (c1 - c0) rounded floor(c + 0.5); written at vofs[n] +
// rank of m among the voxel's masks.  Faces of cell n at fofs[n], ordered by (tetrahedron, triangle); odd tetrahedra swap the winding.
__global__ __launch_bounds__(256) void tsdf_mesh_emit_kernel(const float* __restrict__ tsdf, const float* __restrict__ color, int X, int Y,
                                                             long long N, float ox, float oy, float oz, float voxel,
                                                             const unsigned short* __restrict__ code, const long long* __restrict__ vofs,
                                                             const long long* __restrict__ fofs, float* __restrict__ verts,
                                                             unsigned char* __restrict__ vcol, int* __restrict__ faces, long long nv,
                                                             long long nf) {
    const long long XL = X, XY = (long long)X * Y;
    for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long long)gridDim.x * blockDim.x) {
        const unsigned cd = code[n];
        if (cd == 0) continue;
        const unsigned n32 = (unsigned)n, r = n32 / (unsigned)X, kk = r / (unsigned)Y;
        const long long i = n32 - r * (unsigned)X, j = r - kk * (unsigned)Y, k = kk;
        const unsigned vm = cd & 0x7fu;
        long long vi = vofs[n];
        const float t0 = tsdf[n];
        const float p0[3] = {ox + voxel * (float)i, oy + voxel * (float)j, oz + voxel * (float)k};
        for (int m = 1; m < 8; ++m) {
            if (!((vm >> (m - 1)) & 1u)) continue;
            const long long u = n + corner_offset(m, XL, XY);
            const float t1 = tsdf[u];
            const float p1[3] = {ox + voxel * (float)(i + (m & 1)), oy + voxel * (float)(j + ((m >> 1) & 1)),
                                 oz + voxel * (float)(k + ((m >> 2) & 1))};
            if (vi < nv) {
                float ca[3] = {0.f, 0.f, 0.f}, cb[3] = {0.f, 0.f, 0.f};
                if (vcol) {
                    for (int a = 0; a < 3; ++a) {
                        ca[a] = color[a * N + n];
                        cb[a] = color[a * N + u];
                    }
                }
                mesh_vertex(t0, t1, p0, p1, ca, cb, verts + vi * 3, vcol ? vcol + vi * 3 : nullptr);
            }
            ++vi;
        }
        const unsigned ntri = cd >> 8;
        if (ntri == 0) continue;
        unsigned inside = 0;
        for (int e = 0; e < 8; ++e) inside |= (tsdf[n + corner_offset(e, XL, XY)] < 0.f ? 1u : 0u) << e;
        long long fi = fofs[n];
        for (int t = 0; t < 6; ++t) {
            int cc[4];
            unsigned cs = 0;
            for (int q = 0; q < 4; ++q) {
                cc[q] = chain_corner(t, q);
                cs |= ((inside >> cc[q]) & 1u) << q;
            }
            for (int r = 0; r < kNTri[cs]; ++r) {
                int id[3];
                for (int q = 0; q < 3; ++q) {
                    const int e = kTri[cs][r][q];
                    const int lo = cc[kEdge[e][0]], m = lo ^ cc[kEdge[e][1]];
                    const long long w = n + corner_offset(lo, XL, XY);
                    id[q] = (int)(vofs[w] + __builtin_popcount((unsigned)code[w] & ((1u << (m - 1)) - 1u)));
                }
                if (kParity[t] < 0) {
                    const int tmp = id[1];
                    id[1] = id[2];
                    id[2] = tmp;
                }
                if (fi < nf)
                    for (int q = 0; q < 3; ++q) faces[fi * 3 + q] = id[q];
                ++fi;
            }
        }
    }
}

bool dims_ok(int X, int Y, int Z) {
    return X > 0 && Y > 0 && Z > 0 && (long long)X * Y * Z < (1LL << 31);
}

}  // namespace

extern "C" int cut3r_tsdf_integrate(float* tsdf, float* weight, float* color, int X, int Y, int Z, float ox, float oy, float oz, float voxel,
                                    const float* depth, const unsigned char* rgb, const float* conf, int B, int H, int W, int ch, int cw,
                                    int ds, float conf_min, const float* w2c, const float* K, float trunc, float depth_max, void* stream) {
    if (!tsdf || !weight || !color || !depth || !w2c || !K || !dims_ok(X, Y, Z)) return CUT3R_ERR_ARG;
    if (B < 1 || B > TSDF_MAX_VIEWS || H <= 0 || W <= 0 || !(voxel > 0.f) || !(trunc > 0.f)) return CUT3R_ERR_ARG;
    if (conf && (ch <= 0 || cw <= 0 || ds <= 0)) return CUT3R_ERR_ARG;
    const long long N = (long long)X * Y * Z;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(grid_for(N)), dim3(256), 0, (hipStream_t)stream, tsdf, weight, color, X, Y, N, ox, oy, oz,
                       voxel, depth, rgb, conf, B, H, W, ch, cw, ds, conf_min, w2c, K, trunc, depth_max);
    return cut3r_check_launch();
}

extern "C" long long cut3r_tsdf_mesh_workspace_bytes(int X, int Y, int Z) {
    if (!dims_ok(X, Y, Z)) return -1;
    const long long N = (long long)X * Y * Z;
    return (long long)(align256(sizeof(unsigned short) * N) + 2 * align256(sizeof(long long) * N) + align256(scan_temp_bytes(N)));
}

extern "C" int cut3r_tsdf_mesh_count(const float* tsdf, const float* weight, int X, int Y, int Z, float weight_threshold, void* workspace,
                                     long long workspace_bytes, long long* totals, void* stream) {
    if (!tsdf || !weight || !workspace || !totals || !dims_ok(X, Y, Z)) return CUT3R_ERR_ARG;
    if (workspace_bytes < cut3r_tsdf_mesh_workspace_bytes(X, Y, Z)) return CUT3R_ERR_ARG;
    const long long N = (long long)X * Y * Z;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    unsigned short* code = (unsigned short*)ws;
    long long* vofs = (long long*)(ws + align256(sizeof(unsigned short) * N));
    long long* fofs = (long long*)((char*)vofs + align256(sizeof(long long) * N));
    void* tmp = (char*)fofs + align256(sizeof(long long) * N);
    size_t tb = scan_temp_bytes(N);
    hipLaunchKernelGGL(tsdf_mesh_count_kernel, dim3(grid_for(N)), dim3(256), 0, s, tsdf, weight, X, Y, Z, N, weight_threshold, code);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    rocprim::transform_iterator<const unsigned short*, VoxelCountOp, long long> vit(code, VoxelCountOp());
    rocprim::transform_iterator<const unsigned short*, CellCountOp, long long> fit(code, CellCountOp());
    if (hipcub::DeviceScan::ExclusiveSum(tmp, tb, vit, vofs, (int)N, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    tb = scan_temp_bytes(N);
    if (hipcub::DeviceScan::ExclusiveSum(tmp, tb, fit, fofs, (int)N, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(tsdf_mesh_totals_kernel, dim3(1), dim3(64), 0, s, code, vofs, fofs, N, totals);
    return cut3r_check_launch();
}

extern "C" int cut3r_tsdf_mesh_emit(const float* tsdf, const float* color, int X, int Y, int Z, float ox, float oy, float oz, float voxel,
                                    const void* workspace, long long workspace_bytes, float* verts, unsigned char* colors, int* faces,
                                    long long nv, long long nf, void* stream) {
    if (!tsdf || !color || !workspace || !dims_ok(X, Y, Z) || !(voxel > 0.f) || nv < 0 || nf < 0 || nv >= (1LL << 31)) return CUT3R_ERR_ARG;
    if ((nv > 0 && !verts) || (nf > 0 && !faces)) return CUT3R_ERR_ARG;
    if (workspace_bytes < cut3r_tsdf_mesh_workspace_bytes(X, Y, Z)) return CUT3R_ERR_ARG;
    const long long N = (long long)X * Y * Z;
    const char* ws = (const char*)workspace;
    const unsigned short* code = (const unsigned short*)ws;
    const long long* vofs = (const long long*)(ws + align256(sizeof(unsigned short) * N));
    const long long* fofs = (const long long*)((const char*)vofs + align256(sizeof(long long) * N));
    if (nv == 0 && nf == 0) return CUT3R_OK;
    hipLaunchKernelGGL(tsdf_mesh_emit_kernel, dim3(grid_for(N)), dim3(256), 0, (hipStream_t)stream, tsdf, color, X, Y, N, ox, oy, oz, voxel,
                       code, vofs, fofs, verts, colors, faces, nv, nf);
    return cut3r_check_launch();
}
