// TSDF fusion of depth maps into a dense voxel grid and triangle-mesh extraction by marching tetrahedra (gfx950).
//
// Replaces the Open3D VoxelBlockGrid of the reference's tsdf_integrate.py (:31-62 integrate, :83-88 extract_triangle_mesh) with a
// DENSE grid: structure-of-arrays fp32 planes tsdf [N], weight [N], color [3][N] (0..255 as float), N = X*Y*Z, voxel n =
// (k*Y + j)*X + i (x fastest).  Every formula is written in one fixed order and the file is compiled with -ffp-contract=off: the numpy
// restatement in tests/tsdf_oracle.py reproduces the bits.
//
// The per-voxel fusion and the whole mesh extraction live in tsdf_voxel.h, shared with the sparse brick volume (tsdf_sparse.hip): the mesh
// kernels run here over its DenseStore, whose neighbour of a voxel is plain index arithmetic and is never missing.
//
// Mesh: the Kuhn (Freudenthal) split of every cell into six tetrahedra along its corner-0 -> corner-7 diagonal, one per axis permutation.
// Corners are numbered by bits (bit 0 = +x, bit 1 = +y, bit 2 = +z); the tetrahedron of permutation p is the chain 0 -> 1<<p0 ->
// (1<<p0)|(1<<p1) -> 7, so every tetrahedron edge joins a corner to a superset corner: a global edge is (lower voxel, direction mask m in
// 1..7) and that voxel owns its vertex.  Three passes: count (per voxel: a 7-bit mask of the vertices it owns + the triangles of the cell
// whose corner 0 it is), two exclusive scans of those counts (hipcub), emit.
#include "tsdf_voxel.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------------- integrate
// One thread per voxel (grid-stride); the B <= 16 views of the batch are applied in order with the voxel's state in registers, so the
// planes are read and written at most once per batch -- and not at all for a voxel that no view updates.
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color,
                                                             int X, int Y, long long N, float ox, float oy, float oz, float voxel,
                                                             const float* __restrict__ depth, const unsigned char* __restrict__ rgb,
                                                             const float* __restrict__ conf, int B, int H, int W, int ch, int cw, int ds,
                                                             float conf_min, const float* __restrict__ w2c, const float* __restrict__ K,
                                                             float trunc, float depth_max) {
    __shared__ float sv[TSDF_MAX_VIEWS * 16];
    stage_views(sv, w2c, K, B);
    __syncthreads();
    for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (long long)gridDim.x * blockDim.x) {
        // DenseStore::coords, kept in its unsigned form here: this kernel takes X, Y as plain arguments and converts unsigned i, j, k
        // to float, and its code object is left exactly as it was
        const unsigned n32 = (unsigned)n, r = n32 / (unsigned)X;      // N < 2^31: 32-bit division (a 64-bit one costs ~3x)
        const unsigned i = n32 - r * (unsigned)X, k = r / (unsigned)Y, j = r - k * (unsigned)Y;
        const float px = ox + voxel * (float)i, py = oy + voxel * (float)j, pz = oz + voxel * (float)k;
        tsdf_fuse_voxel<false>(tsdf, weight, color, n, N, px, py, pz, sv, 0u, depth, rgb, conf, B, H, W, ch, cw, ds, conf_min, trunc,
                               depth_max);
    }
}

bool dims_ok(int X, int Y, int Z) {
    return X > 0 && Y > 0 && Z > 0 && (long long)X * Y * Z < (1LL << 31);
}

DenseStore dense_store(int X, int Y, int Z) { return {X, Y, Z, (long long)X * Y, (long long)X * Y * Z}; }

}  // namespace

extern "C" int cut3r_tsdf_integrate(float* tsdf, float* weight, float* color, int X, int Y, int Z, float ox, float oy, float oz, float voxel,
                                    const float* depth, const unsigned char* rgb, const float* conf, int B, int H, int W, int ch, int cw,
                                    int ds, float conf_min, const float* w2c, const float* K, float trunc, float depth_max, void* stream) {
    if (!tsdf || !weight || !color || !dims_ok(X, Y, Z) || !views_ok(depth, conf, B, H, W, ch, cw, ds, w2c, K, voxel, trunc)) return CUT3R_ERR_ARG;
    const long long N = (long long)X * Y * Z;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3(grid_for(N)), dim3(256), 0, (hipStream_t)stream, tsdf, weight, color, X, Y, N, ox, oy, oz,
                       voxel, depth, rgb, conf, B, H, W, ch, cw, ds, conf_min, w2c, K, trunc, depth_max);
    return cut3r_check_launch();
}

extern "C" long long cut3r_tsdf_mesh_workspace_bytes(int X, int Y, int Z) {
    return dims_ok(X, Y, Z) ? MeshWorkspace::bytes((long long)X * Y * Z) : -1;
}

extern "C" int cut3r_tsdf_mesh_count(const float* tsdf, const float* weight, int X, int Y, int Z, float weight_threshold, void* workspace,
                                     long long workspace_bytes, long long* totals, void* stream) {
    if (!tsdf || !weight || !workspace || !totals || !dims_ok(X, Y, Z)) return CUT3R_ERR_ARG;
    if (workspace_bytes < cut3r_tsdf_mesh_workspace_bytes(X, Y, Z)) return CUT3R_ERR_ARG;
    return mesh_count(tsdf, weight, dense_store(X, Y, Z), weight_threshold, workspace, totals, (hipStream_t)stream);
}

extern "C" int cut3r_tsdf_mesh_emit(const float* tsdf, const float* color, int X, int Y, int Z, float ox, float oy, float oz, float voxel,
                                    const void* workspace, long long workspace_bytes, float* verts, unsigned char* colors, int* faces,
                                    long long nv, long long nf, void* stream) {
    if (!tsdf || !color || !workspace || !dims_ok(X, Y, Z)) return CUT3R_ERR_ARG;
    if (workspace_bytes < cut3r_tsdf_mesh_workspace_bytes(X, Y, Z)) return CUT3R_ERR_ARG;
    return mesh_emit(tsdf, color, dense_store(X, Y, Z), ox, oy, oz, voxel, workspace, verts, colors, faces, nv, nf,
                     (hipStream_t)stream);
}
