// Sparse brick TSDF volume (gfx950): the dense volume of tsdf.hip restricted to allocated bricks of 8 x 8 x 8 voxels.
//
// The lattice is the dense one -- voxel (i, j, k) of a virtual grid X x Y x Z at origin + voxel * (float)(i, j, k) -- and so is the
// per-voxel fusion (tsdf_voxel.h, shared with tsdf.hip; both files are compiled with -ffp-contract=off): an allocated voxel holds the
// bits the dense grid would hold.  Structure:
//   flags  u8    [BZ,BY,BX]  1 = allocated, B* = ceil(dim / 8)
//   table  int32 [BZ,BY,BX]  pool slot of the brick, or -1; slots are numbered by ascending linear brick index t = (bz*BY + by)*BX + bx
//   bricks int32 [nb]        t of every slot (ascending)
//   pool   tsdf [nb,512], weight [nb,512], color [3][nb,512] fp32; voxel v = (lk*8 + lj)*8 + li inside a brick (x fastest)
// No hashing: the table is dense over the virtual grid (4 B per 512 voxels).  Limits: X, Y, Z <= 2^20 (indices exact in fp32), table
// entries <= 2^28, pool voxels nb * 512 < 2^31.
//
// mark: which bricks the views can give a negative tsdf (or a neighbour of one).  One thread per pixel with 0 < d <= depth_max: the
// pixel's frustum slab u in [ui - 0.5, ui + 0.5], v in [vi - 0.5, vi + 0.5], z in [d, d + trunc], cut into two z-segments; per segment
// the world AABB of the 8 back-projected corners, dilated by 1.5 voxels (1 for the 26-neighbourhood, 0.5 slack for fp32), and every brick
// that box overlaps is flagged.  A voxel ends with tsdf < 0 only if some view updated it with -trunc <= sdf < 0; then it projects into
// that pixel and lies in its slab, which is convex: inside the hull of its corners.  So every negative voxel and its 26 neighbours are
// allocated, and every cell that produces a triangle or surrounds a vertex-carrying edge (it contains a negative corner) reads
// dense-identical values at all 8 corners.  A missing in-grid neighbour reads as tsdf = 1, weight = 0.
//
// integrate: one workgroup per brick, one thread per voxel.  A view is dropped for the whole brick when the brick's bounding sphere lies
// outside the view's frustum (the planes z = 0, u = -0.5, u = W - 0.5, v = -0.5, v = H - 0.5, z = depth_max + trunc, moved out by a
// margin): it could not have updated any of its voxels.
//
// mesh: the count / scan / emit of tsdf_voxel.h (the code the dense grid runs) over its BrickStore: the pool voxels, neighbours inside the
// brick by arithmetic and across bricks through the table.  Vertices in (pool voxel, direction mask) order, faces in (pool cell,
// tetrahedron, triangle) order.
#include "tsdf_voxel.h"

#define MARK_SEGMENTS 2

namespace {

SparseGrid make_grid(int X, int Y, int Z) { return {X, Y, Z, (X + BRICK - 1) / BRICK, (Y + BRICK - 1) / BRICK, (Z + BRICK - 1) / BRICK}; }

bool grid_ok(int X, int Y, int Z) {
    if (X <= 0 || Y <= 0 || Z <= 0 || X > (1 << 20) || Y > (1 << 20) || Z > (1 << 20)) return false;
    const SparseGrid g = make_grid(X, Y, Z);
    return (long long)g.BX * g.BY * g.BZ <= (1LL << 28);
}

bool pool_ok(int nb) { return nb > 0 && (long long)nb * BRICK_VOXELS < (1LL << 31); }

long long table_entries(int X, int Y, int Z) {
    const SparseGrid g = make_grid(X, Y, Z);
    return (long long)g.BX * g.BY * g.BZ;
}

struct FlagOp {
    __host__ __device__ int operator()(unsigned char f) const { return f ? 1 : 0; }
};

size_t assign_temp_bytes(long long T) {
    size_t a = 0;
    rocprim::transform_iterator<const unsigned char*, FlagOp, int> it(nullptr, FlagOp());
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, it, (int*)nullptr, (int)(T > 0 ? T : 1), (hipStream_t)0);
    return a;
}

// ------------------------------------------------------------------------------------------------------------------------------ mark
// index range [lo, hi] of the voxels of one axis that the dilated interval covers, clamped to the grid; false when it misses the grid
// (or is not a number)
DEVINL bool mark_range(float lo, float hi, float o, float voxel, int dim, int& b0, int& b1) {
    const float flo = floorf((lo - o) / voxel - 1.5f), fhi = ceilf((hi - o) / voxel + 1.5f);
    if (!(fhi >= 0.f && flo <= (float)(dim - 1))) return false;
    b0 = (int)fmaxf(flo, 0.f) >> 3;
    b1 = (int)fminf(fhi, (float)(dim - 1)) >> 3;
    return true;
}

__global__ __launch_bounds__(256) void tsdf_sparse_mark_kernel(unsigned char* __restrict__ flags, SparseGrid g, float ox, float oy, float oz,
                                                               float voxel, const float* __restrict__ depth, long long npix, int H, int W,
                                                               const float* __restrict__ c2w, const float* __restrict__ K, float trunc,
                                                               float depth_max) {
    const long long HW = (long long)H * W;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        const float d = depth[p];
        if (!(d > 0.f) || !(d <= depth_max)) continue;
        const int b = (int)(p / HW), r = (int)(p - (long long)b * HW), vi = r / W, ui = r - vi * W;
        const float* c = c2w + b * 12;
        const float fx = K[b * 4], fy = K[b * 4 + 1], cx = K[b * 4 + 2], cy = K[b * 4 + 3];
        float ax[2], ay[2];
        ax[0] = (((float)ui - 0.5f) - cx) / fx;
        ax[1] = (((float)ui + 0.5f) - cx) / fx;
        ay[0] = (((float)vi - 0.5f) - cy) / fy;
        ay[1] = (((float)vi + 0.5f) - cy) / fy;
        for (int s = 0; s < MARK_SEGMENTS; ++s) {
            const float zz[2] = {d + trunc * ((float)s / (float)MARK_SEGMENTS), d + trunc * ((float)(s + 1) / (float)MARK_SEGMENTS)};
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int q = 0; q < 8; ++q) {
                const float z = zz[q >> 2], xc = ax[q & 1] * z, yc = ay[(q >> 1) & 1] * z;
                for (int a = 0; a < 3; ++a) {
                    const float w = ((c[a * 4] * xc + c[a * 4 + 1] * yc) + c[a * 4 + 2] * z) + c[a * 4 + 3];
                    lo[a] = fminf(lo[a], w);
                    hi[a] = fmaxf(hi[a], w);
                }
            }
            int x0, x1, y0, y1, z0, z1;
            if (!mark_range(lo[0], hi[0], ox, voxel, g.X, x0, x1) || !mark_range(lo[1], hi[1], oy, voxel, g.Y, y0, y1) ||
                !mark_range(lo[2], hi[2], oz, voxel, g.Z, z0, z1))
                continue;
            for (int bz = z0; bz <= z1; ++bz)
                for (int by = y0; by <= y1; ++by)
                    for (int bx = x0; bx <= x1; ++bx) flags[((long long)bz * g.BY + by) * g.BX + bx] = 1;     // same-value races only
        }
    }
}

// table[t] = slot (the exclusive scan already there) where flagged, else -1; total = number of flagged bricks
__global__ __launch_bounds__(256) void tsdf_sparse_assign_kernel(const unsigned char* __restrict__ flags, int* __restrict__ table, long long T,
                                                                 long long* __restrict__ total) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int f = flags[t] ? 1 : 0, s = table[t];
    if (t == T - 1) total[0] = (long long)s + f;
    table[t] = f ? s : -1;
}

// -------------------------------------------------------------------------------------------------------------------------- integrate
// keep = the brick's bounding sphere (centre p, radius rad, in world units) reaches the inside of the plane {a . p + a3 >= 0} moved out
// by the margin; a = the plane in world coordinates (any affine w2c: |a| scales the distance)
DEVINL bool plane_keeps(double a0, double a1, double a2, double a3, const double* p, double rad) {
    const double g = a0 * p[0] + a1 * p[1] + a2 * p[2] + a3;
    return g >= -rad * sqrt(a0 * a0 + a1 * a1 + a2 * a2);
}

__global__ __launch_bounds__(BRICK_VOXELS) void tsdf_sparse_integrate_kernel(
    float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color, const int* __restrict__ bricks, long long NP, SparseGrid g,
    float ox, float oy, float oz, float voxel, const float* __restrict__ depth, const unsigned char* __restrict__ rgb,
    const float* __restrict__ conf, int B, int H, int W, int ch, int cw, int ds, float conf_min, const float* __restrict__ w2c,
    const float* __restrict__ K, float trunc, float depth_max) {
    __shared__ float sv[TSDF_MAX_VIEWS * 16];
    __shared__ unsigned sviews;
    const int tid = threadIdx.x;
    stage_views(sv, w2c, K, B);
    if (tid == 0) sviews = 0u;
    __syncthreads();
    const int t = bricks[blockIdx.x];
    const int bx = t % g.BX, r = t / g.BX, by = r % g.BY, bz = r / g.BY;
    if (tid < B) {
        // Conservative by construction: the sphere around the brick's middle covers its 512 voxel positions (radius 3.5 sqrt(3) voxels,
        // + 0.1 % and 4e-6 of the coordinates' magnitude for the fp32 rounding of the positions and of the projections), and the image
        // planes are moved out by 0.01 pixel + 1e-5 of the pixel coordinates' magnitude, far above the fp32 error of u and v.
        const float* v = sv + tid * 16;
        const double p[3] = {(double)ox + (double)voxel * (bx * BRICK + 3.5), (double)oy + (double)voxel * (by * BRICK + 3.5),
                             (double)oz + (double)voxel * (bz * BRICK + 3.5)};
        const double mag = fabs(p[0]) + fabs(p[1]) + fabs(p[2]) + fabs((double)v[3]) + fabs((double)v[7]) + fabs((double)v[11]);
        const double rad = (double)voxel * (3.5 * 1.7320508075688772 * 1.001) + 4e-6 * mag;
        const double fx = v[12], fy = v[13], cx = v[14], cy = v[15];
        const double mu = 0.51 + 1e-5 * (fabs(cx) + W), mv = 0.51 + 1e-5 * (fabs(cy) + H);
        const double ul = cx + mu, ur = (double)W - 1.0 + mu - cx, vt = cy + mv, vb = (double)H - 1.0 + mv - cy;
        const double zf = (double)depth_max + (double)trunc;
        bool keep = plane_keeps(v[8], v[9], v[10], v[11], p, rad);                                              // z_c >= 0
        keep = keep && plane_keeps(-v[8], -v[9], -v[10], zf * 1.001 - v[11], p, rad);                           // z_c <= depth_max + trunc
        // u >= -mu: fx x_c + (cx + mu) z_c >= 0 (z_c > 0), and the three others alike
        keep = keep && plane_keeps(fx * v[0] + ul * v[8], fx * v[1] + ul * v[9], fx * v[2] + ul * v[10], fx * v[3] + ul * v[11], p, rad);
        keep = keep && plane_keeps(-fx * v[0] + ur * v[8], -fx * v[1] + ur * v[9], -fx * v[2] + ur * v[10], -fx * v[3] + ur * v[11], p, rad);
        keep = keep && plane_keeps(fy * v[4] + vt * v[8], fy * v[5] + vt * v[9], fy * v[6] + vt * v[10], fy * v[7] + vt * v[11], p, rad);
        keep = keep && plane_keeps(-fy * v[4] + vb * v[8], -fy * v[5] + vb * v[9], -fy * v[6] + vb * v[10], -fy * v[7] + vb * v[11], p, rad);
        if (keep || !(fx > 0.0) || !(fy > 0.0)) atomicOr(&sviews, 1u << tid);      // the side planes assume fx, fy > 0: else keep the view
    }
    __syncthreads();
    const unsigned views = sviews;
    if (views == 0u) return;
    const int i = bx * BRICK + (tid & 7), j = by * BRICK + ((tid >> 3) & 7), k = bz * BRICK + (tid >> 6);
    if (i >= g.X || j >= g.Y || k >= g.Z) return;      // the last brick of an axis may reach past the virtual grid: those voxels do not exist
    const float px = ox + voxel * (float)i, py = oy + voxel * (float)j, pz = oz + voxel * (float)k;
    tsdf_fuse_voxel<true>(tsdf, weight, color, (long long)blockIdx.x * BRICK_VOXELS + tid, NP, px, py, pz, sv, views, depth, rgb, conf, B, H,
                          W, ch, cw, ds, conf_min, trunc, depth_max);
}

BrickStore make_store(const int* table, const int* bricks, int nb, int X, int Y, int Z) {
    return {make_grid(X, Y, Z), table, bricks, (long long)nb * BRICK_VOXELS};
}

}  // namespace

extern "C" int cut3r_tsdf_sparse_mark(unsigned char* flags, int X, int Y, int Z, float ox, float oy, float oz, float voxel, const float* depth,
                                      int B, int H, int W, const float* c2w, const float* K, float trunc, float depth_max, void* stream) {
    if (!flags || !depth || !c2w || !K || !grid_ok(X, Y, Z)) return CUT3R_ERR_ARG;
    if (B < 1 || H <= 0 || W <= 0 || (long long)B * H * W >= (1LL << 31) || !(voxel > 0.f) || !(trunc > 0.f)) return CUT3R_ERR_ARG;
    const long long npix = (long long)B * H * W;
    hipLaunchKernelGGL(tsdf_sparse_mark_kernel, dim3(grid_for(npix)), dim3(256), 0, (hipStream_t)stream, flags, make_grid(X, Y, Z), ox, oy, oz,
                       voxel, depth, npix, H, W, c2w, K, trunc, depth_max);
    return cut3r_check_launch();
}

extern "C" long long cut3r_tsdf_sparse_assign_workspace_bytes(int X, int Y, int Z) {
    if (!grid_ok(X, Y, Z)) return -1;
    return (long long)align256(assign_temp_bytes(table_entries(X, Y, Z)));
}

extern "C" int cut3r_tsdf_sparse_assign(const unsigned char* flags, int* table, int X, int Y, int Z, void* workspace, long long workspace_bytes,
                                        long long* total, void* stream) {
    if (!flags || !table || !workspace || !total || !grid_ok(X, Y, Z)) return CUT3R_ERR_ARG;
    if (workspace_bytes < cut3r_tsdf_sparse_assign_workspace_bytes(X, Y, Z)) return CUT3R_ERR_ARG;
    const long long T = table_entries(X, Y, Z);
    hipStream_t s = (hipStream_t)stream;
    size_t tb = assign_temp_bytes(T);
    rocprim::transform_iterator<const unsigned char*, FlagOp, int> it(flags, FlagOp());
    if (hipcub::DeviceScan::ExclusiveSum(workspace, tb, it, table, (int)T, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(tsdf_sparse_assign_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, flags, table, T, total);
    return cut3r_check_launch();
}

extern "C" int cut3r_tsdf_sparse_integrate(float* tsdf, float* weight, float* color, const int* bricks, int nb, int X, int Y, int Z, float ox,
                                           float oy, float oz, float voxel, const float* depth, const unsigned char* rgb, const float* conf,
                                           int B, int H, int W, int ch, int cw, int ds, float conf_min, const float* w2c, const float* K,
                                           float trunc, float depth_max, void* stream) {
    if (!tsdf || !weight || !color || !bricks || !grid_ok(X, Y, Z) || !pool_ok(nb) || nb > table_entries(X, Y, Z)) return CUT3R_ERR_ARG;
    if (!views_ok(depth, conf, B, H, W, ch, cw, ds, w2c, K, voxel, trunc)) return CUT3R_ERR_ARG;
    hipLaunchKernelGGL(tsdf_sparse_integrate_kernel, dim3(nb), dim3(BRICK_VOXELS), 0, (hipStream_t)stream, tsdf, weight, color, bricks,
                       (long long)nb * BRICK_VOXELS, make_grid(X, Y, Z), ox, oy, oz, voxel, depth, rgb, conf, B, H, W, ch, cw, ds, conf_min, w2c,
                       K, trunc, depth_max);
    return cut3r_check_launch();
}

extern "C" long long cut3r_tsdf_sparse_mesh_workspace_bytes(int nb) {
    return pool_ok(nb) ? MeshWorkspace::bytes((long long)nb * BRICK_VOXELS) : -1;
}

extern "C" int cut3r_tsdf_sparse_mesh_count(const float* tsdf, const float* weight, const int* table, const int* bricks, int nb, int X, int Y,
                                            int Z, float weight_threshold, void* workspace, long long workspace_bytes, long long* totals,
                                            void* stream) {
    if (!tsdf || !weight || !table || !bricks || !workspace || !totals || !grid_ok(X, Y, Z) || !pool_ok(nb)) return CUT3R_ERR_ARG;
    if (nb > table_entries(X, Y, Z) || workspace_bytes < cut3r_tsdf_sparse_mesh_workspace_bytes(nb)) return CUT3R_ERR_ARG;
    return mesh_count(tsdf, weight, make_store(table, bricks, nb, X, Y, Z), weight_threshold, workspace, totals, (hipStream_t)stream);
}

extern "C" int cut3r_tsdf_sparse_mesh_emit(const float* tsdf, const float* color, const int* table, const int* bricks, int nb, int X, int Y,
                                           int Z, float ox, float oy, float oz, float voxel, const void* workspace, long long workspace_bytes,
                                           float* verts, unsigned char* colors, int* faces, long long nv, long long nf, void* stream) {
    if (!tsdf || !color || !table || !bricks || !workspace || !grid_ok(X, Y, Z) || !pool_ok(nb)) return CUT3R_ERR_ARG;
    if (nb > table_entries(X, Y, Z) || workspace_bytes < cut3r_tsdf_sparse_mesh_workspace_bytes(nb)) return CUT3R_ERR_ARG;
    return mesh_emit(tsdf, color, make_store(table, bricks, nb, X, Y, Z), ox, oy, oz, voxel, workspace, verts, colors, faces, nv, nf,
                     (hipStream_t)stream);
}
