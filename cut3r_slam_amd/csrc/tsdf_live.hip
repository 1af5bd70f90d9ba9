// Live TSDF volume (gfx950): the sparse brick volume of tsdf_sparse.hip with INTEGER accumulators per voxel, so that views can be put in,
// taken out and re-posed exactly while a run goes on.
//
// The lattice, the brick table (flags, table, bricks; mark and assign) and the per-view gates are those of the sparse volume.  The pool is
//   acc int32 [5][nb*512]   sum_q, count, sum_r, sum_g, sum_b of voxel n = slot * 512 + (lk*8 + lj)*8 + li      (20 B per voxel)
// A view that updates a voxel (tsdf_view_sample of tsdf_voxel.h: the gates of tsdf_fuse_voxel) contributes q = (int)rintf(t * 32768.f)
// -- t in [-1, 1] and the product by a power of two is exact, so |q| <= 32768 --, 1 to the count and its three u8 colour values.  Integer
// sums commute and subtracting a view is the exact inverse of adding it: the accumulators depend on the SET of views that are in, not on
// the order, the batch split or the history.  With at most 65535 views in, 65535 * 32768 < 2^31 and 255 * 65535 fit an int32.
//
// integrate: one workgroup of 512 threads per visited pool slot, one thread per voxel, the brick-sphere versus frustum view mask of
// tsdf_sparse_integrate_kernel (restated below: that kernel's text stays as it is).  `slots` lists the pool slots to visit (the bricks
// allocated since earlier views went in catch up through it); bit b of `subtract` negates view b.  The voxel's deltas stay in registers
// over the <= 16 views; a voxel no view touches is neither read nor written, a touched one gets one load-add-store per plane.  No
// atomics: a voxel belongs to one thread.
//
// resolve: accumulators -> the fp32 pool planes (tsdf, weight, color) that the sparse mesh extraction and ray cast read: correctly rounded
// means, one fp64 division and one rounding to fp32 each; count == 0 gives the initial state (1, 0, 0, 0, 0).
#include "tsdf_voxel.h"

namespace {

// (the grid and pool limits of tsdf_sparse.hip)
SparseGrid live_grid(int X, int Y, int Z) { return {X, Y, Z, (X + BRICK - 1) / BRICK, (Y + BRICK - 1) / BRICK, (Z + BRICK - 1) / BRICK}; }

long long live_table_entries(int X, int Y, int Z) {
    const SparseGrid g = live_grid(X, Y, Z);
    return (long long)g.BX * g.BY * g.BZ;
}

bool grid_ok(int X, int Y, int Z) {
    if (X <= 0 || Y <= 0 || Z <= 0 || X > (1 << 20) || Y > (1 << 20) || Z > (1 << 20)) return false;
    return live_table_entries(X, Y, Z) <= (1LL << 28);
}

bool pool_ok(int nb) { return nb > 0 && (long long)nb * BRICK_VOXELS < (1LL << 31); }

// keep = the brick's bounding sphere (centre p, radius rad) reaches the inside of the plane {a . p + a3 >= 0} (tsdf_sparse.hip)
DEVINL bool live_plane_keeps(double a0, double a1, double a2, double a3, const double* p, double rad) {
    const double g = a0 * p[0] + a1 * p[1] + a2 * p[2] + a3;
    return g >= -rad * sqrt(a0 * a0 + a1 * a1 + a2 * a2);
}

__global__ __launch_bounds__(BRICK_VOXELS) void tsdf_live_integrate_kernel(
    int* __restrict__ acc, const int* __restrict__ bricks, int nb, const int* __restrict__ slots, long long NP, SparseGrid g, float ox,
    float oy, float oz, float voxel, const float* __restrict__ depth, const unsigned char* __restrict__ rgb, const float* __restrict__ conf,
    int B, int H, int W, int ch, int cw, int ds, float conf_min, const float* __restrict__ w2c, const float* __restrict__ K,
    unsigned subtract, float trunc, float depth_max) {
    __shared__ float sv[TSDF_MAX_VIEWS * 16];
    __shared__ unsigned sviews;
    const int tid = threadIdx.x;
    stage_views(sv, w2c, K, B);
    if (tid == 0) sviews = 0u;
    __syncthreads();
    const int slot = slots ? slots[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)slot >= (unsigned)nb) return;        // (a slot outside the pool: the wrapper refuses it; never touch memory for it)
    const int t = bricks[slot];
    const int bx = t % g.BX, r = t / g.BX, by = r % g.BY, bz = r / g.BY;
    if (tid < B) {
        // the conservative view mask of tsdf_sparse_integrate_kernel, with its margins: the sphere around the brick's middle covers its
        // 512 voxel positions, the image planes are moved out by 0.01 pixel + 1e-5 of the pixel coordinates' magnitude
        const float* v = sv + tid * 16;
        const double p[3] = {(double)ox + (double)voxel * (bx * BRICK + 3.5), (double)oy + (double)voxel * (by * BRICK + 3.5),
                             (double)oz + (double)voxel * (bz * BRICK + 3.5)};
        const double mag = fabs(p[0]) + fabs(p[1]) + fabs(p[2]) + fabs((double)v[3]) + fabs((double)v[7]) + fabs((double)v[11]);
        const double rad = (double)voxel * (3.5 * 1.7320508075688772 * 1.001) + 4e-6 * mag;
        const double fx = v[12], fy = v[13], cx = v[14], cy = v[15];
        const double mu = 0.51 + 1e-5 * (fabs(cx) + W), mv = 0.51 + 1e-5 * (fabs(cy) + H);
        const double ul = cx + mu, ur = (double)W - 1.0 + mu - cx, vt = cy + mv, vb = (double)H - 1.0 + mv - cy;
        const double zf = (double)depth_max + (double)trunc;
        bool keep = live_plane_keeps(v[8], v[9], v[10], v[11], p, rad);
        keep = keep && live_plane_keeps(-v[8], -v[9], -v[10], zf * 1.001 - v[11], p, rad);
        keep = keep && live_plane_keeps(fx * v[0] + ul * v[8], fx * v[1] + ul * v[9], fx * v[2] + ul * v[10], fx * v[3] + ul * v[11], p, rad);
        keep = keep && live_plane_keeps(-fx * v[0] + ur * v[8], -fx * v[1] + ur * v[9], -fx * v[2] + ur * v[10], -fx * v[3] + ur * v[11], p, rad);
        keep = keep && live_plane_keeps(fy * v[4] + vt * v[8], fy * v[5] + vt * v[9], fy * v[6] + vt * v[10], fy * v[7] + vt * v[11], p, rad);
        keep = keep && live_plane_keeps(-fy * v[4] + vb * v[8], -fy * v[5] + vb * v[9], -fy * v[6] + vb * v[10], -fy * v[7] + vb * v[11], p, rad);
        if (keep || !(fx > 0.0) || !(fy > 0.0)) atomicOr(&sviews, 1u << tid);
    }
    __syncthreads();
    const unsigned views = sviews;
    if (views == 0u) return;
    const int i = bx * BRICK + (tid & 7), j = by * BRICK + ((tid >> 3) & 7), k = bz * BRICK + (tid >> 6);
    if (i >= g.X || j >= g.Y || k >= g.Z) return;      // the last brick of an axis may reach past the virtual grid
    const float px = ox + voxel * (float)i, py = oy + voxel * (float)j, pz = oz + voxel * (float)k;
    const long long HW = (long long)H * W;
    int dq = 0, dn = 0, dr = 0, dg = 0, db = 0;
    bool touched = false;
    for (int b = 0; b < B; ++b) {
        if (!((views >> b) & 1u)) continue;
        float ts;
        int pix;
        if (!tsdf_view_sample(px, py, pz, sv + b * 16, depth + (long long)b * HW, conf ? conf + (long long)b * ch * cw : nullptr, H, W, ch, cw,
                              ds, conf_min, trunc, depth_max, ts, pix))
            continue;
        const int sgn = ((subtract >> b) & 1u) ? -1 : 1;
        dq += sgn * (int)rintf(ts * 32768.f);
        dn += sgn;
        if (rgb) {
            const unsigned char* p = rgb + (long long)b * 3 * HW + pix;
            dr += sgn * (int)p[0];
            dg += sgn * (int)p[HW];
            db += sgn * (int)p[2 * HW];
        }
        touched = true;
    }
    if (!touched) return;
    const long long n = (long long)slot * BRICK_VOXELS + tid;
    acc[n] += dq;
    acc[NP + n] += dn;
    if (rgb) {
        acc[2 * NP + n] += dr;
        acc[3 * NP + n] += dg;
        acc[4 * NP + n] += db;
    }
}

// four voxels per thread (a brick's 512 voxels and every plane's start are multiples of four: 16-byte loads and stores)
__global__ __launch_bounds__(256) void tsdf_live_resolve_kernel(const int* __restrict__ acc, int nb, const int* __restrict__ slots,
                                                                long long NV4, long long NP, float* __restrict__ tsdf,
                                                                float* __restrict__ weight, float* __restrict__ color) {
    for (long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x; m < NV4; m += (long long)gridDim.x * blockDim.x) {
        const long long e = m * 4;                    // the m-th quad of the visited voxels
        long long n = e;
        if (slots) {
            const int slot = slots[e >> 9];
            if ((unsigned)slot >= (unsigned)nb) continue;
            n = (long long)slot * BRICK_VOXELS + (e & 511);
        }
        const int4 q = *(const int4*)(acc + n), c = *(const int4*)(acc + NP + n);
        const int qq[4] = {q.x, q.y, q.z, q.w}, cc[4] = {c.x, c.y, c.z, c.w};
        float ts[4], wt[4];
        for (int a = 0; a < 4; ++a) {
            ts[a] = cc[a] == 0 ? 1.f : (float)((double)qq[a] / ((double)cc[a] * 32768.0));
            wt[a] = (float)cc[a];
        }
        *(float4*)(tsdf + n) = make_float4(ts[0], ts[1], ts[2], ts[3]);
        *(float4*)(weight + n) = make_float4(wt[0], wt[1], wt[2], wt[3]);
        for (int p = 0; p < 3; ++p) {
            const int4 s = *(const int4*)(acc + (2 + p) * NP + n);
            const int ss[4] = {s.x, s.y, s.z, s.w};
            float col[4];
            for (int a = 0; a < 4; ++a) col[a] = cc[a] == 0 ? 0.f : (float)((double)ss[a] / (double)cc[a]);
            *(float4*)(color + p * NP + n) = make_float4(col[0], col[1], col[2], col[3]);
        }
    }
}

bool aligned16(const void* p) { return ((unsigned long long)p & 15ull) == 0; }

}  // namespace

extern "C" int cut3r_tsdf_live_integrate(int* acc, const int* bricks, int nb, const int* slots, int ns, int X, int Y, int Z, float ox, float oy,
                                         float oz, float voxel, const float* depth, const unsigned char* rgb, const float* conf, int B, int H,
                                         int W, int ch, int cw, int ds, float conf_min, const float* w2c, const float* K,
                                         unsigned subtract_mask, float trunc, float depth_max, void* stream) {
    if (!acc || !bricks || !grid_ok(X, Y, Z) || !pool_ok(nb) || nb > live_table_entries(X, Y, Z)) return CUT3R_ERR_ARG;
    if (!views_ok(depth, conf, B, H, W, ch, cw, ds, w2c, K, voxel, trunc) || (long long)H * W >= (1LL << 31)) return CUT3R_ERR_ARG;
    if (slots && (ns < 1 || ns > nb)) return CUT3R_ERR_ARG;
    if (B < 32 && (subtract_mask >> B) != 0u) return CUT3R_ERR_ARG;
    hipLaunchKernelGGL(tsdf_live_integrate_kernel, dim3(slots ? ns : nb), dim3(BRICK_VOXELS), 0, (hipStream_t)stream, acc, bricks, nb, slots,
                       (long long)nb * BRICK_VOXELS, live_grid(X, Y, Z), ox, oy, oz, voxel, depth, rgb, conf, B, H, W, ch, cw, ds, conf_min, w2c,
                       K, subtract_mask, trunc, depth_max);
    return cut3r_check_launch();
}

extern "C" int cut3r_tsdf_live_resolve(const int* acc, int nb, const int* slots, int ns, float* tsdf, float* weight, float* color,
                                       void* stream) {
    if (!acc || !tsdf || !weight || !color || !pool_ok(nb)) return CUT3R_ERR_ARG;
    if (!aligned16(acc) || !aligned16(tsdf) || !aligned16(weight) || !aligned16(color)) return CUT3R_ERR_ARG;
    if (slots && (ns < 1 || ns > nb)) return CUT3R_ERR_ARG;
    const long long NV4 = (long long)(slots ? ns : nb) * (BRICK_VOXELS / 4);
    hipLaunchKernelGGL(tsdf_live_resolve_kernel, dim3(grid_for(NV4)), dim3(256), 0, (hipStream_t)stream, acc, nb, slots, NV4,
                       (long long)nb * BRICK_VOXELS, tsdf, weight, color);
    return cut3r_check_launch();
}
