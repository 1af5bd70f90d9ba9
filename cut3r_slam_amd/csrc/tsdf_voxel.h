// What the dense (tsdf.hip) and the sparse brick (tsdf_sparse.hip) TSDF volumes share, so that they agree bit for bit by construction:
// the per-voxel fusion of a batch of views, and the whole mesh extraction -- the marching-tetrahedra tables, the count and emit kernels,
// the workspace layout and the host drivers -- written once over a "voxel store" (DenseStore, BrickStore below) that says where voxel
// (i, j, k) and its neighbours are kept.  Both files are compiled with -ffp-contract=off; every formula here is written in one fixed order
// (tests/tsdf_oracle.py restates it in numpy).
#pragma once
#include <hipcub/hipcub.hpp>
#include "common.h"
#include "../../include/cut3r_hip.h"

#define TSDF_MAX_VIEWS 16
#define BRICK 8
#define BRICK_VOXELS 512

namespace {

// the six tetrahedra: axis permutations in lexicographic order, and their parities (+1 even: the chain is positively oriented)
__constant__ int kPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
__constant__ int kParity[6] = {1, -1, -1, 1, 1, -1};
// tetrahedron edges (chain positions a < b) and the triangles of the 16 inside/outside cases (bit q = chain vertex q has tsdf < 0), as
// edge ids, wound so that the normal (b - a) x (c - a) points from negative to positive tsdf on a positively oriented tetrahedron
__constant__ int kEdge[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
__constant__ int kTri[16][2][3] = {
    {{-1, -1, -1}, {-1, -1, -1}}, {{0, 1, 2}, {-1, -1, -1}}, {{0, 4, 3}, {-1, -1, -1}}, {{1, 2, 4}, {1, 4, 3}},
    {{1, 3, 5}, {-1, -1, -1}},    {{0, 5, 2}, {0, 3, 5}},    {{0, 4, 5}, {0, 5, 1}},    {{2, 4, 5}, {-1, -1, -1}},
    {{2, 5, 4}, {-1, -1, -1}},    {{0, 1, 5}, {0, 5, 4}},    {{0, 5, 3}, {0, 2, 5}},    {{1, 5, 3}, {-1, -1, -1}},
    {{1, 3, 4}, {1, 4, 2}},       {{0, 3, 4}, {-1, -1, -1}}, {{0, 2, 1}, {-1, -1, -1}}, {{-1, -1, -1}, {-1, -1, -1}}};
__constant__ int kNTri[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};

DEVINL int chain_corner(int t, int q) {
    if (q == 0) return 0;
    if (q == 3) return 7;
    const int a = 1 << kPerm[t][0];
    return q == 1 ? a : (a | (1 << kPerm[t][1]));
}

struct VoxelCountOp {                                  // code -> vertices owned
    __host__ __device__ long long operator()(unsigned short c) const { return (long long)__builtin_popcount(c & 0x7fu); }
};
struct CellCountOp {                                   // code -> triangles of the cell at this corner 0
    __host__ __device__ long long operator()(unsigned short c) const { return (long long)(c >> 8); }
};

// bit d of the result: the cell (voxel - d) is valid, from ok = weight >= threshold over the 3x3x3 neighbourhood of the voxel
// (bit (dz+1)*9 + (dy+1)*3 + (dx+1))
DEVINL unsigned valid_cells(unsigned ok) {
    unsigned cellv = 0;
    for (int d = 0; d < 8; ++d) {
        bool v = true;
        for (int e = 0; e < 8; ++e) {
            const int q = (((e >> 2) & 1) - ((d >> 2) & 1) + 1) * 9 + (((e >> 1) & 1) - ((d >> 1) & 1) + 1) * 3 + ((e & 1) - (d & 1) + 1);
            v = v && ((ok >> q) & 1u);
        }
        cellv |= (v ? 1u : 0u) << d;
    }
    return cellv;
}

// code of a voxel = (vertex mask: bit m-1 = the edge (voxel, m) carries a vertex) | (triangles of the cell with corner 0 here) << 8, from
// inside (bit e: tsdf < 0 at voxel + e) and cellv (valid_cells).  An edge carries a vertex when its ends differ in sign and some valid
// cell contains it: the cells voxel - d, d in {0,1}^3 with d & m == 0.
DEVINL unsigned short mesh_code(unsigned inside, unsigned cellv) {
    unsigned vm = 0;
    for (int m = 1; m < 8; ++m) {
        if ((((inside >> m) & 1u) != (inside & 1u))) {
            bool any = false;
            for (int d = 0; d < 8; ++d) any = any || (((d & m) == 0) && ((cellv >> d) & 1u));
            if (any) vm |= 1u << (m - 1);
        }
    }
    unsigned nf = 0;
    if (cellv & 1u) {
        for (int t = 0; t < 6; ++t) {
            unsigned cs = 0;
            for (int q = 0; q < 4; ++q) cs |= ((inside >> chain_corner(t, q)) & 1u) << q;
            nf += kNTri[cs];
        }
    }
    return (unsigned short)(vm | (nf << 8));
}

// the views of an integrate launch, staged into LDS by the whole workgroup (the caller synchronises): per view w2c rows [12], fx fy cx cy
DEVINL void stage_views(float* sv, const float* __restrict__ w2c, const float* __restrict__ K, int B) {
    for (int t = threadIdx.x; t < B * 16; t += blockDim.x) {
        const int b = t >> 4, c = t & 15;
        sv[t] = c < 12 ? w2c[b * 12 + c] : K[b * 4 + (c - 12)];
    }
}

// the view arguments of the two integrate entry points
inline bool views_ok(const float* depth, const float* conf, int B, int H, int W, int ch, int cw, int ds, const float* w2c, const float* K,
                     float voxel, float trunc) {
    if (!depth || !w2c || !K || B < 1 || B > TSDF_MAX_VIEWS || H <= 0 || W <= 0 || !(voxel > 0.f) || !(trunc > 0.f)) return false;
    return !conf || (ch > 0 && cw > 0 && ds > 0);
}

// The fusion of the B <= 16 views of a batch into the voxel at (px, py, pz), whose state lives at index n of the planes tsdf [N],
// weight [N], color [3][N]: the views are applied in order with the state in registers, so the planes are read and written at most once
// -- and not at all when no view updates the voxel.  sv: per view w2c rows [12], fx fy cx cy.  MASKED: view b is skipped unless bit b of
// `views` is set (the caller has shown that it cannot update this voxel).
template <bool MASKED>
DEVINL void tsdf_fuse_voxel(float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ color, long long n, long long N,
                            float px, float py, float pz, const float* sv, unsigned views, const float* __restrict__ depth,
                            const unsigned char* __restrict__ rgb, const float* __restrict__ conf, int B, int H, int W, int ch, int cw, int ds,
                            float conf_min, float trunc, float depth_max) {
    const long long HW = (long long)H * W;
    bool loaded = false;
    float ts = 0.f, w = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
    for (int b = 0; b < B; ++b) {
        if (MASKED && !((views >> b) & 1u)) continue;
        const float* v = sv + b * 16;
        const float zc = ((v[8] * px + v[9] * py) + v[10] * pz) + v[11];
        if (!(zc > 0.f)) continue;
        const float xc = ((v[0] * px + v[1] * py) + v[2] * pz) + v[3];
        const float yc = ((v[4] * px + v[5] * py) + v[6] * pz) + v[7];
        // outside the image by more than a pixel: rejected on an approximate reciprocal before the two correctly rounded divisions.
        // The estimate is within ~3e-7 (|u - cx| + |cx|) of the exact u, so the margin of 1 + 1e-6 (|c| + size) never drops a
        // voxel-view the exact test keeps (the bits of what is fused do not depend on it); tiny z_c go to the exact test.
        if (zc > 1e-30f) {
            const float rz = __builtin_amdgcn_rcpf(zc);
            const float ua = (v[12] * xc) * rz + v[14], va = (v[13] * yc) * rz + v[15];
            const float mu = 1.f + 1e-6f * (fabsf(v[14]) + (float)W), mv = 1.f + 1e-6f * (fabsf(v[15]) + (float)H);
            if (ua < -0.5f - mu || ua >= (float)W - 0.5f + mu || va < -0.5f - mv || va >= (float)H - 0.5f + mv) continue;
        }
        const float u = (v[12] * xc) / zc + v[14];
        const float vv = (v[13] * yc) / zc + v[15];
        const float uf = floorf(u + 0.5f), vf = floorf(vv + 0.5f);
        if (!(uf >= 0.f && uf < (float)W && vf >= 0.f && vf < (float)H)) continue;
        const int ui = (int)uf, vi = (int)vf;
        const long long pix = (long long)b * HW + (long long)vi * W + ui;
        const float d = depth[pix];
        if (!(d > 0.f) || !(d <= depth_max)) continue;
        if (conf) {
            const int ci = min(vi / ds, ch - 1), cj = min(ui / ds, cw - 1);
            if (conf[((long long)b * ch + ci) * cw + cj] < conf_min) continue;
        }
        const float sdf = d - zc;
        if (sdf < -trunc) continue;
        const float t = fminf(1.f, sdf / trunc);
        if (!loaded) {
            ts = tsdf[n];
            w = weight[n];
            if (rgb) {
                c0 = color[n];
                c1 = color[N + n];
                c2 = color[2 * N + n];
            }
            loaded = true;
        }
        const float w1 = w + 1.f;
        ts = (ts * w + t) / w1;
        if (rgb) {
            const unsigned char* p = rgb + (long long)b * 3 * HW + (long long)vi * W + ui;
            c0 = (c0 * w + (float)p[0]) / w1;
            c1 = (c1 * w + (float)p[HW]) / w1;
            c2 = (c2 * w + (float)p[2 * HW]) / w1;
        }
        w = w1;
    }
    if (loaded) {
        tsdf[n] = ts;
        weight[n] = w;
        if (rgb) {
            color[n] = c0;
            color[N + n] = c1;
            color[2 * N + n] = c2;
        }
    }
}

// What ONE view contributes to the voxel at (px, py, pz), for the live volume (tsdf_live.hip), whose integer accumulators need the
// sample and not the running average: the projection and every gate of tsdf_fuse_voxel above, restated in the same fixed order (z_c > 0,
// the approximate-reciprocal early reject, the two correctly rounded divisions, floorf(u + 0.5f), the depth range, the confidence gate
// at stride ds, sdf < -trunc).  v: the view's w2c rows [12], fx fy cx cy; depth [H,W] and conf [ch,cw] are the view's own planes.  False:
// the view does not update the voxel; else t = fminf(1, sdf / trunc), in [-1, 1], and pix = vi * W + ui.  tests/test_tsdf_live_gpu.py
// ties the two: a single view fused by either leaves the same voxels updated, with the same t.
DEVINL bool tsdf_view_sample(float px, float py, float pz, const float* v, const float* __restrict__ depth, const float* __restrict__ conf,
                             int H, int W, int ch, int cw, int ds, float conf_min, float trunc, float depth_max, float& t, int& pix) {
    const float zc = ((v[8] * px + v[9] * py) + v[10] * pz) + v[11];
    if (!(zc > 0.f)) return false;
    const float xc = ((v[0] * px + v[1] * py) + v[2] * pz) + v[3];
    const float yc = ((v[4] * px + v[5] * py) + v[6] * pz) + v[7];
    if (zc > 1e-30f) {                                 // the early reject of tsdf_fuse_voxel: never drops what the exact test keeps
        const float rz = __builtin_amdgcn_rcpf(zc);
        const float ua = (v[12] * xc) * rz + v[14], va = (v[13] * yc) * rz + v[15];
        const float mu = 1.f + 1e-6f * (fabsf(v[14]) + (float)W), mv = 1.f + 1e-6f * (fabsf(v[15]) + (float)H);
        if (ua < -0.5f - mu || ua >= (float)W - 0.5f + mu || va < -0.5f - mv || va >= (float)H - 0.5f + mv) return false;
    }
    const float u = (v[12] * xc) / zc + v[14];
    const float vv = (v[13] * yc) / zc + v[15];
    const float uf = floorf(u + 0.5f), vf = floorf(vv + 0.5f);
    if (!(uf >= 0.f && uf < (float)W && vf >= 0.f && vf < (float)H)) return false;
    const int ui = (int)uf, vi = (int)vf;
    pix = vi * W + ui;
    const float d = depth[pix];
    if (!(d > 0.f) || !(d <= depth_max)) return false;
    if (conf) {
        const int ci = min(vi / ds, ch - 1), cj = min(ui / ds, cw - 1);
        if (conf[(long long)ci * cw + cj] < conf_min) return false;
    }
    const float sdf = d - zc;
    if (sdf < -trunc) return false;
    t = fminf(1.f, sdf / trunc);
    return true;
}

// one triangle-mesh vertex on the edge from a voxel (tsdf t0, position p0, colours ca) to a neighbour (t1, p1, cb): s = t0 / (t0 - t1),
// p = p0 + s (p1 - p0) per axis, colour ca + s (cb - ca) rounded floor(c + 0.5)
DEVINL void mesh_vertex(float t0, float t1, const float* p0, const float* p1, const float* ca, const float* cb, float* __restrict__ vert,
                        unsigned char* __restrict__ vcol) {
    const float s = t0 / (t0 - t1);
    for (int a = 0; a < 3; ++a) vert[a] = p0[a] + s * (p1[a] - p0[a]);
    if (vcol) {
        for (int a = 0; a < 3; ++a) {
            const float c = floorf((ca[a] + s * (cb[a] - ca[a])) + 0.5f);
            vcol[a] = (unsigned char)fminf(255.f, fmaxf(0.f, c));
        }
    }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

inline size_t scan_temp_bytes(long long N) {          // the larger of the two count scans' scratch
    size_t a = 0, b = 0;
    rocprim::transform_iterator<const unsigned short*, VoxelCountOp, long long> vit(nullptr, VoxelCountOp());
    rocprim::transform_iterator<const unsigned short*, CellCountOp, long long> fit(nullptr, CellCountOp());
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, a, vit, (long long*)nullptr, (int)(N > 0 ? N : 1), (hipStream_t)0);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, fit, (long long*)nullptr, (int)(N > 0 ? N : 1), (hipStream_t)0);
    return a > b ? a : b;
}

inline int grid_for(long long N) {
    const long long g = (N + 255) / 256;
    return (int)(g < 256 * 64 ? g : 256 * 64);       // grid-stride beyond 64 blocks per CU
}

// ---------------------------------------------------------------------------------------------------------------------- voxel stores
// A store keeps N voxels of the grid X x Y x Z and is passed to the mesh kernels by value:
//   coords(n, i, j, k)                  the grid position of stored voxel n; false when that slot holds no voxel of the grid
//   neighbour(n, i, j, k, di, dj, dk)   the stored index of the IN-GRID voxel (i + di, j + dj, k + dk), d in {-1,0,1}^3, or -1 when it is
//                                       not stored
//   index(i, j, k)                      the stored index of the in-grid voxel (i, j, k), or -1 when it is not stored (the ray cast's entry)
//   kMayMiss                            whether neighbour() can return -1: where it cannot, the handling of -1 folds away at compile time

// the dense grid: voxel n = (k*Y + j)*X + i (x fastest), every voxel stored
struct DenseStore {
    static constexpr bool kMayMiss = false;
    int X, Y, Z;
    long long XY, N;                                   // X*Y, X*Y*Z < 2^31

    DEVINL bool coords(long long n, int& i, int& j, int& k) const {
        const unsigned n32 = (unsigned)n, r = n32 / (unsigned)X, kk = r / (unsigned)Y;      // N < 2^31: 32-bit division (a 64-bit one costs ~3x)
        i = (int)(n32 - r * (unsigned)X);
        j = (int)(r - kk * (unsigned)Y);
        k = (int)kk;
        return true;
    }
    DEVINL long long index(int i, int j, int k) const { return ((long long)k * Y + j) * X + i; }
    DEVINL long long neighbour(long long n, int, int, int, int di, int dj, int dk) const {
        return n + di + dj * (long long)X + dk * XY;
    }
};

struct SparseGrid {
    int X, Y, Z, BX, BY, BZ;
};

// the brick pool: voxel n = slot * 512 + (lk*8 + lj)*8 + li of brick bricks[slot] = (bz*BY + by)*BX + bx; table[brick] = slot or -1.  The last
// brick of an axis may reach past the grid: those slots hold no voxel.
struct BrickStore : SparseGrid {
    static constexpr bool kMayMiss = true;
    const int *table, *bricks;
    long long N;

    DEVINL bool coords(long long n, int& i, int& j, int& k) const {
        const int t = bricks[n >> 9], v = (int)(n & 511);
        const int bx = t % BX, r = t / BX, by = r % BY, bz = r / BY;
        i = bx * BRICK + (v & 7);
        j = by * BRICK + ((v >> 3) & 7);
        k = bz * BRICK + (v >> 6);
        return i < X && j < Y && k < Z;
    }
    DEVINL long long index(int i, int j, int k) const {
        const int s = table[((long long)(k >> 3) * BY + (j >> 3)) * BX + (i >> 3)];
        return s < 0 ? -1 : (long long)s * BRICK_VOXELS + (((k & 7) << 6) | ((j & 7) << 3) | (i & 7));
    }
    DEVINL long long neighbour(long long n, int i, int j, int k, int di, int dj, int dk) const {       // inside the brick without the table
        const unsigned li = (unsigned)((i & 7) + di), lj = (unsigned)((j & 7) + dj), lk = (unsigned)((k & 7) + dk);
        if (li < 8u && lj < 8u && lk < 8u) return n + di + dj * 8 + dk * 64;
        return index(i + di, j + dj, k + dk);
    }
};

// whether neighbour() found no stored voxel; it then reads as the initial state tsdf = 1, weight = 0, colour 0
template <class Store>
DEVINL bool missing(long long u) {
    return Store::kMayMiss && u < 0;
}

// ----------------------------------------------------------------------------------------------------------------------------- count
// code[n] = (vertex mask of voxel n: bit m-1 = the edge (n, m) carries a vertex) | (triangles of the cell with corner 0 at n) << 8.
// An edge carries a vertex when its ends differ in sign and some valid cell (all 8 corners weight >= threshold) contains it: the
// cells n - d, d in {0,1}^3 with d & m == 0.  Every sign-changing edge of a tetrahedron of a valid cell is used by that tetrahedron's
// triangles, so these are exactly the vertices some face references.
template <class Store>
__global__ __launch_bounds__(256) void tsdf_mesh_count_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight, Store st,
                                                              float wth, unsigned short* __restrict__ code) {
    for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < st.N; n += (long long)gridDim.x * blockDim.x) {
        int i, j, k;
        if (!st.coords(n, i, j, k)) {
            code[n] = 0;
            continue;
        }
        // signs of the 8 voxels n + e, e in {0,1}^3 (outside the grid: same sign as n, i.e. no crossing)
        const bool in0 = tsdf[n] < 0.f;
        unsigned inside = in0 ? 1u : 0u;
        bool mixed = false;
        for (int e = 1; e < 8; ++e) {
            const int di = e & 1, dj = (e >> 1) & 1, dk = (e >> 2) & 1;
            bool s = in0;
            if (i + di < st.X && j + dj < st.Y && k + dk < st.Z) {
                const long long u = st.neighbour(n, i, j, k, di, dj, dk);
                s = (missing<Store>(u) ? 1.f : tsdf[u]) < 0.f;
            }
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
            if (a < 0 || b < 0 || c < 0 || a >= st.X || b >= st.Y || c >= st.Z) continue;
            const long long u = st.neighbour(n, i, j, k, dx, dy, dz);
            if ((missing<Store>(u) ? 0.f : weight[u]) >= wth) ok |= 1u << q;
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

// ------------------------------------------------------------------------------------------------------------------------------ emit
// vertex (n, m): s = t0 / (t0 - t1), p = p0 + s (p1 - p0) per axis, colour c0 + s (c1 - c0) rounded floor(c + 0.5); written at vofs[n] +
// rank of m among the voxel's masks.  Faces of cell n at fofs[n], ordered by (tetrahedron, triangle); odd tetrahedra swap the winding.
// In a store that may miss voxels a vertex-carrying edge has a negative end, so both ends are stored whenever the allocation covers the
// negative voxels' neighbourhoods; for any other contents the missing end reads as tsdf = 1, colour 0, and a face corner whose owner is
// missing gets index 0.
template <class Store>
__global__ __launch_bounds__(256) void tsdf_mesh_emit_kernel(const float* __restrict__ tsdf, const float* __restrict__ color, Store st,
                                                             float ox, float oy, float oz, float voxel,
                                                             const unsigned short* __restrict__ code, const long long* __restrict__ vofs,
                                                             const long long* __restrict__ fofs, float* __restrict__ verts,
                                                             unsigned char* __restrict__ vcol, int* __restrict__ faces, long long nv,
                                                             long long nf) {
    for (long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x; n < st.N; n += (long long)gridDim.x * blockDim.x) {
        const unsigned cd = code[n];
        if (cd == 0) continue;
        int i, j, k;
        st.coords(n, i, j, k);
        const unsigned vm = cd & 0x7fu;
        long long vi = vofs[n];
        const float t0 = tsdf[n];
        const float p0[3] = {ox + voxel * (float)i, oy + voxel * (float)j, oz + voxel * (float)k};
        for (int m = 1; m < 8; ++m) {
            if (!((vm >> (m - 1)) & 1u)) continue;
            const long long u = st.neighbour(n, i, j, k, m & 1, (m >> 1) & 1, (m >> 2) & 1);
            const float t1 = missing<Store>(u) ? 1.f : tsdf[u];
            const float p1[3] = {ox + voxel * (float)(i + (m & 1)), oy + voxel * (float)(j + ((m >> 1) & 1)),
                                 oz + voxel * (float)(k + ((m >> 2) & 1))};
            if (vi < nv) {
                float ca[3] = {0.f, 0.f, 0.f}, cb[3] = {0.f, 0.f, 0.f};
                if (vcol) {
                    for (int a = 0; a < 3; ++a) {
                        ca[a] = color[a * st.N + n];
                        cb[a] = missing<Store>(u) ? 0.f : color[a * st.N + u];
                    }
                }
                mesh_vertex(t0, t1, p0, p1, ca, cb, verts + vi * 3, vcol ? vcol + vi * 3 : nullptr);
            }
            ++vi;
        }
        const unsigned ntri = cd >> 8;
        if (ntri == 0) continue;
        long long cn[8];                               // where the cell's corners are stored (a cell with triangles is valid: all inside the grid)
        unsigned inside = 0;
        for (int e = 0; e < 8; ++e) {
            cn[e] = e == 0 ? n : st.neighbour(n, i, j, k, e & 1, (e >> 1) & 1, (e >> 2) & 1);
            inside |= ((missing<Store>(cn[e]) ? 1.f : tsdf[cn[e]]) < 0.f ? 1u : 0u) << e;
        }
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
                    // the vertex's owner, corner lo: by arithmetic where every voxel is stored, else picked from cn without dynamic
                    // indexing of the register array
                    long long w = Store::kMayMiss ? -1 : st.neighbour(n, i, j, k, lo & 1, (lo >> 1) & 1, (lo >> 2) & 1);
                    if (Store::kMayMiss)
                        for (int c = 0; c < 8; ++c) w = c == lo ? cn[c] : w;
                    id[q] = missing<Store>(w) ? 0 : (int)(vofs[w] + __builtin_popcount((unsigned)code[w] & ((1u << (m - 1)) - 1u)));
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

// ------------------------------------------------------------------------------------------------------------------------------ host
// the mesh workspace of N stored voxels: code | vofs | fofs | scan scratch, each part 256-byte aligned
struct MeshWorkspace {
    unsigned short* code;
    long long *vofs, *fofs;
    void* tmp;

    // const in: mesh_emit only reads the parts (every workspace parameter of the emit kernel is const); only mesh_count writes them
    MeshWorkspace(const void* workspace, long long N) {
        char* ws = (char*)workspace;
        code = (unsigned short*)ws;
        vofs = (long long*)(ws + align256(sizeof(unsigned short) * N));
        fofs = (long long*)((char*)vofs + align256(sizeof(long long) * N));
        tmp = (char*)fofs + align256(sizeof(long long) * N);
    }
    static long long bytes(long long N) {
        return (long long)(align256(sizeof(unsigned short) * N) + 2 * align256(sizeof(long long) * N) + align256(scan_temp_bytes(N)));
    }
};

// count -> two exclusive scans -> totals [2] = (vertices, faces); the workspace holds MeshWorkspace::bytes(st.N)
template <class Store>
int mesh_count(const float* tsdf, const float* weight, const Store& st, float wth, void* workspace, long long* totals, hipStream_t s) {
    const MeshWorkspace m(workspace, st.N);
    size_t tb = scan_temp_bytes(st.N);
    hipLaunchKernelGGL(tsdf_mesh_count_kernel<Store>, dim3(grid_for(st.N)), dim3(256), 0, s, tsdf, weight, st, wth, m.code);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    rocprim::transform_iterator<const unsigned short*, VoxelCountOp, long long> vit(m.code, VoxelCountOp());
    rocprim::transform_iterator<const unsigned short*, CellCountOp, long long> fit(m.code, CellCountOp());
    if (hipcub::DeviceScan::ExclusiveSum(m.tmp, tb, vit, m.vofs, (int)st.N, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    tb = scan_temp_bytes(st.N);
    if (hipcub::DeviceScan::ExclusiveSum(m.tmp, tb, fit, m.fofs, (int)st.N, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(tsdf_mesh_totals_kernel, dim3(1), dim3(64), 0, s, m.code, m.vofs, m.fofs, st.N, totals);
    return cut3r_check_launch();
}

// emit into verts [nv,3], colors [nv,3] (or null), faces [nf,3] from the workspace mesh_count filled
template <class Store>
int mesh_emit(const float* tsdf, const float* color, const Store& st, float ox, float oy, float oz, float voxel, const void* workspace,
              float* verts, unsigned char* colors, int* faces, long long nv, long long nf, hipStream_t s) {
    if (!(voxel > 0.f) || nv < 0 || nf < 0 || nv >= (1LL << 31) || (nv > 0 && !verts) || (nf > 0 && !faces)) return CUT3R_ERR_ARG;
    if (nv == 0 && nf == 0) return CUT3R_OK;
    const MeshWorkspace m(workspace, st.N);
    hipLaunchKernelGGL(tsdf_mesh_emit_kernel<Store>, dim3(grid_for(st.N)), dim3(256), 0, s, tsdf, color, st, ox, oy, oz, voxel, m.code,
                       m.vofs, m.fofs, verts, colors, faces, nv, nf);
    return cut3r_check_launch();
}

}  // namespace
