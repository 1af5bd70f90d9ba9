// What the dense (tsdf.hip) and the sparse brick (tsdf_sparse.hip) TSDF volumes share, so that they agree bit for bit by construction:
// the per-voxel fusion of a batch of views, the marching-tetrahedra tables and the packing of the per-voxel mesh counts.  Both files are
// compiled with -ffp-contract=off; every formula here is written in one fixed order (tests/tsdf_oracle.py restates it in numpy).
#pragma once
#include <hipcub/hipcub.hpp>
#include "common.h"

#define TSDF_MAX_VIEWS 16

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

}  // namespace
