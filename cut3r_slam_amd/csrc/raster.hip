// Depth (and face-id) images of a triangle mesh on gfx950, B <= 16 views per launch, and the small kernels of the 2-D depth-L1 mesh
// metric around it.  They replace the off-screen Open3D/OpenGL window of the reference's scripts/eval_recon.py:138-223 (calc_2d_metric)
// and its check_proj (:60-89); the vertex-visibility kernel has no reference counterpart (the reference reads culled GT meshes made by
// an outside script).
//
// The pixel rule (tests/raster_oracle.py restates it bit for bit; the file is compiled with -ffp-contract=off and every formula below is
// written in one fixed order):
//   camera space   p_c = ((T0 x + T1 y) + T2 z) + T3 per row of w2c in fp32, as recon.hip transforms a query
//   ray            d = (rx[j], ry[i], 1), rx[j] = (float(j) - cx) / fx, ry[i] = (float(i) - cy) / fy in fp32 (pixel centres at integers)
// and from these fp32 values on in fp64:
//   cross          (p x q) = (py qz - pz qy, pz qx - px qz, px qy - py qx): q x p is exactly -(p x q)
//   normals        n0 = b x c, n1 = c x a, n2 = a x b;   det = (ax n0x + ay n0y) + az n0z
//   edge values    e_k = (rx n_kx + ry n_ky) + n_kz
//   hit            (e0, e1, e2 all >= 0 or all <= 0), den = (e0 + e1) + e2 != 0, z = float(det / den), z_near < z <= z_far
//   candidates     a triangle with a_z, b_z, c_z all <= 0 is not drawn; with all three > 0 only the pixels lo_u <= j <= hi_u, lo_v <= i <=
//                  hi_v are tried: lo_u = floor(min u) - 1, hi_u = ceil(max u) + 1 over u = fx (x / z) + cx of the three vertices in
//                  fp32, lo_v / hi_v likewise with v = fy (y / z) + cy; any other triangle (across the camera plane): every pixel
//   pixel          the smallest z, ties to the smallest face: an unsigned 64-bit minimum of (float_bits(z) << 32) | face
// The hit test divides no vertex by its depth and nothing is clipped, so triangles that cross the camera plane are rendered where they
// are in front.  In exact arithmetic the candidate clause follows from the hit test (a hit lies inside the projected triangle, its z
// between the vertices' z); it is part of the rule because a sliver's edge values are all within rounding of 0 along its whole line, far
// beyond its ends, where a "hit" would be an artefact and where no exact cull could stop looking for one.
// Two triangles that share an edge (p, q) evaluate p x q and q x p, hence exactly negated edge values: no cracks along edges in any
// precision.  Why fp64: a pixel centre whose ray passes within rounding of a mesh VERTEX has edge values that cancel to the size of their
// own rounding error.  In fp32 (error 1e-7 of the terms, as large as the offset of the rounded ray from the vertex) their signs are noise,
// and now and then every triangle of the fan rejects the pixel: 4 holes in a 96 x 96 image of a room whose wall lattice the pixel centres
// hit (tests/test_raster_cpu.py).  The products of two fp32 values are exact in fp64, the error of an edge value drops to 1e-16 of its
// terms, eight orders below that offset, and the depth loses the fp32 cancellation of the triple products as well.
//
// Culling without changing the rule.  Rounding is monotone, so the computed e_k is a monotone function of rx (direction: the sign of
// n_kx) and of ry (sign of n_ky), and rx[j], ry[i] are non-decreasing tables (fx, fy > 0).  Over a rectangle of pixels the largest and the
// smallest computed e_k are therefore taken at two of its corners, and a rectangle holds no hit when some e_k is < 0 at its maximum (not
// all >= 0) and some e_k is > 0 at its minimum (not all <= 0).  This test is exact for the rule as computed, not only for exact
// arithmetic.  Per (triangle, view) the candidate box (the whole image for a triangle across the camera plane: that case needs nothing
// special) is split in halves along its longer side, depth first, a part is dropped when the rectangle test says so and filled pixel by pixel once it is down to LEAF_AREA
// pixels.  A part far from the triangle is dropped as soon as one edge separates it, so a triangle of a pixel or two costs some tens of
// rectangle tests and one or two leaves, whether or not it crosses the camera plane.  A thread fills at most LEAF_BUDGET leaves itself;
// after that every part still on its stack that passes the test goes to a queue as it is and is filled by one wave, 8 x 8 pixels at a
// time behind the same test (a thread whose push finds the queue full fills the part itself).  The atomic minimum makes the result
// independent of all of this.
#include "common.h"
#include "../../include/cut3r_hip.h"

namespace {

constexpr int MAX_VIEWS = 16;
constexpr int LEAF_AREA = 16;
constexpr int LEAF_BUDGET = 16;
constexpr int STACK = 40;                   // halving 65535 x 65535 pixels down to LEAF_AREA: 28 levels, one sibling kept per level
constexpr long long QUEUE_CAP = 1 << 21;
constexpr int BIG_BLOCKS = 2048;
constexpr unsigned long long EMPTY_KEY = ~0ull;

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// keys [B,H,W] u64 | rays [B, W + H] fp32 | queue counter | queue [cap] uint4 (face, view, i0 << 16 | i1, j0 << 16 | j1)
struct RasterLayout {
    size_t keys, rays, counter, queue, total;
    long long cap;
};

RasterLayout raster_layout(long long F, int B, int H, int W) {
    RasterLayout L;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align256(o + bytes); return r; };
    L.cap = F * B < QUEUE_CAP / STACK ? F * B * STACK : QUEUE_CAP;
    L.keys = take(8 * (size_t)B * H * W);
    L.rays = take(4 * (size_t)B * (W + H));
    L.counter = take(4);
    L.queue = take(16 * (size_t)L.cap);
    L.total = o;
    return L;
}

struct Tri {
    double n[3][3];     // n0 = b x c, n1 = c x a, n2 = a x b
    double det;
};

DEVINL void cam_point(const float* __restrict__ T, const float* __restrict__ p, float* o) {
    const float x = p[0], y = p[1], z = p[2];
    o[0] = ((T[0] * x + T[1] * y) + T[2] * z) + T[3];
    o[1] = ((T[4] * x + T[5] * y) + T[6] * z) + T[7];
    o[2] = ((T[8] * x + T[9] * y) + T[10] * z) + T[11];
}

DEVINL void cross3(const double* p, const double* q, double* o) {
    o[0] = p[1] * q[2] - p[2] * q[1];
    o[1] = p[2] * q[0] - p[0] * q[2];
    o[2] = p[0] * q[1] - p[1] * q[0];
}

DEVINL void tri_setup(const float* af, const float* bf, const float* cf, Tri& t) {
    const double a[3] = {(double)af[0], (double)af[1], (double)af[2]}, b[3] = {(double)bf[0], (double)bf[1], (double)bf[2]};
    const double c[3] = {(double)cf[0], (double)cf[1], (double)cf[2]};
    cross3(b, c, t.n[0]);
    cross3(c, a, t.n[1]);
    cross3(a, b, t.n[2]);
    t.det = (a[0] * t.n[0][0] + a[1] * t.n[0][1]) + a[2] * t.n[0][2];
}

DEVINL double edge_value(const double* n, float rx, float ry) { return ((double)rx * n[0] + (double)ry * n[1]) + n[2]; }

// no pixel of the rectangle rx in [x0, x1], ry in [y0, y1] (table values at its first and last column / row) can be a hit
DEVINL bool rect_empty(const Tri& t, float x0, float x1, float y0, float y1) {
    bool neg = false, pos = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double* n = t.n[k];
        const bool ux = n[0] >= 0.0, uy = n[1] >= 0.0;
        const double emax = edge_value(n, ux ? x1 : x0, uy ? y1 : y0);
        const double emin = edge_value(n, ux ? x0 : x1, uy ? y0 : y1);
        neg |= emax < 0.0;
        pos |= emin > 0.0;
    }
    return neg && pos;
}

DEVINL void pixel(const Tri& t, float rx, float ry, float z_near, float z_far, unsigned face, unsigned long long* key) {
    const double e0 = edge_value(t.n[0], rx, ry), e1 = edge_value(t.n[1], rx, ry), e2 = edge_value(t.n[2], rx, ry);
    if (!((e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0) || (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0))) return;
    const double den = (e0 + e1) + e2;
    if (!(den != 0.0)) return;
    const float z = (float)(t.det / den);
    if (!(z > z_near && z <= z_far)) return;
    const unsigned long long k = ((unsigned long long)__float_as_uint(z) << 32) | face;
    if (k < *key) atomicMin(key, k);            // keys only ever decrease: a larger candidate can be dropped without the atomic
}

DEVINL void fill_rect(const Tri& t, const float* __restrict__ rx, const float* __restrict__ ry, int i0, int i1, int j0, int j1, int W,
                      float z_near, float z_far, unsigned face, unsigned long long* kb) {
    for (int i = i0; i <= i1; ++i) {
        const float y = ry[i];
        for (int j = j0; j <= j1; ++j) pixel(t, rx[j], y, z_near, z_far, face, kb + (size_t)i * W + j);
    }
}

__global__ __launch_bounds__(256) void raster_init_kernel(unsigned long long* __restrict__ keys, long long npix, float* __restrict__ rays,
                                                          const float* __restrict__ K, int B, int H, int W, unsigned* __restrict__ counter) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t == 0) *counter = 0u;
    if (t < (long long)B * (W + H)) {
        const int b = (int)(t / (W + H)), r = (int)(t % (W + H));
        const float* k = K + 4 * b;
        rays[t] = r < W ? ((float)r - k[2]) / k[0] : ((float)(r - W) - k[3]) / k[1];
    }
    for (long long i = t; i < npix; i += (long long)gridDim.x * 256) keys[i] = EMPTY_KEY;
}

// one thread per triangle, the views in a loop (the vertices are fetched once for all of them)
__global__ __launch_bounds__(256) void raster_tri_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                         const float* __restrict__ w2c, const float* __restrict__ K, int B, int H, int W,
                                                         float z_near, float z_far, const float* __restrict__ rays,
                                                         unsigned long long* __restrict__ keys, unsigned* __restrict__ counter,
                                                         uint4* __restrict__ queue, unsigned cap) {
    __shared__ float sT[MAX_VIEWS * 16];
    if (threadIdx.x < B * 16) {
        const int b = threadIdx.x >> 4, k = threadIdx.x & 15;
        sT[threadIdx.x] = k < 12 ? w2c[12 * b + k] : K[4 * b + (k - 12)];
    }
    __syncthreads();
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
    if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) return;     // a face with an index out of range is never drawn
    float wa[3], wb[3], wc[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        wa[k] = verts[3 * (size_t)ia + k];
        wb[k] = verts[3 * (size_t)ib + k];
        wc[k] = verts[3 * (size_t)ic + k];
    }
    for (int b = 0; b < B; ++b) {
        const float* T = sT + 16 * b;
        float a[3], bb[3], c[3];
        cam_point(T, wa, a);
        cam_point(T, wb, bb);
        cam_point(T, wc, c);
        if (a[2] <= 0.f && bb[2] <= 0.f && c[2] <= 0.f) continue;
        int bi0 = 0, bi1 = H - 1, bj0 = 0, bj1 = W - 1;
        if (a[2] > 0.f && bb[2] > 0.f && c[2] > 0.f) {
            const float fx = T[12], fy = T[13], cx = T[14], cy = T[15];
            const float ua = fx * (a[0] / a[2]) + cx, ub = fx * (bb[0] / bb[2]) + cx, uc = fx * (c[0] / c[2]) + cx;
            const float va = fy * (a[1] / a[2]) + cy, vb = fy * (bb[1] / bb[2]) + cy, vc = fy * (c[1] / c[2]) + cy;
            const float ul = floorf(fminf(ua, fminf(ub, uc))) - 1.f, uh = ceilf(fmaxf(ua, fmaxf(ub, uc))) + 1.f;
            const float vl = floorf(fminf(va, fminf(vb, vc))) - 1.f, vh = ceilf(fmaxf(va, fmaxf(vb, vc))) + 1.f;
            if (!(uh >= 0.f && ul <= (float)(W - 1) && vh >= 0.f && vl <= (float)(H - 1))) continue;
            bj0 = ul <= 0.f ? 0 : (int)ul;                              // compared as floats first: a vertex next to the camera plane projects anywhere
            bj1 = uh >= (float)(W - 1) ? W - 1 : (int)uh;
            bi0 = vl <= 0.f ? 0 : (int)vl;
            bi1 = vh >= (float)(H - 1) ? H - 1 : (int)vh;
        }
        Tri t;
        tri_setup(a, bb, c, t);
        if (!(t.det != 0.0)) continue;                                  // z = +-0 / den or NaN: never in (z_near, z_far]
        const float* rx = rays + (size_t)b * (W + H);
        const float* ry = rx + W;
        if (rect_empty(t, rx[bj0], rx[bj1], ry[bi0], ry[bi1])) continue;
        unsigned long long* kb = keys + (size_t)b * H * W;
        uint2 stack[STACK];                                             // (i0 << 16 | i1, j0 << 16 | j1), already past the rectangle test
        int sp = 0, budget = LEAF_BUDGET;
        stack[sp++] = make_uint2(((unsigned)bi0 << 16) | (unsigned)bi1, ((unsigned)bj0 << 16) | (unsigned)bj1);
        while (sp > 0) {
            const uint2 r = stack[--sp];
            const int i0 = (int)(r.x >> 16), i1 = (int)(r.x & 0xFFFFu), j0 = (int)(r.y >> 16), j1 = (int)(r.y & 0xFFFFu);
            const int h = i1 - i0 + 1, w = j1 - j0 + 1;
            const bool leaf = h * w <= LEAF_AREA;
            if (leaf ? budget > 0 : budget > 0 && sp + 2 <= STACK) {
                if (leaf) {
                    --budget;
                    fill_rect(t, rx, ry, i0, i1, j0, j1, W, z_near, z_far, (unsigned)f, kb);
                    continue;
                }
                if (h >= w) {                                           // halves of the longer side, each kept only if it may hold a hit
                    const int m = i0 + (h >> 1);
                    if (!rect_empty(t, rx[j0], rx[j1], ry[m], ry[i1])) stack[sp++] = make_uint2(((unsigned)m << 16) | (unsigned)i1, r.y);
                    if (!rect_empty(t, rx[j0], rx[j1], ry[i0], ry[m - 1])) stack[sp++] = make_uint2(((unsigned)i0 << 16) | (unsigned)(m - 1), r.y);
                } else {
                    const int m = j0 + (w >> 1);
                    if (!rect_empty(t, rx[m], rx[j1], ry[i0], ry[i1])) stack[sp++] = make_uint2(r.x, ((unsigned)m << 16) | (unsigned)j1);
                    if (!rect_empty(t, rx[j0], rx[m - 1], ry[i0], ry[i1])) stack[sp++] = make_uint2(r.x, ((unsigned)j0 << 16) | (unsigned)(m - 1));
                }
                continue;
            }
            const unsigned q = atomicAdd(counter, 1u);                  // out of budget: the part goes to the waves of raster_big_kernel
            if (q < cap) queue[q] = make_uint4((unsigned)f, (unsigned)b, r.x, r.y);
            else fill_rect(t, rx, ry, i0, i1, j0, j1, W, z_near, z_far, (unsigned)f, kb);
        }
    }
}

// one wave per queued part of a (triangle, view): the rectangle in tiles of 8 x 8 pixels, one lane per pixel, a tile skipped when the
// rectangle test says so
__global__ __launch_bounds__(256) void raster_big_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                         const float* __restrict__ w2c, int H, int W, float z_near, float z_far,
                                                         const float* __restrict__ rays, unsigned long long* __restrict__ keys,
                                                         const unsigned* __restrict__ counter, const uint4* __restrict__ queue, unsigned cap) {
    const unsigned n = min(*counter, cap);
    const int lane = threadIdx.x & 63;
    const int li = lane >> 3, lj = lane & 7;
    for (unsigned q = blockIdx.x * 4 + (threadIdx.x >> 6); q < n; q += gridDim.x * 4) {
        const uint4 e = queue[q];
        const int f = (int)e.x, b = (int)e.y;
        const int i0 = (int)(e.z >> 16), i1 = (int)(e.z & 0xFFFFu), j0 = (int)(e.w >> 16), j1 = (int)(e.w & 0xFFFFu);
        const float* T = w2c + 12 * b;
        float a[3], bb[3], c[3];
        cam_point(T, verts + 3 * (size_t)faces[3 * (size_t)f], a);
        cam_point(T, verts + 3 * (size_t)faces[3 * (size_t)f + 1], bb);
        cam_point(T, verts + 3 * (size_t)faces[3 * (size_t)f + 2], c);
        Tri t;
        tri_setup(a, bb, c, t);
        const float* rx = rays + (size_t)b * (W + H);
        const float* ry = rx + W;
        unsigned long long* kb = keys + (size_t)b * H * W;
        for (int ti = i0; ti <= i1; ti += 8)
            for (int tj = j0; tj <= j1; tj += 8) {
                const int te = min(ti + 7, i1), tf = min(tj + 7, j1);
                if (rect_empty(t, rx[tj], rx[tf], ry[ti], ry[te])) continue;
                const int i = ti + li, j = tj + lj;
                if (i <= te && j <= tf) pixel(t, rx[j], ry[i], z_near, z_far, (unsigned)f, kb + (size_t)i * W + j);
            }
    }
}

__global__ __launch_bounds__(256) void raster_resolve_kernel(const unsigned long long* __restrict__ keys, long long npix,
                                                             float* __restrict__ depth, int* __restrict__ face_id) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long long)gridDim.x * 256) {
        const unsigned long long k = keys[i];
        const bool hit = k != EMPTY_KEY;
        depth[i] = hit ? __uint_as_float((unsigned)(k >> 32)) : 0.f;
        if (face_id) face_id[i] = hit ? (int)(unsigned)(k & 0xFFFFFFFFull) : -1;
    }
}

// -------------------------------------------------------------------------------------------------------------------- depth L1
// per view over the pixels with ours > 0: [0] their number, [1] sum |gt - ours|, both fp64.  L1_BLOCKS grid-stride blocks per view; per
// block a wave butterfly and the four waves in order; the blocks folded in order by one thread per view: the same bits on every run.
constexpr int L1_BLOCKS = 64;

__global__ __launch_bounds__(256) void depth_l1_kernel(const float* __restrict__ gt, const float* __restrict__ ours, int HW,
                                                       double* __restrict__ part) {
    __shared__ double sm[4][2];
    const int b = blockIdx.y;
    const float* g = gt + (size_t)b * HW;
    const float* o = ours + (size_t)b * HW;
    double cnt = 0.0, sum = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += L1_BLOCKS * 256) {
        const float v = o[i];
        if (v > 0.f) {
            cnt += 1.0;
            sum += fabs((double)g[i] - (double)v);
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        cnt += __shfl_xor(cnt, s, 64);
        sum += __shfl_xor(sum, s, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sm[threadIdx.x >> 6][0] = cnt;
        sm[threadIdx.x >> 6][1] = sum;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int k = threadIdx.x;
        part[((size_t)b * L1_BLOCKS + blockIdx.x) * 2 + k] = ((sm[0][k] + sm[1][k]) + sm[2][k]) + sm[3][k];
    }
}

__global__ void depth_l1_fold_kernel(const double* __restrict__ part, int B, double* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * B) return;
    const int b = t >> 1, k = t & 1;
    double s = 0.0;
    for (int i = 0; i < L1_BLOCKS; ++i) s += part[((size_t)b * L1_BLOCKS + i) * 2 + k];
    out[t] = s;
}

// ------------------------------------------------------------------------------------------------------------- points in view
// the reference's check_proj with its flips cancelled: p_c as above, z' = z - 1e-5, u = (fx x + cx z) / z', v = (fy y + cy z) / z', counted
// when 0 <= z', edge < u < W - edge and edge < v < H - edge.  Integer counts: the order of the atomics does not matter.
__global__ __launch_bounds__(256) void points_in_view_kernel(const float* __restrict__ pts, int N, const float* __restrict__ w2c,
                                                             const float* __restrict__ K, int B, float W, float H, float edge,
                                                             int* __restrict__ counts) {
    __shared__ float sT[MAX_VIEWS * 16];
    if (threadIdx.x < B * 16) {
        const int b = threadIdx.x >> 4, k = threadIdx.x & 15;
        sT[threadIdx.x] = k < 12 ? w2c[12 * b + k] : K[4 * b + (k - 12)];
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    float p[3] = {0.f, 0.f, 0.f};
    if (i < N) {
        p[0] = pts[3 * (size_t)i];
        p[1] = pts[3 * (size_t)i + 1];
        p[2] = pts[3 * (size_t)i + 2];
    }
    for (int b = 0; b < B; ++b) {
        const float* T = sT + 16 * b;
        float c[3];
        cam_point(T, p, c);
        const float zz = c[2] - 1e-5f;
        const float u = (T[12] * c[0] + T[14] * c[2]) / zz, v = (T[13] * c[1] + T[15] * c[2]) / zz;
        const bool in = i < N && 0.f <= zz && u < W - edge && u > edge && v < H - edge && v > edge;
        const unsigned long long m = __ballot(in);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(counts + b, __popcll(m));
    }
}

// ------------------------------------------------------------------------------------------------------------- vertex visibility
// flags[v] |= 1 when in some view the vertex lies at 0 < z <= z_far, its nearest pixel (floor(u + 0.5), u = fx (x / z) + cx) is inside the
// image and the mesh's own depth d there does not hide it: d == 0 (nothing drawn) or z <= d + eps
__global__ __launch_bounds__(256) void vertex_visible_kernel(const float* __restrict__ verts, int V, const float* __restrict__ depth,
                                                             const float* __restrict__ w2c, const float* __restrict__ K, int B, int H, int W,
                                                             float eps, float z_far, unsigned char* __restrict__ flags) {
    __shared__ float sT[MAX_VIEWS * 16];
    if (threadIdx.x < B * 16) {
        const int b = threadIdx.x >> 4, k = threadIdx.x & 15;
        sT[threadIdx.x] = k < 12 ? w2c[12 * b + k] : K[4 * b + (k - 12)];
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    if (flags[i]) return;
    const float* p = verts + 3 * (size_t)i;
    for (int b = 0; b < B; ++b) {
        const float* T = sT + 16 * b;
        float c[3];
        cam_point(T, p, c);
        if (!(c[2] > 0.f && c[2] <= z_far)) continue;
        const float u = floorf((T[12] * (c[0] / c[2]) + T[14]) + 0.5f), v = floorf((T[13] * (c[1] / c[2]) + T[15]) + 0.5f);
        if (!(u >= 0.f && u <= (float)(W - 1) && v >= 0.f && v <= (float)(H - 1))) continue;
        const float d = depth[((size_t)b * H + (int)v) * W + (int)u];
        if (d == 0.f || c[2] <= d + eps) {
            flags[i] = 1;
            return;
        }
    }
}

bool views_ok(int B, int H, int W) { return B >= 1 && B <= MAX_VIEWS && H >= 1 && W >= 1 && H <= 65535 && W <= 65535; }

}  // namespace

extern "C" long long cut3r_mesh_raster_workspace_bytes(int F, int B, int H, int W) {
    if (F <= 0 || !views_ok(B, H, W)) return -1;
    return (long long)raster_layout(F, B, H, W).total;
}

extern "C" int cut3r_mesh_raster(const float* verts, int V, const int* faces, int F, const float* w2c, const float* K, int B, int H, int W,
                                 float z_near, float z_far, float* depth, int* face_id, void* workspace, long long workspace_bytes,
                                 void* stream) {
    if (!verts || !faces || !w2c || !K || !depth || !workspace || V <= 0 || F <= 0 || !views_ok(B, H, W)) return CUT3R_ERR_ARG;
    if (!(z_near >= 0.f) || !(z_far > z_near)) return CUT3R_ERR_ARG;
    if (workspace_bytes < cut3r_mesh_raster_workspace_bytes(F, B, H, W)) return CUT3R_ERR_ARG;
    const RasterLayout L = raster_layout(F, B, H, W);
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)workspace;
    unsigned long long* keys = (unsigned long long*)(w + L.keys);
    float* rays = (float*)(w + L.rays);
    unsigned* counter = (unsigned*)(w + L.counter);
    uint4* queue = (uint4*)(w + L.queue);
    const long long npix = (long long)B * H * W;
    const long long need = npix > (long long)B * (W + H) ? npix : (long long)B * (W + H);
    const long long gb = (need + 255) / 256;
    const unsigned fill = (unsigned)(gb < 65536 ? gb : 65536);
    hipLaunchKernelGGL(raster_init_kernel, dim3(fill), dim3(256), 0, s, keys, npix, rays, K, B, H, W, counter);
    hipLaunchKernelGGL(raster_tri_kernel, dim3((F + 255) / 256), dim3(256), 0, s, verts, V, faces, F, w2c, K, B, H, W, z_near, z_far, rays, keys,
                       counter, queue, (unsigned)L.cap);
    hipLaunchKernelGGL(raster_big_kernel, dim3(BIG_BLOCKS), dim3(256), 0, s, verts, faces, w2c, H, W, z_near, z_far, rays, keys, counter, queue,
                       (unsigned)L.cap);
    hipLaunchKernelGGL(raster_resolve_kernel, dim3(fill), dim3(256), 0, s, keys, npix, depth, face_id);
    return cut3r_check_launch();
}

extern "C" long long cut3r_depth_l1_workspace_bytes(int B) {
    if (B <= 0) return -1;
    return (long long)(sizeof(double) * 2 * L1_BLOCKS * (size_t)B);
}

extern "C" int cut3r_depth_l1(const float* gt, const float* ours, int B, int H, int W, double* out, void* workspace, long long workspace_bytes,
                              void* stream) {
    if (!gt || !ours || !out || !workspace || B <= 0 || B > 65535 || H <= 0 || W <= 0 || (long long)H * W >= (1ll << 31)) return CUT3R_ERR_ARG;
    if (workspace_bytes < cut3r_depth_l1_workspace_bytes(B)) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)workspace;
    hipLaunchKernelGGL(depth_l1_kernel, dim3(L1_BLOCKS, B), dim3(256), 0, s, gt, ours, H * W, part);
    hipLaunchKernelGGL(depth_l1_fold_kernel, dim3((2 * B + 255) / 256), dim3(256), 0, s, part, B, out);
    return cut3r_check_launch();
}

extern "C" int cut3r_points_in_view(const float* points, int N, const float* w2c, const float* K, int B, int H, int W, float edge, int* counts,
                                    void* stream) {
    if (!points || !w2c || !K || !counts || N <= 0 || !views_ok(B, H, W) || !(edge >= 0.f)) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, sizeof(int) * (size_t)B, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(points_in_view_kernel, dim3((N + 255) / 256), dim3(256), 0, s, points, N, w2c, K, B, (float)W, (float)H, edge, counts);
    return cut3r_check_launch();
}

extern "C" int cut3r_mesh_vertex_visible(const float* verts, int V, const float* depth, const float* w2c, const float* K, int B, int H, int W,
                                         float eps, float z_far, unsigned char* flags, void* stream) {
    if (!verts || !depth || !w2c || !K || !flags || V <= 0 || !views_ok(B, H, W) || !(eps >= 0.f) || !(z_far > 0.f)) return CUT3R_ERR_ARG;
    hipLaunchKernelGGL(vertex_visible_kernel, dim3((V + 255) / 256), dim3(256), 0, (hipStream_t)stream, verts, V, depth, w2c, K, B, H, W, eps,
                       z_far, flags);
    return cut3r_check_launch();
}
