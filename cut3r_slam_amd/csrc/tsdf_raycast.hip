// Ray cast of the TSDF volumes (gfx950): depth, normal and colour images of the fused model at given poses, without a mesh.
//
// The third operation of the Open3D VoxelBlockGrid that the reference builds in tsdf_integrate.py:34 (VoxelBlockGrid.ray_cast), over the
// dense grid of tsdf.hip and the brick pool of tsdf_sparse.hip: one kernel body over the voxel stores of tsdf_voxel.h.  Compiled with
// -ffp-contract=off; every formula is written in one fixed order and tests/raycast_oracle.py restates it in numpy, bit for bit.
//
// Definition (fp32 throughout).  View b, pixel (u, v): origin c = the translation of c2w, direction d = R ((u - cx) / fx, (v - cy) / fy, 1),
// so the ray parameter is the z-depth.  Samples t_k = t_min + (float)k * step, k = 0, 1, ... while t_k <= t_max.  Per axis p = c + t_k d,
// g = (p - origin) / voxel, cell = floor(g), f = g - cell.  A sample is VALID when 0 <= cell < dim - 1 on every axis and all eight
// corners of the cell are stored with weight >= weight_threshold; its value s is the trilinear interpolation of tsdf (x, then y, then z,
// each a + f (b - a)).  The march remembers one predecessor: an invalid sample forgets it, a valid one with s >= 0 becomes it, a valid one
// with s < 0 ends the ray -- as a hit at t_{k-1} + (t_k - t_{k-1}) (s_{k-1} / (s_{k-1} - s_k)) when the predecessor is there, else as a
// miss (depth 0).  Normal and colour are taken in the cell of sample k.
//
// Two accelerations, both invisible (the outputs are the plain march's bits):
//   clipping   every fp32 operation above is monotone in its varying operand, so per axis g(k) is monotone in k and the k with
//              0 <= g < dim - 1 form an interval, as do the k with t_k <= t_max.  Their ends are found by bisection ON THE SAMPLES' OWN
//              PREDICATES (no slab arithmetic whose rounding would need a margin): every k outside the intersection is invalid, and
//              invalid samples only forget the predecessor, which a march that starts at the interval's first sample does not have.
//   bricks     (brick pool) a sample whose cell's corner 0 lies in an unallocated brick is invalid.  The samples whose corner 0 lies
//              in one brick are again an interval of k; a slab estimate proposes a later sample of it, the proposal is checked by
//              evaluating that sample's brick, and only then are the samples in between -- all in that brick, all invalid -- skipped.
// Each lane keeps the slot of the brick it resolved last, so the table is read when a ray changes brick, not per sample.
//
// Launch: one thread per pixel, a wave covers an 8 x 8 pixel tile (its 64 rays walk the same bricks and end after similar trip counts), a
// workgroup of four waves 16 x 16 pixels, one view per blockIdx.z (B <= 16 views per launch).
#include "tsdf_voxel.h"

#define RAY_MAX_SAMPLES (1 << 30)

namespace {

bool dense_dims_ok(int X, int Y, int Z) { return X > 0 && Y > 0 && Z > 0 && (long long)X * Y * Z < (1LL << 31); }

SparseGrid sparse_grid(int X, int Y, int Z) { return {X, Y, Z, (X + BRICK - 1) / BRICK, (Y + BRICK - 1) / BRICK, (Z + BRICK - 1) / BRICK}; }

bool sparse_dims_ok(int X, int Y, int Z, int nb) {
    if (X <= 0 || Y <= 0 || Z <= 0 || X > (1 << 20) || Y > (1 << 20) || Z > (1 << 20)) return false;
    const SparseGrid g = sparse_grid(X, Y, Z);
    const long long T = (long long)g.BX * g.BY * g.BZ;
    return T <= (1LL << 28) && nb > 0 && nb <= T && (long long)nb * BRICK_VOXELS < (1LL << 31);
}

struct Ray {
    float c[3], d[3], o[3];
    float voxel, tmin, step;
    DEVINL float t(int k) const { return tmin + (float)k * step; }
    DEVINL float g(int a, float tk) const { return ((c[a] + tk * d[a]) - o[a]) / voxel; }
};

// the smallest k in [lo, hi) with pred(k), or hi: pred is false up to some k and true from there on
template <class P>
DEVINL int first_true(int lo, int hi, P pred) {
    while (lo < hi) {
        const int m = lo + ((hi - lo) >> 1);
        if (pred(m)) hi = m;
        else lo = m + 1;
    }
    return lo;
}

// the brick a lane resolved last: linear brick index and pool slot (-1: not allocated)
struct BrickMemo {
    int t = -1, slot = -1;
};

// where corner 0 of the cell (i, j, k) is stored, or -1
DEVINL long long cell_base(const DenseStore& st, BrickMemo&, int i, int j, int k) { return st.index(i, j, k); }
DEVINL long long cell_base(const BrickStore& st, BrickMemo& m, int i, int j, int k) {
    const int t = ((k >> 3) * st.BY + (j >> 3)) * st.BX + (i >> 3);
    if (t != m.t) {
        m.t = t;
        m.slot = st.table[t];
    }
    return m.slot < 0 ? -1 : (long long)m.slot * BRICK_VOXELS + (((k & 7) << 6) | ((j & 7) << 3) | (i & 7));
}

// a + f (b - a) along x, then y, then z over the corner values v[e] (bit 0 of e = +x, bit 1 = +y, bit 2 = +z)
DEVINL float trilinear(const float* v, float fx, float fy, float fz) {
    const float c00 = v[0] + fx * (v[1] - v[0]), c10 = v[2] + fx * (v[3] - v[2]);
    const float c01 = v[4] + fx * (v[5] - v[4]), c11 = v[6] + fx * (v[7] - v[6]);
    const float c0 = c00 + fy * (c10 - c00), c1 = c01 + fy * (c11 - c01);
    return c0 + fz * (c1 - c0);
}

// a + f (b - a) over four values in two axes: (q0, q1) along the first, (q2, q3) along the first, then those two along the second
DEVINL float bilinear(float q0, float q1, float q2, float q3, float fa, float fb) {
    const float a0 = q0 + fa * (q1 - q0), a1 = q2 + fa * (q3 - q2);
    return a0 + fb * (a1 - a0);
}

template <class Store>
__global__ __launch_bounds__(256) void tsdf_raycast_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                           const float* __restrict__ color, Store st, float ox, float oy, float oz,
                                                           float voxel, const float* __restrict__ c2w, const float* __restrict__ K, int H,
                                                           int W, float tmin, float tmax, float step, float wth, float* __restrict__ depth,
                                                           float* __restrict__ normal, unsigned char* __restrict__ rgb,
                                                           int* __restrict__ samples) {
    __shared__ float sv[16];                           // the view of this workgroup: c2w rows [12], fx fy cx cy
    const int b = blockIdx.z, tid = threadIdx.x;
    if (tid < 16) sv[tid] = tid < 12 ? c2w[b * 12 + tid] : K[b * 4 + (tid - 12)];
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const int u = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7), v = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (u >= W || v >= H) return;
    const long long HW = (long long)H * W, pix = (long long)b * HW + (long long)v * W + u;

    Ray r;
    const float xc = ((float)u - sv[14]) / sv[12], yc = ((float)v - sv[15]) / sv[13];
    for (int a = 0; a < 3; ++a) {
        r.c[a] = sv[a * 4 + 3];
        r.d[a] = (sv[a * 4] * xc + sv[a * 4 + 1] * yc) + sv[a * 4 + 2];
    }
    r.o[0] = ox, r.o[1] = oy, r.o[2] = oz;
    r.voxel = voxel, r.tmin = tmin, r.step = step;
    const float dimf[3] = {(float)(st.X - 1), (float)(st.Y - 1), (float)(st.Z - 1)};

    // clipping: the samples with t_k <= t_max are [0, kend); per axis those with 0 <= g < dim - 1 are [k0, k1)
    int k0 = 0, k1 = first_true(0, RAY_MAX_SAMPLES, [&](int k) { return !(r.t(k) <= tmax); });
    const int kend = k1;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int lo, hi;
        if (r.d[a] >= 0.f) {                           // g does not decrease with k
            lo = first_true(0, kend, [&](int k) { return r.g(a, r.t(k)) >= 0.f; });
            hi = first_true(0, kend, [&](int k) { return !(r.g(a, r.t(k)) < dimf[a]); });
        } else {                                       // g does not increase with k
            lo = first_true(0, kend, [&](int k) { return r.g(a, r.t(k)) < dimf[a]; });
            hi = first_true(0, kend, [&](int k) { return !(r.g(a, r.t(k)) >= 0.f); });
        }
        k0 = max(k0, lo);
        k1 = min(k1, hi);
    }

    BrickMemo memo;
    bool have = false, hit = false;
    float sp = 0.f, tp = 0.f, out = 0.f;
    float fr[3] = {0.f, 0.f, 0.f}, val[8];
    long long cn[8];
    int evaluated = 0;
    for (int k = k0; k < k1; ++k) {
        const float tk = r.t(k);
        float fl[3];
        bool in = true;
        for (int a = 0; a < 3; ++a) {
            const float g = r.g(a, tk);
            fl[a] = floorf(g);
            fr[a] = g - fl[a];
            in = in && fl[a] >= 0.f && fl[a] < dimf[a];
        }
        if (!in) {                                     // only for inputs that are not numbers: the clipping has removed every other such sample
            have = false;
            continue;
        }
        ++evaluated;
        const int ci = (int)fl[0], cj = (int)fl[1], ck = (int)fl[2];
        const long long n = cell_base(st, memo, ci, cj, ck);
        if (missing<Store>(n)) {
            have = false;
            // the brick of corner 0 is not allocated.  Where the ray leaves it, from the slabs of the brick's far faces; the sample two
            // before that estimate is taken only if its own corner 0 lies in this brick: then so does every sample in between
            float te = INFINITY;
            for (int a = 0; a < 3; ++a) {
                if (r.d[a] == 0.f) continue;
                const float face = floorf(fl[a] * 0.125f) * 8.f + (r.d[a] > 0.f ? 8.f : 0.f);
                te = fminf(te, ((r.o[a] + voxel * face) - r.c[a]) / r.d[a]);
            }
            const float kf = floorf((te - tmin) / step) - 2.f;
            if (kf > (float)k && kf < (float)k1) {
                const int kc = (int)kf;
                const float tc = r.t(kc);
                bool same = true;
                for (int a = 0; a < 3; ++a) same = same && floorf(floorf(r.g(a, tc)) * 0.125f) == floorf(fl[a] * 0.125f);
                if (same) k = kc;
            }
            continue;
        }
        bool ok = true;
        for (int e = 0; e < 8; ++e) {
            cn[e] = e == 0 ? n : st.neighbour(n, ci, cj, ck, e & 1, (e >> 1) & 1, (e >> 2) & 1);
            ok = ok && !missing<Store>(cn[e]);
        }
        if (ok) {
            float w[8];
            for (int e = 0; e < 8; ++e) w[e] = weight[cn[e]];            // eight independent loads, then one verdict
            for (int e = 0; e < 8; ++e) ok = ok && w[e] >= wth;
        }
        if (!ok) {
            have = false;
            continue;
        }
        for (int e = 0; e < 8; ++e) val[e] = tsdf[cn[e]];
        const float s = trilinear(val, fr[0], fr[1], fr[2]);
        if (s < 0.f) {
            if (have) {
                out = tp + (tk - tp) * (sp / (sp - s));
                hit = true;
            }
            break;
        }
        have = true;
        sp = s;
        tp = tk;
    }

    depth[pix] = out;
    if (samples) samples[pix] = evaluated;
    if (normal) {
        float nx = 0.f, ny = 0.f, nz = 0.f;
        if (hit) {
            // the gradient of the trilinear interpolant: the four differences along an axis, interpolated in the other two (lower axis first)
            const float gx = bilinear(val[1] - val[0], val[3] - val[2], val[5] - val[4], val[7] - val[6], fr[1], fr[2]);
            const float gy = bilinear(val[2] - val[0], val[3] - val[1], val[6] - val[4], val[7] - val[5], fr[0], fr[2]);
            const float gz = bilinear(val[4] - val[0], val[5] - val[1], val[6] - val[2], val[7] - val[3], fr[0], fr[1]);
            const float len = sqrtf((gx * gx + gy * gy) + gz * gz);
            if (len > 0.f) nx = gx / len, ny = gy / len, nz = gz / len;
        }
        normal[pix * 3] = nx;
        normal[pix * 3 + 1] = ny;
        normal[pix * 3 + 2] = nz;
    }
    if (rgb) {
        for (int a = 0; a < 3; ++a) {
            unsigned char q = 0;
            if (hit) {
                float cv[8];
                for (int e = 0; e < 8; ++e) cv[e] = color[a * st.N + cn[e]];
                const float c = floorf(trilinear(cv, fr[0], fr[1], fr[2]) + 0.5f);
                q = (unsigned char)fminf(255.f, fmaxf(0.f, c));
            }
            rgb[(long long)b * 3 * HW + a * HW + (long long)v * W + u] = q;
        }
    }
}

bool cast_ok(const float* tsdf, const float* weight, const float* color, const float* c2w, const float* K, int B, int H, int W, float voxel,
             float tmin, float tmax, float step, const float* depth) {
    if (!tsdf || !weight || !color || !c2w || !K || !depth || B < 1 || B > TSDF_MAX_VIEWS || H <= 0 || W <= 0) return false;
    return voxel > 0.f && step > 0.f && tmin >= 0.f && tmax >= tmin && (long long)B * H * W < (1LL << 31);
}

template <class Store>
int ray_cast(const float* tsdf, const float* weight, const float* color, const Store& st, float ox, float oy, float oz, float voxel,
             const float* c2w, const float* K, int B, int H, int W, float tmin, float tmax, float step, float wth, float* depth,
             float* normal, unsigned char* rgb, int* samples, hipStream_t s) {
    const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16), (unsigned)B);
    if (grid.y > 65535u) return CUT3R_ERR_ARG;
    hipLaunchKernelGGL(tsdf_raycast_kernel<Store>, grid, dim3(256), 0, s, tsdf, weight, color, st, ox, oy, oz, voxel, c2w, K, H, W, tmin,
                       tmax, step, wth, depth, normal, rgb, samples);
    return cut3r_check_launch();
}

}  // namespace

extern "C" int cut3r_tsdf_ray_cast(const float* tsdf, const float* weight, const float* color, int X, int Y, int Z, float ox, float oy,
                                   float oz, float voxel, const float* c2w, const float* K, int B, int H, int W, float t_min, float t_max,
                                   float step, float weight_threshold, float* depth, float* normal, unsigned char* rgb, int* samples,
                                   void* stream) {
    if (!dense_dims_ok(X, Y, Z) || !cast_ok(tsdf, weight, color, c2w, K, B, H, W, voxel, t_min, t_max, step, depth)) return CUT3R_ERR_ARG;
    const DenseStore st = {X, Y, Z, (long long)X * Y, (long long)X * Y * Z};
    return ray_cast(tsdf, weight, color, st, ox, oy, oz, voxel, c2w, K, B, H, W, t_min, t_max, step, weight_threshold, depth, normal, rgb,
                    samples, (hipStream_t)stream);
}

extern "C" int cut3r_tsdf_sparse_ray_cast(const float* tsdf, const float* weight, const float* color, const int* table, const int* bricks,
                                          int nb, int X, int Y, int Z, float ox, float oy, float oz, float voxel, const float* c2w,
                                          const float* K, int B, int H, int W, float t_min, float t_max, float step, float weight_threshold,
                                          float* depth, float* normal, unsigned char* rgb, int* samples, void* stream) {
    if (!table || !bricks || !sparse_dims_ok(X, Y, Z, nb)) return CUT3R_ERR_ARG;
    if (!cast_ok(tsdf, weight, color, c2w, K, B, H, W, voxel, t_min, t_max, step, depth)) return CUT3R_ERR_ARG;
    const BrickStore st = {sparse_grid(X, Y, Z), table, bricks, (long long)nb * BRICK_VOXELS};
    return ray_cast(tsdf, weight, color, st, ox, oy, oz, voxel, c2w, K, B, H, W, t_min, t_max, step, weight_threshold, depth, normal, rgb,
                    samples, (hipStream_t)stream);
}
