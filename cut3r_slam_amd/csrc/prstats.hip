// Precision / recall / F-score of a reconstruction on gfx950: the reductions that turn the nearest-neighbour squared distances of
// csrc/recon.hip into the numbers of the Tanks-and-Temples evaluation (counts under a threshold, mean, min, max, cumulative histogram,
// median), and the moments of a point-to-point ICP update WITH scale.  Compiled with -ffp-contract=off; tests/pr_oracle.py restates every
// result bit for bit.  Each kernel streams dist2 (4 Q bytes) once per pass.
//
// dist_stats.  Entry s = dist2[i] is BAD iff !(s >= 0) || s == +inf (NaN, negative, +inf: what cut3r_nn_query leaves for a query without a
// neighbour); a bad entry bumps counts[2] and nothing else.  A good entry has d = fabs(sqrt((double)s)) (IEEE fp64 sqrt; the fabs only
// turns the -0 of s = -0.0 into +0) and
//     counts[0]++;  counts[1]++ iff d < tau (strict);  moments = (sum d, sum (double)s, min d, max d);
//     hist[k]++ for the largest integer k with (double)k * bin_width <= d, iff k < nbins.
// Without a good entry min = +inf and max = -inf.  The histogram is np.histogram(d, np.arange(0, nbins + 1) * bin_width) except for
// numpy's closed last edge: d == nbins * bin_width is dropped here (numpy puts it into the last bin).
// Order of the two fp64 sums (counts, histogram, min and max do not depend on any order): G = min(ceil(Q / 1024), 1024) workgroups of 256
// threads; thread t of workgroup b owns, for k = 0, 1, ..., the four entries 4 ((k G + b) 256 + t) + j, j = 0..3, and adds the good ones
// among them to its sum in increasing (k, j), starting from +0; the 256 thread sums are folded by the halving tree s[t] += s[t + o], o =
// 128, 64, ..., 1; the G workgroup sums are added in increasing b, starting from +0.  The same bits on every run, for every alignment of
// dist2 (an aligned quad is one 16-byte load, anything else four 4-byte loads of the same entries).
// The histogram is counted in LDS with integer atomics and added to hist (zeroed by a memset on the stream) with integer atomics; no
// floating-point atomic anywhere.  One memset, one pass over dist2, one workgroup that folds the partials.  Nothing is read back.
//
// dist_median.  The dist2 values of ascending ranks (n - 1) / 2 and n / 2 among the n good entries (-0.0 as +0.0), NaN when n == 0: the
// radix select of csrc/calib.hip (four 8-bit passes, most significant first, over the uint32 image of the float, which for a non-negative
// float is its bit pattern), with both ranks followed in the same passes: pass 0 fills one 256-bin table, from which n and both first
// digits follow; passes 1..3 fill one table per rank, each counting the entries that carry that rank's chosen digits.  Every workgroup of
// a pass re-derives the chosen digits from the tables of the passes before it.  Integer counts: exact in any arrival order.
//
// icp_moments_scaled.  out[0..16] are cut3r_icp_moments' (the same grid, the same order of every sum: csrc/recon.hip is restated here, and
// tests/test_pr_gpu.py holds the two to the same bits); out[17] = sum of ((double)x (double)x + (double)y (double)y) + (double)z (double)z
// over the same correspondences in the same order, (x, y, z) the fp32 source point under T: what Umeyama's scale divides by.
#include <stdint.h>
#include "common.h"
#include "../../include/cut3r_hip.h"

namespace {

constexpr int T = 256;                    // threads per workgroup
constexpr int MAX_BLOCKS = 1024;
constexpr int MAX_BINS = 4096;

int stream_blocks(int Q) {
    const int b = (int)(((long long)Q + 4 * T - 1) / (4 * T));
    return b < MAX_BLOCKS ? b : MAX_BLOCKS;
}

DEVINL bool good_entry(float s) { return s >= 0.0f && s != __builtin_inff(); }

// the four entries of quad q (entries 4 q .. 4 q + 3); n = how many of them exist
DEVINL int load_quad(const float* __restrict__ dist2, bool aligned, long long q, int Q, float v[4]) {
    const long long i = 4 * q;
    if (aligned && i + 3 < Q) {
        const float4 f = *reinterpret_cast<const float4*>(dist2 + i);
        v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        return 4;
    }
    int n = 0;
    for (int j = 0; j < 4; j++)
        if (i + j < Q) v[n++] = dist2[i + j];
    return n;
}

// -------------------------------------------------------------------------------------------------------------------- dist_stats
struct StatsPartial {                     // one per workgroup
    double sum_d, sum_s, min_d, max_d;
    long long good, below, bad;
};

__global__ __launch_bounds__(T) void dist_stats_kernel(const float* __restrict__ dist2, int Q, double tau, double w, int nbins,
                                                       unsigned* __restrict__ hist, StatsPartial* __restrict__ part) {
    __shared__ unsigned lh[MAX_BINS];
    __shared__ double sa[T], sb[T], smin[T], smax[T];
    __shared__ unsigned sgood[T], sbelow[T], sbad[T];
    const int t = threadIdx.x;
    for (int k = t; k < nbins; k += T) lh[k] = 0;
    __syncthreads();
    const bool aligned = ((uintptr_t)dist2 & 15u) == 0;
    const double top = (double)nbins * w;                          // d >= top: no bin below nbins
    const double inv_w = 1.0 / w;
    double A = 0.0, B = 0.0, lo = __builtin_inf(), hi = -__builtin_inf();
    unsigned good = 0, below = 0, bad = 0;                         // a thread sees at most 2^31 / 256 entries
    const long long nquads = ((long long)Q + 3) / 4;
    auto take = [&](float s) {
        if (!good_entry(s)) {
            bad++;
            return;
        }
        const double d = fabs(sqrt((double)s));
        good++;
        if (d < tau) below++;
        A += d;
        B += (double)s;
        lo = fmin(lo, d);
        hi = fmax(hi, d);
        if (d < top) {                                             // so d / w < nbins + 1: the quotient fits an int
            const double guess = d * inv_w;                        // within one of the bin (no fp64 division per entry); the
            int k = guess < (double)nbins ? (int)guess : nbins - 1;            // two loops below settle it by the rule itself
            k = k < nbins - 1 ? k : nbins - 1;
            while (k + 1 < nbins && (double)(k + 1) * w <= d) k++;
            while (k > 0 && (double)k * w > d) k--;
            atomicAdd(&lh[k], 1u);
        }
    };
    for (long long q = (long long)blockIdx.x * T + t; q < nquads; q += (long long)gridDim.x * T) {
        float v[4];
        const int m = load_quad(dist2, aligned, q, Q, v);
        for (int j = 0; j < m; j++) take(v[j]);
    }
    sa[t] = A, sb[t] = B, smin[t] = lo, smax[t] = hi;
    sgood[t] = good, sbelow[t] = below, sbad[t] = bad;
    __syncthreads();
    for (int o = T / 2; o > 0; o >>= 1) {
        if (t < o) {
            sa[t] += sa[t + o];
            sb[t] += sb[t + o];
            smin[t] = fmin(smin[t], smin[t + o]);
            smax[t] = fmax(smax[t], smax[t + o]);
            sgood[t] += sgood[t + o];                              // a workgroup sees at most 2^31 / G < 2^32 entries
            sbelow[t] += sbelow[t + o];
            sbad[t] += sbad[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        StatsPartial p;
        p.sum_d = sa[0], p.sum_s = sb[0], p.min_d = smin[0], p.max_d = smax[0];
        p.good = sgood[0], p.below = sbelow[0], p.bad = sbad[0];
        part[blockIdx.x] = p;
    }
    for (int k = t; k < nbins; k += T)
        if (lh[k] != 0) atomicAdd(&hist[k], lh[k]);
}

// one workgroup: the partials are staged in LDS by all threads, then thread 0 adds the sum d and thread 64 (another wave) the sum s in
// increasing workgroup order; the order-free quantities are folded by a tree
__global__ __launch_bounds__(T) void dist_stats_fold_kernel(const StatsPartial* __restrict__ part, int nblk, long long* __restrict__ counts,
                                                            double* __restrict__ moments) {
    __shared__ double pa[MAX_BLOCKS], pb[MAX_BLOCKS];
    __shared__ double smin[T], smax[T];
    __shared__ long long sgood[T], sbelow[T], sbad[T];
    const int t = threadIdx.x;
    double lo = __builtin_inf(), hi = -__builtin_inf();
    long long good = 0, below = 0, bad = 0;
    for (int b = t; b < MAX_BLOCKS; b += T) {
        if (b >= nblk) {
            pa[b] = 0.0, pb[b] = 0.0;                              // +0 leaves a sum of non-negative terms as it is
            continue;
        }
        const StatsPartial p = part[b];
        pa[b] = p.sum_d, pb[b] = p.sum_s;
        lo = fmin(lo, p.min_d), hi = fmax(hi, p.max_d);
        good += p.good, below += p.below, bad += p.bad;
    }
    smin[t] = lo, smax[t] = hi, sgood[t] = good, sbelow[t] = below, sbad[t] = bad;
    __syncthreads();
    for (int o = T / 2; o > 0; o >>= 1) {
        if (t < o) {
            smin[t] = fmin(smin[t], smin[t + o]);
            smax[t] = fmax(smax[t], smax[t + o]);
            sgood[t] += sgood[t + o];
            sbelow[t] += sbelow[t + o];
            sbad[t] += sbad[t + o];
        }
        __syncthreads();
    }
    if (t == 0 || t == 64) {
        const double* p = t == 0 ? pa : pb;
        double s = 0.0;
        for (int b = 0; b < nblk; b += 16) {                       // sixteen independent LDS reads, then the sixteen adds in order
            double v[16];
#pragma unroll
            for (int j = 0; j < 16; j++) v[j] = p[b + j];
#pragma unroll
            for (int j = 0; j < 16; j++) s += v[j];
        }
        moments[t == 0 ? 0 : 1] = s;
    }
    if (t == 128) {
        moments[2] = smin[0], moments[3] = smax[0];
        counts[0] = sgood[0], counts[1] = sbelow[0], counts[2] = sbad[0];
    }
}

// ------------------------------------------------------------------------------------------------------------------- dist_median
// tables: [7][256] unsigned: table 0 = pass 0 (both ranks), 1 + 3 r + (j - 1) = pass j >= 1 of rank r.  While the two ranks have chosen the
// same digits in every pass before j (for a large n: nearly always), pass j counts once, into rank 0's table, and rank 1 reads that.
constexpr int MED_TABLES = 7;

DEVINL const unsigned* med_table(const unsigned* tables, int r, int j) { return tables + 256 * (j == 0 ? 0 : 1 + 3 * r + (j - 1)); }

// The state in front of pass `pass`: for both ranks the chosen digits (prefix, in the top 8 pass bits) and the rank of the wanted entry
// among those that carry them; n = the good entries.  All T threads call it and get the same values; s [6] is scratch.  The inclusive
// scan of a table's 256 bins: a shuffle scan inside each of the four waves, then the wave totals through LDS.
DEVINL void med_state(const unsigned* __restrict__ tables, int pass, unsigned* s, unsigned prefix[2], unsigned rank[2], unsigned& n) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    n = 0;
    for (int r = 0; r < 2; r++) {
        prefix[r] = 0, rank[r] = 0;
        for (int j = 0; j < pass; j++) {
            const bool shared = j == 0 || (prefix[r] >> (32 - 8 * j)) == (prefix[0] >> (32 - 8 * j));
            const unsigned c = med_table(tables, shared ? 0 : r, j)[t];
            unsigned inc = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned up = __shfl_up(inc, o, 64);
                if (lane >= o) inc += up;
            }
            __syncthreads();                               // the scratch of the round before has been read
            if (lane == 63) s[wave] = inc;
            if (t == 0) s[4] = 0, s[5] = 0;
            __syncthreads();
            const unsigned total = ((s[0] + s[1]) + s[2]) + s[3];
            for (int w = 0; w < wave; w++) inc += s[w];
            if (j == 0) {
                n = total;
                rank[r] = n > 0 ? (r == 0 ? (n - 1) / 2 : n / 2) : 0;
            }
            if (total > 0 && inc - c <= rank[r] && rank[r] < inc) s[4] = (unsigned)t, s[5] = rank[r] - (inc - c);
            __syncthreads();
            prefix[r] |= s[4] << (24 - 8 * j);
            rank[r] = s[5];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(T) void dist_median_pass_kernel(const float* __restrict__ dist2, int Q, int pass, unsigned* __restrict__ tables) {
    __shared__ unsigned lh[2][256];
    __shared__ unsigned scratch[6];
    const int t = threadIdx.x;
    unsigned prefix[2], rank[2], n;
    med_state(tables, pass, scratch, prefix, rank, n);
    if (pass > 0 && n == 0) return;
    lh[0][t] = 0, lh[1][t] = 0;
    __syncthreads();
    const bool aligned = ((uintptr_t)dist2 & 15u) == 0;
    const int high = 32 - 8 * pass, shift = 24 - 8 * pass;         // bits above the digit of this pass are [high, 32)
    const long long nquads = ((long long)Q + 3) / 4;
    // a thread keeps the digit it saw last and how often in a row: the top digit of a distance is its exponent, nearly the same for
    // all entries, and one LDS atomic per run instead of one per entry keeps 64 lanes from queueing on two or three addresses
    unsigned run_digit[2] = {0, 0}, run_n[2] = {0, 0};
    const int nr = pass == 0 || (prefix[0] >> high) == (prefix[1] >> high) ? 1 : 2;
    auto take = [&](float s) {
        if (!good_entry(s)) return;
        const unsigned key = __float_as_uint(s) & 0x7fffffffu;                 // -0.0 as +0.0
        const unsigned digit = (key >> shift) & 255u;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            if (r >= nr || (pass != 0 && (key >> high) != (prefix[r] >> high))) continue;
            if (digit == run_digit[r]) {
                run_n[r]++;
            } else {
                if (run_n[r] != 0) atomicAdd(&lh[r][run_digit[r]], run_n[r]);
                run_digit[r] = digit, run_n[r] = 1;
            }
        }
    };
    for (long long q = (long long)blockIdx.x * T + t; q < nquads; q += (long long)gridDim.x * T) {
        float v[4];
        const int m = load_quad(dist2, aligned, q, Q, v);
        for (int j = 0; j < m; j++) take(v[j]);
    }
#pragma unroll
    for (int r = 0; r < 2; r++)
        if (run_n[r] != 0) atomicAdd(&lh[r][run_digit[r]], run_n[r]);
    __syncthreads();
    if (pass == 0) {
        if (lh[0][t] != 0) atomicAdd(&tables[t], lh[0][t]);
    } else {
        for (int r = 0; r < nr; r++)
            if (lh[r][t] != 0) atomicAdd(&tables[256 * (1 + 3 * r + (pass - 1)) + t], lh[r][t]);
    }
}

__global__ __launch_bounds__(T) void dist_median_final_kernel(const unsigned* __restrict__ tables, float* __restrict__ out) {
    __shared__ unsigned scratch[6];
    unsigned prefix[2], rank[2], n;
    med_state(tables, 4, scratch, prefix, rank, n);
    if (threadIdx.x < 2) out[threadIdx.x] = n == 0 ? __builtin_nanf("") : __uint_as_float(prefix[threadIdx.x]);
}

// --------------------------------------------------------------------------------------------------------- scaled ICP moments
// csrc/recon.hip's xform_point, icp_blocks, recon_moments_kernel and recon_moments_fold_kernel with an eighteenth moment
constexpr int NM = 18;

DEVINL void xform_point(const float* __restrict__ M, float x, float y, float z, float& ox, float& oy, float& oz) {
    if (!M) {
        ox = x; oy = y; oz = z;
        return;
    }
    ox = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
    oy = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
    oz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
}

int icp_blocks(int Q) {
    const int b = (Q + 255) / 256;
    return b < MAX_BLOCKS ? b : MAX_BLOCKS;
}

__global__ __launch_bounds__(256) void moments_scaled_kernel(const float* __restrict__ src, int Q, const float* __restrict__ ref,
                                                             const float* __restrict__ M, const float* __restrict__ dist2,
                                                             const int* __restrict__ idx, double* __restrict__ part) {
    __shared__ double sm[4][NM];
    double acc[NM];
#pragma unroll
    for (int k = 0; k < NM; ++k) acc[k] = 0.0;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < Q; i += gridDim.x * 256) {
        const int j = idx[i];
        if (j < 0) continue;
        float s[3];
        xform_point(M, src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2], s[0], s[1], s[2]);
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
        acc[17] += ((double)s[0] * (double)s[0] + (double)s[1] * (double)s[1]) + (double)s[2] * (double)s[2];
    }
#pragma unroll
    for (int k = 0; k < NM; ++k) {
        double v = acc[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        acc[k] = v;
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NM; ++k) sm[w][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < NM) {
        const int k = threadIdx.x;
        part[(size_t)blockIdx.x * NM + k] = ((sm[0][k] + sm[1][k]) + sm[2][k]) + sm[3][k];
    }
}

__global__ void moments_scaled_fold_kernel(const double* __restrict__ part, int nblk, double* __restrict__ out) {
    const int k = threadIdx.x;
    if (k >= NM) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)b * NM + k];
    out[k] = s;
}

bool misaligned8(const void* p) { return ((uintptr_t)p & 7u) != 0; }

}  // namespace

extern "C" long long cut3r_dist_stats_workspace_bytes(int Q) {
    if (Q <= 0) return -1;
    return (long long)sizeof(StatsPartial) * stream_blocks(Q);
}

extern "C" int cut3r_dist_stats(const float* dist2, int Q, double tau, double bin_width, int nbins, long long* counts, double* moments,
                                unsigned* hist, void* workspace, long long workspace_bytes, void* stream) {
    if (!dist2 || !counts || !moments || !workspace || Q <= 0 || !(tau > 0.0) || !(bin_width > 0.0)) return CUT3R_ERR_ARG;
    if (nbins < 0 || nbins > MAX_BINS || (nbins > 0 && !hist)) return CUT3R_ERR_ARG;
    if (misaligned8(workspace) || workspace_bytes < cut3r_dist_stats_workspace_bytes(Q)) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int nblk = stream_blocks(Q);
    StatsPartial* part = (StatsPartial*)workspace;
    if (nbins > 0 && hipMemsetAsync(hist, 0, sizeof(unsigned) * (size_t)nbins, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(dist_stats_kernel, dim3(nblk), dim3(T), 0, s, dist2, Q, tau, bin_width, nbins, hist, part);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(dist_stats_fold_kernel, dim3(1), dim3(T), 0, s, (const StatsPartial*)part, nblk, counts, moments);
    return cut3r_check_launch();
}

extern "C" long long cut3r_dist_median_workspace_bytes(int Q) {
    if (Q <= 0) return -1;
    return (long long)sizeof(unsigned) * 256 * MED_TABLES;
}

extern "C" int cut3r_dist_median(const float* dist2, int Q, float* out, void* workspace, long long workspace_bytes, void* stream) {
    if (!dist2 || !out || !workspace || Q <= 0) return CUT3R_ERR_ARG;
    if (misaligned8(workspace) || workspace_bytes < cut3r_dist_median_workspace_bytes(Q)) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    unsigned* tables = (unsigned*)workspace;
    if (hipMemsetAsync(tables, 0, sizeof(unsigned) * 256 * MED_TABLES, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    const int nblk = stream_blocks(Q);
    for (int pass = 0; pass < 4; pass++) {
        hipLaunchKernelGGL(dist_median_pass_kernel, dim3(nblk), dim3(T), 0, s, dist2, Q, pass, tables);
        if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(dist_median_final_kernel, dim3(1), dim3(T), 0, s, (const unsigned*)tables, out);
    return cut3r_check_launch();
}

extern "C" long long cut3r_icp_moments_scaled_workspace_bytes(int Q) {
    if (Q <= 0) return -1;
    return (long long)(sizeof(double) * NM * (size_t)icp_blocks(Q));
}

extern "C" int cut3r_icp_moments_scaled(const float* src, int Q, const float* ref, int P, const float* T34, const float* dist2, const int* idx,
                                        double* out, void* workspace, long long workspace_bytes, void* stream) {
    if (!src || !ref || !dist2 || !idx || !out || !workspace || Q <= 0 || P <= 0) return CUT3R_ERR_ARG;
    if (misaligned8(workspace) || workspace_bytes < cut3r_icp_moments_scaled_workspace_bytes(Q)) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int nblk = icp_blocks(Q);
    double* part = (double*)workspace;
    hipLaunchKernelGGL(moments_scaled_kernel, dim3(nblk), dim3(256), 0, s, src, Q, ref, T34, dist2, idx, part);
    hipLaunchKernelGGL(moments_scaled_fold_kernel, dim3(1), dim3(64), 0, s, (const double*)part, nblk, out);
    return cut3r_check_launch();
}
