"""numpy fp64 restatement of csrc/prstats.hip and of the precision / recall pipeline of cut3r_slam_amd/eval_recon.py: dist_stats with the
kernel's order of the two fp64 sums, the median ranks, the eighteen ICP moments in the kernel's order; an order-free math.fsum version of
the sums; and the whole evaluation by brute-force nearest neighbours for small clouds."""
import math

import numpy as np

from tests import cloud_oracle as CO
from tests import recon_oracle as RO

T = 256
MAX_BLOCKS = 1024
# The threshold of the icosphere tests.  4000 samples on a unit sphere lie 0.056 apart on average, so at the default 0.05 a tenth of them
# has no neighbour within the threshold in an independent sampling of the same surface (precision 0.87): the threshold has to be a few
# spacings for "two spheres 0.02 apart score 100 %" to be a statement about the surfaces and not about the sampling.
SPHERE_TAU = 0.2


def good_mask(dist2):
    s = np.asarray(dist2, np.float32)
    with np.errstate(invalid="ignore"):
        return (s >= 0) & (s != np.float32(np.inf))


def distances(dist2):
    """fp64 d of every entry (0 where the entry is bad) and the mask of the good ones; -0.0 gives +0.0"""
    ok = good_mask(dist2)
    s = np.where(ok, np.asarray(dist2, np.float32), np.float32(0)).astype(np.float64)
    return np.abs(np.sqrt(s)), ok


def bin_index(d, w, nbins):
    """the largest integer k with float64(k) * w <= d, and whether k < nbins"""
    d = np.asarray(d, np.float64)
    inside = d < float(nbins) * w
    k = np.floor(np.where(inside, d, 0.0) / w)
    k = np.minimum(k, max(nbins - 1, 0))
    k = np.where((k + 1 < nbins) & ((k + 1) * w <= d), k + 1, k)
    k = np.where((k > 0) & (k * w > d), k - 1, k)
    return k.astype(np.int64), inside


def stream_blocks(Q):
    return min((Q + 4 * T - 1) // (4 * T), MAX_BLOCKS)


def fixed_order_sum(c):
    """the kernel's sum of c [Q] fp64 (0 where an entry takes no part): thread t of workgroup b adds the entries 4 ((k G + b) 256 + t) + j
    in increasing (k, j), the 256 thread sums fold by the halving tree, the G workgroup sums are added in increasing b"""
    Q = len(c)
    G = stream_blocks(Q)
    K = -(-Q // (4 * T * G))
    pad = np.zeros(K * G * T * 4)
    pad[:Q] = c
    pad = pad.reshape(K, G, T, 4)
    acc = np.zeros((G, T))
    for k in range(K):
        for j in range(4):
            acc = acc + pad[k, :, :, j]
    o = T // 2
    while o > 0:
        acc[:, :o] = acc[:, :o] + acc[:, o:2 * o]
        o //= 2
    s = 0.0
    for b in range(G):
        s = s + acc[b, 0]
    return float(s)


def dist_stats(dist2, tau, w, nbins):
    """(counts int64 [3], moments fp64 [4], hist int64 [nbins]) as cut3r_dist_stats writes them"""
    d, ok = distances(dist2)
    s64 = np.where(ok, np.asarray(dist2, np.float32), np.float32(0)).astype(np.float64)
    counts = np.array([ok.sum(), (ok & (d < tau)).sum(), (~ok).sum()], np.int64)
    moments = np.array([fixed_order_sum(np.where(ok, d, 0.0)), fixed_order_sum(s64), d[ok].min() if ok.any() else np.inf,
                        d[ok].max() if ok.any() else -np.inf])
    k, inside = bin_index(d, w, nbins)
    hist = np.bincount(k[ok & inside], minlength=nbins).astype(np.int64)[:nbins] if nbins else np.zeros(0, np.int64)
    return counts, moments, hist


def fsum_sums(dist2):
    """(sum d, sum dist2) over the good entries, correctly rounded whatever the order (math.fsum)"""
    d, ok = distances(dist2)
    return math.fsum(d[ok]), math.fsum(np.asarray(dist2, np.float32)[ok].astype(np.float64))


def median_ranks(dist2):
    """fp32 [2]: the values of ascending ranks (n - 1) / 2 and n / 2 among the good entries (-0.0 as +0.0), NaN without any"""
    ok = good_mask(dist2)
    v = np.sort(np.abs(np.asarray(dist2, np.float32)[ok]))
    n = len(v)
    return np.float32([v[(n - 1) // 2], v[n // 2]]) if n else np.float32([np.nan, np.nan])


def moments18(src, ref, dist2, idx, T34=None):
    """cut3r_icp_moments_scaled's eighteen fp64 moments in the kernel's order: a grid of min(ceil(Q / 256), 1024) workgroups of 256
    threads, thread t of workgroup b adds the correspondences b 256 + t + k G 256 in increasing k, a 64-lane xor butterfly (32, 16, ...,
    1), the four waves in order, the workgroups in order"""
    s = RO.xform32(T34, src).astype(np.float64)
    Q = len(s)
    idx = np.asarray(idx)
    ok = idx >= 0
    d = np.asarray(ref, np.float32)[np.where(ok, idx, 0)].astype(np.float64)
    terms = np.zeros((Q, 18))
    terms[:, 0] = 1.0
    terms[:, 1] = np.asarray(dist2, np.float32).astype(np.float64)
    terms[:, 2:5] = s
    terms[:, 5:8] = d
    terms[:, 8:17] = (s[:, :, None] * d[:, None, :]).reshape(Q, 9)
    terms[:, 17] = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
    terms[~ok] = 0.0
    G = min((Q + 255) // 256, MAX_BLOCKS)
    K = -(-Q // (G * 256))
    pad = np.zeros((K * G * 256, 18))
    pad[:Q] = terms
    pad = pad.reshape(K, G, 4, 64, 18)
    acc = np.zeros((G, 4, 64, 18))
    for k in range(K):
        acc = acc + pad[k]
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, lane ^ o]
    blk = ((acc[:, 0, 0] + acc[:, 1, 0]) + acc[:, 2, 0]) + acc[:, 3, 0]
    out = np.zeros(18)
    for b in range(G):
        out = out + blk[b]
    return out


# ------------------------------------------------------------------------------------------------------------------ the pipeline
def sim3_fit(s, d):
    """eval_ate.umeyama (with_scale=True) on fp64 point pairs -> 4x4 (s R | t)"""
    mu_s, mu_d = s.mean(0), d.mean(0)
    xs, xd = s - mu_s, d - mu_d
    cov = xd.T @ xs / len(s)
    U, D, Vt = np.linalg.svd(cov)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    scale = np.trace(np.diag(D) @ S) / (xs ** 2).sum() * len(s)
    M = np.eye(4)
    M[:3, :3] = scale * R
    M[:3, 3] = mu_d - scale * R @ mu_s
    return M


def icp(src, dst, threshold, init=None, max_iteration=30, with_scaling=False):
    """recon_oracle.icp with the similarity update -> (T, fitness, rmse, iterations)"""
    if not with_scaling:
        return RO.icp(src, dst, threshold, init, max_iteration)
    dst64 = np.asarray(dst, np.float64)
    M = np.eye(4) if init is None else np.asarray(init, np.float64).copy()

    def evaluate(M):
        d2, idx = RO.nn(dst, src, threshold, M)
        ok = idx >= 0
        n = int(ok.sum())
        s = RO.xform32(M, src)[ok].astype(np.float64)
        return (s, dst64[idx[ok]]), n / len(src), (math.sqrt(d2[ok].astype(np.float64).sum() / n) if n else 0.0)

    pairs, fit, rmse = evaluate(M)
    it = 0
    for i in range(max_iteration):
        M = (sim3_fit(*pairs) if len(pairs[0]) else np.eye(4)) @ M
        pf, pr = fit, rmse
        pairs, fit, rmse = evaluate(M)
        it = i + 1
        if abs(pf - fit) < 1e-6 and abs(pr - rmse) < 1e-6:
            break
    return M, fit, rmse, it


def align_coarse_to_fine(rec, gt, tau, with_scaling=False):
    coarse = CO.voxel_downsample(rec, tau)[0], CO.voxel_downsample(gt, tau)[0]
    fine = CO.voxel_downsample(rec, 0.5 * tau)[0], CO.voxel_downsample(gt, 0.5 * tau)[0]
    M = np.eye(4)
    for (s, d), th in ((coarse, 80 * tau), (fine, 20 * tau), (fine, 2 * tau)):
        M = icp(s, d, th, M, max_iteration=20, with_scaling=with_scaling)[0]
    return M


def transform_points(p, M):
    """eval_recon.transform_points: ((M00 x + M01 y) + M02 z) + M03 in fp64, then fp32"""
    p = np.asarray(p, np.float32).astype(np.float64)
    M = np.asarray(M, np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((x * M[r, 0] + y * M[r, 1]) + z * M[r, 2]) + M[r, 3] for r in range(3)], 1).astype(np.float32)


def one_way(dist2, tau, w, nbins):
    counts, moments, hist = dist_stats(dist2, tau, w, nbins)
    good = int(counts[0])
    mean = moments[0] / good
    med = median_ranks(dist2).astype(np.float64)
    return {"share": int(counts[1]) / good, "mean": float(mean), "median": 0.5 * (math.sqrt(med[0]) + math.sqrt(med[1])),
            "std": math.sqrt(max(moments[1] / good - mean * mean, 0.0)), "min": float(moments[2]), "max": float(moments[3]),
            "counts": counts, "hist": hist, "cum": np.cumsum(hist).astype(np.float64) / good}


def precision_recall(rec, gt, tau=0.05, voxel=None, stretch=5, bins_per_tau=100):
    """eval_recon.precision_recall by brute force: {'rec': one_way, 'gt': one_way, 'precision', 'recall', 'fscore', 'edges'}"""
    voxel = 0.5 * tau if voxel is None else voxel
    rec, gt = np.asarray(rec, np.float32), np.asarray(gt, np.float32)
    if voxel > 0:
        rec, gt = CO.voxel_downsample(rec, voxel)[0], CO.voxel_downsample(gt, voxel)[0]
    nbins, w = stretch * bins_per_tau, tau / bins_per_tau
    a, b = one_way(RO.nn(gt, rec)[0], tau, w, nbins), one_way(RO.nn(rec, gt)[0], tau, w, nbins)
    p, r = a["share"], b["share"]
    return {"rec": a, "gt": b, "precision": p, "recall": r, "fscore": 2 * p * r / (p + r) if p + r > 0 else 0.0,
            "edges": np.arange(nbins + 1, dtype=np.float64) * w}
