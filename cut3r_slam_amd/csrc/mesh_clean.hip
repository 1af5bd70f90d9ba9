// Mesh clean-up after the extraction (cut3r_slam_amd/mesh_clean.py): vertex clustering (the counterpart of Open3D's
// simplify_vertex_clustering with averaged positions, in a fixed order) and removal of small connected components (Open3D's
// cluster_connected_triangles + remove_triangles_by_mask).  Compiled with -ffp-contract=off; tests/mesh_clean_oracle.py restates both.
//
// Every result is one definite set of bits: the clusters are the voxels of the voxel downsample (voxel_cluster.h, shared with cloud.hip),
// duplicates are found by a stable radix sort of the rotated triples with the face index, every output list is a count -> scan -> emit
// compaction in input order, and the only atomics are integer min, add and stores of the constant 1, which give the same result in any
// arrival order.  No kernel waits for another workgroup: the labelling loop runs on the host, one hook and one jump launch per round.
#include "voxel_cluster.h"

namespace {

constexpr unsigned long long TRIPLE_NONE = ~0ull;            // the sort key of a degenerate face: after every real triple

void record(void* const* events, int k, hipStream_t s) {
    if (events && events[k]) (void)hipEventRecord((hipEvent_t)events[k], s);
}

int blocks_of(long long n) { return (int)((n + 255) / 256); }

// ---------------------------------------------------------------------------------------------------- compaction of a flag array
// bcount[blk] = set flags of the block; the entry after the last block is 0
__global__ __launch_bounds__(256) void flag_count_kernel(const unsigned char* __restrict__ flag, long long n, unsigned* __restrict__ bcount) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned total;
    (void)block_rank(i < n && flag[i] != 0, &total);
    if (threadIdx.x == 0) {
        bcount[blockIdx.x] = total;
        if (blockIdx.x == 0) bcount[gridDim.x] = 0;
    }
}

// map[i] = position of item i among the flagged ones, or -1; list[position] = i (list may be NULL); positions >= cap are not written
__global__ __launch_bounds__(256) void flag_index_kernel(const unsigned char* __restrict__ flag, long long n, const unsigned* __restrict__ offs,
                                                         long long cap, int* __restrict__ map, int* __restrict__ list) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool on = i < n && flag[i] != 0;
    unsigned total;
    const unsigned r = block_rank(on, &total);
    if (i >= n) return;
    const long long pos = (long long)offs[blockIdx.x] + r;
    map[i] = on && pos < cap ? (int)pos : -1;
    if (on && list && pos < cap) list[pos] = (int)i;
}

int compact_count(const unsigned char* flag, long long n, unsigned* bcount, unsigned* offs, void* temp, size_t temp_bytes, hipStream_t s) {
    const int nblk = blocks_of(n);
    hipLaunchKernelGGL(flag_count_kernel, dim3(nblk), dim3(256), 0, s, flag, n, bcount);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    if (hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, bcount, offs, nblk + 1, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    return CUT3R_OK;
}

size_t scan_bytes_for(long long n) {
    size_t b = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, b, (unsigned*)nullptr, (unsigned*)nullptr, blocks_of(n) + 1, (hipStream_t)0);
    return b;
}

// out_faces[p] = the kept face's three ids through newid; tri [F,3], fmap [F] (position or -1)
__global__ __launch_bounds__(256) void face_emit_kernel(const int* __restrict__ tri, long long F, const int* __restrict__ fmap,
                                                        const int* __restrict__ newid, long long nid, long long cap, int* __restrict__ out) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const long long p = fmap[f];
    if (p < 0 || p >= cap) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int t = tri[3 * f + k];
        out[3 * p + k] = (t >= 0 && t < nid) ? newid[t] : -1;
    }
}

// --------------------------------------------------------------------------------------------------------------- face index check
__global__ __launch_bounds__(256) void faces_check_kernel(const int* __restrict__ faces, long long n, int V, int* __restrict__ bad) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && (unsigned)faces[i] >= (unsigned)V) *bad = 1;
}

// ---------------------------------------------------------------------------------------------------------------- vertex clustering
// sorted position i -> cid[point] = the run (cluster) it lies in
__global__ __launch_bounds__(256) void cluster_id_kernel(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals, int N,
                                                         const unsigned* __restrict__ offs, int* __restrict__ cid) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool head = voxel_head(keys, i, N);
    unsigned t;
    const unsigned before = block_rank(head, &t);
    if (i >= N) return;
    const unsigned v = vals[i];
    if (v < (unsigned)N) cid[v] = (int)(offs[blockIdx.x] + before + (head ? 1u : 0u)) - 1;
}

// face -> its cluster triple, rotated so that the smallest id leads (orientation kept), or (-1, -1, -1) when two ids are equal; the sort
// keys of the triple (one 64-bit key of 3 x bits, or the low id c and the high pair a, b) and the face index as the sort value
__global__ __launch_bounds__(256) void face_remap_kernel(const int* __restrict__ faces, long long F, int V, const int* __restrict__ cid, int bits,
                                                         int passes, int* __restrict__ tri, unsigned long long* __restrict__ key64,
                                                         unsigned* __restrict__ key32, unsigned* __restrict__ val,
                                                         unsigned long long* __restrict__ ndeg) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    bool deg = false;
    if (f < F) {
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        int a = -1, b = -1, c = -1;
        if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {
            a = cid[i0];
            b = cid[i1];
            c = cid[i2];
        }
        deg = a < 0 || a == b || b == c || a == c;
        if (deg) {
            a = b = c = -1;
        } else if (b < a && b < c) {
            const int t = a;
            a = b, b = c, c = t;
        } else if (c < a && c < b) {
            const int t = c;
            c = b, b = a, a = t;
        }
        tri[3 * f] = a, tri[3 * f + 1] = b, tri[3 * f + 2] = c;
        val[f] = (unsigned)f;
        if (passes == 1) {
            key64[f] = deg ? TRIPLE_NONE
                           : ((unsigned long long)a << (2 * bits)) | ((unsigned long long)b << bits) | (unsigned long long)c;
        } else {
            key32[f] = deg ? ~0u : (unsigned)c;
        }
    }
    unsigned total;
    (void)block_rank(deg, &total);
    if (threadIdx.x == 0 && total) atomicAdd(ndeg, (unsigned long long)total);
}

// second pass of the two-pass sort: the key (a, b) of the face at every position of the order by c
__global__ __launch_bounds__(256) void face_high_key_kernel(const int* __restrict__ tri, const unsigned* __restrict__ order, long long F, int bits,
                                                            unsigned long long* __restrict__ key64) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= F) return;
    const unsigned f = order[k];
    const int a = f < F ? tri[3 * (size_t)f] : -1;
    key64[k] = a < 0 ? TRIPLE_NONE : ((unsigned long long)a << bits) | (unsigned long long)tri[3 * (size_t)f + 1];
}

// in the sorted order equal triples are neighbours with ascending face index: the first of a run is kept, and marks its clusters
__global__ __launch_bounds__(256) void face_first_kernel(const int* __restrict__ tri, const unsigned* __restrict__ order, long long F, long long M,
                                                         unsigned char* __restrict__ fkeep, unsigned char* __restrict__ cref) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= F) return;
    const unsigned f = order[k];
    if (f >= F) return;
    const int a = tri[3 * (size_t)f], b = tri[3 * (size_t)f + 1], c = tri[3 * (size_t)f + 2];
    bool keep = a >= 0 && a < M && b < M && c < M;
    if (keep && k > 0) {
        const unsigned g = order[k - 1];
        if (g < F) keep = tri[3 * (size_t)g] != a || tri[3 * (size_t)g + 1] != b || tri[3 * (size_t)g + 2] != c;
    }
    fkeep[f] = keep ? 1 : 0;
    if (keep) cref[a] = 1, cref[b] = 1, cref[c] = 1;
}

// totals = F', V', degenerate, duplicate
__global__ void cluster_totals_kernel(const unsigned* __restrict__ fo, int fblk, const unsigned* __restrict__ co, int cblk, long long F,
                                      const unsigned long long* __restrict__ ndeg, long long* __restrict__ totals) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long kept = (long long)fo[fblk], deg = (long long)*ndeg;
    totals[0] = kept;
    totals[1] = (long long)co[cblk];
    totals[2] = deg;
    totals[3] = F - deg - kept;
}

__global__ __launch_bounds__(256) void vertex_map_kernel(const int* __restrict__ cid, int V, const int* __restrict__ newid, long long M,
                                                         int* __restrict__ vmap) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int c = cid[v];
    vmap[v] = (c >= 0 && c < M) ? newid[c] : -1;
}

// VoxelLayout of V | cid [V] | tri [F,3] | fkeep [F] | fmap [F] | cref [V] | newid [V] | block counts and offsets of faces and of clusters |
// ndeg | key_a, key_b [F] u64 (key_b holds the two u32 key arrays of the first of two passes) | val_a, val_b [F] | sort / scan scratch
struct ClusterLayout {
    VoxelLayout vox;
    int fblk, vblk;
    size_t cid, tri, fkeep, fmap, cref, newid, fb, fo, cb, co, ndeg, key_a, key_b, val_a, val_b, temp, sort64, sort32, scan, total;
};

ClusterLayout cluster_layout(int V, int F) {
    ClusterLayout L;
    L.vox = voxel_layout(V);
    L.fblk = blocks_of(F);
    L.vblk = blocks_of(V);
    size_t o = L.vox.total;
    auto take = [&](size_t bytes) { const size_t r = o; o = align256(o + bytes); return r; };
    L.cid = take(4 * (size_t)V);
    L.tri = take(12 * (size_t)F);
    L.fkeep = take((size_t)F);
    L.fmap = take(4 * (size_t)F);
    L.cref = take((size_t)V);
    L.newid = take(4 * (size_t)V);
    L.fb = take(4 * ((size_t)L.fblk + 1));
    L.fo = take(4 * ((size_t)L.fblk + 1));
    L.cb = take(4 * ((size_t)L.vblk + 1));
    L.co = take(4 * ((size_t)L.vblk + 1));
    L.ndeg = take(8);
    L.key_a = take(8 * (size_t)F);
    L.key_b = take(8 * (size_t)F);
    L.val_a = take(4 * (size_t)F);
    L.val_b = take(4 * (size_t)F);
    L.sort64 = L.sort32 = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, L.sort64, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned*)nullptr,
                                             (unsigned*)nullptr, F, 0, 64, (hipStream_t)0);
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, L.sort32, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, F,
                                             0, 32, (hipStream_t)0);
    const size_t sf = scan_bytes_for(F), sv = scan_bytes_for(V);
    L.scan = sf > sv ? sf : sv;
    size_t t = L.sort64 > L.sort32 ? L.sort64 : L.sort32;
    if (L.scan > t) t = L.scan;
    L.temp = take(t);
    L.total = o;
    return L;
}

bool mesh_sizes_ok(int V, int F) { return V >= 1 && F >= 1; }     // every index into faces [F,3] is 64-bit

// ------------------------------------------------------------------------------------------------------------ connected components
__global__ __launch_bounds__(256) void label_init_kernel(int* __restrict__ a, int* __restrict__ b, int V) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v < V) a[v] = b[v] = (int)v;
}

// atomicMin(&lab[i], m), skipped when the entry is seen at or below m already: entries only fall during the launch, so a value read
// (however old) is an upper bound of the entry, and a skipped min would have changed nothing.  Spares the one address that the faces of a
// large component all lower.
DEVINL void lower(int* lab, int i, int m) {
    if (*(volatile int*)&lab[i] > m) atomicMin(&lab[i], m);
}

// reads the labels of the round's start (cur: nobody writes them here) and lowers, in nxt, the three vertices and the three labels they
// carry to the face's smallest label: integer atomicMin, so nxt after the launch does not depend on the order of arrival
__global__ __launch_bounds__(256) void label_hook_kernel(const int* __restrict__ faces, long long F, int V, const int* __restrict__ cur,
                                                         int* nxt, int* __restrict__ changed) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return;
    const int l0 = cur[i0], l1 = cur[i1], l2 = cur[i2];
    const int m = min(l0, min(l1, l2));
    if ((unsigned)l0 >= (unsigned)V || (unsigned)l1 >= (unsigned)V || (unsigned)l2 >= (unsigned)V) return;     // labels are vertex indices
    if (l0 == m && l1 == m && l2 == m) return;
    *changed = 1;
    if (l0 > m) lower(nxt, i0, m), lower(nxt, l0, m);
    if (l1 > m) lower(nxt, i1, m), lower(nxt, l1, m);
    if (l2 > m) lower(nxt, i2, m), lower(nxt, l2, m);
}

// pointer jumping to the end of the chain.  lab[x] <= x everywhere, so a chain descends and ends at a fixed point; a concurrent write
// replaces an entry by the end of its own chain, which is the end of every chain through it: the result does not depend on the timing
__global__ __launch_bounds__(256) void label_jump_kernel(int* lab, int* copy, int V) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    int l = lab[v];
    for (int guard = 0; guard < V; guard++) {
        if ((unsigned)l >= (unsigned)V) break;
        const int n = lab[l];
        if (n >= l) break;
        l = n;
    }
    lab[v] = l;
    copy[v] = l;
}

__global__ __launch_bounds__(256) void comp_size_kernel(const int* __restrict__ faces, long long F, int V, const int* __restrict__ labels,
                                                        int* __restrict__ sizes) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    int l = -1;
    if (f < F) {
        const int i0 = faces[3 * f];
        if ((unsigned)i0 < (unsigned)V) l = labels[i0];
        if ((unsigned)l >= (unsigned)V) l = -1;
    }
    // neighbouring faces mostly share a component: one add per distinct label of the wave, not one per face (a surface of millions of
    // faces would otherwise queue them all on one address); integer adds, so the sums are the same
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(l >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int ll = __shfl(l, leader, 64);
        const unsigned long long same = __ballot(l == ll) & todo;
        if (lane == leader) atomicAdd(&sizes[ll], (int)__popcll(same));
        todo &= ~same;
    }
}

// key = (2^32 - 1 - size) << 32 | label: ascending keys are (size descending, label ascending); vertices that label no face sort last
__global__ __launch_bounds__(256) void comp_key_kernel(const int* __restrict__ sizes, int V, unsigned long long* __restrict__ keys,
                                                       unsigned long long* __restrict__ ncomp) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    const int s = v < V ? sizes[v] : 0;
    if (v < V) keys[v] = s > 0 ? ((unsigned long long)(0xffffffffu - (unsigned)s) << 32) | (unsigned long long)v : TRIPLE_NONE;
    unsigned total;
    (void)block_rank(s > 0, &total);
    if (threadIdx.x == 0 && total) atomicAdd(ncomp, (unsigned long long)total);
}

// the kept components are a prefix of the sorted keys: size >= min_faces (min_faces > 0) or rank < keep_largest
__global__ __launch_bounds__(256) void comp_mark_kernel(const unsigned long long* __restrict__ keys, int V, int min_faces, int keep_largest,
                                                        unsigned char* __restrict__ mark, unsigned long long* __restrict__ nkept) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (i < V && keys[i] != TRIPLE_NONE) {
        const unsigned size = 0xffffffffu - (unsigned)(keys[i] >> 32);
        const unsigned label = (unsigned)(keys[i] & 0xffffffffu);
        keep = (min_faces > 0 ? size >= (unsigned)min_faces : i < keep_largest) && label < (unsigned)V;
        if (keep) mark[label] = 1;
    }
    unsigned total;
    (void)block_rank(keep, &total);
    if (threadIdx.x == 0 && total) atomicAdd(nkept, (unsigned long long)total);
}

__global__ __launch_bounds__(256) void comp_face_kernel(const int* __restrict__ faces, long long F, int V, const int* __restrict__ labels,
                                                        const unsigned char* __restrict__ mark, unsigned char* __restrict__ fkeep,
                                                        unsigned char* __restrict__ vref) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    bool keep = (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;
    if (keep) {
        const int l = labels[i0];
        keep = (unsigned)l < (unsigned)V && mark[l] != 0;
    }
    fkeep[f] = keep ? 1 : 0;
    if (keep) vref[i0] = 1, vref[i1] = 1, vref[i2] = 1;
}

// totals = components, kept components, F', V'
__global__ void comp_totals_kernel(const unsigned long long* __restrict__ cnt, const unsigned* __restrict__ fo, int fblk,
                                   const unsigned* __restrict__ vo, int vblk, long long* __restrict__ totals) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    totals[0] = (long long)cnt[0];
    totals[1] = (long long)cnt[1];
    totals[2] = (long long)fo[fblk];
    totals[3] = (long long)vo[vblk];
}

__global__ __launch_bounds__(256) void vertex_gather_kernel(const float* __restrict__ verts, const unsigned char* __restrict__ cols, int V,
                                                            const int* __restrict__ vmap, long long cap, float* __restrict__ out,
                                                            unsigned char* __restrict__ out_col) {
    const long long v = (long long)blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const long long p = vmap[v];
    if (p < 0 || p >= cap) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        out[3 * p + k] = verts[3 * v + k];
        if (cols) out_col[3 * p + k] = cols[3 * v + k];
    }
}

__global__ __launch_bounds__(256) void comp_list_kernel(const unsigned long long* __restrict__ keys, long long K, int* __restrict__ comps) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= K) return;
    comps[2 * i] = (int)(keys[i] & 0xffffffffu);
    comps[2 * i + 1] = (int)(0xffffffffu - (unsigned)(keys[i] >> 32));
}

// sizes [V] | key_a, key_b [V] u64 | mark [V] | vref [V] | fkeep [F] | fmap [F] | block counts and offsets of faces and vertices | cnt [2] |
// sort / scan scratch
struct CompLayout {
    int fblk, vblk;
    size_t sizes, key_a, key_b, mark, vref, fkeep, fmap, fb, fo, vb, vo, cnt, temp, sort, scan, total;
};

CompLayout comp_layout(int V, int F) {
    CompLayout L;
    L.fblk = blocks_of(F);
    L.vblk = blocks_of(V);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t r = o; o = align256(o + bytes); return r; };
    L.sizes = take(4 * (size_t)V);
    L.key_a = take(8 * (size_t)V);
    L.key_b = take(8 * (size_t)V);
    L.mark = take((size_t)V);
    L.vref = take((size_t)V);
    L.fkeep = take((size_t)F);
    L.fmap = take(4 * (size_t)F);
    L.fb = take(4 * ((size_t)L.fblk + 1));
    L.fo = take(4 * ((size_t)L.fblk + 1));
    L.vb = take(4 * ((size_t)L.vblk + 1));
    L.vo = take(4 * ((size_t)L.vblk + 1));
    L.cnt = take(16);
    L.sort = 0;
    (void)hipcub::DeviceRadixSort::SortKeys(nullptr, L.sort, (unsigned long long*)nullptr, (unsigned long long*)nullptr, V, 0, 64, (hipStream_t)0);
    const size_t sf = scan_bytes_for(F), sv = scan_bytes_for(V);
    L.scan = sf > sv ? sf : sv;
    L.temp = take(L.sort > L.scan ? L.sort : L.scan);
    L.total = o;
    return L;
}

}  // namespace

extern "C" int cut3r_mesh_faces_check(const int* faces, int F, int V, int* bad, void* stream) {
    if (!faces || !bad || !mesh_sizes_ok(V, F)) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(bad, 0, sizeof(int), s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(faces_check_kernel, dim3(blocks_of(3ll * F)), dim3(256), 0, s, faces, 3ll * F, V, bad);
    return cut3r_check_launch();
}

extern "C" long long cut3r_mesh_cluster_workspace_bytes(int V, int F) {
    if (!mesh_sizes_ok(V, F)) return -1;
    return (long long)cluster_layout(V, F).total;
}

extern "C" int cut3r_mesh_cluster_count(const float* verts, int V, int F, double cell, const float* lo, const float* hi, void* workspace,
                                        long long workspace_bytes, long long* total, void* stream) {
    if (!verts || !lo || !hi || !workspace || !total || !mesh_sizes_ok(V, F)) return CUT3R_ERR_ARG;
    VoxelFrame fr;
    if (!voxel_frame(cell, lo, hi, &fr)) return CUT3R_ERR_ARG;
    const ClusterLayout L = cluster_layout(V, F);
    if (workspace_bytes < (long long)L.total) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)workspace;
    const int rc = voxel_sort_runs(verts, V, fr, L.vox, w, total, s);
    if (rc != CUT3R_OK) return rc;
    hipLaunchKernelGGL(cluster_id_kernel, dim3(L.vblk), dim3(256), 0, s, (const unsigned long long*)(w + L.vox.keys_out),
                       (const unsigned*)(w + L.vox.vals_out), V, (const unsigned*)(w + L.vox.offs), (int*)(w + L.cid));
    return cut3r_check_launch();
}

extern "C" int cut3r_mesh_cluster_faces(const int* faces, int V, int F, long long M, int passes, void* workspace, long long workspace_bytes,
                                        long long* totals, void* const* events, void* stream) {
    if (!faces || !workspace || !totals || !mesh_sizes_ok(V, F) || M < 1 || M > V) return CUT3R_ERR_ARG;
    int bits = 1;
    while ((1ll << bits) < M) bits++;
    if (passes == 0) passes = 3 * bits <= 64 ? 1 : 2;
    if (passes != 1 && passes != 2) return CUT3R_ERR_ARG;
    if (passes == 1 && 3 * bits > 64) return CUT3R_ERR_ARG;
    const ClusterLayout L = cluster_layout(V, F);
    if (workspace_bytes < (long long)L.total) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)workspace;
    int* tri = (int*)(w + L.tri);
    unsigned long long* key_a = (unsigned long long*)(w + L.key_a);
    unsigned long long* key_b = (unsigned long long*)(w + L.key_b);
    unsigned* k32_a = (unsigned*)(w + L.key_b);
    unsigned* k32_b = k32_a + F;
    unsigned* val_a = (unsigned*)(w + L.val_a);
    unsigned* val_b = (unsigned*)(w + L.val_b);
    unsigned long long* ndeg = (unsigned long long*)(w + L.ndeg);
    unsigned char* fkeep = (unsigned char*)(w + L.fkeep);
    unsigned char* cref = (unsigned char*)(w + L.cref);
    if (hipMemsetAsync(ndeg, 0, 8, s) != hipSuccess || hipMemsetAsync(cref, 0, (size_t)V, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(face_remap_kernel, dim3(L.fblk), dim3(256), 0, s, faces, (long long)F, V, (const int*)(w + L.cid), bits, passes, tri, key_a,
                       k32_a, val_a, ndeg);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    record(events, 0, s);
    const unsigned* order;
    if (passes == 1) {
        size_t tb = L.sort64;
        if (hipcub::DeviceRadixSort::SortPairs(w + L.temp, tb, key_a, key_b, val_a, val_b, F, 0, 3 * bits, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
        order = val_b;
    } else {
        size_t tb = L.sort32;
        if (hipcub::DeviceRadixSort::SortPairs(w + L.temp, tb, k32_a, k32_b, val_a, val_b, F, 0, 32, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
        hipLaunchKernelGGL(face_high_key_kernel, dim3(L.fblk), dim3(256), 0, s, tri, val_b, (long long)F, bits, key_a);
        if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
        tb = L.sort64;
        if (hipcub::DeviceRadixSort::SortPairs(w + L.temp, tb, key_a, key_b, val_b, val_a, F, 0, 64, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
        order = val_a;
    }
    hipLaunchKernelGGL(face_first_kernel, dim3(L.fblk), dim3(256), 0, s, tri, order, (long long)F, M, fkeep, cref);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    record(events, 1, s);
    unsigned* fo = (unsigned*)(w + L.fo);
    unsigned* co = (unsigned*)(w + L.co);
    if (compact_count(fkeep, F, (unsigned*)(w + L.fb), fo, w + L.temp, L.scan, s) != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    if (compact_count(cref, M, (unsigned*)(w + L.cb), co, w + L.temp, L.scan, s) != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(cluster_totals_kernel, dim3(1), dim3(64), 0, s, fo, L.fblk, co, blocks_of(M), (long long)F, ndeg, totals);
    return cut3r_check_launch();
}

extern "C" int cut3r_mesh_cluster_emit(const float* verts, const unsigned char* colors, int V, int F, long long M, void* workspace,
                                       long long workspace_bytes, float* out_verts, unsigned char* out_colors, int* out_faces, int* vertex_map,
                                       int* face_map, long long Vout, long long Fout, long long cap_v, long long cap_f, void* const* events,
                                       void* stream) {
    if (!verts || !workspace || !vertex_map || !mesh_sizes_ok(V, F) || M < 1 || M > V) return CUT3R_ERR_ARG;
    if (Vout < 0 || Vout > M || Fout < 0 || Fout > F || cap_v < Vout || cap_f < Fout) return CUT3R_ERR_ARG;
    if ((Fout > 0) != (Vout > 0)) return CUT3R_ERR_ARG;
    if (Vout > 0 && (!out_verts || !out_faces || !face_map || (colors != nullptr) != (out_colors != nullptr))) return CUT3R_ERR_ARG;
    const ClusterLayout L = cluster_layout(V, F);
    if (workspace_bytes < (long long)L.total) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)workspace;
    int* newid = (int*)(w + L.newid);
    int* fmap = (int*)(w + L.fmap);
    hipLaunchKernelGGL(flag_index_kernel, dim3(blocks_of(M)), dim3(256), 0, s, (const unsigned char*)(w + L.cref), M, (const unsigned*)(w + L.co),
                       Vout, newid, (int*)nullptr);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    if (Vout > 0) {
        const int rc = voxel_means(verts, colors, V, L.vox, w, out_verts, out_colors, nullptr, M, newid, Vout, s);
        if (rc != CUT3R_OK) return rc;
    }
    record(events, 0, s);
    hipLaunchKernelGGL(vertex_map_kernel, dim3(L.vblk), dim3(256), 0, s, (const int*)(w + L.cid), V, newid, M, vertex_map);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    if (Fout == 0) return CUT3R_OK;
    hipLaunchKernelGGL(flag_index_kernel, dim3(L.fblk), dim3(256), 0, s, (const unsigned char*)(w + L.fkeep), (long long)F,
                       (const unsigned*)(w + L.fo), Fout, fmap, face_map);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(face_emit_kernel, dim3(L.fblk), dim3(256), 0, s, (const int*)(w + L.tri), (long long)F, fmap, newid, M, Fout, out_faces);
    return cut3r_check_launch();
}

extern "C" int cut3r_mesh_label_init(int* labels, int* scratch, int V, void* stream) {
    if (!labels || !scratch || V < 1) return CUT3R_ERR_ARG;
    hipLaunchKernelGGL(label_init_kernel, dim3(blocks_of(V)), dim3(256), 0, (hipStream_t)stream, labels, scratch, V);
    return cut3r_check_launch();
}

extern "C" int cut3r_mesh_label_round(const int* faces, int V, int F, int* labels, int* scratch, int* changed, void* stream) {
    if (!faces || !labels || !scratch || !changed || !mesh_sizes_ok(V, F)) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(changed, 0, sizeof(int), s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(label_hook_kernel, dim3(blocks_of(F)), dim3(256), 0, s, faces, (long long)F, V, labels, scratch, changed);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(label_jump_kernel, dim3(blocks_of(V)), dim3(256), 0, s, scratch, labels, V);
    return cut3r_check_launch();
}

extern "C" long long cut3r_mesh_components_workspace_bytes(int V, int F) {
    if (!mesh_sizes_ok(V, F)) return -1;
    return (long long)comp_layout(V, F).total;
}

extern "C" int cut3r_mesh_components_count(const int* faces, int V, int F, const int* labels, int min_faces, int keep_largest, void* workspace,
                                           long long workspace_bytes, long long* totals, void* stream) {
    if (!faces || !labels || !workspace || !totals || !mesh_sizes_ok(V, F)) return CUT3R_ERR_ARG;
    if ((min_faces > 0) == (keep_largest > 0) || min_faces < 0 || keep_largest < 0) return CUT3R_ERR_ARG;
    const CompLayout L = comp_layout(V, F);
    if (workspace_bytes < (long long)L.total) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)workspace;
    int* sizes = (int*)(w + L.sizes);
    unsigned long long* key_a = (unsigned long long*)(w + L.key_a);
    unsigned long long* key_b = (unsigned long long*)(w + L.key_b);
    unsigned long long* cnt = (unsigned long long*)(w + L.cnt);
    unsigned char* mark = (unsigned char*)(w + L.mark);
    unsigned char* vref = (unsigned char*)(w + L.vref);
    unsigned char* fkeep = (unsigned char*)(w + L.fkeep);
    if (hipMemsetAsync(sizes, 0, 4 * (size_t)V, s) != hipSuccess || hipMemsetAsync(cnt, 0, 16, s) != hipSuccess ||
        hipMemsetAsync(mark, 0, (size_t)V, s) != hipSuccess || hipMemsetAsync(vref, 0, (size_t)V, s) != hipSuccess)
        return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(comp_size_kernel, dim3(L.fblk), dim3(256), 0, s, faces, (long long)F, V, labels, sizes);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(comp_key_kernel, dim3(L.vblk), dim3(256), 0, s, sizes, V, key_a, cnt);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    size_t tb = L.sort;
    if (hipcub::DeviceRadixSort::SortKeys(w + L.temp, tb, key_a, key_b, V, 0, 64, s) != hipSuccess) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(comp_mark_kernel, dim3(L.vblk), dim3(256), 0, s, key_b, V, min_faces, keep_largest, mark, cnt + 1);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(comp_face_kernel, dim3(L.fblk), dim3(256), 0, s, faces, (long long)F, V, labels, mark, fkeep, vref);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    unsigned* fo = (unsigned*)(w + L.fo);
    unsigned* vo = (unsigned*)(w + L.vo);
    if (compact_count(fkeep, F, (unsigned*)(w + L.fb), fo, w + L.temp, L.scan, s) != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    if (compact_count(vref, V, (unsigned*)(w + L.vb), vo, w + L.temp, L.scan, s) != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(comp_totals_kernel, dim3(1), dim3(64), 0, s, cnt, fo, L.fblk, vo, L.vblk, totals);
    return cut3r_check_launch();
}

extern "C" int cut3r_mesh_components_emit(const float* verts, const unsigned char* colors, int V, const int* faces, int F, void* workspace,
                                          long long workspace_bytes, float* out_verts, unsigned char* out_colors, int* out_faces,
                                          int* vertex_map, int* face_map, int* comps, long long Vout, long long Fout, long long K, long long cap_v,
                                          long long cap_f, long long cap_k, void* stream) {
    if (!verts || !faces || !workspace || !vertex_map || !mesh_sizes_ok(V, F)) return CUT3R_ERR_ARG;
    if (Vout < 0 || Vout > V || Fout < 0 || Fout > F || K < 0 || K > V || cap_v < Vout || cap_f < Fout || cap_k < K) return CUT3R_ERR_ARG;
    if ((Fout > 0) != (Vout > 0) || (K > 0 && !comps)) return CUT3R_ERR_ARG;
    if (Vout > 0 && (!out_verts || !out_faces || !face_map || (colors != nullptr) != (out_colors != nullptr))) return CUT3R_ERR_ARG;
    const CompLayout L = comp_layout(V, F);
    if (workspace_bytes < (long long)L.total) return CUT3R_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)workspace;
    int* fmap = (int*)(w + L.fmap);
    hipLaunchKernelGGL(flag_index_kernel, dim3(L.vblk), dim3(256), 0, s, (const unsigned char*)(w + L.vref), (long long)V,
                       (const unsigned*)(w + L.vo), Vout, vertex_map, (int*)nullptr);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    if (K > 0) {
        hipLaunchKernelGGL(comp_list_kernel, dim3(blocks_of(K)), dim3(256), 0, s, (const unsigned long long*)(w + L.key_b), K, comps);
        if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    }
    if (Fout == 0) return CUT3R_OK;
    hipLaunchKernelGGL(vertex_gather_kernel, dim3(L.vblk), dim3(256), 0, s, verts, colors, V, vertex_map, Vout, out_verts, out_colors);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(flag_index_kernel, dim3(L.fblk), dim3(256), 0, s, (const unsigned char*)(w + L.fkeep), (long long)F,
                       (const unsigned*)(w + L.fo), Fout, fmap, face_map);
    if (cut3r_check_launch() != CUT3R_OK) return CUT3R_ERR_LAUNCH;
    hipLaunchKernelGGL(face_emit_kernel, dim3(L.fblk), dim3(256), 0, s, faces, (long long)F, fmap, vertex_map, (long long)V, Fout, out_faces);
    return cut3r_check_launch();
}
