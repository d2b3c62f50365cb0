// bre_roots.hip — the tile kernel's work roots and its 4-wide view of the tree: the work-root selection
// (k_roots), a work-root shard's list (k_roots_shard) and the 4-wide collapse (k_collapse4).
#include <hip/hip_runtime.h>

#include "bre_device.h"

namespace bre {

namespace {

// Work roots: the BVH frontier at depth log2(S) (leaves above it stay in the frontier), ordered by the
// number of leaf tiles below each root, largest first (stable): with block map 3 every packet's
// waves on the largest subtrees are dispatched first and the kernel's tail is made of small ones.
// The leaves below a Karras node are a contiguous range (bre_build.hip), found by its leftmost and
// rightmost descents.  The partial sums are added in this root order (k_reduce): deterministic.
//
// Starting from the root, the frontier's LARGEST internal node (leaf tiles below it, Node::nleaf; ties:
// the lowest frontier position) is replaced by its children (the first in its place, the second
// appended) while the frontier stays within S entries, so the S work roots are as equal in size as
// the tree allows: the longest (packet, subtree) waves, which end the launch, are as short as they can
// be (a breadth-first frontier left subtrees of very unequal size, and an emulated 1/8 rank's
// iteration-0 gather 37% above 1/8 of N = 1's).  Then the roots are ordered largest first (ties in
// frontier order) for the LPT block map.
//
// The greedy loop is serial (up to S - 1 expansions: 0.39 ms at C2 as a block-wide reduction per
// expansion), but its result is not: every expanded node has more leaf tiles than its children, so
// the expansions come in decreasing order of size and the expanded set E is the S - 1 largest
// interior nodes (fewer when the tree has fewer), a subtree from the root; the roots are E's children
// outside E.  So, with all threads:
//   1. cache, breadth first, every interior node with at least total / S leaf tiles (the frontier
//      partitions the total over <= S entries, so its largest entry, the only one ever expanded, has
//      at least total / S): its leaf tiles, children, their leaf tiles and cache slots;
//   2. E = the S - 1 cached nodes of largest (leaf tiles, -index), each ranked against all others;
//   3. the roots: E's children outside E (the whole tree's root when S = 1);
//   4. ranks: leaf tiles descending, ties by child index.
// Ties of equal size are broken by node index instead of the frontier position the serial form used
// (any frontier is a valid split; this one is deterministic).  A cache overflow (never seen: C2 caches
// ~600 of 4096 slots at S = 256) still yields a valid split: the cached nodes form a subtree from the
// root, so E's top-(S - 1) choice among them is one too.
constexpr int kRootSlots = 4096;
// the cache, in global scratch (one wave computes the roots: a one-wave workgroup with no LDS fits a
// concurrent gather's slots, bre_slot.hip; round 5's version kept it in 140 KB of LDS, a whole CU)
struct RootsScratch {
    int32_t id[kRootSlots];     // cached node
    int32_t nl[kRootSlots];     // its leaf tiles (Node::nleaf)
    int32_t ch[kRootSlots][2];  // its children
    int32_t cw[kRootSlots][2];  // their leaf tiles (1: a leaf tile, 0: empty)
    int32_t cs[kRootSlots][2];  // their cache slots (-1: not cached)
    int32_t in_e[kRootSlots];
    int32_t fc[kMaxSplit + 1], fw[kMaxSplit + 1];  // the roots, unordered
};

// children, parent and leaf tiles of node x: the record's last 16 bytes
__device__ __forceinline__ int4 node_tail(const Node *__restrict__ nodes, int32_t x) {
    return *reinterpret_cast<const int4 *>(&nodes[x].child[0]);
}

// the wave's own global writes visible to its later reads (device-scope release + acquire)
__device__ __forceinline__ void wave_sync_global() {
    __threadfence();
    __builtin_amdgcn_wave_barrier();
}

// key of a node or root of w leaf tiles and index x: larger first, ties by ascending (signed) index
__device__ __forceinline__ unsigned long long root_key(int32_t w, int32_t x) {
    return ((unsigned long long)(unsigned int)w << 32) | (0xffffffffu - ((unsigned int)x ^ 0x80000000u));
}

// rank of key kk among the n keys key(w[j], x[j]) (the number of larger ones): 64 keys per step, read by
// one lane each and broadcast by readlane
__device__ __forceinline__ int rank_among(const int32_t *w, const int32_t *x, int n, unsigned long long kk) {
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + (int)threadIdx.x;
        const unsigned long long kv = j < n ? root_key(w[j], x[j]) : 0ull;
        const int m = min(64, n - j0);
        for (int q = 0; q < m; ++q) {
            const unsigned long long kj =
                ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane((int)(kv >> 32), q) << 32) |
                (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)kv, q);
            rank += kj > kk;
        }
    }
    return rank;
}

__global__ __launch_bounds__(64) void k_roots(const Node *__restrict__ nodes, int S, int32_t *__restrict__ roots,
                                              RootsScratch *__restrict__ g) {
    const int t = threadIdx.x;
    const unsigned long long below = (1ull << t) - 1ull;
    const int32_t total = nodes[0].nleaf;
    const int32_t heavy = total / S;
    if (t == 0) g->id[0] = 0;
    wave_sync_global();
    // 1. breadth-first cache of the heavy interior nodes (slots handed out in lane order per child)
    int cnt = 1, lo = 0, hi = 1;
    while (lo < hi) {
        for (int k0 = lo; k0 < hi; k0 += 64) {
            const int k = k0 + t;
            const bool act = k < hi;
            const int4 q = act ? node_tail(nodes, g->id[k]) : make_int4(kEmptyChild, kEmptyChild, 0, 0);
            const int32_t c[2] = {q.x, q.y};
            int32_t w[2];
            bool h[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                w[j] = c[j] == kEmptyChild ? 0 : (c[j] < 0 ? 1 : node_tail(nodes, c[j]).w);
                h[j] = act && c[j] >= 0 && w[j] >= heavy;
            }
            int32_t sl[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const unsigned long long m = __ballot(h[j]);
                const int s = cnt + __popcll(m & below);
                sl[j] = (h[j] && s < kRootSlots) ? s : -1;
                if (sl[j] >= 0) g->id[s] = c[j];
                cnt += __popcll(m);
            }
            if (act) {
                g->nl[k] = q.w;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    g->ch[k][j] = c[j];
                    g->cw[k][j] = w[j];
                    g->cs[k][j] = sl[j];
                }
            }
        }
        wave_sync_global();
        lo = hi;
        hi = min(cnt, kRootSlots);
    }
    const int nc = min(cnt, kRootSlots);
    // 2. E: the S - 1 largest cached nodes
    for (int k0 = 0; k0 < nc; k0 += 64) {
        const int k = k0 + t;
        const unsigned long long kk = k < nc ? root_key(g->nl[k], g->id[k]) : ~0ull;
        const int rank = rank_among(g->nl, g->id, nc, kk);
        if (k < nc) g->in_e[k] = rank < S - 1;
    }
    wave_sync_global();
    // 3. the roots: E's children outside E (the whole tree's root when S = 1)
    int nf = 0;
    for (int k0 = 0; k0 < nc; k0 += 64) {
        const int k = k0 + t;
        const bool e = k < nc && g->in_e[k];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            int32_t c = kEmptyChild, s = -1;
            if (e) {
                c = g->ch[k][j];
                s = g->cs[k][j];
            }
            const bool root = e && c != kEmptyChild && !(s >= 0 && g->in_e[s]);
            const unsigned long long m = __ballot(root);
            if (root) {
                const int f = nf + __popcll(m & below);
                g->fc[f] = c;
                g->fw[f] = g->cw[k][j];
            }
            nf += __popcll(m);
        }
    }
    if (!g->in_e[0]) {
        if (t == 0) {
            g->fc[0] = 0;
            g->fw[0] = total;
        }
        nf = 1;
    }
    wave_sync_global();
    // 4. ranks: leaf tiles descending, ties by child index
    for (int k0 = 0; k0 < nf; k0 += 64) {
        const int k = k0 + t;
        const unsigned long long kk = k < nf ? root_key(g->fw[k], g->fc[k]) : ~0ull;
        const int rank = rank_among(g->fw, g->fc, nf, kk);
        if (k < nf) roots[rank] = g->fc[k];
    }
    for (int k = nf + t; k < S; k += 64) roots[k] = kEmptyChild;
    if (t == 0) roots[S] = nf;
}

}  // namespace

// The 4-wide view (Node4): one thread per binary node.  Slot order is the binary order (child 0's
// children, then child 1's), so a fixed-order walk of the 4-wide view visits the leaves in the same
// left-to-right order as a fixed-order binary walk.  A grandchild box lies inside its parent's box, so
// testing it directly prunes at least as tightly as testing both levels.
__global__ __launch_bounds__(64) void k_collapse4(const Node *__restrict__ nodes, int64_t nnodes,
                                                   Node4 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= nnodes) return;
    const Node &n = nodes[i];
    Node4 q;
    int k = 0;
    const auto put = [&](int32_t c, const float *lo, const float *hi) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            q.lo[a][k] = lo[a];
            q.hi[a][k] = hi[a];
        }
        q.child[k] = c;
        ++k;
    };
    for (int c = 0; c < 2; ++c) {
        const int32_t ch = n.child[c];
        if (ch == kEmptyChild) continue;
        if (ch >= 0) {
            const Node &m = nodes[ch];
            for (int d = 0; d < 2; ++d)
                if (m.child[d] != kEmptyChild) put(m.child[d], m.lo[d], m.hi[d]);
        } else {
            put(ch, n.lo[c], n.hi[c]);
        }
    }
    for (; k < 4; ++k) {
#pragma unroll
        for (int a = 0; a < 3; ++a) q.lo[a][k] = q.hi[a][k] = 0.f;
        q.child[k] = kEmptyChild;
    }
    q.pad[0] = q.pad[1] = q.pad[2] = q.pad[3] = 0;
    out[i] = q;
}

hipError_t launch_collapse4(const Node *nodes, int64_t nnodes, Node4 *out, hipStream_t s) {
    if (nnodes <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_collapse4, dim3((unsigned int)((nnodes + 63) / 64)), dim3(64), 0, s, nodes, nnodes, out);
    return hipGetLastError();
}

// A work-root shard's list: the roots rank, rank + count, ... of the size-ordered list (so every shard
// gets large and small subtrees), S2 entries padded with kEmptyChild, their number in out[S2].
__global__ void k_roots_shard(const int32_t *__restrict__ roots, int S, int rank, int count, int S2,
                              int32_t *__restrict__ out) {
    const int n = roots[S];
    const int n2 = n > rank ? (n - rank + count - 1) / count : 0;
    for (int k = threadIdx.x; k < S2; k += blockDim.x) out[k] = k < n2 ? roots[rank + k * count] : kEmptyChild;
    if (threadIdx.x == 0) out[S2] = n2;
}

hipError_t launch_roots_shard(const int32_t *roots, int S, int rank, int count, int S2, int32_t *out,
                              hipStream_t s) {
    hipLaunchKernelGGL(k_roots_shard, dim3(1), dim3(64), 0, s, roots, S, rank, count, S2, out);
    return hipGetLastError();
}

size_t roots_scratch_bytes() { return sizeof(RootsScratch); }

hipError_t launch_roots(const Node *nodes, int S, int32_t *roots, void *scratch, hipStream_t s) {
    hipLaunchKernelGGL(k_roots, dim3(1), dim3(64), 0, s, nodes, S, roots, static_cast<RootsScratch *>(scratch));
    return hipGetLastError();
}

}  // namespace bre
