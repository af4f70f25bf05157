// reorder_kernels.hip.h — part of libqgtc_hip.so (included by qgtc_reorder.hip): node reordering for the tile-compressed adjacency
// (include/qgtc.h, "Node reordering") - size-capped label propagation on the symmetrised graph, then the
// nodes sorted by (label, id).
//
// Neighbour lists: every valid edge s -> d with s != d gives the 46-bit entry keys (s << 23 | d) and (d << 23 | s); one radix sort
// orders them by (node, neighbour), and the first entry of every node gives the row offsets. The nodes are then listed by (degree
// class, parity, id): a sweep t proposes new labels only for the nodes with (x + t) even, and a node's list is read by 16 lanes (up to
// 16 entries), one wave (up to 256) or one workgroup (more: a hash table in the work buffer). A sweep is two launches, both returning
// at once when the two sweeps before changed no label, so the host queues every sweep without reading anything back.
#pragma once

namespace {

constexpr int REORDER_MAX_N = TILED_MAX_N;   // tiled_args.hip.h, included before this file: node ids fit the 23 bits of the keys below
constexpr int REORDER_MAX_SWEEPS = 64;
constexpr uint64_t REORDER_INVALID = (1ull << 46) - 1;   // entry key of a skipped edge: sorts after every valid key (u = v = 2^23 - 1)
constexpr unsigned REORDER_KEY_BITS = 46;
constexpr unsigned REORDER_CLASS_BITS = 26;               // class (0 .. 6) << 23 | node
constexpr uint32_t REORDER_NODE_MASK = (1u << 23) - 1;
constexpr uint32_t REORDER_EMPTY = ~0u;                    // no label (labels are node ids < 2^23)
constexpr int REORDER_SHORT = 16, REORDER_MEDIUM = 256;    // list lengths read by 16 lanes / one wave; longer: one workgroup
constexpr int REORDER_CLASSES = 7;                         // 2 * {short, medium, hub} + parity, then the nodes without entries

__host__ __device__ __forceinline__ uint32_t reorder_mix32(uint32_t x) {   // lowbias32
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// order of a candidate label: more entries first, then the smaller h_t(l) (h_t is a bijection, so no two labels tie on it)
__device__ __forceinline__ uint64_t reorder_rank_key(uint32_t count, uint32_t l, uint32_t salt) {
    return (static_cast<uint64_t>(count) << 32) | static_cast<uint64_t>(~reorder_mix32(l ^ salt));
}

// sweep t runs unless sweeps t - 1 and t - 2 both changed no label
__device__ __forceinline__ bool reorder_stopped(const uint32_t *__restrict__ changed, int t) {
    return t >= 2 && changed[t - 1] == 0 && changed[t - 2] == 0;
}

__device__ __forceinline__ uint32_t reorder_node_of(uint64_t key, int n) {
    return key == REORDER_INVALID ? static_cast<uint32_t>(n) : static_cast<uint32_t>(key >> 23);
}

#define REORDER_GRID_STRIDE(i, count)                                                                                              \
    for (uint64_t i = blockIdx.x * static_cast<uint64_t>(blockDim.x) + threadIdx.x; i < (count);                                   \
         i += static_cast<uint64_t>(gridDim.x) * blockDim.x)

__global__ void k_reorder_entry_keys(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, uint64_t n_edges, int n,
                                     uint64_t *__restrict__ keys, int *__restrict__ bad_index) {
    REORDER_GRID_STRIDE(i, n_edges) {
        const int64_t s = src[i], d = dst[i];
        const bool ok = s >= 0 && s < n && d >= 0 && d < n;
        if (!ok && bad_index) *bad_index = 1;
        const bool use = ok && s != d;
        keys[2 * i] = use ? (static_cast<uint64_t>(s) << 23 | static_cast<uint64_t>(d)) : REORDER_INVALID;
        keys[2 * i + 1] = use ? (static_cast<uint64_t>(d) << 23 | static_cast<uint64_t>(s)) : REORDER_INVALID;
    }
}

// bad_index only (no sweep to run)
__global__ void k_reorder_check(const int64_t *__restrict__ src, const int64_t *__restrict__ dst, uint64_t n_edges, int n,
                                int *__restrict__ bad_index) {
    REORDER_GRID_STRIDE(i, n_edges) {
        const int64_t s = src[i], d = dst[i];
        if (!(s >= 0 && s < n && d >= 0 && d < n)) *bad_index = 1;
    }
}

// off[u] = first sorted entry of node u (off[n] = valid entries), nbr[i] = the neighbour of entry i. Entry i writes the offsets of
// the nodes after entry i - 1's node up to its own, so every offset is written once.
__global__ void k_reorder_offsets(const uint64_t *__restrict__ sorted, uint64_t m, int n, uint64_t *__restrict__ off,
                                  uint32_t *__restrict__ nbr) {
    REORDER_GRID_STRIDE(i, m + 1) {
        const int64_t ui = i < m ? reorder_node_of(sorted[i], n) : n;
        const int64_t up = i > 0 ? static_cast<int64_t>(reorder_node_of(sorted[i - 1], n)) : -1;
        for (int64_t u = up + 1; u <= ui; ++u) off[u] = i;
        if (i < m && ui < n) nbr[i] = static_cast<uint32_t>(sorted[i]) & REORDER_NODE_MASK;
    }
}

__global__ void k_reorder_class_keys(const uint64_t *__restrict__ off, int n, uint64_t *__restrict__ keys) {
    REORDER_GRID_STRIDE(x, static_cast<uint64_t>(n)) {
        const uint64_t d = off[x + 1] - off[x];
        const uint64_t cls = d == 0 ? 6 : (d <= REORDER_SHORT ? 0 : (d <= REORDER_MEDIUM ? 2 : 4)) + (x & 1);
        keys[x] = cls << 23 | x;
    }
}

// order[i] = the i-th node by (class, id); seg[c] = first position of class c (seg[7] = n)
__global__ void k_reorder_segments(const uint64_t *__restrict__ sorted, int n, uint32_t *__restrict__ order, uint32_t *__restrict__ seg) {
    REORDER_GRID_STRIDE(i, static_cast<uint64_t>(n) + 1) {
        const int ci = i < static_cast<uint64_t>(n) ? static_cast<int>(sorted[i] >> 23) : REORDER_CLASSES;
        const int cp = i > 0 ? static_cast<int>(sorted[i - 1] >> 23) : -1;
        for (int c = cp + 1; c <= ci; ++c) seg[c] = static_cast<uint32_t>(i);
        if (i < static_cast<uint64_t>(n)) order[i] = static_cast<uint32_t>(sorted[i]) & REORDER_NODE_MASK;
    }
}

__global__ void k_reorder_init(int n, uint32_t *__restrict__ label) {
    REORDER_GRID_STRIDE(x, static_cast<uint64_t>(n)) label[x] = static_cast<uint32_t>(x);
}

__device__ __forceinline__ void reorder_propose(uint32_t x, uint32_t best, uint32_t *__restrict__ prop, int *__restrict__ size) {
    prop[x] = best;
    atomicAdd(size + best, 1);
}

// Sweep t, first launch: prop[x] for every node and size[l] = the number of nodes proposing l (size cleared by the previous sweep's
// second launch). Every loop below is uniform over the lanes that take part in its shuffles and barriers.
__global__ __launch_bounds__(256) void k_reorder_sweep(int t, int n, const uint64_t *__restrict__ off, const uint32_t *__restrict__ nbr,
                                                       const uint32_t *__restrict__ order, const uint32_t *__restrict__ seg,
                                                       const uint32_t *__restrict__ label, uint32_t *__restrict__ prop,
                                                       int *__restrict__ size, const uint32_t *__restrict__ changed,
                                                       uint32_t *__restrict__ hkey, uint32_t *__restrict__ hcount) {
    if (reorder_stopped(changed, t)) return;
    const uint32_t salt = 0x9E3779B9u * static_cast<uint32_t>(t + 1);
    const int par = t & 1;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint64_t wave = blockIdx.x * static_cast<uint64_t>(blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint64_t waves = gridDim.x * static_cast<uint64_t>(blockDim.x >> 6);

    // nodes that keep their label: the other parity, or no neighbour entries
    REORDER_GRID_STRIDE(x, static_cast<uint64_t>(n)) {
        if ((static_cast<int>(x & 1) != par) || off[x + 1] == off[x]) reorder_propose(static_cast<uint32_t>(x), label[x], prop, size);
    }

    // short lists: 16 lanes a node, lane j holds entry j; its count is the number of lanes of the group with the same label
    {
        const uint64_t s0 = seg[par], s1 = seg[par + 1];
        const int sub = lane >> 4, sl = lane & 15;
        for (uint64_t base = s0 + wave * 4; base < s1; base += waves * 4) {
            const uint64_t i = base + sub;
            uint32_t x = 0, L = REORDER_EMPTY;
            if (i < s1) {
                x = order[i];
                const uint64_t o = off[x], d = off[x + 1] - o;
                if (static_cast<uint64_t>(sl) < d) L = label[nbr[o + sl]];
            }
            uint32_t c = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k) c += __shfl(L, k, 16) == L;
            uint64_t key = L != REORDER_EMPTY ? reorder_rank_key(c, L, salt) : 0;
#pragma unroll
            for (int m = 8; m >= 1; m >>= 1) {
                const uint64_t ok = __shfl_xor(key, m, 16);
                const uint32_t oL = __shfl_xor(L, m, 16);
                if (ok > key) key = ok, L = oL;
            }
            if (i < s1 && sl == 0) reorder_propose(x, L, prop, size);
        }
    }

    // medium lists: one wave a node, lane j holds entries j, j + 64, j + 128, j + 192; the entries are broadcast one by one
    {
        const uint64_t s0 = seg[2 + par], s1 = seg[3 + par];
        for (uint64_t i = s0 + wave; i < s1; i += waves) {
            const uint32_t x = __builtin_amdgcn_readfirstlane(order[i]);
            const uint64_t o = off[x];
            const int d = __builtin_amdgcn_readfirstlane(static_cast<int>(off[x + 1] - o));
            uint32_t L[4], c[4] = {0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < 4; ++r) L[r] = lane + 64 * r < d ? label[nbr[o + lane + 64 * r]] : REORDER_EMPTY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kn = d - 64 * r < 64 ? d - 64 * r : 64;
                for (int k = 0; k < kn; ++k) {
                    const uint32_t Lk = __builtin_amdgcn_readlane(L[r], k);
#pragma unroll
                    for (int q = 0; q < 4; ++q) c[q] += L[q] == Lk;
                }
            }
            uint64_t key = 0;
            uint32_t bl = REORDER_EMPTY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint64_t kr = L[r] != REORDER_EMPTY ? reorder_rank_key(c[r], L[r], salt) : 0;
                if (kr > key) key = kr, bl = L[r];
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const uint64_t ok = __shfl_xor(key, m);
                const uint32_t oL = __shfl_xor(bl, m);
                if (ok > key) key = ok, bl = oL;
            }
            if (lane == 0) reorder_propose(x, bl, prop, size);
        }
    }

    // hub lists: one workgroup a node; an open-addressing table of 2d slots at [2 off[x], 2 off[x + 1]) of hkey / hcount (disjoint for
    // different nodes, at most half full) counts the labels with integer atomics, then the workgroup takes the best slot
    {
        __shared__ uint64_t red_key[4];
        __shared__ uint32_t red_label[4];
        const uint64_t s0 = seg[4 + par], s1 = seg[5 + par];
        for (uint64_t i = s0 + blockIdx.x; i < s1; i += gridDim.x) {
            const uint32_t x = order[i];
            const uint64_t o = off[x], d = off[x + 1] - o, cap = 2 * d;
            uint32_t *hk = hkey + 2 * o, *hc = hcount + 2 * o;
            for (uint64_t j = tid; j < cap; j += blockDim.x) {
                hk[j] = REORDER_EMPTY;
                hc[j] = 0;
            }
            __threadfence();
            __syncthreads();
            for (uint64_t j = tid; j < d; j += blockDim.x) {
                const uint32_t L = label[nbr[o + j]];
                uint64_t s = reorder_mix32(L) % cap;
                for (;;) {
                    const uint32_t prev = atomicCAS(hk + s, REORDER_EMPTY, L);
                    if (prev == REORDER_EMPTY || prev == L) {
                        atomicAdd(hc + s, 1u);
                        break;
                    }
                    s = s + 1 == cap ? 0 : s + 1;
                }
            }
            __threadfence();
            __syncthreads();
            uint64_t key = 0;
            uint32_t bl = REORDER_EMPTY;
            for (uint64_t j = tid; j < cap; j += blockDim.x) {
                const uint32_t k = __hip_atomic_load(hk + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (k == REORDER_EMPTY) continue;
                const uint64_t kr = reorder_rank_key(__hip_atomic_load(hc + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), k, salt);
                if (kr > key) key = kr, bl = k;
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const uint64_t ok = __shfl_xor(key, m);
                const uint32_t oL = __shfl_xor(bl, m);
                if (ok > key) key = ok, bl = oL;
            }
            if (lane == 0) red_key[tid >> 6] = key, red_label[tid >> 6] = bl;
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < static_cast<int>(blockDim.x >> 6); ++w)
                    if (red_key[w] > key) key = red_key[w], bl = red_label[w];
                reorder_propose(x, bl, prop, size);
            }
            __syncthreads();
        }
    }
}

// Sweep t, second launch: accept a proposal when it is the current label or its community holds at most `cap` proposers; count the
// waves with a change into changed[t]; clear the other size array for sweep t + 1.
__global__ __launch_bounds__(256) void k_reorder_accept(int t, int n, int cap, uint32_t *__restrict__ label,
                                                        const uint32_t *__restrict__ prop, const int *__restrict__ size,
                                                        int *__restrict__ size_next, uint32_t *__restrict__ changed) {
    if (reorder_stopped(changed, t)) return;
    bool any = false;
    REORDER_GRID_STRIDE(x, static_cast<uint64_t>(n)) {
        const uint32_t l = label[x], p = prop[x];
        if (p != l && size[p] <= cap) {
            label[x] = p;
            any = true;
        }
        size_next[x] = 0;
    }
    if (__ballot(any) && (threadIdx.x & 63) == 0) atomicAdd(changed + t, 1u);
}

__global__ void k_reorder_rank_keys(const uint32_t *__restrict__ label, int n, uint64_t *__restrict__ keys) {
    REORDER_GRID_STRIDE(x, static_cast<uint64_t>(n)) keys[x] = static_cast<uint64_t>(label[x]) << 23 | x;
}

__global__ void k_reorder_perm(const uint64_t *__restrict__ sorted, int n, int64_t *__restrict__ perm, int64_t *__restrict__ rank) {
    REORDER_GRID_STRIDE(i, static_cast<uint64_t>(n)) {
        const uint32_t x = static_cast<uint32_t>(sorted[i]) & REORDER_NODE_MASK;
        perm[i] = x;
        if (rank) rank[x] = static_cast<int64_t>(i);
    }
}

__global__ void k_reorder_identity(int n, int64_t *__restrict__ perm, int64_t *__restrict__ rank) {
    REORDER_GRID_STRIDE(i, static_cast<uint64_t>(n)) {
        perm[i] = static_cast<int64_t>(i);
        if (rank) rank[i] = static_cast<int64_t>(i);
    }
}

#undef REORDER_GRID_STRIDE

}  // namespace
