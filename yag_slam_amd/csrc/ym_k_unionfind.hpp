// ym_k_unionfind.hpp -- the union-find of the component stages (ym_k_segmenter.hpp seg_cc_*, ym_k_despeckle.hpp dsp_*): cells are
// raster indices, parent[i] <= i, and a union links the higher root under the lower with atomicMin, so the root of a component is
// its first cell whatever the order of arrival.  Which cells are joined, and over what grid, is the caller's.  Plain C++ and vector
// memory operations only.  Part of ym_kernels.hpp.
#pragma once

namespace ym {

constexpr unsigned kUnionCap = 1u << 22; // retries of one union (each one means another thread linked the same root)

// the root of i: parents only ever decrease, so the walk ends within i steps
__device__ __forceinline__ unsigned uf_find(const unsigned *parent, unsigned i) {
    unsigned p = parent[i];
    while (p < i) { // (bounded: a strictly decreasing index)
        i = p;
        p = parent[i];
    }
    return i;
}

// false: kUnionCap retries did not settle it; the caller raises its error word and the host fails the call
__device__ __forceinline__ bool uf_union(unsigned *parent, unsigned i, unsigned j) {
#pragma unroll 1
    for (unsigned it = 0; it < kUnionCap; it++) {
        i = uf_find(parent, i);
        j = uf_find(parent, j);
        if (i == j) return true;
        if (i < j) {
            const unsigned s = i;
            i = j;
            j = s;
        }
        const unsigned old = atomicMin(&parent[i], j); // i > j: link the higher root under the lower
        if (old == i) return true;
        i = old; // i was linked meanwhile: go on from where it points
    }
    return false;
}

// Called by every lane of a wave once the forest is final, `live` for the lanes that hold a cell i: the cell's parent becomes its
// root and every root's size grows by its cells, with one atomic per distinct root of the wave's 64 cells.
__device__ __forceinline__ void uf_wave_sizes(bool live, unsigned i, unsigned *parent, unsigned *size) {
    unsigned long long todo = __ballot(live);
    const int lane = threadIdx.x & 63;
    unsigned root = 0;
    if (live) {
        root = uf_find(parent, i);
        parent[i] = root; // (a reader sees the old parent or the root, both lead to the root)
    }
#pragma unroll 1
    for (int it = 0; it < 64 && todo; it++) {
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned r = (unsigned)__shfl((int)root, leader, 64);
        const unsigned long long same = __ballot(live && root == r) & todo;
        if (lane == leader) atomicAdd(&size[r], (unsigned)__popcll(same));
        todo &= ~same;
    }
}

}  // namespace ym
