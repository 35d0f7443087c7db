// ym_k_select.hpp -- K1b select: Karto's order-dependent "value already set" rule, in its three forms (select_kernel; the split
// select_hash / select_neighbours / select_relax kernels; select_global_kernel).  The table, the bucket search, the neighbour
// probes and the decision step of the relaxation are stated once, ahead of the kernels.
// Part of ym_kernels.hpp (include that, not this file).
#pragma once

namespace ym {

// ================================================================== K1b select (only when the smear kernel has taps == 100 off-centre)
// Karto's AddScan skips a point whose cell already holds 100 ("value already set").  With
// smear_deviation >= 9.99 * resolution the four neighbours of an occupied cell are stamped 100 as
// well, so whether a point is rasterised depends on the points before it: a point is EFFECTIVE iff
// no earlier effective point lies on its cell or one of the four beside it (the kernel's 100-valued
// disc; the host refuses a wider one), in Karto's order (base scans in order, beams in order).
//
// Parallel form of that greedy rule.  Only the earliest point of a cell can be effective (a later
// one is knocked out by it, or by whatever knocked it out).  So: (1) hash every cell to its earliest
// point index (LDS, atomicMin); (2) relax the undecided cells: a cell whose earlier neighbours are
// all decided "no" becomes effective, a cell with an effective earlier neighbour is out -- decisions
// are final, so reading a neighbour's fresh or stale state is equally safe, and the globally
// earliest undecided cell always resolves, so the loop ends; (3) erase every point
// that is not the earliest of an effective cell from `cells`.  One block per item.
struct SelectArgs {
    YmCell *cells;        // [B][max_base][max_n]
    int32_t max_n, max_base;
    int32_t log2cap;      // hash capacity = 1 << log2cap entries (dynamic LDS: 9 bytes per entry)
    unsigned long long *stamps;
};

constexpr int SELECT_NT = 1024;  // threads of the one block per item that runs the relaxation
constexpr int SELECT_PMAX = 12;  // points per thread of it: the host sends at most 12 288 readings (3 * capacity >= 4 * readings, capacity <= 2^14)
constexpr int SELECT_NEIGHBOURS = 4; // the plus-shaped disc

__device__ __forceinline__ unsigned select_key(int x, int y) {
    return ((unsigned)(y + 32768) << 16) | ((unsigned)(x + 32768) & 0xffffu);
}
// key of neighbour n of cell (x, y)
__device__ __forceinline__ unsigned select_neighbour_key(int x, int y, int n) {
    constexpr int DX[SELECT_NEIGHBOURS] = {1, -1, 0, 0};
    constexpr int DY[SELECT_NEIGHBOURS] = {0, 0, 1, -1};
    return select_key(x + DX[n], y + DY[n]);
}

// The table is open addressing over BUCKETS of four keys (one 16-byte read per probe; a plain
// linear-probing table made the slowest lane of a wave walk 20-40 slots).  Keys fill a bucket front
// to back and are never removed, so an empty last slot means "not in this bucket or any later one".
struct SelectTable {
    unsigned *keys;       // [cap], in LDS or global memory
    unsigned cap, bmask;  // slots; buckets - 1
    int shift;            // 32 - log2(buckets)
};
// table `item` of the tables of 1 << log2cap slots that start at `base`
__device__ __forceinline__ SelectTable select_table(unsigned *base, int item, int log2cap) {
    SelectTable T;
    T.cap = 1u << log2cap;
    T.bmask = (T.cap >> 2) - 1u;
    T.shift = 32 - (log2cap - 2);
    T.keys = base + (size_t)item * T.cap;
    return T;
}
__device__ __forceinline__ unsigned select_home(const SelectTable &T, unsigned key) { return (key * 2654435761u) >> T.shift; }
__device__ __forceinline__ uint4 select_bucket(const SelectTable &T, unsigned bk) { return *reinterpret_cast<const uint4 *>(T.keys + 4 * bk); }
// where `key` is in bucket bk as read: its slot; -1 = the bucket ends the search without it; -2 = a full bucket without it
__device__ __forceinline__ int select_match(unsigned bk, const uint4 &q, unsigned key) {
    return q.x == key ? (int)(4 * bk) : q.y == key ? (int)(4 * bk + 1) : q.z == key ? (int)(4 * bk + 2) : q.w == key ? (int)(4 * bk + 3) : q.w == 0u ? -1 : -2;
}
// slot of `key`, or -1; the search starts at bucket bk
__device__ __forceinline__ int select_find_from(const SelectTable &T, unsigned bk, unsigned key) {
    for (;;) {
        const int t = select_match(bk, select_bucket(T, bk), key);
        if (t != -2) return t;
        bk = (bk + 1u) & T.bmask;
    }
}
__device__ __forceinline__ int select_find(const SelectTable &T, unsigned key) { return select_find_from(T, select_home(T, key), key); }
// slot of `key`, inserting it if absent
__device__ __forceinline__ int select_insert(const SelectTable &T, unsigned key) {
    unsigned bk = select_home(T, key);
    for (;;) {
        const uint4 q = select_bucket(T, bk);
        int j = (q.x == key || q.x == 0u) ? 0 : (q.y == key || q.y == 0u) ? 1 : (q.z == key || q.z == 0u) ? 2 : (q.w == key || q.w == 0u) ? 3 : 4;
        for (; j < 4; j++) {
            const unsigned prev = atomicCAS(&T.keys[4 * bk + j], 0u, key);
            if (prev == 0u || prev == key) return (int)(4 * bk + j);
        }
        bk = (bk + 1u) & T.bmask;
    }
}

// The four neighbour cells of (x, y), looked up together: select_probe issues the first probe of every one before any is looked
// at (the probes are latency, not bandwidth), select_probed gives neighbour n's slot or -1.
struct SelectProbes {
    unsigned key[SELECT_NEIGHBOURS], bk[SELECT_NEIGHBOURS];
    uint4 q[SELECT_NEIGHBOURS];
};
__device__ __forceinline__ SelectProbes select_probe(const SelectTable &T, int x, int y) {
    SelectProbes p;
#pragma unroll
    for (int n = 0; n < SELECT_NEIGHBOURS; n++) {
        p.key[n] = select_neighbour_key(x, y, n);
        p.bk[n] = select_home(T, p.key[n]);
        p.q[n] = select_bucket(T, p.bk[n]);
    }
    return p;
}
__device__ __forceinline__ int select_probed(const SelectTable &T, const SelectProbes &p, int n) {
    int t = select_match(p.bk[n], p.q[n], p.key[n]);
    if (t == -2) t = select_find_from(T, (p.bk[n] + 1u) & T.bmask, p.key[n]); // (a full bucket without the key: go on)
    return t;
}

// The states of the cells (0 undecided, 1 effective, 2 out), as the relaxation reads and writes them: bytes in LDS, or words in
// global memory through relaxed agent-scope atomics.
struct SelectStatesLds {
    unsigned char *p;
    __device__ __forceinline__ unsigned get(unsigned s) const { return p[s]; }
    __device__ __forceinline__ void set(unsigned s, unsigned v) const { p[s] = (unsigned char)v; }
};
struct SelectStatesGlobal {
    unsigned *p;
    __device__ __forceinline__ unsigned get(unsigned s) const { return __hip_atomic_load(&p[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void set(unsigned s, unsigned v) const { __hip_atomic_store(&p[s], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
// One step of the relaxation for the cell at slot s, whose neighbour cells with an earlier point are at slots nb_of(j) (`none`:
// no such neighbour): out if one of them is effective, effective if all of them are out, else still undecided.  A decision is
// final and is taken only from final states (a stale "undecided" read merely delays it).  Returns whether the cell is decided.
template <typename STATES, typename NEIGHBOUR>
__device__ __forceinline__ bool select_decide(const STATES &st, unsigned s, unsigned none, NEIGHBOUR nb_of) {
    bool knocked = false, pending = false;
#pragma unroll
    for (int j = 0; j < SELECT_NEIGHBOURS; j++) {
        const unsigned t = nb_of(j);
        if (t != none) {
            const unsigned stt = st.get(t);
            knocked |= stt == 1u;
            pending |= stt == 0u;
        }
    }
    if (knocked) st.set(s, 2u);
    else if (!pending) st.set(s, 1u);
    else return false;
    return true;
}
// bit k: some lane of the wave has bit k of `und` set (the points of the wave's threads that are still undecided)
__device__ __forceinline__ unsigned select_wave_undecided(unsigned und) {
    unsigned wmask = 0;
#pragma unroll
    for (int k = 0; k < SELECT_PMAX; k++) wmask |= __ballot((und >> k) & 1u) ? (1u << k) : 0u;
    return wmask;
}

__global__ __launch_bounds__(SELECT_NT) void select_kernel(SelectArgs a) {
    constexpr int NT = SELECT_NT, PMAX = SELECT_PMAX;
    extern __shared__ unsigned sel_lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const SelectTable T = select_table(sel_lds, 0, a.log2cap);
    unsigned *keys = T.keys;
    unsigned *minidx = sel_lds + T.cap;
    unsigned char *status = reinterpret_cast<unsigned char *>(sel_lds + 2 * T.cap);
    YM_STAMP(a, 24);
    // The thread's points: all loaded at once and kept for step (3), with the slots step (1) finds for them.  (The one block
    // of an item is a latency chain: a load per loop trip -- which the stores of step (3) into the same array keep the
    // compiler from moving -- cost steps (1) and (3) a memory round trip per point, 14 + 58 of the kernel's 118 us.)
    YmCell *cells = a.cells + (size_t)b * a.max_base * a.max_n;
    const int total = a.max_base * a.max_n;
    int2 mine[PMAX];
    unsigned short slot_of[PMAX];
    // A thread takes `per` CONSECUTIVE points and, in steps (2a) / (2b), decides the cells whose earliest point is one of
    // them, in that order: the earlier neighbours of a cell are mostly the cells of the beams just before it, so a wall's
    // chain of dependent decisions resolves inside one thread in one sweep instead of hopping from thread to thread once
    // per sweep (the relaxation took 53 of the kernel's 111 us while a thread owned hash SLOTS).
    const int per = (total + NT - 1) / NT, e0 = tid * per;
#pragma unroll
    for (int q = 0; q < PMAX; q++) {
        const int e = e0 + q;
        mine[q] = (q < per && e < total) ? ym_cell_unpack(cells[e]) : make_int2(YM_CELL_NONE, YM_CELL_NONE);
    }
    for (unsigned i = tid; i < T.cap; i += NT) { keys[i] = 0u; minidx[i] = 0xffffffffu; status[i] = 0; }
    __syncthreads();
    YM_STAMP(a, 25);
    // (1) cell -> earliest point index
#pragma unroll
    for (int q = 0; q < PMAX; q++) {
        slot_of[q] = 0;
        if (mine[q].x == YM_CELL_NONE) continue;
        const int slot = select_insert(T, select_key(mine[q].x, mine[q].y));
        slot_of[q] = (unsigned short)slot;
        atomicMin(&minidx[slot], (unsigned)(e0 + q));
    }
    __syncthreads();
    YM_STAMP(a, 26);
    // (2a) per owned cell (= owned point that is the earliest of its cell): the slots of the neighbour cells that hold an
    // EARLIER point, packed as 16-bit slot numbers (0xffff = none).  A cell with no earlier neighbour is effective.
    unsigned long long nb[PMAX];
    unsigned und = 0;
#pragma unroll
    for (int k = 0; k < PMAX; k++) {
        nb[k] = ~0ull;
        if (mine[k].x == YM_CELL_NONE) continue;
        const unsigned s = slot_of[k], me = (unsigned)(e0 + k);
        if (minidx[s] != me) continue; // a later point of its cell: never effective, nothing to decide
        bool any = false;
        const SelectProbes pr = select_probe(T, mine[k].x, mine[k].y);
#pragma unroll
        for (int j = 0; j < SELECT_NEIGHBOURS; j++) {
            const int t = select_probed(T, pr, j);
            if (t >= 0 && minidx[t] < me) {
                any = true;
                nb[k] &= ~(0xffffull << (16 * j));
                nb[k] |= (unsigned long long)(unsigned)t << (16 * j);
            }
        }
        if (any) und |= 1u << k;
        else status[s] = 1;
    }
    YM_STAMP(a, 3);
    // (2b) asynchronous relaxation, no barriers: every wave keeps re-reading the state of the earlier
    // neighbours of its undecided cells.  All 16 waves of the block are resident, so
    // this terminates with the sequential greedy result whatever the interleaving.
    const SelectStatesLds vst = {status};
    unsigned wmask = select_wave_undecided(und);
    while (wmask) {
        unsigned m = wmask;
        while (m) {
            const int k = __builtin_ctz(m); // wave-uniform
            m &= m - 1;
            bool still = false;
            asm volatile("" ::: "memory"); // re-read the states every time
            if ((und >> k) & 1u) {
                still = !select_decide(vst, slot_of[k], 0xffffu, [&](int j) { return (unsigned)(nb[k] >> (16 * j)) & 0xffffu; });
                if (!still) und &= ~(1u << k);
            }
            if (__ballot(still) == 0ull) wmask &= ~(1u << k);
        }
    }
    __syncthreads();
    YM_STAMP(a, 30);
    // (3) keep only the earliest point of every effective cell
#pragma unroll
    for (int q = 0; q < PMAX; q++) {
        if (mine[q].x == YM_CELL_NONE) continue;
        const int e = e0 + q, t = slot_of[q];
        if (!(status[t] == 1 && minidx[t] == (unsigned)e)) cells[e] = ym_cell_none();
    }
    YM_STAMP(a, 31);
}

// ---- the same rule on a FEW items, split by what is parallel and what is not.  Steps (1) and (2a) of
// select_kernel are parallel work that one block does alone: 45 of its 79 us are 16 waves issuing ~4000 instructions each on
// one CU.  Here they are two launches over all points (hash and earliest-point table in global memory, left zeroed for the
// next call), and the one block per item that remains only runs the chain of dependent decisions (2b) and the erase (3) from
// a 16-byte record per point (SelectSplitArgs::rec): rec.x = slot | owned << 16 | effective << 17 (0xffffffff: no point), rec.y / rec.z = the slots of
// the neighbour cells with an earlier point, 16 bits each (0xffff: none).
struct SelectSplitArgs {
    YmCell *cells;        // [B][max_base][max_n]
    int32_t max_n, max_base;
    int32_t log2cap, pad;
    unsigned *keys;       // [B][cap]  zero between calls
    unsigned *mx;         // [B][cap]  zero between calls: max over the cell's points of ~index (= its earliest point)
    unsigned *slot_of;    // [B][max_base * max_n]  the point's slot (0xffffffff: no cell)
    uint4 *rec;           // [B][12 * 1024]  the record of point e = t * per + q at [q * 1024 + t]: thread t of select_relax_kernel reads its
                          //                 `per` = ceil(points / 1024) consecutive points with coalesced loads
    unsigned long long *stamps;
};
#define YM_SELECT_SPLIT_THREADS 256
// (1) grid (ceil(total / 256), B)
__global__ __launch_bounds__(YM_SELECT_SPLIT_THREADS) void select_hash_kernel(SelectSplitArgs a) {
    const int b = blockIdx.y, e = blockIdx.x * YM_SELECT_SPLIT_THREADS + threadIdx.x;
    const int total = a.max_base * a.max_n;
    if (e >= total) return;
    const int2 c = ym_cell_unpack(a.cells[(size_t)b * total + e]);
    unsigned slot = 0xffffffffu;
    if (c.x != YM_CELL_NONE) {
        const SelectTable T = select_table(a.keys, b, a.log2cap);
        slot = (unsigned)select_insert(T, select_key(c.x, c.y));
        atomicMax(&a.mx[(size_t)b * T.cap + slot], ~(unsigned)e);
    }
    a.slot_of[(size_t)b * total + e] = slot;
}
// (2a) grid (ceil(total / 256), B)
__global__ __launch_bounds__(YM_SELECT_SPLIT_THREADS) void select_neighbours_kernel(SelectSplitArgs a) {
    const int b = blockIdx.y, e = blockIdx.x * YM_SELECT_SPLIT_THREADS + threadIdx.x;
    const int total = a.max_base * a.max_n;
    if (e >= total) return;
    const SelectTable T = select_table(a.keys, b, a.log2cap);
    const unsigned *mx = a.mx + (size_t)b * T.cap;
    const int per = (total + SELECT_NT - 1) / SELECT_NT;
    uint4 *rec = a.rec + (size_t)b * SELECT_PMAX * SELECT_NT + (size_t)(e % per) * SELECT_NT + e / per;
    const unsigned s = a.slot_of[(size_t)b * total + e];
    const int2 c = ym_cell_unpack(a.cells[(size_t)b * total + e]); // (a point without a cell: YM_CELL_NONE, any bucket)
    // the first probes leave before the point's own entry is looked at: one round trip, not two
    const SelectProbes pr = select_probe(T, c.x, c.y);
    if (s == 0xffffffffu) {
        *rec = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0u);
        return;
    }
    const unsigned mine = ~(unsigned)e;
    if (mx[s] != mine) { // a later point of its cell: never effective, nothing to decide
        *rec = make_uint4(s, 0xffffffffu, 0xffffffffu, 0u);
        return;
    }
    int tn[SELECT_NEIGHBOURS];
#pragma unroll
    for (int n = 0; n < SELECT_NEIGHBOURS; n++) tn[n] = select_probed(T, pr, n);
    unsigned mt[SELECT_NEIGHBOURS];
#pragma unroll
    for (int n = 0; n < SELECT_NEIGHBOURS; n++) mt[n] = mx[tn[n] >= 0 ? tn[n] : (int)s]; // (the four entries together)
    unsigned nbv[SELECT_NEIGHBOURS];
    bool any = false;
#pragma unroll
    for (int n = 0; n < SELECT_NEIGHBOURS; n++) {
        const bool earlier = tn[n] >= 0 && mt[n] > mine; // (~index larger = index smaller)
        nbv[n] = earlier ? (unsigned)tn[n] : 0xffffu;
        any |= earlier;
    }
    *rec = make_uint4(s | 1u << 16 | (any ? 0u : 1u << 17), nbv[0] | nbv[1] << 16, nbv[2] | nbv[3] << 16, 0u);
}
// (2b) + (3): grid (B), 1024 threads, dynamic LDS = one state byte per slot
__global__ __launch_bounds__(SELECT_NT) void select_relax_kernel(SelectSplitArgs a) {
    constexpr int NT = SELECT_NT, PMAX = SELECT_PMAX;
    extern __shared__ unsigned sel_lds[];
    unsigned char *status = reinterpret_cast<unsigned char *>(sel_lds);
    const int b = blockIdx.x, tid = threadIdx.x;
    const unsigned cap = 1u << a.log2cap;
    const int total = a.max_base * a.max_n;
    YmCell *cells = a.cells + (size_t)b * total;
    const uint4 *rec = a.rec + (size_t)b * PMAX * NT;
    // a thread takes `per` CONSECUTIVE points (see select_kernel: a wall's chain of decisions resolves inside one thread)
    const int per = (total + NT - 1) / NT, e0 = tid * per;
    YM_STAMP(a, 24);
    uint4 r[PMAX];
#pragma unroll
    for (int q = 0; q < PMAX; q++) {
        const int e = e0 + q;
        r[q] = (q < per && e < total) ? rec[q * NT + tid] : make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0u);
    }
    for (unsigned i = tid; i < cap / 4; i += NT) sel_lds[i] = 0u;
    __syncthreads();
    unsigned und = 0;
#pragma unroll
    for (int q = 0; q < PMAX; q++) {
        if (r[q].x == 0xffffffffu || !(r[q].x & (1u << 16))) continue;
        if (r[q].x & (1u << 17)) status[r[q].x & 0xffffu] = 1;
        else und |= 1u << q;
    }
    YM_STAMP(a, 3);
    // asynchronous relaxation, no barriers (select_kernel, step (2b))
    const SelectStatesLds vst = {status};
    unsigned wmask = select_wave_undecided(und);
    while (wmask) {
#pragma unroll
        for (int k = 0; k < PMAX; k++) { // (unrolled: r[k] stays in registers; a point without undecided lanes costs a scalar test)
            if (!((wmask >> k) & 1u)) continue;
            bool still = false;
            asm volatile("" ::: "memory"); // re-read the states every time
            if ((und >> k) & 1u) {
                const unsigned nbs[SELECT_NEIGHBOURS] = {r[k].y & 0xffffu, r[k].y >> 16, r[k].z & 0xffffu, r[k].z >> 16};
                still = !select_decide(vst, r[k].x & 0xffffu, 0xffffu, [&](int j) { return nbs[j]; });
                if (!still) und &= ~(1u << k);
            }
            if (__ballot(still) == 0ull) wmask &= ~(1u << k);
        }
    }
    __syncthreads();
    YM_STAMP(a, 30);
    // (3) keep only the earliest point of every effective cell
#pragma unroll
    for (int q = 0; q < PMAX; q++) {
        if (r[q].x == 0xffffffffu) continue;
        if (!((r[q].x & (1u << 16)) && status[r[q].x & 0xffffu] == 1)) cells[e0 + q] = ym_cell_none();
    }
    // the tables as the next call expects them
    uint4 *k4 = reinterpret_cast<uint4 *>(a.keys + (size_t)b * cap), *m4 = reinterpret_cast<uint4 *>(a.mx + (size_t)b * cap);
    for (unsigned i = tid; i < cap / 4; i += NT) { k4[i] = make_uint4(0u, 0u, 0u, 0u); m4[i] = make_uint4(0u, 0u, 0u, 0u); }
    YM_STAMP(a, 31);
}

// ---- the same rule for chains too long for one CU's LDS (more than 12 288 readings): hash, earliest-point index, neighbour
// lists and states live in global memory (one 1024-thread block per item again -- the relaxation is a chain of
// dependent decisions, not a parallel job -- but its reads now cost an L2 round trip instead of an LDS one).  LDS only
// holds each thread's shrinking list of undecided slots.  Capacity 2^17 slots = 98 304 readings at load factor 0.75.
struct SelectGlobalArgs {
    YmCell *cells;        // [B][max_base][max_n]
    int32_t max_n, max_base;
    int32_t log2cap;
    unsigned *keys;       // [B][cap]           zeroed by the host
    unsigned *status;     // [B][cap]           zeroed by the host: 0 undecided, 1 effective, 2 out
    unsigned *minidx;     // [B][cap]           set to 0xffffffff by the host
    unsigned *nbr;        // [B][4][cap]        slot of the neighbour cell if it holds an earlier point, else 0xffffffff
};

__global__ __launch_bounds__(SELECT_NT) void select_global_kernel(SelectGlobalArgs a) {
    constexpr int NT = SELECT_NT;
    extern __shared__ unsigned char und_list[]; // [cap / NT][NT]: ordinals k of the slots tid + k * NT still undecided
    const int b = blockIdx.x, tid = threadIdx.x;
    const SelectTable T = select_table(a.keys, b, a.log2cap);
    const unsigned cap = T.cap;
    unsigned *keys = T.keys, *minidx = a.minidx + (size_t)b * cap;
    const SelectStatesGlobal status = {a.status + (size_t)b * cap};
    unsigned *nbr = a.nbr + (size_t)b * SELECT_NEIGHBOURS * cap;
    YmCell *cells = a.cells + (size_t)b * a.max_base * a.max_n;
    const int total = a.max_base * a.max_n;
    // (1) cell -> earliest point index
    for (int e = tid; e < total; e += NT) {
        const int2 c = ym_cell_unpack(cells[e]);
        if (c.x == YM_CELL_NONE) continue;
        const int slot = select_insert(T, select_key(c.x, c.y));
        atomicMin(&minidx[slot], (unsigned)e);
    }
    // the tables were built by atomics in L2: make them visible to this CU's plain loads (its L1 may hold lines fetched
    // while they were still being filled)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // (2a) earlier neighbours of every cell; a cell without one is effective
    int n_und = 0;
    for (unsigned s = tid, k = 0; s < cap; s += NT, k++) {
        const unsigned key = keys[s];
        if (key == 0u) continue;
        const unsigned me = minidx[s];
        const int x = (int)(key & 0xffffu) - 32768, y = (int)(key >> 16) - 32768;
        bool any = false;
#pragma unroll
        for (int n = 0; n < SELECT_NEIGHBOURS; n++) {
            const int t = select_find(T, select_neighbour_key(x, y, n));
            const bool earlier = t >= 0 && minidx[t] < me;
            nbr[(size_t)n * cap + s] = earlier ? (unsigned)t : 0xffffffffu;
            any |= earlier;
        }
        if (any) und_list[(size_t)(n_und++) * NT + tid] = (unsigned char)k;
        else status.set(s, 1u);
    }
    // (2b) asynchronous relaxation (see select_kernel): every wave of the block is resident, so the earliest undecided cell
    // always gets decided
    while (__ballot(n_und > 0)) {
        int kept = 0;
        for (int i = 0; i < n_und; i++) {
            const unsigned k = und_list[(size_t)i * NT + tid], s = tid + k * NT;
            if (!select_decide(status, s, 0xffffffffu, [&](int j) { return nbr[(size_t)j * cap + s]; })) und_list[(size_t)(kept++) * NT + tid] = (unsigned char)k;
        }
        n_und = kept;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // (3) keep only the earliest point of every effective cell
    for (int e = tid; e < total; e += NT) {
        const int2 c = ym_cell_unpack(cells[e]);
        if (c.x == YM_CELL_NONE) continue;
        const int t = select_find(T, select_key(c.x, c.y));
        if (!(t >= 0 && status.get((unsigned)t) == 1u && minidx[t] == (unsigned)e)) cells[e] = ym_cell_none();
    }
}

}  // namespace ym
