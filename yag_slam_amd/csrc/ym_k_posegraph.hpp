// ym_k_posegraph.hpp -- 2-D pose-graph optimisation in fp64 (Konolige et al., "Efficient Sparse Pose Adjustment for 2D
// Mapping", 2010): the kernels of one Levenberg-Marquardt step.  The host (ym_abi_posegraph.hpp) owns the accept rule.
//
// Node i: pose (x, y, theta).  Edge a -> b with mean z and information L (3 x 3, symmetric):
//     e_xy = R(theta_a)^T (t_b - t_a) - z_xy,   e_theta = wrap(theta_b - theta_a - z_theta) into (-pi, pi],   chi2 = sum e^T L e
//     J_a = [[-c, -s, -s dx + c dy], [s, -c, -c dx - s dy], [0, 0, -1]],   J_b = [[c, s, 0], [-s, c, 0], [0, 0, 1]]
// (c, s = cos, sin theta_a; d = t_b - t_a).  Every node is held or free; node 0 is always held.  A step solves
// (H + lambda diag(H)) delta = -g over the free nodes: H, g and diag(H) are summed over all edges, so an edge between a free
// and a held node gives the free node its diagonal block and gradient and nothing else, and an edge between two held nodes
// only its chi2 term.  delta of a held node is exactly 0, and its trial pose is a copy of its pose (no wrap).
// Solve order: slot 0 stands for all held nodes (identity row, right-hand side zero), the F free nodes take the slots 1 .. F
// in index order (slot[N], 0 for a held node; node_of_slot[F + 1], entry 0 is node 0).  With only node 0 held slot(i) = i.
// The band rows, the factor and the CG vectors are laid out by slot: [F + 1] rows, not [N].
//
// pg_linearise_kernel  one lane per edge: e, the edge's cost term rho(e^T L e), and w times each of J_a^T L J_a, J_a^T L J_b,
//                      J_b^T L J_b, J_a^T L e, J_b^T L e
// pg_assemble_kernel   one lane per node: walks the node's incident edges (a CSR the host builds, in edge order) and sums the
//                      diagonal block and the gradient (of every node, held ones too); the blocks between two free nodes
//                      with 0 < slot(j) - slot(i) <= W go into the row of slot(i) of the band A[F+1][W+1] (block k of row s =
//                      A(s, s + k)); a held node writes no row, node 0 writes slot 0's, so no two lanes write one address.
//                      Blocks further from the diagonal stay with their edges: the mat-vec reads every off-diagonal block
//                      from its edge.
// pg_solve_kernel      ONE workgroup.  Wave 0 factors band(A, W) = U^T U, a sweep over the F + 1 block rows with the rows
//                      j .. j + W in an LDS window of (W+1)^2 blocks whose trailing update the lanes share; U is written row by
//                      row and column by column, so both substitutions read one contiguous row a step and keep their W + 1
//                      pending block rows in registers, one scalar a lane (the solved row's three are read with readlane; the
//                      loads of the next rows are in flight several steps ahead).  The whole workgroup then runs
//                      conjugate gradients preconditioned by that factor to the tolerance or the cap: mat-vec by slot over the
//                      free node's incidence list (neighbours of slot 0 skipped), axpys, and dot products reduced in a fixed
//                      shape (a strided partial a thread, a shuffle tree a wave, the waves' sums in order).  W = 0
//                      (block-Jacobi) factors and applies by slot, all threads.
// pg_update_kernel     trial = pose + delta(slot), theta wrapped; a held node's trial is its pose, bit for bit
// pg_chi2_kernel, pg_sum_kernel   the cost at the trial poses: a partial a block, then one block over the partials
// pg_edge_terms_kernel one lane per edge: s = e^T L e and the weight w at the current poses
// Robust kernels: every edge has a kind, a parameter p > 0 and an enabled flag.  With s = e^T L e the
// edge's cost term is rho(s) and its blocks and gradient terms are scaled by w = rho'(s), taken at the poses of the
// linearisation; a disabled edge has rho = w = 0.  The default kind has rho = s and w = 1.0: a product with 1.0 is exact, so a
// graph without robust or disabled edges gets the bits it got before there were kinds.
// No floating-point atomics; every sum has a fixed order, so results are bit-identical from run to run.  Every loop is bounded
// by N, the degree of a node or the iteration cap.  Plain C++ and vector memory operations only.
// Part of ym_kernels.hpp (include that, not this file).
#pragma once

namespace ym {

constexpr int kPgMaxBand = 16;        // the widest band: the LDS window is (kPgMaxBand + 1)^2 blocks
constexpr int kPgSolveThreads = 512;  // the solve workgroup
constexpr double kPgPi = 3.14159265358979323846;
enum { kPgRecCg = 0, kPgRecResidual = 1, kPgRecFlags = 2, kPgRecChi2 = 3, kPgRecWords = 4 };
enum { kPgFlagConverged = 1, kPgFlagPivot = 2, kPgFlagBreakdown = 4 };
enum { kPgRobustNone = 0, kPgRobustHuber = 1, kPgRobustCauchy = 2, kPgRobustGemanMcClure = 3, kPgRobustKinds = 4 };
enum { kPgSumCost = 0, kPgSumTrial = 1, kPgSumPlain = 2 }; // what pg_chi2_kernel sums

struct PgArgs {
    int32_t n_nodes, n_edges, band;
    int32_t n_slots;             // F + 1: slot 0 (the held nodes) and one slot a free node
    const int32_t *slot;         // [N]: 0 for a held node, else 1 .. F in index order
    const int32_t *node_of_slot; // [F + 1]: the node of a slot (entry 0: node 0)
    const double *pose;      // [N][3]
    double *trial;           // [N][3]
    const int32_t *from_to;  // [M][2]
    const double *mean;      // [M][3]
    const double *info;      // [M][9]
    const uint8_t *kind;     // [M]: kPgRobust...
    const uint8_t *enabled;  // [M]: 0 for a disabled edge
    const double *param;     // [M]: the kind's parameter (k or c), > 0
    const int32_t *node_ptr; // [N + 1]
    const int32_t *inc;      // [2 M]: edge << 1 | (0: the node is the edge's a, 1: its b), by node, in edge order
    double *e_blk;           // [M][27]: J_a^T L J_a, J_a^T L J_b, J_b^T L J_b
    double *e_grad;          // [M][6]
    double *e_chi;           // [M]: rho of the edge at the poses of the linearisation
    double *e_s, *e_w;       // [M] each: pg_edge_terms_kernel's s and w
    double *diag;            // [N][9] as assembled (no damping, node 0 included)
    double *grad;            // [N][3] as assembled
    double *aband;           // [F+1][W+1][9]: the damped system in solve order; block 0 is the diagonal block
    double *uband, *ubandT;  // the factor by rows: U(j, j+k) at [j][k]; by columns: U(j-k, j) at [j][k]
    double *vec;             // x, r, z, p, q: [5][3 (F+1)], in solve order
    double *partial;         // [ceil(M / 256)]
    double *record;          // [kPgRecWords]
    double lambda, cg_tol;
    int32_t cg_cap;
};

__device__ inline double pg_wrap(double t) { return t - (2.0 * kPgPi) * ceil((t - kPgPi) / (2.0 * kPgPi)); }

// e and J_a, J_b of one edge at the poses `pose`
__device__ inline void pg_residual(const PgArgs &a, const double *pose, int e, double r[3], double &c, double &s, double &dx, double &dy) {
    const int na = a.from_to[2 * e], nb = a.from_to[2 * e + 1];
    const double *pa = pose + 3 * (size_t)na, *pb = pose + 3 * (size_t)nb, *z = a.mean + 3 * (size_t)e;
    dx = pb[0] - pa[0];
    dy = pb[1] - pa[1];
    c = cos(pa[2]);
    s = sin(pa[2]);
    r[0] = c * dx + s * dy - z[0];
    r[1] = -s * dx + c * dy - z[1];
    r[2] = pg_wrap(pb[2] - pa[2] - z[2]);
}

__device__ inline double pg_quad(const double *L, const double r[3]) {
    const double l0 = L[0] * r[0] + L[1] * r[1] + L[2] * r[2];
    const double l1 = L[3] * r[0] + L[4] * r[1] + L[5] * r[2];
    const double l2 = L[6] * r[0] + L[7] * r[1] + L[8] * r[2];
    return r[0] * l0 + r[1] * l1 + r[2] * l2;
}

// rho(s) of an enabled edge of kind `kind` with parameter p
__device__ inline double pg_rho(int kind, double p, double s) {
    const double p2 = p * p;
    switch (kind) {
    case kPgRobustHuber: return s <= p2 ? s : 2.0 * p * sqrt(s) - p2;
    case kPgRobustCauchy: return p2 * log1p(s / p2);
    case kPgRobustGemanMcClure: return p2 * s / (p2 + s);
    default: return s;
    }
}

// w(s) = rho'(s)
__device__ inline double pg_weight(int kind, double p, double s) {
    const double p2 = p * p;
    switch (kind) {
    case kPgRobustHuber: return s <= p2 ? 1.0 : p / sqrt(s);
    case kPgRobustCauchy: return 1.0 / (1.0 + s / p2);
    case kPgRobustGemanMcClure: { const double q = p2 / (p2 + s); return q * q; }
    default: return 1.0;
    }
}

// the cost term and the weight of edge e, whose e^T L e is s
__device__ inline double pg_edge_rho(const PgArgs &a, int e, double s) { return a.enabled[e] ? pg_rho(a.kind[e], a.param[e], s) : 0.0; }
__device__ inline double pg_edge_weight(const PgArgs &a, int e, double s) { return a.enabled[e] ? pg_weight(a.kind[e], a.param[e], s) : 0.0; }

// out = w X^T Y (3 x 3, row-major)
__device__ inline void pg_atb(const double X[9], const double Y[9], double w, double *out) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) out[r * 3 + c] = w * (X[r] * Y[c] + X[3 + r] * Y[3 + c] + X[6 + r] * Y[6 + c]);
}

// grid: ceil(M / 256), 256 threads
__global__ __launch_bounds__(256) void pg_linearise_kernel(PgArgs a) {
    const int e = (int)(blockIdx.x * 256u + threadIdx.x);
    if (e >= a.n_edges) return;
    double r[3], c, s, dx, dy;
    pg_residual(a, a.pose, e, r, c, s, dx, dy);
    const double *L = a.info + 9 * (size_t)e;
    const double Ja[9] = {-c, -s, -s * dx + c * dy, s, -c, -c * dx - s * dy, 0.0, 0.0, -1.0};
    const double Jb[9] = {c, s, 0.0, -s, c, 0.0, 0.0, 0.0, 1.0};
    double LJa[9], LJb[9], Le[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            LJa[i * 3 + j] = L[i * 3] * Ja[j] + L[i * 3 + 1] * Ja[3 + j] + L[i * 3 + 2] * Ja[6 + j];
            LJb[i * 3 + j] = L[i * 3] * Jb[j] + L[i * 3 + 1] * Jb[3 + j] + L[i * 3 + 2] * Jb[6 + j];
        }
        Le[i] = L[i * 3] * r[0] + L[i * 3 + 1] * r[1] + L[i * 3 + 2] * r[2];
    }
    const double sq = r[0] * Le[0] + r[1] * Le[1] + r[2] * Le[2];
    const double w = pg_edge_weight(a, e, sq);
    double *blk = a.e_blk + 27 * (size_t)e;
    pg_atb(Ja, LJa, w, blk);
    pg_atb(Ja, LJb, w, blk + 9);
    pg_atb(Jb, LJb, w, blk + 18);
    double *g = a.e_grad + 6 * (size_t)e;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        g[i] = w * (Ja[i] * Le[0] + Ja[3 + i] * Le[1] + Ja[6 + i] * Le[2]);
        g[3 + i] = w * (Jb[i] * Le[0] + Jb[3 + i] * Le[1] + Jb[6 + i] * Le[2]);
    }
    a.e_chi[e] = pg_edge_rho(a, e, sq);
}

// grid: ceil(M / 256), 256 threads: e_s = e^T L e of every edge (a disabled one too), e_w = its weight, at a.pose
__global__ __launch_bounds__(256) void pg_edge_terms_kernel(PgArgs a) {
    const int e = (int)(blockIdx.x * 256u + threadIdx.x);
    if (e >= a.n_edges) return;
    double r[3], c, s, dx, dy;
    pg_residual(a, a.pose, e, r, c, s, dx, dy);
    const double sq = pg_quad(a.info + 9 * (size_t)e, r);
    a.e_s[e] = sq;
    a.e_w[e] = pg_edge_weight(a, e, sq);
}

// grid: ceil(N / 256), 256 threads
__global__ __launch_bounds__(256) void pg_assemble_kernel(PgArgs a) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= a.n_nodes) return;
    const int W = a.band, rowlen = (W + 1) * 9, si = a.slot[i];
    const bool rowed = si != 0 || i == 0; // (a held node but node 0 has no row of its own)
    double *row = a.aband + (size_t)si * rowlen;
    if (rowed)
        for (int k = 9; k < rowlen; k++) row[k] = 0.0;
    double d[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
    for (int q = a.node_ptr[i]; q < a.node_ptr[i + 1]; q++) {
        const int v = a.inc[q], e = v >> 1, side = v & 1;
        const double *blk = a.e_blk + 27 * (size_t)e;
        const double *own = blk + (side ? 18 : 0), *ge = a.e_grad + 6 * (size_t)e + 3 * side;
#pragma unroll
        for (int t = 0; t < 9; t++) d[t] += own[t];
#pragma unroll
        for (int t = 0; t < 3; t++) g[t] += ge[t];
        const int other = a.from_to[2 * e + 1 - side];
        const int so = a.slot[other], k = so - si;
        if (si != 0 && so != 0 && k > 0 && k <= W) {
            double *dst = row + 9 * k;
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) dst[r * 3 + c] += side ? blk[9 + c * 3 + r] : blk[9 + r * 3 + c];
        }
    }
#pragma unroll
    for (int t = 0; t < 9; t++) a.diag[9 * (size_t)i + t] = d[t];
#pragma unroll
    for (int t = 0; t < 3; t++) a.grad[3 * (size_t)i + t] = g[t];
    if (!rowed) return;
    if (i == 0) {
#pragma unroll
        for (int t = 0; t < 9; t++) row[t] = (t == 0 || t == 4 || t == 8) ? 1.0 : 0.0;
    } else {
#pragma unroll
        for (int t = 0; t < 9; t++) row[t] = (t == 0 || t == 4 || t == 8) ? d[t] + a.lambda * d[t] : d[t];
    }
}

// ---- the solve
struct PgTri { double i00, u01, u02, i11, u12, i22; }; // U of A = U^T U, the diagonal as reciprocals (no division in a substitution)

// A = U^T U of a symmetric 3 x 3 block (upper entries given); *bad is set on a pivot that is not positive
__device__ inline PgTri pg_chol3(double a00, double a01, double a02, double a11, double a12, double a22, bool *bad) {
    PgTri t;
    if (!(a00 > 0.0)) { *bad = true; a00 = 1.0; }
    t.i00 = 1.0 / sqrt(a00);
    t.u01 = a01 * t.i00;
    t.u02 = a02 * t.i00;
    double d = a11 - t.u01 * t.u01;
    if (!(d > 0.0)) { *bad = true; d = 1.0; }
    t.i11 = 1.0 / sqrt(d);
    t.u12 = (a12 - t.u01 * t.u02) * t.i11;
    d = a22 - t.u02 * t.u02 - t.u12 * t.u12;
    if (!(d > 0.0)) { *bad = true; d = 1.0; }
    t.i22 = 1.0 / sqrt(d);
    return t;
}
// U^T y = r
__device__ inline void pg_lower3(const PgTri &t, double r0, double r1, double r2, double &y0, double &y1, double &y2) {
    y0 = r0 * t.i00;
    y1 = (r1 - t.u01 * y0) * t.i11;
    y2 = (r2 - t.u02 * y0 - t.u12 * y1) * t.i22;
}
// U x = y
__device__ inline void pg_upper3(const PgTri &t, double y0, double y1, double y2, double &x0, double &x1, double &x2) {
    x2 = y2 * t.i22;
    x1 = (y1 - t.u12 * x2) * t.i11;
    x0 = (y0 - t.u01 * x1 - t.u02 * x2) * t.i00;
}

// v of lane `lane` (the same in every lane of the wave), in every lane
__device__ inline double pg_readlane(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// the lanes of one wave exchange data through LDS or global memory: what was written before is visible after
__device__ inline void pg_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the sum of v over the workgroup, the same value in every thread: a shuffle tree a wave, then the waves' sums in order
__device__ inline double pg_block_sum(double v, double *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kPgSolveThreads / 64; w++) s += sh[w];
    __syncthreads();
    return s;
}

// wave 0: band(A, W) = U^T U with the rows j .. j + W in the LDS window `win`; returns whether a pivot was not positive
__device__ inline bool pg_factor_band(const PgArgs &a, double *win, unsigned char *pk1, unsigned char *pk2) {
    const int N = a.n_slots, W = a.band, W1 = W + 1, rowlen = W1 * 9, lane = (int)threadIdx.x;
    const int npairs = W * (W + 1) / 2;
    if (lane == 0) {
        int t = 0;
        for (int k1 = 1; k1 <= W; k1++)
            for (int k2 = k1; k2 <= W; k2++, t++) { pk1[t] = (unsigned char)k1; pk2[t] = (unsigned char)k2; }
    }
    for (int idx = lane; idx < W1 * rowlen; idx += 64) win[idx] = idx / rowlen < N ? a.aband[idx] : 0.0;
    pg_wave_sync();
    bool bad = false;
    for (int j = 0; j < N; j++) {
        double *R = win + (j % W1) * rowlen;
        // the row that enters the window when row j leaves it (at most 153 values: three a lane)
        const bool more = j + W1 < N;
        const double *nrow = a.aband + (size_t)(more ? j + W1 : j) * rowlen;
        const double n0 = lane < rowlen ? nrow[lane] : 0.0;
        const double n1 = lane + 64 < rowlen ? nrow[lane + 64] : 0.0;
        const double n2 = lane + 128 < rowlen ? nrow[lane + 128] : 0.0;
        const PgTri t = pg_chol3(R[0], R[1], R[2], R[4], R[5], R[8], &bad);
        if (lane < 3 * W) { // U(j, j+k) = U_jj^-T A(j, j+k), a column a lane
            const int k = 1 + lane / 3, c = lane % 3;
            double *B = R + 9 * k + c;
            double v0, v1, v2;
            pg_lower3(t, B[0], B[3], B[6], v0, v1, v2);
            B[0] = v0; B[3] = v1; B[6] = v2;
        } else if (lane < 3 * W + 9) {
            const int e = lane - 3 * W;
            R[e] = e == 0 ? t.i00 : e == 1 ? t.u01 : e == 2 ? t.u02 : e == 4 ? t.i11 : e == 5 ? t.u12 : e == 8 ? t.i22 : 0.0;
        }
        pg_wave_sync();
        for (int idx = lane; idx < rowlen; idx += 64) {
            const double v = R[idx];
            const int k = idx / 9;
            a.uband[(size_t)j * rowlen + idx] = v;
            if (j + k < N) a.ubandT[(size_t)(j + k) * rowlen + idx] = v;
        }
        // A(j+k1, j+k2) -= U(j, j+k1)^T U(j, j+k2), 1 <= k1 <= k2 <= W
        for (int q = lane; q < npairs * 9; q += 64) {
            const int pr = q / 9, e = q - 9 * pr, r = e / 3, c = e - 3 * r;
            const int k1 = pk1[pr], k2 = pk2[pr];
            const double *X = R + 9 * k1 + r, *Y = R + 9 * k2 + c;
            win[((j + k1) % W1) * rowlen + 9 * (k2 - k1) + e] -= X[0] * Y[0] + X[3] * Y[3] + X[6] * Y[6];
        }
        pg_wave_sync();
        if (more) {
            if (lane < rowlen) R[lane] = n0;
            if (lane + 64 < rowlen) R[lane + 64] = n1;
            if (lane + 128 < rowlen) R[lane + 128] = n2;
        }
        pg_wave_sync();
    }
    return bad;
}

struct PgRow { PgTri t; double m0, m1, m2, nxt; };
constexpr int kPgPrefetch = 6; // rows whose loads are in flight ahead of a substitution's step

// Step s of a substitution handles block row j = s (forward) or N - 1 - s (backward).  Lane 3 * slot + c holds component c of
// the pending right-hand side of the step s' in [s, s + W] with s' % (W + 1) == slot, k = s' - s steps ahead.  What the lane
// reads for step s: the diagonal block, its three factors of block k, or -- for the slot whose row is solved in this step --
// the scalar of step s + W + 1, which takes the slot over
template <bool FWD>
__device__ inline PgRow pg_row_load(const PgArgs &a, const double *src, int s, int slot, int c) {
    const int N = a.n_slots, W = a.band, W1 = W + 1, rowlen = W1 * 9, j = FWD ? s : N - 1 - s;
    const double *U = (FWD ? a.uband : a.ubandT) + (size_t)j * rowlen;
    PgRow r;
    r.t.i00 = U[0]; r.t.u01 = U[1]; r.t.u02 = U[2]; r.t.i11 = U[4]; r.t.u12 = U[5]; r.t.i22 = U[8];
    r.m0 = r.m1 = r.m2 = r.nxt = 0.0;
    int k = slot - s % W1;
    if (k < 0) k += W1;
    if (slot <= W) {
        if (k >= 1) { // forward: column c of U(j, j+k) (applied transposed); backward: row c of U(j-k, j)
            const double *B = U + 9 * k;
            r.m0 = FWD ? B[c] : B[3 * c];
            r.m1 = FWD ? B[3 + c] : B[3 * c + 1];
            r.m2 = FWD ? B[6 + c] : B[3 * c + 2];
        } else if (s + W1 < N) {
            r.nxt = src[3 * (size_t)(FWD ? s + W1 : N - 1 - s - W1) + c];
        }
    }
    return r;
}

// wave 0: FWD: U^T y = src, else U x = src, one block row a step (dst may be src)
template <bool FWD>
__device__ inline void pg_sweep(const PgArgs &a, const double *src, double *dst) {
    const int N = a.n_slots, W = a.band, W1 = W + 1, lane = (int)threadIdx.x, slot = lane / 3, c = lane - 3 * slot;
    double p = (slot <= W && slot < N) ? src[3 * (size_t)(FWD ? slot : N - 1 - slot) + c] : 0.0;
    PgRow q[kPgPrefetch];
#pragma unroll
    for (int d = 0; d < kPgPrefetch; d++) q[d] = pg_row_load<FWD>(a, src, d < N ? d : N - 1, slot, c);
    for (int s0 = 0; s0 < N; s0 += kPgPrefetch) {
#pragma unroll
        for (int d = 0; d < kPgPrefetch; d++) {
            const int s = s0 + d;
            if (s < N) {
                const PgRow cur = q[d];
                if (s + kPgPrefetch < N) q[d] = pg_row_load<FWD>(a, src, s + kPgPrefetch, slot, c);
                const int cs = s % W1, j = FWD ? s : N - 1 - s;
                const double r0 = pg_readlane(p, 3 * cs), r1 = pg_readlane(p, 3 * cs + 1), r2 = pg_readlane(p, 3 * cs + 2);
                double y0, y1, y2;
                if (FWD) pg_lower3(cur.t, r0, r1, r2, y0, y1, y2);
                else pg_upper3(cur.t, r0, r1, r2, y0, y1, y2);
                if (lane < 3) dst[3 * (size_t)j + lane] = lane == 0 ? y0 : lane == 1 ? y1 : y2;
                p = slot == cs ? cur.nxt : p - (cur.m0 * y0 + cur.m1 * y1 + cur.m2 * y2);
            }
        }
    }
}

// z = band(A, W)^-1 r, by the whole workgroup (ends with a barrier)
__device__ inline void pg_precondition(const PgArgs &a, const double *r, double *z) {
    const int N = a.n_slots;
    if (a.band == 0) {
        for (int i = (int)threadIdx.x; i < N; i += kPgSolveThreads) {
            const double *U = a.uband + 9 * (size_t)i;
            const PgTri t = {U[0], U[1], U[2], U[4], U[5], U[8]};
            double y0, y1, y2, x0, x1, x2;
            pg_lower3(t, r[3 * (size_t)i], r[3 * (size_t)i + 1], r[3 * (size_t)i + 2], y0, y1, y2);
            pg_upper3(t, y0, y1, y2, x0, x1, x2);
            z[3 * (size_t)i] = x0; z[3 * (size_t)i + 1] = x1; z[3 * (size_t)i + 2] = x2;
        }
    } else if (threadIdx.x < 64) {
        pg_sweep<true>(a, r, z);
        pg_wave_sync();
        pg_sweep<false>(a, z, z);
    }
    __syncthreads();
}

// rows of slot sl of q = A p (the damped system in solve order): the diagonal block, then the off-diagonal block of every edge
// from the slot's node to another free node
__device__ inline void pg_matvec_slot(const PgArgs &a, const double *p, int sl, double &q0, double &q1, double &q2) {
    const double *D = a.aband + (size_t)sl * (a.band + 1) * 9, *pi = p + 3 * (size_t)sl;
    q0 = D[0] * pi[0] + D[1] * pi[1] + D[2] * pi[2];
    q1 = D[3] * pi[0] + D[4] * pi[1] + D[5] * pi[2];
    q2 = D[6] * pi[0] + D[7] * pi[1] + D[8] * pi[2];
    if (sl == 0) return;
    const int i = a.node_of_slot[sl];
    for (int q = a.node_ptr[i]; q < a.node_ptr[i + 1]; q++) {
        const int v = a.inc[q], e = v >> 1, side = v & 1;
        const int so = a.slot[a.from_to[2 * e + 1 - side]];
        if (so == 0) continue;
        const double *B = a.e_blk + 27 * (size_t)e + 9, *po = p + 3 * (size_t)so;
        if (side == 0) {
            q0 += B[0] * po[0] + B[1] * po[1] + B[2] * po[2];
            q1 += B[3] * po[0] + B[4] * po[1] + B[5] * po[2];
            q2 += B[6] * po[0] + B[7] * po[1] + B[8] * po[2];
        } else {
            q0 += B[0] * po[0] + B[3] * po[1] + B[6] * po[2];
            q1 += B[1] * po[0] + B[4] * po[1] + B[7] * po[2];
            q2 += B[2] * po[0] + B[5] * po[1] + B[8] * po[2];
        }
    }
}

// grid: 1, kPgSolveThreads threads.  vec[0 .. 3 (F+1)) = delta by slot on return; record[kPgRecCg, kPgRecResidual, kPgRecFlags]
__global__ __launch_bounds__(kPgSolveThreads) void pg_solve_kernel(PgArgs a) {
    __shared__ double win[(kPgMaxBand + 1) * (kPgMaxBand + 1) * 9];
    __shared__ double red[kPgSolveThreads / 64];
    __shared__ unsigned char pk1[kPgMaxBand * (kPgMaxBand + 1) / 2], pk2[kPgMaxBand * (kPgMaxBand + 1) / 2];
    __shared__ int sh_bad;
    const int N = a.n_slots, tid = (int)threadIdx.x; // (every loop below runs over the slots)
    const size_t n3 = 3 * (size_t)N;
    double *x = a.vec, *r = a.vec + n3, *z = a.vec + 2 * n3, *p = a.vec + 3 * n3, *qv = a.vec + 4 * n3;
    if (tid == 0) sh_bad = 0;
    __syncthreads();
    if (a.band == 0) {
        bool bad = false;
        for (int i = tid; i < N; i += kPgSolveThreads) {
            const double *D = a.aband + 9 * (size_t)i;
            const PgTri t = pg_chol3(D[0], D[1], D[2], D[4], D[5], D[8], &bad);
            double *U = a.uband + 9 * (size_t)i;
            U[0] = t.i00; U[1] = t.u01; U[2] = t.u02; U[3] = 0.0; U[4] = t.i11; U[5] = t.u12; U[6] = 0.0; U[7] = 0.0; U[8] = t.i22;
        }
        if (bad) sh_bad = 1;
    } else if (tid < 64) {
        const bool bad = pg_factor_band(a, win, pk1, pk2);
        if (bad && tid == 0) sh_bad = 1;
    }
    // x = 0, r = b = -g of the slot's node, slot 0 zero
    double acc = 0.0;
    for (size_t i = tid; i < n3; i += kPgSolveThreads) {
        const double b = i < 3 ? 0.0 : -a.grad[3 * (size_t)a.node_of_slot[i / 3] + i % 3];
        x[i] = 0.0;
        r[i] = b;
        acc += b * b;
    }
    __syncthreads();
    const double bb = pg_block_sum(acc, red);
    int iters = 0, flags = sh_bad ? kPgFlagPivot : 0;
    double rr = bb;
    if (bb > 0.0) {
        const double stop = a.cg_tol * a.cg_tol * bb;
        pg_precondition(a, r, z);
        acc = 0.0;
        for (size_t i = tid; i < n3; i += kPgSolveThreads) {
            const double zi = z[i];
            p[i] = zi;
            acc += r[i] * zi;
        }
        __syncthreads();
        double rz = pg_block_sum(acc, red);
        for (int it = 0; it < a.cg_cap; it++) {
            acc = 0.0;
            for (int i = tid; i < N; i += kPgSolveThreads) {
                double q0, q1, q2;
                pg_matvec_slot(a, p, i, q0, q1, q2);
                qv[3 * (size_t)i] = q0; qv[3 * (size_t)i + 1] = q1; qv[3 * (size_t)i + 2] = q2;
                acc += p[3 * (size_t)i] * q0 + p[3 * (size_t)i + 1] * q1 + p[3 * (size_t)i + 2] * q2;
            }
            const double pq = pg_block_sum(acc, red);
            if (!(pq > 0.0) || !(rz > 0.0)) { flags |= kPgFlagBreakdown; break; }
            const double alpha = rz / pq;
            acc = 0.0;
            for (size_t i = tid; i < n3; i += kPgSolveThreads) {
                x[i] += alpha * p[i];
                const double ri = r[i] - alpha * qv[i];
                r[i] = ri;
                acc += ri * ri;
            }
            __syncthreads();
            rr = pg_block_sum(acc, red);
            iters++;
            if (rr <= stop) { flags |= kPgFlagConverged; break; }
            pg_precondition(a, r, z);
            acc = 0.0;
            for (size_t i = tid; i < n3; i += kPgSolveThreads) acc += r[i] * z[i];
            const double rz_new = pg_block_sum(acc, red);
            const double beta = rz_new / rz;
            rz = rz_new;
            for (size_t i = tid; i < n3; i += kPgSolveThreads) p[i] = z[i] + beta * p[i];
            __syncthreads();
        }
    } else {
        flags |= kPgFlagConverged;
    }
    if (tid == 0) {
        a.record[kPgRecCg] = (double)iters;
        a.record[kPgRecResidual] = bb > 0.0 ? sqrt(rr / bb) : 0.0;
        a.record[kPgRecFlags] = (double)flags;
    }
}

// grid: ceil(N / 256), 256 threads
__global__ __launch_bounds__(256) void pg_update_kernel(PgArgs a) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= a.n_nodes) return;
    const int sl = a.slot[i];
    const double *p = a.pose + 3 * (size_t)i, *d = a.vec + 3 * (size_t)sl;
    double *t = a.trial + 3 * (size_t)i;
    if (sl == 0) { // held: the pose as it is
        t[0] = p[0]; t[1] = p[1]; t[2] = p[2];
        return;
    }
    t[0] = p[0] + d[0];
    t[1] = p[1] + d[1];
    t[2] = pg_wrap(p[2] + d[2]);
}

__device__ inline double pg_block256_sum(double v, double *sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// grid: ceil(M / 256), 256 threads.  kPgSumTrial: rho at a.trial; kPgSumCost: the terms pg_linearise_kernel left in e_chi;
// kPgSumPlain: the plain chi2, pg_edge_terms_kernel's s of the enabled edges
template <int WHAT>
__global__ __launch_bounds__(256) void pg_chi2_kernel(PgArgs a) {
    __shared__ double sh[4];
    const int e = (int)(blockIdx.x * 256u + threadIdx.x);
    double v = 0.0;
    if (e < a.n_edges) {
        if (WHAT == kPgSumTrial) {
            double r[3], c, s, dx, dy;
            pg_residual(a, a.trial, e, r, c, s, dx, dy);
            v = pg_edge_rho(a, e, pg_quad(a.info + 9 * (size_t)e, r));
        } else if (WHAT == kPgSumPlain) {
            v = a.enabled[e] ? a.e_s[e] : 0.0;
        } else {
            v = a.e_chi[e];
        }
    }
    v = pg_block256_sum(v, sh);
    if (threadIdx.x == 0) a.partial[blockIdx.x] = v;
}

// grid: 1, 256 threads: record[kPgRecChi2] = the partials' sum
__global__ __launch_bounds__(256) void pg_sum_kernel(PgArgs a) {
    __shared__ double sh[4];
    const int nb = (a.n_edges + 255) / 256;
    double v = 0.0;
    for (int i = (int)threadIdx.x; i < nb; i += 256) v += a.partial[i];
    v = pg_block256_sum(v, sh);
    if (threadIdx.x == 0) a.record[kPgRecChi2] = v;
}

}  // namespace ym
