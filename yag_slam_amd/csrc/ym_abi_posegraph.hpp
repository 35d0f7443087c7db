// ym_abi_posegraph.hpp -- C ABI: the pose graph and its optimiser (ym_graph_*; ym_k_posegraph.hpp)
// Part of yagmatch.hip (included inside its extern "C" block); not a header of its own.
// The host keeps every node and constraint (poses are copied back after an optimisation), so the device arrays are plain
// mirrors: whatever changed since the last launch is uploaded whole before the next one.
// Every node is held or free (held[i]; node 0 always held).  The solve order -- slot[N], 0 for a held node and 1 .. F for the
// free ones in index order, and node_of_slot[F + 1] -- is rebuilt on the host whenever the set or the node count changed.
struct ym_graph {
    int device;
    OwnStream stream;
    std::vector<double> pose, mean, info;
    std::vector<int32_t> from_to;
    std::vector<uint8_t> held;                   // [N]: 1 for a held node
    std::vector<uint8_t> kind, enabled;          // [M]: the robust kernel of a constraint (YM_ROBUST_*), 0 for a disabled one
    std::vector<double> param;                   // [M]: the kernel's parameter
    bool robust_stale = true;                    // the device's copy of kind / enabled / param is behind the host's
    std::vector<int32_t> slot, node_of_slot;     // the solve order (valid unless slots_stale)
    bool free_edge = false;                      // some edge has a free end (valid unless slots_stale)
    bool slots_stale = true, slots_unsent = true; // the solve order is behind `held` / the device's copy behind the host's
    bool poses_stale = true, edges_stale = true; // the device mirrors are behind the host's vectors
    int cur = 0;                                 // which of d_pose[2] holds the poses (the other takes the trial step)
    DevBuf<double> d_pose[2], d_mean, d_info, e_blk, e_grad, e_chi, diag, grad, aband, uband, ubandT, vec, partial, record;
    DevBuf<int32_t> d_from_to, node_ptr, inc, d_slot, d_node_of_slot;
    DevBuf<uint8_t> d_kind, d_enabled;
    DevBuf<double> d_param, e_s, e_w;
};
static_assert(YM_ROBUST_NONE == ym::kPgRobustNone && YM_ROBUST_HUBER == ym::kPgRobustHuber && YM_ROBUST_CAUCHY == ym::kPgRobustCauchy &&
              YM_ROBUST_GEMAN_MCCLURE == ym::kPgRobustGemanMcClure, "the kernels read the header's kinds");

ym_graph *ym_graph_create(int device) {
    if (check_device(device) != YM_OK) return nullptr;
    DevGuard guard(device);
    if (guard.status() != YM_OK) return nullptr;
    ym_graph *g = new ym_graph();
    g->device = device;
    if (g->stream.create() != YM_OK) { delete g; return nullptr; } // (the error text is set)
    return g;
}

void ym_graph_destroy(ym_graph *g) {
    if (!g) return;
    DevGuard guard(g->device);
    delete g;
}

static bool graph_finite(const double *v, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(v[i])) return false;
    return true;
}

int ym_graph_add_nodes(ym_graph *g, const double *xyt, int n) {
    if (!g || n < 0 || (n > 0 && !xyt)) return set_err(YM_ERR_INVALID, "bad argument");
    if (!graph_finite(xyt, 3 * (size_t)n)) return set_err(YM_ERR_INVALID, "a pose that is not finite");
    if (g->pose.size() / 3 + (size_t)n > (size_t)(INT32_MAX / 64)) return set_err(YM_ERR_UNSUPPORTED, "too many nodes");
    g->pose.insert(g->pose.end(), xyt, xyt + 3 * (size_t)n);
    g->held.resize(g->pose.size() / 3, 0); // (free when added)
    if (!g->held.empty()) g->held[0] = 1;
    if (n) g->poses_stale = g->edges_stale = g->slots_stale = true; // (the incidence lists are per node)
    return YM_OK;
}

int ym_graph_hold(ym_graph *g, const int32_t *nodes, int n, int hold) {
    if (!g || n < 0 || (n > 0 && !nodes)) return set_err(YM_ERR_INVALID, "bad argument");
    const int64_t N = (int64_t)g->held.size();
    for (int i = 0; i < n; i++) { // (nothing is applied unless every index is good)
        if (nodes[i] < 0 || nodes[i] >= N) return set_err(YM_ERR_INVALID, "hold: node %d out of range (%lld nodes)", nodes[i], (long long)N);
        if (!hold && nodes[i] == 0) return set_err(YM_ERR_INVALID, "hold: node 0 is always held and cannot be released");
    }
    for (int i = 0; i < n; i++) {
        const uint8_t v = hold ? 1 : 0;
        if (g->held[(size_t)nodes[i]] != v) { g->held[(size_t)nodes[i]] = v; g->slots_stale = true; }
    }
    return YM_OK;
}

int ym_graph_held(const ym_graph *g, uint8_t *mask, int n_nodes) {
    if (!g || n_nodes < 0 || (n_nodes > 0 && !mask)) return set_err(YM_ERR_INVALID, "bad argument");
    if ((size_t)n_nodes != g->held.size()) return set_err(YM_ERR_INVALID, "held: a mask of %d, the graph has %lld nodes", n_nodes, (long long)g->held.size());
    std::copy(g->held.begin(), g->held.end(), mask);
    return YM_OK;
}

int ym_graph_add_constraints(ym_graph *g, const int32_t *from_to, const double *mean_xyt, const double *info9, int n) {
    if (!g || n < 0 || (n > 0 && (!from_to || !mean_xyt || !info9))) return set_err(YM_ERR_INVALID, "bad argument");
    const int64_t N = (int64_t)(g->pose.size() / 3);
    if (g->from_to.size() / 2 + (size_t)n > (size_t)(INT32_MAX / 64)) return set_err(YM_ERR_UNSUPPORTED, "too many constraints");
    for (int i = 0; i < n; i++) { // (nothing is added unless every constraint is good)
        const int32_t a = from_to[2 * i], b = from_to[2 * i + 1];
        if (a < 0 || a >= N || b < 0 || b >= N)
            return set_err(YM_ERR_INVALID, "constraint %d: nodes %d -> %d out of range (%lld nodes)", i, a, b, (long long)N);
        if (a == b) return set_err(YM_ERR_INVALID, "constraint %d: from a node to itself (%d)", i, a);
        if (!graph_finite(mean_xyt + 3 * (size_t)i, 3) || !graph_finite(info9 + 9 * (size_t)i, 9))
            return set_err(YM_ERR_INVALID, "constraint %d: a value that is not finite", i);
        const double *L = info9 + 9 * (size_t)i;
        if (!(L[0] > 0.0) || !(L[4] > 0.0) || !(L[8] > 0.0))
            return set_err(YM_ERR_INVALID, "constraint %d: an information matrix without a positive diagonal", i);
    }
    for (int i = 0; i < n; i++) {
        const double *L = info9 + 9 * (size_t)i;
        g->from_to.push_back(from_to[2 * i]);
        g->from_to.push_back(from_to[2 * i + 1]);
        g->mean.insert(g->mean.end(), mean_xyt + 3 * (size_t)i, mean_xyt + 3 * (size_t)i + 3);
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) g->info.push_back((L[3 * r + c] + L[3 * c + r]) / 2.0);
    }
    const size_t M = g->from_to.size() / 2;
    g->kind.resize(M, YM_ROBUST_NONE); // (plain and enabled when added)
    g->enabled.resize(M, 1);
    g->param.resize(M, 1.0);
    if (n) g->edges_stale = g->slots_stale = g->robust_stale = true; // (free_edge is per edge)
    return YM_OK;
}

// the index checks the per-constraint setters share (nothing is applied unless every index is good)
static int graph_edge_indices(const ym_graph *g, const char *what, const int32_t *edges, int n) {
    if (!g || n < 0 || (n > 0 && !edges)) return set_err(YM_ERR_INVALID, "bad argument");
    const int64_t M = (int64_t)g->kind.size();
    for (int i = 0; i < n; i++)
        if (edges[i] < 0 || edges[i] >= M)
            return set_err(YM_ERR_INVALID, "%s: constraint %d out of range (%lld constraints)", what, edges[i], (long long)M);
    return YM_OK;
}

int ym_graph_set_robust(ym_graph *g, const int32_t *edges, int n, int kind, double param) {
    int rc = graph_edge_indices(g, "set_robust", edges, n);
    if (rc != YM_OK) return rc;
    if (kind < YM_ROBUST_NONE || kind > YM_ROBUST_GEMAN_MCCLURE) return set_err(YM_ERR_INVALID, "set_robust: kind %d is not a YM_ROBUST_ value", kind);
    if (!std::isfinite(param) || !(param > 0.0)) return set_err(YM_ERR_INVALID, "set_robust: the parameter must be finite and positive");
    for (int i = 0; i < n; i++) {
        g->kind[(size_t)edges[i]] = (uint8_t)kind;
        g->param[(size_t)edges[i]] = param;
    }
    if (n) g->robust_stale = true;
    return YM_OK;
}

int ym_graph_enable(ym_graph *g, const int32_t *edges, int n, int enable) {
    int rc = graph_edge_indices(g, "enable", edges, n);
    if (rc != YM_OK) return rc;
    const uint8_t v = enable ? 1 : 0;
    std::vector<uint8_t> after(g->enabled);
    for (int i = 0; i < n; i++) after[(size_t)edges[i]] = v;
    if (!enable) { // a free node of a constraint that goes must keep an enabled one: its block would be singular
        std::vector<int32_t> left(g->held.size(), 0);
        for (size_t e = 0; e < after.size(); e++)
            if (after[e]) { left[(size_t)g->from_to[2 * e]]++; left[(size_t)g->from_to[2 * e + 1]]++; }
        for (int i = 0; i < n; i++)
            for (int side = 0; side < 2; side++) {
                const int32_t node = g->from_to[2 * (size_t)edges[i] + side];
                if (!g->held[(size_t)node] && left[(size_t)node] == 0)
                    return set_err(YM_ERR_INVALID, "enable: disabling constraint %d would leave the free node %d without an enabled constraint", edges[i], node);
            }
    }
    if (after != g->enabled) { g->enabled.swap(after); g->robust_stale = true; }
    return YM_OK;
}

int ym_graph_size(const ym_graph *g, int32_t *nodes, int32_t *constraints) {
    if (!g || !nodes || !constraints) return set_err(YM_ERR_INVALID, "null argument");
    *nodes = (int32_t)(g->pose.size() / 3);
    *constraints = (int32_t)(g->from_to.size() / 2);
    return YM_OK;
}

static int graph_range(const ym_graph *g, int first, const double *xyt, int n) {
    if (!g || n < 0 || (n > 0 && !xyt)) return set_err(YM_ERR_INVALID, "bad argument");
    const int64_t N = (int64_t)(g->pose.size() / 3);
    if (first < 0 || (int64_t)first + n > N) return set_err(YM_ERR_INVALID, "nodes %d .. %lld out of range (%lld nodes)", first, (long long)first + n - 1, (long long)N);
    return YM_OK;
}

int ym_graph_set_poses(ym_graph *g, int first, const double *xyt, int n) {
    int rc = graph_range(g, first, xyt, n);
    if (rc != YM_OK) return rc;
    if (!graph_finite(xyt, 3 * (size_t)n)) return set_err(YM_ERR_INVALID, "a pose that is not finite");
    std::copy(xyt, xyt + 3 * (size_t)n, g->pose.begin() + 3 * (size_t)first);
    if (n) g->poses_stale = true;
    return YM_OK;
}

int ym_graph_get_poses(const ym_graph *g, int first, double *xyt, int n) {
    int rc = graph_range(g, first, xyt, n);
    if (rc != YM_OK) return rc;
    std::copy(g->pose.begin() + 3 * (size_t)first, g->pose.begin() + 3 * ((size_t)first + n), xyt);
    return YM_OK;
}

// the solve order of the held set as it stands, on the host (no device)
static void graph_slots(ym_graph *g) {
    if (!g->slots_stale) return;
    const size_t N = g->held.size();
    g->slot.assign(N, 0);
    g->node_of_slot.assign(1, 0);
    for (size_t i = 0; i < N; i++)
        if (!g->held[i]) {
            g->slot[i] = (int32_t)g->node_of_slot.size();
            g->node_of_slot.push_back((int32_t)i);
        }
    g->free_edge = false;
    for (size_t e = 0; e < g->from_to.size() && !g->free_edge; e++) g->free_edge = g->slot[(size_t)g->from_to[e]] != 0;
    g->slots_stale = false;
    g->slots_unsent = true;
}

// the device mirrors, the incidence lists, the solve order and the work arrays of a system of band W; `a` is filled in for
// the launches
static int graph_sync(ym_graph *g, int W, ym::PgArgs *a) {
    const size_t N = g->pose.size() / 3, M = g->from_to.size() / 2, rowlen = 9 * ((size_t)W + 1);
    int rc;
    graph_slots(g);
    const size_t S = g->node_of_slot.size();
    if (g->slots_unsent) {
        if ((rc = g->d_slot.ensure(N)) || (rc = g->d_node_of_slot.ensure(S))) return rc;
        HIP_TRY(hipMemcpy(g->d_slot.p, g->slot.data(), N * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(g->d_node_of_slot.p, g->node_of_slot.data(), S * sizeof(int32_t), hipMemcpyHostToDevice));
        g->slots_unsent = false;
    }
    if ((rc = g->d_pose[0].ensure(3 * N)) || (rc = g->d_pose[1].ensure(3 * N))) return rc;
    if (g->poses_stale) {
        HIP_TRY(hipMemcpy(g->d_pose[g->cur].p, g->pose.data(), 3 * N * sizeof(double), hipMemcpyHostToDevice));
        g->poses_stale = false;
    }
    if (g->edges_stale) {
        if ((rc = g->d_from_to.ensure(2 * M)) || (rc = g->d_mean.ensure(3 * M)) || (rc = g->d_info.ensure(9 * M)) ||
            (rc = g->node_ptr.ensure(N + 1)) || (rc = g->inc.ensure(2 * M)))
            return rc;
        std::vector<int32_t> ptr(N + 1, 0), inc(2 * M);
        for (size_t e = 0; e < 2 * M; e++) ptr[(size_t)g->from_to[e] + 1]++;
        for (size_t i = 0; i < N; i++) ptr[i + 1] += ptr[i];
        std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
        for (size_t e = 0; e < M; e++)
            for (int side = 0; side < 2; side++) inc[(size_t)fill[(size_t)g->from_to[2 * e + side]]++] = (int32_t)(2 * e + side);
        HIP_TRY(hipMemcpy(g->d_from_to.p, g->from_to.data(), 2 * M * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(g->d_mean.p, g->mean.data(), 3 * M * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(g->d_info.p, g->info.data(), 9 * M * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(g->node_ptr.p, ptr.data(), (N + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(g->inc.p, inc.data(), 2 * M * sizeof(int32_t), hipMemcpyHostToDevice));
        g->edges_stale = false;
    }
    if (g->robust_stale) {
        if ((rc = g->d_kind.ensure(M)) || (rc = g->d_enabled.ensure(M)) || (rc = g->d_param.ensure(M))) return rc;
        HIP_TRY(hipMemcpy(g->d_kind.p, g->kind.data(), M * sizeof(uint8_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(g->d_enabled.p, g->enabled.data(), M * sizeof(uint8_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(g->d_param.p, g->param.data(), M * sizeof(double), hipMemcpyHostToDevice));
        g->robust_stale = false;
    }
    if ((rc = g->e_s.ensure(M)) || (rc = g->e_w.ensure(M))) return rc;
    if ((rc = g->e_blk.ensure(27 * M)) || (rc = g->e_grad.ensure(6 * M)) || (rc = g->e_chi.ensure(M)) || (rc = g->diag.ensure(9 * N)) ||
        (rc = g->grad.ensure(3 * N)) || (rc = g->aband.ensure(S * rowlen)) || (rc = g->uband.ensure(S * rowlen)) ||
        (rc = g->ubandT.ensure(S * rowlen)) || (rc = g->vec.ensure(15 * S)) || (rc = g->partial.ensure((M + 255) / 256)) ||
        (rc = g->record.ensure(ym::kPgRecWords)))
        return rc;
    *a = ym::PgArgs{};
    a->n_nodes = (int32_t)N; a->n_edges = (int32_t)M; a->band = W;
    a->n_slots = (int32_t)S; a->slot = g->d_slot.p; a->node_of_slot = g->d_node_of_slot.p;
    a->pose = g->d_pose[g->cur].p; a->trial = g->d_pose[g->cur ^ 1].p;
    a->from_to = g->d_from_to.p; a->mean = g->d_mean.p; a->info = g->d_info.p; a->node_ptr = g->node_ptr.p; a->inc = g->inc.p;
    a->e_blk = g->e_blk.p; a->e_grad = g->e_grad.p; a->e_chi = g->e_chi.p; a->diag = g->diag.p; a->grad = g->grad.p;
    a->aband = g->aband.p; a->uband = g->uband.p; a->ubandT = g->ubandT.p; a->vec = g->vec.p; a->partial = g->partial.p;
    a->record = g->record.p;
    a->kind = g->d_kind.p; a->enabled = g->d_enabled.p; a->param = g->d_param.p; a->e_s = g->e_s.p; a->e_w = g->e_w.p;
    return YM_OK;
}

static unsigned graph_blocks(int n) { return (unsigned)((n + 255) / 256); }

// linearise at a.pose; *chi2 = the sum of the edges' cost terms, F = sum rho (chi2 itself on a graph without robust kernels)
static int graph_linearise(ym_graph *g, const ym::PgArgs &a, double *chi2) {
    hipLaunchKernelGGL(ym::pg_linearise_kernel, dim3(graph_blocks(a.n_edges)), dim3(256), 0, g->stream, a);
    hipLaunchKernelGGL(ym::pg_chi2_kernel<ym::kPgSumCost>, dim3(graph_blocks(a.n_edges)), dim3(256), 0, g->stream, a);
    hipLaunchKernelGGL(ym::pg_sum_kernel, dim3(1), dim3(256), 0, g->stream, a);
    HIP_TRY(hipGetLastError());
    double rec[ym::kPgRecWords];
    HIP_TRY(hipMemcpyAsync(rec, a.record, sizeof rec, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    *chi2 = rec[ym::kPgRecChi2];
    return YM_OK;
}

// s and w of every constraint at a.pose, left in a.e_s and a.e_w (enqueued, not waited for)
static void graph_edge_terms(ym_graph *g, const ym::PgArgs &a) {
    hipLaunchKernelGGL(ym::pg_edge_terms_kernel, dim3(graph_blocks(a.n_edges)), dim3(256), 0, g->stream, a);
}

int ym_graph_chi2(ym_graph *g, double *chi2) {
    if (!g || !chi2) return set_err(YM_ERR_INVALID, "null argument");
    if (g->from_to.empty()) { *chi2 = 0.0; return YM_OK; }
    DEV_GUARD(g->device);
    ym::PgArgs a;
    int rc = graph_sync(g, 0, &a);
    if (rc != YM_OK) return rc;
    graph_edge_terms(g, a);
    hipLaunchKernelGGL(ym::pg_chi2_kernel<ym::kPgSumPlain>, dim3(graph_blocks(a.n_edges)), dim3(256), 0, g->stream, a);
    hipLaunchKernelGGL(ym::pg_sum_kernel, dim3(1), dim3(256), 0, g->stream, a);
    HIP_TRY(hipGetLastError());
    double rec[ym::kPgRecWords];
    HIP_TRY(hipMemcpyAsync(rec, a.record, sizeof rec, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    *chi2 = rec[ym::kPgRecChi2];
    return YM_OK;
}

int ym_graph_cost(ym_graph *g, double *cost) {
    if (!g || !cost) return set_err(YM_ERR_INVALID, "null argument");
    if (g->from_to.empty()) { *cost = 0.0; return YM_OK; }
    DEV_GUARD(g->device);
    ym::PgArgs a;
    int rc = graph_sync(g, 0, &a);
    if (rc != YM_OK) return rc;
    return graph_linearise(g, a, cost);
}

int ym_graph_edge_terms(ym_graph *g, double *s, double *w) {
    if (!g || !s || !w) return set_err(YM_ERR_INVALID, "null argument");
    const size_t M = g->from_to.size() / 2;
    if (M == 0) return YM_OK;
    DEV_GUARD(g->device);
    ym::PgArgs a;
    int rc = graph_sync(g, 0, &a);
    if (rc != YM_OK) return rc;
    graph_edge_terms(g, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(s, a.e_s, M * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(w, a.e_w, M * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return YM_OK;
}

int ym_graph_linearise(ym_graph *g, double *chi2, double *diag9, double *grad3) {
    if (!g || !chi2 || !diag9 || !grad3) return set_err(YM_ERR_INVALID, "null argument");
    const size_t N = g->pose.size() / 3;
    if (g->from_to.empty()) {
        *chi2 = 0.0;
        std::fill(diag9, diag9 + 9 * N, 0.0);
        std::fill(grad3, grad3 + 3 * N, 0.0);
        return YM_OK;
    }
    DEV_GUARD(g->device);
    ym::PgArgs a;
    int rc = graph_sync(g, 0, &a);
    if (rc != YM_OK) return rc;
    a.lambda = 0.0;
    double c2 = 0.0;
    if ((rc = graph_linearise(g, a, &c2)) != YM_OK) return rc;
    hipLaunchKernelGGL(ym::pg_assemble_kernel, dim3(graph_blocks(a.n_nodes)), dim3(256), 0, g->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(g->stream));
    HIP_TRY(hipMemcpy(diag9, a.diag, 9 * N * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(grad3, a.grad, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    *chi2 = c2;
    return YM_OK;
}

// the argument checks a solve shares (iters: of the Levenberg-Marquardt loop; cg: whether the tolerance and the cap count, the
// cap at least min_cg) and the band it runs with
static int graph_solve_args(ym_graph *g, int iters, double lambda, int band, bool cg, int max_cg_iters, int min_cg, double cg_tol, int *W_out) {
    if (iters < 0 || !(lambda > 0.0) || !std::isfinite(lambda)) return set_err(YM_ERR_INVALID, "iters >= 0 and lambda0 > 0 are required");
    if (band < -1 || band > ym::kPgMaxBand) return set_err(YM_ERR_INVALID, "band %d: -1 (automatic) or 0 .. %d", band, ym::kPgMaxBand);
    if (cg && (max_cg_iters < min_cg || !(cg_tol > 0.0) || !std::isfinite(cg_tol)))
        return set_err(YM_ERR_INVALID, "max_cg_iters >= %d and cg_tol > 0 are required", min_cg);
    int W = band;
    if (W < 0) { // the largest |slot(a) - slot(b)| <= kPgMaxBand among the edges whose ends are free or node 0.  (An edge at
        // node 0 has no block in the band; it counts because it always did: with nothing else held this is the largest |a - b|.)
        W = 0;
        graph_slots(g);
        for (size_t e = 0; e < g->from_to.size() / 2; e++) {
            const int32_t na = g->from_to[2 * e], nb = g->from_to[2 * e + 1];
            const int sa = g->slot[(size_t)na], sb = g->slot[(size_t)nb], d = std::abs(sa - sb);
            if ((sa != 0 || na == 0) && (sb != 0 || nb == 0) && d <= ym::kPgMaxBand && d > W) W = d;
        }
    }
    *W_out = W;
    return YM_OK;
}

int ym_graph_solve(ym_graph *g, int band, double lambda, double cg_tol, int max_cg_iters, double *delta3, double *precond3,
                   int32_t *band_used, int32_t *cg_iterations, double *residual, int32_t *flags) {
    if (!g || !delta3 || !band_used || !cg_iterations || !residual || !flags) return set_err(YM_ERR_INVALID, "null argument");
    int W = 0;
    int rc = graph_solve_args(g, 0, lambda, band, true, max_cg_iters, 0, cg_tol, &W);
    if (rc != YM_OK) return rc;
    const size_t N = g->pose.size() / 3, M = g->from_to.size() / 2;
    *band_used = W;
    *cg_iterations = 0;
    *residual = 0.0;
    *flags = 0;
    std::fill(delta3, delta3 + 3 * N, 0.0);
    if (precond3) std::fill(precond3, precond3 + 3 * N, 0.0);
    graph_slots(g);
    if (N < 2 || M == 0 || !g->free_edge) return YM_OK; // (no free node has no edge with a free end either)
    DEV_GUARD(g->device);
    ym::PgArgs a;
    if ((rc = graph_sync(g, W, &a)) != YM_OK) return rc;
    const size_t S = (size_t)a.n_slots;
    a.lambda = lambda;
    a.cg_tol = cg_tol;
    a.cg_cap = max_cg_iters;
    double chi2 = 0.0;
    if ((rc = graph_linearise(g, a, &chi2)) != YM_OK) return rc;
    HIP_TRY(hipMemsetAsync(a.vec, 0, 15 * S * sizeof(double), g->stream)); // (a right-hand side of zero leaves z unwritten)
    hipLaunchKernelGGL(ym::pg_assemble_kernel, dim3(graph_blocks(a.n_nodes)), dim3(256), 0, g->stream, a);
    hipLaunchKernelGGL(ym::pg_solve_kernel, dim3(1), dim3(ym::kPgSolveThreads), 0, g->stream, a);
    HIP_TRY(hipGetLastError());
    double rec[ym::kPgRecWords];
    HIP_TRY(hipMemcpyAsync(rec, a.record, sizeof rec, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    // x and z come back in solve order; the rows of the held nodes stay zero
    std::vector<double> by_slot(9 * S);
    HIP_TRY(hipMemcpy(by_slot.data(), a.vec, 9 * S * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t sl = 1; sl < S; sl++) {
        const size_t i = (size_t)g->node_of_slot[sl];
        std::copy(by_slot.begin() + 3 * sl, by_slot.begin() + 3 * sl + 3, delta3 + 3 * i);
        if (precond3) std::copy(by_slot.begin() + 6 * S + 3 * sl, by_slot.begin() + 6 * S + 3 * sl + 3, precond3 + 3 * i);
    }
    *cg_iterations = (int32_t)rec[ym::kPgRecCg];
    *residual = rec[ym::kPgRecResidual];
    *flags = (int32_t)rec[ym::kPgRecFlags];
    return YM_OK;
}

int ym_graph_optimize(ym_graph *g, const ym_opt_params *p, ym_opt_report *out) {
    if (!g || !p || !out) return set_err(YM_ERR_INVALID, "null argument");
    int W = 0;
    int rc = graph_solve_args(g, p->iters, p->lambda0, p->band, !p->exact, p->max_cg_iters, 1, p->cg_tol, &W);
    if (rc != YM_OK) return rc;
    const size_t N = g->pose.size() / 3, M = g->from_to.size() / 2;
    *out = ym_opt_report{};
    out->lambda_final = p->lambda0;
    out->band = W;
    if (N < 2 || M == 0) return YM_OK;
    DEV_GUARD(g->device);
    ym::PgArgs a;
    if ((rc = graph_sync(g, W, &a)) != YM_OK) return rc;
    if (!g->free_edge) { // nothing can move: zero steps, and the constant cost of the edges between held nodes
        double held_chi2 = 0.0;
        if ((rc = graph_linearise(g, a, &held_chi2)) != YM_OK) return rc;
        out->chi2_initial = out->chi2_final = held_chi2;
        return YM_OK;
    }
    g->poses_stale = true; // (until the poses are back on the host: a call that fails leaves the graph as it was)
    a.cg_tol = p->exact ? 1e-10 : p->cg_tol;
    a.cg_cap = p->exact ? (int32_t)std::min<size_t>(9 * N, 20000) : p->max_cg_iters;
    double chi2 = 0.0, lambda = p->lambda0;
    if ((rc = graph_linearise(g, a, &chi2)) != YM_OK) return rc;
    const double chi2_0 = chi2;
    out->chi2_initial = chi2;
    int status = 0; // 0: the step limit; 1: an accepted step gained no more than 1e-9 chi2; 2: chi2 <= 1e-18 of the initial; 3: lambda > 1e10
    bool linearised = true;
    for (int step = 0; step < p->iters; step++) {
        if (chi2 <= 1e-18 * chi2_0) { status = 2; break; }
        if (!linearised) {
            hipLaunchKernelGGL(ym::pg_linearise_kernel, dim3(graph_blocks(a.n_edges)), dim3(256), 0, g->stream, a);
            linearised = true;
        }
        a.lambda = lambda;
        hipLaunchKernelGGL(ym::pg_assemble_kernel, dim3(graph_blocks(a.n_nodes)), dim3(256), 0, g->stream, a);
        hipLaunchKernelGGL(ym::pg_solve_kernel, dim3(1), dim3(ym::kPgSolveThreads), 0, g->stream, a);
        hipLaunchKernelGGL(ym::pg_update_kernel, dim3(graph_blocks(a.n_nodes)), dim3(256), 0, g->stream, a);
        hipLaunchKernelGGL(ym::pg_chi2_kernel<ym::kPgSumTrial>, dim3(graph_blocks(a.n_edges)), dim3(256), 0, g->stream, a);
        hipLaunchKernelGGL(ym::pg_sum_kernel, dim3(1), dim3(256), 0, g->stream, a);
        HIP_TRY(hipGetLastError());
        double rec[ym::kPgRecWords];
        HIP_TRY(hipMemcpyAsync(rec, a.record, sizeof rec, hipMemcpyDeviceToHost, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        out->lm_steps++;
        out->cg_iterations += (int32_t)rec[ym::kPgRecCg];
        if ((int)rec[ym::kPgRecFlags] & ym::kPgFlagPivot) return set_err(YM_ERR_INVALID, "the system of step %d is not positive definite", step);
        const double chi2_new = rec[ym::kPgRecChi2];
        if (chi2_new < chi2) {
            const double gain = chi2 - chi2_new, before = chi2;
            g->cur ^= 1;
            a.pose = g->d_pose[g->cur].p;
            a.trial = g->d_pose[g->cur ^ 1].p;
            chi2 = chi2_new;
            out->accepted++;
            linearised = false;
            lambda = std::max(lambda / 2.0, 1e-12);
            if (gain <= 1e-9 * before) { status = 1; break; }
        } else { // the poses stay (the trial went to the other buffer)
            lambda *= 2.0;
            if (lambda > 1e10) { status = 3; break; }
        }
    }
    if (status == 0 && chi2 <= 1e-18 * chi2_0) status = 2;
    HIP_TRY(hipMemcpy(g->pose.data(), g->d_pose[g->cur].p, 3 * N * sizeof(double), hipMemcpyDeviceToHost));
    g->poses_stale = false;
    out->chi2_final = chi2;
    out->lambda_final = lambda;
    out->status = status;
    return YM_OK;
}
