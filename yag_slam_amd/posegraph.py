"""The pose-graph optimiser behind `LoopClosingMapper(optimizer=...)`, `mapfile.from_file(..., optimizer=...)` and the
reference's `GraphSlam.opt`: the four calls they make on `sba_cpp.SPA2d` (`add_node`, `add_constraint`, `compute`,
`nodes`; /root/reference/yag_slam/graph_slam.py:64,132-192,262-272), served by `ym_graph_*` of libyagmatch.so in fp64 on
one device.  The formulation is SPA2d's (Konolige et al. 2010); `sba_cpp` itself is not available to this project, so
parity with it is NOT pinned: the semantics are DESIGN.md's ("Pose-graph optimiser"), pinned by tests/posegraph_ref.py.

Beyond SPA2d: `hold(nodes)` / `release(nodes)` / `held` keep any set of nodes where they are (a prior map's vertices, a
survey pose, the old part of a long log); `compute` then solves over the free nodes only.
Robust kernels: a constraint may carry `("huber" | "cauchy" | "geman_mcclure", p)`, given to
`add_constraint(..., robust=...)` or `set_robust(edges, robust)`, and can be switched off and on again (`disable`, `enable`);
`edge_terms()` tells each constraint's s = e^T L e and weight, `cost()` the robust objective.  A constraint's index is the
order it was added in, which `add_constraint` returns.
Adds, holds and the per-constraint settings are validated at once and buffered on the host; what is new goes to the library at
the next `compute` / `chi2` (a `disable` goes at once: the library may refuse it).  The
native handle is created then: without a device that raises `YmError`, nothing is computed on the CPU instead.
"""
import ctypes as C
import math

import numpy as np

from . import _capi

STATUS = {0: "step limit", 1: "converged", 2: "residual vanished", 3: "lambda limit"}
ROBUST_KINDS = {"huber": 1, "cauchy": 2, "geman_mcclure": 3}  # YM_ROBUST_*; None is YM_ROBUST_NONE, 0


class OptReport(object):
    """what one `compute` did (ym_opt_report)"""
    __slots__ = ("chi2_initial", "chi2_final", "lambda_final", "lm_steps", "accepted", "cg_iterations", "band", "status")

    def __init__(self, rep):
        for name in self.__slots__:
            setattr(self, name, getattr(rep, name))

    def __repr__(self):
        return "OptReport(%s)" % ", ".join("%s=%r" % (n, getattr(self, n)) for n in self.__slots__)


class Node(object):
    """an item of `PoseGraphOptimizer.nodes`"""
    __slots__ = ("x", "y", "yaw")

    def __init__(self, row):
        self.x, self.y, self.yaw = float(row[0]), float(row[1]), float(row[2])

    def __repr__(self):
        return "Node(x=%r, y=%r, yaw=%r)" % (self.x, self.y, self.yaw)


class NodeView(object):
    """`SPA2d.nodes`: a sequence over the rows of one (N, 3) array; items are made when they are asked for"""

    def __init__(self, xyt):
        self._xyt = xyt

    def __len__(self):
        return len(self._xyt)

    def __getitem__(self, k):
        if isinstance(k, slice):
            return NodeView(self._xyt[k])
        return Node(self._xyt[k])

    def __iter__(self):
        return (Node(row) for row in self._xyt)


def _finite(*values):
    return all(math.isfinite(v) for v in values)


def _robust_pair(robust, what):
    """(YM_ROBUST_ kind, parameter) of `robust`: None, or (name, p) with p finite and positive"""
    if robust is None:
        return 0, 1.0
    try:
        name, p = robust
    except (TypeError, ValueError):
        raise ValueError("%s: robust must be None or (kind, parameter), not %r" % (what, robust))
    if not isinstance(name, str) or name not in ROBUST_KINDS:
        raise ValueError("%s: robust kind %r: one of %s" % (what, name, ", ".join(sorted(ROBUST_KINDS))))
    try:
        p = float(p)
    except (TypeError, ValueError):
        raise ValueError("%s: the parameter of a robust kernel must be a number, not %r" % (what, p))
    if not math.isfinite(p) or not p > 0.0:
        raise ValueError("%s: the parameter of a robust kernel must be finite and positive, not %r" % (what, p))
    return ROBUST_KINDS[name], p


class PoseGraphOptimizer(object):
    def __init__(self, device=0):
        self.device = int(device)
        self._h = None
        self._xyt = np.zeros((0, 3))   # every node's pose: as added, or as the last compute left it
        self._new_nodes = []           # rows of _xyt the library has not seen
        self._new_edges = []           # (a, b, x, y, yaw, info 3 x 3)
        self._n_edges = 0
        self._held = {0}               # the held nodes as the library will know them after the next flush
        # what the library has not heard of the held set and of the constraints' kernels and switches, in call order:
        # ("hold", int32 nodes, 1 / 0), ("robust", int32 edges, kind, p), ("enable", int32 edges, 1 / 0)
        self._new_ops = []
        self.band = -1                # compute's preconditioner band: -1 automatic, 0 .. 16 (0: block-Jacobi)
        self.last_report = None

    # ---- the SPA2d surface
    def add_node(self, x, y, yaw, num):
        n = len(self._xyt) + len(self._new_nodes)
        if int(num) != n:
            raise ValueError("add_node: num %r, the next node is %d" % (num, n))
        x, y, yaw = float(x), float(y), float(yaw)
        if not _finite(x, y, yaw):
            raise ValueError("add_node: a pose that is not finite")
        self._new_nodes.append((x, y, yaw))

    def add_constraint(self, a, b, x, y, yaw, info, robust=None):
        """`SPA2d.add_constraint`; robust: None or ("huber" | "cauchy" | "geman_mcclure", p).  Returns the constraint's index."""
        n = len(self._xyt) + len(self._new_nodes)
        a, b = int(a), int(b)
        if not (0 <= a < n and 0 <= b < n):
            raise ValueError("add_constraint: nodes %d -> %d out of range (%d nodes)" % (a, b, n))
        if a == b:
            raise ValueError("add_constraint: from a node to itself (%d)" % a)
        info = np.array(info, dtype=np.float64)
        if info.shape != (3, 3):
            raise ValueError("add_constraint: info must be 3 x 3")
        x, y, yaw = float(x), float(y), float(yaw)
        if not _finite(x, y, yaw) or not np.isfinite(info).all():
            raise ValueError("add_constraint: a value that is not finite")
        if not (np.diag(info) > 0).all():
            raise ValueError("add_constraint: an information matrix without a positive diagonal")
        kind, p = _robust_pair(robust, "add_constraint")
        self._new_edges.append((a, b, x, y, yaw, info))
        self._n_edges += 1
        if kind:
            self._new_ops.append(("robust", np.array([self._n_edges - 1], dtype=np.int32), kind, p))
        return self._n_edges - 1

    def compute(self, iters=100, lam=1.0e-4, use_csparse=True, init_tol=1.0e-9, max_cg_iters=50):
        """`SPA2d.compute`.  use_csparse: every step solved to a relative residual of 1e-10 (init_tol and max_cg_iters are
        ignored, as SPA2d's Cholesky path ignores them); otherwise conjugate gradients to init_tol within max_cg_iters."""
        L = self._flush()
        p = _capi.YmOptParams(int(iters), int(bool(use_csparse)), int(max_cg_iters), int(self.band), float(lam), float(init_tol))
        rep = _capi.YmOptReport()
        _capi.check(L.ym_graph_optimize(self._h, C.byref(p), C.byref(rep)))
        if len(self._xyt):
            _capi.check(L.ym_graph_get_poses(self._h, 0, self._xyt.ctypes.data_as(C.POINTER(C.c_double)), len(self._xyt)))
        self.last_report = OptReport(rep)
        return self.last_report

    @property
    def nodes(self):
        return NodeView(self.nodes_xyt)

    # ---- beyond SPA2d
    @property
    def nodes_xyt(self):
        """(N, 3) float64: x, y, yaw of every node"""
        if self._new_nodes:
            return np.concatenate([self._xyt, np.array(self._new_nodes, dtype=np.float64).reshape(-1, 3)])
        return self._xyt

    def hold(self, nodes):
        """Holds the nodes where they are: `compute` solves over the others and leaves a held node's pose bit for bit
        (DESIGN.md section 9).  Node 0 is always held.  Validated at once, buffered like the adds."""
        self._set_held(nodes, 1)

    def release(self, nodes):
        """Frees nodes held before; node 0 cannot be released."""
        self._set_held(nodes, 0)

    @property
    def held(self):
        """the held nodes: a sorted int array that always contains 0"""
        return np.array(sorted(self._held), dtype=np.int64)

    def _set_held(self, nodes, flag):
        what = "hold" if flag else "release"
        arr = np.asarray(list(nodes) if not isinstance(nodes, np.ndarray) else nodes)
        if arr.size and not np.issubdtype(arr.dtype, np.integer):
            raise ValueError("%s: node indices must be integers" % what)
        arr = arr.astype(np.int64).reshape(-1)
        n = len(self._xyt) + len(self._new_nodes)
        bad = arr[(arr < 0) | (arr >= n)]
        if bad.size:
            raise ValueError("%s: node %d out of range (%d nodes)" % (what, int(bad[0]), n))
        if not flag and (arr == 0).any():
            raise ValueError("release: node 0 is always held and cannot be released")
        if not arr.size:
            return
        if flag:
            self._held.update(int(v) for v in arr)
        else:
            self._held.difference_update(int(v) for v in arr)
        self._new_ops.append(("hold", np.ascontiguousarray(arr, dtype=np.int32), flag))

    @property
    def n_constraints(self):
        return self._n_edges

    def _edge_indices(self, edges, what):
        arr = np.asarray(list(edges) if not isinstance(edges, np.ndarray) else edges)
        if arr.size and not np.issubdtype(arr.dtype, np.integer):
            raise ValueError("%s: constraint indices must be integers" % what)
        arr = arr.astype(np.int64).reshape(-1)
        bad = arr[(arr < 0) | (arr >= self._n_edges)]
        if bad.size:
            raise ValueError("%s: constraint %d out of range (%d constraints)" % (what, int(bad[0]), self._n_edges))
        return np.ascontiguousarray(arr, dtype=np.int32)

    def set_robust(self, edges, robust):
        """The robust kernel of these constraints: ("huber" | "cauchy" | "geman_mcclure", p), or None for the plain square."""
        kind, p = _robust_pair(robust, "set_robust")
        arr = self._edge_indices(edges, "set_robust")
        if arr.size:
            self._new_ops.append(("robust", arr, kind, p))

    def enable(self, edges):
        """Switches constraints disabled before on again."""
        arr = self._edge_indices(edges, "enable")
        if arr.size:
            self._new_ops.append(("enable", arr, 1))

    def disable(self, edges):
        """Takes these constraints out of the objective (cost and weight 0) without forgetting them.  Goes to the library at
        once: it raises `YmError`, and changes nothing, if a free node would be left without an enabled constraint."""
        arr = self._edge_indices(edges, "disable")
        if arr.size:
            self._new_ops.append(("enable", arr, 0))
            self._flush()

    def edge_terms(self):
        """(s, w): s = e^T L e of every constraint at the current poses and its weight w = rho'(s); w of a disabled one is 0"""
        L = self._flush()
        s, w = np.zeros(self._n_edges), np.zeros(self._n_edges)
        dp = C.POINTER(C.c_double)
        _capi.check(L.ym_graph_edge_terms(self._h, s.ctypes.data_as(dp), w.ctypes.data_as(dp)))
        return s, w

    def cost(self):
        """F = the sum of rho(s) over the constraints, what `compute` lowers; `chi2()` is the plain sum of s over the enabled ones"""
        L = self._flush()
        out = C.c_double()
        _capi.check(L.ym_graph_cost(self._h, C.byref(out)))
        return out.value

    def chi2(self):
        L = self._flush()
        out = C.c_double()
        _capi.check(L.ym_graph_chi2(self._h, C.byref(out)))
        return out.value

    def linearise(self):
        """(cost, diagonal blocks (N, 3, 3), gradient (N, 3)) of the undamped, weighted system at the current poses, node 0
        included; the cost is chi2 on a graph without robust kernels"""
        L = self._flush()
        n = len(self._xyt)
        chi2, diag, grad = C.c_double(), np.zeros((n, 3, 3)), np.zeros((n, 3))
        dp = C.POINTER(C.c_double)
        _capi.check(L.ym_graph_linearise(self._h, C.byref(chi2), diag.ctypes.data_as(dp), grad.ctypes.data_as(dp)))
        return chi2.value, diag, grad

    def solve_step(self, lam, band=None, cg_tol=1.0e-10, max_cg_iters=0):
        """One damped solve at the current poses, which stay (ym_graph_solve, a test hook): (delta (N, 3), z (N, 3), band,
        iterations, residual, flags).  delta is the conjugate-gradient iterate and z the last application of the
        preconditioner; with max_cg_iters = 0 delta is 0 and z = band(A, band)^-1 b.  band None: `self.band`.  The rows of
        held nodes are zero; the rows of the free nodes in index order are the solve order's slots 1 .. F."""
        L = self._flush()
        n = len(self._xyt)
        delta, z = np.zeros((n, 3)), np.zeros((n, 3))
        used, iters, res, flags = C.c_int32(), C.c_int32(), C.c_double(), C.c_int32()
        dp = C.POINTER(C.c_double)
        _capi.check(L.ym_graph_solve(self._h, int(self.band if band is None else band), float(lam), float(cg_tol), int(max_cg_iters),
                                     delta.ctypes.data_as(dp), z.ctypes.data_as(dp), C.byref(used), C.byref(iters), C.byref(res),
                                     C.byref(flags)))
        return delta, z, used.value, iters.value, res.value, flags.value

    def set_poses(self, xyt, first=0):
        xyt = np.ascontiguousarray(xyt, dtype=np.float64).reshape(-1, 3)
        L = self._flush()
        _capi.check(L.ym_graph_set_poses(self._h, int(first), xyt.ctypes.data_as(C.POINTER(C.c_double)), len(xyt)))
        self._xyt[first:first + len(xyt)] = xyt

    def close(self):
        """frees the native handle; the optimiser is not used afterwards"""
        if self._h is not None:
            _capi.lib().ym_graph_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _flush(self):
        """the native handle, holding everything added so far"""
        L = _capi.lib()
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        if self._h is None:
            h = L.ym_graph_create(self.device)
            if not h:
                raise _capi.YmError(-2, _capi.last_error())
            self._h = h
        if self._new_nodes:
            new = np.ascontiguousarray(np.array(self._new_nodes, dtype=np.float64).reshape(-1, 3))
            _capi.check(L.ym_graph_add_nodes(self._h, new.ctypes.data_as(dp), len(new)))
            self._xyt = np.ascontiguousarray(np.concatenate([self._xyt, new]))
            self._new_nodes = []
        if self._new_edges:
            ft = np.ascontiguousarray([(e[0], e[1]) for e in self._new_edges], dtype=np.int32)
            mean = np.ascontiguousarray([e[2:5] for e in self._new_edges], dtype=np.float64)
            info = np.ascontiguousarray([e[5] for e in self._new_edges], dtype=np.float64)
            _capi.check(L.ym_graph_add_constraints(self._h, ft.ctypes.data_as(ip), mean.ctypes.data_as(dp), info.ctypes.data_as(dp),
                                                   len(ft)))
            self._new_edges = []
        while self._new_ops:  # (an op the library refuses is dropped with the error it raises)
            op = self._new_ops.pop(0)
            if op[0] == "hold":
                _capi.check(L.ym_graph_hold(self._h, op[1].ctypes.data_as(ip), len(op[1]), op[2]))
            elif op[0] == "robust":
                _capi.check(L.ym_graph_set_robust(self._h, op[1].ctypes.data_as(ip), len(op[1]), op[2], op[3]))
            else:
                _capi.check(L.ym_graph_enable(self._h, op[1].ctypes.data_as(ip), len(op[1]), op[2]))
        return L


SPA2d = PoseGraphOptimizer
