"""Sequential mapping driver: the caller side of the hot path.

A minimal restatement of the call pattern of `GraphSlam.process_scan`
(/root/reference/yag_slam/graph_slam.py:306-339): odometry prior = last corrected pose composed
with the odometry increment, `seq_matcher.match_scan(query, running_scans, True, True)`, running
chain of the last `scan_buffer_len` scans (default 10, graph_slam.py:47,336-337).  No pose graph, no
optimiser, no loop closure here -- this only drives the matcher the way yag-slam does, with every
scan resident on the device (one upload per new scan, poses written through).
"""
import math

import numpy as np

from .models import LocalizedRangeScan, native_many, set_corrected_poses
from .transform import Transform


class SequentialMapper(object):
    def __init__(self, seq_matcher, scan_buffer_len=10):
        self.seq_matcher = seq_matcher
        self.scan_buffer_len = scan_buffer_len
        self.running_scans = []
        self.results = []

    def process_scan(self, scan):
        """scan: LocalizedRangeScan with .odom_pose set.  Returns the matcher result (None for the first scan)."""
        query = scan
        if len(self.running_scans) == 0:
            query.num = 0
            self.running_scans.append(query)
            return None
        last_scan = self.running_scans[-1]
        query.num = last_scan.num + 1
        fast = getattr(self.seq_matcher, "process_scan", None)
        res = fast(query, self.running_scans, True, True) if fast is not None else None
        if res is None:  # (any matcher plugin: the three steps of graph_slam.py:320-327)
            odom_diff = query.odom_pose - last_scan.odom_pose
            query.corrected_pose = last_scan.corrected_pose + odom_diff
            res = self.seq_matcher.match_scan(query, self.running_scans, True, True)
            query.corrected_pose = res.best_pose
        self.running_scans.append(query)
        self.running_scans = self.running_scans[-self.scan_buffer_len:]
        self.results.append(res)
        return res


    def process_scans(self, scans, device_chain=False):
        """`process_scan` for every scan of a trajectory with the loop itself inside the library (`ym_map_sequence`: no
        Python between two matches).  Same poses, results and running chain as calling `process_scan` scan by scan;
        returns the list of results (None for the very first scan of a map).  device_chain: the device also hands each
        step's pose to the next without a host round trip (ScanMatcher.map_sequence); poses then agree to rounding."""
        scans = list(scans)
        out = []
        if scans and not self.running_scans:
            out.append(self.process_scan(scans.pop(0)))
        if not scans:
            return out
        native = getattr(self.seq_matcher, "map_sequence", None)
        resident = all(isinstance(s, LocalizedRangeScan) for s in self.running_scans + scans)
        if native is None or not resident:  # (any matcher plugin, any scan type: scan by scan, as process_scan does)
            return out + [self.process_scan(s) for s in scans]
        start = len(self.running_scans)
        seq = self.running_scans + scans
        for k in range(start, len(seq)):
            seq[k].num = seq[k - 1].num + 1
        try:
            res = native(seq, start, self.scan_buffer_len, True, True, device_chain)
        except Exception:
            # the scans matched before the failing one are done (poses final on both sides): the mapper's state is what
            # the per-scan loop would have left when it raised at that scan
            res = list(getattr(self.seq_matcher, "sequence_done", None) or [])
            self.running_scans = (seq[:start + len(res)])[-self.scan_buffer_len:]
            self.results.extend(res)
            raise
        self.running_scans = seq[-self.scan_buffer_len:]
        self.results.extend(res)
        return out + res


def _dist2(a, b):
    """squared planar distance between two scans' corrected poses (helpers.py:383-386)"""
    pa, pb = a.corrected_pose, b.corrected_pose
    return (pa.x - pb.x) ** 2 + (pa.y - pb.y) ** 2


class PoseBuckets(object):
    """Coarse spatial index of scans by corrected pose.

    Same candidate set as the reference's `RadiusHashSearch.crude_radius_search`
    (/root/reference/yag_slam/helpers.py:396-431): scans are bucketed by `(int(x/res), int(y/res))`
    (truncation toward zero) and a query returns every scan whose bucket CORNER `(ix*res, iy*res)` lies
    within `radius + res` of the query position.  Only the bounded block of buckets that can satisfy
    that test is visited instead of the whole table."""

    def __init__(self, res):
        self.res = float(res)
        self.buckets = {}

    def key(self, pose):
        return (int(pose.x / self.res), int(pose.y / self.res))

    def add(self, scan):
        self.buckets.setdefault(self.key(scan.corrected_pose), []).append(scan)

    def rebuild(self, scans):
        self.buckets = {}
        for s in scans:
            self.add(s)

    def near(self, pose, radius):
        reach = radius + self.res
        r2 = reach * reach
        lo_x, hi_x = int((pose.x - reach) / self.res) - 1, int((pose.x + reach) / self.res) + 1
        lo_y, hi_y = int((pose.y - reach) / self.res) - 1, int((pose.y + reach) / self.res) + 1
        out = []
        for ix in range(lo_x, hi_x + 1):
            for iy in range(lo_y, hi_y + 1):
                got = self.buckets.get((ix, iy))
                if got and (ix * self.res - pose.x) ** 2 + (iy * self.res - pose.y) ** 2 < r2:
                    out.extend(got)
        return out

    def near_ordered(self, pose, radius):
        """the scans of `near` in the order `crude_radius_search` returns them (helpers.py:420-431): buckets by their
        first insertion, scans by insertion within a bucket.  Visits the whole table, as the reference does."""
        reach = radius + self.res
        r2 = reach * reach
        out = []
        for (ix, iy), got in self.buckets.items():
            if (ix * self.res - pose.x) ** 2 + (iy * self.res - pose.y) ** 2 < r2:
                out.extend(got)
        return out


class LoopClosingMapper(SequentialMapper):
    """`GraphSlam.process_scan` + `try_to_close_loop` as the matcher sees them
    (/root/reference/yag_slam/graph_slam.py:194-261,272-339), with the per-chain coarse loop of
    `try_to_close_loop` (graph_slam.py:217-220) issued as ONE batched enqueue.

    What is kept: the odometry prior, the running chain, the constraint bookkeeping (previous scan,
    closest scan of the running chain, closest scan of the closing chain), candidate-chain discovery
    with the reference's exact rules (including its comparison of a SQUARED distance with
    `loop_search_dist`, graph_slam.py:290, and its dropping of the last candidate of the sorted list,
    :284), the two-stage acceptance (coarse loop matcher without penalty >= min_response_coarse, then
    the fine sequential matcher seeded with the coarse pose), first acceptable chain wins.
    The sparse pose adjustment the reference runs after a closure (`SPA2d`, third party) is what one
    passes as `optimizer`: `yag_slam_amd.posegraph.PoseGraphOptimizer()` optimises the graph on the
    device and `run_opt` re-poses every vertex; any object with the same four calls (`add_node`,
    `add_constraint`, `compute`, `nodes`) works.  Without one (the default) the closure only corrects
    the closing scan.

    The reference rejects a low FINE response only when `verbose` is set (`... and self.verbose`,
    graph_slam.py:240); `reject_low_fine=None` follows that, True/False overrides it.

    `robust_closures=(kind, p)` (None, the default: everything as before) gives the constraint a closure adds -- and no other:
    odometry and running-chain constraints stay plain -- that robust kernel of the optimiser (DESIGN.md section 9.2;
    `PoseGraphOptimizer.add_constraint(..., robust=)`), so that one false closure cannot bend the trajectory.
    `closure_weights()` then tells how much each closure still counts, and `drop_closures(max_weight)` takes out the ones
    that count less than that."""

    def __init__(self, seq_matcher, loop_matcher, scan_buffer_len=10, loop_search_dist=3,
                 loop_search_min_chain_size=10, min_response_coarse=0.35, min_response_fine=0.45,
                 verbose=False, optimizer=None, reject_low_fine=None, robust_closures=None):
        super().__init__(seq_matcher, scan_buffer_len)
        if robust_closures is not None:
            from .posegraph import _robust_pair
            _robust_pair(robust_closures, "LoopClosingMapper: robust_closures")
        self.robust_closures = robust_closures
        self.loop_matcher = loop_matcher
        self.loop_search_dist = loop_search_dist
        self.loop_search_min_chain_size = loop_search_min_chain_size
        self.min_response_coarse = min_response_coarse
        self.min_response_fine = min_response_fine
        self.verbose = verbose
        self.reject_low_fine = verbose if reject_low_fine is None else reject_low_fine
        self.opt = optimizer
        self.held_nums = set()    # vertices held through hold_vertices
        self.scans = []          # vertex list, index == scan.num
        self.adjacent = []        # adjacency sets by scan.num
        self.constraints = []     # (from_num, to_num, mean Transform, covariance)
        self.index = PoseBuckets(loop_search_dist)
        self.closures = []        # (scan.num, chain nums, coarse result, fine result)
        self.closure_edges = []   # per closure: the index of its constraint in the optimiser (None: it added none)
        self.last_edge = None     # the optimiser's index of the constraint the last link_scans added
        self.dropped_edges = set()  # the constraints drop_closures disabled

    # ---- graph bookkeeping (graph_slam.py:132-192) ----
    def add_vertex(self, scan):
        assert scan.num == len(self.scans)
        self.scans.append(scan)
        self.adjacent.append(set())
        self.index.add(scan)
        if self.opt is not None:
            p = scan.corrected_pose
            self.opt.add_node(p.x, p.y, p.euler[-1], scan.num)

    def link_scans(self, from_scan, to_scan, covariance, robust=None):
        """robust: the optimiser's robust kernel for this constraint, (kind, p); passed on only when set"""
        if to_scan.num in self.adjacent[from_scan.num] or from_scan.num == to_scan.num:
            return False
        mean = to_scan.corrected_pose - from_scan.corrected_pose
        self.adjacent[from_scan.num].add(to_scan.num)
        self.adjacent[to_scan.num].add(from_scan.num)
        self.constraints.append((from_scan.num, to_scan.num, mean, covariance))
        if self.opt is not None:
            import numpy as np
            kw = {} if robust is None else {"robust": robust}
            edge = self.opt.add_constraint(from_scan.num, to_scan.num, mean.x, mean.y, mean.euler[-1],
                                           np.linalg.inv(np.array(covariance)).tolist(), **kw)
            # (an optimiser with SPA2d's four calls returns nothing: its constraints are in the order of `constraints`)
            self.last_edge = edge if isinstance(edge, int) else len(self.constraints) - 1
        return True

    def link_to_closest_scan_in_chain(self, scan, chain, covariance, robust=None):
        return self.link_scans(min(chain, key=lambda s: _dist2(s, scan)), scan, covariance, robust)

    def near_linked(self, scan):
        """scans reachable from `scan` through constraints without leaving the loop_search_dist disc
        (`do_breadth_first_traversal` with `make_near_scan_visitor`, graph.py:73-101, graph_slam.py:32-39)"""
        limit = self.loop_search_dist ** 2
        seen, todo, inside = {scan.num}, [scan.num], set()
        while todo:
            n = todo.pop()
            if not _dist2(self.scans[n], scan) < limit:
                continue
            inside.add(n)
            for a in self.adjacent[n]:
                if a not in seen:
                    seen.add(a)
                    todo.append(a)
        return inside

    def find_possible_loop_closure_chains(self, scan):
        """graph_slam.py:274-304"""
        excluded = self.near_linked(scan)
        cand = sorted(self.index.near(scan.corrected_pose, self.loop_search_dist), key=lambda s: s.num)
        chains, current = [], []
        for s, nxt in zip(cand, cand[1:]):
            if s.num == scan.num or s.num in excluded:
                current = []
                continue
            if _dist2(scan, s) <= self.loop_search_dist:
                current.append(s)
            if len(current) >= self.loop_search_min_chain_size:
                chains.append(current)
                current = []
            if nxt.num - s.num > 1:
                current = []
        if current:
            chains.append(current)
        return chains

    def try_to_close_loop(self, scan):
        """graph_slam.py:194-261"""
        if not self.loop_matcher:
            return False
        chains = self.find_possible_loop_closure_chains(scan)
        if not chains:
            return False
        if hasattr(self.loop_matcher, "match_scan_batch"):
            coarse, _ = self.loop_matcher.match_scan_batch(scan, chains, False, False)
        else:
            coarse = [self.loop_matcher.match_scan(scan, chain, False, False) for chain in chains]
        for chain, res_coarse in zip(chains, coarse):
            if res_coarse.response < self.min_response_coarse:
                continue
            tmp = scan.copy()
            tmp.corrected_pose = res_coarse.best_pose
            res = self.seq_matcher.match_scan(tmp, chain, False, True)
            if res.response < self.min_response_fine and self.reject_low_fine:
                continue
            scan.corrected_pose = res.best_pose
            linked = self.link_to_closest_scan_in_chain(scan, chain, res.covariance, self.robust_closures)
            self.closures.append((scan.num, [s.num for s in chain], res_coarse, res))
            self.closure_edges.append(self.last_edge if linked and self.opt is not None else None)
            self.run_opt()
            return True
        return False

    def make_occupancy_grid(self, resolution=0.05, range_threshold=12):
        """graph_slam.py:341-342: every vertex scan ray-traced into one grid (on the device)"""
        from .occupancy import create_occupancy_grid
        return create_occupancy_grid(self.scans, resolution, range_threshold, device=getattr(self.seq_matcher, "device", 0))

    def make_ros_map(self, resolution=0.05, range_threshold=12):
        """slam_node_ros1:187-209 (`_make_map`): that grid with its specks removed and the codes of nav_msgs/OccupancyGrid"""
        from .occupancy import ros_map
        return ros_map(self.scans, resolution, range_threshold, device=getattr(self.seq_matcher, "device", 0))

    def live_ros_map(self, resolution=0.05, range_threshold=12, **filter_opts):
        """make_ros_map from counts that stay on the device (occupancy.LiveOccupancyGrid): only the
        scans added or moved since the last call are traced.  The grid is made on first use, and anew when the resolution or
        the threshold changes; its lattice is anchored at the first call's bounding-box minimum, so its origin is not the one
        make_ros_map would give (a fraction of a cell apart)."""
        from .occupancy import LiveOccupancyGrid
        live = getattr(self, "live_grid", None)
        if live is None or (live.resolution, live.range_threshold) != (float(resolution), float(range_threshold)):
            if live is not None:
                live.close()
            live = self.live_grid = LiveOccupancyGrid(resolution, range_threshold, device=getattr(self.seq_matcher, "device", 0))
        live.sync(self.scans)
        return live.ros_map(**filter_opts)

    def hold_vertices(self, scans_or_nums):
        """Keeps these vertices (scans, or their nums) where they are in every later `run_opt`: the optimiser's `hold`
        (posegraph.PoseGraphOptimizer).  The vertices of a prior map are the case it is for."""
        if self.opt is None or not hasattr(self.opt, "hold"):
            raise ValueError("hold_vertices: the mapper has no optimizer with hold()")
        nums = [int(getattr(v, "num", v)) for v in scans_or_nums]
        self.opt.hold(nums)
        self.held_nums.update(nums)

    def run_opt(self):
        """graph_slam.py:262-272; a no-op without an optimizer except for the spatial index refresh.  Held vertices are not
        written: their `corrected_pose` keeps its bits."""
        if self.opt is not None:
            self.opt.compute(100, 1.0e-4, True, 1.0e-9, 50)
            n = min(len(self.opt.nodes), len(self.scans))  # (zip's length, as graph_slam.py:268)
            free = [k for k in range(n) if k not in self.held_nums] if self.held_nums else range(n)
            nodes = self.opt.nodes
            set_corrected_poses([self.scans[k] for k in free], [Transform(nodes[k].x, nodes[k].y, 0.0, nodes[k].yaw) for k in free])
        self.index.rebuild(self.scans)

    def closure_weights(self):
        """[(scan num, constraint index, s, w)] of every closure that added a constraint, at the poses of the last `run_opt`:
        s = e^T L e and the weight w its robust kernel gives it (`PoseGraphOptimizer.edge_terms`); w of a closure that fits
        is near 1, of one that contradicts the rest of the graph near 0 (exactly 1 without `robust_closures`)."""
        if self.opt is None or not hasattr(self.opt, "edge_terms"):
            raise ValueError("closure_weights: the mapper has no optimizer with edge_terms()")
        s, w = self.opt.edge_terms()
        return [(c[0], e, float(s[e]), float(w[e])) for c, e in zip(self.closures, self.closure_edges) if e is not None]

    def drop_closures(self, max_weight):
        """Disables the constraint of every closure whose weight (`closure_weights`) is below `max_weight`, forgets that the
        two scans were linked (so that the pair can close again later), runs `run_opt` and returns what it dropped, as
        `closure_weights` lists it.  The closures leave `closures` and `closure_edges`; the constraints stay in `constraints`
        and in the optimiser, disabled (their indices are in `dropped_edges`)."""
        drop = [c for c in self.closure_weights() if c[3] < max_weight]
        if not drop:
            return []
        edges = {c[1] for c in drop}
        self.opt.disable(sorted(edges))  # (refused, and nothing changed, if a free vertex would lose its last constraint)
        for e in edges:  # (the optimiser's constraints are in the order of `constraints`: both are filled by the same calls)
            f, t = self.constraints[e][:2]
            self.adjacent[f].discard(t)
            self.adjacent[t].discard(f)
        keep = [k for k, e in enumerate(self.closure_edges) if e not in edges]
        self.closures = [self.closures[k] for k in keep]
        self.closure_edges = [self.closure_edges[k] for k in keep]
        self.dropped_edges |= edges
        self.run_opt()
        return drop

    def process_scan(self, scan):
        """Returns (result, closed) like graph_slam.py:306-339; (None, None) for the first scan."""
        query = scan
        if len(self.running_scans) == 0:
            query.num = 0
            self.running_scans.append(query)
            self.add_vertex(query)
            return None, None
        last_scan = self.running_scans[-1]
        query.num = last_scan.num + 1
        query.corrected_pose = last_scan.corrected_pose + (query.odom_pose - last_scan.odom_pose)
        res = self.seq_matcher.match_scan(query, self.running_scans, True, True)
        query.corrected_pose = res.best_pose
        self.add_vertex(query)
        self.link_scans(last_scan, query, res.covariance)
        if self.loop_matcher:
            self.link_to_closest_scan_in_chain(query, self.running_scans, res.covariance)
        closed = self.try_to_close_loop(query)
        self.running_scans.append(query)
        self.running_scans = self.running_scans[-self.scan_buffer_len:]
        self.results.append(res)
        return res, closed

    def relocalize(self, scan, cmap, ox, oy, **kw):
        """A node switched on somewhere inside a known map: find where `scan` was taken in the resident CorrelationMap `cmap`
        (cell (0, 0) at world (ox, oy); `ScanMatcher.locate_in_map` of the map's matcher, keywords passed on), set
        `scan.odom_pose` and `scan.corrected_pose` to the located and polished pose and return the result;
        `splice_first_scan(scan)` proceeds from there.  Raises ValueError when nothing reaches min_response."""
        res = cmap.m.locate_in_map(cmap, ox, oy, [scan], **kw)
        p = res.best_pose[0]
        scan.odom_pose = Transform(p.x, p.y, 0.0, p.euler[-1])
        scan.corrected_pose = Transform(p.x, p.y, 0.0, p.euler[-1])
        return res

    def splice_first_scan(self, scan, radius=5):
        """The first live scan after a prior map was ingested (`splicing.map_to_graphslam`): the ROS node's "first scan when
        splicing into a map" (slam_node_ros1:240-253).  `scan.odom_pose` and `scan.corrected_pose` hold the initial pose.
        num = the largest num + 1; candidates = the pose index's scans around `scan.odom_pose`
        (`crude_radius_search(odom_pose, radius)`, in its order); `seq_matcher.match_scan(scan, candidates, True, True)`;
        corrected_pose = best_pose; `add_vertex`; `link_scans(scan, candidates[0], covariance)`; the scan starts the running
        chain.  Returns the matcher result; `process_scan` continues from here.  With no candidate (the reference fails on
        `nearby_scans[0]`) a ValueError is raised before anything changes; if the matcher raises, the scan gets its old num back
        and the mapper is as it was."""
        if not self.scans:
            raise ValueError("splice_first_scan: no map was ingested (the mapper holds no vertex)")
        candidates = self.index.near_ordered(scan.odom_pose, radius)
        if not candidates:
            raise ValueError("splice_first_scan: no scan of the map within %g m of (%g, %g)"
                             % (radius, scan.odom_pose.x, scan.odom_pose.y))
        had_num, old_num = hasattr(scan, "num"), getattr(scan, "num", None)
        scan.num = max(s.num for s in self.scans) + 1
        try:
            res = self.seq_matcher.match_scan(scan, candidates, True, True)
        except Exception:  # the matcher raised: the mapper is untouched, and so is the scan's num
            if had_num:
                scan.num = old_num
            else:
                del scan.num
            raise
        scan.corrected_pose = res.best_pose
        self.add_vertex(scan)
        self.link_scans(scan, candidates[0], res.covariance)
        self.running_scans.append(scan)
        return res


class MapLocalizer(object):
    """Localization mode: follow a robot through a resident map without growing a graph (`ScanMatcher.track_in_map`,
    `ym_map_track`).  No vertex, no constraint, no running chain: the map is the only thing scans are matched against.

    matcher: a `ScanMatcher(..., semantics="yagpy")`; cmap: its resident CorrelationMap whose cell (0, 0) lies at world
    (ox, oy); coarse: dict overriding the coarse pass of `match_scan_sets_with_map`; min_response: below it a step's
    correction is not applied and the scan keeps its odometry prior (dead reckoning).

    `last` is the last scan processed (its `corrected_pose` is the robot's pose in the map), `lost` the number of
    consecutive steps whose correction was not applied, `results` every step's result.

    Alternatives.  `start(scan, places=K)` with K > 1 keeps one `MapAlternative` per distinct place the map offers
    (`ScanMatcher.locate_in_map(places=K)`) and follows them all, one `track_in_map` call per step, until the evidence
    leaves one: `alternatives` (alive, in place order), `ambiguous` (more than one alive), `leader`.  Per step, in this
    order: (1) every alternative's `evidence` grows by its step's response and its `lost` is counted as `MapLocalizer.lost`
    is; (2) the leader is the alternative with the largest evidence, a tie going to the lower place; (3) an alternative
    whose evidence trails the leader's by `evidence_gap` or more, or whose `lost` reached `max_lost`, is dropped -- never the
    leader; (4) an alternative within both merge[0] metres and merge[1] radians (modulo 2 pi) of one with more evidence is
    dropped; (5) the caller's scan takes the leader's pose, and `lost` and `results` follow the leader's.  With one
    alternative left, every later step is the single-track step on the caller's own scans.  The three defaults are policy,
    not measurements."""

    def __init__(self, matcher, cmap, ox, oy, coarse=None, min_response=0.0, evidence_gap=0.5, max_lost=3, merge=(0.2, 0.1)):
        self.matcher, self.cmap, self.ox, self.oy = matcher, cmap, ox, oy
        self.coarse, self.min_response = coarse, min_response
        self.evidence_gap, self.max_lost, self.merge = float(evidence_gap), int(max_lost), (float(merge[0]), float(merge[1]))
        self.last = None
        self.lost = 0
        self.results = []
        self._alts = []

    @property
    def alternatives(self):
        """the alternatives still alive, in place order (empty when the localizer was started without `places`)"""
        return list(self._alts)

    @property
    def ambiguous(self):
        return len(self._alts) > 1

    @property
    def leader(self):
        """the alternative with the largest evidence, a tie going to the lower place (None without alternatives)"""
        best = None
        for a in self._alts:
            if best is None or a.evidence > best.evidence:
                best = a
        return best

    def start(self, scan, places=None, min_separation=(1.0, 0.5), **locate_kw):
        """The first scan.  With its pose known (`corrected_pose` and `odom_pose` set by the caller) it only becomes `last`;
        with keywords for `ScanMatcher.locate_in_map` it is located in the map first (`relocalize`) and both poses are set
        to the located, polished pose.  Returns the locate result, or None.
        places = K > 1: K distinct places (at least `min_separation` = (metres, radians) apart) are located and polished, one
        alternative is kept per place found, and the scan gets the best polished place's pose."""
        self._alts = []
        if places is not None and int(places) > 1:
            return self._start_places(scan, int(places), min_separation, locate_kw)
        res = None
        if locate_kw or places is not None:
            res = self.matcher.locate_in_map(self.cmap, self.ox, self.oy, [scan], **locate_kw)
            p = res.best_pose[0]
            scan.odom_pose = Transform(p.x, p.y, 0.0, p.euler[-1])
            scan.corrected_pose = Transform(p.x, p.y, 0.0, p.euler[-1])
        self.last, self.lost = scan, 0
        return res

    def process_scan(self, scan):
        """One step of one track: prior = last.corrected_pose + (scan.odom_pose - last.odom_pose), the match against the
        map, `scan.corrected_pose` = the corrected pose (or the prior).  Returns the result (meta["accepted"]); the very
        first scan only starts the track (None)."""
        out = self.process_scans([scan])
        return out[0] if out else None

    def process_scans(self, scans):
        """`process_scan` for several scans of the stream in ONE library call; the list of their results.  A scan the
        matcher cannot serve (no valid reading) raises after the scans before it are done; it keeps its prior and the
        track goes on from it."""
        scans = list(scans)
        if scans and self.last is None:
            self.start(scans.pop(0))
        if not scans:
            return []
        if self.ambiguous:
            if len(scans) > 1:
                raise ValueError("MapLocalizer: while alternatives are alive (`ambiguous`) process_scans takes one scan at a time")
            return [self._step_alternatives(scans[0])]
        res, done = self.matcher.track_in_map(self.cmap, self.ox, self.oy, [self.last] + scans, 1, True, True, self.coarse,
                                              self.min_response)
        got = res[1:done]
        for r in got:
            self.lost = 0 if r.meta["accepted"] else self.lost + 1
        self.results.extend(got)
        self.last = ([self.last] + scans)[min(done, len(scans))]
        if done <= len(scans):
            raise ValueError("MapLocalizer: scan %d of the call could not be matched (no valid reading or an empty lattice); "
                             "it keeps its odometry prior" % (done - 1))
        return got

    def _start_places(self, scan, places, min_separation, locate_kw):
        res = self.matcher.locate_in_map(self.cmap, self.ox, self.oy, [scan], places=places, min_separation=min_separation, **locate_kw)
        if "places" not in res.meta:
            raise ValueError("MapLocalizer.start(places=K) needs the polished places: leave refine=True")
        p = res.best_pose[0]
        scan.odom_pose = Transform(p.x, p.y, 0.0, p.euler[-1])
        scan.corrected_pose = Transform(p.x, p.y, 0.0, p.euler[-1])
        for i, polished in enumerate(res.meta["places"]):
            q = polished.best_pose[0]
            own = scan.copy()
            own.corrected_pose = Transform(q.x, q.y, 0.0, q.euler[-1])  # (its odometry stays the caller's: increments are shared)
            self._alts.append(MapAlternative(i, own))
        self.last, self.lost = scan, 0
        self._results_before = list(self.results)
        return res

    def _step_alternatives(self, scan):
        """one step of every alive alternative in one `track_in_map` call, then the five-step rule of the class docstring"""
        alts = self._alts
        copies = []
        for a in alts:
            c = scan.copy()
            c.odom_pose = scan.odom_pose
            copies.append(c)
        out = self.matcher.track_in_map(self.cmap, self.ox, self.oy, [[a.last, c] for a, c in zip(alts, copies)], 1, True, True,
                                        self.coarse, self.min_response)
        served = {}
        for a, c, (res, done) in zip(alts, copies, out):
            a.last = c
            r = res[1] if done > 1 else None
            if r is None:  # the matcher could not serve the scan: it keeps its prior, as a step that was not applied
                a.lost += 1
                continue
            a.evidence += r.response
            a.lost = 0 if r.meta["accepted"] else a.lost + 1
            a.results.append(r)
            served[a.place] = r
        lead = self.leader
        alive = [a for a in alts if a is lead or not (lead.evidence - a.evidence >= self.evidence_gap or a.lost >= self.max_lost)]
        kept = []
        for a in alive:
            pa = a.last.corrected_pose
            for b in alive:
                pb = b.last.corrected_pose
                da = (pa.euler[-1] - pb.euler[-1] + math.pi) % (2 * math.pi) - math.pi
                if b.evidence > a.evidence and math.hypot(pa.x - pb.x, pa.y - pb.y) <= self.merge[0] and abs(da) <= self.merge[1]:
                    break
            else:
                kept.append(a)
        self._alts = kept
        p = lead.last.corrected_pose
        scan.corrected_pose = Transform(p.x, p.y, 0.0, p.euler[-1])
        self.last, self.lost = scan, lead.lost
        self.results = self._results_before + list(lead.results)
        return served.get(lead.place)


class MapAlternative(object):
    """One place a `MapLocalizer` started with `places=K` still follows: `place` (its index in the located order), `last`
    (its own copy of the last scan, at this alternative's pose), `evidence` (the sum of its steps' responses), `lost`
    (consecutive steps whose correction was not applied) and `results` (its steps' results)."""

    def __init__(self, place, last):
        self.place, self.last = place, last
        self.evidence, self.lost, self.results = 0.0, 0, []


class MapBuilder(object):
    """Mapping mode over a resident map: every scan is tracked in the map (`MapLocalizer`'s step, one
    `ScanMatcher.track_in_map` call on [last, scan]) and the scans that moved far enough are then added to it
    (`CorrelationMap.add_scans`), so the robot can leave what the map showed when it started.  No graph, no running chain.

    matcher: a `ScanMatcher(..., semantics="yagpy")`; cmap: an empty map (`matcher.empty_correlation_map`) or a prior map that
    is to be kept current, its cell (0, 0) at world (ox, oy); coarse, min_response: as in `MapLocalizer`; min_distance
    (metres), min_rotation (radians): a tracked scan is added when its pose differs from the last added scan's by at least
    one of the two -- the ROS node's keyframe rule (slam_node_ros1:299-301) negated.  A step whose correction was not applied
    is never added: its pose is dead reckoning.

    window=N (None: no limit) keeps a rolling local map, the resident counterpart of the reference's `running_scans` buffer: at
    most N keyframes stay in the map, and adding one more takes the oldest out in the same library call
    (`CorrelationMap.update_scans`).  That needs a map that can forget, a counted one
    (`matcher.empty_correlation_map(w, h, counted=True, ox=ox, oy=oy)`), which the builder then owns: it
    holds the builder's keyframes and nothing else.

    extent="fixed" (the default) leaves the map's extent as the caller sized it.  "scroll" and "grow" let the map follow the robot
    (`CorrelationMap.reframe`): after a step's pose is known and before the scan is added, a pose nearer
    than `margin` metres to a side of the map moves the window -- "scroll" keeps the size and recentres it on the robot, "grow"
    enlarges it to the union of the old extent and the robot's pose +- margin -- by a whole number of `step` cells.  margin=None:
    the matcher's range threshold plus the coarse search's half-width plus the taps' reach, what a step reads or stamps around
    the pose.  With a window and "scroll" the map need only be twice that across, not as large as the site.  The builder's `ox`,
    `oy` follow the window: the first origin plus the whole offset times the resolution, never step by step (on a counted map
    that is the map's own `origin`).  On a map that keeps no counts a reframe keeps the overlap and nothing else: readings that
    were dropped beyond a side do not come back when the window moves over them.

    forget_seen_through=min_readings (None: off; an integer of at least 1, which needs a counted map as `window` does) lets the
    map notice that the world changed (`CorrelationMap.seen_through`): after a keyframe has been added,
    every other scan of `added` is counted against that one viewer with `clearance` and `protect`, and each scan of which the
    keyframe looks through at least `min_readings` readings is replaced -- all of them in one `CorrelationMap.update_scans` call
    -- by its `blanked(flags)` copy, which takes the old scan's place in `added` (the order and the window's idea of "oldest"
    stay).  Readings go, not scans: the walls an old scan saw stay in the map.  A copy with no valid reading left is only removed
    and goes to `dropped`.  The map stays, bit for bit, the fresh counted map of the scans in `added`.  The defaults of
    `clearance` and `protect` come from a numpy prototype on one synthetic room, not from a device or a
    real log.

    `last` is the last scan processed, `last_added` the last one added, `added` every scan in the map (in order), `dropped`
    the scans the window has taken out again (in order), `lost` the number of consecutive steps whose correction was not
    applied, `results` every step's result, `reframes` the MapReframeStats of every move of the window, `blanked` the
    (old, new) pairs `forget_seen_through` has swapped (in order)."""

    # rebuild() on a counted map: above this share of moved keyframes the map is cleared and filled again.  Measured with 2000
    # scans of 1081 beams (profiles/map_forget_time.json): with 5 x 5 taps moving costs as much as clearing
    # and adding all at a share of 0.2, with 29 x 29 taps only at 1.0 (there a builder may set its REBUILD_SHARE to 1.0).
    REBUILD_SHARE = 0.2

    def __init__(self, matcher, cmap, ox, oy, coarse=None, min_response=0.0, min_distance=0.0, min_rotation=0.0, window=None,
                 extent="fixed", margin=None, step=32, forget_seen_through=None, clearance=2, protect=1):
        if extent not in ("fixed", "scroll", "grow"):
            raise ValueError("MapBuilder: extent %r: \"fixed\", \"scroll\" or \"grow\"" % (extent,))
        if extent != "fixed":
            if isinstance(step, bool) or not isinstance(step, int) or step < 1:
                raise ValueError("MapBuilder: step %r: an integer of at least 1 (cells)" % (step,))
            if margin is not None and not margin > 0:
                raise ValueError("MapBuilder: margin %r: None or metres above 0" % (margin,))
        if window is not None:
            if isinstance(window, bool) or not isinstance(window, int) or window < 1:
                raise ValueError("MapBuilder: window %r: None or an integer of at least 1" % (window,))
            if not getattr(cmap, "counted", False):
                raise ValueError("MapBuilder: a window needs a map that can forget: "
                                 "matcher.empty_correlation_map(w, h, counted=True, ox=ox, oy=oy)")
        if forget_seen_through is not None:
            for name, v, least in (("forget_seen_through", forget_seen_through, 1), ("clearance", clearance, 0), ("protect", protect, 0)):
                if isinstance(v, bool) or not isinstance(v, int) or v < least:
                    raise ValueError("MapBuilder: %s %r: an integer of at least %d" % (name, v, least))
            if not getattr(cmap, "counted", False):
                raise ValueError("MapBuilder: a window needs a map that can forget: "
                                 "matcher.empty_correlation_map(w, h, counted=True, ox=ox, oy=oy)")
        self.matcher, self.cmap, self.ox, self.oy = matcher, cmap, ox, oy
        self.coarse, self.min_response = coarse, min_response
        self.forget_seen_through, self.clearance, self.protect = forget_seen_through, clearance, protect
        self.blanked = []
        self.min_distance, self.min_rotation = min_distance, min_rotation
        self.window = window
        self.extent, self.margin, self.step = extent, margin, step
        self.reframes = []
        if extent != "fixed":
            cfg = matcher.config
            self._res = float(cfg.resolution)
            if margin is None:
                reach = 2 * int(round(float(cfg.smear_deviation) / self._res)) * self._res  # half the taps' width, in metres
                self.margin = float(cfg.range_threshold) + float((coarse or {}).get("xy_search", 0.25)) + reach
            # the lattice the window moves in: a counted map's own anchor and offset, else the origin the caller gave
            anchor = getattr(cmap, "anchor", None) if getattr(cmap, "counted", False) else None
            self._base = (ox, oy) if anchor is None else anchor
            self._offset = (0, 0) if anchor is None else tuple(cmap.window[:2])
        self.last = None
        self.last_added = None
        self.added = []
        self.dropped = []
        self.lost = 0
        self.results = []

    def _add(self, scan):
        if self.window is not None and len(self.added) >= self.window:
            oldest = self.added[0]
            stats = self.cmap.update_scans([oldest], [scan])  # (MapUpdateStats)
            self.dropped.append(self.added.pop(0))
        else:
            stats = self.cmap.add_scans(self.ox, self.oy, [scan])
        self.added.append(scan)
        self.last_added = scan
        if self.forget_seen_through is not None:
            self._forget_seen_through(scan)
        return stats

    def _forget_seen_through(self, keyframe):
        """the readings of the other added scans that `keyframe` looks through go: one count, one swap"""
        others = [s for s in self.added if s is not keyframe]
        if not others:
            return
        st = self.cmap.seen_through([keyframe], scans=others, clearance=self.clearance, protect=self.protect, flags=True)
        olds, news = [], []
        for old, seen, flags in zip(st.scans, st.seen, st.flags):
            if seen >= self.forget_seen_through:
                new = old.blanked(flags)
                olds.append(old)
                with np.errstate(invalid="ignore"):
                    blind = bool(np.all((new.ranges > new.range_threshold) | np.isnan(new.ranges)))  # (no point reading left)
                news.append(None if blind else new)
        if not olds:
            return
        kept = [n for n in news if n is not None]
        native_many(kept, self.matcher.device)  # (the copies' device twins in one library call)
        self.cmap.update_scans(olds, kept)
        place = {id(s): i for i, s in enumerate(self.added)}
        for old, new in zip(olds, news):
            if new is not None:
                self.added[place[id(old)]] = new
                self.blanked.append((old, new))
        gone = {id(o) for o, n in zip(olds, news) if n is None}
        self.dropped.extend(s for s in self.added if id(s) in gone)
        self.added = [s for s in self.added if id(s) not in gone]

    def _follow(self, scan):
        """extent "scroll" / "grow": move the window if the scan's pose is nearer than `margin` to a side; the reframe's stats or None"""
        if self.extent == "fixed":
            return None
        res, (h, w) = self._res, self.cmap.shape
        p = scan.corrected_pose
        px, py, m = (p.x - self.ox) / res, (p.y - self.oy) / res, self.margin / res  # in cells of the window
        if px - m >= 0 and px + m <= w and py - m >= 0 and py + m <= h:
            return None
        k = self.step
        if self.extent == "scroll":
            dx, dy, nw, nh = k * int(round((px - 0.5 * w) / k)), k * int(round((py - 0.5 * h) / k)), w, h
        else:
            x0, y0 = min(0, k * int(math.floor((px - m) / k))), min(0, k * int(math.floor((py - m) / k)))
            x1, y1 = max(w, k * int(math.ceil((px + m) / k))), max(h, k * int(math.ceil((py + m) / k)))
            dx, dy, nw, nh = x0, y0, x1 - x0, y1 - y0
        if (dx, dy, nw, nh) == (0, 0, w, h):
            return None  # (a window narrower than two margins: recentred as well as the step allows)
        stats = self.cmap.reframe(dx, dy, nw, nh)
        self._offset = (self._offset[0] + dx, self._offset[1] + dy)
        # from the first origin and the whole offset, as the library computes a counted map's origin: repeated moves do not drift
        self.ox, self.oy = self._base[0] + self._offset[0] * res, self._base[1] + self._offset[1] * res
        self.reframes.append(stats)
        return stats

    def start(self, scan):
        """The first scan: its pose is known (`corrected_pose` and `odom_pose` set by the caller).  It is added to the map and
        becomes `last` and `last_added`.  Returns the add's MapAddStats."""
        self._follow(scan)
        stats = self._add(scan)
        self.last, self.lost = scan, 0
        return stats

    def _is_keyframe(self, scan):
        p, l = scan.corrected_pose, self.last_added.corrected_pose
        near = ((p.x - l.x) ** 2 + (p.y - l.y) ** 2 < self.min_distance ** 2 and
                abs(p.euler[-1] - l.euler[-1]) < self.min_rotation)
        return not near

    def process_scan(self, scan):
        """One step: prior = last.corrected_pose + (scan.odom_pose - last.odom_pose), the match against the map as it is,
        `scan.corrected_pose` = the corrected pose (or the prior); then, if the correction was applied and the keyframe rule
        holds, the scan is added to the map.  Returns the result (meta["accepted"], meta["added"]); the very first scan only
        starts the map (None).  A scan the matcher cannot serve (no valid reading) raises; it keeps its prior, is not added,
        and the track goes on from it."""
        if self.last is None:
            self.start(scan)
            return None
        res, done = self.matcher.track_in_map(self.cmap, self.ox, self.oy, [self.last, scan], 1, True, True, self.coarse,
                                              self.min_response)
        self.last = scan
        if done < 2:
            raise ValueError("MapBuilder: the scan could not be matched (no valid reading or an empty lattice); "
                             "it keeps its odometry prior")
        r = res[1]
        self.lost = 0 if r.meta["accepted"] else self.lost + 1
        r.meta["added"] = bool(r.meta["accepted"] and self._is_keyframe(scan))
        self._follow(scan)
        if r.meta["added"]:
            self._add(scan)
        self.results.append(r)
        return r

    def process_scans(self, scans):
        """`process_scan` for each scan in turn (every step needs the map as the step before left it); the list of results."""
        out = []
        for s in scans:
            r = self.process_scan(s)
            if r is not None:
                out.append(r)
        return out

    def rebuild(self):
        """Bring the map to the current poses of `added`, after an optimiser moved them.  A map that keeps no counts is cleared
        and every scan of `added` added again, in one library call (a maximum cannot be undone scan by scan); returns the
        add's MapAddStats.  A counted map moves the scans whose pose changed (`CorrelationMap.sync`, MapUpdateStats), which
        costs what moved; when more than REBUILD_SHARE of them moved it is cleared and filled like the other."""
        if getattr(self.cmap, "counted", False):
            moved = self.cmap.moved_scans(self.added)
            if len(moved) <= self.REBUILD_SHARE * len(self.added):
                return self.cmap.sync(moved)  # (the poses of the others have been compared once: 0.6 ms for 2000 scans)
        self.cmap.clear()
        return self.cmap.add_scans(self.ox, self.oy, list(self.added))
