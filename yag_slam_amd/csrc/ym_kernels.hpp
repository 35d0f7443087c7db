// ym_kernels.hpp -- gfx950 kernels of the correlative scan matcher (karto semantics).
//
// Pipeline of one call (B independent items; one item = one query scan vs one chain of base scans):
//   prepare_kernel    point readings, valid-point filter, grid cells, coarse lookup table
//                     (Karto LocalizedRangeScan::Update, ScanMatcher::FindValidPoints, AddScan,
//                      GridIndexLookup::ComputeOffsets)
//   raster_kernel     correlation-grid window with the Gaussian max-smear
//                     (ScanMatcher::AddScans + CorrelationGrid::SmearPoint)
//   correlate_kernel  integer gather-reduce over the coarse (x, y, theta) lattice, split over beam
//                     chunks into partial sums (CorrelateScan loops + GetResponse)
//   score_kernel      partial sums -> sums -> response (+ penalty), per-block maxima
//   finish_kernel     coarse arg-max / tie mean / positional covariance, then the whole fine pass
//                     (offsets, 3x3xN correlate, arg-max, angular covariance) in one block per item
//                     (CorrelateScan tail, ComputePositionalCovariance, ComputeAngularCovariance); for few items
//                     fine_kernel (a block per fine angle) + final_kernel.  Both forms are made of the same pieces,
//                     each stated once in ym_k_finish.hpp: coarse_best_and_mean, positional_covariance,
//                     fine_lattice_setup, generic_gather, fine_best_and_mean, angular_covariance, write_result
// All fp64 arithmetic is written operation-for-operation like oracle/ym_oracle.c and the library is
// compiled with -ffp-contract=off, so responses are bit-identical to the oracle's.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "ym_types.h"

// the kernels, one header per stage
#include "ym_k_common.hpp"
#include "ym_k_prepare.hpp"
#include "ym_k_select.hpp"
#include "ym_k_raster.hpp"
#include "ym_k_correlate.hpp"
#include "ym_k_finish.hpp"
#include "ym_k_region.hpp"
#include "ym_k_gather.hpp"
#include "ym_k_yagpy.hpp"
#include "ym_k_yagmap.hpp"
#include "ym_k_sets.hpp"
#include "ym_k_mapgrow.hpp"
#include "ym_k_seenthrough.hpp"
#include "ym_k_occupancy.hpp"
#include "ym_k_raytrace.hpp"
#include "ym_k_locate.hpp"
#include "ym_k_segments.hpp"
#include "ym_k_unionfind.hpp"
#include "ym_k_segmenter.hpp"
#include "ym_k_despeckle.hpp"
#include "ym_k_posegraph.hpp"
