// libsfem_hip: fields at arbitrary points.  The point locator
// (setup: run-time P1, double arithmetic, one lane per point) and the C-ABI
// entry points of the evaluation kernels of sfem_points.h.
#include "sfem_points.h"

using namespace sfem;

namespace sfem {

constexpr int LOCATE_BLOCK = 64;
constexpr int LOCATE_MAX_P = 12;

struct LocateParams {
  const void* points;
  const void* node_coords;
  const int32_t* elements;
  const int64_t* cell_offsets;
  const int32_t* cell_elems;
  const double* boxes;
  const double* extent;
  int32_t* element;
  void* xi;
  uint8_t* found;
  double nodes[LOCATE_MAX_P];
  double bary[LOCATE_MAX_P];
  double grid_lo[3], grid_hi[3], inv_cell[3];
  double tol_xi, tol_x;
  int64_t num_points, num_nodes, num_elements;
  int32_t ncell[3];
  int32_t max_iter, P1;
};

// One lane per point.  The 1D basis values and derivatives of the lane's
// current xi live in LDS, word (slot, lane) at slot * 64 + lane, so run-time
// P1 indexes LDS and not a register array; a lane reads its own words only,
// so the one barrier is the one after the shared node table is written.
template <typename T, int DIM>
__global__ void __launch_bounds__(LOCATE_BLOCK)
point_locate_kernel(LocateParams lp) {
  __shared__ double sx[LOCATE_MAX_P], sw[LOCATE_MAX_P];
  __shared__ double bl[2 * DIM * LOCATE_MAX_P * LOCATE_BLOCK];
  const int lane = threadIdx.x;
#pragma unroll
  for (int i = 0; i < LOCATE_MAX_P; ++i) {   // every lane, the same values
    sx[i] = lp.nodes[i];
    sw[i] = lp.bary[i];
  }
  __syncthreads();
  const int64_t m = (int64_t)blockIdx.x * LOCATE_BLOCK + lane;
  if (m >= lp.num_points) return;            // no barrier below
  const int P1 = lp.P1;
  constexpr int Z = DIM - 1;   // the last axis: 2 in 3D, in bounds in 2D
  const int n = DIM == 3 ? P1 * P1 * P1 : P1 * P1;
  const T* points = (const T*)lp.points;
  const T* coords = (const T*)lp.node_coords;

  double xp[DIM];
  bool inside = true;
  int64_t cell = 0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) {
    xp[a] = (double)points[m * DIM + a];
    inside = inside && xp[a] >= lp.grid_lo[a] && xp[a] <= lp.grid_hi[a];
    double f = (xp[a] - lp.grid_lo[a]) * lp.inv_cell[a];
    // NaN and out-of-range values land in a valid cell; `inside` decides
    int ca = 0;
    if (f >= 0.0) ca = f < (double)lp.ncell[a] ? (int)f : lp.ncell[a] - 1;
    if (ca > lp.ncell[a] - 1) ca = lp.ncell[a] - 1;
    if (ca < 0) ca = 0;
    cell = cell * lp.ncell[a] + ca;
  }

  int32_t hit = -1;
  double hit_xi[DIM];
#pragma unroll
  for (int a = 0; a < DIM; ++a) hit_xi[a] = 0.0;

  const int64_t s_begin = inside ? lp.cell_offsets[cell] : 0;
  const int64_t s_end = inside ? lp.cell_offsets[cell + 1] : 0;
  for (int64_t s = s_begin; s < s_end && hit < 0; ++s) {
    const int64_t e = lp.cell_elems[s];
    if (e < 0 || e >= lp.num_elements) continue;
    const double* box = lp.boxes + e * 2 * DIM;
    bool in_box = true;
#pragma unroll
    for (int a = 0; a < DIM; ++a)
      in_box = in_box && xp[a] >= box[a] && xp[a] <= box[DIM + a];
    if (!in_box) continue;
    const double ext = lp.extent[e];
    const int32_t* row = lp.elements + e * n;

    double xi[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) xi[a] = 0.0;
    double res = 1e300;
    // Two passes at most.  The map of a curved element, continued past the
    // element, can fold back onto the point, and Newton from the centre can
    // end on that outer preimage of a point on a face; a pass that ends
    // outside starts once more from the nearest point of the reference cube.
    for (int pass = 0; pass < 2 && hit < 0; ++pass) {
      for (int it = 0; it <= lp.max_iter; ++it) {
        // 1D values and derivatives in the product form
        for (int a = 0; a < DIM; ++a) {
          const double x = xi[a];
          for (int i = 0; i < P1; ++i) {
            double p = sw[i], dp = 0.0;
            for (int k = 0; k < P1; ++k) {
              if (k == i) continue;
              const double d = x - sx[k];
              dp = dp * d + p;
              p = p * d;
            }
            bl[((a * 2 + 0) * LOCATE_MAX_P + i) * LOCATE_BLOCK + lane] = p;
            bl[((a * 2 + 1) * LOCATE_MAX_P + i) * LOCATE_BLOCK + lane] = dp;
          }
        }
#define SFEM_BL(a, der, i) \
  bl[(((a) * 2 + (der)) * LOCATE_MAX_P + (i)) * LOCATE_BLOCK + lane]
        double X[DIM], J[DIM][DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
          X[a] = 0.0;
#pragma unroll
          for (int b = 0; b < DIM; ++b) J[a][b] = 0.0;
        }
        if (DIM == 3) {
          for (int i = 0; i < P1; ++i) {
            const double l0 = SFEM_BL(0, 0, i), d0 = SFEM_BL(0, 1, i);
            for (int j = 0; j < P1; ++j) {
              const double l1 = SFEM_BL(1, 0, j), d1 = SFEM_BL(1, 1, j);
              const double vv = l0 * l1, v0 = d0 * l1, v1 = l0 * d1;
              for (int k = 0; k < P1; ++k) {
                const double l2 = SFEM_BL(2, 0, k), d2 = SFEM_BL(2, 1, k);
                const int64_t id = row[(i * P1 + j) * P1 + k];
                const bool ok = id >= 0 && id < lp.num_nodes;
#pragma unroll
                for (int a = 0; a < DIM; ++a) {
                  const double c = ok ? (double)coords[id * DIM + a] : 0.0;
                  X[a] += c * (vv * l2);
                  J[a][0] += c * (v0 * l2);
                  J[a][1] += c * (v1 * l2);
                  J[a][Z] += c * (vv * d2);
                }
              }
            }
          }
        } else {
          for (int i = 0; i < P1; ++i) {
            const double l0 = SFEM_BL(0, 0, i), d0 = SFEM_BL(0, 1, i);
            for (int j = 0; j < P1; ++j) {
              const double l1 = SFEM_BL(1, 0, j), d1 = SFEM_BL(1, 1, j);
              const int64_t id = row[i * P1 + j];
              const bool ok = id >= 0 && id < lp.num_nodes;
#pragma unroll
              for (int a = 0; a < DIM; ++a) {
                const double c = ok ? (double)coords[id * DIM + a] : 0.0;
                X[a] += c * (l0 * l1);
                J[a][0] += c * (d0 * l1);
                J[a][1] += c * (l0 * d1);
              }
            }
          }
        }
#undef SFEM_BL
        double r[DIM];
        res = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
          r[a] = X[a] - xp[a];
          const double ar = fabs(r[a]);
          res = ar > res || ar != ar ? ar : res;
        }
        if (it == lp.max_iter || res <= 1e-13 * ext) break;
        double dxi[DIM];
        double det;
        if (DIM == 3) {
          const double c00 = J[1][1] * J[Z][Z] - J[1][Z] * J[Z][1];
          const double c01 = J[1][0] * J[Z][Z] - J[1][Z] * J[Z][0];
          const double c02 = J[1][0] * J[Z][1] - J[1][1] * J[Z][0];
          det = J[0][0] * c00 - J[0][1] * c01 + J[0][Z] * c02;
          const double r0 = r[0], r1 = r[1], r2 = r[Z];
          dxi[0] = r0 * c00 -
                   J[0][1] * (r1 * J[Z][Z] - J[1][Z] * r2) +
                   J[0][Z] * (r1 * J[Z][1] - J[1][1] * r2);
          dxi[1] = J[0][0] * (r1 * J[Z][Z] - J[1][Z] * r2) -
                   r0 * c01 +
                   J[0][Z] * (J[1][0] * r2 - r1 * J[Z][0]);
          dxi[Z] = J[0][0] * (J[1][1] * r2 - r1 * J[Z][1]) -
                         J[0][1] * (J[1][0] * r2 - r1 * J[Z][0]) +
                         r0 * c02;
        } else {
          det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
          dxi[0] = r[0] * J[1][1] - J[0][1] * r[1];
          dxi[1] = J[0][0] * r[1] - r[0] * J[1][0];
        }
        if (!(fabs(det) > 0.0)) {   // singular or NaN: this candidate is out
          res = 1e300;
          break;
        }
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
          double v = xi[a] - dxi[a] / det;
          v = v < 1.5 ? v : 1.5;      // a NaN becomes 1.5 and fails below
          v = v > -1.5 ? v : -1.5;
          xi[a] = v;
        }
      }
      double amax = 0.0;
#pragma unroll
      for (int a = 0; a < DIM; ++a)
        amax = fabs(xi[a]) > amax ? fabs(xi[a]) : amax;
      if (amax <= 1.0 + lp.tol_xi && res <= lp.tol_x * ext) {
        hit = (int32_t)e;
#pragma unroll
        for (int a = 0; a < DIM; ++a) hit_xi[a] = xi[a];
      }
      if (!(amax > 1.0 + lp.tol_xi)) break;   // inside and refused: no restart
#pragma unroll
      for (int a = 0; a < DIM; ++a)
        xi[a] = xi[a] < 1.0 ? (xi[a] > -1.0 ? xi[a] : -1.0) : 1.0;
    }
  }

  lp.element[m] = hit;
  lp.found[m] = hit >= 0 ? 1 : 0;
  T* xo = (T*)lp.xi + m * DIM;
#pragma unroll
  for (int a = 0; a < DIM; ++a) xo[a] = (T)hit_xi[a];
}

}  // namespace sfem

namespace {

int check_point_args(const sfem_point_args* a, const char* who,
                     bool transpose) {
  SFEM_REQUIRE(a, "%s: null args", who);
  SFEM_REQUIRE(a->num_points >= 0 && a->num_found >= 0 && a->num_chunks >= 0 &&
                   a->num_segments >= 0 && a->num_elements >= 0 &&
                   a->num_nodes >= 0,
               "%s: negative size", who);
  SFEM_REQUIRE(a->num_found <= a->num_points,
               "%s: more found points than points", who);
  SFEM_REQUIRE(a->ncomp >= 1, "%s: ncomp=%d", who, a->ncomp);
  int rc = check_shape(who, a->dtype, a->ndim, "P1", a->P1, 2, 12);
  if (rc) return rc;
  SFEM_REQUIRE(a->nodes && a->bary, "%s: null basis table", who);
  const int64_t launches = transpose ? a->num_segments : a->num_chunks;
  rc = check_groups(who, launches);
  if (rc) return rc;
  if (a->num_found == 0 || launches == 0) return SFEM_OK;
  SFEM_REQUIRE(a->values && a->elements && a->xi && a->perm,
               "%s: null pointer", who);
  if (transpose)
    SFEM_REQUIRE(a->rows && a->seg_elem && a->seg_offsets,
                 "%s: null pointer (rows or segments)", who);
  else
    SFEM_REQUIRE(a->field && a->chunk_elem && a->chunk_start && a->chunk_count,
                 "%s: null pointer (field or chunks)", who);
  return SFEM_OK;
}

int run_point_eval(const sfem_point_args* a, bool transpose,
                   sfem_stream_t stream) {
  return with_real(a->dtype, [&](auto zero) {
    using T = decltype(zero);
    PointParams<T> pp{};
    pp.field = (const T*)a->field;
    pp.values = (T*)a->values;
    pp.rows = (T*)a->rows;
    pp.elements = a->elements;
    pp.xi = (const T*)a->xi;
    pp.perm = a->perm;
    pp.chunk_elem = a->chunk_elem;
    pp.chunk_start = a->chunk_start;
    pp.chunk_count = a->chunk_count;
    pp.seg_elem = a->seg_elem;
    pp.seg_offsets = a->seg_offsets;
    pp.num_chunks = a->num_chunks;
    pp.num_segments = a->num_segments;
    pp.node_stride = a->node_stride;
    pp.comp_stride = a->comp_stride;
    pp.ncomp = a->ncomp;
    return with_dim(a->ndim, [&](auto d) {
      return dispatch_point_eval<T, decltype(d)::value>(
          pp, a->P1, a->nodes, a->bary, transpose, as_stream(stream));
    });
  });
}

}  // namespace

extern "C" {

int sfem_point_locate(const sfem_point_locate_args* a, sfem_stream_t stream) {
  const char* who = "sfem_point_locate";
  SFEM_REQUIRE(a, "%s: null args", who);
  SFEM_REQUIRE(a->num_points >= 0 && a->num_nodes >= 0 && a->num_elements >= 0,
               "%s: negative size", who);
  int rc = check_shape(who, a->dtype, a->ndim, "P1", a->P1, 2, LOCATE_MAX_P);
  if (rc) return rc;
  SFEM_REQUIRE(a->max_iter >= 0 && a->max_iter <= 64,
               "%s: max_iter=%d outside 0..64", who, a->max_iter);
  SFEM_REQUIRE(a->tol_xi >= 0.0 && a->tol_x >= 0.0,
               "%s: negative or NaN tolerance", who);
  for (int d = 0; d < a->ndim; ++d) {
    SFEM_REQUIRE(a->ncell[d] >= 1, "%s: ncell[%d]=%d", who, d, a->ncell[d]);
    SFEM_REQUIRE(a->grid_hi[d] >= a->grid_lo[d] && a->inv_cell[d] >= 0.0,
                 "%s: bad grid along axis %d", who, d);
  }
  SFEM_REQUIRE(a->nodes && a->bary, "%s: null basis table", who);
  if (a->num_points == 0) return SFEM_OK;
  SFEM_REQUIRE(a->points && a->element && a->xi && a->found,
               "%s: null pointer (points or outputs)", who);
  SFEM_REQUIRE(a->node_coords && a->elements && a->cell_offsets &&
                   a->cell_elems && a->boxes && a->extent,
               "%s: null pointer (mesh or candidates)", who);
  const int64_t groups = (a->num_points + LOCATE_BLOCK - 1) / LOCATE_BLOCK;
  rc = check_groups(who, groups);
  if (rc) return rc;
  LocateParams lp{};
  lp.points = a->points;
  lp.node_coords = a->node_coords;
  lp.elements = a->elements;
  lp.cell_offsets = a->cell_offsets;
  lp.cell_elems = a->cell_elems;
  lp.boxes = a->boxes;
  lp.extent = a->extent;
  lp.element = a->element;
  lp.xi = a->xi;
  lp.found = a->found;
  for (int i = 0; i < LOCATE_MAX_P; ++i) {
    lp.nodes[i] = i < a->P1 ? a->nodes[i] : 0.0;
    lp.bary[i] = i < a->P1 ? a->bary[i] : 0.0;
  }
  for (int d = 0; d < 3; ++d) {
    const bool on = d < a->ndim;
    lp.grid_lo[d] = on ? a->grid_lo[d] : 0.0;
    lp.grid_hi[d] = on ? a->grid_hi[d] : 0.0;
    lp.inv_cell[d] = on ? a->inv_cell[d] : 0.0;
    lp.ncell[d] = on ? a->ncell[d] : 1;
  }
  lp.tol_xi = a->tol_xi;
  lp.tol_x = a->tol_x;
  lp.num_points = a->num_points;
  lp.num_nodes = a->num_nodes;
  lp.num_elements = a->num_elements;
  lp.max_iter = a->max_iter;
  lp.P1 = a->P1;
  const dim3 grid((unsigned)groups), block(LOCATE_BLOCK);
  hipStream_t s = as_stream(stream);
  with_real(a->dtype, [&](auto zero) {
    return with_dim(a->ndim, [&](auto d) {
      hipLaunchKernelGGL(
          (point_locate_kernel<decltype(zero), decltype(d)::value>), grid,
          block, 0, s, lp);
      return (int)SFEM_OK;
    });
  });
  SFEM_LAUNCH_CHECK();
  return SFEM_OK;
}

int sfem_point_eval(const sfem_point_args* a, sfem_stream_t stream) {
  const int rc = check_point_args(a, "sfem_point_eval", false);
  if (rc != SFEM_OK) return rc;
  if (a->num_found == 0 || a->num_chunks == 0) return SFEM_OK;
  return run_point_eval(a, false, stream);
}

int sfem_point_eval_t(const sfem_point_args* a, sfem_stream_t stream) {
  const int rc = check_point_args(a, "sfem_point_eval_t", true);
  if (rc != SFEM_OK) return rc;
  if (a->num_found == 0 || a->num_segments == 0) return SFEM_OK;
  return run_point_eval(a, true, stream);
}

}  // extern "C"
