// Host-side scaffold shared by every element-kernel family (not part of the
// ABI): the launch preamble, the run-time -> compile-time selectors of a
// launcher and a dispatch, and the argument checks of the extern "C" entry
// points.  Host code only: nothing here reaches a kernel, so a change here
// cannot move a register (scripts/device_code_digest.py shows that it did
// not).
//
// A kernel family is a params struct, a kernel, and
//
//   template <typename T, int P, int DIM>
//   int launch_x(const XParams<T>& prm, hipStream_t stream) {
//     ElementLaunch<T, P> L;
//     if (int rc = element_launch<HelmholtzTile<T, P, DIM>>("x", prm, &L))
//       return rc;
//     with_geo_mode(prm.geo_mode, [&](auto gm) {
//       hipLaunchKernelGGL((x_kernel<T, P, DIM, decltype(gm)::value>), L.grid,
//                          L.block, 0, stream, prm, L.dm);
//     });
//     SFEM_LAUNCH_CHECK();
//     return SFEM_OK;
//   }
//
// plus a dispatch over P whose body is one with_order call, instantiated by
// one one-line translation unit per (dtype, ndim).
#pragma once
#include <type_traits>
#include <utility>

#include "sfem_common.h"

namespace sfem {

enum GeoMode { GEO_POINT = 0, GEO_AFFINE = 1, GEO_MULTILINEAR = 3 };
constexpr int GEO_BOX = 5;   // facet-table launches only

template <typename T, int P>
struct DMat;
template <typename T, int P>
DMat<T, P> make_dmat(const T* d, const T* w, const T* x);

// ------------------------------------------------------------- preamble ---
// Grid, block and the by-value matrix argument of one launch.
template <typename T, int P>
struct ElementLaunch {
  dim3 grid, block;
  DMat<T, P> dm;
};

inline int check_groups(const char* who, int64_t groups) {
  if (groups > 0x7fffffff) {
    set_error("%s: too many workgroups (%lld)", who, (long long)groups);
    return SFEM_EINVAL;
  }
  return SFEM_OK;
}

// `groups` workgroups of `block` lanes; the three tables are host arrays.
template <typename T, int P>
int element_launch(const char* who, int64_t groups, int block, const T* dmat,
                   const T* weights, const T* nodes, ElementLaunch<T, P>* L) {
  if (int rc = check_groups(who, groups)) return rc;
  L->grid = dim3((unsigned)groups);
  L->block = dim3(block);
  L->dm = make_dmat<T, P>(dmat, weights, nodes);
  return SFEM_OK;
}

// Tile::EPB elements per workgroup of Tile::BLOCK lanes; `prm` carries
// num_elements and the host tables (HelmholtzParams, StokesParams).
template <typename Tile, typename PRM, typename T, int P>
int element_launch(const char* who, const PRM& prm, ElementLaunch<T, P>* L) {
  return element_launch(who, (prm.num_elements + Tile::EPB - 1) / Tile::EPB,
                        Tile::BLOCK, prm.dmat_host, prm.weights_host,
                        prm.nodes_host, L);
}

// ------------------------------------------------------------ selectors ---
// f(std::integral_constant<int, GM>()) for the geometry kind of a launch;
// whatever is neither stored nor affine takes the multilinear kernel (the
// entry points have refused what no kernel takes).
template <typename F>
inline void with_geo_mode(int geo_mode, F&& f) {
  switch (geo_mode) {
    case GEO_POINT: f(std::integral_constant<int, GEO_POINT>()); break;
    case GEO_AFFINE: f(std::integral_constant<int, GEO_AFFINE>()); break;
    default: f(std::integral_constant<int, GEO_MULTILINEAR>()); break;
  }
}

// f(std::true_type()) or f(std::false_type()), and what f returns.
template <typename F>
inline auto with_flag(bool flag, F&& f) {
  return flag ? f(std::true_type()) : f(std::false_type());
}

template <int LO, typename F, int... K>
inline bool order_one_of(int P, F& f, int* rc,
                         std::integer_sequence<int, K...>) {
  return ((P == LO + K
               ? (*rc = f(std::integral_constant<int, LO + K>()), true)
               : false) || ...);
}

// f(std::integral_constant<int, P>()), an int status, for LO <= P <= HI: the
// orders a translation unit instantiates.  Any other P is SFEM_EUNSUPPORTED,
// with a message unless `who` is null (a caller that then takes another path).
template <int LO, int HI, typename F>
inline int with_order(const char* who, int P, F&& f) {
  int rc = SFEM_EUNSUPPORTED;
  if (!order_one_of<LO>(P, f, &rc,
                        std::make_integer_sequence<int, HI - LO + 1>()) &&
      who)
    set_error("%s: P=%d outside the compiled range %d..%d", who, P, LO, HI);
  return rc;
}

// f(double(0)) or f(float(0)) for a checked dtype, f(integral_constant 3 or 2)
// for a checked ndim: the tails of the entry points.
template <typename F>
inline int with_real(int dtype, F&& f) {
  return dtype == SFEM_F64 ? f(double(0)) : f(float(0));
}

template <typename F>
inline int with_dim(int ndim, F&& f) {
  return ndim == 3 ? f(std::integral_constant<int, 3>())
                   : f(std::integral_constant<int, 2>());
}

// --------------------------------------------------------- entry points ---
// dtype (SFEM_EINVAL), then ndim 2..3 and lo <= P <= hi (SFEM_EUNSUPPORTED);
// `pname` is the field's name in the args struct.
inline int check_shape(const char* who, int dtype, int ndim, const char* pname,
                       int P, int lo, int hi) {
  SFEM_REQUIRE(dtype == SFEM_F32 || dtype == SFEM_F64, "%s: unknown dtype %d",
               who, dtype);
  if (ndim != 2 && ndim != 3) {
    set_error("%s: ndim=%d (the kernel supports 2 and 3)", who, ndim);
    return SFEM_EUNSUPPORTED;
  }
  if (P < lo || P > hi) {
    set_error("%s: %s=%d outside the compiled range %d..%d", who, pname, P,
              lo, hi);
    return SFEM_EUNSUPPORTED;
  }
  return SFEM_OK;
}

// Kernels that take the three geometry kinds of with_geo_mode and no other.
inline int check_geo_mode(const char* who, int geo_mode) {
  if (geo_mode != SFEM_GEO_POINT && geo_mode != SFEM_GEO_AFFINE &&
      geo_mode != SFEM_GEO_MULTILINEAR) {
    set_error("%s: geo_mode %d (point, affine or multilinear)", who, geo_mode);
    return SFEM_EUNSUPPORTED;
  }
  return SFEM_OK;
}

// The arrays a geometry kind reads; `stored` / `stored_name`: the per-point
// array of SFEM_GEO_POINT (`geo` or `kfac`).
inline int check_geometry(const char* who, int geo_mode, const void* stored,
                          const char* stored_name, const void* geo_elem,
                          const void* weights, const void* nodes) {
  if (geo_mode == SFEM_GEO_POINT) {
    SFEM_REQUIRE(stored, "%s: per-point geometry needs `%s`", who,
                 stored_name);
  } else if (geo_mode == SFEM_GEO_AFFINE || geo_mode == SFEM_GEO_MULTILINEAR ||
             geo_mode == SFEM_GEO_BOX) {
    SFEM_REQUIRE(geo_elem && weights && nodes,
                 "%s: on-the-fly geometry needs geo_elem, weights and nodes",
                 who);
  } else {
    set_error("%s: unknown geo_mode %d", who, geo_mode);
    return SFEM_EINVAL;
  }
  return SFEM_OK;
}

// *work = the elements of this launch: the list's length or all of them.
inline int check_elem_list(const char* who, const void* elem_list,
                           int64_t num_listed, int64_t num_elements,
                           int64_t* work) {
  *work = elem_list ? num_listed : num_elements;
  SFEM_REQUIRE(*work >= 0 && *work <= num_elements,
               "%s: bad element list length", who);
  return SFEM_OK;
}

}  // namespace sfem
