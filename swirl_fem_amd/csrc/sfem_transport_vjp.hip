// libsfem_hip: C-ABI entry point of the vector-Jacobian product of the
// scalar-transport right-hand side.
#include "sfem_transport_vjp.h"

using namespace sfem;

extern "C" {

int sfem_transport_rhs_vjp(const sfem_transport_vjp_args* a,
                           sfem_stream_t stream) {
  const char* who = "sfem_transport_rhs_vjp";
  SFEM_REQUIRE(a, "%s: null args", who);
  SFEM_REQUIRE(a->num_elements >= 0 && a->num_levels >= 0,
               "%s: bad sizes", who);
  SFEM_REQUIRE(a->dtype == SFEM_F32 || a->dtype == SFEM_F64,
               "%s: unknown dtype %d", who, a->dtype);
  if (a->ndim != 2 && a->ndim != 3) {
    set_error("%s: ndim=%d (the kernel supports 2 and 3)", who, a->ndim);
    return SFEM_EUNSUPPORTED;
  }
  if (a->P < 2 || a->P > 12) {
    set_error("%s: P=%d outside the compiled range 2..12", who, a->P);
    return SFEM_EUNSUPPORTED;
  }
  if (a->num_levels > SFEM_TRANSPORT_LEVELS) {
    set_error("%s: %d levels (at most %d)", who, a->num_levels,
              SFEM_TRANSPORT_LEVELS);
    return SFEM_EUNSUPPORTED;
  }
  if (a->geo_mode != SFEM_GEO_POINT && a->geo_mode != SFEM_GEO_AFFINE &&
      a->geo_mode != SFEM_GEO_MULTILINEAR) {
    set_error("%s: geo_mode %d (point, affine or multilinear)", who,
              a->geo_mode);
    return SFEM_EUNSUPPORTED;
  }
  if (a->num_elements == 0) return SFEM_OK;
  SFEM_REQUIRE(a->cotangent && a->dmat, "%s: null pointer", who);
  bool needs_wdet = a->dsource != nullptr;
  for (int l = 0; l < a->num_levels; ++l) {
    SFEM_REQUIRE(!a->dvelocity[l] || (a->scalar[l] && a->velocity[l]),
                 "%s: dvelocity of level %d needs its scalar and velocity",
                 who, l);
    needs_wdet = needs_wdet || (a->dscalar[l] && a->mass_coef[l] != 0.0);
  }
  SFEM_REQUIRE(!needs_wdet || a->wdet,
               "%s: mass terms and dsource need `wdet`", who);
  if (a->geo_mode == SFEM_GEO_POINT)
    SFEM_REQUIRE(a->kfac, "%s: per-point geometry needs `kfac`", who);
  else
    SFEM_REQUIRE(a->geo_elem && a->weights && a->nodes,
                 "%s: on-the-fly geometry needs geo_elem, weights and nodes",
                 who);
  const int64_t work = a->elem_list ? a->num_listed : a->num_elements;
  SFEM_REQUIRE(work >= 0 && work <= a->num_elements,
               "%s: bad element list length", who);
  if (work == 0) return SFEM_OK;
  auto run = [&](auto zero) -> int {
    using T = decltype(zero);
    TransportVjpParams<T> tp{};
    tp.geo.kfac = (const T*)a->kfac;
    tp.geo.geo_elem = (const T*)a->geo_elem;
    tp.geo.geo_index = a->geo_index;
    tp.geo.elem_list = a->elem_list;
    tp.geo.dmat_host = (const T*)a->dmat;
    tp.geo.weights_host = (const T*)a->weights;
    tp.geo.nodes_host = (const T*)a->nodes;
    tp.geo.num_elements = work;
    tp.geo.geo_mode = a->geo_mode;
    tp.lam = (const T*)a->cotangent;
    for (int l = 0; l < a->num_levels; ++l) {
      tp.scalar[l] = (const T*)a->scalar[l];
      tp.velocity[l] = (const T*)a->velocity[l];
      tp.mass_coef[l] = (T)a->mass_coef[l];
      tp.conv_coef[l] = (T)a->conv_coef[l];
      tp.dscalar[l] = (T*)a->dscalar[l];
      tp.dvelocity[l] = (T*)a->dvelocity[l];
    }
    tp.wdet = (const T*)a->wdet;
    tp.dsource = (T*)a->dsource;
    tp.num_levels = a->num_levels;
    if (a->ndim == 3)
      return dispatch_transport_vjp<T, 3>(tp, a->P, as_stream(stream));
    return dispatch_transport_vjp<T, 2>(tp, a->P, as_stream(stream));
  };
  if (a->dtype == SFEM_F64) return run(double(0));
  return run(float(0));
}

}  // extern "C"
