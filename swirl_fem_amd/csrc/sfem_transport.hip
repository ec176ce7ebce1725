// libsfem_hip: C-ABI entry point of the scalar-transport right-hand side.
#include "sfem_transport.h"

using namespace sfem;

extern "C" {

int sfem_transport_rhs(const sfem_transport_args* a, sfem_stream_t stream) {
  const char* who = "sfem_transport_rhs";
  SFEM_REQUIRE(a, "%s: null args", who);
  SFEM_REQUIRE(a->num_elements >= 0 && a->num_levels >= 0,
               "%s: bad sizes", who);
  int rc = check_shape(who, a->dtype, a->ndim, "P", a->P, 2, 12);
  if (rc) return rc;
  if (a->num_levels > SFEM_TRANSPORT_LEVELS) {
    set_error("%s: %d levels (at most %d)", who, a->num_levels,
              SFEM_TRANSPORT_LEVELS);
    return SFEM_EUNSUPPORTED;
  }
  rc = check_geo_mode(who, a->geo_mode);
  if (rc) return rc;
  if (a->num_elements == 0) return SFEM_OK;
  SFEM_REQUIRE(a->out && a->dmat, "%s: null pointer", who);
  bool needs_wdet = a->source != nullptr;
  for (int l = 0; l < a->num_levels; ++l) {
    SFEM_REQUIRE(a->scalar[l], "%s: null scalar of level %d", who, l);
    needs_wdet = needs_wdet || a->mass_coef[l] != 0.0;
  }
  SFEM_REQUIRE(!needs_wdet || a->wdet,
               "%s: mass terms and a source need `wdet`", who);
  rc = check_geometry(who, a->geo_mode, a->kfac, "kfac", a->geo_elem,
                      a->weights, a->nodes);
  if (rc) return rc;
  int64_t work;
  rc = check_elem_list(who, a->elem_list, a->num_listed, a->num_elements,
                       &work);
  if (rc) return rc;
  if (work == 0) return SFEM_OK;
  return with_real(a->dtype, [&](auto zero) {
    using T = decltype(zero);
    TransportParams<T> tp{};
    tp.geo.kfac = (const T*)a->kfac;
    tp.geo.geo_elem = (const T*)a->geo_elem;
    tp.geo.geo_index = a->geo_index;
    tp.geo.elem_list = a->elem_list;
    tp.geo.dmat_host = (const T*)a->dmat;
    tp.geo.weights_host = (const T*)a->weights;
    tp.geo.nodes_host = (const T*)a->nodes;
    tp.geo.num_elements = work;
    tp.geo.geo_mode = a->geo_mode;
    for (int l = 0; l < a->num_levels; ++l) {
      tp.scalar[l] = (const T*)a->scalar[l];
      tp.velocity[l] = (const T*)a->velocity[l];
      tp.mass_coef[l] = (T)a->mass_coef[l];
      tp.conv_coef[l] = (T)a->conv_coef[l];
    }
    tp.source = (const T*)a->source;
    tp.wdet = (const T*)a->wdet;
    tp.out = (T*)a->out;
    tp.num_levels = a->num_levels;
    return with_dim(a->ndim, [&](auto d) {
      return dispatch_transport_rhs<T, decltype(d)::value>(tp, a->P,
                                                           as_stream(stream));
    });
  });
}

}  // extern "C"
