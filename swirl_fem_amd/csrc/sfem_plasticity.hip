// libsfem_hip: C-ABI entry point of the J2 plasticity residual and tangent.
#include "sfem_plasticity.h"

using namespace sfem;

extern "C" {

int sfem_plasticity_local(const sfem_plasticity_args* a,
                          sfem_stream_t stream) {
  const char* who = "sfem_plasticity_local";
  SFEM_REQUIRE(a, "%s: null args", who);
  SFEM_REQUIRE(a->num_elements >= 0, "%s: bad sizes", who);
  int rc = check_shape(who, a->dtype, a->ndim, "P", a->P, 2, 12);
  if (rc) return rc;
  rc = check_geo_mode(who, a->geo_mode);
  if (rc) return rc;
  if (a->mode != SFEM_PLAST_RESIDUAL && a->mode != SFEM_PLAST_TANGENT) {
    set_error("%s: unknown mode %d", who, (int)a->mode);
    return SFEM_EUNSUPPORTED;
  }
  const bool tangent = a->mode == SFEM_PLAST_TANGENT;
  SFEM_REQUIRE(!tangent || a->lin,
               "%s: the tangent needs the lin state of a residual launch",
               who);
  SFEM_REQUIRE(!tangent || (!a->hist_in && !a->hist_out && !a->stress),
               "%s: the history and the stress belong to the residual mode "
               "only", who);
  SFEM_REQUIRE(!a->hist_in || a->hist_in != a->hist_out,
               "%s: hist_in and hist_out must not alias", who);
  if (a->num_elements == 0) return SFEM_OK;
  SFEM_REQUIRE(a->u && a->out && a->dmat && a->wdet, "%s: null pointer", who);
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
    PlasticityParams<T> pp{};
    fill_elasticity<T>(a, work, &pp.el);
    pp.yield = (const T*)a->yield;
    pp.hard = (const T*)a->hard;
    pp.yield_const = (T)a->yield_const;
    pp.hard_const = (T)a->hard_const;
    pp.hist_in = (const T*)a->hist_in;
    pp.hist_out = (T*)a->hist_out;
    pp.lin = (T*)a->lin;
    pp.stress = (T*)a->stress;
    return with_dim(a->ndim, [&](auto d) {
      return dispatch_plasticity<T, decltype(d)::value>(
          pp, a->P, a->mode, as_stream(stream));
    });
  });
}

}  // extern "C"
