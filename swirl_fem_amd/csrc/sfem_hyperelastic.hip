// libsfem_hip: C-ABI entry point of the neo-Hookean residual and tangent.
#include "sfem_hyperelastic.h"

using namespace sfem;

extern "C" {

int sfem_hyperelastic_local(const sfem_hyperelastic_args* a,
                            sfem_stream_t stream) {
  const char* who = "sfem_hyperelastic_local";
  SFEM_REQUIRE(a, "%s: null args", who);
  SFEM_REQUIRE(a->num_elements >= 0, "%s: bad sizes", who);
  int rc = check_shape(who, a->dtype, a->ndim, "P", a->P, 2, 12);
  if (rc) return rc;
  rc = check_geo_mode(who, a->geo_mode);
  if (rc) return rc;
  if (a->mode != SFEM_HYPER_RESIDUAL && a->mode != SFEM_HYPER_TANGENT) {
    set_error("%s: unknown mode %d", who, (int)a->mode);
    return SFEM_EUNSUPPORTED;
  }
  SFEM_REQUIRE(a->mode != SFEM_HYPER_TANGENT || a->state,
               "%s: the tangent needs the state of a residual launch", who);
  SFEM_REQUIRE(a->mode != SFEM_HYPER_TANGENT || !a->psi,
               "%s: psi is an output of the residual mode only", who);
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
    HyperelasticParams<T> hp{};
    fill_elasticity<T>(a, work, &hp.el);
    hp.state = (T*)a->state;
    hp.psi = (T*)a->psi;
    return with_dim(a->ndim, [&](auto d) {
      return dispatch_hyperelastic<T, decltype(d)::value>(
          hp, a->P, a->mode, as_stream(stream));
    });
  });
}

}  // extern "C"
