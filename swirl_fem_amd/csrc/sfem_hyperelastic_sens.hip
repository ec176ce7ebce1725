// libsfem_hip: C-ABI entry point of the neo-Hookean coefficient sensitivities.
#include "sfem_hyperelastic_sens.h"

using namespace sfem;

extern "C" {

int sfem_hyperelastic_sens(const sfem_hyperelastic_sens_args* a,
                           sfem_stream_t stream) {
  const char* who = "sfem_hyperelastic_sens";
  SFEM_REQUIRE(a, "%s: null args", who);
  SFEM_REQUIRE(a->num_elements >= 0, "%s: bad sizes", who);
  int rc = check_shape(who, a->dtype, a->ndim, "P", a->P, 2, 12);
  if (rc) return rc;
  rc = check_geo_mode(who, a->geo_mode);
  if (rc) return rc;
  SFEM_REQUIRE(a->dlam || a->dmu || a->drho, "%s: no output asked for", who);
  SFEM_REQUIRE(!a->drho || a->u, "%s: drho needs the displacement u", who);
  if (a->num_elements == 0) return SFEM_OK;
  SFEM_REQUIRE(a->v && a->state && a->dmat && a->wdet, "%s: null pointer",
               who);
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
    HyperelasticSensParams<T> sp{};
    fill_geometry<T>(a, work, &sp.geo);
    sp.v = (const T*)a->v;
    sp.state = (const T*)a->state;
    sp.u = (const T*)a->u;
    sp.wdet = (const T*)a->wdet;
    sp.dlam = (T*)a->dlam;
    sp.dmu = (T*)a->dmu;
    sp.drho = (T*)a->drho;
    sp.lambda0 = (T)a->lambda0;
    return with_dim(a->ndim, [&](auto d) {
      return dispatch_hyperelastic_sens<T, decltype(d)::value>(
          sp, a->P, as_stream(stream));
    });
  });
}

}  // extern "C"
