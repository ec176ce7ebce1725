// libsfem_hip: C-ABI entry points of the linear-elasticity operator, of its
// coefficient sensitivities and of stress recovery with its vjp.
#include "sfem_elasticity.h"
#include "sfem_elasticity_sens.h"
#include "sfem_elasticity_stress.h"

using namespace sfem;

extern "C" {

int sfem_elasticity_local(const sfem_elasticity_args* a, sfem_stream_t stream) {
  const char* who = "sfem_elasticity_local";
  SFEM_REQUIRE(a, "%s: null args", who);
  SFEM_REQUIRE(a->num_elements >= 0, "%s: bad sizes", who);
  int rc = check_shape(who, a->dtype, a->ndim, "P", a->P, 2, 12);
  if (rc) return rc;
  rc = check_geo_mode(who, a->geo_mode);
  if (rc) return rc;
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
    ElasticityParams<T> ep{};
    fill_elasticity<T>(a, work, &ep);
    return with_dim(a->ndim, [&](auto d) {
      return dispatch_elasticity<T, decltype(d)::value>(ep, a->P,
                                                        as_stream(stream));
    });
  });
}

int sfem_elasticity_sens(const sfem_elasticity_sens_args* a,
                         sfem_stream_t stream) {
  const char* who = "sfem_elasticity_sens";
  SFEM_REQUIRE(a, "%s: null args", who);
  SFEM_REQUIRE(a->num_elements >= 0, "%s: bad sizes", who);
  int rc = check_shape(who, a->dtype, a->ndim, "P", a->P, 2, 12);
  if (rc) return rc;
  rc = check_geo_mode(who, a->geo_mode);
  if (rc) return rc;
  SFEM_REQUIRE(a->dlam || a->dmu || a->drho, "%s: no output asked for", who);
  if (a->num_elements == 0) return SFEM_OK;
  SFEM_REQUIRE(a->u && a->v && a->dmat && a->wdet, "%s: null pointer", who);
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
    ElasticitySensParams<T> sp{};
    fill_geometry<T>(a, work, &sp.geo);
    sp.u = (const T*)a->u;
    sp.v = (const T*)a->v;
    sp.wdet = (const T*)a->wdet;
    sp.dlam = (T*)a->dlam;
    sp.dmu = (T*)a->dmu;
    sp.drho = (T*)a->drho;
    sp.lambda0 = (T)a->lambda0;
    return with_dim(a->ndim, [&](auto d) {
      return dispatch_elasticity_sens<T, decltype(d)::value>(
          sp, a->P, as_stream(stream));
    });
  });
}

int sfem_elasticity_stress(const sfem_elasticity_stress_args* a,
                           sfem_stream_t stream) {
  const char* who = "sfem_elasticity_stress";
  SFEM_REQUIRE(a, "%s: null args", who);
  SFEM_REQUIRE(a->num_elements >= 0, "%s: bad sizes", who);
  int rc = check_shape(who, a->dtype, a->ndim, "P", a->P, 2, 12);
  if (rc) return rc;
  rc = check_geo_mode(who, a->geo_mode);
  if (rc) return rc;
  SFEM_REQUIRE(a->sigma || a->vm, "%s: no output asked for", who);
  if (a->num_elements == 0) return SFEM_OK;
  SFEM_REQUIRE(a->u && a->dmat && a->wdet, "%s: null pointer", who);
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
    ElasticityStressParams<T> sp{};
    fill_geometry<T>(a, work, &sp.geo);
    sp.u = (const T*)a->u;
    sp.wdet = (const T*)a->wdet;
    sp.lam = (const T*)a->lam;
    sp.mu = (const T*)a->mu;
    sp.sigma = (T*)a->sigma;
    sp.vm = (T*)a->vm;
    sp.lam_const = (T)a->lam_const;
    sp.mu_const = (T)a->mu_const;
    sp.plane_stress = a->plane_stress != 0;
    return with_dim(a->ndim, [&](auto d) {
      return dispatch_elasticity_stress<T, decltype(d)::value>(
          sp, a->P, as_stream(stream));
    });
  });
}

int sfem_elasticity_stress_vjp(const sfem_elasticity_stress_vjp_args* a,
                               sfem_stream_t stream) {
  const char* who = "sfem_elasticity_stress_vjp";
  SFEM_REQUIRE(a, "%s: null args", who);
  SFEM_REQUIRE(a->num_elements >= 0, "%s: bad sizes", who);
  int rc = check_shape(who, a->dtype, a->ndim, "P", a->P, 2, 12);
  if (rc) return rc;
  rc = check_geo_mode(who, a->geo_mode);
  if (rc) return rc;
  SFEM_REQUIRE(a->ubar || a->dlam || a->dmu, "%s: no output asked for", who);
  if (a->num_elements == 0) return SFEM_OK;
  SFEM_REQUIRE(a->sbar && a->dmat && a->wdet, "%s: null pointer", who);
  SFEM_REQUIRE(a->u || !(a->dlam || a->dmu),
               "%s: dlam and dmu need the displacement u", who);
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
    ElasticityStressVjpParams<T> sp{};
    fill_geometry<T>(a, work, &sp.geo);
    sp.sbar = (const T*)a->sbar;
    sp.u = (const T*)a->u;
    sp.wdet = (const T*)a->wdet;
    sp.lam = (const T*)a->lam;
    sp.mu = (const T*)a->mu;
    sp.ubar = (T*)a->ubar;
    sp.dlam = (T*)a->dlam;
    sp.dmu = (T*)a->dmu;
    sp.lam_const = (T)a->lam_const;
    sp.mu_const = (T)a->mu_const;
    sp.plane_stress = a->plane_stress != 0;
    return with_dim(a->ndim, [&](auto d) {
      return dispatch_elasticity_stress_vjp<T, decltype(d)::value>(
          sp, a->P, as_stream(stream));
    });
  });
}

}  // extern "C"
