// libsfem_hip: C-ABI entry points of the linear-elasticity operator, of its
// coefficient sensitivities and of stress recovery with its vjp.
#include "sfem_elasticity.h"
#include "sfem_elasticity_sens.h"
#include "sfem_elasticity_stress.h"

using namespace sfem;

// The geometry and launch fields shared by the two stress entry points.
template <typename T, typename Args>
static void stress_geometry(const Args* a, int64_t work, StokesParams<T>* g) {
  g->kfac = (const T*)a->kfac;
  g->geo_elem = (const T*)a->geo_elem;
  g->geo_index = a->geo_index;
  g->elem_list = a->elem_list;
  g->dmat_host = (const T*)a->dmat;
  g->weights_host = (const T*)a->weights;
  g->nodes_host = (const T*)a->nodes;
  g->num_elements = work;
  g->geo_mode = a->geo_mode;
}

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
    ep.geo.kfac = (const T*)a->kfac;
    ep.geo.geo_elem = (const T*)a->geo_elem;
    ep.geo.geo_index = a->geo_index;
    ep.geo.elem_list = a->elem_list;
    ep.geo.dmat_host = (const T*)a->dmat;
    ep.geo.weights_host = (const T*)a->weights;
    ep.geo.nodes_host = (const T*)a->nodes;
    ep.geo.num_elements = work;
    ep.geo.geo_mode = a->geo_mode;
    ep.u = (const T*)a->u;
    ep.out = (T*)a->out;
    ep.wdet = (const T*)a->wdet;
    ep.lam = (const T*)a->lam;
    ep.mu = (const T*)a->mu;
    ep.rho = (const T*)a->rho;
    ep.lam_const = (T)a->lam_const;
    ep.mu_const = (T)a->mu_const;
    ep.rho_const = (T)a->rho_const;
    ep.lambda0 = (T)a->lambda0;
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
    sp.geo.kfac = (const T*)a->kfac;
    sp.geo.geo_elem = (const T*)a->geo_elem;
    sp.geo.geo_index = a->geo_index;
    sp.geo.elem_list = a->elem_list;
    sp.geo.dmat_host = (const T*)a->dmat;
    sp.geo.weights_host = (const T*)a->weights;
    sp.geo.nodes_host = (const T*)a->nodes;
    sp.geo.num_elements = work;
    sp.geo.geo_mode = a->geo_mode;
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
    stress_geometry<T>(a, work, &sp.geo);
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
    stress_geometry<T>(a, work, &sp.geo);
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
