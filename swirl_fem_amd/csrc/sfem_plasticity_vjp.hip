// libsfem_hip: C-ABI entry point of the plasticity VJP (the radial return's
// vector-Jacobian product, displacement and state modes).
#include "sfem_plasticity_vjp.h"

using namespace sfem;

extern "C" {

int sfem_plasticity_vjp(const sfem_plasticity_vjp_args* a,
                        sfem_stream_t stream) {
  const char* who = "sfem_plasticity_vjp";
  SFEM_REQUIRE(a, "%s: null args", who);
  SFEM_REQUIRE(a->num_elements >= 0, "%s: bad sizes", who);
  int rc = check_shape(who, a->dtype, a->ndim, "P", a->P, 2, 12);
  if (rc) return rc;
  rc = check_geo_mode(who, a->geo_mode);
  if (rc) return rc;
  if (a->mode != SFEM_PLAST_VJP_DISPLACEMENT &&
      a->mode != SFEM_PLAST_VJP_STATE) {
    set_error("%s: unknown mode %d", who, (int)a->mode);
    return SFEM_EUNSUPPORTED;
  }
  const bool state = a->mode == SFEM_PLAST_VJP_STATE;
  const bool any_state_out = a->hbar_prev || a->dlam || a->dmu || a->dyield ||
                             a->dhard || a->drho;
  SFEM_REQUIRE(state || (!a->w && !any_state_out),
               "%s: w, hbar_prev and the coefficient derivatives belong to "
               "the state mode only", who);
  SFEM_REQUIRE(!state || !a->out,
               "%s: out belongs to the displacement mode only", who);
  SFEM_REQUIRE(!state || any_state_out, "%s: the state mode needs an output",
               who);
  SFEM_REQUIRE(!a->hbar_prev || (a->hbar_prev != a->hist_in &&
                                 a->hbar_prev != a->hbar),
               "%s: hbar_prev must alias neither hist_in nor hbar", who);
  if (a->num_elements == 0) return SFEM_OK;
  SFEM_REQUIRE(a->u && a->dmat && a->wdet, "%s: null pointer", who);
  SFEM_REQUIRE(state ? a->w != nullptr : (a->hbar && a->out),
               "%s: null pointer", who);
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
    PlasticityVjpParams<T> pp{};
    fill_geometry<T>(a, work, &pp.el.geo);
    pp.el.u = (const T*)a->u;
    pp.el.out = (T*)a->out;
    pp.el.wdet = (const T*)a->wdet;
    pp.el.lam = (const T*)a->lam;
    pp.el.mu = (const T*)a->mu;
    pp.el.lam_const = (T)a->lam_const;
    pp.el.mu_const = (T)a->mu_const;
    pp.el.lambda0 = T(0);   // the output stage adds no mass term
    pp.w = (const T*)a->w;
    pp.yield = (const T*)a->yield;
    pp.hard = (const T*)a->hard;
    pp.yield_const = (T)a->yield_const;
    pp.hard_const = (T)a->hard_const;
    pp.hist_in = (const T*)a->hist_in;
    pp.hbar = (const T*)a->hbar;
    pp.hbar_prev = (T*)a->hbar_prev;
    pp.dlam = (T*)a->dlam;
    pp.dmu = (T*)a->dmu;
    pp.dyield = (T*)a->dyield;
    pp.dhard = (T*)a->dhard;
    pp.drho = (T*)a->drho;
    pp.lambda0 = (T)a->lambda0;
    return with_dim(a->ndim, [&](auto d) {
      return dispatch_plasticity_vjp<T, decltype(d)::value>(
          pp, a->P, a->mode, as_stream(stream));
    });
  });
}

}  // extern "C"
