/*
 * sfem.h -- C-ABI of libsfem_hip.so: MI355X (gfx950) kernels for the
 * spectral-element operator-apply + gather-scatter hot path of swirl_fem.
 *
 * The reference (google-research/swirl-fem) is pure Python/JAX and has no FFI
 * layer; its boundary for this path is the Python object API.  Each entry point
 * below names the reference call site(s) it replaces (paths relative to the
 * reference root).  swirl_fem_amd/_ops.py binds them with ctypes; a maintainer
 * of the reference would bind them the same way.
 *
 * Conventions
 *   - all pointers are DEVICE pointers owned by the caller unless marked host;
 *     nothing is allocated or freed inside a call, no call synchronises;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the
 *     legacy default stream);
 *   - `dtype` is SFEM_F32 or SFEM_F64 and applies to every `void*` real array
 *     of the call; index arrays are int32 with -1 (SFEM_SENTINEL) = "missing";
 *   - element-local arrays are (E, n) with n = P^ndim and lexicographic node
 *     order inside an element, axis 0 slowest (reference core/mesh.py:39-46);
 *     quadrature arrays are (E, Q), Q = q^ndim, same ordering;
 *   - vector fields carry their `ncomp` components innermost: (N, ncomp),
 *     (E, n, ncomp), (E, Q, ncomp), gradients (E, Q, ndim, ncomp) with
 *     [j][k] = d u_k / d x_j (reference core/fespace.py:221-225);
 *   - return value: SFEM_OK (0) or a negative error; sfem_last_error() gives a
 *     thread-local message.  Nothing throws across the ABI.
 */
#ifndef SFEM_H_
#define SFEM_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFEM_ABI_VERSION 10

enum { SFEM_F32 = 0, SFEM_F64 = 1 };
enum {
  SFEM_OK = 0,
  SFEM_EINVAL = -1,       /* bad argument (null pointer, size, dtype, ...)   */
  SFEM_EHIP = -2,         /* a HIP runtime call failed                        */
  SFEM_EUNSUPPORTED = -3  /* shape outside the compiled template range        */
};
#define SFEM_SENTINEL (-1)
#define SFEM_MAX_P 16     /* nodes / quadrature points per direction          */

/* Encoded element index used by the fused operators (sfem_encode_elements):
 * low 30 bits node id (all ones = padding slot: reads 0, writes nothing),
 * two flag bits on top.                                                      */
#define SFEM_IDX_MASK 0x3FFFFFFF
#define SFEM_IDX_PAD 0x3FFFFFFF
#define SFEM_IDX_DIRICHLET 0x80000000u /* row zeroed by the interior mask     */
#define SFEM_IDX_SHARED 0x40000000u /* node belongs to >1 slot: atomic add   */

typedef void* sfem_stream_t;

int sfem_abi_version(void);
const char* sfem_last_error(void);

/* ---------------------------------------------------------------- gather ---
 * out[i] = indices[i] == -1 ? fill : u[indices[i]]          i in [0, count)
 * Replaces gather_scatter.gather (core/gather_scatter.py:121-127) /
 * Mesh.gather (core/mesh.py:155-160).                                        */
int sfem_gather(const void* u, const int32_t* indices, void* out,
                int64_t count, double fill, int dtype, sfem_stream_t stream);

/* out[i, k] = indices[i] == -1 ? 0 : x[indices[i], k]   k in [0, ncomp)
 * Replaces the vmapped gathers Mesh.element_coords (core/mesh.py:170-172) and
 * StokesVelocity.gather (navier_stokes/navier_stokes.py:210-211).            */
int sfem_gather_rows(const void* x, const int32_t* indices, void* out,
                     int64_t count, int ncomp, int dtype, sfem_stream_t stream);

/* --------------------------------------------------------------- scatter ---
 * out[indices[i], k] += u_local[i, k]; entries with index -1 are skipped.
 * `out` (num_nodes, ncomp) is zero-filled by the call first.  Accumulation
 * uses HBM float atomics (order not reproducible).
 * Replaces gather_scatter.scatter (core/gather_scatter.py:130-133) /
 * Mesh.scatter (core/mesh.py:165-168).                                       */
int sfem_scatter_add(const void* u_local, const int32_t* indices, void* out,
                     int64_t count, int64_t num_nodes, int ncomp, int dtype,
                     sfem_stream_t stream);

/* Deterministic direct-stiffness sum through the inverse map (CSR by node):
 * out[v, k] = sum_{s in [offsets[v], offsets[v+1])} u_local[slots[s], k],
 * summed in slot order, so results are bitwise reproducible.                 */
int sfem_scatter_csr(const void* u_local, const int64_t* offsets,
                     const int32_t* slots, void* out, int64_t num_nodes,
                     int ncomp, int dtype, sfem_stream_t stream);

/* -------------------------------------------------------------- exchange ---
 * Unpartitioned QQ^T (periodic images), core/gather_scatter.py:189-261 with
 * axis_name=None:  out = u;  sums[unique[i]] += u[gidx[i]];
 * out[gidx[i]] = sums[unique[i]].   `sums` is caller workspace of num_unique
 * reals (zeroed by the call).  gidx entries of -1 are skipped.               */
int sfem_exchange_local(const void* u, void* out, const int32_t* gidx,
                        const int32_t* unique, int64_t count,
                        int64_t num_nodes, void* sums, int64_t num_unique,
                        int ncomp, int dtype, sfem_stream_t stream);

/* The same QQ^T in place and in ONE launch, from the classes themselves
 * (CSR: class c holds the nodes members[offsets[c] .. offsets[c+1])):
 * every member receives the sum over its class, summed in member order
 * (reproducible, no workspace, no atomics).  `u[k * node_stride +
 * c * comp_stride]` addresses node k, component c: (N, nc) row-major is
 * (nc, 1), component-major strips are (1, N).                               */
int sfem_exchange_classes(void* u, const int32_t* members,
                          const int32_t* offsets, int64_t num_classes,
                          int ncomp, int64_t node_stride, int64_t comp_stride,
                          int dtype, sfem_stream_t stream);

/* Clears `nstrips` strips of `strip_len` reals, `strip_stride` reals apart:
 * the shared-node range of every component ahead of an atomically assembled
 * apply (one launch for short strips, the runtime's fill for long ones).     */
int sfem_zero_strips(void* base, int64_t strip_len, int64_t strip_stride,
                     int nstrips, int dtype, sfem_stream_t stream);

/* Partitioned QQ^T, the pack / unpack halves around the RCCL neighbour
 * exchange that replaces lax.psum (core/gather_scatter.py:247-248):
 *   pack:       buf[i, k] = idx[i] == -1 ? 0 : u[idx[i], k]
 *   unpack_add: u[idx[i], k] += buf[i, k]  (idx unique within one call)      */
int sfem_pack(const void* u, const int32_t* idx, void* buf, int64_t count,
              int ncomp, int dtype, sfem_stream_t stream);
int sfem_unpack_add(const void* buf, const int32_t* idx, void* u,
                    int64_t count, int ncomp, int dtype, sfem_stream_t stream);

/* Single-launch forms for a whole partition interface: `u` is an (N, ncomp)
 * view with element strides (node_stride, comp_stride) -- row-major or
 * component-major -- and `idx` is the concatenation of all per-neighbour lists,
 * so a node may occur several times: the unpack adds atomically.             */
int sfem_pack_strided(const void* u, const int32_t* idx, void* buf,
                      int64_t count, int ncomp, int64_t node_stride,
                      int64_t comp_stride, int dtype, sfem_stream_t stream);
int sfem_unpack_add_atomic(const void* buf, const int32_t* idx, void* u,
                           int64_t count, int ncomp, int64_t node_stride,
                           int64_t comp_stride, int dtype,
                           sfem_stream_t stream);

/* ------------------------------------------------------ geometric factors ---
 * From element node coordinates (E, n, ndim) computes, per quadrature point,
 *   jac[i][j]  = d x_j / d xi_i      (core/fespace.py:338, via I1/G1 factors)
 *   invjac     = jac^-1  (E, Q, ndim, ndim)   (core/fespace.py:345)
 *   jacdet     = det jac (E, Q), signed       (core/fespace.py:346)
 *   quad_coords (E, Q, ndim) or NULL          (core/fespace.py:332-333)
 * interp1 (q, P) = 1D interpolation matrix, grad1 (q, P) = interp1 @ D1, both
 * row-major device arrays of `dtype`.                                        */
int sfem_geom_factors(const void* elem_coords, const void* interp1,
                      const void* grad1, int64_t num_elements, int ndim, int P,
                      int q, void* invjac, void* jacdet, void* quad_coords,
                      int dtype, sfem_stream_t stream);

/* ------------------------------------------------------- basis evaluation ---
 * Sum-factorised evaluation of nodal fields at quadrature points
 * (core/interpolation.py:254-263, :288-292 vmapped by core/fespace.py:178-225):
 *   val  (E, Q, ncomp)        = (I x .. x I) u                  or NULL
 *   grad (E, Q, ndim, ncomp)  = invjac . reference gradient     or NULL
 * invjac == NULL returns the reference-space gradient.  `collocated` != 0
 * skips the interpolation for `val` exactly like interpolation.py:257-258.   */
int sfem_basis_eval(const void* u_local, const void* interp1,
                    const void* grad1, const void* invjac, void* val,
                    void* grad, int64_t num_elements, int ndim, int P, int q,
                    int ncomp, int collocated, int dtype, sfem_stream_t stream);

/* Exact transpose of sfem_basis_eval composed with quadrature: the operator
 * action produced by jax.linear_transpose in FiniteElementSpace.local_covector
 * (core/fespace.py:458-471):
 *   out[e, n, k] = sum_q wdet[e,q] ( val-basis^T c0 + grad-basis^T invjac^T c1 )
 * c0 (E, Q, ncomp) or NULL; c1 (E, Q, ndim, ncomp) or NULL; wdet (E, Q) =
 * jacdet * quadrature weight.                                                */
int sfem_basis_eval_t(const void* c0, const void* c1, const void* interp1,
                      const void* grad1, const void* invjac, const void* wdet,
                      void* out, int64_t num_elements, int ndim, int P, int q,
                      int ncomp, int collocated, int dtype,
                      sfem_stream_t stream);

/* --------------------------------------------------- fused Helmholtz apply ---
 * Collocated (quadrature points == GLL nodes) operator
 *     out = mask * scatter( lambda0 * B_local(g) + lambda1 * A_local(g) ),
 *     g = gather(u)
 * i.e. the mass form u.v, the stiffness form grad u : grad v and their
 * combination H = (beta_k/dt) B + mu A in one pass over the elements:
 * examples/poisson.py:141-154, navier_stokes.py:220-236, :295-307, :431.
 *
 * The per-point symmetric factors G = w detJ (J^-1 J^-T) and W = w detJ come
 * from one of three sources (`geo_mode`):
 *   SFEM_GEO_POINT        stored: ndim(ndim+1)/2 + 1 reals per point in `geo`
 *                         (written by sfem_helmholtz_setup).  Element e uses
 *                         slot geo_index[e] (or e when geo_index is NULL).
 *   SFEM_GEO_MULTILINEAR  computed in registers from the element's multilinear
 *                         map (every refine_premesh mesh): `geo_elem` (E, 24),
 *                         written by sfem_helmholtz_setup_multilinear, plus the
 *                         1D quadrature weights and node values (host arrays).
 *   SFEM_GEO_AFFINE       same data, constant Jacobian: G is a per-element
 *                         constant times the tensor quadrature weight.
 * `elem_list` (device int32, num_listed entries) restricts a launch to some
 * elements, so a mesh mixing the kinds is applied by one call per kind.       */
/* Variable-coefficient modes (kappa / sigma / coef_mode of
 * sfem_helmholtz_args and sfem_diag_args): off, one value per element, one
 * value per quadrature point.                                               */
enum { SFEM_COEF_NONE = 0, SFEM_COEF_ELEM = 1, SFEM_COEF_POINT = 2 };
enum { SFEM_GEO_POINT = 0, SFEM_GEO_AFFINE = 1, SFEM_GEO_MULTILINEAR = 3,
       SFEM_GEO_BOX = 5 /* affine with diagonal J^-1 J^-T (Cartesian boxes):  */
                        /* facet-table applies only.  Helmholtz: needs        */
                        /* `geo_const`; Stokes: `geo_elem` whose Jacobian is  */
                        /* itself diagonal (x_c depends on reference axis c)  */ };

int sfem_helmholtz_setup(const void* invjac, const void* jacdet,
                         const void* weights_nd /* (Q,) */, void* geo,
                         int64_t num_elements, int ndim, int Q, int dtype,
                         sfem_stream_t stream);
/* elem_coords (E, P^ndim, ndim) -> geo_elem (E, 24)                           */
int sfem_helmholtz_setup_multilinear(const void* elem_coords, void* geo_elem,
                                     int64_t num_elements, int ndim, int P,
                                     int dtype, sfem_stream_t stream);

/* enc[i] = node id | flags.  dirichlet (num_nodes,) uint8 or NULL.  The SHARED
 * flag (accumulate instead of store) is set for slots whose node has
 * multiplicity[node] > 1 (multiplicity (num_nodes,) int32 = number of slots
 * referencing the node), or, when slot_shared (count,) uint8 is given, for the
 * slots it marks (coloured assembly: every slot but the first toucher).       */
int sfem_encode_elements(const int32_t* elements, const uint8_t* dirichlet,
                         const int32_t* multiplicity,
                         const uint8_t* slot_shared, int32_t* enc,
                         int64_t count, sfem_stream_t stream);

typedef struct sfem_helmholtz_args {
  const void* u;          /* (N, ncomp); sfem_helmholtz_local: (E, n, ncomp)  */
  void* out;              /* same shape as u                                  */
  const int32_t* enc;     /* (E, n) encoded indices (apply only)              */
  const void* geo;        /* per-point factors or NULL                        */
  const void* geo_elem;   /* (E, 24) or NULL                                  */
  const int32_t* geo_index; /* (E,) slot of element in `geo`, or NULL         */
  const int32_t* elem_list; /* (num_listed,) element ids, or NULL = all       */
  const void* dmat;       /* HOST: (P, P) 1D differentiation matrix           */
  const void* weights;    /* HOST: (P,) 1D quadrature weights, or NULL        */
  const void* nodes;      /* HOST: (P,) 1D node values, or NULL               */
  int64_t num_elements;   /* E                                                */
  int64_t num_listed;     /* length of elem_list                              */
  int64_t num_nodes;      /* N (apply only)                                   */
  int64_t zero_begin;     /* apply: out[zero_begin:zero_end) is cleared first;*/
  int64_t zero_end;       /*   must cover every SHARED / unreferenced node    */
  int32_t ndim;
  int32_t P;
  int32_t ncomp;
  int32_t dtype;          /* of every real array incl. the host ones          */
  int32_t geo_mode;       /* SFEM_GEO_*                                       */
  int32_t colored;        /* apply: != 0 if the listed elements share no node */
                          /*   with each other (one colour class per launch,  */
                          /*   launches stream-ordered): SHARED slots then    */
                          /*   read-modify-write `out` without atomics, the   */
                          /*   sum order is fixed and the result bitwise      */
                          /*   reproducible                                   */
  double lambda0;         /* mass coefficient                                 */
  double lambda1;         /* stiffness coefficient                            */
  int64_t node_stride;    /* layout of u / out in elements: entry (node, k) at*/
  int64_t comp_stride;    /*   node*node_stride + k*comp_stride.  0, 0 = the  */
                          /*   default (N, ncomp) row-major layout; (1, N) =  */
                          /*   component-major storage seen as an (N, ncomp)  */
                          /*   view, which keeps every component contiguous   */
  double* dot_out;        /* apply: NULL, or SFEM_DOT_SLOTS device doubles    */
                          /*   that accumulate partial sums of u . out (the   */
                          /*   p.Ap of CG, cg.py:78, for free in the scatter) */
  const uint16_t* shared_order; /* apply: NULL, or (E, shared_stride): the    */
  int32_t shared_stride;  /*   slots of each element's SHARED, non-Dirichlet  */
                          /*   nodes in ascending node order, padded with     */
                          /*   0xFFFF.  The atomics are then issued in that   */
                          /*   order (values change lanes through LDS): twice */
                          /*   the lanes per 64-byte line, same sums          */
  /* apply, 3D, P = 4..8: cluster assembly (NULL / 0 = off).  One workgroup   */
  /* takes the <= cluster_size elements of a cluster, sums the nodes they     */
  /* share in LDS and touches HBM once per node: plain stores for nodes held  */
  /* by this cluster only, atomics for the cluster surface.                   */
  const int32_t* cluster_elems;   /* (num_clusters, cluster_size) element     */
                                  /*   ids, -1 = empty place                  */
  const int32_t* cluster_offsets; /* (num_clusters + 1,) start of each        */
                                  /*   cluster's table in cluster_nodes       */
  const uint32_t* cluster_nodes;  /* tables, ascending node id per cluster:   */
                                  /*   id | SFEM_IDX_DIRICHLET | SFEM_IDX_    */
                                  /*   SHARED (= also held by an element      */
                                  /*   outside the cluster); at most          */
                                  /*   max_shared entries per cluster (from   */
                                  /*   sfem_helmholtz_cluster_limits; longer  */
                                  /*   tables are truncated by the kernel)    */
  int64_t num_clusters;           /* `enc` must then be in cluster form: a    */
                                  /*   slot whose node is in the table holds  */
                                  /*   SFEM_IDX_SHARED | DIRICHLET bit | its  */
                                  /*   POSITION in the table, other slots     */
                                  /*   id | DIRICHLET bit; elem_list unused   */
  /* apply, 3D, P = 6..12: compact connectivity (NULL = off, `enc` is then    */
  /* required).  (E, 27, 4) int32 from sfem_facet_table_build; every listed   */
  /* element must have qualified there.  `enc`, `shared_order` are not read.  */
  /* Needs node_stride = 1 (scalar or component-major fields).                */
  const int32_t* facet_table;
  const void* geo_const;  /* (E, 8) from sfem_helmholtz_setup_affine: needed  */
                          /*   with facet_table for SFEM_GEO_AFFINE / _BOX    */
  /* facet_table applies of scalar or component-major (node_stride = 1)       */
  /* fields, the latter one launch per component: the elements as chains      */
  /* (NULL / 0 = one workgroup per listed element).  Segment s is the elements */
  /* chain_elems[chain_offsets[s] .. chain_offsets[s+1]); inside a segment    */
  /* the face a = P-1 of every element IS the face a = 0 of the next, node    */
  /* for node: elements[e][(P-1) P^2 + t] == elements[next][t], t < P^2.      */
  /* One wave walks a segment and carries that face in registers (gathered    */
  /* once, summed before it is written: its interior needs no atomic).  The   */
  /* segments must hold every element of the launch exactly once; elem_list   */
  /* is not read.                                                             */
  const int32_t* chain_offsets;   /* (num_chains + 1,)                        */
  const int32_t* chain_elems;     /* (chain_offsets[num_chains],)             */
  int64_t num_chains;
  /* apply with facet_table, scalar fields: layered assembly (0 = off).  `out` */
  /* is then an extended vector of layered_extent reals (see                   */
  /* sfem_cg_update_r_layered) and facet_table is in its LAYERED form          */
  /*   { id0 | flags,  position in `out` | SFEM_IDX_DIRICHLET,  sa,            */
  /*     (si & 0xffff) | (sj << 16) }                                          */
  /* where the position is layer base + id0 of the layer this (element, facet) */
  /* writes: every writer of a facet has a layer of its own (in a chain        */
  /* segment the element that hands a face on does not write it, its successor */
  /* writes the sum).  Slots no element writes must hold zero; the kernel      */
  /* issues plain stores only and clears nothing (zero_begin/zero_end unused). */
  int64_t layered_extent;
  /* with layered_extent and dot_out: 0 = dot_out is SFEM_DOT_SLOTS atomically  */
  /* accumulated slots as above; > 0 = dot_out holds dot_slots doubles, at      */
  /* least one per wave of the launch (workgroups x ceil(P^2 / 64)); wave w     */
  /* STORES its partial sum of u . out at dot_out[w] -- nothing to clear, and   */
  /* the sum over the slots in index order (sfem_cg_scalars_n) is bitwise       */
  /* reproducible                                                               */
  int64_t dot_slots;
  /* Advective term (NULL = off): the operator becomes                        */
  /*   lambda0 B_c + lambda1 A_k + C_b,                                       */
  /*   C_b[i,j] = sum_q W_q phi_i(q) b_q . grad phi_j(q),                     */
  /* not scaled by either lambda.  `beta` holds the velocity with the         */
  /* geometry folded in, beta[e,q,d] = W[e,q] sum_j b[e,q,j] invjac[e,q,j,d]  */
  /* (d = reference direction), at the element's points in slot order         */
  /* (lexicographic, axis 0 slowest), indexed by element id, in the dtype of  */
  /* the field.  Honoured by sfem_helmholtz_apply on index rows and by        */
  /* sfem_helmholtz_local; every geo_mode but SFEM_GEO_BOX.  kappa / sigma    */
  /* (below) then come per point only (SFEM_COEF_POINT, or off), folded into  */
  /* the stored factors for SFEM_GEO_POINT.  Vector fields, cluster,          */
  /* facet, chain, layered and sorted assembly, dot_out and SFEM_COEF_ELEM    */
  /* return SFEM_EUNSUPPORTED.                                                */
  /* The field sits in front of the coefficient block, which stays the tail   */
  /* of the struct; callers that zero the struct keep the operator without    */
  /* the term.                                                                */
  const void* beta;       /* (E, n, ndim) or NULL = off                       */
  /* 0: C_b as above.  != 0: its transpose,                                   */
  /*   (C_b^T v)_i = sum_q (sum_d beta[q,d] D_d phi_i(q)) v(q),               */
  /* so that the call applies (lambda0 B_c + lambda1 A_k + C_b)^T (B_c and    */
  /* A_k are symmetric).  Honoured wherever `beta` is; ignored without        */
  /* `beta`, when the operator is symmetric.  ABI version 10.                 */
  int32_t adv_transpose;
  /* Variable coefficients (NULL / 0 = off): the operator becomes             */
  /*   lambda0 B_c + lambda1 A_k,  B_c[i,j] = sum_q c_q W_q phi_i phi_j,      */
  /*   A_k[i,j] = sum_q k_q grad phi_i . G_q grad phi_j.                      */
  /* coef_mode SFEM_COEF_ELEM: kappa / sigma hold one value per element (E,); */
  /* SFEM_COEF_POINT: (E, n) values at the element's points in slot order     */
  /* (lexicographic, axis 0 slowest).  Indexed by element id, in the dtype of */
  /* the field; a NULL array stands for 1, but not both.  Scalar fields       */
  /* (ncomp = 1) on index rows only (no cluster, facet, layered or sorted     */
  /* assembly), SFEM_GEO_AFFINE / _MULTILINEAR elements: curved elements take */
  /* the coefficients folded into their stored factors (k G, c W).            */
  const void* kappa;      /* diffusivity k (> 0)                              */
  const void* sigma;      /* reaction coefficient c (>= 0)                    */
  int32_t coef_mode;      /* SFEM_COEF_*                                      */
} sfem_helmholtz_args;

/* Compact connectivity of refiner-numbered meshes (reference numbering:
 * core/mesh_refiner.py:143-251: the interior nodes of every premesh facet are
 * one contiguous block, read through a cube orientation).  For element e and
 * facet f = 9 cls(a) + 3 cls(i) + cls(j), cls = 0 (index 0) / 1 (interior) /
 * 2 (index P-1), table[e][f] = { id0 | SFEM_IDX_* flags, sa, si, sj } with
 *   elements[e][a, i, j] = id0 + sa (a - 1) + si (i - 1) + sj (j - 1)
 * for every node of the facet (strides of fixed directions are 0).  ok[e] = 1
 * iff all P^3 ids of the element, the Dirichlet flag and the SHARED flag
 * (multiplicity > 1) of every node agree with its table; other elements must
 * be applied through `enc`.  elements (E, P^3), ndim = 3, 2 <= P <= 12.       */
int sfem_facet_table_build(const int32_t* elements, const uint8_t* dirichlet,
                           const int32_t* multiplicity, int32_t* table,
                           uint8_t* ok, int64_t num_elements,
                           int64_t num_nodes, int P, sfem_stream_t stream);

/* Self-test of an assumption of the facet / chain kernels: they read their
 * by-value matrix argument through the kernarg segment at the offset the
 * current code-object ABI places it.  Launches probe kernels that OR a
 * non-zero value into *bad (a zeroed device int32) if the bytes seen there
 * differ from the argument.  The Python layer runs it once per process before
 * the first facet launch and refuses to continue on a mismatch.              */
int sfem_kernarg_selftest(int32_t* bad, sfem_stream_t stream);

/* 1 if a chain launch (chain_offsets set) on a field of `field_bytes` bytes
 * touches the next element's nodes one compute phase before it gathers them,
 * else 0.  Decided per launch from the environment variable SFEM_CHAIN_TOUCH:
 * unset or "0" never (the default), "1" always, "auto" from 256 MiB on
 * (fields that do not stay in the caches between two kernels).  The results
 * do not depend on it.                                                       */
int sfem_chain_touch_enabled(int64_t field_bytes);

/* geo_elem (E, 24) of affine elements -> geo_const (E, 8) =
 * { G00, G01, G02, G11, G12, G22, detJ, box } with G = detJ J^-1 J^-T (no
 * quadrature weight) and box = 1 when |G01|, |G02|, |G12| <= box_tol *
 * max(G00, G11, G22) (the element may then be applied as SFEM_GEO_BOX).      */
int sfem_helmholtz_setup_affine(const void* geo_elem, void* geo_const,
                                int64_t num_elements, double box_tol,
                                int dtype, sfem_stream_t stream);

/* cluster_size and max_shared (table entries per cluster) the cluster kernels
 * of (P, dtype) were compiled for; SFEM_EUNSUPPORTED outside P = 4..8.       */
int sfem_helmholtz_cluster_limits(int P, int dtype, int* cluster_size,
                                  int* max_shared);
#define SFEM_DOT_SLOTS 1024

int sfem_helmholtz_apply(const sfem_helmholtz_args* args, sfem_stream_t stream);

/* Element-local variant (no gather/scatter, no mask): u, out are (E, n, ncomp).
 * StokesVelocity.A_local / B_local (navier_stokes.py:220-236).               */
int sfem_helmholtz_local(const sfem_helmholtz_args* args, sfem_stream_t stream);

/* Coefficient sensitivities of  A(k, c, beta) = lambda0 B_c + lambda1 A_k +
 * C_beta  (sfem_helmholtz_args: kappa, sigma, beta), element-local: for two
 * scalar fields u, lam given at the operator's points, (E, n) each, per point
 *   dkappa[e,q]  = d(lam . A u) / d k[e,q]      = lambda1 g_lam . G g_u
 *   dsigma[e,q]  = d(lam . A u) / d c[e,q]      = lambda0 W lam u
 *   dbeta[e,q,d] = d(lam . A u) / d beta[e,q,d] = lam (D_d u)
 * with g the reference-space gradients, D_d the derivative along reference
 * direction d, and G, W the geometric factors WITHOUT coefficients: pass the
 * bare stored factors in `geo`, not a copy with k and c folded in.  No gather,
 * no scatter; arrays are indexed by element id, points in slot order
 * (lexicographic, axis 0 slowest), dbeta with ndim consecutive reals per
 * point.  Each output is optional: NULL skips the product and its stores;
 * with all three NULL the call does nothing.  geo / geo_elem / geo_index /
 * elem_list / dmat / weights / nodes / geo_mode as in sfem_helmholtz_args
 * (every geo_mode but SFEM_GEO_BOX).  ncomp != 1, ndim outside 2..3 and P
 * outside 2..12 return SFEM_EUNSUPPORTED; u or lam NULL is SFEM_EINVAL.
 * ABI version 10.                                                           */
typedef struct sfem_helmholtz_sens_args {
  const void* u;          /* (E, n)                                           */
  const void* lam;        /* (E, n)                                           */
  void* dkappa;           /* (E, n) or NULL                                   */
  void* dsigma;           /* (E, n) or NULL                                   */
  void* dbeta;            /* (E, n, ndim) or NULL                             */
  const void* geo;
  const void* geo_elem;
  const int32_t* geo_index;
  const int32_t* elem_list;
  const void* dmat;       /* HOST (P, P)                                      */
  const void* weights;    /* HOST (P,)                                        */
  const void* nodes;      /* HOST (P,)                                        */
  int64_t num_elements;
  int64_t num_listed;
  int32_t ndim, P, ncomp, dtype, geo_mode;
  double lambda0, lambda1;
} sfem_helmholtz_sens_args;
int sfem_helmholtz_sens(const sfem_helmholtz_sens_args* args,
                        sfem_stream_t stream);

/* ------------------------------------------------- fused Stokes operators ---
 * The P_N - P_{N-2} divergence D and pressure gradient D^T of
 * navier_stokes/navier_stokes.py:313-338 as one kernel each (gather, 3 d
 * sum-factorised derivative lines, cofactor geometry, projection onto /
 * interpolation from the P - 2 Gauss pressure nodes, scatter):
 *
 *   sfem_stokes_div:     p_out = pressure.scatter(D_local(velocity.gather(s u)))
 *       D_local(u)_k = sum_q phi_k(x_q) w_q detJ_q div u(x_q)          (:313-320)
 *       `scale` (optional; same layout as u, or one value per node) multiplies u as it is
 *       gathered: E = D Q D^T applies Q = (dt/beta_k) B^-1 (:340-348) for free.
 *   sfem_stokes_grad_t:  out = mask * velocity.scatter(Dt_local(pressure.gather(p)))
 *       Dt_local(p)_{i,c} = sum_q w_q detJ_q p(x_q) d phi_i/d x_c      (:322-338)
 *       DIRICHLET / SHARED bits of `enc` as in sfem_helmholtz_apply; the shared
 *       range [zero_begin, zero_end) of `out` is cleared by the call.  `scale`
 *       (optional, as for div) multiplies every element's contribution before it
 *       is assembled: for a factor that is equal on all copies of a node this
 *       is scale * (D^T p) after QQ^T, and E = D QQ^T (Q . D^T) spares D the
 *       gather of Q.
 *
 * Both integrate on the velocity GLL points (the `quadrature` of :279-282).
 * Geometry: SFEM_GEO_AFFINE / SFEM_GEO_MULTILINEAR evaluate the cofactors of
 * the Jacobian from `geo_elem` (sfem_helmholtz_setup_multilinear) in registers;
 * SFEM_GEO_POINT reads `kfac` (slots, ndim*ndim, Q) from sfem_stokes_setup:
 *   kfac[e][a*ndim + c][q] = w_q detJ_q invjac[e][q][c][a].
 * `interp` (HOST, (P, P-2) row-major) = pressure basis phi_k at the GLL points;
 * `penc` (E, (P-2)^ndim) = pressure node ids (negative = skip) or NULL for
 * e * (P-2)^ndim + k.  P = 4..12, ndim = 2, 3.                                */
typedef struct sfem_stokes_args {
  const void* u;          /* div: (N, ndim) velocity                           */
  void* out;              /* grad_t: (N, ndim) result                          */
  const void* p_in;       /* grad_t: (Np,) pressure                            */
  void* p_out;            /* div: (Np,) result                                 */
  const void* scale;      /* div: optional per-node factor, or NULL: (N, ndim)
                             in the layout of u, or (N,) if scale_per_node   */
  const int32_t* enc;     /* (E, n) encoded velocity indices                   */
  const int32_t* penc;    /* (E, np) pressure node ids or NULL                 */
  const void* kfac;       /* per-point weighted cofactors or NULL              */
  const void* geo_elem;   /* (E, 24) or NULL                                   */
  const int32_t* geo_index; /* (E,) slot of element e in kfac, or NULL = e     */
  const int32_t* elem_list; /* element ids of this launch, or NULL = all       */
  const void* dmat;       /* HOST (P, P)                                       */
  const void* weights;    /* HOST (P,)                                         */
  const void* nodes;      /* HOST (P,)                                         */
  const void* interp;     /* HOST (P, P-2)                                     */
  int64_t num_elements;
  int64_t num_listed;
  int64_t num_nodes;
  int64_t zero_begin, zero_end;   /* grad_t only                               */
  int32_t ndim, P, dtype, geo_mode;
  int64_t node_stride, comp_stride;  /* layout of u / out / scale (0 = (N, ndim)
                                        row-major)                             */
  int32_t scale_per_node; /* scale is one (N,) factor shared by the components */
  const uint16_t* shared_order; /* grad_t / e_first: as in sfem_helmholtz_args, */
  int32_t shared_stride;        /*   or NULL                                    */
  double* dot_out;        /* div: NULL, or SFEM_DOT_SLOTS device doubles that    */
                          /*   accumulate partial sums of p_in . p_out (the p.Ap */
                          /*   of the pressure CG when p_in is its direction)    */
  /* div / grad_t, 3D, P = 6..8, node_stride = 1 (component-major fields):    */
  /* compact connectivity of the velocity mesh and its chains, exactly as in  */
  /* sfem_helmholtz_args (NULL = off; `enc` / `shared_order` are then not     */
  /* read).  Both are needed: a launch without chains passes segments of one  */
  /* element.  The segments must hold every element of the launch once.       */
  /* geo_mode SFEM_GEO_BOX (these launches only): elements whose `geo_elem`   */
  /* has a diagonal constant Jacobian -- component c of div / grad_t then     */
  /* takes the one 1D derivative along axis c.                                */
  const int32_t* facet_table;     /* (E, 27, 4) from sfem_facet_table_build   */
  const int32_t* chain_offsets;   /* (num_chains + 1,)                        */
  const int32_t* chain_elems;
  int64_t num_chains;
} sfem_stokes_args;

int sfem_stokes_setup(const void* invjac, const void* jacdet,
                      const void* weights_nd, void* kfac, int64_t num_elements,
                      int ndim, int Q, int dtype, sfem_stream_t stream);
int sfem_stokes_div(const sfem_stokes_args* args, sfem_stream_t stream);
/* Convection integrand on a collocated grid of P points per direction (the
 * over-integration grid of StokesVelocity.C_local, navier_stokes.py:238-245,
 * after interpolation to it):  u, out (E, P^ndim, ndim) element-local,
 *   out[e,q,c] = w_q detJ_q sum_j u_j(x_q) d u_c/d x_j(x_q).
 * `dmat`, `weights`, `nodes` are those of that grid; enc / penc / interp /
 * p_in / p_out / scale are unused.                                           */
int sfem_stokes_convect_local(const sfem_stokes_args* args,
                              sfem_stream_t stream);
int sfem_stokes_grad_t(const sfem_stokes_args* args, sfem_stream_t stream);
/* E = D Q D^T (StokesSEM.E, navier_stokes.py:340-348) in two halves for a
 * diagonal Q = `scale`.  A velocity node held by one element only, and not part
 * of the periodic / partition exchange (`enc` must flag every other node
 * SHARED), is complete after that element's D^T, so the first half keeps it
 * in registers: scaled by Q it goes straight into the element's D.
 *   sfem_stokes_e_first : p_in -> `out` (SHARED nodes only: zero-filled range +
 *                         atomics; other entries are not written) and
 *                         p_out = D (Q . complete part)
 *   [caller: QQ^T exchange of `out` on the shared nodes]
 *   sfem_stokes_e_second: p_out += D (Q . u restricted to the SHARED nodes)
 * Same argument block as sfem_stokes_div / sfem_stokes_grad_t; `scale`
 * applies in both halves.  At P = 8 in 3D 216 of the 512 nodes of an element
 * never reach memory.                                                        */
int sfem_stokes_e_first(const sfem_stokes_args* args, sfem_stream_t stream);
int sfem_stokes_e_second(const sfem_stokes_args* args, sfem_stream_t stream);

/* ------------------------------------------- scalar transport: BDF/EXT rhs ---
 * The explicit right-hand side of a BDFk/EXTk step of
 *   dT/dt + u . grad T - div(k grad T) = s
 * on a collocated grid of P points per direction (the quadrature grid of the
 * implicit Helmholtz solve, after interpolation to it), element-local:
 *
 *   out[e,q] = wdet[e,q] (source[e,q] + sum_j mass_coef[j] T_j[e,q])
 *            + sum_j conv_coef[j] sum_a (sum_c Kw[a][c] u_j,c[e,q])
 *                                       d T_j / d xi_a [e,q]
 *
 * over num_levels <= SFEM_TRANSPORT_LEVELS time levels j, with
 * Kw[a][c] = w_q detJ_q d xi_a / d x_c the weighted cofactors of
 * sfem_stokes_convect_local (same geometry arguments: SFEM_GEO_AFFINE /
 * SFEM_GEO_MULTILINEAR from `geo_elem`, SFEM_GEO_POINT from `kfac` with
 * `geo_index`; `elem_list` / `num_listed` select the elements of a launch)
 * and wdet = w_q detJ_q given per point.  Arrays are indexed by element id,
 * points in slot order (lexicographic, axis 0 slowest), a velocity with ndim
 * consecutive reals per point.  A level with velocity[j] NULL or
 * conv_coef[j] = 0 contributes its mass term only.  `source` is optional;
 * `wdet` may be NULL when every mass_coef is 0 and there is no source.
 * ndim outside 2..3, P outside 2..12, more than SFEM_TRANSPORT_LEVELS levels
 * and any other geo_mode return SFEM_EUNSUPPORTED; a NULL out, dmat, scalar[j]
 * (j < num_levels), a missing geometry array or a missing required wdet is
 * SFEM_EINVAL.  ABI version 10.                                              */
#define SFEM_TRANSPORT_LEVELS 3
typedef struct sfem_transport_args {
  const void* scalar[SFEM_TRANSPORT_LEVELS];    /* T_j (E, n)                 */
  const void* velocity[SFEM_TRANSPORT_LEVELS];  /* u_j (E, n, ndim) or NULL   */
  double mass_coef[SFEM_TRANSPORT_LEVELS];
  double conv_coef[SFEM_TRANSPORT_LEVELS];
  const void* source;     /* (E, n) or NULL                                   */
  const void* wdet;       /* (E, n) or NULL                                   */
  void* out;              /* (E, n)                                           */
  const void* kfac;       /* per-point weighted cofactors or NULL             */
  const void* geo_elem;   /* (E, 24) or NULL                                  */
  const int32_t* geo_index; /* (E,) slot of element e in kfac, or NULL = e    */
  const int32_t* elem_list; /* element ids of this launch, or NULL = all      */
  const void* dmat;       /* HOST (P, P)                                      */
  const void* weights;    /* HOST (P,)                                        */
  const void* nodes;      /* HOST (P,)                                        */
  int64_t num_elements;
  int64_t num_listed;
  int32_t num_levels, ndim, P, dtype, geo_mode;
} sfem_transport_args;
int sfem_transport_rhs(const sfem_transport_args* args, sfem_stream_t stream);

/* The vector-Jacobian product of sfem_transport_rhs.  The right-hand side is
 * linear in the source and bilinear in (T_j, u_j); with `cotangent` = lam the
 * cotangent of `out`, per element and point
 *
 *   dsource[q]         = wdet[q] lam[q]
 *   dscalar[j][q]      = mass_coef[j] wdet[q] lam[q]
 *                      + conv_coef[j] sum_a (D_a^T (U_j,a . lam))[q],
 *                        U_j,a = sum_c Kw[a][c] u_j,c
 *   dvelocity[j][q][c] = conv_coef[j] lam[q] sum_a Kw[a][c][q] (D_a T_j)[q]
 *
 * with D_a the derivative along reference axis a.  Geometry arguments, array
 * layouts, `elem_list` / `num_listed` and the level conventions are those of
 * sfem_transport_args; element-local, no atomics.  Every output is optional
 * (NULL skips its work and its stores): without dvelocity[j] the level does
 * not read scalar[j], which may then be NULL; without dscalar[j] the
 * transposed derivative stage is skipped.  A level with velocity[j] NULL or
 * conv_coef[j] = 0 contributes its mass term to dscalar[j] only (a
 * dvelocity[j] given with conv_coef[j] = 0 is written as zeros).  Rows of
 * elements outside the launch are not written.  `wdet` may be NULL when no
 * dscalar[j] with mass_coef[j] != 0 and no dsource is asked for.
 * ndim outside 2..3, P outside 2..12, more than SFEM_TRANSPORT_LEVELS levels
 * and any other geo_mode return SFEM_EUNSUPPORTED; a NULL cotangent or dmat,
 * a dvelocity[j] without scalar[j] or velocity[j], a missing geometry array
 * or a missing required wdet is SFEM_EINVAL.  ABI version 10 (a pure
 * addition).                                                                */
typedef struct sfem_transport_vjp_args {
  const void* cotangent;                        /* lam (E, n)                  */
  const void* scalar[SFEM_TRANSPORT_LEVELS];    /* T_j; may be NULL when       */
                                                /* dvelocity[j] is NULL        */
  const void* velocity[SFEM_TRANSPORT_LEVELS];  /* u_j (E, n, ndim) or NULL    */
  double mass_coef[SFEM_TRANSPORT_LEVELS];
  double conv_coef[SFEM_TRANSPORT_LEVELS];
  const void* wdet;       /* (E, n) or NULL                                   */
  void* dscalar[SFEM_TRANSPORT_LEVELS];         /* (E, n) or NULL              */
  void* dvelocity[SFEM_TRANSPORT_LEVELS];       /* (E, n, ndim) or NULL        */
  void* dsource;          /* (E, n) or NULL                                   */
  const void* kfac;       /* per-point weighted cofactors or NULL             */
  const void* geo_elem;   /* (E, 24) or NULL                                  */
  const int32_t* geo_index; /* (E,) slot of element e in kfac, or NULL = e    */
  const int32_t* elem_list; /* element ids of this launch, or NULL = all      */
  const void* dmat;       /* HOST (P, P)                                      */
  const void* weights;    /* HOST (P,)                                        */
  const void* nodes;      /* HOST (P,)                                        */
  int64_t num_elements;
  int64_t num_listed;
  int32_t num_levels, ndim, P, dtype, geo_mode;
} sfem_transport_vjp_args;
int sfem_transport_rhs_vjp(const sfem_transport_vjp_args* args,
                           sfem_stream_t stream);

/* ------------------------------------------------------ linear elasticity ---
 * out = K u + lambda0 M_rho u on a collocated grid of P points per direction
 * (the quadrature grid of the solve, after interpolation to it), element-
 * local, with v^T K u = int sigma(u) : grad v and
 * sigma = lam tr(eps) I + 2 mu eps (plane strain in 2D).  Per element and
 * point, with Kw[a][j] = w_q detJ_q d xi_a / d x_j the weighted cofactors of
 * sfem_transport_args (same geometry arguments, `elem_list` / `num_listed`)
 * and W = wdet = w_q detJ_q:
 *
 *   G[c][a] = d u_c / d xi_a
 *   H[c][j] = (1/W) sum_a Kw[a][j] G[c][a]
 *   S[c][j] = lam (tr H) delta_cj + mu (H[c][j] + H[j][c])
 *   F[c][a] = sum_j Kw[a][j] S[c][j]
 *   out[e,m,c] = sum_a sum_q D_a[q,m] F[c][a](q) + lambda0 rho W u_c(m)
 *
 * `u` and `out` are (E, n, ndim) row-major, points in slot order; `wdet` is
 * required.  `lam`, `mu` and `rho` are (E, n) per-point arrays, or NULL for
 * the scalar lam_const / mu_const / rho_const.  lambda0 = 0 skips the mass
 * term.  ndim outside 2..3, P outside 2..12 and any other geo_mode return
 * SFEM_EUNSUPPORTED; a NULL u, out, dmat, wdet or a missing geometry array is
 * SFEM_EINVAL.  ABI version 10 (a pure addition).                            */
typedef struct sfem_elasticity_args {
  const void* u;          /* (E, n, ndim)                                     */
  void* out;              /* (E, n, ndim)                                     */
  const void* wdet;       /* (E, n)                                           */
  const void* lam;        /* (E, n) or NULL                                   */
  const void* mu;         /* (E, n) or NULL                                   */
  const void* rho;        /* (E, n) or NULL                                   */
  double lam_const, mu_const, rho_const, lambda0;
  const void* kfac;       /* per-point weighted cofactors or NULL             */
  const void* geo_elem;   /* (E, 24) or NULL                                  */
  const int32_t* geo_index; /* (E,) slot of element e in kfac, or NULL = e    */
  const int32_t* elem_list; /* element ids of this launch, or NULL = all      */
  const void* dmat;       /* HOST (P, P)                                      */
  const void* weights;    /* HOST (P,)                                        */
  const void* nodes;      /* HOST (P,)                                        */
  int64_t num_elements;
  int64_t num_listed;
  int32_t ndim, P, dtype, geo_mode;
} sfem_elasticity_args;
int sfem_elasticity_local(const sfem_elasticity_args* args,
                          sfem_stream_t stream);

/* Lame and density sensitivities of that operator: for two displacement
 * fields `u` and `v` on the collocated grid ((E, n, ndim) each) and
 * H_u = (1/W) Kw G_u, H_v = (1/W) Kw G_v as above, per point q
 *
 *   dlam[q] = W tr(H_u) tr(H_v)
 *   dmu[q]  = W sum_{c,j} (H_u[c][j] + H_u[j][c]) H_v[c][j]
 *   drho[q] = lambda0 W sum_c u_c v_c
 *
 * the derivatives of v^T (K + lambda0 M_rho) u with respect to lam[q], mu[q]
 * and rho[q].  Each output is (E, n) in the layout of the per-point
 * coefficients, or NULL: its product and its stores are skipped, and with
 * `dlam` and `dmu` both NULL no derivative is formed.  Element-local: no
 * gather, no scatter, no atomics.  Geometry and launch arguments are those of
 * sfem_elasticity_args.  ndim outside 2..3, P outside 2..12 and any other
 * geo_mode return SFEM_EUNSUPPORTED; a NULL u, v, dmat or wdet, all three
 * outputs NULL or a missing geometry array is SFEM_EINVAL.  ABI version 10 (a
 * pure addition).                                                            */
typedef struct sfem_elasticity_sens_args {
  const void* u;          /* (E, n, ndim)                                     */
  const void* v;          /* (E, n, ndim)                                     */
  const void* wdet;       /* (E, n)                                           */
  void* dlam;             /* (E, n) or NULL                                   */
  void* dmu;              /* (E, n) or NULL                                   */
  void* drho;             /* (E, n) or NULL                                   */
  double lambda0;
  const void* kfac;       /* per-point weighted cofactors or NULL             */
  const void* geo_elem;   /* (E, 24) or NULL                                  */
  const int32_t* geo_index; /* (E,) slot of element e in kfac, or NULL = e    */
  const int32_t* elem_list; /* element ids of this launch, or NULL = all      */
  const void* dmat;       /* HOST (P, P)                                      */
  const void* weights;    /* HOST (P,)                                        */
  const void* nodes;      /* HOST (P,)                                        */
  int64_t num_elements;
  int64_t num_listed;
  int32_t ndim, P, dtype, geo_mode;
} sfem_elasticity_sens_args;
int sfem_elasticity_sens(const sfem_elasticity_sens_args* args,
                         sfem_stream_t stream);

/* Stress recovery on the collocated grid: for a displacement field `u`
 * ((E, n, ndim)) and H = (1/W) Kw G, t = tr H as above, per point q
 *
 *   sigma_cc = lam t + 2 mu H[c][c],   sigma_cj = mu (H[c][j] + H[j][c])
 *   vm = sqrt(0.5 ((sxx-syy)^2 + (syy-szz)^2 + (szz-sxx)^2)
 *             + 3 (sxy^2 + sxz^2 + syz^2))
 *
 * `sigma` is (E, n, NV): NV = 6 in 3D, slots (xx, yy, zz, xy, xz, yz); NV = 4
 * in 2D, slots (xx, yy, xy, zz) with sigma_zz = lam t (plane strain), or 0
 * when `plane_stress` is set (the caller then passes the modified lambda).
 * `vm` is (E, n).  Either output may be NULL and is then skipped.  Points
 * with W = 0 (the all -1 rows of a padded mesh) give zeros.  `lam` and `mu`
 * are (E, n) arrays or NULL for lam_const / mu_const.  Element-local: no
 * gather, no scatter, no atomics.  Geometry and launch arguments are those of
 * sfem_elasticity_args.  ndim outside 2..3, P outside 2..12 and any other
 * geo_mode return SFEM_EUNSUPPORTED; a NULL u, dmat or wdet, both outputs
 * NULL or a missing geometry array is SFEM_EINVAL.  ABI version 10 (a pure
 * addition).                                                                 */
typedef struct sfem_elasticity_stress_args {
  const void* u;          /* (E, n, ndim)                                     */
  void* sigma;            /* (E, n, NV) or NULL                               */
  void* vm;               /* (E, n) or NULL                                   */
  const void* wdet;       /* (E, n)                                           */
  const void* lam;        /* (E, n) or NULL                                   */
  const void* mu;         /* (E, n) or NULL                                   */
  double lam_const, mu_const;
  const void* kfac;       /* per-point weighted cofactors or NULL             */
  const void* geo_elem;   /* (E, 24) or NULL                                  */
  const int32_t* geo_index; /* (E,) slot of element e in kfac, or NULL = e    */
  const int32_t* elem_list; /* element ids of this launch, or NULL = all      */
  const void* dmat;       /* HOST (P, P)                                      */
  const void* weights;    /* HOST (P,)                                        */
  const void* nodes;      /* HOST (P,)                                        */
  int64_t num_elements;
  int64_t num_listed;
  int32_t ndim, P, dtype, geo_mode;
  int32_t plane_stress;   /* 2D: sigma_zz = 0                                 */
} sfem_elasticity_stress_args;
int sfem_elasticity_stress(const sfem_elasticity_stress_args* args,
                           sfem_stream_t stream);

/* The vector-Jacobian product of sfem_elasticity_stress: for a cotangent
 * `sbar` ((E, n, NV), the slots of `sigma`) and dbar = sum_c sbar_cc (plus
 * sbar_zz in 2D plane strain)
 *
 *   Hbar[c][j] = lam dbar delta_cj + mu (c == j ? 2 sbar_cc : sbar_cj)
 *   Gbar[c][a] = (1/W) sum_j Kw[a][j] Hbar[c][j]
 *   ubar[e,m,c] = sum_a sum_q D_a[q,m] Gbar[c][a](q)
 *   dlam[q] = tr(H_u) dbar
 *   dmu[q]  = sum_c 2 H_u[c][c] sbar_cc
 *             + sum_{c<j} (H_u[c][j] + H_u[j][c]) sbar_cj
 *
 * No W weights the sums: stress is a pointwise value.  `ubar` is (E, n, ndim),
 * `dlam` and `dmu` are (E, n); each may be NULL and is then skipped.  `u` is
 * read for `dlam` / `dmu` only and may be NULL without them.  Points with
 * W = 0 give zeros.  A NULL sbar, dmat or wdet, a NULL u where dlam or dmu is
 * asked for, all three outputs NULL or a missing geometry array is
 * SFEM_EINVAL; the shape checks are those above.  ABI version 10 (a pure
 * addition).                                                                 */
typedef struct sfem_elasticity_stress_vjp_args {
  const void* sbar;       /* (E, n, NV)                                       */
  const void* u;          /* (E, n, ndim), or NULL without dlam and dmu       */
  void* ubar;             /* (E, n, ndim) or NULL                             */
  void* dlam;             /* (E, n) or NULL                                   */
  void* dmu;              /* (E, n) or NULL                                   */
  const void* wdet;       /* (E, n)                                           */
  const void* lam;        /* (E, n) or NULL                                   */
  const void* mu;         /* (E, n) or NULL                                   */
  double lam_const, mu_const;
  const void* kfac;       /* per-point weighted cofactors or NULL             */
  const void* geo_elem;   /* (E, 24) or NULL                                  */
  const int32_t* geo_index; /* (E,) slot of element e in kfac, or NULL = e    */
  const int32_t* elem_list; /* element ids of this launch, or NULL = all      */
  const void* dmat;       /* HOST (P, P)                                      */
  const void* weights;    /* HOST (P,)                                        */
  const void* nodes;      /* HOST (P,)                                        */
  int64_t num_elements;
  int64_t num_listed;
  int32_t ndim, P, dtype, geo_mode;
  int32_t plane_stress;   /* 2D: sbar_zz takes no part                        */
} sfem_elasticity_stress_vjp_args;
int sfem_elasticity_stress_vjp(const sfem_elasticity_stress_vjp_args* args,
                               sfem_stream_t stream);

/* ------------------------------------- finite-strain (neo-Hookean) elasticity ---
 * Compressible neo-Hookean material, total Lagrangian (the geometry is the
 * reference mesh), on the collocated grid of sfem_elasticity_args, element-
 * local.  With F = I + H, H[c][j] = d u_c / d X_j = (1/W) sum_a Kw[a][j]
 * G[c][a] as above, J = det F (plane strain in 2D: the 2 x 2 block):
 *
 *   psi(F) = mu/2 (F:F - d) - mu ln J + lam/2 (ln J)^2
 *   P(F)   = mu (F - F^-T) + lam ln J F^-T
 *   dP[dH] = mu dH + (mu - lam ln J) F^-T dH^T F^-T + lam tr(F^-1 dH) F^-T
 *
 * mode = SFEM_HYPER_RESIDUAL: `u` is the displacement and
 *
 *   out[e,m,c] = sum_a sum_q D_a[q,m] (sum_j Kw[a][j] P[c][j])(q)
 *                + lambda0 rho W u_c(m)
 *
 * the local part of R(u) = int P(F) : grad v + lambda0 int rho u . v.  Where
 * `state` is non-NULL it receives (E, n, d*d + 1) reals, per point F^-1
 * row-major in slots 0 .. d*d - 1 and ln J in slot d*d; where `psi` is
 * non-NULL it receives (E, n) values W psi(F) + lambda0/2 rho W |u|^2, whose
 * sum is the energy.
 *
 * mode = SFEM_HYPER_TANGENT: `u` is an increment w, `state` the output of a
 * residual launch at the point of linearisation, and
 *
 *   out[e,m,c] = sum_a sum_q D_a[q,m] (sum_j Kw[a][j] dP[dH_w][c][j])(q)
 *                + lambda0 rho W w_c(m)
 *
 * with F^-1 and ln J read from `state`: no inverse and no logarithm is taken.
 * At state (I, 0) this is sfem_elasticity_local.
 *
 * J <= 0 at a point (an inverted state) is not an error: the logarithm is
 * NaN or -inf and the outputs of that element are non-finite.  Points with
 * W = 0 take H = 0.  `lam`, `mu`, `rho`, the geometry and launch arguments
 * are those of sfem_elasticity_args.  ndim outside 2..3, P outside 2..12 and
 * any other geo_mode or mode return SFEM_EUNSUPPORTED; a NULL u, out, dmat,
 * wdet or a missing geometry array, the tangent mode with a NULL `state` or
 * with a non-NULL `psi` is SFEM_EINVAL.  ABI version 10 (a pure addition).   */
#define SFEM_HYPER_RESIDUAL 0
#define SFEM_HYPER_TANGENT 1
typedef struct sfem_hyperelastic_args {
  const void* u;          /* (E, n, ndim): displacement, or the increment     */
  void* out;              /* (E, n, ndim)                                     */
  const void* wdet;       /* (E, n)                                           */
  const void* lam;        /* (E, n) or NULL                                   */
  const void* mu;         /* (E, n) or NULL                                   */
  const void* rho;        /* (E, n) or NULL                                   */
  double lam_const, mu_const, rho_const, lambda0;
  const void* kfac;       /* per-point weighted cofactors or NULL             */
  const void* geo_elem;   /* (E, 24) or NULL                                  */
  const int32_t* geo_index; /* (E,) slot of element e in kfac, or NULL = e    */
  const int32_t* elem_list; /* element ids of this launch, or NULL = all      */
  const void* dmat;       /* HOST (P, P)                                      */
  const void* weights;    /* HOST (P,)                                        */
  const void* nodes;      /* HOST (P,)                                        */
  int64_t num_elements;
  int64_t num_listed;
  int32_t ndim, P, dtype, geo_mode;
  void* state;            /* (E, n, ndim*ndim + 1): out (residual, or NULL),
                             in (tangent)                                     */
  void* psi;              /* (E, n) or NULL; residual mode only               */
  int32_t mode;           /* SFEM_HYPER_RESIDUAL / SFEM_HYPER_TANGENT         */
} sfem_hyperelastic_args;
int sfem_hyperelastic_local(const sfem_hyperelastic_args* args,
                            sfem_stream_t stream);

/* Lame and density sensitivities of that residual: for a displacement `u`
 * whose residual launch stored `state` ((E, n, d*d + 1): F^-1 row-major and
 * ln J per point), a second field `v` on the collocated grid ((E, n, ndim))
 * and H_v = (1/W) Kw G_v as above, per point q
 *
 *   dlam[q] = W lnJ tr(F^-1 H_v)
 *   dmu[q]  = W (F : H_v - tr(F^-1 H_v))
 *   drho[q] = lambda0 W sum_c u_c v_c
 *
 * the derivatives of v^T R(u; lam, mu, rho) with respect to lam[q], mu[q] and
 * rho[q]; tr(F^-1 H_v) = sum_{c,j} F^-1[j][c] H_v[c][j], and F is recovered
 * from `state` by the adjugate of F^-1, so `u` is neither interpolated nor
 * differentiated again and is read for `drho` alone.  Each output is (E, n) in
 * the layout of the per-point coefficients, or NULL: its product and its
 * stores are skipped, and with `dlam` and `dmu` both NULL no derivative is
 * formed.  A point with W = 0 gives exactly 0 in every output whatever its
 * state row holds.  Element-local: no gather, no scatter, no atomics.
 * Geometry and launch arguments are those of sfem_elasticity_args.  ndim
 * outside 2..3, P outside 2..12 and any other geo_mode return
 * SFEM_EUNSUPPORTED; a NULL v, state, dmat or wdet, all three outputs NULL,
 * `drho` without `u` or a missing geometry array is SFEM_EINVAL.  ABI version
 * 10 (a pure addition).                                                      */
typedef struct sfem_hyperelastic_sens_args {
  const void* v;          /* (E, n, ndim)                                     */
  const void* state;      /* (E, n, ndim*ndim + 1)                            */
  const void* u;          /* (E, n, ndim), or NULL where drho is NULL         */
  const void* wdet;       /* (E, n)                                           */
  void* dlam;             /* (E, n) or NULL                                   */
  void* dmu;              /* (E, n) or NULL                                   */
  void* drho;             /* (E, n) or NULL                                   */
  double lambda0;
  const void* kfac;       /* per-point weighted cofactors or NULL             */
  const void* geo_elem;   /* (E, 24) or NULL                                  */
  const int32_t* geo_index; /* (E,) slot of element e in kfac, or NULL = e    */
  const int32_t* elem_list; /* element ids of this launch, or NULL = all      */
  const void* dmat;       /* HOST (P, P)                                      */
  const void* weights;    /* HOST (P,)                                        */
  const void* nodes;      /* HOST (P,)                                        */
  int64_t num_elements;
  int64_t num_listed;
  int32_t ndim, P, dtype, geo_mode;
} sfem_hyperelastic_sens_args;
int sfem_hyperelastic_sens(const sfem_hyperelastic_sens_args* args,
                           sfem_stream_t stream);

/* --------------------------------------- small-strain J2 (von Mises) plasticity ---
 * Rate-independent von Mises plasticity with linear isotropic hardening on
 * the collocated grid of sfem_elasticity_args, element-local, modelled on
 * sfem_hyperelastic_local: a residual launch that stores a per-point state and
 * a tangent launch that reads it.  With H[c][j] = d u_c / d x_j = (1/W) sum_a
 * Kw[a][j] G[c][a] as above, eps = sym(H) (plane strain in 2D: the 3 x 3
 * tensor with eps_zz = eps_xz = eps_yz = 0) and the committed history
 * (eps_p, alpha) of the point, eps_p symmetric and trace-free, alpha >= 0:
 *
 *   e = eps - eps_p,  s_tr = 2 mu dev(e),  q = sqrt(3/2) |s_tr|
 *   f = q - (sigma_y + Hh alpha)
 *   f <= 0: sigma = lam tr(eps) I + 2 mu e,  history unchanged,
 *           a = 2 mu, b = 0, n = 0
 *   f >  0: dg = f / (3 mu + Hh),  n = s_tr / |s_tr|
 *           eps_p' = eps_p + sqrt(3/2) dg n,  alpha' = alpha + dg
 *           sigma  = (lam + 2 mu / 3) tr(eps) I + theta s_tr
 *           theta  = 1 - 3 mu dg / q,  a = 2 mu theta
 *           b      = 2 mu (1 / (1 + Hh / (3 mu)) - (1 - theta))
 *   dsigma[deps] = lam tr(deps) I + 2 mu deps - (2 mu - a) dev(deps)
 *                  - b (n : deps) n
 *
 * Voigt slots are those of sfem_elasticity_stress: 3D (xx, yy, zz, xy, xz,
 * yz); 2D (xx, yy, xy), with zz last where it is stored.  Per point
 *
 *   history  NH = 7 in 3D: eps_p in the six slots, then alpha
 *            NH = 4 in 2D: eps_p xx, yy, xy, then alpha (eps_p,zz = -(xx + yy))
 *   lin      NL = 8 in 3D: a, b, then n in the six slots
 *            NL = 5 in 2D: a, b, n_xx, n_yy, n_xy (deps_zz = 0)
 *   stress   6 in 3D; 4 in 2D: xx, yy, xy, zz
 *
 * mode = SFEM_PLAST_RESIDUAL: `u` is the displacement and
 *
 *   out[e,m,c] = sum_a sum_q D_a[q,m] (sum_j Kw[a][j] sigma[c][j])(q)
 *                + lambda0 rho W u_c(m)
 *
 * the local part of R(u) = int sigma : grad v + lambda0 int rho u . v.
 * `hist_in` ((E, n, NH), or NULL for virgin material) is read and never
 * written.  `hist_out` (E, n, NH) receives the trial history (eps_p',
 * alpha'), `lin` (E, n, NL) the state of the tangent and `stress` (E, n, 6 | 4)
 * sigma, each where non-NULL.  `hist_in` and `hist_out` must not be the same
 * array.
 *
 * mode = SFEM_PLAST_TANGENT: `u` is an increment w, `lin` the output of a
 * residual launch at the point of linearisation, and
 *
 *   out[e,m,c] = sum_a sum_q D_a[q,m] (sum_j Kw[a][j] dsigma[deps_w][c][j])(q)
 *                + lambda0 rho W w_c(m)
 *
 * with no square root and no division.  With lin = (2 mu, 0, 0) this is
 * sfem_elasticity_local.
 *
 * Points with W = 0 take H = 0 and every output is finite there.  `lam`,
 * `mu`, `rho`, `yield` (sigma_y > 0) and `hard` (Hh >= 0) are (E, n) arrays
 * or NULL for their constants; the geometry and launch arguments are those of
 * sfem_elasticity_args.  ndim outside 2..3, P outside 2..12 and any other
 * geo_mode or mode return SFEM_EUNSUPPORTED; a NULL u, out, dmat, wdet or a
 * missing geometry array, the tangent mode with a NULL `lin` or with a
 * non-NULL `hist_in`, `hist_out` or `stress`, and hist_in == hist_out (both
 * non-NULL) are SFEM_EINVAL.  ABI version 10 (a pure addition).              */
#define SFEM_PLAST_RESIDUAL 0
#define SFEM_PLAST_TANGENT 1
typedef struct sfem_plasticity_args {
  const void* u;          /* (E, n, ndim): displacement, or the increment     */
  void* out;              /* (E, n, ndim)                                     */
  const void* wdet;       /* (E, n)                                           */
  const void* lam;        /* (E, n) or NULL                                   */
  const void* mu;         /* (E, n) or NULL                                   */
  const void* rho;        /* (E, n) or NULL                                   */
  double lam_const, mu_const, rho_const, lambda0;
  const void* kfac;       /* per-point weighted cofactors or NULL             */
  const void* geo_elem;   /* (E, 24) or NULL                                  */
  const int32_t* geo_index; /* (E,) slot of element e in kfac, or NULL = e    */
  const int32_t* elem_list; /* element ids of this launch, or NULL = all      */
  const void* dmat;       /* HOST (P, P)                                      */
  const void* weights;    /* HOST (P,)                                        */
  const void* nodes;      /* HOST (P,)                                        */
  int64_t num_elements;
  int64_t num_listed;
  int32_t ndim, P, dtype, geo_mode;
  double yield_const, hard_const;
  void* yield;            /* (E, n) or NULL                                   */
  void* hard;             /* (E, n) or NULL                                   */
  void* hist_in;          /* (E, n, NH) or NULL = virgin; residual only       */
  void* hist_out;         /* (E, n, NH) or NULL; residual only                */
  void* lin;              /* (E, n, NL): out (residual, or NULL), in (tangent)*/
  void* stress;           /* (E, n, 6 | 4) or NULL; residual only             */
  int32_t mode;           /* SFEM_PLAST_RESIDUAL / SFEM_PLAST_TANGENT         */
} sfem_plasticity_args;
int sfem_plasticity_local(const sfem_plasticity_args* args,
                          sfem_stream_t stream);

/* ---------------------------- vector-Jacobian product of the radial return ---
 * The point map of sfem_plasticity_local is (eps, eps_p, alpha; lam, mu,
 * sigma_y, Hh) -> (sigma, eps_p', alpha').  With cotangents S of sigma, Pb of
 * eps_p' (symmetric 3 x 3) and ab of alpha', r32 = sqrt(3/2), e = eps - eps_p,
 * s = 2 mu dev(e), sn = |s|, n = s / sn, f = r32 sn - sigma_y - Hh alpha,
 * c = 1 / (3 mu + Hh), dg = c f:
 *
 *   common:   eps_b = lam tr(S) I + 2 mu S;  lam_b = tr(eps) tr(S);
 *             Z = Pb - 2 mu S
 *   f <= 0:   epsp_b = Z;  alpha_b = ab;  mu_b = 2 (eps - eps_p) : S;
 *             sy_b = Hh_b = 0
 *   f >  0:   mu_b   = 2 (eps - eps_p') : S
 *             dg_b   = ab + r32 (n : Z);      n_b = r32 dg Z
 *             f_b    = c dg_b;   mu_b -= 3 c dg dg_b
 *             Hh_b   = -c dg dg_b - alpha f_b
 *             sy_b   = -f_b;     alpha_b = ab - Hh f_b
 *             s_b    = (n_b - (n : n_b) n) / sn + r32 f_b n
 *             e_b    = 2 mu dev(s_b);   mu_b += (s : s_b) / mu
 *             eps_b += e_b;   epsp_b = Z - e_b
 *
 * Cotangents of histories refer to the stored (E, n, NH) arrays: Pb_xy =
 * hbar[xy] / 2 on input and hbar_prev[xy] = 2 epsp_b_xy on output (a stored
 * off-diagonal slot stands for two tensor entries); in 2D Pb_zz = 0 and
 * hbar_prev[xx] = epsp_b_xx - epsp_b_zz, likewise yy (eps_p,zz = -(xx + yy)
 * is implied).  The launch repeats the return mapping from `u` on the grid
 * and `hist_in` (NULL: virgin); it reads no output of a forward launch.
 *
 * mode = SFEM_PLAST_VJP_DISPLACEMENT: `out` (E, n, ndim) = d(hbar . Phi)/du,
 * Phi the history update hist_in -> (eps_p', alpha'): the point VJP with
 * S = 0, eps_b / W folded through the cofactors and the transposed
 * derivatives as the stress of the residual is (no quadrature weight).
 * Needs u, hbar, out; w, hbar_prev and the five d* must be NULL.
 *
 * mode = SFEM_PLAST_VJP_STATE: for a second field `w` (E, n, ndim), the point
 * VJP with S = W sym(H_w), Pb and ab from `hbar` (NULL: zero).  Each where
 * non-NULL: `hbar_prev` (E, n, NH) the cotangent of hist_in, `dlam`, `dmu`,
 * `dyield`, `dhard` (E, n) the derivatives of w . R(u) + hbar . Phi(u) by the
 * point's coefficients, `drho` (E, n) = lambda0 W u . w.  Needs u, w and one
 * output; `out` must be NULL.  hbar_prev must be neither hist_in nor hbar.
 *
 * A point with W = 0 stores exact zeros in every output.  The coefficient,
 * geometry and launch arguments are those of sfem_plasticity_args; the return
 * codes follow sfem_plasticity_local.  ABI version 10 (a pure addition).     */
#define SFEM_PLAST_VJP_DISPLACEMENT 0
#define SFEM_PLAST_VJP_STATE 1
typedef struct sfem_plasticity_vjp_args {
  const void* u;          /* (E, n, ndim): displacement                       */
  const void* w;          /* (E, n, ndim): second field; state mode           */
  const void* wdet;       /* (E, n)                                           */
  const void* lam;        /* (E, n) or NULL                                   */
  const void* mu;         /* (E, n) or NULL                                   */
  const void* yield;      /* (E, n) or NULL                                   */
  const void* hard;       /* (E, n) or NULL                                   */
  double lam_const, mu_const, yield_const, hard_const, lambda0;
  const void* hist_in;    /* (E, n, NH) or NULL = virgin                      */
  const void* hbar;       /* (E, n, NH); NULL = zero in the state mode        */
  void* out;              /* (E, n, ndim); displacement mode                  */
  void* hbar_prev;        /* (E, n, NH) or NULL; state mode, as the five below*/
  void* dlam;             /* (E, n) or NULL                                   */
  void* dmu;
  void* dyield;
  void* dhard;
  void* drho;
  const void* kfac;       /* per-point weighted cofactors or NULL             */
  const void* geo_elem;   /* (E, 24) or NULL                                  */
  const int32_t* geo_index; /* (E,) slot of element e in kfac, or NULL = e    */
  const int32_t* elem_list; /* element ids of this launch, or NULL = all      */
  const void* dmat;       /* HOST (P, P)                                      */
  const void* weights;    /* HOST (P,)                                        */
  const void* nodes;      /* HOST (P,)                                        */
  int64_t num_elements;
  int64_t num_listed;
  int32_t ndim, P, dtype, geo_mode;
  int32_t mode;           /* SFEM_PLAST_VJP_DISPLACEMENT / SFEM_PLAST_VJP_STATE */
} sfem_plasticity_vjp_args;
int sfem_plasticity_vjp(const sfem_plasticity_vjp_args* args,
                        sfem_stream_t stream);

/* ------------------------------------- fields at points: locate, eval, eval^T ---
 * A field of order P1 - 1 on element e is u(xi) = sum_n u[elements[e, n]]
 * l_n(xi) with l_n the tensor product of the 1D Lagrange polynomials on
 * `nodes` (HOST, P1 doubles; `bary` = 1 / prod_{k != i} (nodes[i] - nodes[k]),
 * HOST, P1 doubles), n lexicographic with axis 0 slowest.  The basis is formed
 * in the product form l_i(x) = bary[i] prod_{k != i} (x - nodes[k]), which is
 * finite at the nodes.
 *
 * sfem_point_locate finds, for each of `num_points` points (mesh dtype,
 * (M, ndim)), an element and reference coordinates with x(xi) = point, where
 * x(xi) is the same expansion of `node_coords`.  Candidates come from a
 * uniform grid of ncell[0] x .. x ncell[ndim-1] cells over [grid_lo, grid_hi]
 * (cell of x along axis a: floor((x_a - grid_lo[a]) * inv_cell[a]), clamped;
 * cell index lexicographic with axis 0 slowest) as a CSR list `cell_offsets`
 * / `cell_elems` of element ids, ascending per cell.  A point outside
 * [grid_lo, grid_hi] is not found.  One lane per point walks its cell's
 * candidates: reject by `boxes` (E, 2, ndim doubles: lower corner, upper
 * corner), then at most `max_iter` Newton steps from xi = 0 in double
 * arithmetic (Cramer's rule, xi clamped to [-1.5, 1.5] after each step) and,
 * when that pass ends outside the reference cube, once more at most
 * `max_iter` steps from the nearest point of the cube (the continued map of a
 * curved element can fold back onto a point on a face), then accept when max |xi| <= 1 + tol_xi and max_a |x(xi) - point|_a <= tol_x *
 * extent[e] (E doubles).  The first accepted candidate (the lowest element id)
 * wins.  Outputs: `element` (M,) int32 (-1 when not found), `xi` (M, ndim) in
 * the mesh dtype (0 when not found), `found` (M,) uint8.  No atomics, no
 * barriers, every loop bounded by an argument.  Every entry of cell_elems
 * must be a row of `elements` without -1 in [0, num_elements), every node id
 * in [0, num_nodes); a node id outside that range reads coordinate 0.
 * ndim outside 2..3 and P1 outside 2..12 return SFEM_EUNSUPPORTED; null
 * pointers, max_iter outside 0..64, a negative tolerance or size, a
 * non-positive ncell or a CSR too long for int32 element ids are SFEM_EINVAL.
 * ABI version 10 (a pure addition).                                          */
typedef struct sfem_point_locate_args {
  const void* points;          /* (M, ndim)                                   */
  const void* node_coords;     /* (N, ndim)                                   */
  const int32_t* elements;     /* (E, P1^ndim)                                */
  const int64_t* cell_offsets; /* (cells + 1,)                                */
  const int32_t* cell_elems;   /* (cell_offsets[cells],)                      */
  const double* boxes;         /* (E, 2, ndim)                                */
  const double* extent;        /* (E,)                                        */
  const double* nodes;         /* HOST (P1,)                                  */
  const double* bary;          /* HOST (P1,)                                  */
  int32_t* element;            /* out (M,)                                    */
  void* xi;                    /* out (M, ndim)                               */
  uint8_t* found;              /* out (M,)                                    */
  double grid_lo[3];
  double grid_hi[3];
  double inv_cell[3];
  double tol_xi, tol_x;
  int64_t num_points, num_nodes, num_elements;
  int32_t ncell[3];
  int32_t max_iter, ndim, P1, dtype;
} sfem_point_locate_args;
int sfem_point_locate(const sfem_point_locate_args* args, sfem_stream_t stream);

/* Evaluation at located points and its transpose, from a plan: the found
 * points sorted stably by element (`perm[p]` = index of sorted point p among
 * the M points, `xi` (F, ndim) in sorted order), cut into segments of one
 * element each (`seg_elem` (S,), ascending; `seg_offsets` (S + 1,) into the
 * sorted order) and, for the evaluation, into chunks of at most 64 points of
 * one element (`chunk_elem`, `chunk_start`, `chunk_count` (K,)).
 *
 * sfem_point_eval:    values[perm[p], c] = sum_n u[elements[e_p, n], c]
 *                                          l_n(xi_p)
 *   One wave per chunk: the element's nodal values of one component go to
 *   LDS through the index row (a -1 slot reads 0), each lane contracts its
 *   point sum-factorised.  `field` is addressed as field[k * node_stride +
 *   c * comp_stride] (sfem_exchange_classes); `values` is (M, ncomp)
 *   row-major, rows of points outside the plan are not written.
 * sfem_point_eval_t:  rows[s, n, c] = sum_{p in segment s} values[perm[p], c]
 *                                     l_n(xi_p)
 *   One workgroup per segment, its lanes own nodes and add the points in
 *   sorted order: no atomics, bitwise reproducible.  `rows` is (S, P1^ndim,
 *   ncomp); sfem_scatter_csr assembles it.  `field`, the strides and the
 *   chunk arrays are not read.
 * Every element id of the plan must be in [0, num_elements), every perm
 * entry in [0, num_points): the caller validates them on the host.
 * ndim outside 2..3 and P1 outside 2..12 return SFEM_EUNSUPPORTED; null
 * pointers, negative sizes, ncomp < 1 and more than 2^31 - 1 chunks or
 * segments are SFEM_EINVAL.  ABI version 10 (a pure addition).               */
#define SFEM_POINT_CHUNK 64
typedef struct sfem_point_args {
  const void* field;           /* eval: nodal field (strided)                 */
  void* values;                /* (M, ncomp): eval out, eval_t in             */
  void* rows;                  /* eval_t out (S, P1^ndim, ncomp)              */
  const int32_t* elements;     /* (E, P1^ndim)                                */
  const void* xi;              /* (F, ndim), sorted order                     */
  const int64_t* perm;         /* (F,)                                        */
  const int32_t* chunk_elem;   /* (K,)                                        */
  const int64_t* chunk_start;  /* (K,)                                        */
  const int32_t* chunk_count;  /* (K,) 1..SFEM_POINT_CHUNK                    */
  const int32_t* seg_elem;     /* (S,)                                        */
  const int64_t* seg_offsets;  /* (S + 1,)                                    */
  const double* nodes;         /* HOST (P1,)                                  */
  const double* bary;          /* HOST (P1,)                                  */
  int64_t num_points, num_found, num_chunks, num_segments;
  int64_t num_elements, num_nodes;
  int64_t node_stride, comp_stride;
  int32_t ncomp, ndim, P1, dtype;
} sfem_point_args;
int sfem_point_eval(const sfem_point_args* args, sfem_stream_t stream);
int sfem_point_eval_t(const sfem_point_args* args, sfem_stream_t stream);

/* ------------------------------------------------------------ CG kernels ---
 * Preconditioned CG of linalg/cg.py:30-97 with device-resident scalars: no
 * host synchronisation inside an iteration (the reference keeps its loop on
 * device with lax.while_loop, cg.py:94-95).  `scalars` is a device array of
 * SFEM_CG_NSCALARS (= 80) doubles -- ALL of them are read and written by the
 * update kernels and the scalar phases (ABI <= 2 callers allocated 16: they
 * must grow the array):
 *   [0] gamma = r.M r   [1] p.Ap   [2] gamma_new   [3] alpha   [4] beta
 *   [5] b.b   [6] atol2 = max(tol^2 b.b, atol^2)   [7] done (0/1)
 *   [8] iterations   [9] an iteration is open (phases 5 / 6)
 *   [11] r.Mr - r.r of the iteration, [12] the mean c (sfem_cg_update_xp_mean)
 *   [10] status, SFEM_CG_STATUS_*: why `done` was raised.  Beyond the
 *        reference's stop rule (cg.py:68-73, which reads a negative or NaN
 *        r.Mr as "converged" and divides by any p.Ap) the solve stops with
 *        BAD_GAMMA when r.Mr is negative or not finite and with BAD_PAP when
 *        p.Ap is zero or not finite (checked before that iteration's updates,
 *        so x is the last good iterate); a negative p.Ap is divided by, as in
 *        the reference.
 * Once `done` is set every kernel below is a no-op, so the host may run ahead
 * and poll [7] asynchronously; unless one of the two breakdowns occurs, the
 * iterate and the iteration count are exactly those of a loop that tests the
 * condition of cg.py:68-73 every iteration.
 * No-op means: the vectors and `scalars` keep their bits.  Phase 2 starts the
 * next solve whatever [7] holds.  The `partials` an operator accumulates into
 * are workspace, not state: phases 1, 2 and 5 of sfem_cg_scalars clear them
 * whether `done` is set or not, because the apply that ran ahead of the flag
 * has added to them.  sfem_cg_flush_x is not guarded: it runs after the solve
 * has stopped.
 *
 * sfem_dot:            *result  = sum a*b          (clears result first)
 * sfem_dot_accumulate: *result += sum a*b
 * sfem_cg_scalars:     phase 2 = init (after b.b and gamma0 are in place),
 *                      phase 0 = after p.Ap, phase 1 = end of iteration,
 *                      phase 3 = p.Ap <- sum of the SFEM_DOT_SLOTS partial
 *                      sums written by sfem_helmholtz_apply (`partials`);
 *                      phase 4 = phase 3 then phase 0 in one launch;
 *                      phase 5 = [close the previous iteration as phase 1
 *                      would, if one is open: scalars[9]] then phase 4, and
 *                      `partials` is cleared at once: ONE scalar launch per
 *                      iteration, placed between the apply and the updates;
 *                      the done flag is then raised one (harmless) apply
 *                      late; phase 6 = close the open iteration now (before
 *                      the host reads [0], [7] or [8]);
 *                      phase 7 = fold the striped r.r (below) into [2] now,
 *                      before the caller corrects or all-reduces it;
 *                      phases 1 and 2 clear `partials` when it is given
 *                      gamma_new is scalars[2] PLUS the SFEM_CG_RR_SLOTS partial
 *                      sums scalars[16..80): sfem_cg_update_r with fuse_rr = 2
 *                      spreads its per-workgroup r.r sums over them (one
 *                      address would serialise 32 k atomics); every consumer
 *                      (update_p, update_xp, the closing phases) adds them up,
 *                      the closing phases clear them
 * sfem_cg_update_xr:   x += alpha p; r -= alpha Ap;  (cg.py:80-81)
 *                      fuse_rr != 0 also accumulates gamma_new += r.r (M = I)
 * sfem_cg_update_p:    p = z + beta p                (cg.py:84-85)
 * sfem_cg_update_r / sfem_cg_update_xp: the same two updates regrouped into
 *                      8 instead of 9 vector passes (bitwise the same result):
 *                      r -= alpha Ap (+ gamma_new += r.r), then, once beta is
 *                      known,  x += alpha p;  p = z + beta p
 * sfem_cg_update_r_mean / sfem_cg_update_xp_mean: the same pair for the
 *                      preconditioner  M r = r - (w . r / total) 1  (the mean
 *                      projection of the pressure solve, navier_stokes.py:
 *                      73-78, w = B 1, total = 1 . B 1) without storing z = M r:
 *                      update_r_mean also sums r.r (striped slots), 1.r and w.r
 *                      (`sums`: SFEM_CG_MEAN_SUMS device doubles, zero before
 *                      the first iteration, owned by the solve); update_xp_mean
 *                      forms c = w.r / total, gamma_new = r.r - c 1.r, beta, and
 *                      p = (r - c) + beta p.  9 vector passes per iteration
 *                      instead of 12.  The closing phases of sfem_cg_scalars
 *                      pick up gamma_new - r.r from scalars[11].               */
#define SFEM_CG_NSCALARS_NAMED 16 /* [0..16): the named scalars above      */
#define SFEM_CG_RR_SLOTS 64       /* [16..80): partial sums of gamma_new     */
#define SFEM_CG_NSCALARS (SFEM_CG_NSCALARS_NAMED + SFEM_CG_RR_SLOTS)
#define SFEM_CG_MEAN_SUMS (4 * SFEM_CG_RR_SLOTS) /* 2 parities x (1.r, w.r) */
#define SFEM_CG_STATUS_RUNNING 0.0
#define SFEM_CG_STATUS_CONVERGED 1.0
#define SFEM_CG_STATUS_MAXITER 2.0
#define SFEM_CG_STATUS_BAD_PAP 3.0
#define SFEM_CG_STATUS_BAD_GAMMA 4.0
int sfem_dot(const void* a, const void* b, int64_t count, double* result,
             int dtype, sfem_stream_t stream);
int sfem_dot_accumulate(const void* a, const void* b, int64_t count,
                        double* result, int dtype, sfem_stream_t stream);
/* *result += scale * sum_i w[i] * sum_k a[idx[i], k] b[idx[i], k]: the interface
 * correction that turns the plain local dot of two partition-consistent
 * vectors into this rank's share of the global inner product (scale = -1,
 * w = 1 - 1/holders).  a, b: (N,) or (N, ncomp) views with the given strides. */
int sfem_dot_indexed(const void* a, const void* b, const int64_t* idx,
                     const double* w, int64_t count, int ncomp,
                     int64_t node_stride, int64_t comp_stride, double scale,
                     double* result, int dtype, sfem_stream_t stream);
/* out = w - (b . w / total) 1: the nullspace projection of the pressure
 * preconditioner (navier_stokes.py:73-78 with b = B 1, total = 1 . B 1).
 * Two launches; `partials`: SFEM_DOT_SLOTS device doubles of workspace (need
 * not be cleared).  `out` may alias `w`.  `dot_result`: NULL, or one device
 * double that accumulates w . out (the r . z of a CG preconditioned by this
 * projection: its separate dot pass disappears).                             */
int sfem_subtract_weighted_mean(const void* w, const void* b, double total,
                                void* out, double* partials, int64_t count,
                                double* dot_result, int dtype,
                                sfem_stream_t stream);
int sfem_cg_scalars(double* scalars, int phase, double maxiter, double tol,
                    double atol, double* partials, sfem_stream_t stream);
int sfem_cg_update_xr(void* x, void* r, const void* p, const void* ap,
                      int64_t count, double* scalars, int fuse_rr, int dtype,
                      sfem_stream_t stream);
int sfem_cg_update_p(void* p, const void* z, int64_t count, double* scalars,
                     int dtype, sfem_stream_t stream);
int sfem_cg_update_r(void* r, const void* ap, int64_t count, double* scalars,
                     int fuse_rr, int dtype, sfem_stream_t stream);
int sfem_cg_update_xp(void* x, void* p, const void* z, int64_t count,
                      double* scalars, int dtype, sfem_stream_t stream);
/* Reproducible inner products.  sfem_cg_scalars_n = sfem_cg_scalars reading
 * `num_partials` STORED partial sums of p.Ap (sfem_helmholtz_args.dot_slots;
 * phases 3, 4, 5: summed in a fixed order, not cleared), plus phase 8:
 * gamma_new (scalars[2]) <- the fixed-order sum of `num_partials` stored
 * per-workgroup sums of r.r.  sfem_cg_update_r_layered with rr_partials != NULL
 * (fuse_rr != 0) stores its workgroups' sums there instead of accumulating them
 * atomically; `*num_rr` receives the number of workgroups (<= rr_capacity, the
 * launch is sized to fit).  A CG iteration built from these and the layered
 * apply is bitwise reproducible from run to run.                              */
/* `partials` must have room for num_partials + SFEM_FOLD_GROUPS doubles: long
 * sums are taken in two fixed-order stages through the scratch behind them.   */
#define SFEM_FOLD_GROUPS 256
int sfem_cg_scalars_n(double* scalars, int phase, double maxiter, double tol,
                      double atol, double* partials, int64_t num_partials,
                      sfem_stream_t stream);
int sfem_cg_update_r_layered_det(void* r, const void* ap_ext, int64_t count,
                                 const int64_t* layer_len,
                                 const int64_t* layer_off, int num_layers,
                                 const uint8_t* layer_masks,
                                 const int64_t* mask_off,
                                 double* scalars, double* rr_partials,
                                 int64_t rr_capacity, int64_t* num_rr,
                                 int dtype, sfem_stream_t stream);
/* Lazy solution update: sfem_cg_update_xp with x touched every m-th iteration
 * only.  `pring`: m direction vectors, slot s at pring + s * ring_stride
 * (elements; ring_stride a multiple of 16 bytes); p_k lives in slot k mod m,
 * k = scalars[8], and  p_{k+1} = z + beta p_k  goes to the next slot.  When
 * (k + 1) mod m = 0 the pending terms are added,
 *   x = (((x + alpha_{k-m+1} p_{k-m+1}) + ...) + alpha_k p_k),
 * in the order and with the roundings of the iteration-by-iteration update
 * (cg.py:80): bitwise the same x, (4 m + 1) / m vector passes per iteration
 * instead of 5.  `lazy`: 1 + SFEM_CG_LAZY_MAX device doubles owned by the
 * solve, zero before the first iteration ([0] = iterations already in x,
 * [1 + s] = alpha of slot s).  sfem_cg_flush_x adds what is still pending
 * after scalars[8] iterations (call it before reading x; the open iteration
 * of the one-scalar-launch scheme must be closed first: sfem_cg_scalars
 * phase 6).                                                                  */
#define SFEM_CG_LAZY_MAX 8
int sfem_cg_update_xp_lazy(void* x, void* pring, int64_t ring_stride,
                           const void* z, int64_t count, double* scalars,
                           double* lazy, int m, int dtype,
                           sfem_stream_t stream);
int sfem_cg_flush_x(void* x, const void* pring, int64_t ring_stride,
                    int64_t count, const double* scalars, double* lazy, int m,
                    int dtype, sfem_stream_t stream);
/* Layered assembly (sfem_helmholtz_args.layered_extent): the operator result
 * is an EXTENDED vector  [ count nodal values | layer 1 | layer 2 | ... ];
 * layer k (k = 0 .. num_layers-1 here) holds further contributions to the
 * nodes [0, layer_len[k]) and starts at element layer_off[k] of the vector
 * (HOST arrays; lengths and offsets multiples of 16 bytes, lengths not
 * increasing, at most SFEM_MAX_LAYERS).  The assembled value of node i is
 *   ext[i] + sum_{k : i < layer_len[k]} ext[layer_off[k] + i],
 * added in layer order -- the direct-stiffness sum of core/gather_scatter.py:
 * 130-133 in a fixed order: no atomics, no cleared range, bitwise reproducible.
 * sfem_cg_update_r_layered = sfem_cg_update_r (cg.py:81) reading Ap that way,
 * where it streams Ap anyway; sfem_fold_layers writes the assembled values
 * back into ext[0 .. count) for every other consumer.                         */
#define SFEM_MAX_LAYERS 15
/* layer_masks / mask_off (optional, NULL = read every layer in full): one byte
 * per SFEM_LAYER_CHUNK nodes of a layer, layer k's bytes starting at
 * layer_masks[mask_off[k]] (device array, host offsets; mask_off[k] < 0 = no
 * mask for that layer); 0 = no element writes into the chunk (it holds zeros
 * and is not read).                                                          */
#define SFEM_LAYER_CHUNK 512
int sfem_cg_update_r_layered(void* r, const void* ap_ext, int64_t count,
                             const int64_t* layer_len,
                             const int64_t* layer_off, int num_layers,
                             const uint8_t* layer_masks,
                             const int64_t* mask_off, double* scalars,
                             int fuse_rr, int dtype, sfem_stream_t stream);
int sfem_fold_layers(void* out_ext, int64_t count, const int64_t* layer_len,
                     const int64_t* layer_off, int num_layers, int dtype,
                     sfem_stream_t stream);
/* The same at `num_idx` DISTINCT nodes idx[] (negative entries skipped), and
 * the folded layer slots are cleared: a partitioned operator makes its
 * interface values whole before it packs them for the neighbours
 * (core/gather_scatter.py:247-248), later consumers of the layers find zeros. */
int sfem_fold_layers_at(void* out_ext, const int64_t* idx, int64_t num_idx,
                        int64_t count, const int64_t* layer_len,
                        const int64_t* layer_off, int num_layers, int dtype,
                        sfem_stream_t stream);
int sfem_cg_update_r_mean(void* r, const void* ap, const void* w,
                          int64_t count, double* scalars, double* sums,
                          int dtype, sfem_stream_t stream);
int sfem_cg_update_xp_mean(void* x, void* p, const void* r, int64_t count,
                           double* scalars, double* sums, double total,
                           int dtype, sfem_stream_t stream);
/* Element-wise fast diagonalisation solve: for every element e
 *   z_e = (S_0 (x) .. (x) S_{d-1}) [ w_e .* (S_0 (x) .. (x) S_{d-1})^T r_e ]
 * r_e / z_e: the Pp^ndim values of element e at r[pel[e][.]] (pel NULL: element
 * e owns the contiguous range [e Pp^d, (e + 1) Pp^d)), lexicographic, axis 0
 * slowest; S (num_cases, Pp, Pp) eigenvector matrices (rows = nodes, columns =
 * modes), cases (ndim, E): which one element e takes along its axis a; w
 * (E, Pp^d) the (pseudo-)inverted eigenvalues.  The local part of the opt-in
 * pressure preconditioner (swirl_fem_amd/navier_stokes/
 * pressure_preconditioner.py) for the reference's hook
 * navier_stokes/navier_stokes.py:354, :449-452.  Pp <= 10.                   */
int sfem_fdm_solve(const void* r, void* z, const int64_t* pel, const void* S,
                   const int32_t* cases, const void* inv_eigenvalues,
                   int64_t num_elements, int ndim, int Pp, int dtype,
                   sfem_stream_t stream);
/* The same solve that also hands back, per element, elem_sum[e] = sum of r
 * over the element (the restriction R_0 r of the coarse level) and, when
 * `weighted_sum` is given, weighted_sum[e] = sum_i weights[node] z[node] (the
 * element's share of the mean projection that closes the preconditioner):
 * two vector passes less per application.                                    */
int sfem_fdm_solve_sums(const void* r, void* z, const int64_t* pel,
                        const void* S, const int32_t* cases,
                        const void* inv_eigenvalues, const void* weights,
                        void* elem_sum, void* weighted_sum,
                        int64_t num_elements, int ndim, int Pp, int dtype,
                        sfem_stream_t stream);
/* z[e n + i] += yc[e] - shift[e / elems_per_member] (element e owns the nodes
 * [e n, (e + 1) n)): coarse correction and mean removal in one pass; `shift`
 * is a device array (one value per ensemble member, 1 without ensembles).    */
int sfem_add_element_constants(void* z, const void* yc, const void* shift,
                               int64_t num_elements, int n,
                               int64_t elems_per_member, int dtype,
                               sfem_stream_t stream);
/* x = q(D^-1 A) D^-1 b: `steps` steps of the Chebyshev iteration for the
 * interval [lmin, lmax] of the Jacobi-scaled sparse matrix A, a FIXED
 * polynomial (no inner products; linear, symmetric positive definite whenever
 * lmax bounds the spectrum): the coarse solve of the same preconditioner.
 * A: n rows of `width` entries, column-major (entry k of row i at
 * [k * n + i]; unused entries: value 0, any valid column); dinv = 1 / diag(A);
 * work: 3 n reals.  One launch per step.                                      */
int sfem_ell_chebyshev(const int32_t* cols, const void* vals, const void* dinv,
                       const void* b, void* x, void* work, int64_t n,
                       int width, int steps, double lmin, double lmax,
                       int dtype, sfem_stream_t stream);
/* --------------------------------------------- CG for an ensemble (vmap) ---
 * B independent CG recurrences in one set of launches: what the reference
 * gets from jax.vmap of its solver step over an ensemble (niles/train.py:232,
 * :262-264).  Member m owns the contiguous range [m len, (m + 1) len) of every
 * vector (B disjoint copies of the mesh seen as one mesh, so the operator
 * kernels serve all members in one launch unchanged) and the
 * SFEM_ENS_NSCALARS doubles at scalars + m SFEM_ENS_NSCALARS, same slots as
 * the single solve above ([0] gamma [1] p.Ap [3] alpha [4] beta [5] b.b
 * [6] atol2 [7] done [8] iterations [9] active in this iteration [10] status;
 * [12] c = w.r / total of the iteration, written by sfem_ens_close_mean).
 * Each member follows linalg/cg.py:60-97 with its own step lengths and stop
 * test; a member that has stopped is a no-op from then on.  Inner products are
 * stored partial sums, `partials`: members x 2 x SFEM_ENS_GROUPS doubles,
 * added in index order by the consumers (no atomics, nothing to clear).
 * One iteration:
 *     Ap = A p;  sfem_ens_dot(p, Ap, which = 0);  sfem_ens_update_r;
 *     z = M r;   sfem_ens_dot(r, z, which = 1);   sfem_ens_close;
 *     sfem_ens_update_xp
 * and before the first: sfem_ens_dot(b, b, 0), sfem_ens_dot(r, z, 1),
 * sfem_ens_init.  len = 0 is allowed everywhere: sfem_ens_dot then stores
 * zeros (a and b may be NULL), the entry points with vectors do nothing.     */
#define SFEM_ENS_NSCALARS 16
#define SFEM_ENS_GROUPS 32
#define SFEM_ENS_MAX_MEMBERS 4096
int sfem_ens_dot(const void* a, const void* b, int64_t len, int members,
                 double* partials, int which, int dtype, sfem_stream_t stream);
int sfem_ens_init(double* scalars, const double* partials, int members,
                  double maxiter, double tol, double atol,
                  sfem_stream_t stream);
/* r -= alpha Ap, alpha = gamma / p.Ap from the partial sums                  */
int sfem_ens_update_r(void* r, const void* ap, int64_t len, int members,
                      const double* scalars, const double* partials,
                      int dtype, sfem_stream_t stream);
/* closes the iteration of every member: alpha, beta, gamma <- gamma_new,
 * counter, stop test (cg.py:68-73 + the breakdown guards of the single solve) */
int sfem_ens_close(double* scalars, const double* partials, int members,
                   double maxiter, sfem_stream_t stream);
/* x += alpha p;  p = z + beta p  for the members active in this iteration    */
int sfem_ens_update_xp(void* x, void* p, const void* z, int64_t len,
                       int members, const double* scalars, int dtype,
                       sfem_stream_t stream);
/* The same iteration for M r = r - (w . r / total) 1 per member (w: ONE
 * member's weights, len values) without storing z = M r, as
 * sfem_cg_update_r_mean / sfem_cg_update_xp_mean do for the single solve:
 *     Ap = A p;  sfem_ens_dot(p, Ap, 0);  sfem_ens_update_r_mean;
 *     sfem_ens_close_mean;  sfem_ens_update_xp_mean
 * `sums`: members x 3 x SFEM_ENS_GROUPS doubles (r.r, 1.r, w.r); the mean c of
 * the iteration is left in scalars[12].                                      */
int sfem_ens_update_r_mean(void* r, const void* ap, const void* w, int64_t len,
                           int members, const double* scalars,
                           const double* partials, double* sums, int dtype,
                           sfem_stream_t stream);
int sfem_ens_close_mean(double* scalars, const double* partials,
                        const double* sums, double total, int members,
                        double maxiter, sfem_stream_t stream);
int sfem_ens_update_xp_mean(void* x, void* p, const void* r, int64_t len,
                            int members, const double* scalars, int dtype,
                            sfem_stream_t stream);
/* out_m = w_m - (b . w_m / total) 1 for every member m (b: one member's
 * weights, len values; partials: members x SFEM_ENS_GROUPS doubles): the mean
 * projection of the pressure solve (navier_stokes.py:73-78) per member.      */
int sfem_ens_subtract_weighted_mean(const void* w, const void* b, double total,
                                    void* out, double* partials, int64_t len,
                                    int members, int dtype,
                                    sfem_stream_t stream);
/* ------------------------------------------- Jacobi preconditioning ---
 * sfem_helmholtz_diag: the element diagonals of the mass and stiffness parts
 * of the operator sfem_helmholtz_apply / sfem_helmholtz_local apply, in the
 * same form (G = w detJ J^-1 J^-T and W = w detJ, stored per point for
 * SFEM_GEO_POINT elements -- geo, geo_index as in sfem_helmholtz_args -- or
 * evaluated from the (E, 24) multilinear coefficients geo_elem for
 * SFEM_GEO_AFFINE / SFEM_GEO_MULTILINEAR elements at the quadrature `nodes`).
 * Node i = (i0, i1[, i2]) of element e, axis 0 slowest:
 *   mass_out[e, i]  = sum_q W(q) prod_c B(q_c, i_c)^2
 *   stiff_out[e, i] = sum_q sum_ab G_ab(q) g_a(q) g_b(q),
 *                     g_a = prod_c (c == a ? Dt(q_c, i_c) : B(q_c, i_c))
 * with B = bmat, the (Q, P) interpolation from the P nodes to the Q
 * quadrature points, and Dt = dtil its derivative (Q, P) (D_q B).  bmat = NULL:
 * collocated (Q = P, B = I, dtil = the nodal differentiation matrix).  Only
 * the listed elements' rows are written.  Either output may be NULL.  All
 * pointers are device pointers.                                            */
typedef struct sfem_diag_args {
  void* mass_out;           /* (E, P^d) or NULL                              */
  void* stiff_out;          /* (E, P^d) or NULL                              */
  const void* geo;          /* stored factors (SFEM_GEO_POINT) or NULL       */
  const void* geo_elem;     /* (E, 24) multilinear coefficients or NULL      */
  const int32_t* geo_index; /* (E,) slot of element in `geo`, or NULL        */
  const int32_t* elem_list; /* (num_listed,) element ids, or NULL = all      */
  const void* bmat;         /* (Q, P) or NULL (collocated)                   */
  const void* dtil;         /* (Q, P)                                         */
  const void* weights;      /* (Q,) 1D quadrature weights                    */
  const void* nodes;        /* (Q,) 1D quadrature points in [-1, 1]          */
  int64_t num_elements;
  int64_t num_listed;
  int ndim;                 /* 2 or 3                                         */
  int P;                    /* 2..12                                          */
  int Q;                    /* P..16 (ignored when collocated)                */
  int dtype;
  int geo_mode;             /* SFEM_GEO_POINT / _AFFINE / _MULTILINEAR        */
  /* Variable coefficients as in sfem_helmholtz_args (NULL / 0 = off): G of   */
  /* point q of element e is scaled by kappa, W by sigma; SFEM_COEF_POINT     */
  /* arrays are (E, Q^d) at the quadrature points (P^d when collocated).      */
  const void* kappa;
  const void* sigma;
  int coef_mode;
} sfem_diag_args;
int sfem_helmholtz_diag(const sfem_diag_args* args, sfem_stream_t stream);
/* CG with M r = dinv (.) r folded into the two vector updates (z = M r is
 * never stored), the Jacobi form of sfem_cg_update_r / sfem_cg_update_xp:
 *   sfem_cg_update_r_jacobi : r -= alpha Ap;  gamma_new += r . (dinv (.) r)
 *   sfem_cg_update_xp_jacobi: x += alpha p;   p = dinv (.) r + beta p
 * `dinv`: (period,) shared by the `ncomp` components of a component-major
 * field (component c at c * period; ncomp > 1 needs period to be a multiple
 * of the 16-byte vector width).  update_r_jacobi takes Ap in the layered form
 * of sfem_cg_update_r_layered (num_layers = 0: plain Ap; layers need
 * ncomp = 1).  rz_partials = NULL: the r.z sums go to the striped slots of
 * `scalars` (as sfem_cg_update_r with fuse_rr = 2); otherwise one STORED sum
 * per workgroup (at most rz_capacity; *num_rz receives the count) for the
 * fixed-order sum of sfem_cg_scalars_n phase 8 -- bitwise reproducible.   */
int sfem_cg_update_r_jacobi(void* r, const void* ap_ext, const void* dinv,
                            int64_t period, int ncomp,
                            const int64_t* layer_len,
                            const int64_t* layer_off, int num_layers,
                            const uint8_t* layer_masks,
                            const int64_t* mask_off, double* scalars,
                            double* rz_partials, int64_t rz_capacity,
                            int64_t* num_rz, int dtype, sfem_stream_t stream);
int sfem_cg_update_xp_jacobi(void* x, void* p, const void* r,
                             const void* dinv, int64_t period, int ncomp,
                             double* scalars, int dtype,
                             sfem_stream_t stream);
/* ------------------------------------------------------- p-multigrid ---
 * Transfers between two polynomial orders of the same elements
 * (linalg/pmg.py), sizes in points per direction, 2 <= pc < pf <= 13, ndim 2
 * or 3.  The pairs of the default schedules p -> p / 2 (points 3->2, 4->2,
 * 5->3, 6->3, 7->4, 8->4, 9->5, 10->5, 11->6, 12->6, 13->7) are compiled with
 * fixed sizes, other pairs run with run-time sizes.  One wave per element.
 *   cidx (E, pc^ndim), fidx (E, pf^ndim): int32 index rows; a Dirichlet node
 *       is stored as ~id (reads as 0; prolong stores 0 there);
 *   owner (E, ceil(pf^ndim / 32)) uint32: bit t of element e set iff e owns
 *       its local fine node t; every fine node has exactly one owner;
 *   mat (pf, pc) row-major: the 1D interpolation from the coarse to the fine
 *       points (Lagrange basis of the coarse points at the fine points).
 * sfem_pmg_prolong:  uf = P uc (add != 0: uf += P uc, Dirichlet nodes left as
 *                    they are), written once per fine node at its owner: no
 *                    atomics, no element-local result in memory;
 * sfem_pmg_restrict: rc_local[e] = the transposed contraction of the owned
 *                    fine values of element e, coarse Dirichlet slots 0;
 *                    sfem_scatter_csr over the coarse mesh sums them in a
 *                    fixed order, and the two together are exactly P^T.     */
int sfem_pmg_prolong(const void* uc, void* uf, const int32_t* cidx,
                     const int32_t* fidx, const uint32_t* owner,
                     const void* mat, int64_t num_elements, int ndim, int pc,
                     int pf, int add, int dtype, sfem_stream_t stream);
int sfem_pmg_restrict(const void* rf, void* rc_local, const int32_t* cidx,
                      const int32_t* fidx, const uint32_t* owner,
                      const void* mat, int64_t num_elements, int ndim, int pc,
                      int pf, int dtype, sfem_stream_t stream);
/* The same transfers for nodal vector fields with ndim components per node,
 * dense (N, ndim): the flat vectors of the elasticity solve
 * (linalg/pmg_elasticity.py).  Sizes, pairs, `owner` and `mat` as above.
 * Fixed components are per component, not per node, so
 *   cidx (E, pc^ndim), fidx (E, pf^ndim): plain int32 ids in [0, N), and
 *   cfix (N_c,), ffix (N_f,) uint8: bit c of a node's byte is set iff its
 *       component c is fixed (reads as 0; prolong stores 0 there).
 * One launch, one wave per element: the components go one after another
 * through the same LDS buffers, so the index rows, owner words and flag bytes
 * are fetched from memory once per element.
 * sfem_pmg_prolong_vec:  uf (N_f, ndim) = P uc (N_c, ndim) per component
 *                    (add != 0: uf += P uc, fixed fine components left as
 *                    they are), every fine node written at its owner only;
 * sfem_pmg_restrict_vec: rc_local (E, pc^ndim, ndim) = the transposed
 *                    contraction of the owned, non-fixed fine values, fixed
 *                    coarse slots 0; sfem_scatter_csr with ncomp = ndim sums
 *                    them in a fixed order.  No atomics.
 * Status codes as sfem_pmg_prolong / sfem_pmg_restrict.                     */
int sfem_pmg_prolong_vec(const void* uc, void* uf, const int32_t* cidx,
                         const int32_t* fidx, const uint32_t* owner,
                         const uint8_t* cfix, const uint8_t* ffix,
                         const void* mat, int64_t num_elements, int ndim,
                         int pc, int pf, int add, int dtype,
                         sfem_stream_t stream);
int sfem_pmg_restrict_vec(const void* rf, void* rc_local, const int32_t* cidx,
                          const int32_t* fidx, const uint32_t* owner,
                          const uint8_t* cfix, const uint8_t* ffix,
                          const void* mat, int64_t num_elements, int ndim,
                          int pc, int pf, int dtype, sfem_stream_t stream);
/* One step of the Chebyshev-Jacobi smoother in one pass over n values:
 *   mode 0:  d = a d + c dinv (b - ax);  x += d
 *   mode 1:  d = c dinv b;  x = d          (start from x = 0: ax, x, d unread)
 *   mode 2:  r = b - ax                    (the residual before restriction)
 *   mode 3:  d = c dinv (b - ax);  x += d  (d unread)
 * dinv is 0 on Dirichlet rows.  Pointers a mode does not use may be NULL.   */
int sfem_cheb_step(void* x, void* d, const void* ax, const void* b,
                   const void* dinv, void* r, double a, double c, int64_t n,
                   int mode, int dtype, sfem_stream_t stream);
/* CG that stops on the true-residual norm r.r instead of r.Mr (a V-cycle M
 * approximates A^-1, so r.Mr is an energy norm), with reproducible inner
 * products: sfem_pmg_dot2 stores, per workgroup g < groups, the sum of a.b at
 * partials[g] and (c != NULL) of a.c at partials[groups + g];
 * sfem_pmg_cg_scalars adds n stored partials in a fixed order:
 *   phase 3: [5] b.b = sum partials[0, n)
 *   phase 2: init: [13] r.r = sum [0, n), [0] gamma = r.z = sum [n, 2n),
 *            atol2, counters, status; done if r.r <= atol2
 *   phase 0: [1] p.Ap = sum [0, n); alpha; [2] = 0 (BAD_PAP as phase 0 of
 *            sfem_cg_scalars)
 *   phase 4: [13] r.r = sum [0, n), [2] gamma_new = r.z = sum [n, 2n)
 *   phase 1: close: beta, gamma <- gamma_new, ++iterations; done when
 *            r.r <= atol2, r.z is negative / not finite, or maxiter.
 * The scalar slots are those of sfem_cg_scalars, so sfem_cg_update_r
 * (fuse_rr = 0), sfem_cg_update_r_layered and sfem_cg_update_xp run
 * unchanged between them.                                                    */
int sfem_pmg_dot2(const void* a, const void* b, const void* c, int64_t n,
                  double* partials, int groups, int dtype,
                  sfem_stream_t stream);
int sfem_pmg_cg_scalars(double* scalars, int phase, const double* partials,
                        int64_t n, double maxiter, double tol, double atol,
                        sfem_stream_t stream);
/* y = A x on some rows of an ELL matrix in the layout of sfem_ell_chebyshev
 * (n rows of `width` entries, column-major: entry k of row i at [k n + i];
 * every column index in [0, n)): the rows [row_begin, row_end) when `rows` is
 * NULL, else the `num_rows` rows listed in `rows` (int32, each in [0, n),
 * no repeats).  Rows not named are not written.  The coarse Chebyshev step of
 * p-multigrid on a partition (linalg/pmg.py): interface rows, exchange posted,
 * interior rows, exchange finished, sfem_cheb_step.  A row range runs 2
 * (fp64) / 4 (fp32) rows per lane with 16-byte loads of the values when n is
 * a multiple of that; row lists one row per lane.                            */
int sfem_ell_spmv(const int32_t* cols, const void* vals, const void* x,
                  void* y, int64_t n, int width, int64_t row_begin,
                  int64_t row_end, const int32_t* rows, int64_t num_rows,
                  int dtype, sfem_stream_t stream);
/* ---------------------------------------------------- boundary facets ---
 * Integrals over the facets of a physical group (core/fespace.py
 * boundary_points / boundary_covector; the call site is the inhomogeneous
 * Dirichlet / Neumann data that the reference leaves as a TODO,
 * swirl_fem/examples/poisson.py:79-90, served by examples/helmholtz.py).
 * A facet is a (d-1)-dimensional isoparametric element with its own nodes,
 * integrated with the space's 1D rule in each facet direction.  One wave per
 * facet.  Accepted: 2 <= p1 <= 16 and 1 <= q <= 16 (SFEM_EINVAL otherwise,
 * for num_facets = 0 too).  The 24 pairs with q = p1 or p1 + 1, 2 <= p1 <= 13,
 * are compiled with fixed sizes; every other pair (q < p1, q > p1 + 1,
 * p1 >= 14) runs with run-time sizes.
 *   coords (N, ndim), facets (F, p1^(ndim-1)) int32 node ids in [0, N),
 *       lexicographic on the facet;
 *   bmat (q, p1) row-major: B, the 1D interpolation from the nodes to the
 *       points; dmat (q, p1): D_q = B D; weights (q): the 1D rule.
 * sfem_boundary_geom:     xq (F, q^(ndim-1), ndim) the physical points;
 *                         wj (F, q^(ndim-1)) = w_s w_t |x_s x x_t| (ndim 3)
 *                         or w_s |x_s| (ndim 2);
 * sfem_boundary_covector: out_local (F, p1^(ndim-1)) = (B (x) B)^T (wj g),
 *                         g the values at the points (F, q^(ndim-1)), or
 *                         (nodal != 0) nodal values (N,) gathered through
 *                         `facets` and interpolated by B (x) B; summed per
 *                         node by sfem_scatter_csr in a fixed order.         */
int sfem_boundary_geom(const void* coords, const int32_t* facets,
                       int64_t num_facets, const void* bmat, const void* dmat,
                       const void* weights, int ndim, int p1, int q, void* xq,
                       void* wj, int dtype, sfem_stream_t stream);
int sfem_boundary_covector(const void* g, int nodal, const int32_t* facets,
                           int64_t num_facets, const void* wj,
                           const void* bmat, int ndim, int p1, int q,
                           void* out_local, int dtype, sfem_stream_t stream);
/* The facet mass operator of a Robin term (core/fespace.py boundary_mass):
 * M_f = (B (x) B)^T diag(aw) (B (x) B), aw (F, q^(ndim-1)) = alpha wJ at the
 * points, formed once by the caller.  Same sizes, pairs and launch shape as
 * the covector.  `facets` may store a node as ~id (a Dirichlet node): that
 * slot reads 0 and its output is 0, so the term loses the Dirichlet rows and
 * columns, like the masked volume operator.
 * sfem_boundary_mass_apply: out_local (F, p1^(ndim-1)) = scale M_f u_f, u_f
 *                           gathered from u (N,) through `facets`;
 * sfem_boundary_mass_diag:  out_local (F, p1^(ndim-1)) = scale diag(M_f) =
 *                           scale sum_q aw_q prod_c B(q_c, i_c)^2;
 * sfem_boundary_add_rows:   out[rows[r]] += sum over s in [offsets[r],
 *                           offsets[r+1]) of local[slots[s]], summed in slot
 *                           order, for r < num_rows (rows int32, distinct;
 *                           offsets int64 (num_rows + 1); slots int32).  Only
 *                           the listed rows are read or written: the Robin
 *                           term costs O(boundary), with no atomics.         */
int sfem_boundary_mass_apply(const void* u, const int32_t* facets,
                             int64_t num_facets, const void* aw,
                             const void* bmat, int ndim, int p1, int q,
                             double scale, void* out_local, int dtype,
                             sfem_stream_t stream);
int sfem_boundary_mass_diag(const int32_t* facets, int64_t num_facets,
                            const void* aw, const void* bmat, int ndim, int p1,
                            int q, double scale, void* out_local, int dtype,
                            sfem_stream_t stream);
int sfem_boundary_add_rows(const void* local, const int32_t* rows,
                           const int64_t* offsets, const int32_t* slots,
                           int64_t num_rows, void* out, int dtype,
                           sfem_stream_t stream);
/* ---------------------------------------------------------------- BiCGStab ---
 * Right-preconditioned BiCGStab (linalg/bicgstab.py) for the non-symmetric
 * systems of an advective term: r is the true residual and the solve stops on
 * r.r <= max(tol^2 b.b, atol^2).  As in the CG core the scalars live in a
 * device array, `scalars` of SFEM_BICGSTAB_NSCALARS doubles, every kernel
 * returns at once when `done` is set and the host only polls:
 *   [0] rho = r0.r of the open iteration   [1] r0.r being summed   [2] alpha
 *   [3] omega   [4] beta   [5] r0.v   [6] s.s   [7] t.s   [8] t.t
 *   [9] r.r being summed   [10] b.b   [11] max(tol^2 b.b, atol^2)   [12] done
 *   [13] iterations   [14] status, SFEM_BICGSTAB_STATUS_*
 *   [15] the iteration stopped after its first half (s.s under the threshold:
 *        x += alpha phat, r = s, no second apply is read)
 *   [16] r.r of the last closed iteration
 * One iteration, with phat = M p and shat = M s (M = diag(dinv) is folded into
 * the kernels; dinv NULL: phat / shat are p / s themselves):
 *   sfem_bicgstab_update_p    p = r + beta (p - omega v); phat = dinv p
 *   v = A phat;  sfem_bicgstab_dot(r0, v, slot 5);  scalars phase 1: alpha
 *   sfem_bicgstab_update_s    s = r - alpha v; shat = dinv s; [6] += s.s
 *   scalars phase 2 (half-step test);  t = A shat
 *   sfem_bicgstab_dot(t, s, slot 7, two = 1)   [7] += t.s, [8] += t.t
 *   sfem_bicgstab_update_xr   omega = [7] / [8]; x += alpha phat + omega shat;
 *                             r = s - omega t; [9] += r.r, [1] += r0.r
 *   scalars phase 3           closes: beta, rho, counter, stop test
 * Phase 0 starts a solve from [10] = b.b, [9] = r.r, [1] = r0.r; p and v must
 * start as zeros.  rho = 0, r0.v = 0 and omega = 0 (t.s = 0 or t = 0) end the
 * solve with BAD_RHO / BAD_ALPHA / BAD_OMEGA before anything is divided by
 * them: x stays finite.                                                       */
#define SFEM_BICGSTAB_NSCALARS 32
#define SFEM_BICGSTAB_STATUS_RUNNING 0.0
#define SFEM_BICGSTAB_STATUS_CONVERGED 1.0
#define SFEM_BICGSTAB_STATUS_MAXITER 2.0
#define SFEM_BICGSTAB_STATUS_BAD_RHO 3.0
#define SFEM_BICGSTAB_STATUS_BAD_OMEGA 4.0
#define SFEM_BICGSTAB_STATUS_BAD_ALPHA 5.0
int sfem_bicgstab_scalars(double* scalars, int phase, double maxiter,
                          double tol, double atol, sfem_stream_t stream);
/* scalars[slot] += a.b (two != 0: also scalars[slot + 1] += a.a, and the pass
 * is skipped after a half-step stop)                                          */
int sfem_bicgstab_dot(const void* a, const void* b, int64_t count,
                      double* scalars, int slot, int two, int dtype,
                      sfem_stream_t stream);
int sfem_bicgstab_update_p(void* p, void* phat, const void* r, const void* v,
                           const void* dinv, int64_t count, double* scalars,
                           int dtype, sfem_stream_t stream);
int sfem_bicgstab_update_s(void* s, void* shat, const void* r, const void* v,
                           const void* dinv, int64_t count, double* scalars,
                           int dtype, sfem_stream_t stream);
int sfem_bicgstab_update_xr(void* x, void* r, const void* phat,
                            const void* shat, const void* s, const void* t,
                            const void* r0, int64_t count, double* scalars,
                            int dtype, sfem_stream_t stream);

/* y = a*x + b*y (plain fused vector update used outside the CG core)         */
int sfem_axpby(double a, const void* x, double b, void* y, int64_t count,
               int dtype, sfem_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif  /* SFEM_H_ */
