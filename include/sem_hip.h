/*
 * sem_hip.h -- C ABI of the MI355X spectral-element operator engine
 * (libsem_hip.so, built from spectralelementmethod_amd/csrc/).
 *
 * The reference (nchisholm/SpectralElementMethod) has no FFI: its hot path is
 * Python/NumPy classes.  Each entry point below replaces one piece of that
 * path; the reference interface it stands in for is cited per function
 * (paths relative to the reference checkout).  INTEGRATION.md shows the
 * ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - n = p + 1 GLL nodes per direction; element-local nodal arrays are
 *     [n][n] in lexicographic (xi0, xi1) order, C-contiguous, float64
 *     (sem/basis_functions.py:647, sem/mapping.py:113).
 *   - element->node map: uint32 [n_elem][n][n] (sem/discrete.py:1044).
 *   - DOF index = dpn * node + comp (sem/discrete.py:567-574).
 *   - Pointers named d_* are DEVICE pointers (caller-owned, e.g. PyTorch
 *     tensors); pointers named h_* are host pointers.
 *   - Every int-returning call returns SEM_OK (0) or a negative SEM_E_* code;
 *     sem_last_error() gives a thread-local message.
 *   - Work is enqueued on the caller's stream (hipStream_t passed as void*;
 *     NULL = the legacy default stream).  sem_apply and the vector kernels
 *     allocate nothing and do not synchronise (graph-capturable).
 */
#ifndef SEM_HIP_H
#define SEM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (mapped to the reference's Python exceptions) ---- */
#define SEM_OK 0
#define SEM_E_INVALID (-1)      /* ValueError      (sem/discrete.py:134, sem/basis_functions.py:358) */
#define SEM_E_NOTIMPL (-2)      /* NotImplementedError (sem/basis_functions.py:366-369, sem/mapping.py:110-111) */
#define SEM_E_DETJ (-3)         /* AssertionError detJ > 0 (sem/mapping.py:117) */
#define SEM_E_HIP (-4)          /* HIP runtime failure */
#define SEM_E_STATE (-5)        /* call order violated (e.g. apply before geometry) */

/* ---- operator kinds ---- */
#define SEM_OP_POISSON 0        /* scalar Laplacian Lse, examples/poisson.py:168-193 */
#define SEM_OP_AXISYM_STOKES 1  /* [Lve.w ; E2e.psi - Me.w], squirmer-axisymmetric.py:193-254,278-295 (Re=0) */
#define SEM_OP_AXISYM_NS 2      /* Re > 0 residual [Ae.w.psi + Lve.w ; E2e.psi - Me.w], squirmer:229-297 */
#define SEM_OP_AXISYM_NS_JVP 3  /* its Newton Jacobian (jac_l, squirmer:272-291) times a direction */

/* number of geometric factors per local node for an operator kind (3, 7 or 9) */
int sem_op_ncomp(int op_kind);

const char* sem_last_error(void);
const char* sem_version(void);

/* ------------------------------------------------------------------ */
/* Host-side basis data (C twins of the reference's 1-D basis layer)   */
/* ------------------------------------------------------------------ */

/* GLL nodes, barycentric and quadrature weights for 1 <= p <= 16, unfolded
 * from the stored non-negative half exactly as LagrangeGaussLobatto.__init__
 * (sem/basis_functions.py:349-393).  Orders 1..10 are the reference's
 * basis-data.hdf5 values; 11..16 come from its generator
 * sem/basis_data.py:19-109.  Each output has p+1 entries. */
int sem_gll_table(int p, double* h_nodes, double* h_bary, double* h_quad);

/* First-derivative matrix D1 (n*n, row-major) from nodes and barycentric
 * weights: BarycentricLagrange.__init__ (sem/basis_functions.py:213-219). */
int sem_diff_matrix(int n, const double* h_nodes, const double* h_bary, double* h_D);

/* Lagrange basis evaluated at points: B[i][j] = l_j(x_i) (n_x*n, row-major),
 * BarycentricLagrange.__call__ (sem/basis_functions.py:226-255). */
int sem_lagrange_eval(int n, const double* h_nodes, const double* h_bary,
                      int64_t n_x, const double* h_x, double* h_B);

/* Equispaced interpolation matrix V_eq (= B at linspace(-1,1,n),
 * sem/basis_functions.py:221-224) and its inverse (the lu_solve of
 * TensorProduct.compute_coeffs_grid_eq, sem/basis_functions.py:599-624). */
int sem_interp_eq_matrix(int n, const double* h_nodes, const double* h_bary,
                         double* h_Veq, double* h_Veq_inv);

/* C twins of sem/bary_interp.c:10-36 (legeval) and :39-90
 * (barycentric_lagrange, 2 <= n <= 17 here; the reference's table stops at
 * n = 9).  Interpolating exactly at a node returns the nodal value. */
double sem_legeval(double x, unsigned n);
double sem_barycentric_lagrange(const double* h_f, unsigned n, double x);

/* Node orderings of a cell-node map (host, no device): the reverse
 * Cuthill-McKee renumbering of DOFManager(mesh, rcm_order=True)
 * (sem/discrete.py:169-178 -> scipy.sparse.csgraph.reverse_cuthill_mckee on
 * the graph joining every two nodes of a cell, sem/discrete.py:142-167), run
 * on the cell map itself instead of materialising that graph (5.5e9 entries
 * at 1024^2 cells, p = 8).  h_cells: [n_cells][nloc] node ids.
 *   sem_node_degrees: scipy's degree of each node (row length + 1 for the
 *     diagonal; 0 for a node no cell references);
 *   sem_cuthill_mckee: Cuthill-McKee order (h_order[k] = k-th node) from
 *     h_seeds = argsort(degree) (the caller's sort, so ties follow numpy);
 *     RCM is h_order reversed.  Equal to scipy's on the same graph
 *     (tests/test_order.py). */
int sem_node_degrees(const uint32_t* h_cells, int64_t n_cells, int nloc, int64_t n_node,
                     int32_t* h_degree);
int sem_cuthill_mckee(const uint32_t* h_cells, int64_t n_cells, int nloc, int64_t n_node,
                      const int32_t* h_degree, const int64_t* h_seeds, int64_t* h_order);

/* ------------------------------------------------------------------ */
/* Operator context (one per GPU)                                      */
/* ------------------------------------------------------------------ */
typedef struct sem_ctx sem_ctx;

/* Replaces DOFManager(mesh, dofs_per_node, basis) bookkeeping
 * (sem/discrete.py:81-124) for the batched operator path. */
int sem_ctx_create(sem_ctx** out, int p, int64_t n_elem, int64_t n_node, int dpn, int device);
void sem_ctx_destroy(sem_ctx* ctx);

/* The same for a mesh of dimension ndim: 2 = quadrilaterals (sem_ctx_create),
 * 3 = hexahedra.  The reference's basis layer is N-dimensional
 * (TensorProduct.deriv / gradient, compute_coeffs_grid_eq,
 * sem/basis_functions.py:599-650; TensorQuadratureRule.xweight,
 * sem/quadratures.py:268-275; NCube, sem/geometry.py:32-216); only its 2x2
 * Jacobian inverse stops at 2-D (sem/mapping.py:110-111).  On a hexahedral
 * context (1 <= p <= 16, dpn = 1, Poisson; above p = 10 the equispaced ->
 * GLL transform runs as compensated passes, above p = 12 the action runs the
 * row form of the kernel by default):
 *   - element-local arrays are [n][n][n] in lexicographic (xi0, xi1, xi2)
 *     order, xi2 fastest; the map is uint32 [n_elem][n][n][n];
 *   - sem_geom_from_nodes takes nodes float64 [3][n_node] and stores the 6
 *     factors G_kl = detJxW sum_j invJ[k][j] invJ[l][j] per node;
 *     sem_geom_fields writes x_phys [E][3][n][n][n], J / invJ
 *     [E][3][3][n][n][n] (J[c][d] = d x_c / d xi_d, invJ = J^-1), detJ and
 *     detJxW [E][n][n][n]; sem_set_geom takes [E][6][n][n][n] in the order
 *     (00, 01, 02, 11, 12, 22);
 *   - sem_apply / sem_apply_dot / sem_diag / sem_assemble / sem_zero_shared /
 *     sem_pcg_solve work as on quadrilaterals (stored geometry; the column
 *     kernels by default, SEM_KERNEL_MFMA at p = 11..16, see sem_set_kernel;
 *     SEM_GEOM_NODAL, SEM_KERNEL_MFMA at other orders, node states and the
 *     axisymmetric kinds return SEM_E_NOTIMPL);
 *   - sem_plan_info: [0] workgroups, [1] zero list, [2] 0, [3] 1, [4]
 *     element slots per workgroup, [5] chains along xi0, [6] sub-chain length
 *     cap, [7] launch positions, [8] sub-chains, [9] seam nodes, [10] slotted
 *     writes, [11] plain stores, [12] threads per workgroup, [13] 3, [14]
 *     geometry ready, [15] action kernel (2 matrix-core form, 1 row form,
 *     0 three-block),
 *     [16] xi2 faces merged in LDS (z-merge), [17] xi1 faces merged in LDS
 *     too (y-merge): slots per row of the workgroup's slot grid, 0 = off,
 *     [18] template map: every element's node ids are its first node's id +
 *     one shared offset block, read as one base per element
 *     (SEM_HEX_TMAP=0 turns it off). */
int sem_ctx_create_nd(sem_ctx** out, int ndim, int p, int64_t n_elem, int64_t n_node, int dpn,
                      int device);

/* Basis of the operator: D (n*n, host) and 1-D quadrature weights w (n,
 * host): TensorProductQS.get_D1_matrices() / quad_rule.weights
 * (sem/basis_functions.py:156-162, sem/quadratures.py:246-252). */
int sem_set_basis(sem_ctx* ctx, const double* h_D, const double* h_w);

/* Element->node map (device, uint32 [n_elem][n][n]): the per-element
 * FiniteElement.node_ind gather/scatter index (sem/discrete.py:658-663,
 * 810-812).  The library keeps a repacked copy (coalesced per wavefront)
 * plus the list of element-boundary nodes; synchronises `stream`. */
int sem_set_map(sem_ctx* ctx, const uint32_t* d_e2n, void* stream);

/* sem_set_map for an operator that shares y with other operators applied in
 * stream order (e.g. partition-interface elements first, interior elements
 * second, so the interface sum can start early -- SURVEY.md §8(e)).
 * d_node_state (device uint8 [n_node], may be NULL):
 *   SEM_NODE_PRIOR  y[node] already holds the earlier operators' sum when this
 *                   one runs: its first touch adds (read-modify-write) and the
 *                   node is never zeroed;
 *   SEM_NODE_OTHER  a later operator writes y[node]: not zeroed here when this
 *                   operator does not reference it. */
#define SEM_NODE_PRIOR 1
#define SEM_NODE_OTHER 2
int sem_set_map_shared(sem_ctx* ctx, const uint32_t* d_e2n, const uint8_t* d_node_state,
                       void* stream);

/* Setup plan of the last sem_set_map (diagnostics): info[0] groups (one
 * wavefront of elements each), [1] zero-list length, [2] groups in
 * atomic-fallback chains, [3] mesh conforming (0/1), [4] elements per group,
 * [5] colour classes, [6] rounds of 4 groups per chain (one workgroup per
 * chain), [7] packed group slots, [8..16] chains per colour class (one launch
 * each; elements for the MFMA kernel), [17] kernel family (SEM_KERNEL_COLUMN
 * or SEM_KERNEL_MFMA), [18] bytes per packed map entry the Poisson column
 * kernel streams (2: 16-bit row offsets, used when every group row spans
 * < 4096 node ids; 4 otherwise; SEM_MAP16=0 in the environment forces 4).
 * [19] the Poisson geometry mode the action uses (SEM_GEOM_NODAL or
 * SEM_GEOM_STORED, AUTO resolved; nodal only once x_phys per node exists).
 * [20] scatter plan: 0 chains of consecutive elements (carry / merge codes),
 * 1 element-coloured chains (chosen when the element order defeats the chain
 * patterns: more than half of the groups would need atomics; SEM_PLAN=1 / 0
 * in the environment forces / forbids it), 2 one element per wavefront
 * (MFMA kernel), 4 the seam plan (Poisson, dofs_per_node == 1; AUTO where a
 * colour launch would be about one generation of resident workgroups or
 * less -- p >= 10, or few chains per colour; SEM_SEAM=1 / 0
 * forces / forbids): all chains in one launch in element order, nodes
 * written by several chains stored per writer colour and summed in colour
 * order by a second launch, bitwise equal to the colour launches; [5] is
 * then 1 and [8] the chain count.  (3 was a retired one-launch plan.)
 * 5: the n = 17 MFMA kernel's seam form (SEM_SEAM=1; measured slower than
 * its colour launches, which stay the default): every element in one launch in breadth-first
 * order, a node of several elements stored per element colour and summed
 * by the seam launch.
 * [21] the axisymmetric Stokes geometry mode (as [19]; 0 when
 * dofs_per_node != 2).  [22] seam nodes of the seam plan.  [23] 1 when the
 * chains use the block layout (structured numberings: a chain is [6]
 * stacked lines of elements, and the node row between two rounds is carried
 * in registers; SEM_BLOCK_ROUNDS=R in the environment forces R rounds, 0
 * turns it off), [24] the packed map entries so carried.
 * [25] 1 when the Poisson column kernels take D as compile-time constants:
 * sem_set_basis found the context's D equal to the baked standard GLL D
 * bit for bit (csrc/deo_const.h; 16-bit maps) at an order where that is
 * measured faster; SEM_CONST_D=0 / 1 in the environment
 * turns it off / on at every order.
 * [26] patterns of the 16-bit map's pattern table (0: one block of entries
 * per group): groups whose entries repeat share one copy and the map stream
 * shrinks to the per-row bases (SEM_MAP_PATTERNS=0 in the environment turns
 * it off; built for p >= 2).
 * Writes min(n_info, 27) values. */
int sem_plan_info(sem_ctx* ctx, int64_t* info, int n_info);

/* How the Poisson action obtains its geometric factors.
 *  SEM_GEOM_AUTO (default): NODAL for p = 1, 2, 4, 5, 8, STORED otherwise
 *    (per-order MI355X sweep at ~10^7 DOF, DESIGN.md §7: STORED wins at
 *    p = 3, 6, 7 and above 8, where the nodal kernel's register demand
 *    halves occupancy).
 *  SEM_GEOM_NODAL: sem_geom_from_nodes keeps x_phys per global node
 *    (16 B/node) and the action re-derives J, det, invJ and detJxW at every
 *    quadrature node from it -- the reference's own order of work, which
 *    recomputes the geometry inside the element loop (sem/discrete.py:189-209,
 *    582-597) -- trading ~600 FLOP for ~1.9 KB of HBM per element at p = 8.
 *  SEM_GEOM_STORED: the 3 factors per quadrature node are precomputed and
 *    streamed (24 B per element node).
 * Takes effect at the next sem_geom_from_nodes; sem_set_geom always installs
 * stored factors.  The axisymmetric Stokes block (SEM_OP_AXISYM_STOKES) reads
 * the same modes: NODAL re-derives its 7 factors per node from x_phys, with
 * rho = x (16 B/node instead of 56 B per element node; AUTO: NODAL,
 * DESIGN.md §4.2); the Navier-Stokes kinds always use stored factors.
 * x_phys per node is one array per context: sem_geom_from_nodes of either
 * kind recomputes it from the nodes it is given. */
#define SEM_GEOM_STORED 0
#define SEM_GEOM_NODAL 1
#define SEM_GEOM_AUTO 2
int sem_set_geom_mode(sem_ctx* ctx, int mode);

/* Kernel family of the Poisson action; takes effect at the next sem_set_map,
 * which plans the scatter for it.
 *  SEM_KERNEL_COLUMN: k_poisson_apply -- a wavefront holds floor(64/n)
 *    elements, each lane one element column; contractions along the lane in
 *    registers (D in even-odd form), transposes through LDS; chains of 4
 *    groups hand shared columns over through LDS; NODAL or STORED geometry.
 *  SEM_KERNEL_MFMA: k_poisson_mfma -- one element per wavefront as 16 x 16
 *    tiles on the fp64 matrix cores (v_mfma_f64_16x16x4_f64, four products
 *    per element with two transposes through a wave-private LDS tile;
 *    block-diagonal packing of 16/n x 16/n elements per tile for n <= 8);
 *    element-level colouring; stored factors, or x_phys per node when
 *    SEM_GEOM_NODAL is requested; n = p + 1 <= 16 and dpn = 1, else
 *    SEM_E_NOTIMPL.
 *  SEM_KERNEL_AUTO (default): COLUMN -- on its seam plan it measured ahead
 *    of MFMA at every order on MI355X; the build knob
 *    SEM_MFMA_MIN_N (default 17: never) restores an MFMA range.
 * On a hexahedral context (ndim = 3) SEM_KERNEL_MFMA selects k_hex_mfma, the
 * matrix-core form of the hexahedral action on the same chain / seam plan
 * (all six contractions per element as 16 x 16 tiles of
 * v_mfma_f64_16x16x4_f64, stored factors), for p = 11..16;
 * at other orders it returns SEM_E_NOTIMPL.  COLUMN and AUTO keep the
 * three-block kernel below p = 13 and the row form from p = 13
 * (SEM_HEX_ROWS honoured); the diagonal always runs the three-block kernel.
 * The environment variable SEM_KERNEL (0/1/2) sets the initial value; on
 * hexahedral contexts a value of 1 selects the matrix-core form at
 * p = 11..16 and is ignored at other orders. */
#define SEM_KERNEL_COLUMN 0
#define SEM_KERNEL_MFMA 1
#define SEM_KERNEL_AUTO 2
int sem_set_kernel(sem_ctx* ctx, int kernel);

/* Geometry from mesh nodes (device, float64 [2][n_node]) for op_kind:
 * x_phys = V_eq^-1 X V_eq^-T (Mapping._compute_x_phys, sem/mapping.py:98-103),
 * J = gradient(x_phys) (sem/mapping.py:105-114), det/inverse
 * (sem/linalg.py:105-115), detJxW (sem/discrete.py:594-597) and the operator's
 * per-node factors (Poisson 3, axisymmetric 7).  h_Veq_inv is n*n host.
 * Returns SEM_E_DETJ if any detJ <= 0 (count in *n_bad_nodes if non-NULL). */
int sem_geom_from_nodes(sem_ctx* ctx, const double* d_nodes, const double* h_Veq_inv,
                        int op_kind, int64_t* n_bad_nodes, void* stream);

/* Stored factors for op_kind from x_phys given per element (device, float64
 * [n_elem][2][n][n], the FiniteElement.x_phys of each element,
 * sem/discrete.py:582-585): J, det/inverse and detJxW as sem_geom_from_nodes
 * computes them, without the equispaced->GLL transform.  With x_phys from the
 * reference's own LU path (Mapping._compute_x_phys, sem/mapping.py:98-103),
 * the factors carry the reference's float64 rounding of that transform --
 * which dominates the action's error above p = 10.
 * Quadrilaterals; SEM_E_DETJ as sem_geom_from_nodes. */
int sem_geom_from_xphys(sem_ctx* ctx, const double* d_x_phys, int op_kind, int64_t* n_bad_nodes,
                        void* stream);

/* Reference-layout geometry fields for FiniteElement properties
 * (x_phys [E][2][n][n], J and invJ [E][2][2][n][n], detJ and detJxW
 * [E][n][n]; any output may be NULL).  sem/discrete.py:582-597. */
int sem_geom_fields(sem_ctx* ctx, const double* d_nodes, const double* h_Veq_inv,
                    double* d_x_phys, double* d_J, double* d_invJ, double* d_detJ,
                    double* d_detJxW, void* stream);

/* Install precomputed per-node factors (device, [n_elem][ncomp][n][n]). */
int sem_set_geom(sem_ctx* ctx, const double* d_G, int op_kind, void* stream);

/* Global operator action y (=|+=) K u over all elements: the element loop
 * finite_elements() -> einsum('pqrs,rs', Op, u[loc]) -> y[loc] +=
 * (sem/discrete.py:189-209; examples/squirmer-axisymmetric.py:286,293;
 * examples/poisson.py:168-193), matrix-free by sum factorisation.
 * u, y: device float64 of length dpn*n_node.
 * flags: 0 overwrites y (shared entries are zeroed first by a small list
 * kernel); SEM_APPLY_ACCUMULATE adds into y; SEM_APPLY_SKIP_ZERO (overwrite
 * mode only) states that the caller already ran sem_zero_shared on y. */
#define SEM_APPLY_ACCUMULATE 1
#define SEM_APPLY_SKIP_ZERO 2
#define SEM_APPLY_LINEARIZE 4  /* SEM_OP_AXISYM_NS: also record the Newton
                                * linearisation at u for SEM_OP_AXISYM_NS_JVP */
int sem_apply(sem_ctx* ctx, int op_kind, const double* d_u, double* d_y, int flags,
              void* stream);

/* y = K u (overwrite) and *d_dot = u . y (a device double), for the
 * preconditioned CG's p . Kp: on the seam plan of a single-rank Poisson
 * context the dot is summed inside the action's own two launches (each
 * node's final value is stored exactly once: u[gid] * value at that store,
 * per-workgroup partials, one fixed-order sum -- deterministic); on any other
 * plan the action is followed by a separate dot pass.  Same y as sem_apply. */
int sem_apply_dot(sem_ctx* ctx, int op_kind, const double* d_u, double* d_y, double* d_dot,
                  void* stream);

/* Reynolds number N_Re of the SEM_OP_AXISYM_NS residual and its Jacobian
 * (the n_rey scaling of the advection operator Ae, squirmer:230-250).
 * SEM_OP_AXISYM_NS with u = (psi, omega) interleaved gives
 *   y[2k]   = Ae.omega.psi + Lve.omega,   y[2k+1] = E2e.psi - Me.omega
 * (compute_local_system res_l, squirmer:259-297; Ae at quadrature node
 * (m, n) = Re [w_m w_n (d0 psi d1 w - d1 psi d0 w) + (W/rho) w dpsi/dz]).
 * With SEM_APPLY_LINEARIZE it also stores 5 coefficients per element node so
 * that SEM_OP_AXISYM_NS_JVP applies the Jacobian at that state to any
 * direction u -- the matrix-free form of jac_l (squirmer:272-291). */
int sem_set_reynolds(sem_ctx* ctx, double re);

/* Zero the entries of y that the overwrite-mode kernel does not store
 * (element-boundary and unreferenced nodes; all dpn components). */
int sem_zero_shared(sem_ctx* ctx, double* d_y, void* stream);

/* Assembly of element-local nodal values through the element map:
 * out[map[e][i][j]] (+)= vals[e][i][j] (vals device float64 [n_elem][n][n],
 * dpn = 1) -- the reference's global RHS assembly grhs[inds] += lrhs
 * (examples/poisson.py:219-243, sem/discrete.py:478-500), e.g. the load
 * vector of f = 1 from detJxW (sem_geom_fields). */
int sem_assemble(sem_ctx* ctx, const double* d_vals, double* d_out, int accumulate, void* stream);

/* Diagonal of the assembled operator (Jacobi preconditioner for the
 * assembled Poisson solve; diag(Lse) summed through the map). */
int sem_diag(sem_ctx* ctx, int op_kind, double* d_diag, void* stream);

/* Batched tensor-product operator on device arrays [batch][n][n]:
 * out[b][m][q] = sum_{r,s} A0[m][r] A1[q][s] in[b][r][s]; A0/A1 are n*n host
 * matrices, NULL meaning identity.  TensorProduct.deriv / gradient
 * (D(x)I, I(x)D; sem/basis_functions.py:626-650), compute_coeffs_grid_eq
 * (V_eq^-1 (x) V_eq^-1; :599-624), interpolate_on_grid_eq (:539-569). */
int sem_tensor_apply(int n, int64_t batch, const double* h_A0, const double* h_A1,
                     const double* d_in, double* d_out, void* stream);

/* det_inv_2x2 (sem/linalg.py:105-115) over n points: d_mat [2][2][n] ->
 * d_det [n], d_inv [2][2][n]. */
int sem_det_inv_2x2(int64_t n, const double* d_mat, double* d_det, double* d_inv, void* stream);

/* ------------------------------------------------------------------ */
/* Device vector helpers (multi-GPU interface exchange, CG)            */
/* ------------------------------------------------------------------ */
/* dst[i] = src[idx[i]] */
int sem_gather(const double* d_src, const uint32_t* d_idx, int64_t n, double* d_dst, void* stream);
/* dst[i] += src[i] */
int sem_vec_add(double* d_dst, const double* d_src, int64_t n, void* stream);
/* dst[idx[i]] += src[i]  (idx entries unique) */
int sem_scatter_add(double* d_dst, const uint32_t* d_idx, int64_t n, const double* d_src,
                    void* stream);

/* Matrix-free preconditioned CG for K x = b on the free DOFs
 * (mask[i] != 0 => Dirichlet DOF: x[i] fixed, row/col removed), Jacobi
 * preconditioner.  Replaces the assembled solve of DOFManagerSC.solve
 * (sem/discrete.py:502-528; spsolve of the condensed system).  x holds the
 * Dirichlet values and the initial guess on entry.  Device-resident: alpha,
 * beta and the dot products never leave the device; the host reads the
 * residual history once every SEM_PCG_CHECK_EVERY iterations (one small copy
 * + one stream synchronisation), so up to SEM_PCG_CHECK_EVERY - 1 iterations
 * run past the converged one (they only refine x).  *iters = iterations
 * executed, *final_relres = ||r|| / ||r0|| after the last one.
 * SEM_E_INVALID if not converged within max_iter; rtol = 0 runs exactly
 * max_iter iterations (benchmarking) and returns SEM_OK. */
#define SEM_PCG_CHECK_EVERY 16
int sem_pcg_solve(sem_ctx* ctx, int op_kind, const double* d_b, double* d_x,
                  const uint8_t* d_dirichlet, double rtol, int max_iter,
                  int* iters, double* final_relres, void* stream);

/* ------------------------------------------------------------------ */
/* Static condensation (DOFManagerSC, sem/discrete.py:283-528)         */
/* ------------------------------------------------------------------ */
/* Element Schur complements of local systems in hierarchical order
 * (exterior DOFs first; DOFManagerSC.reorder_local_system_hier), all
 * elements in one launch: compute_local_sc_system (sem/discrete.py:428-466)
 *   S_e = A_ee - A_ei A_ii^-1 A_ie,  s_e = b_e - A_ei A_ii^-1 b_i.
 * d_mat [n_elem][nl][nl], d_rhs [n_elem][nl] -> d_sc_mat [n_elem][ne][ne],
 * d_sc_rhs [n_elem][ne]; d_work [n_elem][nl-ne][nl+1] keeps
 * A_ii^-1 [A_ie | b_i] for sem_schur_backsolve.  Gauss-Jordan with partial
 * pivoting, one workgroup per element (nl - ne <= 512).  SEM_E_INVALID
 * (count in *n_singular) when an interior block is singular (a pivot column
 * exactly zero) or holds a NaN or an off-diagonal inf, where the reference's
 * linalg.solve(..., check_finite=False) raises too; non-finite couplings
 * A_ie, A_ei, b_i and infinite diagonal entries of A_ii propagate as they
 * do there (sem/discrete.py:465-468). */
int sem_schur_batched(int64_t n_elem, int nl, int ne, const double* d_mat, const double* d_rhs,
                      double* d_work, double* d_sc_mat, double* d_sc_rhs, int64_t* n_singular,
                      void* stream);
/* Interior DOFs from the exterior ones, x_i = A_ii^-1 (b_i - A_ie x_e)
 * (_solve_interior_dofs, sem/discrete.py:512-524): d_xe [n_elem][ne] ->
 * d_xi [n_elem][nl-ne], from the d_work of sem_schur_batched. */
int sem_schur_backsolve(int64_t n_elem, int nl, int ne, const double* d_work, const double* d_xe,
                        double* d_xi, void* stream);
/* Jacobi-PCG (as sem_pcg_solve) on an assembled symmetric positive definite
 * CSR matrix (device int64 row pointers, int32 columns, float64 values):
 * the condensed exterior system of _solve_boundary_dofs
 * (sem/discrete.py:502-510, a scipy spsolve in the reference). */
int sem_csr_pcg_solve(int64_t n, const int64_t* d_rowptr, const int32_t* d_colind,
                      const double* d_val, const double* d_b, double* d_x,
                      const uint8_t* d_dirichlet, double rtol, int max_iter, int* iters,
                      double* final_relres, int device, void* stream);
/* Direct solve of a general (non-symmetric) square CSR system A x = b by
 * banded LU with partial pivoting: the condensed exterior system of
 * _solve_boundary_dofs when it is not symmetric (the axisymmetric Stokes /
 * Navier-Stokes block; scipy.sparse.linalg.spsolve in the reference,
 * sem/discrete.py:502-511).  kl / ku: lower / upper bandwidth of A as
 * ordered by the caller (reverse Cuthill-McKee, as the reference orders its
 * nodes); any kl (the multipliers are kept in the band, LAPACK's
 * in-place L).  Duplicate entries are summed.  Band storage
 * n (2 kl + ku + 1) doubles, allocated on the stream.  *info = 0 on
 * success, j + 1 when column j has an exactly zero pivot (A singular; x is
 * then not written), as LAPACK gbsv.  Synchronises the stream. */
int sem_band_lu_solve(int64_t n, int kl, int ku, const int64_t* d_rowptr, const int32_t* d_colind,
                      const double* d_val, const double* d_b, double* d_x, int* info,
                      void* stream);

/* ------------------------------------------------------------------ */
/* Domain decomposition across GPUs (one process per GPU)              */
/* ------------------------------------------------------------------ */
/* The reference's element loop (sem/discrete.py:189-209) is serial; its
 * elements are independent except for the scatter-add, so a rank owns a set
 * of elements and sums only the DOFs it shares with other ranks
 * (SURVEY.md §8(e)).  A sem_dd holds two operator contexts of one rank:
 *   iface     the elements touching a shared node, either over the rank's
 *             own numbering (the context holds ndof_local DOFs: it reads u
 *             directly and writes a private rank-sized vector) or over a
 *             COMPACT numbering of their n_iface_dofs DOFs; in both cases
 *             d_iface_dofs[i] = local DOF of compact DOF i (device uint32,
 *             the DOFs interface elements touch);
 *   interior  every other element, over the local numbering (ndof_local
 *             DOFs); NULL when the rank has no interior element.
 * iface is NULL (n_iface_dofs = 0, no peers) on a rank that shares no node;
 * it still takes part in the global dot products.
 * sem_dd_apply enqueues the interface elements on an internal side stream,
 * packs their shared entries and exchanges them with the peers while the
 * interior elements run on the caller's stream; the caller's stream then
 * adds the interface result into y.  Peer k receives/sends
 * h_peer_counts[k] values: d_peer_dofs (device uint32, concatenated over
 * peers) lists the COMPACT DOFs shared with each peer, in an order both
 * sides agree on (e.g. ascending global id).  d_not_owned (device uint8
 * [ndof_local], may be NULL) marks DOFs whose owner is another rank (left out
 * of the global dot products of sem_dd_pcg_solve). */
typedef struct sem_dd sem_dd;
int sem_dd_create(sem_dd** out, sem_ctx* iface, sem_ctx* interior, int64_t ndof_local,
                  const uint32_t* d_iface_dofs, int64_t n_iface_dofs, int n_peers,
                  const int* h_peers, const int64_t* h_peer_counts, const uint32_t* d_peer_dofs,
                  const uint8_t* d_not_owned, int device);
void sem_dd_destroy(sem_dd* dd);

/* Transport, native: an RCCL communicator over all ranks (ncclSend/ncclRecv
 * with each peer inside one group, ncclAllReduce for the dot products, all
 * on the library's streams; xGMI between the GPUs of one node).  Rank 0
 * creates the id with sem_rccl_unique_id and the caller broadcasts its
 * SEM_RCCL_ID_BYTES bytes (e.g. through torch.distributed). */
#define SEM_RCCL_ID_BYTES 128
int sem_rccl_unique_id(void* h_id, int nbytes);
int sem_dd_init_rccl(sem_dd* dd, const void* h_id, int world, int rank);

/* Transport, caller-supplied (tests, other communication libraries): the
 * exchange callback must leave in d_recv[off[k]..off[k+1]) the values peer
 * peers[k] sent from its d_send range, ordered after the work already on
 * `side_stream` and before anything enqueued on it later; the all-reduce
 * callback sums `count` doubles of d_buf over all ranks in place, ordered on
 * `stream`.  Both return 0 on success. */
typedef int (*sem_exchange_fn)(void* user, int n_peers, const int* peers, const int64_t* off,
                               double* d_send, double* d_recv, void* side_stream);
typedef int (*sem_allreduce_fn)(void* user, double* d_buf, int count, void* stream);
int sem_dd_set_transport(sem_dd* dd, sem_exchange_fn exchange, sem_allreduce_fn allreduce,
                         void* user, int world, int rank);

/* Transport, diagnostic loopback: every exchange copies this rank's own send
 * buffer into its receive buffer (one kernel on the side stream, the bytes
 * RCCL's send/recv would move), every all-reduce is the identity, world 1.
 * Times ONE rank of a decomposition alone on one GPU (bench.py --time-rank):
 * the kernels, streams and host enqueue of the real step, values NOT the
 * global action. */
int sem_dd_set_loopback(sem_dd* dd);

/* Transport, timing: RCCL on a one-rank communicator of this process, every
 * exchange a ncclSend / ncclRecv pair per peer addressed to this rank itself
 * inside one group on the side stream (RCCL's own host enqueue, proxy and
 * copy kernels in place of the loopback kernel), all-reduces over one rank.
 * Like sem_dd_set_loopback it times ONE rank of a decomposition alone
 * (bench.py --time-rank --time-rank-transport rccl_self); values NOT the
 * global action.  sem_dd_info [4] = 4. */
int sem_dd_set_rccl_self(sem_dd* dd);

/* hipMemcpyAsync(dst, src, nbytes, hipMemcpyDefault, stream): lets a
 * caller-supplied transport stage the library's device buffers. */
int sem_copy_async(void* dst, const void* src, int64_t nbytes, void* stream);

/* info[0] ndof_local, [1] n_iface_dofs, [2] peers, [3] exchanged values per
 * direction, [4] transport (0 none, 1 RCCL, 2 callbacks, 3 loopback),
 * [5] has interior, [6] captured step on (sem_dd_set_graphs), [7] captures,
 * [8] replays, [9] sem_dd_apply calls, [10] host nanoseconds spent in them,
 * [11] of which inside the transport call (a caller transport that
 * synchronises with the device makes [11] the device time up to the
 * exchange), eager steps only: [12] enqueueing the side-stream part (gather,
 * interface elements, pack), [13] the interior elements, [14] the finish;
 * [15] bit 0: the interior's zero list folded into the finish, bit 1: the
 * interior's seam sum fused with the finish (one launch), bit 2: the
 * interface seam sum fused with the pack, bit 3: the finish split around the
 * join, bit 4: the stream-join events are recorded without the system-scope
 * fence (only the one-device transports, loopback and RCCL to self, unless
 * SEM_DD_EVENT_FENCE=system|device forces a scope).
 * Hexahedral contexts (sem_ctx_create_nd, ndim 3) are accepted for both
 * iface and interior (interface context over the local numbering). */
int sem_dd_info(sem_dd* dd, int64_t* info, int n_info);

/* Captured step (default off; SEM_DD_GRAPH=1 in the environment turns it
 * on): sem_dd_apply and the PCG operator action replay the step's launches
 * as four HIP graphs around the transport call (side stream: gather,
 * interface elements, pack | unpack; caller's stream: interior elements |
 * final add), re-captured when the operator kind or the u / y pointers
 * change.  Same kernels, same order, same results as the eager path; the
 * host enqueues 4 graph launches instead of ~15 kernel launches, which on
 * ROCm 7 costs more host time, not less. */
int sem_dd_set_graphs(sem_dd* dd, int enable);

/* y = K u on this rank's DOFs, shared DOFs summed over all ranks (u, y local
 * device vectors, must not alias). */
int sem_dd_apply(sem_dd* dd, int op_kind, const double* d_u, double* d_y, void* stream);
/* diagonal of the globally assembled operator on this rank's DOFs */
int sem_dd_diag(sem_dd* dd, int op_kind, double* d_diag, void* stream);
/* sem_pcg_solve over the decomposition: global dot products over owned DOFs
 * (one all-reduce per dot), convergence read every check_every iterations. */
int sem_dd_pcg_solve(sem_dd* dd, int op_kind, const double* d_b, double* d_x,
                     const uint8_t* d_dirichlet, double rtol, int max_iter, int check_every,
                     int* iters, double* final_relres, void* stream);

/* ------------------------------------------------------------------ */
/* Points: location and field evaluation at arbitrary physical points  */
/* ------------------------------------------------------------------ */
/* The batched device form of DOFManager.find_elem_containing_point /
 * interpolate (sem/discrete.py:221-233, 263-280) and Mapping.inv
 * (sem/mapping.py:146-178), which the reference runs one point at a time
 * (a sort of every cell centroid per query, then up to 8 Newton steps of
 * Python barycentric evaluations).  Quadrilaterals and hexahedra,
 * 1 <= p <= 16 (GLL nodes and barycentric weights of csrc/gll_table.h).
 * Point arrays are component-major: d_xq / d_xi / d_x_out float64
 * [ndim][n_pts]; element ids int32 [n_pts]; n_pts < 2^31. */
typedef struct sem_points sem_points;
typedef struct sem_pplan sem_pplan;

/* Relative inflation (of its own extent, per axis and side) of an element's
 * axis-aligned box over its GLL coefficients: a Lagrange interpolant is not
 * bounded by its nodal hull.  An element is a candidate for a point only
 * when the point lies in its inflated box. */
#define SEM_POINTS_BOX_MARGIN 0.25
/* A located point is accepted when every |xi_k| <= 1 + SEM_POINTS_XI_SLACK
 * and is then clamped to [-1, 1]. */
#define SEM_POINTS_XI_SLACK 1e-10

/* d_x_phys: float64 [n_elem][ndim][n^ndim] exactly as sem_geom_fields writes
 * it; BORROWED (the caller keeps it alive and unchanged).  Builds, per
 * element, the inflated box and the centroid (mean of the 2^ndim corner
 * coefficients, Mesh._compute_cell_centroids sem/discrete.py:1108-1113) with
 * one kernel; the boxes (32 or 48 B per element, never x_phys) are copied to
 * the host, which lays a uniform grid of about n_elem cells over the mesh
 * box and lists per cell the elements whose box meets it (CSR, uploaded).
 * Synchronises `stream`.  SEM_E_INVALID: ndim not 2 or 3, p < 1, n_elem < 1,
 * NULL pointers, non-finite coordinates; SEM_E_NOTIMPL: p > 16 (checked
 * before any device call). */
int sem_points_create(sem_points** out, int ndim, int p, int64_t n_elem, const double* d_x_phys,
                      int device, void* stream);
void sem_points_destroy(sem_points* pts);

/* For each point: the candidates of its grid cell, in ascending centroid
 * distance (the reference's order; ties by element id), each tried with the
 * reference's Newton (sem/rootfind.py:22-53 as called at sem/mapping.py:171):
 * xi = 0, at most 8 iterations, stop at |dx|_2 <= 1e-8, Jacobian
 * sum c l' (x) l (equal to the reference's interpolated nodal J field),
 * closed-form 2x2 / 3x3 solve.  Deviations from the reference:
 *  1. a candidate whose Newton does not converge, meets a singular Jacobian
 *     or a non-finite iterate is skipped (the reference lets SolverFailure
 *     escape, which is all it returns for points outside the mesh);
 *  2. acceptance is |xi_k| <= 1 + SEM_POINTS_XI_SLACK, then a clamp to
 *     [-1, 1] (the reference's strict test can reject a point of the domain
 *     boundary from every element by one ulp);
 *  3. a point in no candidate gets elem = -1, xi = NaN, is counted in
 *     *n_outside (may be NULL), and the call still returns SEM_OK.
 * A point on a shared face may be given to either neighbour.  Work per point
 * is bounded by 8 Newton steps times its cell's candidate count.
 * Synchronises `stream` (the count is read back).  The count's device word
 * and the "last locate" figures of sem_points_info belong to `pts`: one
 * sem_points_locate at a time per sem_points (calls from several streams or
 * threads on one object must be serialised by the caller; invert, map, plan
 * and eval keep no state in `pts` and may run concurrently). */
int sem_points_locate(sem_points* pts, int64_t n_pts, const double* d_xq, int32_t* d_elem,
                      double* d_xi, int64_t* n_outside, void* stream);

/* The same Newton in caller-given elements (Mapping.inv for many points):
 * d_xi_guess may be NULL (xi = 0).  d_status (uint8, may be NULL): 0 inside
 * (slack and clamp as above), 1 converged outside [-1, 1]^d (xi as
 * converged), 2 failed or element id outside [0, n_elem) (xi = NaN; no
 * memory is indexed with a bad id).  Does not synchronise. */
int sem_points_invert(sem_points* pts, int64_t n_pts, const double* d_xq,
                      const int32_t* d_elem_in, const double* d_xi_guess, double* d_xi,
                      uint8_t* d_status, void* stream);

/* x(xi) in the given elements (Mapping.__call__, sem/mapping.py:141-144; the
 * evaluator of the Newton residual); NaN for ids outside [0, n_elem). */
int sem_points_map(sem_points* pts, int64_t n_pts, const int32_t* d_elem, const double* d_xi,
                   double* d_x_out, void* stream);

/* Buckets a located point set by element (device count, host prefix sum of
 * the n_elem counts, device fill) and cuts every element's run into items of
 * at most W points; W = 16 when the touched elements hold 24 points or fewer
 * on average (four items share a wavefront), else 64.  Points whose id is
 * outside [0, n_elem) belong to no run.  Holds the permutation and the items;
 * d_elem is not needed afterwards.  Synchronises `stream`. */
int sem_points_plan(sem_points* pts, int64_t n_pts, const int32_t* d_elem,
                    sem_pplan** out, void* stream);
void sem_points_plan_destroy(sem_pplan* plan);

/* out[c][i] = sum_{jk..} u[c * comp_stride + e2n[elem_i][j][k].. * node_stride]
 *                        l_j(xi0_i) l_k(xi1_i) ..          (c < ncomp)
 * (FiniteElement.interpolate of coeffs[..., fe.node_ind],
 * sem/discrete.py:231-233) for the planned points, in the caller's point
 * order; d_out float64 [ncomp][n_pts].  Component-major fields: comp_stride =
 * n_node, node_stride = 1; interleaved DOFs: comp_stride = 1, node_stride =
 * dpn.  d_e2n: uint32 [n_elem][n^ndim] (the caller's map, as sem_set_map
 * takes it); d_xi as located.  At xi exactly on a GLL node the basis is the
 * Kronecker delta (as sem_barycentric_lagrange): no 0/0 reaches the output.
 * Points in no run get NaN and index no memory at all: a bad element id
 * cannot cause an out-of-bounds access.  The map's entries are the caller's
 * obligation: d_u must hold at least max(d_e2n) + 1 nodes per component
 * (entries up to (ncomp - 1) * comp_stride + max(d_e2n) * node_stride), which
 * this call cannot check without reading the map; points.PointSet.evaluate
 * refuses a u of any other size.  Allocates nothing and does not
 * synchronise (graph-capturable, like sem_apply). */
int sem_points_eval(sem_pplan* plan, const uint32_t* d_e2n, const double* d_xi, int ncomp,
                    int64_t comp_stride, int64_t node_stride, const double* d_u, double* d_out,
                    void* stream);

/* info[0] ndim, [1] p, [2] n_elem, [3..5] grid cells per axis, [6] cells,
 * [7] CSR entries, [8] most candidates in one cell, [9] / [10] points found /
 * outside in the last sem_points_locate, [11] Newton iteration cap.
 * Writes min(n_info, 12) values. */
int sem_points_info(sem_points* pts, int64_t* info, int n_info);
/* info[0] points, [1] points in runs, [2] items, [3] touched elements,
 * [4] lanes per item W, [5] items per workgroup.  min(n_info, 6) values. */
int sem_points_plan_info(sem_pplan* plan, int64_t* info, int n_info);

/* ------------------------------------------------------------------ */
/* Faces: normals, surface integrals and Neumann loads on element faces */
/* ------------------------------------------------------------------ */
/* The batched device form of SubMapping / SubFiniteElement
 * (sem/mapping.py:184-272, sem/discrete.py:708-775), which the reference
 * builds as one Python object per face (its 3-D normal is unfinished:
 * _compute_normal_vec drops the cross product).  Quadrilaterals and
 * hexahedra, 1 <= p <= 16, isoparametric.
 *
 * Conventions (the reference's _subface_slice, sem/mapping.py:19-76, and
 * SubMapping._tangents, :233-256):
 *   - face id = 2 * axis + side; axis indexes the element array's axes (xi0
 *     first), side 0 is xi = -1, side 1 is xi = +1;
 *   - nf = n^(ndim-1) nodes per face, index q;
 *   - 2-D faces run counter-clockwise round the element: on faces 0 and 3
 *     q runs against the element's own index, on faces 1 and 2 along it;
 *   - 3-D faces: q = q0 * n + q1; on a side-1 face (q0, q1) index the axes
 *     (axis+1, axis+2) mod 3 in this cyclic order, on a side-0 face the axes
 *     (axis+2, axis+1) mod 3, the reverse order;
 *   - tangents are the columns of J (J[c][i] = d x_c / d xi_i) of the face's
 *     axes in that order, at the face nodes; the 2-D tangent is negated on
 *     faces 0 and 3;
 *   - n_dS = (t_y, -t_x) in 2-D, t0 x t1 in 3-D: outward on every face;
 *   - dS = |n_dS|, unit_normal = n_dS / dS, dSxW = dS times the tensor of the
 *     1-D quadrature weights on the face.
 * Face arrays: vectors float64 [F][ndim][nf], scalars [F][nf], matrices
 * [F][ndim][ndim][nf], node ids uint32 [F][nf]. */
typedef struct sem_faces sem_faces;

/* d_x_phys: float64 [n_elem][ndim][n^ndim] exactly as sem_geom_fields writes
 * it; d_e2n: uint32 [n_elem][n^ndim]; h_elem / h_face: the n_faces (element,
 * face) pairs (a pair may repeat; n_faces == 0 is valid); h_D: the 1-D
 * differentiation matrix [n][n] (sem_diff_matrix), h_w: the n quadrature
 * weights.  Every pair is checked on the host before any device call:
 * SEM_E_INVALID for an element id outside [0, n_elem), a face >= 2 * ndim,
 * ndim not 2 or 3, p < 1, NULL arrays, n_faces * nf >= 2^31; SEM_E_NOTIMPL for
 * p > 16.  One kernel (one workgroup per face) computes and stores per face
 * node x, J (the derivative along the face's normal axis taken with the first
 * or last row of D), invJ, detJ, n_dS, dSxW and the global node id in face
 * order; the node ids are read back and the host lists the distinct boundary
 * nodes (ascending) with the CSR of their (face, q) contributions in
 * ascending (face, q) order.  Nothing is borrowed after the call returns.
 * Synchronises `stream`. */
int sem_faces_create(sem_faces** out, int ndim, int p, int64_t n_elem, const double* d_x_phys,
                     const uint32_t* d_e2n, int64_t n_faces, const int32_t* h_elem,
                     const uint8_t* h_face, const double* h_D, const double* h_w, int device,
                     void* stream);
void sem_faces_destroy(sem_faces* faces);

/* Copies of the stored face fields (SubFiniteElement.x_phys / n_dS / dS /
 * dSxW / unit_normal / node_ind, SubMapping.J / invJ / detJ); any output may
 * be NULL.  invJ[i][j] = d xi_i / d x_j.  One launch, no synchronisation. */
int sem_faces_geometry(sem_faces* faces, double* d_x, double* d_n_dS, double* d_dS,
                       double* d_dSxW, double* d_unit, uint32_t* d_node_ind, double* d_J,
                       double* d_invJ, double* d_detJ, void* stream);

/* Physical gradient of the parent element's interpolant at the face nodes,
 * grad_j = sum_i invJ[i][j] du/dxi_i (FiniteElement.gradient sliced to the
 * face, sem/discrete.py:771-774), d_grad [ncomp][F][ndim][nf], and its
 * product with the unit normal, d_dudn [ncomp][F][nf]; either may be NULL.
 * u is read as u[c * comp_stride + e2n[..] * node_stride] (sem_points_eval's
 * strides); d_e2n is the map given at create.  d_u's size is the caller's
 * obligation, as in sem_points_eval; faces.FaceSet refuses a u of any other
 * size.  ncomp <= 65535.  One launch; allocates nothing and does not
 * synchronise (graph-capturable). */
int sem_faces_gradient(sem_faces* faces, const uint32_t* d_e2n, int ncomp, int64_t comp_stride,
                       int64_t node_stride, const double* d_u, double* d_grad, double* d_dudn,
                       void* stream);

/* d_per_face[c][f] = sum_q d_vals[c][f][q] dSxW[f][q]
 * (SubFiniteElement.integrate, sem/discrete.py:768-769) and d_total[c] =
 * sum_f of these; either output may be NULL (d_per_face only up to ncomp =
 * 8: the handle's own scratch then holds the per-face values).  Fixed-order
 * two-stage sum (per face, then one workgroup per component over the faces):
 * bitwise repeatable.  With no faces the totals are 0 and nothing else is
 * written.  Allocates nothing and does not synchronise. */
int sem_faces_integrate(sem_faces* faces, int ncomp, const double* d_vals, double* d_per_face,
                        double* d_total, void* stream);

/* The same sums of grad u . unit_normal, without writing the gradient out:
 * the flux of u through every face and through the whole list. */
int sem_faces_flux(sem_faces* faces, const uint32_t* d_e2n, int ncomp, int64_t comp_stride,
                   int64_t node_stride, const double* d_u, double* d_per_face, double* d_total,
                   void* stream);

/* The Neumann load vector: d_out[node] (+)= sum d_vals[f][q] dSxW[f][q] over
 * the (f, q) entries of each distinct boundary node, one thread per node over
 * its CSR row; no atomics, bitwise deterministic; nodes on no listed face are
 * untouched in both modes.  d_out holds n_node entries: SEM_E_INVALID when a
 * face node id (known from create) is >= n_node.  Does not synchronise. */
int sem_faces_assemble(sem_faces* faces, const double* d_vals, double* d_out, int64_t n_node,
                       int accumulate, void* stream);

/* info[0] ndim, [1] p, [2] faces, [3] nf, [4] distinct boundary nodes,
 * [5] longest CSR row, [6] largest node id on a face (-1 with no faces).
 * Writes min(n_info, 7) values. */
int sem_faces_info(sem_faces* faces, int64_t* info, int n_info);

/* ------------------------------------------------------------------ */
/* Transfer: fields between two polynomial orders of one mesh           */
/* ------------------------------------------------------------------ */
/* Two discretisations "from" and "to" of the same elements: the same n_elem
 * and element order, the same local axis orientation per element, maps
 * e2n_from uint32 [n_elem][n_from^ndim] and e2n_to [n_elem][n_to^ndim]
 * (n = p + 1).  Quadrilaterals and hexahedra, any 1 <= p_from, p_to <= 16 in
 * either direction; p_from > p_to is nodal interpolation down, p_from == p_to
 * a renumbering copy.  The reference has no counterpart.
 *
 * J [n_to][n_from], J[i][j] = l_j^from(x_i^to): the order-p_from GLL Lagrange
 * basis at the order-p_to GLL nodes (sem_gll_table, sem_lagrange_eval: a
 * coincident node gives exactly 0 or 1).
 *   - prolong: u_to[g] = ((J x J [x J]) u_from[e2n_from[e]])[l] for the owner
 *     (e, l) of the "to" node g, the lowest (element, local index) pair that
 *     references g.  On a conforming input every referencing element gives
 *     the same value up to rounding; the owner rule makes the result bitwise
 *     repeatable.  "To" nodes no element references are left untouched.
 *   - restrict: r_from = P^T r_to, the exact transpose of that matrix P: per
 *     element r_to at its owned entries (zero elsewhere) times Jt x Jt [x Jt],
 *     summed into the "from" nodes in ascending (element, local index) order
 *     per node, without atomics: bitwise repeatable.
 * Vectors are read and written as v[c * comp_stride + node * node_stride]
 * (sem_points_eval's strides), c < ncomp <= 65535. */
typedef struct sem_transfer sem_transfer;

/* d_e2n_from / d_e2n_to: the two device maps, BORROWED until
 * sem_transfer_destroy: the kernels read them at every call, the caller keeps
 * them allocated and unchanged.  They are copied to the host once, where
 * every id is checked before any launch and the plan is made (the owner mask
 * of the "to" map, the CSR of the (element, local) entries of every "from"
 * node): SEM_E_INVALID for ndim not 2 or 3, an order < 1, n_elem < 0 (0 is
 * valid), a node count outside [0, 2^32], n_elem * n^ndim >= 2^31 on either
 * side, a NULL map, an id >= its n_node; SEM_E_NOTIMPL for an order > 16.
 * The handle owns a scratch of 2 * n_elem * n_from^ndim doubles for restrict.
 * Synchronises `stream`. */
int sem_transfer_create(sem_transfer** out, int ndim, int p_from, int p_to, int64_t n_elem,
                        const uint32_t* d_e2n_from, int64_t n_node_from,
                        const uint32_t* d_e2n_to, int64_t n_node_to, int device, void* stream);
void sem_transfer_destroy(sem_transfer* transfer);

/* d_u_to = P d_u_from.  d_u_from holds n_node_from nodes per component,
 * d_u_to n_node_to (the caller's obligation, as in sem_points_eval;
 * transfer.Transfer refuses any other size).  One launch; allocates nothing
 * and does not synchronise (graph-capturable).  SEM_E_INVALID for a NULL
 * handle or array, ncomp outside [1, 65535], a stride < 0 / < 1. */
int sem_transfer_prolong(sem_transfer* transfer, int ncomp, int64_t comp_stride_from,
                         int64_t node_stride_from, const double* d_u_from,
                         int64_t comp_stride_to, int64_t node_stride_to, double* d_u_to,
                         void* stream);

/* d_r_from (+)= P^T d_r_to.  Overwrite mode (accumulate = 0) writes every
 * "from" node, 0 where no element references it; accumulate != 0 adds to
 * d_r_from and leaves such nodes alone.  Two launches per two components
 * (element kernel into the handle's scratch, then one thread per "from" node
 * over its CSR row); allocates nothing and does not synchronise.  Calls on
 * one handle must be ordered (one stream, or events): they share the scratch. */
int sem_transfer_restrict(sem_transfer* transfer, int ncomp, int64_t comp_stride_to,
                          int64_t node_stride_to, const double* d_r_to,
                          int64_t comp_stride_from, int64_t node_stride_from, double* d_r_from,
                          int accumulate, void* stream);

/* info[0] ndim, [1] p_from, [2] p_to, [3] elements, [4] / [5] "from" / "to"
 * node counts, [6] owned "to" entries (= referenced "to" nodes), [7] longest
 * CSR row of a "from" node, [8] scratch bytes.  Writes min(n_info, 9) values. */
int sem_transfer_info(sem_transfer* transfer, int64_t* info, int n_info);

/* ------------------------------------------------------------------ */
/* Volume: gradients, recovery, integrals, norms, lumped mass           */
/* ------------------------------------------------------------------ */
/* The batched device form of FiniteElement.gradient / deriv / integrate
 * (sem/discrete.py:674-689), which the reference runs per element in NumPy,
 * plus what convergence studies build from them: the continuous nodal
 * gradient, the GLL-quadrature L2 / H1 norms and the lumped mass.
 * Quadrilaterals and hexahedra, 1 <= p <= 16, isoparametric.
 *
 * Arrays are element-major: element fields float64 [n_elem][n^ndim] with the
 * local index lexicographic (xi0 slowest), gradients [n_elem][ndim][n^ndim].
 * Global vectors are read and written as v[c * comp_stride + node *
 * node_stride] (sem_points_eval's strides), c < ncomp <= 65535.  With
 * J[c][i] = d x_c / d xi_i from x_phys and D, invJ its inverse by cofactors,
 * detJxW = det J times the tensor of the 1-D quadrature weights
 * (sem/discrete.py:594-597).  No per-node J / invJ is stored: every call
 * recomputes the geometry from x_phys.  No atomics: every sum is taken in a
 * fixed order, so two calls give the same bits. */
typedef struct sem_volume sem_volume;

/* d_x_phys: float64 [n_elem][ndim][n^ndim] exactly as sem_geom_fields writes
 * it; d_e2n: uint32 [n_elem][n^ndim].  Both are BORROWED until
 * sem_volume_destroy: the kernels read them at every call, the caller keeps
 * them allocated and unchanged.  h_D [n][n] (sem_diff_matrix) and h_w [n] are
 * read before the call returns.  The map is copied to the host once, where
 * every id is checked before any launch and the CSR of the (element, local)
 * entries of every node is planned, rows in ascending order
 * (csrc/sem_volume_plan.cpp): SEM_E_INVALID for ndim not 2 or 3, p < 1,
 * n_elem < 0 (0 is valid), n_node outside [0, 2^32], n_elem * n^ndim >= 2^31,
 * a NULL array, an id >= n_node; SEM_E_NOTIMPL for p > 16.  One launch then
 * computes detJ at every element node: SEM_E_DETJ, with the count in the
 * message, when any detJ <= 0 (sem/mapping.py:117); a node kernel sums the
 * lumped mass m[g] = sum of detJxW[e][l] over the CSR row of g, in the row's
 * order.  The handle owns m, detJxW (one double per element node, what the
 * integrals weigh with) and one scratch of n_elem * ndim * n^ndim doubles for
 * the recovery.  Synchronises `stream`. */
int sem_volume_create(sem_volume** out, int ndim, int p, int64_t n_elem, const double* d_x_phys,
                      const uint32_t* d_e2n, int64_t n_node, const double* h_D, const double* h_w,
                      int device, void* stream);
void sem_volume_destroy(sem_volume* vol);

/* d_m [n_node]: a copy of the lumped mass, 0 at nodes no element references.
 * Does not synchronise. */
int sem_volume_mass(sem_volume* vol, double* d_m, void* stream);

/* d_grad[c][e][j][l] = sum_i invJ[i][j] du_c/dxi_i: FiniteElement.gradient
 * (sem/discrete.py:680-684) of u_c[e2n[e]] for all elements, d_grad float64
 * [ncomp][n_elem][ndim][n^ndim].  d_u holds n_node nodes per component (the
 * caller's obligation, as in sem_points_eval; volume.VolumeSet refuses any
 * other size).  One launch; allocates nothing and does not synchronise
 * (graph-capturable).  SEM_E_INVALID for a NULL handle or array, ncomp
 * outside [1, 65535], a stride < 0 / < 1. */
int sem_volume_gradient(sem_volume* vol, int ncomp, int64_t comp_stride, int64_t node_stride,
                        const double* d_u, double* d_grad, void* stream);

/* The continuous nodal gradient, the lumped-mass L2 projection of the element
 * gradients: d_g[c * out_comp_stride + j * out_dim_stride + node *
 * out_node_stride] = (sum over the node's CSR row of detJxW[e][l] *
 * grad[c][e][j][l]) / m[node], rows summed in ascending (element, local)
 * order; 0 at nodes no element references.  Two launches per component (the
 * element kernel into the handle's scratch, then one thread per node over its
 * row); allocates nothing and does not synchronise.  Calls on one handle that
 * use the scratch (this one, and the sums below when d_per_elem is NULL) must
 * be ordered: one stream, or events. */
int sem_volume_recover(sem_volume* vol, int ncomp, int64_t comp_stride, int64_t node_stride,
                       const double* d_u, int64_t out_comp_stride, int64_t out_dim_stride,
                       int64_t out_node_stride, double* d_g, void* stream);

/* d_per_elem[c][e] = sum_l detJxW[e][l] u_c[e2n[e][l]] and d_total[c] = sum_e
 * of these, for a nodal field; either output may be NULL (without d_per_elem
 * the per-element values pass through the handle's scratch).  Fixed-order
 * two-stage sum as sem_faces_integrate (per element, then one workgroup per
 * component over the elements).  With no elements the totals are 0.
 * Allocates nothing and does not synchronise. */
int sem_volume_integrate(sem_volume* vol, int ncomp, int64_t comp_stride, int64_t node_stride,
                         const double* d_u, double* d_per_elem, double* d_total, void* stream);

/* The same for element-local values d_vals [ncomp][n_elem][n^ndim]:
 * FiniteElement.integrate (sem/discrete.py:686-688) of every element. */
int sem_volume_integrate_local(sem_volume* vol, int ncomp, const double* d_vals,
                               double* d_per_elem, double* d_total, void* stream);

/* With d = u - v formed at the nodes first (d_v NULL: v = 0; d_v has d_u's
 * strides): d_per_elem[c][e][0] = sum_l detJxW d^2, [c][e][1] = sum_l detJxW
 * |grad d|^2, the GLL-quadrature discrete L2^2 and H1-seminorm^2 (the
 * quadrature of Lse, examples/poisson.py:166-193), and d_total[c][0..1] their
 * fixed-order sums over the elements.  Either output may be NULL.  The
 * gradient is never written to memory.  Allocates nothing and does not
 * synchronise. */
int sem_volume_norms(sem_volume* vol, int ncomp, int64_t comp_stride, int64_t node_stride,
                     const double* d_u, const double* d_v, double* d_per_elem, double* d_total,
                     void* stream);

/* info[0] ndim, [1] p, [2] elements, [3] nodes, [4] referenced nodes,
 * [5] longest CSR row, [6] scratch bytes.  Writes min(n_info, 7) values. */
int sem_volume_info(sem_volume* vol, int64_t* info, int n_info);

/* ------------------------------------------------------------------ */
/* Element matrices: the dense local systems of the assembled path      */
/* ------------------------------------------------------------------ */
/* The dense element operators the reference builds per element in Python --
 * Lse (examples/poisson.py:166-193) and the Newton system jac_l / -res_l of
 * compute_local_system (examples/squirmer-axisymmetric.py:259-297) -- for the
 * elements [elem_begin, elem_begin + elem_count) in one launch.  Quadrilaterals
 * (ndim = 2), 1 <= p <= 16.  op_kind: SEM_OP_POISSON (dpn = 1),
 * SEM_OP_AXISYM_STOKES (dpn = 2), SEM_OP_AXISYM_NS (dpn = 2; `re` and d_state
 * required).  nl = dpn * n * n; local DOF dpn * (i * n + j) + comp, as
 * FiniteElement.loc_dof_ind_hier assumes (sem/discrete.py:562-571).
 *
 * d_mat: float64 [elem_count][nl][nl].  Column k of an element's matrix is
 * what the action of the kind (sem_apply) gives for that element alone on the
 * k-th local unit vector:
 *   Poisson  A[(p,q),(r,s)] = d_qs sum_m G00[m,q] D[m,p] D[m,r]
 *                           + G01[r,q] D[r,p] D[q,s] + G01[p,s] D[s,q] D[p,r]
 *                           + d_pr sum_n G11[p,n] D[n,q] D[n,s];
 *   Stokes   jac_l at Re = 0 (squirmer :276-291): rows 0::2 (the omega
 *            equation) hold Lve in the columns 1::2, rows 1::2 (the psi
 *            equation) E2e in the columns 0::2 and -Me in the columns 1::2;
 *   Navier-Stokes  the same plus d(Ae omega psi)/d psi in [0::2, 0::2] and
 *            d/d omega in [0::2, 1::2] at d_state, the global vector
 *            interleaved (psi, omega) gathered through d_e2n (the five
 *            coefficients per node of SEM_OP_AXISYM_NS_JVP).
 * d_rhs: float64 [elem_count][nl] or NULL; needs d_state: minus the
 * element-local residual of the kind at the state, the reference's -res_l
 * (-A_e u_e for the two linear kinds, which read d_state for nothing else).
 *
 * h_local_order: nl entries or NULL (lexicographic): row and column a of the
 * output are local DOF h_local_order[a], so the hierarchical order of
 * reorder_local_system_hier (sem/discrete.py:428-436) is written directly.
 * d_x_phys: float64 [n_elem][2][n][n] exactly as sem_geom_fields writes it;
 * d_e2n: uint32 [n_elem][n][n]; h_D [n][n], h_w [n] as in sem_faces_create
 * (read before the call returns).  The per-node factors are derived from
 * x_phys as the stored ones are (sem_geom_from_nodes); the context's packed
 * geometry is not read.  Non-finite values on the axis: W / rho at rho = 0 is
 * formed exactly as the stored factors form it and propagates as there
 * (squirmer :217-221, the reference divides by rho as well); there is no
 * special case.  The state's size (2 * (max(d_e2n) + 1) entries, one per node
 * for Poisson) is the caller's obligation, as in sem_points_eval;
 * SEMOperator.element_matrices refuses a state of any other size.
 *
 * Checked before any device call: SEM_E_INVALID for NULL arrays, p < 1, a
 * range outside [0, n_elem], an order that is not a permutation of 0..nl-1,
 * d_rhs without d_state, SEM_OP_AXISYM_NS without d_state, an unknown kind;
 * SEM_E_NOTIMPL for p > 16, ndim != 2, SEM_OP_AXISYM_NS_JVP as a kind.  All
 * indexing is int64: the batch is [elem_count] x 52 KB at p = 8 scalar, 2.7 MB
 * at p = 16 with two DOFs per node, hence the range.  One launch on the
 * current device; allocates nothing and does not synchronise
 * (graph-capturable, like sem_apply). */
int sem_elem_matrices(int op_kind, int ndim, int p, int64_t n_elem, const double* d_x_phys,
                      const double* h_D, const double* h_w, double re, const uint32_t* d_e2n,
                      const double* d_state, const int32_t* h_local_order, int64_t elem_begin,
                      int64_t elem_count, double* d_mat, double* d_rhs, void* stream);

/* ------------------------------------------------------------------ */
/* p-multigrid: a V-cycle preconditioner of the Poisson PCG             */
/* ------------------------------------------------------------------ */
/* Levels p_0 > p_1 > ... > p_L on the same elements, each order a divisor of
 * its predecessor, so that the equispaced mesh nodes of a level are a subset
 * of the finer level's.  The reference has no counterpart (its solve is a
 * direct one, sem/discrete.py:502-528).
 *
 * Host-side planning (no device, csrc/sem_mg_plan.cpp; all arrays are HOST
 * arrays):
 *   - sem_mg_ladder: the default ladder of order p, dividing by the smallest
 *     prime factor down to 1 (16 8 4 2 1; 12 6 3 1; 9 3 1; 10 5 1; 7 1; 1),
 *     into ladder[0 .. *n_levels), *n_levels <= capacity (5 always suffices).
 *   - sem_mg_check_ladder: SEM_E_INVALID unless ladder[0 .. n_levels) is a
 *     descending divisor chain of orders in 1..16.
 *   - sem_mg_coarsen: e2n_coarse[e][i, j(, k)] = the node of e2n_fine[e][s i,
 *     s j(, s k)], s = p_fine / p_coarse, with the kept fine ids compacted in
 *     ascending order; h_keep[c] (capacity n_node_fine) is the fine id of
 *     coarse node c, *n_node_coarse their count.  Any conforming mesh, any
 *     numbering, no orientation logic.
 *   - sem_mg_coarse_mask: a coarse node is fixed iff in some element that
 *     contains it every fine node of its entity is fixed; the entity is, per
 *     local axis, the same end of the element where the coarse local index is
 *     an end and the open range 1 .. p_fine - 1 where it is not (the vertex
 *     itself, an open edge, an open face or the open interior).
 * SEM_E_INVALID for ndim not 2 or 3, orders that are no divisor pair, sizes
 * out of range (as sem_transfer_create), a NULL array, an id >= its node
 * count; SEM_E_NOTIMPL for p > 16 in sem_mg_ladder. */
int sem_mg_ladder(int p, int* ladder, int capacity, int* n_levels);
int sem_mg_check_ladder(const int* ladder, int n_levels);
int sem_mg_coarsen(int ndim, int p_fine, int p_coarse, int64_t n_elem, const uint32_t* h_e2n_fine,
                   int64_t n_node_fine, uint32_t* h_e2n_coarse, uint32_t* h_keep,
                   int64_t* n_node_coarse);
int sem_mg_coarse_mask(int ndim, int p_fine, int p_coarse, int64_t n_elem,
                       const uint32_t* h_e2n_fine, int64_t n_node_fine, const uint8_t* h_mask_fine,
                       const uint32_t* h_e2n_coarse, int64_t n_node_coarse,
                       uint8_t* h_mask_coarse);

/* The cycle z = M r (csrc/sem_mg.hip).  Level l: a Poisson context with one
 * DOF per node and its geometry set, its Dirichlet mask, D = its diagonal,
 * D^-1 := 0 on fixed DOFs.  Smoother: the degree-k Chebyshev iteration for
 * D^-1 A on [lambda_max / ratio, lambda_max],
 *     d = D^-1 r / theta;  then k - 1 times:  x += d, r -= A d,
 *     d = rho' rho d + (2 rho' / delta) D^-1 r,
 * theta = (b + a) / 2, delta = (b - a) / 2, sigma = theta / delta, rho_0 =
 * 1 / sigma, rho' = 1 / (2 sigma - rho), and a last x += d.
 *     level l < L:  x = smoother(b) from x = 0 (smooth_degree, smooth_ratio),
 *                   r = (b - A x) on free DOFs, 0 on fixed ones,
 *                   b_{l+1} = restrict(r) (sem_transfer_restrict),
 *                   the cycle of level l + 1,
 *                   x += prolong(x_{l+1}) on free DOFs,
 *                   x = smoother(b) from that x (the same polynomial);
 *     level L:      x = smoother(b) from x = 0 (coarse_degree, coarse_ratio).
 * No inner Krylov solve or dot product: M is a fixed symmetric positive
 * definite matrix on the free DOFs (given lambda_max[l] >= the largest
 * eigenvalue of D^-1 A on level l's free DOFs), so plain PCG applies.  A
 * smoothed level costs 2 smooth_degree operator actions per cycle, the
 * coarsest coarse_degree - 1 (sem_mg_info).
 *
 * sem_mg_create: ctxs [n_levels] and transfers [n_levels - 1] (transfer l:
 * "from" level l + 1 "to" level l) are BORROWED until sem_mg_destroy;
 * d_dirichlet [n_levels] device uint8 masks (read here only);
 * h_lambda_max [n_levels] host.  Allocates every vector the cycle and the
 * solve use (7 per level, 1 more on level 0; rows padded to 32 doubles).
 * SEM_E_INVALID for n_levels outside 1..16, a NULL entry, a degree < 1, a
 * ratio <= 1, a lambda_max <= 0 or not finite, a context on another device, a
 * transfer whose node counts differ from its two levels'; SEM_E_NOTIMPL for a
 * context with dofs_per_node != 1.  Synchronises `stream`. */
typedef struct sem_mg sem_mg;
int sem_mg_create(sem_mg** out, int n_levels, sem_ctx* const* ctxs,
                  sem_transfer* const* transfers, const uint8_t* const* d_dirichlet,
                  const double* h_lambda_max, int smooth_degree, int coarse_degree,
                  double smooth_ratio, double coarse_ratio, int device, void* stream);
void sem_mg_destroy(sem_mg* mg);

/* d_z = M d_r (level-0 vectors; entries of d_r on fixed DOFs are ignored, d_z
 * is 0 there; d_z must not alias d_r).  One chain of launches on `stream`:
 * allocates nothing and does not synchronise (graph-capturable, no parallel
 * branches).  Calls on one handle must be ordered: they share its vectors. */
int sem_mg_vcycle(sem_mg* mg, const double* d_r, double* d_z, void* stream);

/* One cycle as sem_mg_vcycle with events between the levels' segments:
 * h_ms [n_levels] (host) takes the milliseconds of each level (its way down
 * plus its way up; the restriction counts to the finer level, the
 * prolongation too).  Diagnostic: creates events and synchronises. */
int sem_mg_profile(sem_mg* mg, const double* d_r, double* d_z, double* h_ms, void* stream);

/* Solve K x = b on the free DOFs of level 0 with PCG preconditioned by the
 * cycle; the semantics of sem_pcg_solve: d_x carries the Dirichlet values on
 * entry, every scalar stays on the device, the r.r history is read back every
 * check_every iterations (< 1: 1), rtol = 0 runs exactly max_iter
 * iterations, SEM_E_INVALID when not converged or on a non-finite residual.
 * Dot products are fixed-order two-stage sums: two solves give the same
 * bits.  An iteration allocates nothing. */
int sem_mg_pcg_solve(sem_mg* mg, const double* d_b, double* d_x, double rtol, int max_iter,
                     int check_every, int* iters, double* relres, void* stream);

/* info[0] levels, [1] smooth_degree, [2] coarse_degree, [3] bytes of the
 * handle's vectors, then 5 values per level l at [4 + 5 l]: DOFs, operator
 * actions per cycle, vector passes of this unit per cycle (both as planned),
 * and the actions and passes the last cycle enqueued.  Writes min(n_info,
 * 4 + 5 levels) values. */
int sem_mg_info(sem_mg* mg, int64_t* info, int n_info);

#ifdef __cplusplus
}
#endif
#endif /* SEM_HIP_H */
