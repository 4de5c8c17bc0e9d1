/* mfgpu.h -- C-ABI of the MI355X-native matrix-free Laplace operator apply.
 *
 * Drop-in boundary for ONE hot path of kalj/dealii-cuda: LaplaceOperatorGpu::vmult
 * (reference laplace_operator_gpu.h:216-223) as driven by bmop.cu:134-153.
 *
 * The reference has no FFI layer: its boundary is a C++ template API whose inputs come
 * from deal.II (DoFHandler, ConstraintMatrix, FEValues, ShapeInfo).  deal.II objects cannot
 * cross a C-ABI, so this ABI sits exactly at the OUTPUT of MatrixFreeGpu::reinit
 * (matrix_free_gpu.cu:448-563) and ConstraintHandlerGpu::reinit
 * (constraint_handler_gpu.cu:68-95): plain host arrays, plain device pointers, sizes.
 * All file:line citations are relative to the reference tree.
 *
 * Conventions: every function returns 0 on success or a negative MFGPU_E* code (no C++
 * exception crosses the boundary; the reference throws dealii::ExcMessage,
 * cuda_utils.cuh:15-25); mfgpu_last_error() gives the message of the calling thread's
 * last failure.  Handles are independent (no process-global shape tables, unlike
 * matrix_free_gpu.h:45-48), thread-compatible, not thread-safe per handle.  All calls on ONE handle must be ordered on
 * a single stream (or serialised by the caller with events): every vmult uses the handle's halo buffer, so two
 * vmults of one handle in flight on different streams race on it.
 * `stream` arguments are hipStream_t passed as void* (NULL = default stream).
 */
#ifndef MFGPU_H
#define MFGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFGPU_OK 0
#define MFGPU_EINVAL (-1)   /* bad argument / inconsistent description        */
#define MFGPU_EHIP (-2)     /* HIP runtime error (message has the HIP string) */
#define MFGPU_ENOMEM (-3)
#define MFGPU_EUNSUPPORTED (-4) /* (dim, degree, number type) not instantiated */

/* number_type */
#define MFGPU_F64 0
#define MFGPU_F32 1 /* reference: -DBMOP_USE_FLOATS, bmop.cu:60-64 */

/* flags */
#define MFGPU_UNIFORM_J0 (1u << 0)    /* inv_jac holds ONE scalar J^-1[0][0] per cell
                                         (MATRIX_FREE_UNIFORM_MESH, matrix_free_gpu.cu:332-334,
                                         fee_gpu.cuh:225-241).  Without it: the reference's default
                                         geometry path, a full J^-1 per quadrature point (fee_gpu.cuh:
                                         235-241,275-281) -- implemented in two-pass
                                         scatter mode (2D and 3D, with or without hanging nodes); with
                                         MFGPU_COLORED_SCATTER: MFGPU_EUNSUPPORTED                  */
#define MFGPU_HANGING_NODES (1u << 1) /* constraint_mask is given (MATRIX_FREE_HANGING_NODES,
                                         fee_gpu.cuh:333-335,349-351)                           */

#define MFGPU_COLORED_SCATTER (1u << 8) /* scatter mode: one launch per batch colour with first-touch
                                         stores and later-colour adds (the reference's use_coloring idea,
                                         matrix_free_gpu.h:374-379, fee_gpu.cuh:359-362, at batch level).
                                         Default is the two-pass mode: one sweep over all batches, batch-
                                         surface partial sums reduced per dof by a second kernel.           */

#define MFGPU_NO_SHARED_RECORDS (1u << 9) /* plane kernels: keep the per-batch index records in their expanded form
                                         even where the plan would share repeated ones (below, "shared form"): for
                                         tests and for A/B measurements inside one build                            */

#define MFGPU_UPDATABLE_COEFFICIENTS (1u << 10) /* the operator, level or integrator created from the description
                                         keeps on the device what a re-fold of its coefficients reads, so that
                                         mfgpu_update_coefficients / mfgpu_level_update_coefficients /
                                         mfgpu_integrator_update_coefficients (below) can replace a and c from device
                                         arrays without a new plan: JxW [n_cells * n^dim], inv_jac (one scalar per cell,
                                         or the full J^-1 per point), the plan's cell order [n_cells] (uint32) and, where
                                         the cell loop runs a plane kernel, two uint32 tables over the plane batches'
                                         cells.  Opt-in because of the memory: mfgpu_memory_consumption grows by exactly
                                         these bytes -- with the full J^-1 in 3D (8 + 72 =) 80 B per quadrature point in
                                         double; with MFGPU_UNIFORM_J0 8 B per point plus 12 B per cell (20 on plane plans).  Plan, kernel
                                         choice and every result are the same with and without the flag;
                                         mfgpu_plan_create and mfgpu_suggest_renumbering ignore it.                  */

typedef struct mfgpu_handle mfgpu_handle; /* replaces MatrixFreeGpu + coefficient + ConstraintHandlerGpu
                                             inside LaplaceOperatorGpu (laplace_operator_gpu.h:85-95) */

/* Output of MatrixFreeGpu::reinit / ConstraintHandlerGpu::reinit as plain HOST arrays.
 * Per-cell arrays are UNPADDED (row length n^dim, not the power-of-two `rowlength` of
 * matrix_free_gpu.cu:483) and hold all cells of all colours in one array; colouring is
 * done by the library (coloring.cc:8-33 is replaced).                       */
typedef struct mfgpu_desc {
  int32_t dim;         /* 2 or 3                                    (bmop.cu:53-57)   */
  int32_t degree;      /* FE_Q degree p, n = p+1 points per direction (bmop.cu:47-51) */
  int32_t number_type; /* MFGPU_F64 / MFGPU_F32: type of every `const void*` array and of the vectors */
  uint32_t flags;
  uint32_t n_dofs;  /* vector length                              (matrix_free_gpu.cu:494)     */
  uint32_t n_cells; /* active cells                               (matrix_free_gpu.cu:495)     */
  const uint32_t *loc2glob;        /* [n_cells * n^dim] lexicographic (x fastest), hanging-node
                                      entries already substituted   (matrix_free_gpu.cu:287-300).
                                      ANY cell-to-dof map with entries < n_dofs is accepted; the operator is
                                      A = sum_cells P_c^T K_c P_c with P_c the gather through the cell's entries.
                                      In particular: dofs identified across periodic boundaries (rings of 1, 2, ...
                                      cells and tori included), one dof listed several times by one cell, any
                                      numbering of the dofs, any order of the cells, ids no cell lists (rows of
                                      zeros, or identity rows where constrained), and a vertex with more than 8
                                      cells.  The one limit: the batches that list one dof must get different
                                      colours (both scatter modes), and there are 64 colours -- a dof listed by
                                      cells of more than 64 batches (a vertex of valence 125 under
                                      max_cells_per_batch = 1) is refused with MFGPU_EUNSUPPORTED, "more than 64
                                      batch colours needed".  Larger batches lift such a case below the limit.   */
  const uint32_t *constraint_mask; /* [n_cells] or NULL              (hanging_nodes.cuh:23-53)   */
  const void *JxW;                 /* [n_cells * n^dim]              (matrix_free_gpu.cu:315-322) */
  const void *inv_jac;             /* UNIFORM_J0: [n_cells]; else [n_cells * n^dim * dim*dim],
                                      per quadrature point row-major J^-1[d1][d2]
                                      (matrix_free_gpu.cu:324-338)                                */
  const void *coefficient;         /* [n_cells * n^dim] values at quadrature points, or NULL to
                                      evaluate 1/(0.05+2|x|^2) from quadrature_points on the device
                                      (laplace_operator_gpu.h:191-211, poisson_common.h:149-151)   */
  const void *quadrature_points;   /* [n_cells * n^dim * dim] (x,y,z per point) or NULL
                                      (matrix_free_gpu.cu:305-313)                                */
  const void *shape_values;        /* [n*n], index dof*n + q         (matrix_free_gpu.cu:502-509) */
  const void *shape_gradients;     /* [n*n], index dof*n + q         (matrix_free_gpu.cu:510-513) */
  const double *constraint_weights; /* [n*n] row-major W[i][j] or NULL (hanging_nodes.cuh:580-598) */
  const uint32_t *constrained_dofs; /* ascending list of every constrained DoF, Dirichlet AND
                                       hanging                        (constraint_handler_gpu.cu:68-95) */
  uint32_t n_constrained;
  /* tuning knobs, 0 = library default (no reference counterpart; replaces
     cells_per_block_shmem, matrix_free_gpu.h:298-315) */
  uint32_t max_cells_per_batch;
  uint32_t max_dofs_per_batch;
  uint32_t kernel; /* MFGPU_KERNEL_*: which cell-loop kernel family to use; 0 = the library's choice */
  uint32_t cell_loop_segments; /* two-pass mode: the cell loop runs as this many launches over consecutive batch
                                  ranges; the shared-dof sums (pass 2) a finished range completes run on a side
                                  stream of the handle, next to the following range's cells.  0 = the library's
                                  choice, 1 = one launch, pass 2 strictly after it                              */
  uint32_t max_workgroups;     /* cap on the resident workgroups of the persistent cell-loop launches (0 = as many
                                  as fit on the device): leaves room for other work on the GPU; also lets small
                                  meshes exercise the multi-batch loop of a workgroup                          */
  const void *mass_coefficient; /* [n_cells * n^dim] values of c at the quadrature points (number_type), or NULL:
                                   adds the mass term int c u v to the operator, A = sum_cells P^T C^T (K_cell + M_cell)
                                   C P with M_cell[i][j] = sum_q phi_i(x_q) phi_j(x_q) c_q JxW_q on free rows, the
                                   identity on constrained rows as before.  NULL = no mass term (the Laplace operator).
                                   c is not checked for sign (a Helmholtz operator with c < 0 is the caller's business).
                                   A pure mass matrix: coefficient = zeros plus mass_coefficient.  No reference
                                   counterpart (LaplaceOperatorGpu has the stiffness term only; this is the value half
                                   of FEEvaluationGpu, fee_gpu.cuh: evaluate / get_value / submit_value / integrate).
                                   Carried by everything created from a description: mfgpu_create, mfgpu_level_create
                                   (level operator and interface matrices), mfgpu_integrator_create (Dirichlet lift).
                                   Ignored by mfgpu_plan_create and mfgpu_suggest_renumbering: the plan of a degree does
                                   not depend on it, except that mfgpu_create serves p = 5, 6 in 3D with apply_batches_x
                                   when the field is set.  Appended last: a caller that zeroes
                                   the struct before filling it keeps today's operator.                                */
} mfgpu_desc;

/* sizeof(mfgpu_desc) of the library: lets a binding check its mirror of the struct against this header */
size_t mfgpu_desc_size(void);

/* mfgpu_desc.kernel (all variants compute the same operator; non-default ones exist for tests and measurements).
 * With a mass term every family has an instantiation except the plane kernels at p = 5, 6 (apply_planes4w, whose
 * registers the extra plane does not fit) and MFGPU_KERNEL_PLANES_2W at p = 4 in double (it would spill): forcing
 * one of them returns MFGPU_EUNSUPPORTED.                                                                            */
#define MFGPU_KERNEL_AUTO 0
#define MFGPU_KERNEL_PENCILS 1   /* apply_batches: a thread owns a 1D pencil, 2 workgroups per CU (2D; coloured mode)   */
#define MFGPU_KERNEL_PENCILS_X 2 /* apply_batches_x: the same for 3 workgroups per CU (3D two-pass; hanging nodes)      */
#define MFGPU_KERNEL_PLANES 3    /* apply_planes3: a thread owns a 2D plane, one wave per batch, one wave per SIMD (3D, p = 2..4) */
#define MFGPU_KERNEL_PLANES_2W 4 /* apply_planes4: the same plan and records with half the resources per wave -- one LDS
                                    transpose array aliased with the batch array, <= 256 registers -- for two waves per
                                    SIMD; measures equal to apply_planes3 on MI355X (profiles/r03_notes.md), not the default */

/* ---- operator (replaces LaplaceOperatorGpu::reinit / vmult / vmult_add / clear) -------- */

/* laplace_operator_gpu.h:120-151 (reinit): copies the description to the device, builds the
 * batch plan, folds coefficient * J0^2 * JxW (general geometry: the symmetric coefficient * JxW * J^-1 J^-T per
 * quadrature point) and, with mass_coefficient, the mass weight c * JxW.  Uses the current HIP device.  Fails
 * (MFGPU_EHIP) if no HIP device / kernel image is available: there is no CPU fallback.        */
int mfgpu_create(const mfgpu_desc *desc, mfgpu_handle **out);

/* laplace_operator_gpu.h:216-223: dst = A src.  dst, src: device vectors of n_dofs Numbers.
 * Unlike the reference (const_cast at :293,302) src is never written.  Asynchronous.         */
int mfgpu_vmult(mfgpu_handle *h, void *dst_dev, const void *src_dev, void *stream);

/* laplace_operator_gpu.h:286-303: dst += A src on free rows, dst_c += src_c on constrained rows. */
int mfgpu_vmult_add(mfgpu_handle *h, void *dst_dev, const void *src_dev, void *stream);

/* ---- the operator applied to several vectors at once (the components of a vector Laplacian, several right-hand sides,
 * block Krylov methods).  On general geometry (3D, no MFGPU_UNIFORM_J0: apply_batches_g) an apply mostly streams the
 * folded metric, which does not depend on the vector; a FUSED group of 2 or 3 vectors reads it, the dof lists and the
 * index runs once (apply_batches_g and reduce_classes at width 2 or 3).  Every other handle -- 2D, the uniform-Jacobian families,
 * coloured scatter -- has no fused instantiation and applies the vectors one by one.                                  */
#define MFGPU_MULTI_ADD   (1u << 0) /* vmult_add semantics for every vector */
#define MFGPU_MULTI_LOOP  (1u << 1) /* one single-vector apply per vector (tests, A/B inside one build) */
#define MFGPU_MULTI_FUSED (1u << 2) /* fused groups or MFGPU_EUNSUPPORTED: never fall back silently */

/* dst_k = A src_k (MFGPU_MULTI_ADD: dst_k += A src_k on free rows, dst_k += src_k on constrained rows), k < n_vectors;
 * vector k starts at element k * stride of dst_dev / src_dev (handle's number type).  Asynchronous on `stream` and
 * ordered like every call on the handle; src is never written; the elements n_dofs .. stride - 1 of every vector are
 * never touched.  n_vectors is cut into groups of the handle's fused widths, widest first (7 = 3 + 3 + 1); a remainder of
 * one vector and every handle without a fused instantiation go through the single-vector path.  Without
 * MFGPU_MULTI_LOOP / _FUSED the library fuses where that measured faster per vector (table in mfgpu_api.hip) and loops
 * elsewhere; with MFGPU_MULTI_FUSED it fuses wherever mfgpu_multi_width(h) > 1 and returns MFGPU_EUNSUPPORTED where it is
 * 1 (n_vectors == 1 included: nothing to fuse).  A handle with cell_loop_segments > 1 runs a fused group as ONE segment,
 * pass 2 after the cell loop on `stream`.
 * MFGPU_EINVAL, nothing written: n_vectors == 0; stride < n_dofs with n_vectors > 1; LOOP and FUSED both set; unknown
 * flag bits; the dst range [dst, dst + (n_vectors - 1) * stride + n_dofs) overlaps the src range.
 * Memory: a fused group of width W sums its shared dofs through W halo buffers.  The handle owns one; the buffers
 * 2 .. mfgpu_multi_width(h) are allocated together by the FIRST call that runs a fused group.  That is the only
 * allocation and the only possible host synchronisation of this function: a caller that captures graphs calls it once
 * before capturing.  The buffers count in mfgpu_memory_consumption from then on; mfgpu_destroy frees them.             */
int mfgpu_vmult_multi(mfgpu_handle *h, void *dst_dev, const void *src_dev, uint32_t n_vectors, size_t stride,
                      uint32_t flags, void *stream);
/* widest group one fused sweep of this handle serves; 1 = every vector is a single apply */
int mfgpu_multi_width(const mfgpu_handle *h);

/* New coefficients for an operator created with MFGPU_UPDATABLE_COEFFICIENTS (no reference counterpart: the reference
 * evaluates its coefficient once, in reinit).  coefficient_dev / mass_coefficient_dev: DEVICE arrays [n_cells * n^dim] of
 * the handle's number type, values at the quadrature points in the description's cell order; NULL leaves that term as it
 * is.  Folds with the kernels and the arithmetic of mfgpu_create into the handle's existing arrays: afterwards vmult,
 * vmult_add, vmult_dist* and compute_inverse_diagonal are those of a handle created with the new values.  Asynchronous on
 * `stream` and ordered like every other call on the handle; allocates nothing, does not synchronise with the host, reads
 * the arrays when the stream gets there.  MFGPU_EINVAL (nothing is written): no MFGPU_UPDATABLE_COEFFICIENTS at
 * creation; both pointers NULL; mass_coefficient_dev on a handle created without mass_coefficient (its kernels were
 * bound without the mass term, and at p = 5, 6 the kernel family depends on it).  A handle created with coefficient =
 * NULL (the built-in 1/(0.05+2|x|^2)) is updated from an explicit array like any other.                              */
int mfgpu_update_coefficients(mfgpu_handle *h, const void *coefficient_dev, const void *mass_coefficient_dev,
                              void *stream);

/* laplace_operator_gpu.h:53-54 m() / n() */
uint32_t mfgpu_n_dofs(const mfgpu_handle *h);

/* laplace_operator_gpu.h:434-445 */
size_t mfgpu_memory_consumption(const mfgpu_handle *h);

/* laplace_operator_gpu.h:110-117 (clear) / matrix_free_gpu.cu:566-596 (free) */
void mfgpu_destroy(mfgpu_handle *h);

const char *mfgpu_last_error(void);

/* Plan statistics (for DESIGN/bench reporting and the CPU-side host-logic tests).
 * stats[0]=n_batches [1]=cell-loop launches per vmult (colours; 1 in two-pass mode) [2]=total batch dofs
 * [3]=max dofs/batch [4]=max cells/batch [5]=n_orphan_dofs
 * [6]=first-touch stores (coloured) / shared dofs (two-pass) [7]=RMW adds (coloured) / halo slots (two-pass) */
int mfgpu_plan_stats(const mfgpu_handle *h, uint64_t stats[8]);

/* Index records of the plane kernels: stats[0] bit 0 = the cell loop reads the shared form (repeated per-batch records
 * stored once; 0: the expanded form), bit 1 = pass 2 does [1]=distinct dof-list records [2]=distinct index-run
 * records (both counted either way; 0 without plane batches) [3]=bytes of the cell loop's records on the device    */
int mfgpu_record_stats(const mfgpu_handle *h, uint64_t stats[4]);

/* Name of the cell-loop kernel this operator launches ("apply_batches_x", "apply_batches", ...): the
 * kernel the roofline figures of bench.py and the rocprofv3 summaries under profiles/ refer to.      */
const char *mfgpu_kernel_name(const mfgpu_handle *h);

/* Average device time of the cell-loop kernels of the most recent mfgpu_vmult* calls, measured
 * with hipEvents on the launch stream when profiling is enabled (bench.py roofline leg).       */
int mfgpu_profile_enable(mfgpu_handle *h, int on);
int mfgpu_profile_read(mfgpu_handle *h, double *kernel_ms_total, uint64_t *n_vmults);
/* ... and of the pass-2 kernels (reduce_classes) of the same mfgpu_vmult / mfgpu_vmult_add calls: 0 in coloured mode. */
int mfgpu_profile_read_pass2(mfgpu_handle *h, double *pass2_ms_total);

/* ---- host-only plan (no GPU needed): same planner the handle uses -------------------------
 * Lets CPU tests check the batching / colouring / first-touch logic.                         */
typedef struct mfgpu_plan mfgpu_plan;
int mfgpu_plan_create(const mfgpu_desc *desc, mfgpu_plan **out);
void mfgpu_plan_destroy(mfgpu_plan *p);
/* what: 0 batch_cell_off[n_batches+1] 1 batch_dof_off[n_batches+1] 2 color_batch_off[n_colors+1]
 *       3 cell_order[n_cells] (plan position -> caller cell) 4 bdofs[total] 5 orphans[n_orphans]
 *       6 batch_nint[n_batches] 7 halo_off[n_batches+1] 8 sdofs[n_shared] 9 s_off[n_shared+1] 10 s_idx
 *       11 chunks[4*n_chunks] {sdofs position, count | k<<16, gstarts offset, offset in group} 12 gstarts
 *       plane plans (apply_planes3): 13 dof-list records [n_plane_batches * slots * 64] 14 index-run records
 *       15 hanging-node records of the batches of masked cells (layout: mfgpu_internal.h p_hn_rows)
 *       16 per plane batch the index of its record in 15, or 0xffffffff (a batch of cells without a mask)
 *       shared form of 13 / 14 (every distinct record once): 17 distinct dof-list records, each entry minus the
 *       batch's smallest dof id (bit 31 kept) 18 distinct index-run records 19 per plane batch 4 words {smallest dof
 *       id, record number in 17, record number in 18, 0}
 *       shared form of pass 2 (8-10 regrouped by the batch of a dof's first partial sum, distinct records once):
 *       20 records 21 per batch {smallest dof id, word offset of its record in 20} (layout: mfgpu_internal.h Plan)
 * returns element count, *ptr = host pointer valid until mfgpu_plan_destroy                  */
int64_t mfgpu_plan_array_u32(const mfgpu_plan *p, int what, const uint32_t **ptr);
/* bit 0: a handle of this plan reads the shared form of the cell loop's records (it is clearly smaller than 13 + 14);
 * bit 1: the same for pass 2 (20 + 21 against the class arrays built from 8-10)                                    */
int mfgpu_plan_shares_records(const mfgpu_plan *p);
/* How mfgpu_vmult_multi cuts n_vectors into groups for a handle with the given fused widths (descending): widest first,
 * what is left over as groups of 1.  Writes at most `capacity` group sizes and returns their number.                */
int mfgpu_plan_multi_groups(uint32_t n_vectors, const uint32_t *widths, uint32_t n_widths, uint32_t *groups,
                            uint32_t capacity);
int64_t mfgpu_plan_lmap(const mfgpu_plan *p, const uint16_t **ptr);   /* [n_cells*n^dim], plan order */
int64_t mfgpu_plan_bflags(const mfgpu_plan *p, const uint8_t **ptr);  /* bit0 constrained, bit1 add */

/* ---- optional: a dof numbering that suits the operator (deal.II's MatrixFree::renumber_dofs; the reference does not
 * renumber, and nothing here requires it).  new_index[old dof] = new dof, batch-major: the dofs of a batch are one
 * contiguous run (coalesced gathers and stores of the cell loop), the dofs shared between batches follow in the order
 * pass 2 walks them.  The caller renumbers ITS DoFHandler (DoFHandler::renumber_dofs; stand-in: mfgpu_mesh_renumber)
 * and describes the renumbered mesh to mfgpu_create; vectors then live in the new numbering.  Host only.          */
int mfgpu_suggest_renumbering(const mfgpu_desc *desc, uint32_t *new_index /* [n_dofs] */);

/* ---- what a CG / Chebyshev caller needs from the operator besides vmult -------------
 * LaplaceOperatorGpu::compute_diagonal + get_diagonal_inverse (laplace_operator_gpu.h:401-429): writes
 * 1 / diag(A) into inv_diag[n_dofs] (device, operator's number type); the local diagonal of every cell
 * (DiagonalLocalOperator, :355-399) is distributed like a cell result, including the transposed hanging-node
 * resolution, constrained rows are set to 1 before the inversion (:412-414).  With a mass term the local diagonal is
 * K_ii + M_ii, M_ii = sum_q c_q JxW_q prod_d S[i_d][q_d]^2.
 * Asynchronous on `stream` and ordered like every call on the handle.  Memory: the FIRST call on a handle uploads two
 * small 1D tables (2 n^2 numbers) with a blocking copy.  That is the only allocation and the only host synchronisation
 * of this function: a caller that captures graphs calls it once before capturing.  The bytes count in
 * mfgpu_memory_consumption from then on; mfgpu_destroy frees them.                                         */
int mfgpu_compute_inverse_diagonal(mfgpu_handle *h, void *inv_diag, void *stream);
/* ConstraintHandlerGpu::set_constrained_values (constraint_handler_gpu.cu:126-137): vec[c] = value for every
 * constrained dof c of the description.                                                                   */
int mfgpu_set_constrained_values(mfgpu_handle *h, void *vec, double value, void *stream);

/* ---- GpuVector BLAS-1 and reductions (gpu_vec.h:105-157, gpu_vec.cu:222-617) -------
 * v, w, x: device vectors of n elements of number_type.  The element-wise operations are asynchronous on
 * `stream`; the reductions block until the result is on the host (as the reference's do, gpu_vec.cu:556-560)
 * and accumulate in double in a fixed order (deterministic).  The reductions synchronise `stream` and cannot be
 * captured in a graph; the first one on a device allocates its scratch of partial sums.                     */
int mfgpu_vec_sadd(void *v, double s, double a, const void *w, size_t n, int number_type, void *stream);  /* v = s v + a w   gpu_vec.cu:308-314 */
int mfgpu_vec_equ(void *v, double a, const void *w, size_t n, int number_type, void *stream);             /* v = a w         :346-352 */
int mfgpu_vec_scale(void *v, const void *w, size_t n, int number_type, void *stream);                     /* v[i] *= w[i]    :320-325 */
int mfgpu_vec_divide(void *v, const void *w, size_t n, int number_type, void *stream);                    /* v[i] /= w[i]    :328-333 */
int mfgpu_vec_invert(void *v, size_t n, int number_type, void *stream);                                   /* v[i] = 1/v[i]   :336-342 */
int mfgpu_vec_mul(void *v, double a, size_t n, int number_type, void *stream);                            /* v *= a          :357-362 */
int mfgpu_vec_dot(const void *v, const void *w, size_t n, int number_type, void *stream, double *result); /* v . w           :542-563 */
int mfgpu_vec_l2_norm(const void *v, size_t n, int number_type, void *stream, double *result);            /* sqrt(v . v)     :367-369 */
int mfgpu_vec_add_and_dot(void *v, double a, const void *x, const void *w, size_t n, int number_type,
                          void *stream, double *result);                              /* v += a x; return v . w   :597-617 */
int mfgpu_vec_all_zero(const void *v, size_t n, int number_type, void *stream, int *result);              /* :512-540 */

/* ---- GpuVector pieces that are on the path (gpu_vec.h:44,69,84-88,164-172) -------------- */
/* gpu_vec.cu:166-182, zero-filled; the fill is complete when the call returns, so the vector reads as zero on every
 * stream, non-blocking ones included (a set-up call: it synchronises the null stream)                            */
int mfgpu_vec_alloc(void **dev, size_t n, int number_type);
int mfgpu_vec_free(void *dev);
int mfgpu_vec_fill(void *dev, size_t n, int number_type, double value, void *stream); /* vec_init, gpu_vec.cu:281-291 */
int mfgpu_vec_from_host(void *dev, const void *host, size_t n, int number_type);
int mfgpu_vec_to_host(void *host, const void *dev, size_t n, int number_type);
int mfgpu_device_synchronize(void);
/* free / total bytes of the current device (hipMemGetInfo): lets callers and tests check that
 * mfgpu_destroy / mfgpu_vec_free return everything mfgpu_create / mfgpu_vec_alloc took              */
int mfgpu_device_memory_info(size_t *free_bytes, size_t *total_bytes); /* bmop.cu:148 */

/* ---- guard mode: a debugging aid for the library's OWN device arrays (no reference counterpart) ---------------
 * Off by default and switched by these calls only; the library reads no environment variable.  While the mode is on,
 * every device array a handle allocates (halo, batch arrays, workspaces, the solvers' vectors; not mfgpu_vec_alloc's
 * caller vectors and not the static buffer of the blocking reductions) is one allocation
 *     [front guard | payload | back guard]
 * whose payload begins at a multiple of 256 bytes, at least guard_bytes in, and whose back guard of guard_bytes bytes
 * begins at the payload's last byte + 1.  Both guards hold 0xFF bytes (a NaN as double and as float).  A payload of
 * floating-point numbers that the library allocates WITHOUT filling it holds the same bytes, so a kernel that uses a
 * slot nothing wrote returns NaN; zero-filled and uploaded payloads are what they always are, and arrays of integers
 * are never poisoned.  The fills are complete when the allocating call returns.  mfgpu_*_memory_consumption keeps
 * counting payload bytes only.  Arrays allocated before _begin are neither padded nor registered; arrays allocated
 * during the mode stay registered, and checked, until they are freed, also after _end.  Set-up calls only: do not
 * switch the mode while another thread creates or destroys handles.
 *   _begin   guard_bytes in [1, 2^30], else MFGPU_EINVAL; a second _begin changes the size for later allocations
 *   _layout  the padding arithmetic alone (needs no device): total bytes of the allocation and the payload's offset
 *   _check   synchronises the device, copies both guards of every registered array to the host and compares them byte
 *            for byte.  n_live: registered arrays; n_damaged: damaged guards (an array has two).  report (len bytes,
 *            may be NULL with len 0) gets one line for each of the first 8 damaged guards:
 *              "array #<ordinal> (<payload bytes> payload bytes): back guard, offset +<k>: 0x<byte>"
 *              "array #<ordinal> (<payload bytes> payload bytes): front guard, offset -<k>: 0x<byte>"
 *            with the damaged byte nearest the payload: +0 is the first byte behind it, -1 the last in front of it.
 *            Ordinals count the mode's allocations from 0 in allocation order.
 *   _selftest  (guard mode only, else MFGPU_EINVAL) allocates one unfilled and one zero-filled array of doubles and
 *            reads both back: *poisoned_ok = the first is all 0xFF, *zeroed_ok = the second all zero.  It then copies
 *            8 bytes of 0x5a over the first bytes behind the unfilled array's payload and 8 over the last bytes in front
 *            of it -- both inside that array's own allocation --, returns what _check then reports, and frees both.   */
int mfgpu_debug_guard_begin(size_t guard_bytes);
int mfgpu_debug_guard_end(void);
int mfgpu_debug_guard_layout(size_t bytes, size_t guard_bytes, size_t *total, size_t *payload_offset);
int mfgpu_debug_guard_check(uint64_t *n_live, uint64_t *n_damaged, char *report, size_t len);
int mfgpu_debug_guard_selftest(uint64_t *n_damaged, char *report, size_t len, int *poisoned_ok, int *zeroed_ok);

/* ---- single-node multi-GPU mode (no reference counterpart: the reference is single-GPU) --------
 * One process per GPU; the mesh is cut into z-slabs (mfgpu_mesh_create_uniform's slab arguments), each rank owns the
 * vector entries of its slab including both interface planes.  After the slab's cell loop an interface plane holds
 * only the rank's own cells' contributions; the exchange adds the neighbour's, leaving the full sum on both sharers
 * (constrained rows are identity rows on both sides and are not summed).  Transport: RCCL point-to-point send / recv
 * with the two z-neighbours on a side stream, overlapped with pass 2 of the slab's other dofs.                       */
typedef struct mfgpu_dist mfgpu_dist;
/* rank 0: a 128-byte RCCL unique id to hand to every rank (any out-of-band channel) */
int mfgpu_dist_unique_id(void *id128);
/* collective over all ranks when id128 != NULL and world > 1 (ncclCommInitRank on the current HIP device).
 * lower_ids / upper_ids: local dof ids of the slab's lower / upper interface plane in the order both neighbours
 * agree on (mfgpu_mesh_interface_dofs); constrained: the description's constrained_dofs.  id128 == NULL: no RCCL
 * communicator; the neighbours are connected in-process with mfgpu_dist_connect_local (tests).                    */
int mfgpu_dist_create(const void *id128, int rank, int world, const uint32_t *lower_ids, uint32_t n_lower,
                      const uint32_t *upper_ids, uint32_t n_upper, const uint32_t *constrained_dofs,
                      uint32_t n_constrained, uint32_t n_dofs, int number_type, mfgpu_dist **out);
int mfgpu_dist_connect_local(mfgpu_dist *lower_rank, mfgpu_dist *upper_rank);
/* tells the operator which dofs the exchange needs first (re-orders its pass 2); once per (operator, dist) pair */
int mfgpu_dist_attach(mfgpu_dist *d, mfgpu_handle *h);
/* the schedule mfgpu_dist_attach chose: info[0] = 1: interface-first (the batches [0, info[1]) and
 * [info[2], info[3]) touch an interface plane and run first, their pass 2, the pack and the exchange run on a side
 * stream next to the interior batches [info[1], info[2]) and the rest of pass 2); 0: whole cell loop, then the exchange
 * next to pass 2 of the non-interface dofs (thin slabs, segmented or coloured cell loops)                              */
int mfgpu_dist_schedule(const mfgpu_dist *d, uint32_t info[4]);
/* dst = A src on the slab, then the exchange.  _begin: cell loop, pass 2 of the interface dofs, start of the
 * transfers (side stream), pass 2 of the rest; _end: wait for the transfers, add.  mfgpu_vmult_dist = both (RCCL
 * transport or world == 1; with the in-process transport call _begin on every slab before any _end).             */
int mfgpu_vmult_dist_begin(mfgpu_handle *h, mfgpu_dist *d, void *dst_dev, const void *src_dev, void *stream);
int mfgpu_vmult_dist_end(mfgpu_handle *h, mfgpu_dist *d, void *dst_dev, void *stream);
int mfgpu_vmult_dist(mfgpu_handle *h, mfgpu_dist *d, void *dst_dev, const void *src_dev, void *stream);
void mfgpu_dist_destroy(mfgpu_dist *d);

/* ---- multigrid level transfer (MGTransferMatrixFreeGpu, mg_transfer_matrix_free_gpu.h:140-252,
 * mg_transfer_matrix_free_gpu.cu:391-660) between two globally refined levels.  The boundary is the output of
 * MGTransferMatrixFreeGpu::build (:150-330): per coarse cell its (p+1)^dim level dofs and the (2p+1)^dim level dofs of
 * the patch of its children, both lexicographic (level_dof_indices), the coarse level's Dirichlet dofs
 * (dirichlet_indices) and the 1D prolongation matrix (shape_values; NULL = FE_Q on Gauss-Lobatto nodes).  The level
 * operators are ordinary mfgpu_handles of the level meshes (LaplaceOperatorGpu::reinit(dof_handler,
 * mg_constrained_dofs, level), laplace_operator_gpu.h:154-186).                                                      */
typedef struct mfgpu_transfer mfgpu_transfer;
int mfgpu_transfer_create(int dim, int degree, int number_type, uint32_t n_coarse_cells,
                          const uint32_t *coarse_cell_dofs /* [n_coarse_cells * (p+1)^dim]  */,
                          const uint32_t *fine_patch_dofs  /* [n_coarse_cells * (2p+1)^dim] */, uint32_t n_coarse_dofs,
                          uint32_t n_fine_dofs, const uint32_t *coarse_dirichlet, uint32_t n_coarse_dirichlet,
                          const double *prolongation_1d /* [(2p+1) * (p+1)], fine index major, or NULL */,
                          mfgpu_transfer **out);
/* :595-627  dst_fine = P (src_coarse with the coarse Dirichlet dofs read as 0); every fine dof is written */
int mfgpu_transfer_prolongate(mfgpu_transfer *t, void *dst_fine_dev, const void *src_coarse_dev, void *stream);
/* :631-660  dst_coarse += P^T src_fine on the non-Dirichlet coarse dofs (floating-point atomics, as the reference) */
int mfgpu_transfer_restrict_and_add(mfgpu_transfer *t, void *dst_coarse_dev, const void *src_fine_dev, void *stream);
/* dst_fine += P src_coarse: the coarse-grid correction of a V-cycle in one pass.  The prolongation kernel with a plain
 * read-modify-write by the owner patch of every fine dof (no atomics: deterministic); fine dofs no patch lists are left
 * alone.  The same numbers as mfgpu_transfer_prolongate into a temporary followed by mfgpu_vec_sadd(dst, 1, 1, tmp).    */
int mfgpu_transfer_prolongate_add(mfgpu_transfer *t, void *dst_fine_dev, const void *src_coarse_dev, void *stream);
size_t mfgpu_transfer_memory_consumption(const mfgpu_transfer *t); /* :333-347 */
void mfgpu_transfer_destroy(mfgpu_transfer *t);

/* ---- p-multigrid: the transfer between FE_Q(degree_coarse) and FE_Q(degree_fine) on the SAME
 * cells, 1 <= degree_coarse < degree_fine <= 6, for callers who have one mesh and no coarser meshes behind it: the same
 * triangulation with a second DoFHandler of lower degree is the coarse level.  Per cell its (pc+1)^dim
 * coarse dofs and its (pf+1)^dim fine dofs, both lexicographic in the cell's own frame (the two descriptions' loc2glob,
 * same cell order).  prolongation_1d [(pf+1) * (pc+1)], fine index major, or NULL = the coarse FE_Q Lagrange basis
 * (Gauss-Lobatto nodes) evaluated at the fine FE_Q nodes.  Conforming meshes only (no hanging-node masks).  The object
 * is an mfgpu_transfer: prolongate / prolongate_add / restrict_and_add / memory_consumption / destroy and mfgpu_vcycle
 * take it like an h-transfer, with the same semantics -- every fine dof is owned by the first cell that lists it;
 * prolongate is the owner's plain store with the coarse Dirichlet dofs read as 0 (fine dofs no cell lists are zeroed);
 * prolongate_add the owner's plain read-modify-write; restrict_and_add reads a fine dof through its owner, skips the
 * coarse Dirichlet dofs and accumulates with floating-point atomics.  All three only enqueue work.  h- and p-transfers
 * mix freely in one V-cycle (h-levels at degree 1, then degree 1 -> 2 -> 4 on the finest mesh).
 * MFGPU_EINVAL, nothing created: degree_coarse >= degree_fine, a degree outside 1..6, null arrays, a dof index outside
 * its vector, dof counts >= 2^31.                                                                                     */
int mfgpu_transfer_create_p(int dim, int degree_coarse, int degree_fine, int number_type, uint32_t n_cells,
                            const uint32_t *coarse_cell_dofs /* [n_cells * (pc+1)^dim] */,
                            const uint32_t *fine_cell_dofs /* [n_cells * (pf+1)^dim] */, uint32_t n_coarse_dofs,
                            uint32_t n_fine_dofs, const uint32_t *coarse_dirichlet, uint32_t n_coarse_dirichlet,
                            const double *prolongation_1d /* [(pf+1) * (pc+1)], fine index major, or NULL */,
                            mfgpu_transfer **out);
/* host only: the default matrix of mfgpu_transfer_create_p, [(pf+1) * (pc+1)]; rows of fine nodes that are coarse nodes
 * (the end points; 1/2 when both degrees are even) hold exact zeros and a one                                        */
int mfgpu_transfer_p_prolongation_1d(int degree_coarse, int degree_fine, double *p1);
/* The p-transfer on cells with hanging nodes: an active DoFHandler with hanging nodes at two
 * degrees.  The arguments of mfgpu_transfer_create_p -- both index lists in the description's form, hanging entries
 * already substituted -- and two more:
 *   constraint_mask            [n_cells], the mfgpu_desc.constraint_mask of BOTH descriptions (it is geometric, so the same
 *                              at every degree); NULL: conforming, the object is the one mfgpu_transfer_create_p makes
 *   coarse_constraint_weights  [(pc+1)^2] row-major, the COARSE description's constraint_weights; NULL: those of FE_Q(pc)
 * A local position of a cell is CONSTRAINED if resolve_hanging_nodes with the cell's mask can write it (a position on a
 * flagged face, in 3D also on a flagged edge).  The owner of a fine dof is the first cell, in cell order, that lists it at
 * a position that is not constrained.  For the owner cell K and owned position i
 *   (P x)[fine(K, i)] = [ P_loc C_pc(mask_K) gather_K(x with the coarse Dirichlet dofs read as 0) ]_i
 * with C_pc = resolve_hanging_nodes<NOTRANSPOSE> at degree pc and P_loc the tensor product of prolongation_1d.  The three
 * calls keep their meaning: prolongate stores (fine dofs no cell lists -- the hanging ones -- become 0), prolongate_add
 * read-modify-writes (and leaves those alone), restrict_and_add adds Z P^T src with floating-point atomics.  Only
 * enqueue, as before.
 * MFGPU_EINVAL, nothing created: what mfgpu_transfer_create_p refuses; a mask with bits outside the 9 defined ones, or in
 * 2D with one of the 3D bits (TYPE z, FACE z, EDGE); a fine dof that some cell lists but no cell owns (masks and index
 * lists that do not belong together).                                                                               */
int mfgpu_transfer_create_p_hn(int dim, int degree_coarse, int degree_fine, int number_type, uint32_t n_cells,
                               const uint32_t *coarse_cell_dofs /* [n_cells * (pc+1)^dim] */,
                               const uint32_t *fine_cell_dofs /* [n_cells * (pf+1)^dim] */, uint32_t n_coarse_dofs,
                               uint32_t n_fine_dofs, const uint32_t *coarse_dirichlet, uint32_t n_coarse_dirichlet,
                               const double *prolongation_1d /* [(pf+1) * (pc+1)], fine index major, or NULL */,
                               const uint32_t *constraint_mask /* [n_cells] or NULL */,
                               const double *coarse_constraint_weights /* [(pc+1)^2] or NULL */, mfgpu_transfer **out);
/* host only, no device needed: the fine index list as the create calls upload it, bit 31 set on every entry but the
 * owner's; constraint_mask NULL: the first cell that lists a dof owns it.  MFGPU_EINVAL as above.                     */
int mfgpu_transfer_p_owner_list(int dim, int degree_fine, uint32_t n_cells, const uint32_t *fine_cell_dofs,
                                const uint32_t *constraint_mask /* [n_cells] or NULL */, uint32_t n_fine_dofs,
                                uint32_t *out /* [n_cells * (pf+1)^dim] */);
/* ---- global-coarsening multigrid: the h-transfer between two ACTIVE meshes with hanging nodes at
 * one degree, the fine mesh's cells each a cell of the coarse mesh (child = 0) or child k of one (child = 1 + k, bit d of
 * k: the upper half in direction d) -- two members of deal.II's create_geometric_coarsening_sequence, what
 * MGTransferGlobalCoarsening transfers between.  Every level is a complete mesh served by an ordinary
 * mfgpu_handle: no refinement edges, no interface matrices, no copy pairs.  Both index lists are in the description's
 * form, hanging entries already substituted; parent [n_fine_cells] is the coarse cell's index.
 *   prolongation_1d     [(2p+1) * (p+1)] as for mfgpu_transfer_create (rows 0..p: the lower child, rows p..2p: the upper
 *                       one), or NULL
 *   coarse_mask         [n_coarse_cells], the coarse description's constraint_mask, or NULL (no hanging nodes there)
 *   fine_mask           [n_fine_cells], the fine description's, or NULL
 *   constraint_weights  [(p+1)^2] row-major, or NULL: those of FE_Q(p)
 * Section 19's semantics with two masks.  The owner of a fine dof is the first fine cell that lists it at a position its
 * FINE mask does not constrain (mfgpu_transfer_p_owner_list with the fine mask).  For the owner F with parent K
 *   (P x)[fine(F, i)] = [ E(child_F) C_p(coarse_mask_K) gather_K(x with the coarse Dirichlet dofs read as 0) ]_i
 * E the tensor product of the halves of prolongation_1d that `child` selects, the identity for child = 0 (such a cell
 * passes its values through bit for bit when its coarse mask is 0; it may carry a coarse mask it does not have in the
 * fine mesh, because its neighbour was coarsened).  prolongate stores (fine dofs no cell lists become 0), prolongate_add
 * read-modify-writes (and leaves them alone), neither with atomics; restrict_and_add is the exact transpose and adds with
 * floating-point atomics, skipping the coarse Dirichlet dofs.  All three only enqueue.  The object is an mfgpu_transfer:
 * memory_consumption, destroy and mfgpu_vcycle_create take it unchanged, and it mixes with the p-transfer in one V-cycle
 * (coarsened meshes at degree 1, then 1 -> 2 -> 4 on the active mesh).
 * MFGPU_EINVAL, nothing created: what mfgpu_transfer_create_p_hn refuses, where it applies; a parent out of range; a
 * child > 2^dim; a fine dof that is listed but owned by nobody.                                                      */
int mfgpu_transfer_create_h_hn(int dim, int degree, int number_type, uint32_t n_coarse_cells, uint32_t n_fine_cells,
                               const uint32_t *coarse_cell_dofs /* [n_coarse_cells * (p+1)^dim] */,
                               const uint32_t *fine_cell_dofs /* [n_fine_cells * (p+1)^dim] */,
                               const uint32_t *parent /* [n_fine_cells] */, const uint32_t *child /* [n_fine_cells] */,
                               uint32_t n_coarse_dofs, uint32_t n_fine_dofs, const uint32_t *coarse_dirichlet,
                               uint32_t n_coarse_dirichlet, const double *prolongation_1d /* [(2p+1) * (p+1)] or NULL */,
                               const uint32_t *coarse_mask /* [n_coarse_cells] or NULL */,
                               const uint32_t *fine_mask /* [n_fine_cells] or NULL */,
                               const double *constraint_weights /* [(p+1)^2] or NULL */, mfgpu_transfer **out);

/* Level operator with refinement edges (laplace_operator_gpu.h:154-186, 306-352): `desc` describes the level mesh with
 * the level's Dirichlet dofs as constrained_dofs (no hanging nodes on a level mesh, :174-176), edge_dofs are the level's
 * refinement-edge dofs (MGConstrainedDoFs::get_refinement_edge_indices).  mfgpu_level_operator is the level matrix
 * (constrained rows = Dirichlet + edge dofs: vmult, inverse diagonal ... through the ordinary calls; owned by the level);
 * the interface matrices are what deal.II's Multigrid::set_edge_matrices takes (poisson_mg.cu:367-375).               */
typedef struct mfgpu_level mfgpu_level;
int mfgpu_level_create(const mfgpu_desc *desc, const uint32_t *edge_dofs, uint32_t n_edge, mfgpu_level **out);
mfgpu_handle *mfgpu_level_operator(mfgpu_level *level);
/* Both interface products are asynchronous on `stream`: a copy or fill, index kernels and one mfgpu_vmult through two
 * temporaries of the level, all enqueued on `stream` as kernels and device-to-device copies (no memset nodes); no
 * allocation, no host synchronisation, so they can be captured in a graph.  One level is used on one stream at a time,
 * like a handle.                                                                                                    */
int mfgpu_level_vmult_interface_down(mfgpu_level *level, void *dst_dev, const void *src_dev, void *stream); /* :306-330 */
int mfgpu_level_vmult_interface_up(mfgpu_level *level, void *dst_dev, const void *src_dev, void *stream);   /* :332-352 */
/* mfgpu_update_coefficients for the level operator and the operator behind the interface matrices (both carry the
 * description's MFGPU_UPDATABLE_COEFFICIENTS); same arguments, same errors */
int mfgpu_level_update_coefficients(mfgpu_level *level, const void *coefficient_dev, const void *mass_coefficient_dev,
                                    void *stream);
void mfgpu_level_destroy(mfgpu_level *level);

/* copy_to_mg / copy_from_mg (mg_transfer_matrix_free_gpu.cu:690-760): dst[dst_idx[i]] = src[src_idx[i]] for the index
 * pairs of copy_indices (active dof <-> level dof), kept on the device                                              */
typedef struct mfgpu_index_pairs mfgpu_index_pairs;
int mfgpu_index_pairs_create(const uint32_t *dst_idx, const uint32_t *src_idx, uint32_t n, mfgpu_index_pairs **out);
int mfgpu_vec_copy_pairs(const mfgpu_index_pairs *p, void *dst_dev, const void *src_dev, int number_type, void *stream);
void mfgpu_index_pairs_destroy(mfgpu_index_pairs *p);

/* ---- mixed-precision multigrid: a float V-cycle under a double CG (the reference's level_number, bmop_mg.cu:58-59,
 * poisson_mg.cu:51; deal.II's copy_to_mg / copy_from_mg with OtherNumber), and the fused Chebyshev smoother updates.
 * All asynchronous on `stream`; MFGPU_EINVAL on a number type other than MFGPU_F64 / MFGPU_F32.                    */
/* dst[i] = (dst_type) src[i], i < n.  MFGPU_F64 -> MFGPU_F32 rounds to nearest even (overflow gives +-inf, as numpy's
 * astype(float32)); MFGPU_F32 -> MFGPU_F64 is exact; the same type is a copy.                                     */
int mfgpu_vec_convert(void *dst, int dst_type, const void *src, int src_type, size_t n, void *stream);
/* dst[dst_idx[i]] = (dst_type) src[src_idx[i]] over the pairs of mfgpu_index_pairs_create; other entries untouched */
int mfgpu_vec_copy_pairs_convert(const mfgpu_index_pairs *p, void *dst, int dst_type, const void *src, int src_type,
                                 void *stream);
/* One PreconditionChebyshev sweep in two kinds of launch instead of five BLAS-1 launches per inner step.  Device
 * vectors of n elements of number_type; x, upd and r are written and must not alias each other or an input
 * (MFGPU_EINVAL).
 *   start :  r = b - t (t == NULL: r = b);  upd = (f r) dinv;  x = upd if zero_start, else x += upd
 *   update:  r -= t;  upd = f1 upd + (f2 r) dinv;  x += upd
 * The scalars are rounded to number_type first, as GpuVector's calls round theirs.                                */
int mfgpu_vec_chebyshev_start(void *x, void *upd, void *r, const void *b, const void *t, const void *dinv, double f,
                              int zero_start, size_t n, int number_type, void *stream);
int mfgpu_vec_chebyshev_update(void *x, void *upd, void *r, const void *t, const void *dinv, double f1, double f2,
                               size_t n, int number_type, void *stream);
/* t = b - t (e == NULL) or t = b - (t + e): the residual of a V-cycle level after t = A x, with the edge rows e = down x.
 * One launch; the same numbers as mfgpu_vec_sadd(t, 1, 1, e) followed by mfgpu_vec_sadd(t, -1, 1, b).  16-byte accesses
 * when every pointer is 16-byte aligned.  MFGPU_EINVAL: the range of t overlaps that of b or e.                    */
int mfgpu_vec_residual(void *t, const void *b, const void *e, size_t n, int number_type, void *stream);

/* ---- device-resident conjugate gradients (no reference counterpart: the reference calls deal.II's
 * SolverCG, whose three scalar products per iteration each stop the host).  The algorithm is SolverCG::solve of
 * host/mfgpu_shim_poisson.h: zero start (x = 0, r = b), absolute tolerance tested against sqrt(r.r), 0 iterations when
 * |b| <= tolerance.  Every scalar (rz, pq, rr, alpha, beta, tolerance, iteration count, status) lives in a device state
 * block that the kernels read directly; the sums accumulate in double over a fixed grid in a fixed order; alpha and beta
 * are formed in double and rounded to the handle's number type before any element-wise use.
 * mfgpu_cg_begin and mfgpu_cg_iterate only enqueue work on `stream` (no allocation, no synchronisation, no host
 * read-back: they can be captured in a graph); mfgpu_cg_status is the only blocking call.
 * Freeze rule: the status leaves 0 when sqrt(r.r) <= tolerance (1), when the count reaches max_iterations (2) or when p.q
 * is not a positive finite number (3).  From then on every solver kernel returns without writing (the operator and the
 * preconditioner still run, on the unchanged p and r), so x, r, the count and the residual do not depend on how many
 * iterations were enqueued past the end, nor on check_every.
 * Like its handle, one mfgpu_cg is used on one stream at a time; x, b and inv_diag must stay valid and unchanged (x:
 * untouched by others) from mfgpu_cg_begin until the solve is over.                                                    */
#define MFGPU_CG_NONE 0       /* z = r */
#define MFGPU_CG_JACOBI 1     /* z = inv_diag .* r, fused, z never stored */
#define MFGPU_CG_CHEBYSHEV 2  /* z = p(A) r: the sweep PreconditionChebyshev::vmult runs with fused_updates, zero start,
                                 on inv_diag, with (degree, lambda_max, smoothing_range) given by the caller */
#define MFGPU_CG_CALLBACK 3   /* z = fn(ctx, z_dev, r_dev, stream): any preconditioner the caller can enqueue (a V-cycle) */

typedef struct mfgpu_cg mfgpu_cg;
typedef struct mfgpu_cg_info {
  uint32_t iterations;
  uint32_t status; /* 0 running 1 converged 2 max iterations 3 breakdown */
  double residual; /* sqrt(r.r) after `iterations` iterations */
  double initial_residual;
} mfgpu_cg_info;

/* All allocation happens here: the work vectors r, p, q (3 vectors of n_dofs numbers; MFGPU_CG_CALLBACK: + z = 4;
 * MFGPU_CG_CHEBYSHEV: + z and the sweep's three vectors = 7), 3 * 2048 doubles of partial sums, the 128-byte state block
 * -- mfgpu_cg_memory_consumption is exactly their sum -- and a pinned host mirror of the state block.  inv_diag_dev
 * (handle's number type, e.g. from mfgpu_compute_inverse_diagonal) is read by JACOBI and CHEBYSHEV and not copied; the
 * Chebyshev arguments are read by CHEBYSHEV only.  MFGPU_EINVAL, nothing created: null A / out, unknown preconditioner,
 * inv_diag_dev missing for JACOBI / CHEBYSHEV, CHEBYSHEV with degree 0, lambda_max <= 0 or smoothing_range <= 1.       */
int mfgpu_cg_create(mfgpu_handle *A, int preconditioner, const void *inv_diag_dev, uint32_t chebyshev_degree,
                    double lambda_max, double smoothing_range, mfgpu_cg **out);
/* MFGPU_CG_CALLBACK: fn enqueues z = M^-1 r on `stream` (and nothing that waits for the host, if the caller captures
 * graphs); a non-zero return ends mfgpu_cg_begin / mfgpu_cg_iterate with that code */
int mfgpu_cg_set_callback(mfgpu_cg *s, int (*fn)(void *ctx, void *z_dev, const void *r_dev, void *stream), void *ctx);
/* x = 0, r = b, z = M^-1 r, p = z; status 1 with 0 iterations if |b| <= tolerance.  MFGPU_EINVAL, nothing written: null
 * pointers, CALLBACK without a callback, x overlapping b.  16-byte accesses when x, b and inv_diag are 16-byte aligned. */
int mfgpu_cg_begin(mfgpu_cg *s, void *x_dev, const void *b_dev, double tolerance, uint32_t max_iterations, void *stream);
/* The same with tolerance = relative_tolerance * |b|, formed on the device: the first direction launch of the solve
 * writes it into the state block, so no norm visits the host (a solve inside a preconditioner, a captured graph).
 * |b| = 0 ends with status 1 and 0 iterations.  MFGPU_EINVAL also for a negative or non-finite relative tolerance.    */
int mfgpu_cg_begin_relative(mfgpu_cg *s, void *x_dev, const void *b_dev, double relative_tolerance,
                            uint32_t max_iterations, void *stream);
/* n_iterations more iterations (MFGPU_EINVAL before mfgpu_cg_begin): per iteration vmult, the partial sums of p.q, one
 * kernel for alpha, x += alpha p, r -= alpha q and the partial sums of r.r (NONE, JACOBI: and of r.z), the
 * preconditioner and the partial sums of r.z (CHEBYSHEV, CALLBACK), one kernel for count, status, beta, p = z + beta p */
int mfgpu_cg_iterate(mfgpu_cg *s, uint32_t n_iterations, void *stream);
/* one asynchronous copy of the state block into the pinned mirror and a stream synchronisation; at any point after
 * mfgpu_cg_begin (MFGPU_EINVAL before) */
int mfgpu_cg_status(mfgpu_cg *s, void *stream, mfgpu_cg_info *info);
/* begin; { iterate(check_every); status } until the status leaves 0.  check_every == 0: MFGPU_EINVAL */
int mfgpu_cg_solve(mfgpu_cg *s, void *x_dev, const void *b_dev, double tolerance, uint32_t max_iterations,
                   uint32_t check_every, void *stream, mfgpu_cg_info *info);
size_t mfgpu_cg_memory_consumption(const mfgpu_cg *s);
void mfgpu_cg_destroy(mfgpu_cg *s);
/* host only, no device: the scalars of the Chebyshev sweep, f[0] = 1/theta, then (f1, f2) per inner step k = 1..degree-1
 * (lambda_min = lambda_max / smoothing_range, theta and delta the centre and half width of [lambda_min, lambda_max],
 * sigma = theta / delta, rho_0 = 1 / sigma, rho_new = 1 / (2 sigma - rho), f1 = rho_new rho, f2 = 2 rho_new / delta).
 * MFGPU_EINVAL: null f, degree 0, lambda_max <= 0, smoothing_range <= 1.                                               */
int mfgpu_cg_chebyshev_scalars(uint32_t degree, double lambda_max, double smoothing_range, double *f /* [2*degree-1] */);

/* ---- the multigrid V-cycle as one object: deal.II's Multigrid::level_v_step + PreconditionMG with
 * PreconditionChebyshev smoothers (poisson_mg.cu:343-380), composed from the level operators, transfers and copy pairs
 * above, which it borrows: they must outlive it.  Schedule of one mfgpu_vcycle_apply: copy_to_mg; per level l > 0
 * pre-smoothing from zero, t = defect - A x - down x, restrict_and_add into level l - 1; the coarse solve on level 0; on
 * the way up x += P x_coarse, post-smoothing on defect - up x; copy_from_mg.  The smoother is the fused sweep of
 * mfgpu_vec_chebyshev_start / _update on the inverse diagonal of the level matrix.
 * mfgpu_vcycle_create is the set-up call: it may block and allocates everything -- per level l > 0 the vectors defect,
 * solution, t, r, upd and the inverse diagonal (6 vectors of n_dofs(l) level numbers) and one more (edge) where the
 * level has edges; on level 0, which has no smoother, defect and solution plus the coarse solver's data: DENSE the
 * inverse in double, n0 rows of n0 rounded up to an even number of doubles; CG an internal mfgpu_cg
 * (mfgpu_cg_memory_consumption).  mfgpu_vcycle_memory_consumption is exactly that sum.  (An estimate of level 0's
 * lambda_max, made only when lambda_max == NULL, goes through an inverse diagonal that is freed again inside create.)
 * mfgpu_vcycle_apply allocates nothing, synchronises nothing and reads nothing back: kernels and device-to-device copies
 * on `stream` only, no memset nodes; it can be captured in a graph.  One object is used on one stream at a time.
 * After mfgpu_level_update_coefficients the inverse diagonals, eigenvalue estimates and the dense inverse are stale:
 * mfgpu_vcycle_refresh (below) recomputes them in place on the caller's stream, without stopping the host.             */
#define MFGPU_VCYCLE_COARSE_AUTO 0  /* DENSE when n_dofs(0) <= MFGPU_VCYCLE_DENSE_MAX, else CG */
#define MFGPU_VCYCLE_COARSE_DENSE 1 /* x = A0^-1 b with the inverse formed at creation (host Cholesky in double): one launch */
#define MFGPU_VCYCLE_COARSE_CG 2    /* unpreconditioned device CG, coarse_max_iterations iterations enqueued per apply.
                                       Cost: EVERY apply enqueues all of them -- one vmult and three solver launches
                                       each -- whether or not the solve has frozen before; the frozen ones run and write
                                       nothing.  With the default n_dofs(0) that is thousands of launches per V-cycle
                                       where AUTO picks this mode (above the dense cap): set coarse_max_iterations to
                                       what the level-0 problem needs (DESIGN.md section 16 has a measured case)   */
#define MFGPU_VCYCLE_DENSE_MAX 2048 /* 32 MB of inverse */

typedef struct mfgpu_vcycle mfgpu_vcycle;
typedef struct mfgpu_vcycle_level_desc {
  mfgpu_handle *op;                 /* level matrix, borrowed (mfgpu_level_operator(edges) or an mfgpu_create handle) */
  mfgpu_level *edges;               /* NULL: no refinement edges on this level; else op == mfgpu_level_operator(edges) */
  mfgpu_transfer *from_coarser;     /* level-1 -> level; NULL on level 0 only */
  const mfgpu_index_pairs *to_mg;   /* level <- active; NULL on EVERY level = globally refined: the active vector IS */
  const mfgpu_index_pairs *from_mg; /* active <- level;   the finest level's vector (n_active == n_dofs(top))         */
} mfgpu_vcycle_level_desc;
typedef struct mfgpu_vcycle_desc {
  uint32_t n_levels;
  const mfgpu_vcycle_level_desc *levels;
  int32_t active_type;            /* type and length of z and r of mfgpu_vcycle_apply; the type may differ from the    */
  uint32_t n_active;              /* levels' (a float V-cycle under a double CG: converted in the copies)              */
  uint32_t smoother_degree;       /* 0 = 5  */
  double smoothing_range;         /* 0 = 15 */
  uint32_t eig_iterations;        /* 0 = 15: minimum number of power-iteration steps */
  const double *lambda_max;       /* [n_levels] or NULL = estimate (level 0's entry is not used by the coarse solvers) */
  uint32_t coarse;                /* MFGPU_VCYCLE_COARSE_* */
  double coarse_tolerance;        /* CG: relative, 0 = max(1e-10, 100 eps of the level type) */
  uint32_t coarse_max_iterations; /* CG: 0 = n_dofs(0) */
} mfgpu_vcycle_desc;
/* MFGPU_EINVAL, nothing created: null pointers, n_levels == 0, a level without op, a missing transfer above level 0 or one
 * whose sizes or type are not the two levels'; edges with an op that is not that level's operator; levels of different
 * number types; pairs on some levels and not on others (or only one of to_mg / from_mg); no pairs and n_active !=
 * n_dofs(top); a smoothing range <= 1 or a lambda_max <= 0 on a level above 0; an unknown coarse mode; DENSE above
 * MFGPU_VCYCLE_DENSE_MAX; a level-0 matrix that is not positive definite (the V-cycle is an SPD preconditioner by
 * contract; a mass term with c < 0 is the caller's business).                                                       */
int mfgpu_vcycle_create(const mfgpu_vcycle_desc *d, mfgpu_vcycle **out);
int mfgpu_vcycle_apply(mfgpu_vcycle *v, void *z_dev, const void *r_dev, void *stream); /* z = M^-1 r */
/* the smoothers' lambda_max (given or estimated; with an estimate, level 0's too) */
int mfgpu_vcycle_lambda_max(const mfgpu_vcycle *v, double *lambda /* [n_levels] */);
size_t mfgpu_vcycle_memory_consumption(const mfgpu_vcycle *v);
void mfgpu_vcycle_destroy(mfgpu_vcycle *v);
/* MFGPU_CG_CALLBACK solvers: the library's own callback, z = M^-1 r = mfgpu_vcycle_apply(v, z, r, stream).  MFGPU_EINVAL:
 * not a CALLBACK solver, or the V-cycle's active type / length are not the solver's.  v must outlive the solves.      */
int mfgpu_cg_set_vcycle(mfgpu_cg *s, mfgpu_vcycle *v);
/* PreconditionChebyshev's eigenvalue estimate (host/mfgpu_shim_mg.h): power iteration on D^-1 A from the start vector
 * sin(0.7 i) + 0.3, at least max(5, min_iterations) steps, on until the estimate moves by <= 1 % per step, at most 200;
 * *lambda_max = 1.2 x the estimate.  inv_diag_dev: the operator's number type.  A blocking set-up call (two norms per
 * step are read back; two work vectors are allocated and freed).                                                    */
int mfgpu_estimate_lambda_max(mfgpu_handle *op, const void *inv_diag_dev, uint32_t min_iterations, double *lambda_max);
/* the same call, which also reports how many steps the iteration took (what mfgpu_vcycle_refresh enqueues by default) */
int mfgpu_estimate_lambda_max_steps(mfgpu_handle *op, const void *inv_diag_dev, uint32_t min_iterations, double *lambda_max,
                                    uint32_t *steps);
/* host only, no device: inv = a^-1 for a symmetric positive definite a [n * n] (row-major; only the lower triangle is
 * read) by a Cholesky factorisation in double.  MFGPU_EINVAL on a non-positive (or non-finite) pivot; inv may not alias a. */
int mfgpu_spd_inverse(uint32_t n, const double *a, double *inv);

/* ---- refreshing a V-cycle after a coefficient update.  The three set-up pieces above as calls that
 * only enqueue on `stream` -- no allocation, no synchronisation, nothing read back, capturable in a graph -- and
 * mfgpu_vcycle_refresh, which runs them on an existing object.                                                         */
/* mfgpu_vec_chebyshev_start / _update with the scalars in device memory: f_dev[0] = f, f12_dev[0..1] = f1, f2, doubles,
 * read by the kernel when the stream gets there and rounded to number_type as the by-value forms round theirs, so the
 * two forms give equal bits on equal scalars.  Aliasing rules and errors as the by-value forms; MFGPU_EINVAL also for a
 * null scalar pointer or one that is not 8-byte aligned.                                                             */
int mfgpu_vec_chebyshev_start_dev(void *x, void *upd, void *r, const void *b, const void *t, const void *dinv,
                                  const double *f_dev, int zero_start, size_t n, int number_type, void *stream);
int mfgpu_vec_chebyshev_update_dev(void *x, void *upd, void *r, const void *t, const void *dinv,
                                   const double *f12_dev /* f1, f2 */, size_t n, int number_type, void *stream);
/* mfgpu_cg_chebyshev_scalars on a lambda_max in device memory: one small launch, the same recurrence in double, f_dev
 * [2 * degree - 1].  MFGPU_EINVAL: null pointers, degree 0, smoothing_range <= 1 (lambda_max cannot be checked: a value
 * <= 0 gives the non-finite scalars the formulas give).                                                              */
int mfgpu_cg_chebyshev_scalars_dev(uint32_t degree, const double *lambda_max_dev, double smoothing_range,
                                   double *f_dev /* [2*degree-1] */, void *stream);
/* The power iteration of mfgpu_estimate_lambda_max without the host: the start vector is written by a kernel, then
 * n_steps steps are enqueued, each one mfgpu_vmult and two launches (w = inv_diag .* w with the partial sums of w.w and
 * v.v; estimate = |w| / |v| and v = w / |w|).  The host's stopping rule is a freeze rule: after at least
 * max(5, min_iterations) steps, once the estimate moved by at most 1 % in the last step, status = 1 and the solver
 * kernels of the later steps return without writing (the operator applies still run).  status 2: n_steps used up,
 * lambda_max = 1.2 x the last estimate; status 3: a norm was not a positive finite number, lambda_max is not written; 0
 * while running.  lambda_max = 1.2 x estimate for status 1 and 2; steps = the steps that counted.
 * The workspace (16-byte aligned, MFGPU_EINVAL otherwise) is, in this order: the 64-byte state block, which starts with
 * an mfgpu_eig_result the caller copies out when it wants it; 2 * 2048 doubles of partial sums; the two work vectors,
 * each n_dofs numbers of number_type rounded up to a multiple of 16 bytes:
 *   mfgpu_eig_workspace_bytes = 64 + 32768 + 2 * round16(n_dofs * sizeof(number))       (0 for an unknown number type)
 * MFGPU_EINVAL, nothing enqueued: null pointers, n_steps == 0, an operator without dofs.                              */
typedef struct mfgpu_eig_result {
  double lambda_max, estimate;
  uint32_t steps, status;
} mfgpu_eig_result;
size_t mfgpu_eig_workspace_bytes(uint32_t n_dofs, int number_type); /* host only */
int mfgpu_estimate_lambda_max_enqueue(mfgpu_handle *op, const void *inv_diag_dev, uint32_t min_iterations, uint32_t n_steps,
                                      void *workspace_dev, void *stream);
/* mfgpu_spd_inverse on the device, in double: Cholesky of the lower triangle of a_dev (n rows of lda doubles; only the
 * lower triangle is read), L^-1, inv = L^-T L^-1 into inv_dev, n rows of ld doubles; the columns n .. ld - 1 of every row
 * get zeros (with ld = n rounded up to even that is the layout of the V-cycle's dense coarse solve).  Three launches:
 * one workgroup factorises (the matrix stays in global memory, i.e. in L2), one wave per column inverts L, one workgroup
 * per row forms the product; no atomics, two calls give equal bits.  A pivot that is not a positive finite number sets
 * *status_dev = 1 and the two later kernels return without writing, so inv_dev keeps its contents; otherwise *status_dev
 * = 0.  Workspace: mfgpu_spd_inverse_workspace_bytes = 2 * n * n * 8 (L and L^-1), 8-byte aligned.
 * MFGPU_EINVAL, nothing enqueued: n == 0 or n > MFGPU_SPD_INVERSE_DEVICE_MAX (the factorisation keeps a column in
 * LDS), null pointers, lda or ld < n, misaligned or overlapping a, inv and workspace.                                */
#define MFGPU_SPD_INVERSE_DEVICE_MAX 512
size_t mfgpu_spd_inverse_workspace_bytes(uint32_t n); /* host only */
int mfgpu_spd_inverse_enqueue(uint32_t n, const double *a_dev, uint32_t lda, double *inv_dev, uint32_t ld,
                              void *workspace_dev, uint32_t *status_dev, void *stream);
/* Recompute, from whatever the level operators hold now, (a) the inverse diagonal of every level above 0, (b) where the
 * object estimated its own lambda_max at creation (desc.lambda_max == NULL) the estimate of every level above 0 by
 * mfgpu_estimate_lambda_max_enqueue with the object's eig_iterations, and from it the smoother's Chebyshev scalars by
 * mfgpu_cg_chebyshev_scalars_dev -- eig_steps steps are enqueued per level, 0 = as many as that level's estimate took at
 * creation; with a lambda_max given at creation the values and the scalars stay -- and (c) in COARSE_DENSE mode the
 * inverse: the level-0 operator applied to the unit vectors, converted to double and symmetrised from the lower triangle
 * as at creation, then mfgpu_spd_inverse_enqueue into the object's inverse.  COARSE_CG has nothing to refresh.  Level
 * 0's lambda_max, which no coarse solver reads, keeps its creation value.  Legal on levels created without
 * MFGPU_UPDATABLE_COEFFICIENTS (it recomputes the same values).
 * Everything is enqueued on `stream`; nothing is read back.  The FIRST refresh of an object allocates, once and
 * together, what refreshes need beyond the level vectors (t, r and upd are scratch between applies and serve as work
 * vectors) -- the only allocation and the only possible host synchronisation of the function:
 *   16                                           the coarse status word
 *   + (n_levels - 1) * (64 + round16(8 * (2 * smoother_degree - 1)))    per level above 0: state block, scalar table
 *   + 32768                                      partial sums, only with desc.lambda_max == NULL
 *   + 2 * round16(n0 * n0 * sizeof(level number)) + round16(8 * n0 * n0) + round16(16 * n0 * n0)
 *                                                only COARSE_DENSE: identity block, A0 in the level type, A0 in
 *                                                double, the workspace of mfgpu_spd_inverse_enqueue; n0 = n_dofs(0)
 * (round16 = up to a multiple of 16).  mfgpu_vcycle_memory_consumption grows by exactly that from then on and
 * mfgpu_vcycle_destroy frees it.  Until the first refresh mfgpu_vcycle_apply and mfgpu_vcycle_memory_consumption are
 * unchanged; from the first refresh on the smoother reads its scalars from the device table (the _dev forms above), so
 * a graph captured AFTER the first refresh -- of apply alone or of "update coefficients, refresh, apply" -- stays valid
 * across later refreshes.  Capture after the first refresh, and with the same eig_steps if the refresh is inside.
 * MFGPU_EINVAL: null object.  MFGPU_EUNSUPPORTED, nothing enqueued or allocated: COARSE_DENSE with n_dofs(0) >
 * MFGPU_SPD_INVERSE_DEVICE_MAX (re-create the object, or use the CG coarse mode).
 * A level-0 matrix that is no longer positive definite cannot be an error code of a call that only enqueues: the old
 * inverse stays and mfgpu_vcycle_refresh_status reports coarse_status = 1.                                           */
int mfgpu_vcycle_refresh(mfgpu_vcycle *v, uint32_t eig_steps, void *stream);
typedef struct mfgpu_vcycle_refresh_info {
  uint32_t coarse_status;  /* 0, or 1: the level-0 matrix was not positive definite, the inverse is the old one */
  uint32_t eig_status_max; /* the largest status of the estimates (mfgpu_eig_result; 0 with a given lambda_max) */
  uint32_t eig_steps_max;  /* the largest step count of the estimates */
  uint32_t reserved;
} mfgpu_vcycle_refresh_info;
/* blocking: copies the result blocks of the last refresh back (one copy and a synchronisation of `stream`) and updates
 * what mfgpu_vcycle_lambda_max reports; before this call it reports the previous values.  MFGPU_EINVAL: null pointers,
 * or no refresh yet.                                                                                                 */
int mfgpu_vcycle_refresh_status(mfgpu_vcycle *v, void *stream, mfgpu_vcycle_refresh_info *info);

/* ---- cell integrals of a Poisson solve (poisson.cu:152-229, 277-292) ------------------------------------------
 * A separate object created from the same description as the operator; it keeps its own device copy of the geometry
 * (loc2glob, constraint mask, quadrature points, JxW, the folded coefficient) and leaves mfgpu_handle untouched.
 * MFGPU_F64 only (MFGPU_F32: MFGPU_EUNSUPPORTED; the reference's poisson uses double); every (dim, degree) of
 * mfgpu_create, uniform-J0 and general geometry, with and without hanging nodes.  quadrature_points are required
 * (MFGPU_EINVAL without).  Geometry at the QGauss(p+2) error points is interpolated from the QGauss(p+1) quadrature
 * points with the 1D Lagrange basis on those points: exact for mappings of degree <= p per direction (affine cells and
 * MappingQ1, i.e. every mesh stand-in below), not for higher-order mappings.  No floating-point atomics: two calls on
 * the same inputs give bitwise-equal results.  All vectors are device vectors of doubles.                          */
typedef struct mfgpu_integrator mfgpu_integrator;
int mfgpu_integrator_create(const mfgpu_desc *desc, mfgpu_integrator **out);
/* poisson.cu:182-221: rhs_i = sum_cells int phi_i f - int grad phi_i . a grad u_b on the description's quadrature
 * points, distributed like a cell result (transposed hanging-node resolution), constrained rows 0, every entry written.
 * f_qp: [n_cells * (p+1)^dim] values at the quadrature points, or NULL = RightHandSide<dim> (poisson_common.h:277-296,
 * which assumes the built-in coefficient).  u_b: read on every dof a cell references, constrained dofs included (unlike
 * vmult), hanging-node interpolated as in the cell loop; NULL = no lift.  a = the description's coefficient or the
 * built-in one, as mfgpu_create.  With mass_coefficient the lift is - int a grad phi_i . grad u_b - int c phi_i u_b;
 * f_qp = NULL still means the built-in Poisson load, so a caller with a mass term normally passes f_qp.  Asynchronous. */
int mfgpu_integrator_rhs(mfgpu_integrator *it, void *rhs, const void *f_qp, const void *u_b, void *stream);
/* VectorTools::integrate_difference(..., QGauss(p+2), L2_norm), poisson.cu:277-292.  u in the operator's numbering;
 * entries of hanging dofs are not read (values come through loc2glob + hanging-node interpolation).  exact:
 * [n_cells * (p+2)^dim] values at the error points, or NULL = Solution<dim> (poisson_common.cc:5-175).  per_cell:
 * [n_cells] squared cell errors, or NULL.  *l2 = sqrt(sum of the squared cell errors), fixed-order sum; blocks.     */
int mfgpu_integrator_l2_error(mfgpu_integrator *it, const void *u, const void *exact, void *per_cell, void *stream,
                              double *l2);
/* the (p+2)^dim error points of every cell, [n_cells * (p+2)^dim * dim] (x, y, z per point, x fastest), so that a
 * caller can supply `exact`.  Asynchronous.                                                                       */
int mfgpu_integrator_error_points(mfgpu_integrator *it, void *points, void *stream);
/* The same for the Dirichlet lift of mfgpu_integrator_rhs: a and c of an integrator created with
 * MFGPU_UPDATABLE_COEFFICIENTS (it then keeps inv_jac on the device; JxW is resident anyway).  Double device arrays;
 * arguments, execution rules and errors as mfgpu_update_coefficients.                                                */
int mfgpu_integrator_update_coefficients(mfgpu_integrator *it, const void *coefficient_dev,
                                         const void *mass_coefficient_dev, void *stream);
/* The finite element field at the description's quadrature points -- the read_dof_values + evaluate + get_value /
 * get_gradient half of FEEvaluationGpu (fee_gpu.cuh), which the reference only uses inside its cell loop.  u: device
 * vector [n_dofs], read on every dof a cell references, constrained dofs included, hanging-node interpolated as in
 * mfgpu_integrator_rhs.  values_qp: [n_cells * (p+1)^dim]; gradients_qp: [n_cells * (p+1)^dim * dim], real-space
 * gradients (J^-T applied), x, y, z per point; cell-major in the description's cell order, points x fastest.  Either
 * output may be NULL (both: MFGPU_EINVAL).  Gradients need inv_jac on the device: gradients_qp != NULL on an
 * integrator created without MFGPU_UPDATABLE_COEFFICIENTS is MFGPU_EINVAL; values work on every integrator.  One
 * wave per cell, no atomics: two calls give bitwise-equal results.  Asynchronous.  With this and the BLAS-1 calls a
 * coefficient a(u) is formed on the device and handed to the update calls (host/nonlinear.cc).                       */
int mfgpu_integrator_evaluate(mfgpu_integrator *it, const void *u, void *values_qp, void *gradients_qp, void *stream);
/* Cell-based gradient-recovery error indicator (Zienkiewicz-Zhu style): per_cell [n_cells] =
 * eta_K^2 of the field u [n_dofs].  Device doubles.  weight_qp: [n_cells * (p+1)^dim] at the quadrature points, or NULL
 * for 1 (pass the coefficient for the energy norm).  With N = p+1, ND = N^dim:
 *  a. Cell gradient at the nodes.  u is gathered through loc2glob with hanging-node interpolation and its real-space
 *     gradient grad u_h is formed at the cell's ND quadrature points, both exactly as mfgpu_integrator_evaluate does.
 *     Per component, g_K [ND] are the nodal coefficients of the Q_p polynomial that takes those ND values at the
 *     quadrature points: g_K = (T x T (x T)) values, T [i][q] the inverse of the square 1D table [q][i] = phi_i(x_q)
 *     (= shape_values transposed), x fastest.
 *  b. Nodal average.  |K| = sum_q JxW_q.  A local position is constrained when it lies on a constrained face or, in 3D,
 *     a constrained edge of the cell -- the pencils the hanging-node resolution rewrites: with the mask bits of
 *     hanging_nodes.cuh:38-50, face d (bit 3+d) at index 0 of direction d if type bit d is set, else p; the edge along
 *     e (bits 7, 8, 6 for e = x, y, z) at those indices of both other directions.  Every position i that is not
 *     constrained adds |K| g_K,i (per component) to the numerator and |K| to the denominator of the dof
 *     loc2glob[K][i], Dirichlet dofs included, summed per dof in ascending (cell, local index) order.
 *     G_dof = numerator / denominator; a dof without contribution (a hanging dof) gets 0 and is never read.
 *  c. eta_K^2 = sum_q weight_q |G(x_q) - grad u_h(x_q)|^2 JxW_q, with G read through loc2glob with hanging-node
 *     interpolation, component by component, and evaluated at the quadrature points with phi_i(x_q).
 * Needs inv_jac on the device: MFGPU_EINVAL on an integrator created without MFGPU_UPDATABLE_COEFFICIENTS, and on NULL
 * u or per_cell.  The index list and the denominator of step b are built at creation; the double scratch (dim local
 * buffers [n_cells * ND], dim nodal vectors [n_dofs]) is allocated by the first call and kept, so call once before
 * capturing the call in a graph.  Three launches (a, b, c), one wave per cell in a and c, no atomics: two calls give
 * bitwise-equal results.  Asynchronous: enqueues on `stream` and reads nothing back.                                 */
int mfgpu_integrator_recovery_indicator(mfgpu_integrator *it, const void *u, const void *weight_qp, void *per_cell,
                                        void *stream);
/* The transpose of mfgpu_integrator_evaluate -- the submit_value / submit_gradient / integrate /
 * distribute_local_to_global half of FEEvaluationGpu (fee_gpu.cuh) for point data the caller formed:
 *   dst_i = sum_cells sum_q JxW_q [ phi_i(x_q) v_q + grad_x phi_i(x_q) . g_q ]
 * values_qp: v [n_cells * (p+1)^dim]; gradients_qp: g [n_cells * (p+1)^dim * dim], real-space vectors (x, y, z per
 * point; the kernel applies J^-1 per point, or J0^-1, before the reference-gradient contraction); both in the layout
 * mfgpu_integrator_evaluate writes.  Either may be NULL (both: MFGPU_EINVAL).  gradients_qp != NULL on an integrator
 * created without MFGPU_UPDATABLE_COEFFICIENTS is MFGPU_EINVAL (inv_jac is needed on the device), as for evaluate.
 * Distributed like a cell result (transposed hanging-node resolution) through the CSR gather of mfgpu_integrator_rhs:
 * constrained rows 0, every entry of dst written, no atomics (two calls give bitwise-equal results).  It uses the
 * integrator's per-cell scratch, as mfgpu_integrator_rhs and every mfgpu_qop of the integrator do: calls that share
 * an integrator must be ordered (one stream, or events).  Asynchronous.                                            */
int mfgpu_integrator_integrate(mfgpu_integrator *it, void *dst, const void *values_qp, const void *gradients_qp,
                               void *stream);
void mfgpu_integrator_destroy(mfgpu_integrator *it);

/* ---- the general linear second-order operator on quadrature-point coefficients (no reference counterpart; deal.II: a
 * user LocOp over FEEvaluation) -------------------------------------------------------------
 * Free rows:
 *   (A u)_i = sum_cells sum_q JxW_q [ grad phi_i . (D_q grad u_q + gamma_q u_q) + phi_i (beta_q . grad u_q + c_q u_q) ]
 * constrained rows are identity rows (dst_c = src_c) and constrained entries of src are read as 0, both as mfgpu_vmult,
 * so mfgpu_vec_* solvers written for the operator work unchanged; a dof no cell references gets 0.  One cell kernel
 * (one wave per cell, evaluate -> point-wise terms -> integrate in LDS) plus the integrator's per-dof gather; no
 * atomics, bitwise repeatable, enqueue only.  MFGPU_F64 only, as the integrator.
 *
 * The object is created from an integrator, BORROWS its geometry, gather lists and per-cell scratch, and must be
 * destroyed before it; calls on one integrator and its operators must be ordered (see mfgpu_integrator_integrate).
 * terms: a non-empty set of the bits below; both diffusion bits, or an unknown bit: MFGPU_EINVAL.  Every term but
 * MFGPU_QOP_REACTION needs an integrator created with MFGPU_UPDATABLE_COEFFICIENTS (else MFGPU_EINVAL).
 *
 * mfgpu_qop_set_coefficients FOLDS the caller's real-space device arrays (doubles, cell-major in the description's cell
 * order, points x fastest, vectors (x, y, z) and matrices row-major per point) into reference form:
 *   JxW J^-1 D J^-T (dim^2 values per point; scalar D = a I on MFGPU_UNIFORM_J0: the one value a J0^2 JxW),
 *   JxW J^-1 gamma, JxW J^-1 beta (dim values each), JxW c (one value),
 * so mfgpu_qop_vmult reads neither inv_jac nor JxW.  A pointer for a term in `terms` replaces that term, NULL keeps its
 * last values; a pointer for a term not in `terms`, or NULL everywhere, is MFGPU_EINVAL.  It only enqueues (the arrays
 * may be reused after the stream passes the call), reads nothing back and allocates nothing.  mfgpu_qop_vmult and
 * mfgpu_qop_compute_inverse_diagonal before every term has been set once: MFGPU_EINVAL.
 *
 * Only the terms in `terms` get storage; mfgpu_qop_memory_consumption returns exactly the folded bytes.  Per point:
 *   MFGPU_QOP_DIFFUSION_SCALAR  8 (MFGPU_UNIFORM_J0)  or 8 dim^2 (general geometry)
 *   MFGPU_QOP_DIFFUSION_TENSOR  8 dim^2
 *   MFGPU_QOP_CONVECTION        8 dim
 *   MFGPU_QOP_FLUX              8 dim
 *   MFGPU_QOP_REACTION          8
 * e.g. all five terms in 3D: 8 (9 + 3 + 3 + 1) = 128; scalar diffusion + reaction on a uniform-J0 mesh: 16.
 *
 * mfgpu_qop_vmult flags: 0, or MFGPU_QOP_TRANSPOSE for A^T (D -> D^T, beta <-> gamma on the folded arrays).  src is
 * never written; dst may be src (in place: the cell kernel has read src into the per-cell scratch before the gather
 * writes dst, and an identity row reads its entry before it writes it).
 * mfgpu_qop_compute_inverse_diagonal: inv_diag_i = 1 / A_ii of the operator above with the hanging-node constraints
 * applied (the cell operator on local unit vectors, both resolutions); 1 on constrained and unreferenced dofs.  Set-up
 * work: (p+1)^dim cell applies per cell.                                                                             */
typedef struct mfgpu_qop mfgpu_qop;
#define MFGPU_QOP_DIFFUSION_SCALAR (1u << 0) /* D = a I,   a [n_cells*ND]                    */
#define MFGPU_QOP_DIFFUSION_TENSOR (1u << 1) /* D [n_cells*ND*dim*dim] row-major, any matrix */
#define MFGPU_QOP_CONVECTION       (1u << 2) /* beta  [n_cells*ND*dim]                       */
#define MFGPU_QOP_FLUX             (1u << 3) /* gamma [n_cells*ND*dim]                       */
#define MFGPU_QOP_REACTION         (1u << 4) /* c [n_cells*ND]                               */
#define MFGPU_QOP_TRANSPOSE        (1u << 0) /* vmult flag: apply A^T (D -> D^T, beta <-> gamma) */
typedef struct mfgpu_qop_coefficients {
  const void *diffusion, *convection, *flux, *reaction; /* device arrays */
} mfgpu_qop_coefficients;
int mfgpu_qop_create(mfgpu_integrator *it, uint32_t terms, mfgpu_qop **out);
int mfgpu_qop_set_coefficients(mfgpu_qop *q, const mfgpu_qop_coefficients *c, void *stream);
int mfgpu_qop_vmult(mfgpu_qop *q, void *dst, const void *src, uint32_t flags, void *stream);
int mfgpu_qop_compute_inverse_diagonal(mfgpu_qop *q, void *inv_diag, void *stream);
size_t mfgpu_qop_memory_consumption(const mfgpu_qop *q);
void mfgpu_qop_destroy(mfgpu_qop *q);

/* ---- the vector-valued quadrature-point operator: linear elasticity (no reference counterpart; deal.II: a user LocOp
 * over FEEvaluation<dim, p, p+1, dim>) ---------------------------------------------------------
 * A field has dim components on the description's scalar FE_Q(p) space, stored in BLOCKS: u[a * n_dofs + i] is component
 * a at scalar dof i, length dim * n_dofs.  Every component uses the integrator's loc2glob, constraint masks and gather
 * lists; a component is a plain scalar vector for mfgpu_integrator_evaluate / _integrate, mfgpu_points_* and the
 * transfers, and the whole vector one for mfgpu_vec_* and mfgpu_bicgstab.  Free rows, with sigma the point-wise stress:
 *   (A u)_(a,i) = sum_cells sum_q JxW_q [ sum_k d_k phi_i(x_q) sigma_ak(x_q) + phi_i(x_q) rho_q u_a(x_q) ]
 *   MFGPU_VQOP_ISOTROPIC  sigma = lambda_q (div u) I + mu_q (grad u + grad u^T)
 *   MFGPU_VQOP_TENSOR4    sigma_ak = sum_bl C_q[a][k][b][l] d_l u_b   (any tensor: no symmetry is assumed)
 *   MFGPU_VQOP_MASS       the rho term
 * Constrained rows are identity rows, constrained entries of src are read as 0 (the rules of mfgpu_vmult and
 * mfgpu_qop_vmult); a dof no cell references gets 0.  MFGPU_F64 only, dim 2 and 3, degree 1..6, uniform-J0 and general
 * geometry; with hanging nodes the cell's mask applies to every component.
 *
 * mfgpu_vqop_create BORROWS the integrator as mfgpu_qop_create does (destroy the operator first; calls that share an
 * integrator must be ordered).  terms: a non-empty set of the three bits; both stress bits, or an unknown bit:
 * MFGPU_EINVAL.  ISOTROPIC and TENSOR4 need an integrator created with MFGPU_UPDATABLE_COEFFICIENTS (else MFGPU_EINVAL);
 * a MASS-only operator works on any integrator.
 * constrained: an ascending list of n_constrained indices in the block numbering [0, dim * n_dofs), copied; NULL: the
 * description's constrained_dofs in every component.  Not strictly ascending, or an index out of range: MFGPU_EINVAL.
 * A caller's own list fixes single components on a face (sliding and symmetry boundaries).  It must contain, in every
 * component, each hanging dof and every other dof of the description's constrained_dofs (MFGPU_EINVAL otherwise): the
 * integrator's gather lists leave those rows empty.  For boundary dofs that are free in some component, create the
 * integrator from a description whose constrained_dofs holds the hanging dofs alone.
 *
 * mfgpu_vqop_set_coefficients folds the caller's real-space device arrays once per update (enqueue only, no allocation,
 * no read-back), cell-major, points x fastest; per point lambda, mu, mass: one double; tensor: dim^4 doubles row-major
 * (a, k, b, l).  NULL keeps a term's last values.  lambda without mu or mu without lambda, a pointer for a term not in
 * `terms`, or NULL everywhere: MFGPU_EINVAL.  vmult / the diagonal before every term has been set once: MFGPU_EINVAL.
 * Folded forms ([cell][component][q]) and bytes per point -- mfgpu_vqop_memory_consumption returns exactly their sum
 * over the points plus the dim * n_dofs bytes of the operator's own constraint flags:
 *   MFGPU_VQOP_TENSOR4    JxW sum_kl J^-1[e][k] C[a][k][b][l] J^-1[f][l]        8 dim^4  (128 in 2D, 648 in 3D)
 *   MFGPU_VQOP_ISOTROPIC  uniform-J0: lambda J0^2 JxW, mu J0^2 JxW              16
 *                         general: lambda JxW, mu JxW; the apply reads the      16  (+ the integrator's 8 dim^2 inv_jac,
 *                         integrator's inv_jac: grad_x u_b = J^-T grad_xi u_b,       read, not stored again)
 *                         sigma, then the reference flux J^-1 sigma_a
 *   MFGPU_VQOP_MASS       JxW rho                                               8
 *
 * mfgpu_vqop_vmult: one cell kernel (one wave per cell: gather dim components, hanging-node resolution, dim^2 reference
 * gradients, the law in place, integration per component, transposed resolution, dim local vectors -- the integrator's
 * scratch plus dim - 1 copies of its size that the operator owns) and one gather launch for all components, which
 * writes the identity rows.  No atomics, bitwise repeatable, every entry of dst written, src never written, dst may be
 * src.  mfgpu_vqop_compute_inverse_diagonal: 1 / A_jj with the hanging-node constraints applied (cell applies on local
 * unit vectors), 1 on constrained and unreferenced entries.  mfgpu_vqop_set_constrained_values: vec[j] = value on the
 * operator's constrained list (makes a right-hand side built per component by mfgpu_integrator_integrate consistent
 * with a per-component list).  All three only enqueue.                                                              */
typedef struct mfgpu_vqop mfgpu_vqop;
#define MFGPU_VQOP_ISOTROPIC (1u << 0) /* lambda, mu [n_cells*ND] each                          */
#define MFGPU_VQOP_TENSOR4   (1u << 1) /* C [n_cells*ND*dim^4], row-major (a,k,b,l), any tensor */
#define MFGPU_VQOP_MASS      (1u << 2) /* rho [n_cells*ND]                                      */
typedef struct mfgpu_vqop_coefficients {
  const void *lambda, *mu, *tensor, *mass; /* device arrays */
} mfgpu_vqop_coefficients;
int mfgpu_vqop_create(mfgpu_integrator *it, uint32_t terms, const uint32_t *constrained, size_t n_constrained,
                      mfgpu_vqop **out);
int mfgpu_vqop_set_coefficients(mfgpu_vqop *q, const mfgpu_vqop_coefficients *c, void *stream);
int mfgpu_vqop_vmult(mfgpu_vqop *q, void *dst, const void *src, void *stream);
int mfgpu_vqop_compute_inverse_diagonal(mfgpu_vqop *q, void *inv_diag, void *stream);
int mfgpu_vqop_set_constrained_values(mfgpu_vqop *q, void *vec, double value, void *stream);
size_t mfgpu_vqop_memory_consumption(const mfgpu_vqop *q);
void mfgpu_vqop_destroy(mfgpu_vqop *q);

/* ---- device-resident BiCGStab (no reference counterpart): the solver for the non-symmetric
 * operators above, in the style of mfgpu_cg.  The algorithm is SolverBicgstab::solve of host/mfgpu_shim_qop.h:
 * right-preconditioned, zero start (x = 0, r = r0 = b), per iteration p = r + beta (p - omega v), y = M^-1 p, v = A y,
 * alpha = rho / (r0.v), x += alpha y, s = r - alpha v (kept in r), exit when |s| <= tolerance; else z = M^-1 s, t = A z,
 * omega = (t.s) / (t.t), x += omega z, r = s - omega t, exit when |r| <= tolerance.  Every scalar (rho, alpha, omega,
 * beta, the norms, the tolerance, the iteration count, the status) lives in a 128-byte device state block; the sums
 * accumulate in double over a fixed grid in a fixed order; the scalars are formed in double and rounded to the number
 * type before any element-wise use.  mfgpu_bicgstab_begin and _iterate only enqueue work on `stream` (no allocation, no
 * synchronisation, no host read-back: they can be captured in a graph); mfgpu_bicgstab_status is the only blocking call.
 * The operator is a callback, so that a handle, a mfgpu_qop (or its transpose) or the caller's own code serves.
 * Status (mfgpu_cg_info): 0 running, 1 converged, 2 max iterations, 3 breakdown (r0.v, t.t or rho zero or not finite; x
 * is then at the last complete update).  iterations counts as SolverControl::steps does: an exit after the half step of
 * iteration k reports k, with residual = |s|.  That exit takes effect on the device: the operator apply and the sums
 * that were enqueued behind it run and write t and partial sums only.
 * Freeze rule: once the status has left 0 every solver kernel returns without writing a vector (the operator and the
 * preconditioner still run, on unchanged inputs), so x, the count and the residual do not depend on how many iterations
 * were enqueued past the end, nor on check_every.
 * One object is used on one stream at a time; x, b and inv_diag must stay valid and unchanged (x: untouched by others)
 * from begin until the solve is over; the operator, V-cycle and callbacks are borrowed and must outlive the solves.   */
typedef struct mfgpu_bicgstab mfgpu_bicgstab;
/* All allocation happens here: the work vectors r, r0, p, v, t (5 vectors of n_dofs numbers; MFGPU_CG_JACOBI and
 * MFGPU_CG_CALLBACK: + y and z = 7; with MFGPU_CG_NONE y is p and z is r), 6 * 2048 doubles of partial sums, the 128-byte
 * state block -- mfgpu_bicgstab_memory_consumption is exactly their sum -- and a pinned host mirror of the state block.
 * preconditioner: MFGPU_CG_NONE, MFGPU_CG_JACOBI (inv_diag_dev of the number type, read, not copied) or
 * MFGPU_CG_CALLBACK.  MFGPU_EINVAL, nothing created: null out, n_dofs == 0, an unknown number type, an unknown
 * preconditioner or MFGPU_CG_CHEBYSHEV (not offered), JACOBI without inv_diag_dev.                                     */
int mfgpu_bicgstab_create(size_t n_dofs, int number_type, int preconditioner, const void *inv_diag_dev,
                          mfgpu_bicgstab **out);
/* the operator, one of three: apply enqueues dst = A src on `stream` (a non-zero return ends begin / iterate with that
 * code); a handle (mfgpu_vmult; MFGPU_EINVAL unless its number type and length are the solver's); a mfgpu_qop
 * (mfgpu_qop_vmult with flags 0 or MFGPU_QOP_TRANSPOSE; MFGPU_EINVAL unless the solver is MFGPU_F64 and of its length) */
int mfgpu_bicgstab_set_operator(mfgpu_bicgstab *s, int (*apply)(void *ctx, void *dst_dev, const void *src_dev, void *stream),
                                void *ctx);
int mfgpu_bicgstab_set_operator_handle(mfgpu_bicgstab *s, mfgpu_handle *A);
int mfgpu_bicgstab_set_operator_qop(mfgpu_bicgstab *s, mfgpu_qop *q, uint32_t flags);
/* a mfgpu_vqop (mfgpu_vqop_vmult; MFGPU_EINVAL unless the solver is MFGPU_F64 and of length dim * n_dofs) */
int mfgpu_bicgstab_set_operator_vqop(mfgpu_bicgstab *s, mfgpu_vqop *q);
/* MFGPU_CG_CALLBACK: fn enqueues z = M^-1 r on `stream`, twice per iteration (y from p, z from s); the library's own
 * callback for a V-cycle, z = mfgpu_vcycle_apply(v, z, r, stream) (MFGPU_EINVAL unless the V-cycle's active type and
 * length are the solver's).  Both: MFGPU_EINVAL for a solver that is not a CALLBACK solver.                          */
int mfgpu_bicgstab_set_callback(mfgpu_bicgstab *s, int (*fn)(void *ctx, void *z_dev, const void *r_dev, void *stream),
                                void *ctx);
int mfgpu_bicgstab_set_vcycle(mfgpu_bicgstab *s, mfgpu_vcycle *v);
/* x = 0, r = r0 = b, p = r, y = M^-1 p; status 1 with 0 iterations if |b| <= tolerance.  MFGPU_EINVAL, nothing written:
 * null pointers, no operator set, CALLBACK without a callback, x overlapping b.  _begin_relative: tolerance =
 * relative_tolerance * |b| formed on the device; MFGPU_EINVAL also for a negative or non-finite relative tolerance.
 * 16-byte accesses when x, b and inv_diag are 16-byte aligned.                                                       */
int mfgpu_bicgstab_begin(mfgpu_bicgstab *s, void *x_dev, const void *b_dev, double tolerance, uint32_t max_iterations,
                         void *stream);
int mfgpu_bicgstab_begin_relative(mfgpu_bicgstab *s, void *x_dev, const void *b_dev, double relative_tolerance,
                                  uint32_t max_iterations, void *stream);
/* n_iterations more iterations (MFGPU_EINVAL before begin): per iteration two operator applies and five solver launches
 * -- the sums of r0.v; alpha, x += alpha y, r -= alpha v, the sums of s.s; the sums of t.s and t.t in one pass; omega,
 * x += omega z, r -= omega t, the sums of r.r and r0.r; count, status, beta and the new p -- plus two preconditioner
 * calls for CALLBACK                                                                                                 */
int mfgpu_bicgstab_iterate(mfgpu_bicgstab *s, uint32_t n_iterations, void *stream);
/* one asynchronous copy of the state block into the pinned mirror and a stream synchronisation (MFGPU_EINVAL before
 * begin) */
int mfgpu_bicgstab_status(mfgpu_bicgstab *s, void *stream, mfgpu_cg_info *info);
/* begin; { iterate(check_every); status } until the status leaves 0.  check_every == 0: MFGPU_EINVAL */
int mfgpu_bicgstab_solve(mfgpu_bicgstab *s, void *x_dev, const void *b_dev, double tolerance, uint32_t max_iterations,
                         uint32_t check_every, void *stream, mfgpu_cg_info *info);
size_t mfgpu_bicgstab_memory_consumption(const mfgpu_bicgstab *s);
void mfgpu_bicgstab_destroy(mfgpu_bicgstab *s);

/* ---- fields and point sources at arbitrary points (no reference counterpart; deal.II: VectorTools::point_value /
 * point_gradient, FEPointEvaluation::evaluate / integrate, create_point_source_vector) --------
 * MFGPU_F64 only (MFGPU_F32 description or integrator: MFGPU_EUNSUPPORTED), dim 2 and 3, degree 1..6, uniform-J0 and
 * general geometry, with and without hanging nodes.  One definition throughout, with N = p+1, x_q the description's
 * quadrature_points of a cell (QGauss(N), x fastest) and L_q the tensor Lagrange basis on the 1D Gauss abscissae:
 *   mapping   x(xi) = sum_q L_q(xi) x_q -- exact for affine cells and MappingQ1 (every mesh stand-in below), not for
 *             mappings of a higher degree (the restriction of the integrator's error points);
 *   field     U_q = the cell's nodal values at the Gauss points, by the steps of mfgpu_integrator_evaluate (gather
 *             through loc2glob, hanging-node resolution, S x S (x S)); u_h(xi) = sum_q L_q(xi) U_q, the same polynomial;
 *   gradient  grad_x u_h = J(xi)^-T grad_xi u_h with J(xi) = sum_q grad L_q(xi) x_q (inv_jac is not needed on the
 *             device, so every integrator serves; with MFGPU_UNIFORM_J0 J is one scalar per cell).
 *
 * mfgpu_locate_points (host only): for each of the n points x [n * dim] the cell that holds it and its reference
 * coordinates xi [n * dim] in [0, 1]^dim.  It reads dim, degree, n_cells, quadrature_points and number_type of the
 * description.  Conditions of the interface (stated, not measured), shared word for word by mfgpu_locator_locate below
 * (the same candidate grid, the same constants: csrc/mfgpu_points.h):
 *   - a cell is a candidate when the point lies in the bounding box of the cell's 2^dim corners (the mapping at xi in
 *     {0, 1}^dim) inflated by 1e-10 of the box's diagonal; candidates are found through a uniform bin grid;
 *   - per candidate, Newton on x(xi) = x from the cell's centre, at most 30 steps, converged when |delta xi|_inf <= 1e-14;
 *     an iteration that diverges or does not converge means "not in this cell";
 *   - a converged candidate is accepted when every xi_d lies in [-1e-10, 1 + 1e-10]; xi is then clamped to [0, 1];
 *   - among the accepting cells the one with the lowest index wins, whatever the bin grid;
 *   - a point no cell accepts gets cell = MFGPU_POINT_NOT_FOUND and xi = 0 and is counted in *n_not_found (may be NULL):
 *     not an error.                                                                                                 */
#define MFGPU_POINT_NOT_FOUND 0xffffffffu
int mfgpu_locate_points(const mfgpu_desc *desc, const double *x, uint32_t n, uint32_t *cell, double *xi,
                        uint32_t *n_not_found);
/* The points object: n points, each in a cell of the integrator's description (or in none), ready for the two calls
 * below.  It BORROWS the integrator's device geometry (loc2glob, constraint mask, tables, quadrature points): the
 * integrator must outlive it.  mfgpu_points_create = mfgpu_locate_points on `desc` (the description the integrator was
 * created from), then mfgpu_points_create_in_cells, which takes (cell [n], xi [n * dim]) as given: MFGPU_POINT_NOT_FOUND is
 * allowed as a cell; any other cell >= n_cells, or a xi outside [0, 1], is MFGPU_EINVAL.  n = 0 is allowed.  The points
 * are sorted by cell and each cell's points are cut into work items of at most 512; everything either call needs is
 * allocated here (the local vectors of integrate and its dof -> slot CSR included), so both calls only enqueue and can
 * be captured in a graph.                                                                                           */
typedef struct mfgpu_points mfgpu_points;
int mfgpu_points_create(mfgpu_integrator *it, const mfgpu_desc *desc, const double *x, uint32_t n, mfgpu_points **out);
int mfgpu_points_create_in_cells(mfgpu_integrator *it, const uint32_t *cell, const double *xi, uint32_t n,
                                 mfgpu_points **out);
/* the cell of every point in the caller's order (host array owned by the object); returns n */
int64_t mfgpu_points_cells(const mfgpu_points *p, const uint32_t **cell);
uint32_t mfgpu_points_n_not_found(const mfgpu_points *p);
/* values [n] = u_h(x_k), gradients [n * dim] = grad_x u_h(x_k) (x, y, z per point), in the caller's point order; device
 * doubles.  Either output may be NULL (both: MFGPU_EINVAL).  u [n_dofs] is read on every dof a cell lists, constrained
 * dofs included, hanging dofs never, as mfgpu_integrator_evaluate does.  Points without a cell get 0.  Every output
 * entry is written by exactly one thread; two calls give bitwise-equal results.  One wave per work item.  Asynchronous. */
int mfgpu_points_evaluate(mfgpu_points *p, const void *u, void *values, void *gradients, void *stream);
/* rhs_i = sum_k w_k phi_i(x_k), the transpose of the value part of mfgpu_points_evaluate, distributed like a cell
 * result: hanging-node resolution transposed, constrained rows 0, every entry of rhs [n_dofs] written.  weights [n] in
 * the caller's point order, NULL = all 1; points without a cell contribute nothing.  No floating-point atomics: the
 * work items' local vectors are summed per dof in ascending (work item, local index) order, so two calls give
 * bitwise-equal results.  Asynchronous; two calls on one object may not overlap (they share the local vectors).      */
int mfgpu_points_integrate(mfgpu_points *p, void *rhs, const void *weights, void *stream);
size_t mfgpu_points_memory_consumption(const mfgpu_points *p); /* device bytes the object owns */
void mfgpu_points_destroy(mfgpu_points *p);

/* ---- point location on the device: mfgpu_locate_points for points that move ---------------
 * The locator is created once per mesh from the integrator and the description it was created from (MFGPU_EINVAL when
 * dim, degree or n_cells disagree or quadrature_points is missing; MFGPU_F32: MFGPU_EUNSUPPORTED).  It builds the
 * candidate grid of mfgpu_locate_points on the host and keeps it on the device; the cells' Gauss points are BORROWED from
 * the integrator, which must outlive the locator.
 *
 * mfgpu_locator_locate: x [n * dim], hint [n] (or NULL), cell [n], xi [n * dim] and n_not_found (one uint32_t, or NULL)
 * are DEVICE pointers.  The call only enqueues on `stream`, allocates nothing and can be captured in a graph; n = 0 is
 * allowed.  The result is defined exactly as for mfgpu_locate_points -- candidates in ascending order through the same
 * bin grid, Newton on F(xi) = sum_q L_q(xi) (x_q - x) from the cell's centre with the same limits and tolerances, the
 * first accepting cell wins, xi clamped to [0, 1], a point no cell accepts (outside the global box and NaN included)
 * gets MFGPU_POINT_NOT_FOUND and xi = 0 -- evaluated in the device's arithmetic: the cells agree with the host's, xi to
 * rounding.  *n_not_found is overwritten by every call (zeroed on the stream, then whole numbers added per wave): it does
 * not accumulate and is deterministic.  One lane per point, every output entry written by its own lane, no
 * floating-point atomics: two calls give bitwise-equal cell and xi.
 * Hints: with hint[k] < n_cells the hinted cell is tried first, Newton from its centre, and taken only if the iteration
 * converges with every xi_d in [1e-8, 1 - 1e-8]; otherwise (also for MFGPU_POINT_NOT_FOUND and any other value >=
 * n_cells) the lane runs the ordinary search from the beginning.  Condition of the interface: the cells do not overlap
 * and neighbouring cells differ in size by less than a factor of 100.  Then a point that far inside a cell is at least
 * 1e-8 h from its boundary while any other cell accepts at most 1e-10 h' beyond its own, so no other cell accepts it and
 * the hinted result equals the unhinted one bit for bit.  Every mesh stand-in below meets the condition.
 * `hint` may be the same pointer as `cell` (a lane reads its hint before it writes its cell); no other pair of
 * arguments may alias.  MFGPU_EINVAL: NULL x, cell or xi with n > 0.                                                    */
typedef struct mfgpu_locator mfgpu_locator;
int mfgpu_locator_create(mfgpu_integrator *it, const mfgpu_desc *desc, mfgpu_locator **out);
int mfgpu_locator_locate(mfgpu_locator *l, const double *x, uint32_t n, const uint32_t *hint, uint32_t *cell, double *xi,
                         uint32_t *n_not_found, void *stream);
size_t mfgpu_locator_memory_consumption(const mfgpu_locator *l); /* device bytes the object owns */
void mfgpu_locator_destroy(mfgpu_locator *l);
/* The points object of (cell [n], xi [n * dim]) in DEVICE memory, as mfgpu_locator_locate leaves them: synchronises
 * `stream`, downloads both (4 + 8 dim bytes per point) and calls mfgpu_points_create_in_cells.  This is the one
 * synchronising step between locating on the device and evaluating; the object is the one described above.            */
int mfgpu_points_create_located(mfgpu_integrator *it, const uint32_t *cell_dev, const double *xi_dev, uint32_t n,
                                void *stream, mfgpu_points **out);

/* ---- deal.II stand-in for the setup side (host only) --------------------------------------
 * Produces what Triangulation + DoFHandler + ConstraintMatrix + FEValues + ShapeInfo hand to
 * MatrixFreeGpu::reinit, for the meshes bmop uses (bmop_common.h:108-120).                    */
typedef struct mfgpu_mesh mfgpu_mesh;

/* hyper_cube(lo,hi) subdivided n_per_dir[d] times per direction (generalises refine_global,
 * poisson_common.h:62-64 + bmop_common.h:119); cells_z_begin/end select a z-slab (last
 * direction) of cells for the multi-GPU partition: DoFs are renumbered slab-locally.         */
int mfgpu_mesh_create_uniform(int dim, int degree, const uint32_t *n_per_dir, double lo, double hi,
                              uint32_t slab_begin, uint32_t slab_end, int number_type,
                              mfgpu_mesh **out);
/* bmop_common.h:49-105 pseudo_adaptive_refinement on the cube (ADAPTIVE_GRID), n_ref as in
 * bmop's argv; octree with 2:1 balance and hanging-node constraints.                          */
int mfgpu_mesh_create_adaptive(int dim, int degree, int n_ref, int number_type, mfgpu_mesh **out);
/* BALL domain of bmop / poisson (-DBALL_GRID; poisson_common.h:65-70, bmop_common.h:108-120): hyper_ball (unit
 * ball, 5 / 7 coarse cells), spherical manifold on the boundary, n_ref global refinements, MappingQ1.  Unstructured;
 * the description has a full J^-1 per quadrature point (no MFGPU_UNIFORM_J0).                                     */
int mfgpu_mesh_create_ball(int dim, int degree, int n_ref, int number_type, mfgpu_mesh **out);
/* MGTransferMatrixFreeGpu::build for two stand-in meshes (uniform cubes n and 2n cells per direction, or ball meshes
 * of n_ref and n_ref + 1): the transfer between them, in the fine mesh's number type                               */
int mfgpu_transfer_create_from_meshes(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, mfgpu_transfer **out);
/* mfgpu_transfer_create_p for two stand-in meshes of the same cells and two degrees, in the fine mesh's number type, with
 * the coarse mesh's Dirichlet dofs; the meshes' current loc2glob is used as it is, so renumbered meshes work.
 * MFGPU_EINVAL: not the same cells (dimension, kind, cells per direction and slab of a cube, n_ref of a ball, cell
 * count) or degree_coarse >= degree_fine; MFGPU_EUNSUPPORTED: a mesh with hanging nodes (adaptive, from leaves)      */
int mfgpu_transfer_create_p_from_meshes(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, mfgpu_transfer **out);
/* mfgpu_transfer_create_p_hn for two stand-in meshes: every pair the call above accepts, and adaptive meshes or meshes
 * from leaves with the same leaves in the same order (then the masks are equal); with the coarse mesh's constraint
 * weights and constrained dofs.  MFGPU_EINVAL: the cells differ, or degree_coarse >= degree_fine                     */
int mfgpu_transfer_create_p_hn_from_meshes(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, mfgpu_transfer **out);
/* the index arrays that call hands to mfgpu_transfer_create, on the host (no GPU needed): coarse_cell_dofs
 * [n_cells * (p+1)^dim], fine_patch_dofs [n_cells * (2p+1)^dim], n_cells = the coarse mesh's; returns n_cells     */
int64_t mfgpu_mesh_transfer_patches(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, uint32_t *coarse_cell_dofs,
                                    uint32_t *fine_patch_dofs);
/* DoFHandler::renumber_dofs on the stand-in: loc2glob, constrained dofs, dof coordinates, interface planes */
int mfgpu_mesh_renumber(mfgpu_mesh *m, const uint32_t *new_index);
/* the same recipe with Triangulation::limit_level_difference_at_vertices (2:1 over vertices too), which the reference's
 * multigrid programs set (poisson_mg.cu:131): required by mfgpu_mg_hierarchy_create                                  */
int mfgpu_mesh_create_adaptive_mg(int dim, int degree, int n_ref, int number_type, mfgpu_mesh **out);
/* Multigrid level hierarchy of an adaptive octree stand-in mesh (host only): what distribute_mg_dofs +
 * MGConstrainedDoFs + MGTransferMatrixFreeGpu::build provide on a locally refined mesh (poisson_mg.cu:152,199-209,
 * 325-326).  Level l = all cells of level l; see csrc/mfgpu_mg_hierarchy.cpp.  The level meshes belong to the hierarchy. */
typedef struct mfgpu_mg_hierarchy mfgpu_mg_hierarchy;
int mfgpu_mg_hierarchy_create(const mfgpu_mesh *adaptive, mfgpu_mg_hierarchy **out);
int mfgpu_mg_n_levels(const mfgpu_mg_hierarchy *h);
const mfgpu_mesh *mfgpu_mg_level_mesh(const mfgpu_mg_hierarchy *h, int level);
int64_t mfgpu_mg_edge_dofs(const mfgpu_mg_hierarchy *h, int level, const uint32_t **ptr); /* refinement-edge dofs */
/* copy_indices of the level: returns n, (active dof, level dof) pairs */
int64_t mfgpu_mg_copy_pairs(const mfgpu_mg_hierarchy *h, int level, const uint32_t **active_dofs, const uint32_t **level_dofs);
/* arrays for mfgpu_transfer_create(level - 1 -> level): returns the number of refined cells of level - 1 */
int64_t mfgpu_mg_transfer_arrays(const mfgpu_mg_hierarchy *h, int level, const uint32_t **coarse_cell_dofs,
                                 const uint32_t **fine_patch_dofs);
void mfgpu_mg_hierarchy_destroy(mfgpu_mg_hierarchy *h);
/* same setup from an explicit one-irregular set of octree leaves (level, cx, cy, cz) x n_leaves on
 * hyper_cube(-1,1): lets tests build the awkward small cases of test_hanging_nodes_gpu.cu:297-331 */
int mfgpu_mesh_create_from_leaves(int dim, int degree, const uint32_t *leaves, uint32_t n_leaves,
                                  int number_type, mfgpu_mesh **out);
/* (level, cx, cy, cz) of every cell in mesh order [n_cells*4]; empty for uniform meshes */
int64_t mfgpu_mesh_cell_levels(const mfgpu_mesh *m, const uint32_t **ptr);
/* ---- global coarsening (host only).  One coarsening step of a set of leaves (level, cx, cy, cz) as
 * for mfgpu_mesh_create_from_leaves, what one step of create_geometric_coarsening_sequence does to a triangulation: every
 * complete family of sibling leaves (all 2^dim children active) is replaced by its parent; then, until nothing changes,
 * a new parent is split again where it breaks one-irregularity (a leaf two or more levels finer than it touches it over
 * a face or, in 3D, an edge).  The result is one-irregular and does not depend on the order.  Returns the number of coarse
 * leaves written to out [room for n_leaves * 4]; MFGPU_EINVAL for a set that is not one-irregular, is not a partition
 * of the root cell, or is the single root cell.                                                                      */
int64_t mfgpu_mesh_coarsen_leaves(int dim, const uint32_t *leaves, uint32_t n_leaves, uint32_t *out /* [n_leaves * 4] */);
/* the map between two leaf meshes (adaptive, from leaves), found from their cell_levels: for every fine cell the index
 * of its coarse cell and child = 0 (the same cell) or 1 + k (child k of it; bit d of k: the upper half in direction d).
 * MFGPU_EINVAL: the meshes differ in dim, or some fine leaf is neither a coarse leaf nor the child of one              */
int mfgpu_mesh_coarsening_map(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, uint32_t *parent /* [n_fine_cells] */,
                              uint32_t *child /* [n_fine_cells] */);
/* mfgpu_transfer_create_h_hn for two leaf meshes of equal degree, the fine one's leaves those of the coarse one or their
 * children (mfgpu_mesh_coarsening_map), in the fine mesh's number type, with the coarse mesh's constrained dofs and
 * constraint weights.  MFGPU_EINVAL: not two leaf meshes, the degrees or dimensions differ, no map                    */
int mfgpu_transfer_create_h_hn_from_meshes(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, mfgpu_transfer **out);
/* ---- adaptive refinement (host only).  One refinement step of a set of leaves: every leaf i with
 * flags[i] != 0 is replaced by its 2^dim children (child k: bit d of k = the upper half in direction d, as in
 * mfgpu_mesh_coarsening_map); then, until nothing changes, every leaf that is touched by a leaf two or more levels finer
 * is split too -- touched over a face or, in 3D, an edge (the relation of mfgpu_mesh_coarsen_leaves), with
 * balance_vertices != 0 also over a vertex (the rule of mfgpu_mesh_create_adaptive_mg).  Splitting only makes the set
 * finer, so the fixed point does not depend on the order.  The input must be one-irregular in the same relation -- over
 * faces and edges, with balance_vertices over vertices too (mfgpu_mesh_create_adaptive_mg meshes and results of this
 * call with balance_vertices are) -- and is refused otherwise: the call balances what it splits, it does not repair an
 * unbalanced input.  The input being one-irregular in that relation, only input leaves ever split:
 * every output leaf is an input leaf or a child of one, and mfgpu_mesh_coarsening_map and
 * mfgpu_transfer_create_h_hn_from_meshes apply to the pair.  Output order: the input order, the children of a split
 * leaf in its place in child order.  Returns the number of leaves written to out [out_capacity * 4]; MFGPU_EINVAL when
 * out_capacity is too small (the message names the needed count), when the input is not a partition of the root cell or
 * not one-irregular over faces and edges (with balance_vertices: and vertices), or when a child would be deeper than
 * level 18.                                                                                                          */
int64_t mfgpu_mesh_refine_leaves(int dim, const uint32_t *leaves, uint32_t n_leaves, const uint8_t *flags,
                                 uint32_t balance_vertices, uint32_t *out, uint64_t out_capacity /* leaves */);
/* ---- refinement and coarsening in one step (host only), what
 * Triangulation::execute_coarsening_and_refinement does with both kinds of flags.
 *  1. R is what mfgpu_mesh_refine_leaves(leaves, refine_flags, balance_vertices) yields: the same closure, the same
 *     checks and refusals.
 *  2. A family (a parent Q with its 2^dim children) is a candidate when all its children are input leaves, all of them
 *     have coarsen_flags != 0, none has a refine flag, and all are still leaves of R (the closure split none).
 *  3. Every candidate family in R is replaced by its parent.
 *  4. Until nothing changes, a new parent is split again when a leaf two or more levels finer touches it, in the
 *     relation of the closure (faces, 3D edges, with balance_vertices vertices): mfgpu_mesh_coarsen_leaves' rollback.  A
 *     rollback only makes the set finer, so the fixed point does not depend on the order.
 * The result is `new`; `mid` is the input with exactly the surviving families replaced by their parents, the common
 * coarsening of old and new.  What holds:
 *  - refinement wins over coarsening;
 *  - new and mid are one-irregular in the relation of the call;
 *  - every old leaf is a leaf of mid or the child of one, and so is every new leaf: mfgpu_mesh_coarsening_map and the
 *    h_hn creators apply to both pairs (mid, old) and (mid, new);
 *  - no flags: new == mid == old; refine flags only: new == mfgpu_mesh_refine_leaves(...), mid == old; all coarsen flags,
 *    no refine flags, no balance_vertices: new == mid == mfgpu_mesh_coarsen_leaves(old) as sets.
 * Order: the input's; the children of a split leaf in its place in child order; a surviving parent where its child 0
 * stood, its other children dropped.  Returns the number of leaves written to out_new [new_capacity * 4] and sets *n_mid
 * to the number written to out_mid [n_leaves * 4].  MFGPU_EINVAL, nothing written: what mfgpu_mesh_refine_leaves
 * refuses, and a new_capacity that is too small (the message names the needed count).                                */
int64_t mfgpu_mesh_adapt_leaves(int dim, const uint32_t *leaves, uint32_t n_leaves, const uint8_t *refine_flags,
                                const uint8_t *coarsen_flags, uint32_t balance_vertices, uint32_t *out_new,
                                uint64_t new_capacity /* leaves */, uint32_t *out_mid /* [n_leaves * 4] */,
                                uint32_t *n_mid);
/* ---- interpolation on the h_hn transfer: the fine function's nodal interpolant on the coarser
 * mesh, what MGTwoLevelTransfer::interpolate and SolutionTransfer give.  The two creators take the arguments of
 * mfgpu_transfer_create_h_hn (mfgpu_transfer_create_h_hn_from_meshes) and make the same object -- prolongate,
 * prolongate_add and restrict_and_add agree bit for bit with it -- plus an interpolation image: per coarse cell the
 * indices of its fine cells, the fine masks per fine cell, a coarse list with owner marking, and interpolation_1d.
 * mfgpu_transfer_interpolate returns MFGPU_EINVAL for any object made without the image; objects from the other creators
 * do not grow.
 *   The owner of a coarse dof is the first coarse cell that lists it at a position its COARSE mask does not constrain
 * (mfgpu_transfer_p_owner_list with the coarse lists and mask).  For the owner K and the local position
 * i = (i_0, ..., i_{dim-1}), xi the Gauss-Lobatto nodes of FE_Q(p) on [0, 1]:
 *  - K is also a fine cell F (child = 0):  v_i = [ C_p(fine_mask_F) gather_F(src) ]_i.  The gather reads every entry of
 *    F's list as it stands in src.
 *  - otherwise b_d = 0 if xi_{i_d} <= 1/2, else 1; k = sum_d b_d 2^d, F_k that child of K;
 *      v_i = sum_j prod_d J1[i_d][j_d] [ C_p(fine_mask_{F_k}) gather_{F_k}(src) ]_j,   J1[i][j] = phi_j(2 xi_i - b(i)),
 *    phi the Lagrange basis of FE_Q(p) on its Gauss-Lobatto nodes.  interpolation_1d [(p+1)^2] row-major replaces J1;
 *    NULL: this default.  At p = 1, 2 every row of J1 is a unit vector: the call is an injection, bit for bit.
 *  - dst[coarse(K, i)] = v_i for owned entries that are not coarse Dirichlet dofs; coarse Dirichlet dofs and dofs that
 *    no coarse cell owns become 0.
 * Stores are plain, no atomics: the same input gives the same bits on two calls and in a replayed graph.  The call only
 * enqueues, reads nothing back and allocates nothing; double and float.  interpolate(prolongate(x)) = x on owned
 * non-Dirichlet dofs up to rounding; an unchanged cell without a fine mask passes its values through bit for bit.
 * The creators refuse (MFGPU_EINVAL) what mfgpu_transfer_create_h_hn refuses, and a pair in which a coarse cell is not
 * exactly one fine cell with child = 0 or all 2^dim children, each once.                                              */
int mfgpu_transfer_create_h_hn_interp(int dim, int degree, int number_type, uint32_t n_coarse_cells, uint32_t n_fine_cells,
                                      const uint32_t *coarse_cell_dofs, const uint32_t *fine_cell_dofs,
                                      const uint32_t *parent, const uint32_t *child, uint32_t n_coarse_dofs,
                                      uint32_t n_fine_dofs, const uint32_t *coarse_dirichlet, uint32_t n_coarse_dirichlet,
                                      const double *prolongation_1d, const uint32_t *coarse_mask, const uint32_t *fine_mask,
                                      const double *constraint_weights,
                                      const double *interpolation_1d /* [(p+1)^2] or NULL */, mfgpu_transfer **out);
int mfgpu_transfer_create_h_hn_interp_from_meshes(const mfgpu_mesh *coarse, const mfgpu_mesh *fine, mfgpu_transfer **out);
int mfgpu_transfer_interpolate(mfgpu_transfer *t, void *dst_coarse_dev, const void *src_fine_dev, void *stream);
void mfgpu_mesh_destroy(mfgpu_mesh *m);
/* fills *desc with pointers into the mesh (valid until mfgpu_mesh_destroy) */
int mfgpu_mesh_desc(const mfgpu_mesh *m, mfgpu_desc *desc);
/* support-point coordinates of every DoF [n_dofs*dim] (double) */
int64_t mfgpu_mesh_dof_coords(const mfgpu_mesh *m, const double **ptr);
/* multi-GPU slabs: local indices of the DoFs on the lower / upper slab interface plane, in the
 * same (lexicographic) order on both neighbours; which = 0 lower, 1 upper                      */
int64_t mfgpu_mesh_interface_dofs(const mfgpu_mesh *m, int which, const uint32_t **ptr);

#ifdef __cplusplus
}
#endif
#endif /* MFGPU_H */
