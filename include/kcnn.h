/*
 * include/kcnn.h -- extern "C" entry points of libkcnn.so above the kernel
 * shim (include/cnsl-hip-kernels.h): the CuMatrixBase extension methods and
 * the nnet2 components, callable with plain device pointers + MatrixDim.
 *
 * Each entry replaces one reference interface:
 *   kcnn_mat_*        CuMatrixBase<float>::{Conv2D, AddMatRepVec, FlipMat,
 *                     PaddingZero, TpBlock, TpInsideBlock, ModPermuteRow,
 *                     Maxpool_prop, Maxpool_backprop}
 *                     (reference src/cudamatrix/cu-matrix.h:451-480;
 *                     bodies src/cnslmat/conv2D.cc:43-684)
 *   kcnn_component_*  nnet2::Component / UpdatableComponent virtuals as the
 *                     nnet0 components override them
 *                     (reference src/nnet0/nnet-component-nnet0.h:23-232,
 *                     src/nnet2/nnet-component.h:157-348) and the factory
 *                     Component::NewFromString / ReadNew
 *                     (src/nnet2/nnet-component.cc:38-136)
 *                     Also the upstream nnet2 components either side of
 *                     the CNN path: SpliceComponent and
 *                     RectifiedLinearComponent (src/nnet2/nnet-component.cc
 *                     :799-827, :2524-2866), by the same entry points.
 *   kcnn_nnet_*       the propagate/backprop loop of upstream nnet2's
 *                     NnetUpdater (not vendored by the reference)
 *                     over a stack of these components.
 *
 * Conventions: every pointer argument to matrix data is DEVICE memory on the
 * active HIP device; functions return 0 on success and a nonzero code on
 * failure (KALDI_ASSERT / KALDI_ERR / HIP errors), with the message in
 * kcnn_last_error().  Output matrices are caller-allocated with the sizes the
 * reference methods would Resize() them to.  All work is enqueued on the
 * stream set by kcnn_set_stream (default: the legacy NULL stream).
 */
#ifndef KCNN_KCNN_H_
#define KCNN_KCNN_H_

#include <stddef.h>
#include <stdint.h>

#include "cnsl-hip-kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- runtime ------------------------------------------------------------ */
const char *kcnn_last_error(void);
const char *kcnn_version(void);
/* Device allocations (CuDevice::Malloc calls) so far: a HIP graph captured
 * over the caching allocator's blocks stays valid while this does not move
 * (bench.py --graph). */
unsigned long long kcnn_device_malloc_calls(void);
/* The f16x3 implicit GEMM's cumulative counts since the last reset (a test
 * and bench diagnostic, no reference counterpart): out[0] its calls, out[1]
 * the tiles and out[2] the single elements its fp32 fix-up kernels
 * recomputed; reset != 0 zeroes them.  Synchronises the device. */
int kcnn_conv_fix_counts(unsigned long long *out, int reset);
/* CuDevice::SelectGpuId(use_gpu, device) (upstream cu-device.h). */
int kcnn_init(int device);
int kcnn_set_stream(kcnn_stream_t stream);
int kcnn_synchronize(void);
int kcnn_set_literal_path(int literal);  /* replay reference call sequences */
int kcnn_set_profiling(int on);
/* kcnn_nnet_* runtime: run a ConvolutionComponent followed by a
 * non-overlapping MaxpoolComponent (1 x 1 x pc, or a 3-D window) as one fused
 * forward that also saves the pool's routing mask, and backprop that pool
 * from the mask.  Outputs and derivatives are identical either way.
 *   0: off.
 *   1 (default): on; the conv output, which nothing in the training step
 *      reads any more, is not stored.  kcnn_nnet_output recomputes it on
 *      request until that conv's backprop has run, and fails after.
 *   2: on, and the conv output is stored as well.
 * Env KCNN_FUSE sets the initial mode. */
int kcnn_set_fusion(int mode);
/* How CuMatrixBase::AddMatMat (every FullyConnectedComponent GEMM) computes
 * its fp32 product (upstream: cuBLAS sgemm, cu-matrix.cc AddMatMat):
 *   0: rocBLAS sgemm on the fp32-input MFMA;
 *   1: the in-house kernel on the bf16 MFMA with each fp32 operand split
 *      exactly into three bf16 parts and the six leading cross products kept
 *      (cu-gemm-x6.hip); the dot-product error bound of sgemm (1e-5 * S per
 *      element) for operands above 2^-110;
 *   2 (default): the in-house kernel on the f16 MFMA with each operand scaled
 *      by a power of two per row of op(A) / column of op(B) and split into
 *      two f16 parts, three cross products kept (cu-gemm-f16x3.hip); the
 *      split's own bound is per scale group (f16-split.h), and the products
 *      touching a group with elements far under its max are checked and
 *      recomputed in fp32 where needed, so every element meets the 1e-5 * S
 *      bound at any fp32 range; IEEE Inf / NaN rows and columns; shapes past
 *      its 32-bit addressing run mode 1.  The tile of C per workgroup,
 *      256 x 128 or 256 x 256, is chosen per call by a cost model of the
 *      call's shape, transposes and alignment alone (same bits either way
 *      where K is not split);
 *   3: mode 2 with the 256 x 256 tile for every call that can take it (no
 *      row-contiguous operand with an unaligned pitch);
 *   4: mode 2 with the 256 x 128 tile for every call.
 * Env KCNN_GEMM (0 to 4) sets the initial mode. */
int kcnn_set_gemm_mode(int mode);
/* The f16x3 GEMM's launches since the last reset: out[0] on the 256 x 128
 * tile, out[1] on the 256 x 256 tile; reset != 0 zeroes them (a test and
 * bench diagnostic, no reference counterpart). */
int kcnn_gemm_tile_counts(unsigned long long *out, int reset);
/* The plan the f16x3 GEMM would give a call under the current "gemm"
 * selector, computed without a GPU: out[0] the tile's columns (128 or 256),
 * out[1] the split-K count, out[2] the whole tiles in front of the split
 * ones.  lda / ldb are the pitches of A and B (16-B aligned bases assumed). */
int kcnn_gemm_plan(int trans_a, int trans_b, int m, int n, int k, int lda, int ldb, int *out);
/* The f16x3 GEMM's split-K calls since the last reset: out[0] those that
 * launched the fix-up kernel after the reduce, out[1] those that skipped it
 * (their reduce recomputes every rejected element itself); reset != 0 zeroes
 * them.  A call launches the fix-up when its site (shape, transposes,
 * momentum or not) is new, has no slot in the site table, or reported a
 * deferred group in its previous call.  Host counters: no device call. */
int kcnn_gemm_fixup_counts(unsigned long long *out, int reset);
/* Forget every fix-up call site: the next split-K call at any key is a new
 * site and launches the fix-up.  Host only, no device call; meant for a
 * synchronised device (a reduce still in flight may set a reused word, which
 * costs one fix-up launch, never a result).  A test diagnostic. */
int kcnn_gemm_fixup_sites_reset(void);
/* Kernel-family selectors (kaldi-lite/kcnn-knobs.h): each picks
 * one of the implementations of the same fp32 math: the split-operand
 * kernels on the f16 / bf16 matrix cores (f16x3: two f16 parts under a
 * power-of-two scale, three products; bf16x6: three bf16 parts, six
 * products) or the fp32-input MFMA kernels (0).
 *   "fwd_x6"   frame-resident conv forward      2 (default, f16x3) / 1 / 0
 *   "bwd_x6"   fused conv backward              1 (default) / 0
 *   "igemm_x6" implicit-GEMM forward and dgrad  2 (default: f16x3 for
 *              convolutions of >= 2^34 flop, bf16x6 below) / 3 (f16x3 for
 *              all) / 1 (bf16x6) / 0
 *   "wgrad_x6" long-kernel weight gradient      2 (default, wide bf16x6) / 3
 *              (wide f16x3) / 1 (128-wide bf16x6) / 0
 *   "gemm"     AddMatMat (= kcnn_set_gemm_mode) 2 (default, f16x3, tile by
 *              the cost model) / 3 (f16x3, 256 x 256 tile) / 4 (f16x3,
 *              256 x 128 tile) / 1 / 0
 * The environment variables KCNN_FWD_X6, KCNN_BWD_X6, KCNN_IGEMM_X6,
 * KCNN_WGRAD_X6 and KCNN_GEMM set the initial values.  Returns nonzero for
 * an unknown name or value. */
int kcnn_set_kernel_family(const char *name, int value);
/* The current value of a selector, or -1 for an unknown name. */
int kcnn_get_kernel_family(const char *name);
/* C[m x n] = alpha * op(A) op(B) + beta * C on row-major fp32 matrices,
 * exactly CuMatrixBase::AddMatMat(alpha, A, transA, B, transB, beta) with
 * op(X) = X^T when trans_x (cu-matrix.h, upstream Kaldi). */
int kcnn_gemm(int trans_a, int trans_b, int m, int n, int k, float alpha,
              const float *a, int lda, const float *b, int ldb, float beta,
              float *c, int ldc);
/* The bf16 plane form of an fp32 matrix (kaldi-lite/cu-gemm-x6.hip): x =
 * h + m + l exactly, the three bf16 planes [rows x cols] at dst, dst + ps,
 * dst + 2 ps (pitch ldp elements). */
int kcnn_split_planes(const float *src, int rows, int cols, int ld, uint16_t *dst, int ldp,
                      int64_t ps);
/* kcnn_gemm from plane-split operands (a, b as made by kcnn_split_planes,
 * plane strides aps, bps): the six-product bf16 MFMA kernel with no split
 * work in it.  Needs k % 32 == 0, lda / ldb / plane strides % 8 == 0 and,
 * on a row-contiguous operand (A^T or B), its row count % 8 == 0. */
int kcnn_gemm_planes(int trans_a, int trans_b, int m, int n, int k, float alpha,
                     const uint16_t *a, int lda, int64_t aps, const uint16_t *b, int ldb,
                     int64_t bps, float beta, float *c, int ldc);
/* Writes the per-function hipEvent profile (CuDevice::PrintProfile). */
int kcnn_profile_string(char *buf, size_t len);
/* Drops every accumulated and pending profile entry (CuDevice::ResetProfile). */
int kcnn_reset_profile(void);
void kcnn_set_randn_seed(uint64_t seed);
/* Host-side self test of the FastDiv helper; no GPU needed. */
int kcnn_selftest_fastdiv(void);

/* ---- CuMatrixBase methods (cu-matrix.h:451-480) ---------------------------- */
int kcnn_mat_conv2d(const float *in, MatrixDim in_dim, const float *kernel,
                    MatrixDim kernel_dim, int in_height, int in_width,
                    int in_channel, int kernel_height, int kernel_width,
                    int group, float *out, MatrixDim out_dim, int concat);
int kcnn_mat_add_mat_rep_vec(float *m, MatrixDim dim, const float *vec,
                             int vec_dim, int rep);
int kcnn_mat_flip_mat(const float *m, MatrixDim dim, int kernel_height,
                      int kernel_width, int in_channel, int group, float *flip,
                      MatrixDim flip_dim);
int kcnn_mat_padding_zero(const float *m, MatrixDim dim, int orig_height,
                          int orig_width, int orig_channel, int kernel_height,
                          int kernel_width, float *padmat, MatrixDim pad_dim);
int kcnn_mat_tp_block(const float *m, MatrixDim dim, int in_channel,
                      int block_size, float *out, MatrixDim out_dim);
int kcnn_mat_tp_inside_block(const float *m, MatrixDim dim, int group,
                             int block_size, float *out, MatrixDim out_dim);
int kcnn_mat_mod_permute_row(const float *m, MatrixDim dim, int in_channel,
                             int block_size, float *out, MatrixDim out_dim);
/* CuMatrixBase::ModPermuteChannel (conv2D.cc:685-727); comp is written when
 * from_comp_to_container == 0. */
int kcnn_mat_mod_permute_channel(float *comp, MatrixDim dim, int comp_idx,
                                 int num_component, int in_height, int in_width,
                                 float *container, MatrixDim container_dim,
                                 int from_comp_to_container);
int kcnn_mat_maxpool_prop(const float *in, MatrixDim in_dim, int in_height,
                          int in_width, int pool_height_dim,
                          int pool_width_dim, int pool_channel_dim,
                          int overlap, int overlap2D, float *out,
                          MatrixDim out_dim);
int kcnn_mat_maxpool_backprop(const float *in_value, MatrixDim in_dim,
                              const float *out_value, MatrixDim ov_dim,
                              const float *out_deriv, MatrixDim od_dim,
                              float *in_deriv, MatrixDim id_dim, int in_height,
                              int in_width, int pool_height_dim,
                              int pool_width_dim, int pool_channel_dim,
                              int overlap, int overlap2D);

/* ---- components ------------------------------------------------------------ */
typedef struct kcnn_component kcnn_component;

/* Component::NewFromString, e.g. "ConvolutionComponent in-height=40 ...". */
kcnn_component *kcnn_component_new_from_string(const char *initializer_line);
/* Component::ReadNew from a Kaldi stream file written by kcnn_component_write
 * (binary files start with the "\0B" header). */
kcnn_component *kcnn_component_read(const char *path);
int kcnn_component_write(const kcnn_component *c, const char *path, int binary);
kcnn_component *kcnn_component_copy(const kcnn_component *c);
void kcnn_component_free(kcnn_component *c);
int kcnn_component_type(const kcnn_component *c, char *buf, size_t len);
int kcnn_component_info(const kcnn_component *c, char *buf, size_t len);
int kcnn_component_input_dim(const kcnn_component *c);
int kcnn_component_output_dim(const kcnn_component *c);
/* Component::Context() (reference nnet-component.h:186-188): the frame
 * offsets the component reads per output frame -- {0} except SpliceComponent
 * (its left..right context).  Writes up to max_len offsets, returns the count
 * (-1 on error).  For propagate/backprop the input chunk is the output chunk
 * widened by this context: in_rows/num_chunks = out_rows/num_chunks +
 * back - front. */
int kcnn_component_context(const kcnn_component *c, int *offsets, int max_len);
/* NonlinearComponent::ValueSum()/DerivSum()/Count() (reference
 * nnet-component.h:377-379; accumulated by UpdateStats in Backprop when
 * to_update is set): copies up to max_len fp64 values to HOST arrays, *len =
 * their length (0 before the first update). */
int kcnn_component_nonlinear_stats(const kcnn_component *c, double *value_sum,
                                   double *deriv_sum, int max_len, int *len,
                                   double *count);
int kcnn_component_backprop_needs_input(const kcnn_component *c);
int kcnn_component_backprop_needs_output(const kcnn_component *c);
/* Component::Propagate(ChunkInfo(in_dim.cols, num_chunks, 0, rows/num_chunks-1),
 * ..., in, out). */
int kcnn_component_propagate(const kcnn_component *c, const float *in,
                             MatrixDim in_dim, float *out, MatrixDim out_dim,
                             int num_chunks);
/* Component::Backprop(..., to_update = update ? this : NULL, in_deriv);
 * in_deriv may be NULL to skip the data gradient. */
int kcnn_component_backprop(kcnn_component *c, const float *in_value,
                            MatrixDim in_dim, const float *out_value,
                            MatrixDim ov_dim, const float *out_deriv,
                            MatrixDim od_dim, float *in_deriv,
                            MatrixDim id_dim, int num_chunks, int update);
/* Parameter access.  which: 0 = linear params, 1 = bias (as a 1 x N matrix),
 * 2 = prev_grad_ (momentum buffer).  Sizes via kcnn_component_param_dim. */
int kcnn_component_param_dim(const kcnn_component *c, int which, int *rows,
                             int *cols);
int kcnn_component_get_param(const kcnn_component *c, int which, float *dst,
                             MatrixDim dst_dim);
int kcnn_component_set_param(kcnn_component *c, int which, const float *src,
                             MatrixDim src_dim);
float kcnn_component_learning_rate(const kcnn_component *c);
int kcnn_component_set_learning_rate(kcnn_component *c, float lr);
/* UpdatableComponent::DotProduct / SetZero / Scale / Add / PerturbParams. */
int kcnn_component_dot_product(const kcnn_component *a, const kcnn_component *b,
                               float *out);
int kcnn_component_set_zero(kcnn_component *c, int treat_as_gradient);
int kcnn_component_scale(kcnn_component *c, float scale);
int kcnn_component_add(kcnn_component *c, float alpha,
                       const kcnn_component *other);
int kcnn_component_perturb_params(kcnn_component *c, float stddev);
/* Data-parallel split of Update: flat gradient [linear | bias] (floats). */
int kcnn_component_num_gradient_params(const kcnn_component *c);
int kcnn_component_compute_gradient(const kcnn_component *c,
                                    const float *in_value, MatrixDim in_dim,
                                    const float *out_deriv, MatrixDim od_dim,
                                    float *grad);
int kcnn_component_apply_gradient(kcnn_component *c, const float *grad,
                                  int num_sample);
/* Backprop without update (in_deriv nullable: no data gradient) AND
 * ComputeGradient in one call; ConvolutionComponent runs both from a single
 * pass over out_deriv (hipF_conv2d_backward).  in_deriv must be preallocated
 * [rows x InputDim]. */
int kcnn_component_backprop_gradient(const kcnn_component *c,
                                     const float *in_value, MatrixDim in_dim,
                                     const float *out_deriv, MatrixDim od_dim,
                                     float *in_deriv, MatrixDim id_dim,
                                     float *grad);
/* ConvolutionComponent only: 1 if Backprop's reference branch is
 * "flip kernel" (nnet-component-nnet0.cc:489-497). */
int kcnn_component_conv_flip_branch(const kcnn_component *c);
/* DropoutComponent only.  SetDropoutScale (reference nnet-component.h:1611):
 * a scale of 1.0 makes Propagate the identity (inference).  The mask of
 * Propagate call k is a pure function of (seed, k, row, column): the seed is
 * drawn from the host generator (kcnn_set_randn_seed) by Init, Copy and Read;
 * setting it also restarts the call count. */
int kcnn_component_set_dropout_scale(kcnn_component *c, float scale);
int kcnn_component_dropout_seed(const kcnn_component *c, uint64_t *seed);
int kcnn_component_set_dropout_seed(kcnn_component *c, uint64_t seed);
/* The row of the minibatch that row 0 of Propagate's input is (default 0):
 * the mask of row r is the one drawn for row offset + r, so data-parallel
 * ranks that share a seed and a call count draw the masks of their own shards
 * of one global minibatch, and offset 0 draws what a whole minibatch draws.
 * A Propagate with offset + rows > 2^32 is an error that runs no kernel.  The
 * offset is not written to files and a copy starts at 0. */
int kcnn_component_set_dropout_row_offset(kcnn_component *c, uint64_t offset);

/* CuMatrix::CompObjfAndDeriv (reference cudamatrix/cu-matrix.h:624-637) for
 * num HOST elements {rows[i], cols[i], weights[i]} with no repeated (row,
 * col), all inside the matrix (checked; an error runs no kernel): on the
 * DEVICE matrices, deriv(row, col) += weight / probs(row, col); *tot_objf =
 * sum weight * log probs(row, col) and *tot_weight = sum weight (host fp64,
 * reduced in a fixed order).  Synchronises. */
int kcnn_comp_objf_and_deriv(const int32_t *rows, const int32_t *cols, const float *weights,
                             int num, const float *probs, MatrixDim p_dim, float *deriv,
                             MatrixDim d_dim, double *tot_objf, double *tot_weight);

/* The forward half of the above plus the frame accuracy (upstream
 * NnetUpdater::ComputeTotAccuracy over CuMatrixBase::FindRowMaxId, reference
 * cudamatrix/cu-matrix.h:257), with no derivative: for num HOST elements as
 * above (checked; an error runs no kernel) and the DEVICE matrix probs,
 * out[0] = sum weight * log probs(row, col), out[1] = sum weight and out[2] =
 * the sum of the weights of the elements whose column is their row's best
 * column: the lowest column whose value is greater than every earlier
 * column's, the comparison starting from -1e21 (so a NaN is never the best,
 * and a row may have no best column).  Host fp64, reduced in a fixed order.
 * Synchronises. */
int kcnn_comp_objf_accuracy(const int32_t *rows, const int32_t *cols, const float *weights,
                            int num, const float *probs, MatrixDim p_dim, double out[3]);

/* ---- component stack (NnetUpdater-style) -------------------------------- */
typedef struct kcnn_nnet kcnn_nnet;
/* One component initializer line per '\n'-separated line of `config`. */
kcnn_nnet *kcnn_nnet_new(const char *config);
/* A whole network from / to a Kaldi stream file in the layout of upstream
 * Nnet::Read / Nnet::Write (what nnet-init writes and nnet-am-copy and
 * nnet-train* pass around):
 *   <Nnet> <NumComponents> int32 n <Components> n x Component::Write
 *   </Components> </Nnet>
 * binary after the "\0B" header, else text with a newline after each
 * component.  Reading expects exactly these tokens in this order, then checks
 * the network as kcnn_nnet_new does; anything else (a missing or unknown
 * token, a count that disagrees with the content, a truncated file,
 * mismatched dimensions) returns NULL with the message in kcnn_last_error().
 * The AmNnet wrapper of a .mdl file (TransitionModel and priors around the
 * Nnet) is not read. */
kcnn_nnet *kcnn_nnet_read(const char *path);
int kcnn_nnet_write(const kcnn_nnet *n, const char *path, int binary);
/* nnet-am-copy: a NEW network of Component::Copy()s of n's components; n is
 * not changed.  scales != NULL (upstream --scales, Nnet::ScaleComponents):
 * num_scales must be the number of updatable components, and the k-th of them
 * is scaled by UpdatableComponent::Scale(scales[k]).  remove_dropout != 0
 * (--remove-dropout, Nnet::RemoveDropout): every DropoutComponent is left
 * out.  The result is checked as kcnn_nnet_new checks; NULL on error. */
kcnn_nnet *kcnn_nnet_copy(const kcnn_nnet *n, const float *scales, int num_scales,
                          int remove_dropout);
void kcnn_nnet_free(kcnn_nnet *n);
int kcnn_nnet_num_components(const kcnn_nnet *n);
kcnn_component *kcnn_nnet_component(kcnn_nnet *n, int i);  /* borrowed */
/* Forward over all components; keeps every layer's output for Backprop. */
int kcnn_nnet_propagate(kcnn_nnet *n, const float *in, MatrixDim in_dim);
/* Device pointer + dims of layer i's output (i = -1: the input copy). */
int kcnn_nnet_output(const kcnn_nnet *n, int i, const float **data,
                     MatrixDim *dim);
/* Device pointer + dims of d(input_i) left by the last backprop of
 * component i (rows = 0 before one ran, or when it was skipped). */
int kcnn_nnet_input_deriv(const kcnn_nnet *n, int i, const float **data,
                          MatrixDim *dim);
/* Backprop of component i given d(output_i) = the buffer filled by the
 * previous call (or `out_deriv` for the last component).  mode 0: reference
 * (update in place); 1: write the gradient into grad (device, length
 * kcnn_component_num_gradient_params) without updating; 2: data gradient
 * only; 3: the gradient only, for an updatable component that is not half
 * of a fused Conv -> Maxpool pair (a mode 2 call then adds its data
 * gradient; data parallelism starts the gradient's all-reduce in between).
 * The data gradient of component 0 is skipped when skip_first_dx. */
int kcnn_nnet_backprop_component(kcnn_nnet *n, int i, const float *out_deriv,
                                 MatrixDim od_dim, int mode, float *grad,
                                 int skip_first_dx);
/* Full backward pass, last component to first, mode 0 (reference). */
/* An affine layer (FullyConnected / Affine) in data-parallel training: its
 * parameter gradient into grad (mode 3), then between(ctx) -- where the caller
 * starts the gradient's all-reduce -- then its input derivative (mode 2),
 * unless i == 0 and skip_first_dx.  The same results as the mode 3 and mode 2
 * calls; both GEMMs' operand statistics come from one launch set. */
int kcnn_nnet_backprop_split(kcnn_nnet *n, int i, const float *out_deriv, MatrixDim od_dim,
                             float *grad, int skip_first_dx, void (*between)(void *),
                             void *ctx);
int kcnn_nnet_backprop(kcnn_nnet *n, const float *out_deriv, MatrixDim od_dim);
/* A training step's backward from labels (upstream NnetUpdater::
 * ComputeObjfAndDeriv + Backprop): num HOST elements {row, col, weight} of
 * the last Propagate's output, rows non-decreasing, every (row, col) inside
 * the output and none repeated -- checked on the host before anything is
 * launched; a violation is an error that runs no kernel.  The objective
 * sum weight * log output(row, col) and the weight are added to device fp64
 * totals (kcnn_nnet_objf_total); the call does not synchronise.  The output
 * derivative weight / output(row, col) is backpropagated through every
 * component in mode 0.  When the last component is a SoftmaxComponent the
 * derivative, the objective and its Backprop run as one kernel, unless
 * kcnn_set_literal_path(1) asks for the literal sequence. */
int kcnn_nnet_backprop_xent(kcnn_nnet *n, const int32_t *rows, const int32_t *cols,
                            const float *weights, int num, int skip_first_dx);
/* The first half of kcnn_nnet_backprop_xent, for a caller that runs the
 * backward itself (data parallelism: per component, the gradients all-reduced
 * before the update): the same label contract and the same checks before any
 * launch; the labels are staged, the objective and the weight added to the
 * totals of kcnn_nnet_objf_total, and the output derivative is left where
 * kcnn_nnet_backprop_component / _backprop_split read it.  *first is the
 * component the backward starts at; *out_deriv / *od_dim are what to pass to
 * those calls (the library's matrix, valid until the next call of this
 * function).  With a last SoftmaxComponent, unless kcnn_set_literal_path(1),
 * the fused kernel has already written that Softmax's input derivative:
 * *first is num_components - 2 (-1 for a network of one Softmax: nothing is
 * left to run), *out_deriv is NULL with a zero dim, since no component below
 * the last reads it, and kcnn_nnet_backprop_component / _backprop_split of
 * the LAST component are an error until the next forward pass -- its output
 * derivative was never formed.  Otherwise *first is num_components - 1.
 * Does not synchronise. */
int kcnn_nnet_xent_deriv(kcnn_nnet *n, const int32_t *rows, const int32_t *cols,
                         const float *weights, int num, int *first, const float **out_deriv,
                         MatrixDim *od_dim);
/* kcnn_component_set_dropout_row_offset on every DropoutComponent of the
 * stack; nothing for a stack without one.  Holds until it is set again. */
int kcnn_nnet_set_row_offset(kcnn_nnet *n, uint64_t offset);
/* Every DropoutComponent of the stack counts one Propagate call without
 * running one (the mask is a function of the call number): a data-parallel
 * rank whose shard of a minibatch is empty runs no forward pass, and with this
 * call its next masks are still those of the other ranks' call number. */
int kcnn_nnet_skip_dropout_call(kcnn_nnet *n);
/* out[0] = the objective, out[1] = the weight accumulated by
 * kcnn_nnet_backprop_xent / _xent_deriv since the last reset (their ratio is
 * the average log-probability per frame); reset != 0 zeroes them.
 * Synchronises. */
int kcnn_nnet_objf_total(kcnn_nnet *n, double *out, int reset);
/* nnet-compute-prob on one minibatch: the forward pass over `in` and, for num
 * HOST label elements under the contract of kcnn_nnet_backprop_xent (checked
 * by the same code before anything is launched; a violation runs no kernel),
 * the objective sum weight * log output(row, col), the weight, and the
 * accuracy weight of kcnn_comp_objf_accuracy, added to device fp64 totals of
 * their own (kcnn_nnet_prob_total; not those of kcnn_nnet_objf_total).  The
 * call does not synchronise.  It changes no parameter, no momentum buffer and
 * no NonlinearComponent statistic, and it runs the components as they are: a
 * DropoutComponent still draws its mask, so evaluate the network that
 * kcnn_nnet_copy(n, scales, k, 1) gives.  When the last component is a
 * SoftmaxComponent it is not run: one kernel forms each probability from the
 * logits with the Softmax's own operation sequence and takes the three sums,
 * and the output matrix is never written; kcnn_set_literal_path(1) asks for
 * the literal sequence (Propagate, then one pass over the stored output).
 * Afterwards there is nothing to backpropagate: kcnn_nnet_backprop,
 * _backprop_component, _backprop_split and _backprop_xent fail until the
 * next kcnn_nnet_propagate.  kcnn_nnet_output still works: the last output,
 * where it was not stored, is recomputed on request. */
int kcnn_nnet_compute_prob(kcnn_nnet *n, const float *in, MatrixDim in_dim,
                           const int32_t *rows, const int32_t *cols,
                           const float *weights, int num);
/* out[0] = the objective, out[1] = the weight and out[2] = the accuracy weight
 * accumulated by kcnn_nnet_compute_prob since the last reset (out[0] / out[1]
 * is the average log-probability per frame, out[2] / out[1] the frame
 * accuracy); reset != 0 zeroes them.  Synchronises. */
int kcnn_nnet_prob_total(kcnn_nnet *n, double out[3], int reset);

/* The frames the network reads before / after the frame it computes: the sums
 * over the components of -Context().front() / Context().back() (upstream
 * Nnet::LeftContext / Nnet::RightContext; 10 and 10 for nnet.config). */
int kcnn_nnet_left_context(const kcnn_nnet *n);
int kcnn_nnet_right_context(const kcnn_nnet *n);
/* The forward pass of upstream NnetComputer (nnet-am-compute, the decodable
 * of nnet-latgen-faster) on num_utts >= 1 whole utterances: `in` is the
 * DEVICE matrix [sum of lengths x InputDim] of their feature frames stacked
 * row-wise, lengths the HOST array of their frame counts (each >= 1).  Each
 * utterance is propagated as ONE chunk of many rows (Nnet::ComputeChunkInfo
 * (num_rows, 1)), all of them in one pass.  With L and R the contexts above:
 *   pad_input != 0 (upstream's default): an utterance of T frames is seen as
 *     frames -L .. T-1+R, frame f being frame clamp(f, 0, T-1), and gives T
 *     rows.  The padded frames are never stored.
 *   pad_input == 0: it is seen as it is and gives T - L - R rows; T <= L + R
 *     is an error.
 * The result, *data / *dim, is a borrowed device view, valid until the next
 * forward call (kcnn_nnet_propagate, _compute_prob, _compute), of [sum of the
 * utterances' result rows x OutputDim], utterances in order.  From the last
 * output P it is
 *   apply_log != 0: log(max(P, 1e-20)) - prior_scale * log(priors[col])
 *     (nnet-am-compute --apply-log --divide-by-priors, DecodableAmNnet), a NaN
 *     staying NaN; priors == NULL drops the second term.  log in fp64 of the
 *     fp32 P, the log-priors formed on the host in fp64, one fp64 subtraction,
 *     one rounding to fp32.  A last SoftmaxComponent is then not run: one
 *     kernel forms each probability from its input and writes the result
 *     (kcnn_set_literal_path(1): Softmax, then a pass over its stored output;
 *     the same bits).
 *   apply_log == 0: P itself; priors are then REFUSED (P / prior^prior_scale
 *     is not offered).
 * priors: num_priors == OutputDim HOST floats, all finite and > 0.  Every
 * check (lengths, their sum against in_dim.rows, the columns, the priors) is
 * made before anything is launched; a violation is an error that runs no
 * kernel and leaves the last result as it was.  The call does not synchronise
 * and reads nothing back.  It changes no component (a DropoutComponent still
 * draws its mask: use the test model kcnn_nnet_copy(n, scales, k, 1) gives)
 * and leaves the state kcnn_nnet_compute_prob leaves: the backprop calls fail
 * until the next kcnn_nnet_propagate, and kcnn_nnet_objf_total / _prob_total
 * are untouched.  kcnn_nnet_output(n, i) gives layer i's whole-utterance
 * activation: an utterance has there the rows of its result plus the context
 * of the components above (i = -1: the input, or, when component 0 is not a
 * SpliceComponent, pad_input != 0 and L + R > 0, the clamped frames laid out
 * for it). */
int kcnn_nnet_compute(kcnn_nnet *n, const float *in, MatrixDim in_dim, const int32_t *lengths,
                      int num_utts, int pad_input, const float *priors, int num_priors,
                      float prior_scale, int apply_log, const float **data, MatrixDim *dim);

/* kcnn_nnet_compute with the convolutional layers run once per time step
 * instead of once per window (opt-in; kcnn_nnet_compute is the default and the
 * yardstick).  For a stack that starts SpliceComponent -> {Convolution |
 * Maxpool | RectifiedLinear}..., every column of a window's convolution output
 * is a function of the frames under that column alone, so frames t and t + 1
 * share all but one column of each such layer.  Those leading components (the
 * prefix; kcnn_nnet_time_shared_prefix of them) then run as TIME MAPS, one row
 * per row of the input (with pad_input laid out clamped, T + L + R rows an
 * utterance).  A level is (channels C, height H, positions n, dilation d): a
 * map row holds H C floats, element (h, c) at column h + c H, and element
 * (h, position k, channel c) of the window-layout row of result frame t of
 * utterance u, column h + k H + c H n, is row base_u + t + d k, column h + c H
 * of the map, base_u the utterance's first input row.  Level 0, the Splice's
 * output, is (1, input-dim, L + R + 1, 1).  Covered:
 *   - a Convolution of its level's geometry (in-channel C, in-height H,
 *     in-width n) with stride 1 and no padding, kernel-height <= H and
 *     kernel-width <= n: (group, H - kh + 1, n - kw + 1, d).  Along time alone
 *     (the whole frame on the Splice, H = 1 above) its taps are GEMMs of the
 *     library's engine on row-shifted views; along frequency too (kh < H, or a
 *     level with H > 1 below) it is one implicit GEMM over (tap, channel,
 *     kernel row) on the bf16 matrix cores;
 *   - a Maxpool ph x pw x pc of its level's geometry, not overlapping and
 *     dividing evenly: (C / pc, H / ph, n / pw, d pw), the reference's fold
 *     over channels, dilated rows and heights;
 *   - a RectifiedLinear of dim C H n.
 * A gather then writes the output of component prefix - 1 in the window
 * layout, and from component prefix upwards the pass is kcnn_nnet_compute's
 * own.  Same arguments, checks, errors (under this function's name), result
 * layout and state as kcnn_nnet_compute.  The values agree with
 * kcnn_nnet_compute's to the error bar of the GEMMs (both are fp32-exact
 * products under the same bar), not to the bit: the sums are taken in another
 * order.  Afterwards kcnn_nnet_output(n, i) fails for i in [0, prefix - 2] --
 * those activations are never formed -- and kcnn_nnet_time_map gives the maps.
 * When the prefix is 0 this IS kcnn_nnet_compute (the same bits). */
int kcnn_nnet_compute_shared(kcnn_nnet *n, const float *in, MatrixDim in_dim,
                             const int32_t *lengths, int num_utts, int pad_input,
                             const float *priors, int num_priors, float prior_scale,
                             int apply_log, const float **data, MatrixDim *dim);
/* The number of leading components kcnn_nnet_compute_shared runs as time maps
 * (14 for nnet.config, 4 for train_conv.config and for freq_conv.config), 0
 * when it would run kcnn_nnet_compute instead: component 0 is not a
 * SpliceComponent with a contiguous context and const-component-dim = 0, no
 * Convolution follows it before another kind of component (a pool or a ReLU
 * of the Splice's output itself has no prefix), a Convolution or Maxpool of
 * the run is not of the shape above (in-pad-height or in-pad-width set, a
 * stride, in-channel != 1 on the Splice, a geometry that is not its level's,
 * an overlapping or uneven pool, more filters or rows than one launch takes),
 * a component above component 0 has a context of its own, or
 * kcnn_set_literal_path(1) is in force.  Touches no device. */
int kcnn_nnet_time_shared_prefix(const kcnn_nnet *n);
/* Level `level` in [0, prefix) of the last kcnn_nnet_compute_shared (level i
 * is the output of component i; level 0 the input, clamped when padded): a
 * borrowed device view *data / *dim of its computed rows -- all of level 0's,
 * fewer above by the taps' reach -- of *channels channels (dim->cols is the
 * level's height times *channels, kcnn_nnet_time_map_height; level 0: channels
 * = 1 and dim->cols = InputDim), with the level's positions and dilation.  Rows
 * whose taps cross from one utterance into the next are computed and read by
 * nothing.  Valid until the next forward call; an error when the last forward
 * call was not a kcnn_nnet_compute_shared over time maps.  For tests and
 * debugging. */
int kcnn_nnet_time_map(const kcnn_nnet *n, int level, const float **data, MatrixDim *dim,
                       int *channels, int *positions, int *dilation);
/* The height H of that level: dim->cols of kcnn_nnet_time_map is H *channels,
 * element (h, c) at column h + c H (level 0: H = InputDim, one channel; 1 for
 * a level without a frequency axis).  The same errors. */
int kcnn_nnet_time_map_height(const kcnn_nnet *n, int level, int *height);

/* ---- training from a corpus that stays on the device --------------------- */
/* What nnet-get-egs and nnet-shuffle-egs do for nnet-train, without the
 * window matrices: the corpus is the DEVICE matrix feats [sum of lengths x
 * InputDim] of whole utterances stacked row-wise, lengths the HOST array of
 * their num_utts >= 1 frame counts (each >= 1, summing to dim.rows).  The
 * handle BORROWS feats, which must outlive it, and keeps the utterances' starts
 * as a host prefix array, so a minibatch does no O(utterances) work.  NULL on
 * error (bad lengths, an empty matrix or one of 2^31 elements), the message
 * in kcnn_last_error(); nothing on the device is touched. */
typedef struct kcnn_corpus kcnn_corpus;
kcnn_corpus *kcnn_corpus_new(const float *feats, MatrixDim dim, const int32_t *lengths,
                             int num_utts);
void kcnn_corpus_free(kcnn_corpus *c);
/* kcnn_nnet_propagate on a minibatch given as num_frames >= 1 HOST indices of
 * corpus rows, in any order, repeats allowed.  Example n with row r =
 * frames[n] in the utterance of rows [s, e) has the input chunk of rows
 * clamp(r + o, s, e - 1) for the offsets o = -L .. R of the contexts above
 * (what nnet-get-egs writes for frame r), and the pass computes what
 * kcnn_nnet_propagate computes on the [(L + 1 + R) * num_frames x InputDim]
 * matrix of those chunks, bit for bit; the rows of the output are the
 * examples in order, and kcnn_nnet_backprop_xent / _backprop / _backprop_
 * component follow as after kcnn_nnet_propagate.  The chunks are gathered on
 * the device from {r, s, e - 1} triples staged by the host:
 *   component 0 a SpliceComponent: its output is gathered straight from the
 *     corpus and the chunk matrix is never stored.  kcnn_nnet_output(n, -1) is
 *     the corpus.  The Splice's Backprop is then not run (it has no
 *     parameters, and its input derivative would be a chunk matrix of rows
 *     that examples share): kcnn_nnet_input_deriv(n, 0) is an error until the
 *     next kcnn_nnet_propagate.
 *   any other component 0: the same kernel lays the chunk matrix out in a
 *     contiguous matrix of the network's, kcnn_nnet_output(n, -1), and
 *     everything runs on it as after kcnn_nnet_propagate.
 * Every check (no frames, an index outside the corpus, corpus columns other
 * than InputDim, (L + 1 + R) * num_frames or any activation reaching 2^31 rows
 * or elements) is made before anything is launched; a violation is an error
 * that runs no kernel and changes nothing.  Does not synchronise. */
int kcnn_nnet_propagate_frames(kcnn_nnet *n, const kcnn_corpus *corpus, const int32_t *frames,
                               int num_frames);
/* kcnn_nnet_compute_prob on such a minibatch: the labels' rows are 0 ..
 * num_frames - 1, row n being example frames[n].  Same checks, then those of
 * the labels; the state kcnn_nnet_compute_prob leaves. */
int kcnn_nnet_compute_prob_frames(kcnn_nnet *n, const kcnn_corpus *corpus,
                                  const int32_t *frames, int num_frames, const int32_t *rows,
                                  const int32_t *cols, const float *weights, int num);
/* kcnn_nnet_propagate_frames with the leading Splice -> {Convolution | Maxpool
 * | ReLU}... components (kcnn_nnet_time_train_prefix of them) run as TIME MAPS,
 * once per time step of each RUN of the list: a maximal stretch of entries
 * with frames[i + 1] == frames[i] + 1 in one utterance.  Any list is legal (any
 * order, repeats, runs of one frame) and output row n stays example frames[n].
 * A run of k frames is a segment of k + L + R level-0 rows, corpus rows clamp(r0
 * - L + j, s, e - 1); the maps, their levels and kcnn_nnet_time_map are those
 * of kcnn_nnet_compute_shared, and kcnn_nnet_output below prefix - 1 is an
 * error.  The values are kcnn_nnet_propagate_frames' to the error bar of the
 * GEMMs, not the bits.  kcnn_nnet_backprop / _backprop_xent then run the
 * components from the prefix upwards as always and the prefix once, over the
 * maps: the adjoint of the gather, the pool and ReLU backward on a map, and per
 * Convolution the weight, bias and data gradients as per-tap GEMMs on
 * row-shifted views, each Convolution stepping by kcnn_component_apply_gradient's rule
 * with num_sample = num_frames.  The prefix's RectifiedLinearComponents
 * accumulate no <ValueSum> / <DerivSum> / <Count> in such a step.  Until the
 * next forward call kcnn_nnet_backprop_component, _backprop_split and
 * _input_deriv of a prefix component are errors that change nothing.  The
 * checks of kcnn_nnet_propagate_frames, then the maps' (every map below 2^31
 * rows and elements), precede every launch.  With a training prefix of 0 the
 * call is kcnn_nnet_propagate_frames itself. */
int kcnn_nnet_propagate_frames_shared(kcnn_nnet *n, const kcnn_corpus *corpus,
                                      const int32_t *frames, int num_frames);
/* The leading components kcnn_nnet_propagate_frames_shared runs as time maps as
 * the literal path now stands: kcnn_nnet_time_shared_prefix, or 0 when a level
 * of that prefix keeps a height (convolutions along frequency do not train
 * this way). */
int kcnn_nnet_time_train_prefix(const kcnn_nnet *n);
/* After kcnn_nnet_propagate_frames_shared and a backward pass, until the next
 * forward call: the derivative map of `level`, as kcnn_nnet_time_map gives the
 * map (rows that no window reads are 0).  Level 0, and a Maxpool's own level
 * when a ReLU follows it, have none: an error.  For tests and debugging. */
int kcnn_nnet_time_map_deriv(const kcnn_nnet *n, int level, const float **data, MatrixDim *dim,
                             int *channels, int *positions, int *dilation);
/* The flat gradient ([KernelDim x Group] then Group biases, kcnn_component_compute_gradient's
 * layout) that backward applied to Convolution i of the prefix: *num floats on
 * the DEVICE. */
int kcnn_nnet_time_gradient(const kcnn_nnet *n, int i, const float **data, int *num);

/* ---- streaming forward pass over concurrent utterances -------------------- */
/* Upstream NnetOnlineComputer(nnet, pad_input = true), the decodable of
 * online2-wav-nnet2-latgen-faster --online=true, for num_streams >= 1
 * concurrent utterances ("slots") batched into one pass per step; each step
 * gives a slot at most max_chunk >= 1 new frames.  priors / num_priors /
 * prior_scale / apply_log are kcnn_nnet_compute's, fixed for the computer's
 * life and checked as there (priors finite and > 0, OutputDim of them, only
 * with apply_log).  The handle BORROWS n, which must outlive it.  With L and R
 * the contexts of kcnn_nnet_left_context / _right_context, each slot owns two
 * device buffers of L + R + max_chunk rows of InputDim floats, allocated once,
 * by the first accepted step: creating the handle touches no device.  NULL on
 * error (no net, num_streams < 1, max_chunk < 1, bad priors, an arena of 2^31
 * rows or elements), the message in kcnn_last_error(). */
typedef struct kcnn_online kcnn_online;
kcnn_online *kcnn_online_new(kcnn_nnet *n, int num_streams, int max_chunk, const float *priors,
                             int num_priors, float prior_scale, int apply_log);
/* kcnn_online_new with share_time != 0: a step whose network kcnn_nnet_compute_
 * shared's plan accepts (kcnn_online_shared_prefix > 0) runs the leading Splice
 * -> {Convolution | Maxpool | ReLU}... components once per time step instead of
 * once per emitted frame's window.  Each slot that emits k frames gives a
 * segment of k + L + R rows of the frames it holds (clamped at the utterance's
 * ends); the packed segments are a small unpadded whole-utterance input, every
 * Convolution level of it one launch (fp32 products on the bf16 matrix cores
 * with bias and ReLU in the store), the pools, ReLUs and the gather those of
 * kcnn_nnet_compute_shared; the components above the prefix run as without
 * share_time.  To the error bar of the products, not the bits, the same
 * values.  The level maps are the computer's own, allocated once by the first
 * accepted step for the most rows a step can have, num_streams x (max_chunk +
 * L + 2 R); nothing is carried from step to step beyond what kcnn_online_new
 * keeps, and a step takes either route whatever the last one took.  A step of
 * a network the plan declines is kcnn_online_new's, bit for bit.  After a
 * time-shared step kcnn_nnet_output below prefix - 1 is an error.
 * share_time = 0: kcnn_online_new. */
kcnn_online *kcnn_online_new_shared(kcnn_nnet *n, int num_streams, int max_chunk,
                                    const float *priors, int num_priors, float prior_scale,
                                    int apply_log, int share_time);
/* The number of leading components the next step would run as time maps: the
 * network's kcnn_nnet_time_shared_prefix as the literal path now stands for a
 * computer made with share_time, else 0.  -1 on error.  Touches no device. */
int kcnn_online_shared_prefix(const kcnn_online *o);
void kcnn_online_free(kcnn_online *o);
/* One step.  For i < num (HOST arrays), slot streams[i] -- each slot named at
 * most once -- gets num_new[i] frames, 0 <= num_new[i] <= max_chunk: the next
 * rows of `chunk`, the DEVICE matrix [sum of num_new x InputDim] (any row
 * stride; NULL allowed for no rows).  final[i] != 0 ends the slot's utterance
 * with these frames; num_new[i] == 0 is allowed only then (a pure flush).  A
 * slot that has seen `seen` frames and emitted `emitted` rows has, after the
 * step, ready = seen if final, else max(0, seen - R), and contributes the rows
 * of frames [emitted, ready): frame t is what the network gives for the input
 * frames clamp(t + o, 0, T - 1), o = -L .. R, of the eventual utterance of T
 * frames, as kcnn_nnet_compute(pad_input) gives it.  final then frees the
 * slot for a new utterance (a final step on a slot that saw nothing emits
 * nothing).  Slots not named keep their state.  num_out[i] (HOST, written) is
 * the number of rows slot streams[i] contributes; *data / *out_dim is the
 * borrowed device view [sum of num_out x OutputDim] of those rows, slots in the
 * step's order, frames ascending, valid until the next forward call of the net
 * (this one included): P, or with apply_log log(max(P, 1e-20)) - prior_scale *
 * log(priors[col]) as kcnn_nnet_compute forms it.  A step that emits nothing
 * gives [0 x OutputDim], *data NULL, and runs no network kernel.
 * One kernel moves each named slot's history and new frames into the slot's
 * other buffer (nothing is copied through the host or in place); the forward
 * pass is kcnn_nnet_propagate_frames' with that arena as its corpus and, for
 * each emitted frame, a host-made triple as its example, then kcnn_nnet_
 * compute's epilogue.  The net's activations hold nothing of a stream: its
 * other forward calls between steps disturb none.  A DropoutComponent draws
 * its mask: use the test model.  Leaves the net in the state kcnn_nnet_compute
 * leaves.  Every check -- a slot out of range or named twice, num_new outside
 * [0, max_chunk], num_new == 0 without final, chunk rows other than the sum of
 * num_new, chunk columns other than InputDim, a stride below the columns, any
 * activation reaching 2^31 rows or elements -- is made before anything is
 * launched and before any slot changes; a violation is an error that runs
 * nothing.  Does not synchronise and reads nothing back. */
int kcnn_online_accept(kcnn_online *o, const float *chunk, MatrixDim dim, const int32_t *streams,
                       const int32_t *num_new, const int32_t *final, int num, int32_t *num_out,
                       const float **data, MatrixDim *out_dim);
/* Abandons the slot's utterance: the slot is free, nothing is emitted. */
int kcnn_online_reset(kcnn_online *o, int stream);
/* out[0] = the frames the slot's utterance has seen, out[1] = the rows it has
 * emitted (both 0 for a free slot). */
int kcnn_online_frames(const kcnn_online *o, int stream, int64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif /* KCNN_KCNN_H_ */
