// nnet2/nnet-kernels.h -- HIP launchers of the upstream nnet2 components on
// either side of the CNN path: RectifiedLinearComponent
// and SpliceComponent.  Internal to libkcnn.so (the components are the
// boundary); plain pointers + MatrixDim + stream like cnsl-hip-kernels.h.
#ifndef KCNN_NNET2_NNET_KERNELS_H_
#define KCNN_NNET2_NNET_KERNELS_H_

#include <stddef.h>
#include <stdint.h>

#include "cnsl-hip-kernels.h"

#ifdef __cplusplus
extern "C" {
#endif

/* RectifiedLinearComponent::Propagate (reference nnet-component.cc:799-806):
 * out = in, then ApplyFloor(0): x < 0 -> 0 (NaN and -0 stay). */
int kn_relu_prop(const float *in, MatrixDim in_dim, float *out, MatrixDim out_dim,
                 kcnn_stream_t st);

/* RectifiedLinearComponent::Backprop (:808-827): in_deriv = Heaviside(out_value)
 * * out_deriv (a product, so 0 * inf = NaN as in the reference).  With stats
 * != NULL also UpdateStats (:337-363): column sums (fp32, fixed order) of
 * out_value and of Heaviside(out_value) added to the fp64 value_sum/deriv_sum.
 * ws: kn_relu_stats_ws(out_dim) bytes. */
size_t kn_relu_stats_ws(MatrixDim dim);
int kn_relu_backprop(const float *out_value, MatrixDim ov_dim, const float *out_deriv,
                     MatrixDim od_dim, float *in_deriv, MatrixDim id_dim,
                     double *value_sum, double *deriv_sum, void *ws, kcnn_stream_t st);

/* SpliceComponent (:2638-2819) for contiguous chunk offsets: out row
 * (chunk, oi) takes, for context slot c, input row chunk*in_cs +
 * (out_first + oi + context[c] - in_first); the const_dim tail copies input
 * row chunk*in_cs + oi.  Backprop is the gather form of the reference's
 * CopyRows/AddMat sequence: in_deriv row r sums, over c in order, the out_deriv
 * block of the output row that read it (0 if none). */
#define KN_SPLICE_MAX_CONTEXT 64
/* Non-contiguous chunk offsets (a gapped context deeper in a stack): table
 * = 1 and in_index[c * out_cs + oi] is the in-chunk input row that splice
 * block c of output row oi reads (ChunkInfo::GetIndex of out offset oi +
 * context[c]); num_splice * out_cs <= KN_SPLICE_MAX_TAB.  table = 0: the
 * contiguous form, in row = out_first + oi + context[c] - in_first. */
#define KN_SPLICE_MAX_TAB 1024
typedef struct {
  int num_chunks, in_cs, out_cs, in_first, out_first;
  int dim, const_dim, num_splice;
  int context[KN_SPLICE_MAX_CONTEXT];
  int table;
  short in_index[KN_SPLICE_MAX_TAB];
} kn_splice_geom;
int kn_splice_prop(const float *in, MatrixDim in_dim, float *out, MatrixDim out_dim,
                   kn_splice_geom geom, kcnn_stream_t st);
int kn_splice_backprop(const float *out_deriv, MatrixDim od_dim, float *in_deriv,
                       MatrixDim id_dim, kn_splice_geom geom, kcnn_stream_t st);

/* SpliceComponent::Propagate on whole utterances of different lengths stacked
 * row-wise, each one chunk (upstream NnetComputer: Nnet::ComputeChunkInfo
 * (num_rows, 1) per utterance).  utt_start (DEVICE, num_utts + 1 ascending
 * entries from 0 to total) holds the row starts of the utterances' final
 * output frames; an activation carries `ext` more rows per utterance, so
 * utterance u has utt_start[u + 1] - utt_start[u] + ext rows from row
 * utt_start[u] + u * ext (in_ext for `in`, out_ext for `out`).  Output row t
 * of utterance u takes, for context slot c, the utterance's input row
 * clamp(t + context[c] + shift, 0, its last row); the const_dim tail copies
 * its input row clamp(t + const_shift, ...).  The clamp repeats the first and
 * the last frame (NnetComputer's pad_input) where shift asks for rows the
 * input does not hold; elsewhere it never acts.  A row's utterance is found
 * by a search over utt_start: their number and lengths are bounded by the
 * matrices alone (fewer than 2^31 rows, fewer than 2^31 elements a matrix). */
typedef struct {
  int num_utts, total;
  int in_ext, out_ext;
  int shift, const_shift;
  int dim, const_dim, num_splice;
  int context[KN_SPLICE_MAX_CONTEXT];
} kn_ragged_splice_geom;
int kn_splice_ragged_prop(const float *in, MatrixDim in_dim, float *out, MatrixDim out_dim,
                          const int *utt_start, kn_ragged_splice_geom geom, kcnn_stream_t st);

/* SpliceComponent::Propagate on a minibatch given as rows of a corpus that
 * stays on the device (whole utterances stacked row-wise in `feats`): the
 * window matrix kn_splice_prop would read is never stored.  examples (DEVICE,
 * 3 * num_examples ints) holds per example n {r, lo, hi}: its corpus row and
 * the first and last row of its utterance.  Output row (n, oi) takes, for
 * context slot c, corpus row clamp(r + out_offset(oi) + context[c], lo, hi),
 * out_offset(oi) being the frame offset of output row oi from the example's
 * own frame: out_first + oi, or out_offset[oi] with table = 1 (a gapped
 * context deeper in the stack; out_cs <= KN_SPLICE_MAX_TAB).  The const_dim
 * tail follows kn_splice_prop's rule, the input chunk's row oi: corpus row
 * clamp(r + const_first + oi, lo, hi), const_first the offset of the input
 * chunk's first frame.  num_splice = 1, context = {0}, out_cs the input chunk
 * lays the window matrix itself out.  Rows are clamped into `feats` at last,
 * so triples that disagree with the matrix still read inside it. */
typedef struct {
  int num_examples, out_cs;
  int dim, const_dim, num_splice;
  int context[KN_SPLICE_MAX_CONTEXT];
  int const_first, out_first;
  int table;
  short out_offset[KN_SPLICE_MAX_TAB];
} kn_frames_splice_geom;
int kn_splice_frames_prop(const float *feats, MatrixDim dim, float *out, MatrixDim out_dim,
                          const int *examples, kn_frames_splice_geom geom, kcnn_stream_t st);

/* One step of the streaming forward pass's history arena (capi/stream-state.h):
 * for each of num_slots slots named by the step, desc (DEVICE, 5 ints a slot)
 * holds {src, tail, dst, chunk_first, num_new}: arena rows [src, src + tail)
 * -- the frames the slot still needs, in its current buffer -- are copied to
 * arena rows [dst, dst + tail), its other buffer, and chunk rows [chunk_first,
 * chunk_first + num_new) behind them.  row_start (DEVICE, num_slots + 1
 * ascending entries from 0 to total_rows) is the prefix of tail + num_new; a
 * written row's slot is found by a search over it.  The host keeps a step's
 * sources and destinations disjoint; nothing is copied in place.  `chunk` is
 * read with its own stride and may be NULL when no slot has new frames.  A
 * row outside its matrix is not copied, so descriptors that disagree with the
 * matrices still stay inside them. */
int kn_stream_assemble(float *arena, MatrixDim arena_dim, const float *chunk, MatrixDim chunk_dim,
                       const int *row_start, const int *desc, int num_slots, int total_rows,
                       kcnn_stream_t st);

/* The level-0 time map of a time-shared streaming step (capi/stream-state.h,
 * StepSegments): desc (DEVICE, 5 ints a segment, first destination rows
 * ascending) holds {src, lo, hi, dst, rows}: map row dst + j, j < rows, is
 * arena row clamp(src + j, lo, hi); src may lie below lo (the frames before an
 * utterance's first repeat it) and src + rows - 1 above hi (those after its
 * last).  Map rows that no segment covers are not written.  A source row is
 * clamped into the arena at last, so descriptors that disagree with the
 * matrices still read inside it; a destination row is a row of `map` by the
 * search.  16-byte lanes where the strides and bases allow. */
int kn_stream_segments(const float *arena, MatrixDim arena_dim, float *map, MatrixDim map_dim,
                       const int *desc, int num_segs, kcnn_stream_t st);

/* fp64 stat vectors of NonlinearComponent (Scale/Add/UpdateStats):
 * y = beta * y + alpha * x  (x may be NULL: y = beta * y). */
int kn_dvec_update(double *y, const double *x, double alpha, double beta, int n,
                   kcnn_stream_t st);

/* ---- nnet-loss-kernels.hip: Softmax, Dropout and the cross-entropy objective ---- */

/* SoftmaxComponent::Propagate (reference nnet-component.cc:930-947): per row
 * y = exp(x - max x) / sum, then ApplyFloor(1e-20) (NaN stays). */
int kn_softmax_prop(const float *in, MatrixDim in_dim, float *out, MatrixDim out_dim,
                    kcnn_stream_t st);

/* SoftmaxComponent::Backprop (:949-1000): D = P o E - diag(rowdot(P, E)) P.
 * With value_sum != NULL also UpdateStats(out_value): the column sums of P
 * (fixed order) added to the fp64 value_sum.  ws: kn_softmax_stats_ws(dim)
 * bytes. */
size_t kn_softmax_stats_ws(MatrixDim dim);
int kn_softmax_backprop(const float *out_value, MatrixDim ov_dim, const float *out_deriv,
                        MatrixDim od_dim, float *in_deriv, MatrixDim id_dim, double *value_sum,
                        void *ws, kcnn_stream_t st);

/* CuMatrix::CompObjfAndDeriv (reference cu-matrix.h:624-637) for num DEVICE
 * elements {row, col, weight} with no repeated (row, col): deriv(row, col) +=
 * weight / probs(row, col); tot[0] += sum weight * log probs(row, col), tot[1]
 * += sum weight (device fp64, reduced in a fixed order).  Elements outside
 * the matrix are skipped.  ws: kn_objf_ws(kn_comp_objf_blocks(num)) bytes. */
size_t kn_objf_ws(int num_blocks);
int kn_comp_objf_blocks(int num);
int kn_comp_objf_and_deriv(const int *el_row, const int *el_col, const float *el_w, int num,
                           const float *probs, MatrixDim p_dim, float *deriv, MatrixDim d_dim,
                           double *tot, void *ws, kcnn_stream_t st);

/* Zeroed derivative + CompObjfAndDeriv + Softmax Backprop in one pass, for a
 * SoftmaxComponent that is the last component.  Labels sorted by row: row r's
 * are lab_col / lab_w [row_start[r], row_start[r + 1]) (device; row_start has
 * rows + 1 entries).  S_r = sum of the row's weights; in_deriv = -P S_r, plus
 * the weight at a label; tot as above; value_sum (nullable) as in
 * kn_softmax_backprop.  objf_ws: kn_objf_ws(kn_softmax_xent_blocks(dim)). */
int kn_softmax_xent_blocks(MatrixDim dim);
int kn_softmax_xent_backprop(const float *out_value, MatrixDim ov_dim, float *in_deriv,
                             MatrixDim id_dim, const int *row_start, const int *lab_col,
                             const float *lab_w, double *value_sum, void *stats_ws, double *tot,
                             void *objf_ws, kcnn_stream_t st);

/* The objective and the frame accuracy of nnet-compute-prob (upstream
 * NnetUpdater::ComputeObjfAndDeriv without the derivative, ComputeTotAccuracy
 * over CuMatrixBase::FindRowMaxId, reference cu-matrix.h:257), forward only.
 * Labels sorted by row as for kn_softmax_xent_backprop (device; all inside the
 * matrix, none repeated).  tot[0] += sum weight * log((double)probs(row, col)),
 * tot[1] += sum weight, tot[2] += sum of the weights of the labels whose
 * column is their row's best column: the lowest column whose value is greater
 * than every earlier column's, starting from -1e21 (a NaN is never the best;
 * a row may have none).  Device fp64, per-block partials reduced in a fixed
 * order.  Each labelled row is read once; nothing but tot and ws is written.
 * ws: kn_prob_ws(kn_prob_blocks(dim)) bytes. */
int kn_prob_blocks(MatrixDim dim);
size_t kn_prob_ws(int num_blocks);
int kn_objf_accuracy(const float *probs, MatrixDim p_dim, const int *row_start,
                     const int *lab_col, const float *lab_w, double *tot, void *ws,
                     kcnn_stream_t st);

/* The same from the logits of a last SoftmaxComponent: each probability is
 * formed in registers by kn_softmax_prop's operation sequence (the bits
 * kn_softmax_prop gives for this input into a 16-byte aligned output with a
 * row stride that is a multiple of 4) and never stored. */
int kn_softmax_objf_accuracy(const float *logits, MatrixDim l_dim, const int *row_start,
                             const int *lab_col, const float *lab_w, double *tot, void *ws,
                             kcnn_stream_t st);

/* The log-likelihoods of upstream nnet-am-compute --apply-log
 * --divide-by-priors (DecodableAmNnet): out(r, c) = (float)(log((double)
 * max(probs(r, c), 1e-20f)) - offset[c]), a NaN staying NaN (ApplyFloor).
 * offset: DEVICE fp64, cols entries (prior_scale * log prior[c], formed on
 * the host), or NULL for none.  One fp64 subtraction, one rounding. */
int kn_loglikes(const float *probs, MatrixDim p_dim, float *out, MatrixDim out_dim,
                const double *offset, kcnn_stream_t st);

/* The same from the logits of a last SoftmaxComponent, each probability formed
 * in registers as kn_softmax_objf_accuracy forms it and never stored: the bits
 * of kn_softmax_prop into an output laid out as `out`, then kn_loglikes. */
int kn_softmax_loglikes(const float *logits, MatrixDim l_dim, float *out, MatrixDim out_dim,
                        const double *offset, kcnn_stream_t st);

/* DropoutComponent::Propagate (:3592-3625).  The uniform draw of element
 * (row, col) is output col % 4 of Philox4x32-10 with key = seed and counter =
 * (col / 4, row_offset + row, call low, call high), u = (x >> 8) * 2^-24;
 * then in fp32 mask = Heaviside(u - dropout_proportion), scaled by
 * high_minus_low unless that is 1, plus low unless that is 0; out = mask * in.
 * row_offset is the matrix's first row in the minibatch the mask belongs to (a
 * data-parallel rank's shard start; 0 for a whole minibatch).  row_offset < 0
 * or row_offset + rows > 2^32 is hipErrorInvalidValue and launches nothing. */
int kn_dropout_prop(const float *in, MatrixDim in_dim, float *out, MatrixDim out_dim,
                    float dropout_proportion, float high_minus_low, float low, uint64_t seed,
                    uint64_t call, int64_t row_offset, kcnn_stream_t st);

/* DropoutComponent::Backprop (:3627-3637), upstream AddMatMatDivMat:
 * in_deriv = in_value == 0 ? out_deriv : out_deriv * out_value / in_value. */
int kn_dropout_backprop(const float *in_value, MatrixDim iv_dim, const float *out_value,
                        MatrixDim ov_dim, const float *out_deriv, MatrixDim od_dim,
                        float *in_deriv, MatrixDim id_dim, kcnn_stream_t st);

/* ---- nnet-normalize-kernels.hip: NormalizeComponent ---- */

/* NormalizeComponent::Propagate (reference nnet-component.cc:580-592): per row
 * p = (1 / cols) * sum x^2, floored at kNormFloor = 2^-66 (NaN stays),
 * out = x * p^-0.5.  A product: a row with an inf entry or whose sum of
 * squares overflows is scaled by 0.  Each element is read and written once
 * for rows of up to 16384 columns; wider rows are read twice. */
int kn_normalize_prop(const float *in, MatrixDim in_dim, float *out, MatrixDim out_dim,
                      kcnn_stream_t st);

/* NormalizeComponent::Backprop (:616-639): with f = p^-0.5 as above,
 * in_deriv = f * out_deriv - (1 / cols) * (rowdot(out_deriv, in_value) * g) *
 * in_value, g = f^3, or 0 where p <= kNormFloor.  in_deriv may be out_deriv
 * (same pointer and stride). */
int kn_normalize_backprop(const float *in_value, MatrixDim iv_dim, const float *out_deriv,
                          MatrixDim od_dim, float *in_deriv, MatrixDim id_dim,
                          kcnn_stream_t st);

/* ---- nnet-timemap-kernels.hip: the time-shared whole-utterance forward ---- */

/* One pass over a time map (capi/time-plan.h): `in` holds one row per time
 * step and one column per channel.  With pooled != NULL, a MaxpoolComponent
 * 1 x pool_width x pool_channel along time at dilation delta: pooled(r, oc) is
 * the reference's fold (start -1e20f, replace when v < x) over c < pool_channel
 * (outer), w < pool_width (inner) of in(r + delta w, oc pool_channel + c), for
 * r < rows; in_dim.rows must hold the last row's highest tap.  With relu !=
 * NULL, RectifiedLinearComponent::Propagate (x < 0 -> 0) of the pooled values,
 * or of `in` itself when pooled == NULL (pool_width = pool_channel = 1), to
 * relu(r, oc).  Both: the pool level and the ReLU level from one read.  16-byte
 * accesses when pool_channel = 1 and every stride, base and the column count
 * allow; scalar otherwise. */
int kn_timemap_epilogue(const float *in, MatrixDim in_dim, float *pooled, MatrixDim p_dim,
                        float *relu, MatrixDim r_dim, int rows, int pool_width, int pool_channel,
                        int delta, kcnn_stream_t st);

/* The window layout of the last time map: out(r, k + c positions) = map(r + u
 * ext + dilation k, c) for result row r of utterance u (utt_start: DEVICE,
 * num_utts + 1 ascending entries from 0 to out_dim.rows, as for
 * kn_splice_ragged_prop; the map holds ext more rows an utterance), k <
 * positions <= KN_TIMEMAP_MAX_POSITIONS, c < map_dim.cols.  The map is read
 * along c and the output written in contiguous runs, staged through LDS.  A
 * source row is clamped into the map, so a table that disagrees with the
 * matrices still reads inside it. */
#define KN_TIMEMAP_MAX_POSITIONS 8192
int kn_timemap_gather(const float *map, MatrixDim map_dim, float *out, MatrixDim out_dim,
                      const int *utt_start, int num_utts, int ext, int positions, int dilation,
                      kcnn_stream_t st);

/* ---- nnet-timemap-conv.hip: a Convolution level of the time maps, one launch ---- */

/* out(s, g) = act(bias[g] + sum_{d < kernel_width} sum_{c < C} in(s + delta d, c)
 * * w(c wc + d wd, g)) for s < rows, g < group: C = in_dim.cols, group =
 * w_dim.cols = out_dim.cols, w the component's LinearParams() read as fp32.
 * (wc, wd) = (1, C) directly on the Splice, where a filter spans the frame;
 * (kernel_width, 1) above it.  act: the identity, or with relu != 0 x < 0 -> 0
 * (NaN and -0 stay).  The products are bf16x6 (x6::mfma6 on the truncating
 * three-way split of both operands, made in the kernel on every call), the
 * accumulation fp32, the bias added in fp32 at the store.  Any rows, C and
 * group >= 1, any strides >= the columns; a base or a stride of `in` that is
 * not 16-byte aligned, or C % 4 != 0, takes 4-byte loads.  Refused with
 * hipErrorInvalidValue before any launch: a highest tap rows - 1 + delta
 * (kernel_width - 1) that is not a row of `in`, a highest weight row (C - 1)
 * wc + (kernel_width - 1) wd that is not one of `w`, out_dim.rows < rows. */
int kn_timemap_conv(const float *in, MatrixDim in_dim, const float *w, MatrixDim w_dim,
                    const float *bias, float *out, MatrixDim out_dim, int rows, int kernel_width,
                    int delta, int wc, int wd, int relu, kcnn_stream_t st);

/* ---- nnet-timemap-2d.hip: time maps that keep a height (frequency) axis ---- */

/* A map row of such a level (capi/time-plan.h, (C, H, n, delta)) holds H C
 * floats, element (h, c) at column h + c H.  The most (row, height) pairs of
 * one map: a 32-bit index in the kernels. */
#define KN_TIMEMAP_MAX_ROW_HEIGHTS 2147483647

/* A Convolution level, kernel_height <= height:
 *   out(s, oh + g OH) = act(bias[g] + sum_{d < kernel_width} sum_{c < channels}
 *       sum_{i < kernel_height} in(s + delta d, oh + i + c height)
 *                               * w(i + d kernel_height + c kernel_height kernel_width, g))
 * for s < rows, oh < OH = height - kernel_height + 1, g < group = w_dim.cols,
 * w the component's LinearParams() read as fp32.  act: the identity, or with
 * relu != 0 x < 0 -> 0 (NaN and -0 stay).  An implicit GEMM, M = (s, oh), N =
 * g, K = (d, c, i): bf16x6 products (x6::mfma6 on the truncating three-way
 * split of both operands, made in the kernel on every call; no statistics
 * pass), fp32 accumulation in a fixed order, the bias added in fp32 at the
 * store.  Any sizes >= 1 and any strides >= the columns, up to
 * KN_TIMEMAP_MAX_ROW_HEIGHTS for rows OH and 65535 * 32 filters.  Refused with
 * hipErrorInvalidValue before any launch: null operands, a highest tap rows -
 * 1 + delta (kernel_width - 1) that is not a row of `in`, a highest weight
 * row kernel_width channels kernel_height - 1 that is not one of `w`,
 * in_dim.cols < height channels, out_dim.cols != OH group, out_dim.rows <
 * rows. */
int kn_timemap_conv2d(const float *in, MatrixDim in_dim, const float *w, MatrixDim w_dim,
                      const float *bias, float *out, MatrixDim out_dim, int rows, int height,
                      int channels, int kernel_height, int kernel_width, int delta, int relu,
                      kcnn_stream_t st);

/* A MaxpoolComponent pool_height x pool_width x pool_channel level, not
 * overlapping, on a map of in_dim.cols = height C columns (pool_height |
 * height, pool_channel | C): with H' = height / pool_height,
 * pooled(s, oh + oc H') is the reference's fold (start -1e20f, replace when v
 * < x) over c < pool_channel (outer), w < pool_width, h < pool_height (inner)
 * of in(s + delta w, oh pool_height + h + (oc pool_channel + c) height), for s
 * < rows; in_dim.rows must hold the last row's highest tap.  With relu !=
 * NULL also RectifiedLinearComponent::Propagate (x < 0 -> 0) of the pooled
 * values to relu(s, .): the pool level and the ReLU level from one read. */
int kn_timemap_pool2d(const float *in, MatrixDim in_dim, float *pooled, MatrixDim p_dim,
                      float *relu, MatrixDim r_dim, int rows, int height, int pool_height,
                      int pool_width, int pool_channel, int delta, kcnn_stream_t st);

/* The window layout of the last time map when it keeps a height: out(r, h + k
 * height + c height positions) = map(r + u ext + dilation k, h + c height)
 * for result row r of utterance u, k < positions, h < height, c <
 * map_dim.cols / height; utt_start, ext and the clamping of a source row into
 * the map as for kn_timemap_gather.  The output is written contiguously, the
 * map read in runs of `height` floats; no limit on positions. */
int kn_timemap_gather2d(const float *map, MatrixDim map_dim, float *out, MatrixDim out_dim,
                        const int *utt_start, int num_utts, int ext, int height, int positions,
                        int dilation, kcnn_stream_t st);

/* ---- nnet-timemap-bwd.hip: a training step over time maps ---- */

/* Level 0 of a training pass over runs of consecutive corpus rows
 * (capi/time-plan.h): map(base_j + i, .) = feats(clamp(r0_j - left + i, lo_j,
 * hi_j), .) for run j < num_runs and every map row, base_j = run_start[j] + j
 * ext.  run_start (DEVICE): the num_runs + 1 ascending starts of the runs'
 * result rows; runs (DEVICE): {r0, first row, last row of its utterance} per
 * run, as kn_splice_frames_prop's triples; ext = L + R >= left.  All
 * map_dim.rows rows are written; a source row is clamped into `feats` at last,
 * so a table that disagrees with the matrices still reads inside them. */
int kn_timemap_layout(const float *feats, MatrixDim dim, float *map, MatrixDim map_dim,
                      const int *run_start, const int *runs, int num_runs, int left, int ext,
                      kcnn_stream_t st);

/* The adjoint of kn_timemap_gather: dmap(s, c) = the sum over k ascending of
 * dy(utt_start[u] + t, k + c positions), t = s - base_u - dilation k, over the
 * k < positions with 0 <= t < F_u, for every s < rows and c < dmap_dim.cols; u
 * is the segment of map row s (base_u = utt_start[u] + u ext, F_u its result
 * rows).  Rows that no window reads get 0.  One writer an element, no atomics.
 * Refused: dy_dim.cols != dmap_dim.cols positions, dmap_dim.rows < rows, a last
 * window that passes row rows - 1. */
int kn_timemap_scatter(const float *dy, MatrixDim dy_dim, float *dmap, MatrixDim dmap_dim,
                       const int *utt_start, int num_utts, int ext, int positions, int dilation,
                       int rows, kcnn_stream_t st);

/* The backward of kn_timemap_epilogue in its three forms.  g(s, oc) = dout(s,
 * oc), or with relu != NULL (the ReLU'd map the forward wrote) relu(s, oc) > 0
 * ? dout(s, oc) : 0, RectifiedLinearComponent::Backprop on the output value.
 * With pooled != NULL (the pool's own output; `in` its input): din(r, ch) = the
 * sum over w ascending of g(r - delta w, ch / pool_channel) over the w <
 * pool_width with 0 <= r - delta w < rows and in(r, ch) == pooled(r - delta w,
 * ch / pool_channel), for every r < rows + delta (pool_width - 1): every tied
 * maximum receives the gradient, a NaN routes nothing.  With pooled == NULL
 * (pool_width = pool_channel = 1; `in` is not read) din = g.  din_dim.cols =
 * do_dim.cols pool_channel. */
int kn_timemap_epilogue_bwd(const float *in, MatrixDim in_dim, const float *pooled,
                            MatrixDim p_dim, const float *relu, MatrixDim r_dim,
                            const float *dout, MatrixDim do_dim, float *din, MatrixDim di_dim,
                            int rows, int pool_width, int pool_channel, int delta,
                            kcnn_stream_t st);

#ifdef __cplusplus
}
#endif
#endif
