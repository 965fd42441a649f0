// capi/time-plan.h -- host-side plan of NnetStack::ComputeShared (nnet-stack.h;
// kcnn_nnet_compute_shared): which leading components of a stack run as TIME
// MAPS, one row per time step of the concatenated (padded) utterances instead
// of one row per frame holding the frame's whole window, and the row
// bookkeeping of such a pass.  Pure host code with no GPU call: a pass whose
// rows do not fit is refused here, before any launch, so it can never become
// an out-of-range device access.  Header-only so that a stand-alone program
// can run it under a host sanitizer (scripts/time_plan_check.cc).
//
// time_schedule turns a plan and its rows into the ordered launches of one
// pass; NnetStack::RunTimeSchedule runs them.  Two callers, two routes:
//   kUtteranceRoute, ComputeShared: a 1-D Convolution level is kw GEMMs of the
//     matrix layer on row-shifted views and every level is formed (TimeMap
//     exposes them).  At tens of thousands of rows the GEMM's tiles and
//     operand statistics pay (profiles/compute_shared.md).
//   kStreamRoute, an OnlineComputer's share_time step: such a level is one
//     kn_timemap_conv, and a ReLU on any Convolution goes into its store, the
//     convolution's own level never formed.  At about a thousand rows a launch
//     and its latency are the cost (profiles/online_compute_shared.md).
// Everything else -- the height-map kernels, the weight rows of a tap, a pool
// with the ReLU on it, the gather -- is the same and decided here, where
// scripts/time_schedule_check.cc checks it without a GPU.
//
// A level is the output of one component of the prefix, described by (C, n,
// delta): channels, positions per window, dilation.  The window-layout row of
// result frame t of utterance u has element (position k, channel c) at column
// k + c n, and that element is map[base_u + t + delta k][c]; base_u, the
// utterance's first row in the (padded) input, is the same at every level: the
// maps keep the input's row numbering.
//   level 0, the Splice output: the map is the (clamped) feature matrix, rows
//     of `width` = input-dim floats; n = L + R + 1, delta = 1 (C = 1)
//   Convolution, kw taps: n' = n - kw + 1, delta' = delta;
//     map'[s][g] = b[g] + sum_d map[s + delta d][:] . W_d[:][g]
//   Maxpool 1 x pw x pc: n' = n / pw, delta' = delta pw, C' = C / pc;
//     map'[s][oc] folds map[s + delta w][oc pc + c] over c (outer), w (inner)
//   ReLU: element-wise
// Level l reads `reach` = delta (taps - 1) rows past its own row, so with M
// rows of input the first M - (sum of the reaches up to l) rows of level l are
// computed, in one piece over all utterances.  The rows whose taps cross from
// one utterance into the next are computed and never read: utterance u's
// windows read its rows [base_u, base_u + F_u + delta (n - 1)) only (F_u its
// result frames), and delta (n - 1) never grows from level to level.
//
// With height maps (make_time_plan's third parameter; NnetStack::TimeSharedPlan
// sets it) a level is (C, H, n, delta): a map row keeps a frequency axis of H
// floats a channel, `width` = H C floats with element (h, c) at column h + c
// H; the window-layout element (h, k, c) is at column h + k H + c H n
// (conv-geom.h: h + w H + c H W) and is map[base_u + t + delta k][h + c H].
// Level 0 is (1, input-dim, L + R + 1, 1); with H = 1 everything is as above.
//   Convolution kh x kw on (C, H, n, delta), stride 1, no padding: (G, H - kh
//     + 1, n - kw + 1, delta);
//     map'[s][oh + g OH] = b[g] + sum_{d, c, i} map[s + delta d][oh + i + c H]
//                                               W[i + d kh + c kh kw][g]
//   Maxpool ph x pw x pc, not overlapping: (C / pc, H / ph, n / pw, delta pw);
//     map'[s][oh + oc H'] folds map[s + delta w][oh ph + h + (oc pc + c) H]
//     over c (outer), w, h (inner)
#ifndef KCNN_CAPI_TIME_PLAN_H_
#define KCNN_CAPI_TIME_PLAN_H_

#include <stdint.h>

#include <sstream>
#include <string>
#include <vector>

#include "frame-index.h"  // check_frames_matrix: the limits of a training pass

namespace kcnn {

constexpr int64_t kTimeRowLimit = (int64_t)1 << 31;  // rows of a matrix
// positions per window the gather stages for one channel (its LDS tile)
constexpr int kTimeMaxPositions = 8192;
// filters of a height-map Convolution (kn_timemap_conv2d: 32 a block on grid y)
constexpr int kTimeMaxGroup2d = 65535 * 32;
// (row, height) pairs of one height map: a 32-bit index in the kernels
constexpr int64_t kTimeMaxRowHeights = ((int64_t)1 << 31) - 1;

// What the plan reads of a component (NnetStack fills it from the component).
struct TimeComp {
  enum Kind { kOther, kSplice, kConv, kPool, kRelu };
  Kind kind = kOther;
  int input_dim = 0, output_dim = 0;
  // -Context().front(), Context().back(); every component has them
  int left = 0, right = 0;
  // Splice
  bool contiguous = true;  // the context is left .. right without gaps
  int const_dim = 0;
  // Convolution and Maxpool
  int in_height = 0, in_width = 0, in_channel = 0;
  // Convolution
  int kernel_height = 0, kernel_width = 0, stride = 1, pad_height = 0, pad_width = 0;
  int group = 0, out_height = 0, out_width = 0;
  // Maxpool
  int pool_height = 0, pool_width = 0, pool_channel = 0;
  bool overlap = false;
};

struct TimeLevel {
  TimeComp::Kind kind;
  int channels, positions, dilation;  // (C, n, delta) of this level's map
  int width;                          // floats a map row holds: H C, input-dim at level 0
  int taps;                           // kw of a Convolution, pw of a Maxpool, else 1
  int pool_channel;                   // pc of a Maxpool, else 1
  int reach;                          // rows past its own that a row reads below: delta_in (taps - 1)
  int sum_reach;                      // the reaches of levels 1 .. this one
  int height = 1;                     // H: the frequency axis of a map row (height maps)
  int pool_height = 1;                // ph of a Maxpool, else 1
};

struct TimePlan {
  // levels[l] is the output of component l; empty when the plan declines
  std::vector<TimeLevel> levels;
  std::string declined;  // why, when it does
  int prefix() const { return (int)levels.size(); }
};

// height_maps: levels may keep a height (frequency) axis; without it a plan
// covers 1-D convolutions along time only, as before height maps existed.
inline TimePlan make_time_plan(const std::vector<TimeComp> &comps, bool literal_path,
                               bool height_maps = false) {
  TimePlan plan;
  std::ostringstream why;
  auto decline = [&]() {
    plan.levels.clear();
    plan.declined = why.str();
    return plan;
  };
  if (literal_path) {
    why << "the literal path is on";
    return decline();
  }
  if (comps.empty() || comps[0].kind != TimeComp::kSplice) {
    why << "component 0 is not a SpliceComponent";
    return decline();
  }
  const TimeComp &sp = comps[0];
  if (!sp.contiguous || sp.const_dim != 0) {
    why << "component 0 has a gapped context or a const-component-dim";
    return decline();
  }
  if (sp.left < 0 || sp.right < 0 || sp.input_dim < 1 ||
      (int64_t)sp.left + sp.right + 1 > kTimeMaxPositions) {
    why << "component 0 has a context of " << sp.left << " + " << sp.right << " frames";
    return decline();
  }
  for (size_t i = 1; i < comps.size(); i++)
    if (comps[i].left != 0 || comps[i].right != 0) {
      why << "component " << i << " has a context of its own";
      return decline();
    }
  TimeLevel cur;
  cur.kind = TimeComp::kSplice;
  cur.channels = 1;
  cur.positions = sp.left + sp.right + 1;
  cur.dilation = 1;
  cur.width = sp.input_dim;
  cur.taps = cur.pool_channel = 1;
  cur.reach = cur.sum_reach = 0;
  cur.height = sp.input_dim;
  plan.levels.push_back(cur);
  bool conv_seen = false;
  for (size_t i = 1; i < comps.size(); i++) {
    const TimeComp &c = comps[i];
    const TimeLevel in = plan.levels.back();
    TimeLevel out = in;
    out.kind = c.kind;
    out.taps = out.pool_channel = out.pool_height = 1;
    if (c.kind == TimeComp::kConv && height_maps) {
      if (c.pad_height != 0 || c.pad_width != 0) {
        why << "Convolution " << i << " has in-pad-height or in-pad-width set";
        return decline();
      }
      if (c.in_channel != in.channels || c.in_height != in.height ||
          c.in_width != in.positions || c.stride != 1 || c.kernel_height < 1 ||
          c.kernel_height > c.in_height || c.kernel_width < 1 || c.kernel_width > c.in_width ||
          c.out_height != c.in_height - c.kernel_height + 1 ||
          c.out_width != c.in_width - c.kernel_width + 1 || c.group < 1) {
        why << "Convolution " << i << " is not an unpadded stride-1 convolution of its input ("
            << in.channels << " channels, height " << in.height << ", " << in.positions
            << " positions)";
        return decline();
      }
      if (c.group > kTimeMaxGroup2d || (int64_t)c.group * c.out_height >= kTimeRowLimit) {
        why << "Convolution " << i << " has " << c.group << " filters of height " << c.out_height;
        return decline();
      }
      out.channels = c.group;
      out.height = c.out_height;
      out.width = c.group * c.out_height;
      out.positions = c.out_width;
      out.taps = c.kernel_width;
      conv_seen = true;
    } else if (c.kind == TimeComp::kPool && height_maps) {
      if (!conv_seen) break;  // (a pool of the Splice output itself: no prefix)
      if (c.overlap || c.pool_height < 1 || c.pool_width < 1 || c.pool_channel < 1 ||
          c.in_height != in.height || c.in_width != in.positions ||
          c.in_channel != in.channels || c.in_height % c.pool_height != 0 ||
          c.in_width % c.pool_width != 0 || c.in_channel % c.pool_channel != 0) {
        why << "Maxpool " << i << " is overlapping or does not divide its input ("
            << in.channels << " channels, height " << in.height << ", " << in.positions
            << " positions) evenly";
        return decline();
      }
      out.channels = in.channels / c.pool_channel;
      out.height = in.height / c.pool_height;
      out.width = out.channels * out.height;
      out.positions = in.positions / c.pool_width;
      out.dilation = in.dilation * c.pool_width;
      out.taps = c.pool_width;
      out.pool_channel = c.pool_channel;
      out.pool_height = c.pool_height;
    } else if (c.kind == TimeComp::kConv) {
      const bool first = in.kind == TimeComp::kSplice;
      // directly on the Splice a filter spans the whole frame; above, one row
      const int height = first ? in.width : 1, chans = first ? 1 : in.channels;
      if (c.in_channel != chans || c.in_height != height || c.kernel_height != c.in_height ||
          c.pad_height != 0 || c.pad_width != 0 || c.in_width != in.positions ||
          c.stride != 1 || c.kernel_width < 1 || c.kernel_width > c.in_width ||
          c.out_height != 1 || c.out_width != c.in_width - c.kernel_width + 1 || c.group < 1) {
        why << "Convolution " << i << " is not a 1-D convolution along time of its input ("
            << chans << " channels, height " << height << ", " << in.positions << " positions)";
        return decline();
      }
      out.channels = out.width = c.group;
      out.height = 1;
      out.positions = c.out_width;
      out.taps = c.kernel_width;
      conv_seen = true;
    } else if (c.kind == TimeComp::kPool) {
      if (!conv_seen) break;  // (a pool of the Splice output itself: no prefix)
      if (c.overlap || c.pool_height != 1 || c.in_height != 1 || c.pool_width < 1 ||
          c.pool_channel < 1 || c.in_width != in.positions || c.in_channel != in.channels ||
          c.in_width % c.pool_width != 0 || c.in_channel % c.pool_channel != 0) {
        why << "Maxpool " << i << " is overlapping, pools over height or does not divide its "
            << "input (" << in.channels << " channels, " << in.positions << " positions) evenly";
        return decline();
      }
      out.channels = out.width = in.channels / c.pool_channel;
      out.positions = in.positions / c.pool_width;
      out.dilation = in.dilation * c.pool_width;
      out.taps = c.pool_width;
      out.pool_channel = c.pool_channel;
    } else if (c.kind == TimeComp::kRelu) {
      if (!conv_seen) break;
      // (the stack checks dimensions)
      if ((int64_t)c.input_dim != (int64_t)in.channels * in.height * in.positions) break;
    } else {
      break;
    }
    out.reach = in.dilation * (out.taps - 1);
    out.sum_reach = in.sum_reach + out.reach;
    plan.levels.push_back(out);
  }
  if (!conv_seen) {
    why << "no Convolution follows component 0";
    return decline();
  }
  return plan;
}

// Whether level l (> 0) of a plan runs on the height-map kernels
// (kn_timemap_conv2d, kn_timemap_pool2d): its input keeps a height, and it is
// not the Splice's full-frame convolution, which contracts a whole map row a
// tap as a 1-D level does.  A ReLU is element-wise on H C columns either way.
inline bool time_level_2d(const TimePlan &plan, int l) {
  const TimeLevel &lev = plan.levels[(size_t)l], &below = plan.levels[(size_t)l - 1];
  if (lev.kind == TimeComp::kConv)
    return below.kind == TimeComp::kSplice ? lev.height > 1 : below.height > 1;
  return lev.kind == TimeComp::kPool && below.height > 1;
}

// The rows of one pass: utterance u has len[u] input frames and, with L + R =
// context, gives F_u = len[u] (pad_input: it is laid out clamped, len[u] +
// context rows) or len[u] - context result rows.
struct TimeRows {
  int64_t input_rows = 0;              // M: the rows of the level-0 map
  int64_t result_rows = 0;             // the sum of F_u
  std::vector<int64_t> base, frames;   // base_u, F_u
  std::vector<int64_t> computed;       // per level: its first `computed` rows are
};

// "" and *rows, or what is wrong: lengths the pass cannot take, 2^31 rows, a
// tap or a window that would read past the rows computed below it.
inline std::string plan_time_rows(const TimePlan &plan, const int32_t *lengths, int num_utts,
                                  bool pad_input, TimeRows *rows) {
  std::ostringstream err;
  if (plan.levels.empty()) return "no plan";
  if (lengths == nullptr || num_utts < 1) return "no utterances";
  const int64_t context = plan.levels[0].positions - 1;
  TimeRows r;
  for (int u = 0; u < num_utts; u++) {
    const int64_t f = pad_input ? lengths[u] : lengths[u] - context;
    if (f < 1) {
      err << "utterance " << u << " has " << lengths[u] << " frames; at least "
          << (pad_input ? 1 : context + 1) << " are needed";
      return err.str();
    }
    r.base.push_back(r.input_rows);
    r.frames.push_back(f);
    r.input_rows += f + context;
    r.result_rows += f;
    if (r.input_rows >= kTimeRowLimit) return "too many rows";
  }
  for (size_t l = 0; l < plan.levels.size(); l++) {
    const TimeLevel &lev = plan.levels[l];
    const int64_t computed = r.input_rows - lev.sum_reach;
    // the highest row of the level below that this level's last row reads
    if (l > 0 && computed - 1 + lev.reach > r.computed[l - 1] - 1) {
      err << "level " << l << " reads past the " << r.computed[l - 1] << " rows below it";
      return err.str();
    }
    // every window of every utterance lies in the computed rows
    const int64_t span = (int64_t)lev.dilation * (lev.positions - 1);
    if (computed < 1 || span > context ||
        r.base.back() + r.frames.back() - 1 + span > computed - 1) {
      err << "level " << l << " computes " << computed << " rows, fewer than its windows read";
      return err.str();
    }
    // (level 0 is indexed by rows alone)
    if (l > 0 && computed * lev.height > kTimeMaxRowHeights) {
      err << "level " << l << " has " << computed << " rows of height " << lev.height
          << ": too many";
      return err.str();
    }
    r.computed.push_back(computed);
  }
  *rows = r;
  return "";
}

// Which launches a caller's pass is made of (the header of this file).
struct TimeRoute {
  bool conv_kernel;     // a 1-D Convolution level is one kn_timemap_conv, not per-tap GEMMs
  bool fuse_conv_relu;  // a ReLU on a Convolution goes into the convolution's store
};
constexpr TimeRoute kUtteranceRoute = {false, false}, kStreamRoute = {true, true};

// One launch of a pass.  An argument the op's kernel does not take is 0.
struct TimeLaunch {
  enum Op { kConvTaps, kConv, kConv2d, kPool2d, kEpilogue, kGather, kGather2d };
  Op op;
  int comp;                  // the component whose level this is (a conv: whose W and bias)
  int in_level, in_rows;     // reads the first in_rows rows of that level
  // the map written (a pool's, a convolution's own) and the ReLU'd map written
  // with it or instead of it; -1: none (both for the gather)
  int out_level, act_level;
  int rows;                  // rows computed; the gather: result rows
  int height, channels, kernel_height;  // kConv2d: (H, C) below and kh; kPool2d, kGather2d: H
  int taps, dilation;                   // kw or pw, and the dilation of the map read
  int wc, wd;                           // kConvTaps, kConv: weight row c wc + d wd
  int relu;                             // the convolutions: the ReLU in the store
  int pool_height, pool_channel;
  int positions, context;               // the gathers
};

// The launches of one pass over `plan` in order, the gather last; `rows` is
// plan_time_rows' for it.  An empty plan gives none.
inline std::vector<TimeLaunch> time_schedule(const TimePlan &plan, const TimeRows &rows,
                                             TimeRoute route) {
  std::vector<TimeLaunch> out;
  const int p = plan.prefix();
  if (p == 0) return out;
  out.reserve((size_t)p);
  for (int l = 1; l < p; l++) {
    const TimeLevel &lev = plan.levels[(size_t)l], &below = plan.levels[(size_t)l - 1];
    const bool conv = lev.kind == TimeComp::kConv, pool = lev.kind == TimeComp::kPool;
    // The launch forms level l + 1 too: a pool and the ReLU on it from one read,
    // or a convolution with the ReLU in its store, its own level never formed.
    const bool with_relu = l + 1 < p && plan.levels[(size_t)l + 1].kind == TimeComp::kRelu &&
                           (pool || (conv && route.fuse_conv_relu));
    TimeLaunch t = {TimeLaunch::kEpilogue, l, l - 1, (int)rows.computed[(size_t)l - 1], l, -1,
                    (int)rows.computed[(size_t)l]};
    t.taps = lev.taps;  // (a lone ReLU: taps = pool_channel = 1)
    t.dilation = below.dilation;
    if (with_relu || !(conv || pool)) t.act_level = with_relu ? l + 1 : l;
    if (!pool && t.act_level >= 0) t.out_level = -1;
    if (conv && time_level_2d(plan, l)) {
      // a filter shorter than its input is high, or a level with a height below
      t.op = TimeLaunch::kConv2d;
      t.height = below.height;
      t.channels = below.channels;
      t.kernel_height = below.height - lev.height + 1;
    } else if (conv) {
      // weight row i + d kh + c kh kw: a whole frame's block a tap on the Splice
      // (c = 0, kh = the frame), every kw-th row from d above (kh = 1)
      const bool on_splice = below.kind == TimeComp::kSplice;
      t.op = route.conv_kernel ? TimeLaunch::kConv : TimeLaunch::kConvTaps;
      t.wc = on_splice ? 1 : lev.taps;
      t.wd = on_splice ? below.width : 1;
    } else if (pool && time_level_2d(plan, l)) {
      t.op = TimeLaunch::kPool2d;
      t.height = below.height;
      t.pool_height = lev.pool_height;
    }
    if (conv) t.relu = with_relu;
    else t.pool_channel = lev.pool_channel;
    out.push_back(t);
    l += with_relu;
  }
  const TimeLevel &top = plan.levels[(size_t)p - 1];
  TimeLaunch g = {top.height > 1 ? TimeLaunch::kGather2d : TimeLaunch::kGather, p - 1, p - 1,
                  (int)rows.computed[(size_t)p - 1], -1, -1, (int)rows.result_rows};
  g.height = top.height > 1 ? top.height : 0;
  g.dilation = top.dilation;
  g.positions = top.positions;
  g.context = plan.levels[0].positions - 1;
  out.push_back(g);
  return out;
}

// The rows of level `l` that utterance u's windows read: [first, first + num).
inline void time_valid_rows(const TimePlan &plan, const TimeRows &rows, int l, int u,
                            int64_t *first, int64_t *num) {
  const TimeLevel &lev = plan.levels[(size_t)l];
  *first = rows.base[(size_t)u];
  *num = rows.frames[(size_t)u] + (int64_t)lev.dilation * (lev.positions - 1);
}

// ---- training on runs of consecutive corpus rows -------------------------------
// NnetStack::PropagateFramesShared (kcnn_nnet_propagate_frames_shared) runs the
// prefix of a TRAINING step as time maps.  A run (r0, k) of the frame list
// (frame-index.h, frame_runs) in utterance rows [s, e) is one SEGMENT: its
// level-0 rows are corpus rows clamp(r0 - L + j, s, e - 1), j < k + L + R, and
// its k result rows start at the sum of the earlier runs' lengths.  These are
// plan_time_rows' rows of num_runs unpadded "utterances" of k + L + R frames;
// the forward is time_schedule under kUtteranceRoute, which forms every level,
// and the backward time_backward_schedule below.

// The plan of a training step: `plan` itself (make_time_plan's), declined when
// any of its levels runs on the height-map kernels, which have no backward.
inline TimePlan time_train_plan(TimePlan plan) {
  for (int l = 1; l < plan.prefix(); l++)
    if (time_level_2d(plan, l)) {
      std::ostringstream why;
      why << "level " << l << " keeps a height; training covers 1-D levels only";
      plan.levels.clear();
      plan.declined = why.str();
      break;
    }
  return plan;
}

// The rows of a training pass over runs of run_lengths[j] = k_j frames: "" and
// *rows, or what is wrong.  Beyond plan_time_rows' limits, every map, every
// derivative map and the window-layout output stay below 2^31 rows and elements.
inline std::string plan_train_rows(const TimePlan &plan, const int32_t *run_lengths,
                                   int num_runs, TimeRows *rows) {
  if (plan.levels.empty()) return "no plan";
  if (run_lengths == nullptr || num_runs < 1) return "no runs";
  const int64_t context = plan.levels[0].positions - 1;
  std::vector<int32_t> lengths((size_t)num_runs);
  for (int j = 0; j < num_runs; j++) {
    if (run_lengths[j] < 1 || run_lengths[j] + context >= kTimeRowLimit) return "too many rows";
    lengths[(size_t)j] = (int32_t)(run_lengths[j] + context);
  }
  TimeRows r;
  std::string bad = plan_time_rows(plan, lengths.data(), num_runs, false, &r);
  for (size_t l = 0; bad.empty() && l < plan.levels.size(); l++)
    bad = check_frames_matrix("a time map", r.computed[l], plan.levels[l].width);
  const TimeLevel &top = plan.levels.back();
  if (bad.empty())
    bad = check_frames_matrix("the window-layout output", r.result_rows,
                              (int64_t)top.width * top.positions);
  if (bad.empty()) *rows = r;
  return bad;
}

// One launch of the backward pass over time maps.  Levels name forward maps
// (`in`, `pooled`, `act`) and derivative maps (`dout` read, `din` written whole);
// -1: none.
struct TimeBackLaunch {
  enum Op { kScatter, kEpilogueBwd, kConvBwd };
  Op op;
  int comp;                // the component (a conv: whose W is read and updated)
  int dout_level;          // kScatter: -1, it reads d(Output(prefix - 1))
  int rows;                // rows of dout; kScatter: result rows
  int din_level, in_rows;  // -1: the convolution directly above level 0 has no data gradient
  int in_level;            // the forward map below: a pool's or a convolution's input
  int pooled_level, act_level;  // kEpilogueBwd: the pool's own output, the ReLU'd map
  int taps, dilation;      // kw or pw, and the dilation of the map below
  int pool_channel;
  int wc, wd;              // kConvBwd: gradient row c wc + d wd
  int positions, context;  // kScatter
};

// The launches of the backward pass in order, top level first: the scatter
// (the gather's adjoint), then per forward launch, reversed, a pool and/or ReLU
// backward or a convolution backward.  `plan` is a training plan.
inline std::vector<TimeBackLaunch> time_backward_schedule(const TimePlan &plan,
                                                          const TimeRows &rows) {
  std::vector<TimeBackLaunch> out;
  const std::vector<TimeLaunch> fwd = time_schedule(plan, rows, kUtteranceRoute);
  for (size_t i = fwd.size(); i-- > 0;) {
    const TimeLaunch &t = fwd[i];
    TimeBackLaunch b = {TimeBackLaunch::kScatter, t.comp, -1, t.rows, t.in_level, t.in_rows,
                        t.in_level, -1, -1, t.taps, t.dilation, 0, 0, 0, 0, 0};
    if (t.op == TimeLaunch::kGather) {
      b.in_level = -1;
      b.taps = 0;
      b.positions = t.positions;
      b.context = t.context;
    } else if (t.op == TimeLaunch::kEpilogue) {
      b.op = TimeBackLaunch::kEpilogueBwd;
      b.dout_level = t.act_level >= 0 ? t.act_level : t.out_level;
      b.pooled_level = t.out_level;
      b.act_level = t.act_level;
      b.pool_channel = t.pool_channel;
    } else {  // kConvTaps: a training plan has no other convolution
      b.op = TimeBackLaunch::kConvBwd;
      b.dout_level = t.out_level;
      if (t.in_level == 0) b.din_level = -1;
      b.wc = t.wc;
      b.wd = t.wd;
    }
    out.push_back(b);
  }
  return out;
}

}  // namespace kcnn

#endif  // KCNN_CAPI_TIME_PLAN_H_
