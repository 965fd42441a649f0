// capi/stream-state.h -- host-side bookkeeping of kcnn::OnlineComputer
// (online-computer.h; kcnn_online_*): the per-slot state of num_streams
// concurrent utterances fed a few frames at a time, every check of a step, and
// what a checked step puts on the device: the per-slot copy descriptors of
// kn_stream_assemble and the {row, first row, last row} triple of every frame
// the step emits (the examples of kn_splice_frames_prop, nnet2/nnet-kernels.h),
// the arena being the `feats` they index.  Pure host code with no GPU call: a
// bad step is refused here, before any launch and before any state changes, so
// it can never become an out-of-range device access.  Header-only so that a
// stand-alone program can run it under a host sanitizer
// (scripts/stream_state_check.cc).
//
// The arena: each slot owns two buffers of cap = L + R + max_chunk rows; buffer
// b of slot s is arena rows [(2 s + b) cap, (2 s + b + 1) cap).  A slot's
// current buffer holds its frames [base, seen) from the buffer's row 0.  A step
// writes, into the slot's other buffer, the tail it still needs -- frames
// [max(0, emitted - L), seen), at most L + R of them -- and behind it the new
// frames; then the slot flips.  Nothing is copied in place.
//
// A computer made with share_time reads a checked step a second way (Segments):
// as the packed level-0 rows of a small whole-utterance pass over time maps,
// one segment per emitting slot, out of the buffers the step writes
// (kn_stream_segments; scripts/stream_segments_check.cc).  It keeps no state
// of its own.
#ifndef KCNN_CAPI_STREAM_STATE_H_
#define KCNN_CAPI_STREAM_STATE_H_

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <sstream>
#include <string>
#include <vector>

namespace kcnn {

constexpr int64_t kStreamLimit = (int64_t)1 << 31;  // rows and elements of a matrix

// ints of a slot's copy descriptor: {first arena row of the tail, rows of the
// tail, first arena row written, first chunk row of the new frames, their number}
constexpr int kStreamDescInts = 5;

// "" when an arena for these numbers can exist: at least one stream and one
// frame a chunk, contexts >= 0, and 2 x num_streams x (L + R + max_chunk) rows
// of `cols` floats below 2^31 rows and elements.
inline std::string check_stream_geometry(int64_t left, int64_t right, int64_t max_chunk,
                                         int64_t num_streams, int64_t cols) {
  std::ostringstream err;
  if (num_streams < 1) {
    err << "num_streams " << num_streams << "; at least 1 is needed";
  } else if (max_chunk < 1) {
    err << "max_chunk " << max_chunk << "; at least 1 is needed";
  } else if (left < 0 || right < 0 || cols < 1) {
    err << "a context of " << left << " + " << right << " frames of " << cols << " columns";
  } else if (left + right + max_chunk >= kStreamLimit ||
             2 * num_streams >= kStreamLimit / (left + right + max_chunk) ||
             2 * num_streams * (left + right + max_chunk) * cols >= kStreamLimit) {
    err << "an arena of 2 x " << num_streams << " x " << left + right + max_chunk << " rows of "
        << cols << " columns reaches 2^31 rows or elements";
  }
  return err.str();
}

// One step as the caller gives it: slot streams[i] gets num_new[i] frames, rows
// of the chunk in order, and ends its utterance where final[i] != 0.
struct StreamStep {
  const int32_t *streams, *num_new, *final;
  int num;
  int64_t chunk_rows;
};

// What a checked step will do: the rows the assembly writes and the frames
// the step emits, over all its slots.
struct StepTotals {
  int copy_rows = 0, out_rows = 0;
};

// The staged image of a step, all int32: the prefix of the slots' written
// rows (num + 1 entries from 0 to copy_rows, what a block searches), the
// descriptors, the triples.
struct StepLayout {
  size_t row_start, desc, triples, bytes;  // the first three in int32s
};
inline StepLayout step_layout(int num, const StepTotals &t) {
  StepLayout l;
  l.row_start = 0;
  l.desc = (size_t)num + 1;
  l.triples = l.desc + (size_t)kStreamDescInts * (size_t)num;
  l.bytes = sizeof(int32_t) * (l.triples + 3 * (size_t)t.out_rows);
  return l;
}

// ints of a segment's descriptor (kn_stream_segments): {first source arena row,
// which may lie below lo; lo; hi; first map row; rows}
constexpr int kStreamSegmentInts = 5;

// A checked step as a small whole-utterance pass over time maps (time-plan.h):
// each slot that emits k > 0 frames e0 .. e0 + k - 1 gives one segment of k + L
// + R level-0 map rows, row j being the slot's frame clamp(e0 - L + j, 0, its
// newest frame), read from the buffer the step's assembly writes.  The
// segments are packed in the step's order: an unpadded input of `lengths` with
// k_i result rows each, out_start their prefix (num + 1 entries).
struct StepSegments {
  int num = 0;
  int map_rows = 0, out_rows = 0;
  std::vector<int32_t> desc;       // kStreamSegmentInts a segment
  std::vector<int32_t> lengths;    // k_i + L + R
  std::vector<int32_t> out_start;  // 0, k_0, k_0 + k_1, ...
};

class StreamState {
 public:
  // geometry that check_stream_geometry accepted
  StreamState(int left, int right, int max_chunk, int num_streams)
      : left_(left), right_(right), max_chunk_(max_chunk),
        slots_((size_t)num_streams), named_((size_t)num_streams, 0) {}

  int num_streams() const { return (int)slots_.size(); }
  int cap() const { return left_ + right_ + max_chunk_; }
  int arena_rows() const { return 2 * num_streams() * cap(); }

  // "" and *totals, or what is wrong with the step; no slot changes either way.
  std::string Check(const StreamStep &step, StepTotals *totals) {
    std::ostringstream err;
    if (step.num < 0 || (step.num > 0 && (step.streams == nullptr || step.num_new == nullptr ||
                                          step.final == nullptr)))
      return "bad stream arrays";
    if (step.num > num_streams()) {  // (one is then named twice; found before the sums)
      err << step.num << " slots named in a step of " << num_streams() << " streams";
      return err.str();
    }
    const uint32_t mark = ++generation_;
    if (mark == 0) {  // the counter wrapped: every old mark is void
      std::fill(named_.begin(), named_.end(), 0);
      generation_ = 1;
    }
    int64_t sum_new = 0, copy = 0, out = 0;
    for (int i = 0; i < step.num; i++) {
      const int32_t s = step.streams[i], n = step.num_new[i];
      if (s < 0 || s >= num_streams()) {
        err << "entry " << i << ": stream " << s << " outside [0, " << num_streams() << ")";
        return err.str();
      }
      if (named_[s] == generation_) {
        err << "entry " << i << ": stream " << s << " is named twice";
        return err.str();
      }
      named_[s] = generation_;
      if (n < 0 || n > max_chunk_) {
        err << "entry " << i << ": " << n << " new frames outside [0, max_chunk = " << max_chunk_
            << "]";
        return err.str();
      }
      if (n == 0 && !step.final[i]) {
        err << "entry " << i << ": no new frames for stream " << s << " that is not final";
        return err.str();
      }
      const Slot &sl = slots_[s];
      sum_new += n;
      copy += Tail(sl) + n;
      out += Ready(sl.seen + n, step.final[i] != 0) - sl.emitted;
    }
    if (sum_new != step.chunk_rows) {
      err << "the new frames sum to " << sum_new << ", the chunk has " << step.chunk_rows
          << " rows";
      return err.str();
    }
    // (each at most num_streams x cap: below 2^31 by the geometry)
    totals->copy_rows = (int)copy;
    totals->out_rows = (int)out;
    return "";
  }

  // A CHECKED step: fills `image` (step_layout(step.num, totals).bytes) and
  // num_out (step.num entries: the rows each slot emits, in the step's order,
  // frames ascending), and advances the slots.
  void Plan(const StreamStep &step, const StepTotals &totals, void *image, int32_t *num_out) {
    const StepLayout lay = step_layout(step.num, totals);
    int32_t *img = static_cast<int32_t *>(image);
    int32_t *row_start = img + lay.row_start, *desc = img + lay.desc, *tri = img + lay.triples;
    int32_t chunk_row = 0, copy = 0;
    for (int i = 0; i < step.num; i++) {
      Slot &sl = slots_[step.streams[i]];
      const int32_t n = step.num_new[i], tail = Tail(sl);
      const bool final = step.final[i] != 0;
      const int32_t src = BufferRow(step.streams[i], sl.cur) + (int32_t)(sl.seen - tail - sl.base);
      const int32_t dst = BufferRow(step.streams[i], sl.cur ^ 1);
      row_start[i] = copy;
      int32_t *d = desc + (size_t)kStreamDescInts * i;
      d[0] = src;
      d[1] = tail;
      d[2] = dst;
      d[3] = chunk_row;
      d[4] = n;
      chunk_row += n;
      copy += tail + n;
      // the other buffer now holds frames [seen - tail, seen + n)
      sl.base = sl.seen - tail;
      sl.seen += n;
      sl.cur ^= 1;
      const int64_t ready = Ready(sl.seen, final);
      num_out[i] = (int32_t)(ready - sl.emitted);
      const int32_t last = dst + (int32_t)(sl.seen - sl.base) - 1;
      for (int64_t t = sl.emitted; t < ready; t++, tri += 3) {
        tri[0] = dst + (int32_t)(t - sl.base);
        tri[1] = dst;  // frame 0 while it is held; else below every row read
        tri[2] = last;
      }
      sl.emitted = ready;
      if (final) sl = Slot();
    }
    row_start[step.num] = copy;
  }

  // The most map rows a step can need: every slot emitting its most, max_chunk
  // + R frames (a final step of a slot whose last R frames were waiting).
  int64_t max_map_rows() const {
    return (int64_t)num_streams() * ((int64_t)max_chunk_ + left_ + 2 * (int64_t)right_);
  }

  // The segments of a CHECKED step, BEFORE Plan advances the slots (which this
  // does not): what Plan will leave in the arena, read as time-map rows.
  void Segments(const StreamStep &step, StepSegments *segs) const {
    segs->num = segs->map_rows = segs->out_rows = 0;
    segs->desc.clear();
    segs->lengths.clear();
    segs->out_start.assign(1, 0);
    for (int i = 0; i < step.num; i++) {
      const Slot &sl = slots_[step.streams[i]];
      const int32_t n = step.num_new[i];
      const int64_t seen = sl.seen + n;
      const int64_t k = Ready(seen, step.final[i] != 0) - sl.emitted;
      if (k <= 0) continue;
      // Plan writes frames [base, seen) to the slot's other buffer from row 0
      const int64_t base = sl.seen - Tail(sl);
      const int32_t dst = BufferRow(step.streams[i], sl.cur ^ 1);
      const int32_t rows = (int32_t)(k + left_ + right_);
      segs->desc.push_back(dst + (int32_t)(sl.emitted - left_ - base));
      segs->desc.push_back(dst);
      segs->desc.push_back(dst + (int32_t)(seen - base) - 1);
      segs->desc.push_back(segs->map_rows);
      segs->desc.push_back(rows);
      segs->lengths.push_back(rows);
      segs->map_rows += rows;
      segs->out_rows += (int32_t)k;
      segs->out_start.push_back(segs->out_rows);
      segs->num++;
    }
  }

  // Abandons the slot's utterance; false for a slot out of range.
  bool Reset(int stream) {
    if (stream < 0 || stream >= num_streams()) return false;
    slots_[stream] = Slot();
    return true;
  }
  // {frames seen, rows emitted} of the slot's utterance; false out of range.
  bool Frames(int stream, int64_t out[2]) const {
    if (stream < 0 || stream >= num_streams()) return false;
    out[0] = slots_[stream].seen;
    out[1] = slots_[stream].emitted;
    return true;
  }

 private:
  struct Slot {
    int64_t seen = 0, emitted = 0;
    int64_t base = 0;  // the frame in row 0 of the current buffer
    int32_t cur = 0;   // the current buffer, 0 or 1
  };
  // frames computable once `seen` are in: all when the utterance has ended,
  // else those whose right context is in
  int64_t Ready(int64_t seen, bool final) const {
    return final ? seen : std::max<int64_t>(0, seen - right_);
  }
  // the frames a slot holds that frames still to be emitted read: those from
  // emitted - L on; at most L + R, since seen - emitted <= R between steps
  int32_t Tail(const Slot &sl) const {
    return (int32_t)(sl.seen - std::max<int64_t>(0, sl.emitted - left_));
  }
  int32_t BufferRow(int32_t stream, int32_t b) const { return (2 * stream + b) * cap(); }

  int left_, right_, max_chunk_;
  std::vector<Slot> slots_;
  // named_[s] == generation_: the step being checked has named slot s
  std::vector<uint32_t> named_;
  uint32_t generation_ = 0;
};

}  // namespace kcnn

#endif  // KCNN_CAPI_STREAM_STATE_H_
