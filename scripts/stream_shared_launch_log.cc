// scripts/stream_shared_launch_log.cc -- what the two launchers of the
// time-shared streaming step would launch, without a GPU (nnet2_launch_log.cc's
// counterpart for kn_timemap_conv and kn_stream_segments; the interposed
// hipLaunchKernel and friends are launch_log.h's).  Loads the libkcnn.so given
// as argv[1] and reads cases from standard input, one per line, each a list of
// integers separated by blanks: the launcher's number, then its arguments.  An
// operand is four integers, "rows cols stride lead": its MatrixDim and the
// floats between a 4096-byte aligned address and its base (lead -1: a NULL
// pointer).  Operands are fake device pointers, never dereferenced.
//
//    0 kn_timemap_conv     in w out bias_null rows kernel_width delta wc wd relu
//    1 kn_stream_segments  arena map desc_null num_segs
//
// Prints per case "case <k>", its launches and " rc <return code>":
//   g++ -O1 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude \
//       -Ikaldi-cnn_amd/src/nnet2 scripts/stream_shared_launch_log.cc \
//       -o stream_shared_launch_log -rdynamic -ldl
//   ./stream_shared_launch_log kaldi-cnn_amd/libkcnn.so < cases.txt > new.raw
//   python scripts/conv_launch_names.py --short kaldi-cnn_amd/libkcnn.so new.raw
// (tests/test_stream_shared_routes.py pins its own case table this way).
#include <string.h>

#include <vector>

#include "nnet-kernels.h"
#include "launch_log.h"

namespace {

struct Args {
  std::vector<long> v;
  size_t at = 0;
  bool bad = false;
  int next() {
    if (at >= v.size()) { bad = true; return 0; }
    return (int)v[at++];
  }
};

struct Op {
  float *p;
  MatrixDim d;
};

// the k-th operand of a case: its own 4 GiB of fake address space
Op operand(Args &a, int k) {
  Op o;
  o.d.rows = a.next();
  o.d.cols = a.next();
  o.d.stride = a.next();
  const int lead = a.next();
  o.p = lead < 0 ? nullptr : (float *)(0x100000000ull * (uintptr_t)(k + 1)) + lead;
  return o;
}

}  // namespace

int main(int argc, char **argv) {
  setvbuf(stdout, nullptr, _IONBF, 0);
  if (argc != 2) {
    fprintf(stderr, "usage: %s libkcnn.so < cases\n", argv[0]);
    return 2;
  }
  open_lib(argv[1]);
  auto conv = sym<decltype(&kn_timemap_conv)>("kn_timemap_conv");
  auto segments = sym<decltype(&kn_stream_segments)>("kn_stream_segments");
  float *BIAS = (float *)0xd80000000ull;
  int *DESC = (int *)0xd00000000ull;

  char line[4096];
  int k = 0;
  while (fgets(line, sizeof line, stdin)) {
    Args a;
    for (char *p = line, *e;; p = e) {
      const long x = strtol(p, &e, 10);
      if (e == p) break;
      a.v.push_back(x);
    }
    if (a.v.empty()) continue;
    printf("case %d\n", k++);
    const int which = a.next();
    int rc = -1;
    if (which == 0) {
      Op in = operand(a, 0), w = operand(a, 1), out = operand(a, 2);
      const int bias_null = a.next(), rows = a.next(), kw = a.next(), delta = a.next();
      const int wc = a.next(), wd = a.next(), relu = a.next();
      if (!a.bad)
        rc = conv(in.p, in.d, w.p, w.d, bias_null ? nullptr : BIAS, out.p, out.d, rows, kw, delta,
                  wc, wd, relu, nullptr);
    } else if (which == 1) {
      Op arena = operand(a, 0), map = operand(a, 1);
      const int desc_null = a.next(), num = a.next();
      if (!a.bad)
        rc = segments(arena.p, arena.d, map.p, map.d, desc_null ? nullptr : DESC, num, nullptr);
    } else {
      a.bad = true;
    }
    if (a.bad || a.at != a.v.size()) {
      fprintf(stderr, "bad case %d: %s", k - 1, line);
      return 2;
    }
    printf(" rc %d\n", rc);
  }
  return 0;
}
